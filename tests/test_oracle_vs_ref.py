"""Pins oracle/ggml_oracle.c (the restatement) against the UNMODIFIED reference compiled from
/root/reference into oracle/_ref/ (SURVEY.md §8c). Scalar flavour: bit-for-bit for everything that is integer/byte work or plain IEEE float
arithmetic (quantizers, dequantizers, vec_dot, mul_mat, rms_norm, rope). The exp-based ops
(soft_max, silu) are compared to <= 4 ulp: even the -march=x86-64 build of the reference uses its
SSE2 polynomial ggml_v_expf (ggml.c:2706) for full vectors and libm expf only for tails, while the
oracle restates the documented scalar fallback (libm expf). AVX2 flavour: integer parts bit-for-bit,
float sums within summation-order tolerance."""
import numpy as np
import pytest

from _bind import F16, Q4_K, Q5_K, Q6_K, Q8_0, QUANT_TYPES, TYPE_NAMES, rand_blocks, row_size, tiny_model, vec_dot_type
from _rope_cases import POSITIONS, ROWS, ROW_IDS, freq_factors, rope_kw


def _acts(rng, k, kind):
    if kind == "normal":
        return rng.normal(0, 1, k).astype(np.float32)
    if kind == "cos":      # the reference's own synthetic data, tests/test-quantize-fns.cpp:30-34
        return (0.1 + 2 * np.cos(np.arange(k, dtype=np.float32))).astype(np.float32)
    if kind == "zeros":
        return np.zeros(k, dtype=np.float32)
    if kind == "ties":     # +a and -a both maximal: sign of the first one must win
        x = rng.normal(0, 0.1, k).astype(np.float32)
        x[5::256] = -3.0
        x[9::256] = 3.0
        return x
    if kind == "halfway":  # values that land on .5 after scaling
        x = (np.arange(k) % 255 - 127).astype(np.float32) * 0.5
        return x
    raise ValueError(kind)


def _nmse(a, b):
    """The reference's own backend-comparison metric (tests/test-backend-ops.cpp:176-189)."""
    a = np.asarray(a, dtype=np.float64).ravel()
    b = np.asarray(b, dtype=np.float64).ravel()
    return float(((a - b) ** 2).sum() / max((b ** 2).sum(), 1e-30))


def _ulp_diff(a, b):
    a = np.ascontiguousarray(a, dtype=np.float32).view(np.int32).astype(np.int64)
    b = np.ascontiguousarray(b, dtype=np.float32).view(np.int32).astype(np.int64)
    return int(np.abs(a - b).max())


@pytest.mark.parametrize("kind", ["normal", "cos", "zeros", "ties", "halfway"])
def test_quantize_q8_K_bitexact(oracle, ref_scalar, kind):
    rng = np.random.default_rng(1)
    x = _acts(rng, 2048, kind)
    a, b = oracle.quantize_row_q8_K(x), ref_scalar.quantize_row_q8_K(x)
    a, b = a.reshape(-1, 292), b.reshape(-1, 292)
    if kind == "zeros":   # reference leaves bsums of an all-zero block unwritten
        a, b = a[:, :260], b[:, :260]
    assert np.array_equal(a, b)


@pytest.mark.parametrize("kind", ["normal", "cos", "zeros", "halfway"])
def test_quantize_q8_0_bitexact(oracle, ref_scalar, kind):
    rng = np.random.default_rng(2)
    x = _acts(rng, 1024, kind)
    assert np.array_equal(oracle.quantize_row_q8_0(x), ref_scalar.quantize_row_q8_0(x))


def test_fp16_conversion_exhaustive(oracle, ref_scalar):
    h = np.arange(65536, dtype=np.uint16)
    f_ref = ref_scalar.fp16_to_fp32_row(h)
    f_np = h.view(np.float16).astype(np.float32)
    fin = ~np.isnan(f_np)                                   # NaN payloads are implementation-defined
    assert np.array_equal(np.isnan(f_ref), ~fin)
    assert np.array_equal(f_ref.view(np.uint32)[fin], f_np.view(np.uint32)[fin])
    sel = np.r_[0:65536:97, 0:2048, 0x7bf0:0x7c01, 0xfbf0:0xfc01]
    assert np.array_equal(oracle.f16_to_f32(h[sel]).view(np.uint32), f_ref[sel].view(np.uint32))
    rng = np.random.default_rng(3)
    x = np.concatenate([rng.normal(0, 1, 4000), rng.normal(0, 1e-6, 2000), rng.normal(0, 3e4, 2000),
                        [0.0, -0.0, 65504.0, 65519.9, 65520.0, 1e9, 5.96e-8, 2.98e-8, 2.99e-8, 6.1e-5]]).astype(np.float32)
    mid = (f_np[1000:1200] + f_np[1001:1201]) / 2           # exact ties between neighbouring halfs
    x = np.concatenate([x, mid.astype(np.float32)])
    assert np.array_equal(oracle.f32_to_f16(x), ref_scalar.fp32_to_fp16_row(x))


@pytest.mark.parametrize("t", QUANT_TYPES)
def test_dequantize_bitexact(oracle, ref_scalar, t):
    rng = np.random.default_rng(4)
    k = 1024
    blocks = rand_blocks(t, 3, k, rng)
    for r in range(3):
        b = blocks[r * row_size(t, k):(r + 1) * row_size(t, k)]
        assert np.array_equal(oracle.dequantize_row(t, b, k).view(np.uint32),
                              ref_scalar.dequantize_row(t, b, k).view(np.uint32))


@pytest.mark.parametrize("t", QUANT_TYPES)
@pytest.mark.parametrize("source", ["random_blocks", "quantized"])
def test_vec_dot_bitexact_vs_scalar_ref(oracle, ref_scalar, t, source):
    rng = np.random.default_rng(5)
    k, nrows = 2048, 8
    if source == "random_blocks":
        W = rand_blocks(t, nrows, k, rng)
    else:
        W = ref_scalar.quantize_weights(t, rng.normal(0, 1 / np.sqrt(k), (nrows, k)).astype(np.float32))
    x = rng.normal(0, 1, k).astype(np.float32)
    a = oracle.quantize_act(t, x)
    rs = row_size(t, k)
    for r in range(nrows):
        w = W[r * rs:(r + 1) * rs]
        got, want = oracle.vec_dot(t, k, w, a), ref_scalar.vec_dot(t, k, w, a)
        assert np.float32(got).view(np.uint32) == np.float32(want).view(np.uint32), (TYPE_NAMES[t], r, got, want)


@pytest.mark.parametrize("t", QUANT_TYPES)
def test_vec_dot_close_to_avx2_ref_and_int_partials_consistent(oracle, ref_avx2, t):
    rng = np.random.default_rng(6)
    k, nrows = 4096, 8
    W = rand_blocks(t, nrows, k, rng)
    x = rng.normal(0, 1, k).astype(np.float32)
    a = oracle.quantize_act(t, x)
    assert np.array_equal(a, ref_avx2.quantize_row_q8_K(x) if vec_dot_type(t) != Q8_0 else ref_avx2.quantize_row_q8_0(x))
    rs = row_size(t, k)
    for r in range(nrows):
        w = W[r * rs:(r + 1) * rs]
        got, want = oracle.vec_dot(t, k, w, a), ref_avx2.vec_dot(t, k, w, a)
        # same integer partials, different float summation order
        mag = np.abs(oracle.dequantize_row(t, w, k)) @ np.abs(x)
        assert abs(got - want) <= 2e-6 * mag, (TYPE_NAMES[t], got, want)


@pytest.mark.parametrize("t", QUANT_TYPES + [F16])
def test_mul_mat_vs_ref(oracle, ref_scalar, t):
    rng = np.random.default_rng(7)
    K, N, cols = 512, 24, 3
    if t == F16:
        W = rng.normal(0, 1 / np.sqrt(K), (N, K)).astype(np.float16).view(np.uint8).reshape(-1)
    else:
        W = rand_blocks(t, N, K, rng)
    x = rng.normal(0, 1, (cols, K)).astype(np.float32)
    got, want = oracle.mul_mat(t, W, K, N, x), ref_scalar.mul_mat(t, W, K, N, x, n_threads=2)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_rms_norm_bitexact(oracle, ref_scalar):
    rng = np.random.default_rng(8)
    x = rng.normal(0, 2, (3, 1024)).astype(np.float32)
    w = (1 + rng.normal(0, 0.02, 1024)).astype(np.float32)
    for eps in (1e-5, 1e-6):
        assert np.array_equal(oracle.rms_norm(x, w, eps).view(np.uint32), ref_scalar.rms_norm(x, w, eps).view(np.uint32))
    assert np.array_equal(oracle.rms_norm(x, None, 1e-5).view(np.uint32), ref_scalar.rms_norm(x, None, 1e-5).view(np.uint32))


@pytest.mark.parametrize("mode", [0, 2])
@pytest.mark.parametrize("with_ff", [False, True])
@pytest.mark.parametrize("yarn", [False, True])
def test_rope_bitexact(oracle, ref_scalar, mode, with_ff, yarn):
    rng = np.random.default_rng(9)
    x = rng.normal(0, 1, (5, 6, 128)).astype(np.float32)
    pos = np.array([0, 1, 7, 511, 4095], dtype=np.int32)
    ff = (1 + rng.uniform(0, 7, 64)).astype(np.float32) if with_ff else None
    kw = dict(freq_factors=ff, mode=mode, freq_base=500000.0)
    if yarn:
        kw.update(freq_scale=0.25, ext_factor=1.0, attn_factor=1.1, n_ctx_orig=4096)
    assert np.array_equal(oracle.rope(x, pos, **kw).view(np.uint32), ref_scalar.rope(x, pos, **kw).view(np.uint32))
    # far positions (a one-ulp deviation in theta is amplified by the position) and partial rotation, where tests/test_gpu_rope.py leans on the oracle
    far = np.array([32765, 65536, 131071, 4095, 37], dtype=np.int32)
    for n_dims in (64, 96, 128):
        kw["n_dims"] = n_dims
        assert np.array_equal(oracle.rope(x, far, **kw).view(np.uint32), ref_scalar.rope(x, far, **kw).view(np.uint32)), n_dims


@pytest.mark.parametrize("row", ROWS, ids=ROW_IDS)
def test_rope_bitexact_on_the_gpu_tests_rows(oracle, ref_scalar, row):
    """The parameter rows of tests/test_gpu_rope.py (beta_fast / beta_slow, attn_factor, n_ctx_orig, freq factors, n_dims as there) at its positions:
    the oracle those tests compare every kernel with is the reference bit for bit."""
    rng = np.random.default_rng(12)
    pos = np.concatenate([np.arange(p, p + 4) for p in POSITIONS] + [[65536]]).astype(np.int32)
    x = rng.normal(0, 1, (pos.size, 3, row.dh)).astype(np.float32)
    kw = dict(rope_kw(row), freq_factors=freq_factors(row))
    got, want = oracle.rope(x, pos, **kw), ref_scalar.rope(x, pos, **kw)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(got[:, :, row.n_dims:].view(np.uint32), x[:, :, row.n_dims:].view(np.uint32))


def test_soft_max_bitexact(oracle, ref_scalar):
    rng = np.random.default_rng(10)
    heads, nr, nc = 4, 3, 96
    x = rng.normal(0, 3, (heads, nr, nc)).astype(np.float32)
    mask = np.zeros((nr, nc), dtype=np.float32)
    for r in range(nr):
        mask[r, 40 + r:] = -np.inf
    for mb in (0.0, 8.0):
        got = oracle.soft_max_ext(x, mask, 0.0884, mb)
        want = ref_scalar.soft_max_ext(x, mask, 0.0884, mb)
        assert np.array_equal(got == 0, want == 0)
        assert _ulp_diff(got, want) <= 4
        assert np.allclose(got.sum(-1), 1.0, atol=1e-6)
    assert _ulp_diff(oracle.soft_max_ext(x, None, 1.0), ref_scalar.soft_max_ext(x, None, 1.0)) <= 4


def test_silu_mul_bitexact(oracle, ref_scalar):
    rng = np.random.default_rng(11)
    g = rng.normal(0, 3, 4096).astype(np.float32)
    u = rng.normal(0, 1, 4096).astype(np.float32)
    assert _ulp_diff(oracle.silu_mul(g, u), ref_scalar.silu_mul(g, u)) <= 4


@pytest.mark.parametrize("arch", [0, 1])
def test_model_eval_vs_ref(oracle, ref_scalar, arch):
    """Whole tiny Llama/Qwen2 stack: prefill 5 tokens then 3 single-token decode steps, KV cache included.
    Not bit-exact end to end only because of the exp-based ops (see module docstring)."""
    rng = np.random.default_rng(12 + arch)
    d = tiny_model(rng, arch=arch, rope_freqs=(arch == 0), quantize=ref_scalar.quantize_weights)
    ho, hr = oracle.model_new(d), ref_scalar.model_new(d)
    toks = rng.integers(0, d.n_vocab, 8).astype(np.int32)
    steps = [(toks[:5], 0), (toks[5:6], 5), (toks[6:7], 6), (toks[7:8], 7)]
    for tk, p0 in steps:
        h1, l1 = oracle.model_eval(ho, d, tokens=tk, pos0=p0)
        h2, l2 = ref_scalar.model_eval(hr, d, tokens=tk, pos0=p0, n_threads=2)
        # an ulp-level exp difference can flip an int8/f16 rounding downstream (activations are
        # re-quantized at every mat-mul), so whole-stack parity is statistical: NMSE, like the
        # reference's test_llama (max_nmse_err 2e-3, tests/test-backend-ops.cpp:3000) - but far tighter.
        assert _nmse(h1, h2) < 1e-4, _nmse(h1, h2)
        assert _nmse(l1, l2) < 1e-3, _nmse(l1, l2)
        assert int(np.argmax(l1)) == int(np.argmax(l2))
    for which in (0, 1):      # layer 0's cache is upstream of every exp: bit-exact
        assert np.array_equal(oracle.model_kv(ho, d, 0, which), ref_scalar.model_kv(hr, d, 0, which))
    for il in range(1, d.n_layer):
        for which in (0, 1):
            a = oracle.model_kv(ho, d, il, which).view(np.float16).astype(np.float32)
            b = ref_scalar.model_kv(hr, d, il, which).view(np.float16).astype(np.float32)
            assert _nmse(a, b) < 1e-4
    oracle.model_free(ho)
    ref_scalar.model_free(hr)
