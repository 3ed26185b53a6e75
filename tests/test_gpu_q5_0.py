"""Q5_0 weights on the GPU (run with -m gpu on an MI355X): repack, the single-token mat-vec, 2..8 columns, the small-batch mat-mul, the prompt GEMM,
and whole Qwen2-shaped models with the reference's Q4_K_M fallback (ffn_down Q5_0 / Q8_0) through the plug-in and the engine.

Yardsticks: block_q5_0 (ggml-common.h:165-170: half d | u8 qh[4] | u8 qs[16]), dequantize_row_q5_0 (ggml-quants.c:1563) and ggml_vec_dot_q5_0_q8_0
(ggml-quants.c:4789: per block the exact int32 sum of w * a, times d_w * d_a in f32) restated in numpy from the block bytes; the Q8_0 activation
blocks come from the CPU oracle's quantize_row_q8_0 (bit-exact with the reference, tests/test_oracle_vs_ref.py). Where the reference library is built
the same numbers are also checked against its own ggml_vec_dot_q5_0_q8_0 / dequantize_row_q5_0."""
import os

import numpy as np
import pytest

from _bind import have_ref, llama_driver_path, run_llama_driver

pytestmark = pytest.mark.gpu
Q5_0, Q8_0 = 6, 8


@pytest.fixture(scope="module")
def P():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("GPU tests need a HIP device")
    import prima_cpp_amd.ops as ops
    ops.torch = torch
    return ops


def _dev(P, a):
    return P.torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def _blocks(N, K, seed, scale=None):
    from prima_cpp_amd import gguf as G
    return G.random_valid_blocks(Q5_0, N, K, np.random.default_rng(seed), scale=scale).reshape(N, -1)


def _q5_0_ints(blocks, N, K):
    """-> int8 weights q - 16 [N, nb, 32] and f32 scales [N, nb] (dequantize_row_q5_0's arithmetic)."""
    b = np.ascontiguousarray(blocks).reshape(N, K // 32, 22)
    d = b[..., 0:2].copy().view(np.float16)[..., 0].astype(np.float32)
    qh = b[..., 2:6].copy().view(np.uint32)[..., 0].astype(np.int64)
    qs = b[..., 6:22].astype(np.int64)
    j = np.arange(32)
    nib = np.where(j < 16, qs[..., j % 16] & 0xF, qs[..., j % 16] >> 4)
    q = (nib | (((qh[..., None] >> j) & 1) << 4)) - 16
    return q.astype(np.int64), d


def _q8_0_act(oracle, x):
    """f32 [K] -> (int8 [nb, 32], f32 d [nb]) of quantize_row_q8_0."""
    a = np.ascontiguousarray(oracle.quantize_row_q8_0(x)).reshape(-1, 34)
    return a[:, 2:].view(np.int8).astype(np.int64), a[:, 0:2].copy().view(np.float16)[:, 0].astype(np.float32)


def _ref_matmul(oracle, blocks, K, N, x):
    """ggml_vec_dot_q5_0_q8_0 for every (token, row): the integer block sums, then sumf += (d_w * d_a) * sumi in f32 block order."""
    q, d = _q5_0_ints(blocks, N, K)
    x = np.atleast_2d(x)
    out = np.zeros((x.shape[0], N), dtype=np.float32)
    for t in range(x.shape[0]):
        aq, ad = _q8_0_act(oracle, x[t])
        isum = np.einsum("nbk,bk->nb", q, aq)
        acc = np.zeros(N, dtype=np.float32)
        for b in range(K // 32):
            acc = acc + (d[:, b] * ad[b]).astype(np.float32) * isum[:, b].astype(np.float32)
        out[t] = acc
    return out


@pytest.mark.parametrize("K", [256, 4096, 29568])
def test_q5_0_repack_round_trip_and_layout(P, K):
    """set_tensor -> get_tensor bit-exact; the HBM row is qs[nb][16] | qh[nb][4] | d[nb] with the qh and d streams padded to 16 bytes."""
    import torch
    from prima_cpp_amd import lib as L
    N = 37
    blocks = _blocks(N, K, 10 + K)
    w = P.upload_weight(Q5_0, blocks, K, N)
    assert np.array_equal(P.download_weight(w).reshape(N, -1), blocks)
    nb = K // 32
    r16 = lambda v: (v + 15) // 16 * 16
    stride = L.load().pm355_row_stride(Q5_0, K)
    assert stride == 16 * nb + r16(4 * nb) + r16(2 * nb) and stride % 16 == 0
    hbm = w.data.cpu().numpy().reshape(N, stride)
    b = blocks.reshape(N, nb, 22)
    assert np.array_equal(hbm[:, :16 * nb].reshape(N, nb, 16), b[..., 6:22])
    assert np.array_equal(hbm[:, 16 * nb:20 * nb].reshape(N, nb, 4), b[..., 2:6])
    d0 = 16 * nb + r16(4 * nb)
    assert np.array_equal(hbm[:, d0:d0 + 2 * nb].reshape(N, nb, 2), b[..., 0:2])
    # the staged uploader (the plug-in's set_tensor / the engine's loader) writes the same bytes
    lib = L.load()
    up = lib.pm355_uploader_new(1 << 20, 2)
    try:
        host = np.ascontiguousarray(blocks).reshape(-1)
        dst = torch.zeros_like(w.data)
        assert lib.pm355_upload(up, Q5_0, K, host.ctypes.data, dst.data_ptr(), host.size, 1) == 0
        assert lib.pm355_uploader_sync(up) == 0
        assert torch.equal(dst, w.data)
    finally:
        lib.pm355_uploader_free(up)


@pytest.mark.parametrize("K,N", [(256, 3), (4096, 37), (8192, 64), (29568, 6)])
def test_q5_0_gemv_integer_partials_bitexact_and_float_close(P, oracle, K, N):
    rng = np.random.default_rng(24 + K)
    blocks = _blocks(N, K, K + N)
    x = rng.normal(0, 1, K).astype(np.float32)
    w = P.upload_weight(Q5_0, blocks, K, N)
    assert P.vec_dot_act_type(Q5_0) == Q8_0
    xq = P.quantize_act(_dev(P, x[None]), Q8_0)
    y, ip = P.mul_mat_vec_dbg(w, xq)
    y, ip = y.cpu().numpy(), ip.cpu().numpy().astype(np.int64)
    q, d = _q5_0_ints(blocks, N, K)
    aq, _ = _q8_0_act(oracle, x)
    assert ip.shape == (N, K // 32, 2)
    assert np.array_equal(ip[:, :, 0], np.einsum("nbk,bk->nb", q, aq))          # per block: the reference's exact int32 sum
    assert not ip[:, :, 1].any()
    want = _ref_matmul(oracle, blocks, K, N, x)[0]
    mag = np.abs(q * d[..., None]).reshape(N, K) @ np.abs(x)
    assert (np.abs(y - want) <= 4e-6 * mag + 1e-30).all(), np.abs(y - want).max()
    y1 = P.mul_mat_vec(w, x=_dev(P, x[None])).cpu().numpy()[0]                   # f32 activation quantized in the kernel prologue
    assert (np.abs(y1 - want) <= 4e-6 * mag + 1e-30).all()


@pytest.mark.skipif(not have_ref("scalar"), reason="oracle/_ref/libggml_ref_scalar.so not built")
def test_q5_0_numpy_restatement_matches_the_reference_library(oracle):
    import ctypes as C
    from _bind import Ref
    ref = Ref("scalar")
    K, N = 4096, 5
    rng = np.random.default_rng(5)
    blocks = _blocks(N, K, 77)
    q, d = _q5_0_ints(blocks, N, K)
    deq = ref.fn("dequantize_row_q5_0", None, [C.c_void_p, C.c_void_p, C.c_int64])
    dot = ref.fn("ggml_vec_dot_q5_0_q8_0", None, [C.c_int, C.POINTER(C.c_float), C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int])
    x = rng.normal(0, 1, K).astype(np.float32)
    a = np.ascontiguousarray(ref.quantize_row_q8_0(x))
    want = _ref_matmul(oracle, blocks, K, N, x)[0]
    for r in range(N):
        row = np.ascontiguousarray(blocks[r])
        out = np.empty(K, dtype=np.float32)
        deq(row.ctypes.data, out.ctypes.data, K)
        assert np.array_equal(out, (q[r] * d[r][:, None]).astype(np.float32).reshape(-1))
        s = C.c_float(0)
        dot(K, C.byref(s), 0, row.ctypes.data, 0, a.ctypes.data, 0, 1)
        assert s.value == want[r]


@pytest.mark.parametrize("C", [2, 3, 4, 5, 7, 8])
def test_q5_0_gemv_epilogues_and_columns(P, oracle, C):
    rng = np.random.default_rng(25)
    K, N = 4096, 70
    b1 = _blocks(N, K, 31)
    x = rng.normal(0, 1, (C, K)).astype(np.float32)
    bias = rng.normal(0, 1, N).astype(np.float32)
    resid = rng.normal(0, 1, (C, N)).astype(np.float32)
    w1 = P.upload_weight(Q5_0, b1, K, N)
    want1 = _ref_matmul(oracle, b1, K, N, x)
    tol = dict(rtol=2e-5, atol=2e-5)
    y = P.mul_mat_vec(w1, x=_dev(P, x)).cpu().numpy()
    assert np.allclose(y, want1, **tol)
    y = P.mul_mat_vec(w1, x=_dev(P, x), bias=_dev(P, bias), resid=_dev(P, resid)).cpu().numpy()
    assert np.allclose(y, want1 + bias[None] + resid, **tol)
    xq = P.quantize_act(_dev(P, x), Q8_0)
    y = P.mul_mat_vec(w1, xq=xq, ncols=C, bias=_dev(P, bias), resid=_dev(P, resid)).cpu().numpy()    # 2 / 4 / 8-column launches (mmvq_cols.hip)
    assert np.allclose(y, want1 + bias[None] + resid, **tol)


@pytest.mark.parametrize("T", [2, 3, 8, 9, 16, 17, 32, 33, 64])
def test_q5_0_small_batch_matmul(P, oracle, T):
    """mmq_i8.hip MT<Q5_0>: one 32-k integer matrix instruction per block, Q8_0's tables and passes. K = 29568: 924 blocks, the last step holds 4 of 8."""
    rng = np.random.default_rng(4100 + T)
    for K, N in ((4096, 70), (608, 600), (29568, 40)):
        if K == 608 and T not in (3, 17, 64): continue
        b = _blocks(N, K, 7 * T + K)
        x = rng.normal(0, 1, (T, K)).astype(np.float32)
        bias = rng.normal(0, 1, N).astype(np.float32)
        resid = rng.normal(0, 1, (T, N)).astype(np.float32)
        w = P.upload_weight(Q5_0, b, K, N)
        want = _ref_matmul(oracle, b, K, N, x)
        tol = dict(rtol=2e-5, atol=2e-5 * np.sqrt(K / 4096))
        y = P.mul_mat_small(w, x=_dev(P, x)).cpu().numpy()
        assert np.isfinite(y).all()
        assert np.allclose(y, want, **tol), (K, N, np.abs(y - want).max())
        xq = P.quantize_act(_dev(P, x), Q8_0)
        y2 = P.mul_mat_small(w, xq=xq, n_tokens=T, bias=_dev(P, bias), resid=_dev(P, resid)).cpu().numpy()
        assert np.allclose(y2, want + bias[None] + resid, **tol)
        if T <= 8:
            y1 = P.mul_mat_vec(w, xq=xq, ncols=T).cpu().numpy()
            assert np.allclose(y, y1, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("K,N,T", [(29568, 8192, 80), (29568, 8192, 512), (4096, 1028, 80), (4096, 1028, 512)])
def test_q5_0_prompt_gemm(P, oracle, K, N, T):
    """F16 prompt GEMM (mmq.hip: Q5_0 dequantized exactly in f32 and rounded to F16, F16 activations, f32 accumulation) - the F16 tier of the Q8_0 prompt tests:
    NMSE < 1e-6 against the exact product of the dequantized weights, < 5e-4 against the reference arithmetic (Q8_0 activations). Checked on
    a sample of rows (the whole 29568 x 8192 product in f64 would be 2 GB)."""
    rng = np.random.default_rng(71 + T)
    blocks = _blocks(N, K, 1000 + T, scale=1.0)
    w = P.upload_weight(Q5_0, blocks, K, N)
    x = rng.normal(0, 1, (T, K)).astype(np.float32)
    bias = rng.normal(0, 1, N).astype(np.float32)
    resid = rng.normal(0, 1, (T, N)).astype(np.float32)
    got = P.mul_mat_mfma(w, _dev(P, x), bias=_dev(P, bias), resid=_dev(P, resid)).cpu().numpy()
    assert np.isfinite(got).all()
    rows = np.sort(rng.choice(N, size=min(N, 96), replace=False))
    rows[-1] = N - 1
    q, d = _q5_0_ints(blocks[rows], len(rows), K)
    Wf = (q * d[..., None]).reshape(len(rows), K).astype(np.float64)
    exact = x.astype(np.float64) @ Wf.T + bias[rows] + resid[:, rows]
    g = got[:, rows].astype(np.float64)
    nm_exact = ((g - exact) ** 2).sum() / (exact ** 2).sum()
    assert nm_exact < 1e-6, nm_exact
    tt = np.unique(np.r_[0, rng.choice(T, size=7, replace=False), T - 1])
    ref = _ref_matmul(oracle, blocks[rows], K, len(rows), x[tt]) + bias[rows] + resid[tt][:, rows]
    nm_ref = ((g[tt] - ref) ** 2).sum() / (ref ** 2).sum()
    assert nm_ref < 5e-4, nm_ref


def test_q5_0_embedding_rows_are_refused_not_zeros(P):
    """Q5_0 GET_ROWS (token embeddings) is not served: pm355_get_rows and the engine's token embedding refuse a Q5_0 table with an error
    instead of returning zero rows (a Q4_K_M file whose n_embd is no multiple of 256 has a Q5_0 token_embd under the reference's fallback).
    The plug-in leaves such a GET_ROWS to the CPU backend (supports_op). The same calls still serve Q8_0 tables."""
    import torch
    from prima_cpp_amd import engine as E
    from prima_cpp_amd import lib as L
    K, V = 512, 64
    tok = torch.tensor([3, 0, 63], dtype=torch.int32, device="cuda")
    w = P.upload_weight(Q5_0, _blocks(V, K, 5), K, V)
    with pytest.raises(L.PM355Error, match="get_rows"):
        P.get_rows(w, tok)
    w8 = P.upload_weight(Q8_0, np.zeros(V * L.row_size(Q8_0, K), dtype=np.uint8), K, V)
    assert not P.get_rows(w8, tok).cpu().numpy().any()
    hp = dict(arch=1, n_layer=1, n_embd=K, n_head=8, n_head_kv=2, head_dim=64, n_ff=1408, n_vocab=V, rms_eps=1e-6, rope_freq_base=1000000.0)
    win = E.Window(hp, n_ctx=64)
    try:
        with pytest.raises(L.PM355Error, match="token embedding"):
            win.set_tensor(E.T_TOK_EMBD, -1, Q5_0, _blocks(V, K, 6))
        with pytest.raises(L.PM355Error, match="token embedding"):
            win.fill_tensor(E.T_TOK_EMBD, -1, Q5_0, 1, 1.0)
        win.set_tensor(E.T_FFN_DOWN, 0, Q5_0, _blocks(K, 1408, 7))          # a Q5_0 layer matrix is accepted
    finally:
        win.close()


# ---- whole models: a small Qwen2 shape with n_ff = 128 (mod 256) and the reference's Q4_K_M fallback --------------------------------------------
SHAPE = dict(arch=1, n_layer=4, n_embd=512, n_head=8, n_head_kv=2, n_ff=1408, n_vocab=1024, distinct_layers=4)


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    if llama_driver_path() is None:
        pytest.skip("oracle/_ref/llama-ref-driver-* not built")
    from prima_cpp_amd import gguf as G
    path = str(tmp_path_factory.mktemp("q5_0") / "qwen2_q4km_fallback.gguf")
    G.write_synthetic_model(path, fallback="reference", **SHAPE)
    g = G.GGUFFile(path)
    downs = [g.tensors[f"blk.{il}.ffn_down.weight"][0] for il in range(SHAPE["n_layer"])]
    g.close()
    assert Q5_0 in downs and Q8_0 in downs, downs                   # mixed Q5_0 / Q8_0 ffn_down in one window
    return path


def _check(*a, **k):
    from test_gpu_llama_decode import _check as c
    return c(*a, **k)


@pytest.mark.parametrize("chunk", [None, 8], ids=["prompt40", "chunks8"])
def test_q5_0_model_through_the_plugin(model, chunk):
    """Greedy decode under the reference's llama_decode with the plug-in (a 40-token prompt batch: the F16 prompt GEMM; fed in 8-token chunks: the
    small-batch mat-mul; then single tokens: the fused mat-vec plan and its hipGraph), teacher-forced against the reference's CPU backend."""
    prompt = np.random.default_rng(99).integers(0, SHAPE["n_vocab"], 40)
    n = 10
    tg, lg, st = run_llama_driver(model, prompt, n, ngl=99, n_ctx=128, extra_args=["--keep-out-in-cuda"], chunk=chunk)
    assert "MI355" in st["stderr"]
    _check(f"Qwen2 Q4_K_M fallback (Q5_0 / Q8_0 ffn_down) plug-in {chunk or 'prompt'}", tg, lg, model, prompt, n, 128)


def _engine_greedy(path, prompt, n_gen, n_ctx=128):
    import torch
    import prima_cpp_amd.engine as eng
    s = SHAPE
    hp = dict(arch=1, n_layer=s["n_layer"], n_embd=s["n_embd"], n_head=s["n_head"], n_head_kv=s["n_head_kv"], head_dim=s["n_embd"] // s["n_head"],
              n_ff=s["n_ff"], n_vocab=s["n_vocab"], rms_eps=1e-6, rope_freq_base=1000000.0)
    w = eng.Window(hp, n_ctx=n_ctx)
    w.load_gguf(path)
    w.finalize(max_tokens=max(len(prompt), 1))
    toks, logits = [], []
    _, lg, _ = w.decode(tokens=torch.from_numpy(np.asarray(prompt, dtype=np.int32)).cuda(), pos0=0, want_hidden=False)
    w.set_pos(len(prompt))
    tok_d = torch.empty(1, dtype=torch.int32, device="cuda")
    lg_d = torch.empty(s["n_vocab"], dtype=torch.float32, device="cuda")
    for i in range(n_gen):
        l = lg.cpu().numpy().reshape(-1)[-s["n_vocab"]:]
        t = int(np.argmax(l))
        toks.append(t)
        logits.append(l.copy())
        if i == n_gen - 1:
            break
        tok_d.fill_(t)
        w.step(token=tok_d, logits=lg_d)
        lg = lg_d
    w.close()
    return np.array(toks), np.stack(logits)


@pytest.mark.parametrize("n_prompt", [40, 8])
def test_q5_0_model_on_the_engine(model, n_prompt):
    """The resident engine (Window.load_gguf): a 40-token prompt (F16 prompt GEMMs) or an 8-token one (small-batch path: silu * up quantized straight
    into the Q5_0 / Q8_0 ffn_down tables), then single-token steps through the captured graph - teacher-forced against the reference's CPU backend."""
    prompt = np.random.default_rng(7).integers(0, SHAPE["n_vocab"], n_prompt)
    n = 8
    te, le = _engine_greedy(model, prompt, n)
    _check(f"Qwen2 Q4_K_M fallback engine, {n_prompt}-token prompt", te, le, model, prompt, n, 128)
