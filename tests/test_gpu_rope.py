"""Every fused RoPE site against the CPU oracle on scaled (linear), YaRN, partial-rotation and far positions.

RoPE is computed in nine places (rope_kv_store_kernel, rope_table_kernel, the mat-vec and small-batch QKV epilogues, attn_rope_body, the flash and
three-launch split forms, two Q8_0-cache forms, pm355_op_rope). Eight of them share rope_cs() but each has its own pair indexing, its own "dims
beyond n_dims pass through" branch and its own cache store. The rows of _rope_cases.ROWS put freq_scale, ext_factor (YaRN, pairs in all three
regimes of the ramp), attn_factor, freq factors and n_dims < head_dim through them, at positions up to 131071: one ulp of deviation in theta
(a non-IEEE division by a freq factor, a contracted multiply-add in the YaRN mix, a running product in another order) is amplified by the
position and hides inside the tolerance at position 37.

Bound of every comparison with the oracle: |got - oracle| <= 4e-6 * ms * max|src| (test_rope_kv_store_vs_oracle's bound scaled by the rotation's
magnitude ms): both sides run the same f32 operation sequence on the same host-computed theta_scale / corr dims; only device cosf / sinf / logf
may differ from glibc, by <= 2 ulp each. The oracle itself is bit-exact against the reference on these rows (tests/test_oracle_vs_ref.py).

Where each site is reached:
  1 rope_kv_store_kernel                 test_rope_kv_store_vs_oracle_params, test_attn_rope_fused_equals_two_kernel_path_params
  2 rope_table_kernel                    test_rope_table_vs_oracle, test_qkv_epilogue_rotation_vs_oracle
  3 mat-vec QKV epilogue (NORM, NEOX)    test_qkv_epilogue_rotation_vs_oracle
  4 small-batch QKV epilogue             tests/test_gpu_engine.py::test_window_prefill_and_decode_with_linear_rope_scaling
  5 attn_rope_body                       test_attn_token_rotation_every_form[fused-*], test_attn_rope_fused_equals_two_kernel_path_params
  6 flash split form                     test_attn_token_rotation_every_form[flash]
  7 three-launch split form              test_attn_token_rotation_every_form[three-launch] (child process under PM355_ATTN_FLASH=0)
  8 Q8_0-cache forms (two sites)         test_attn_token_rotation_every_form[q8_0], [q8_0-long]
  9 pm355_op_rope                        the reference's test-backend-ops (tests/test_gpu_llama_decode.py)
and all of 1 - 8 under a real graph: tests/test_gpu_llama_decode.py::test_llama_decode_plugin_rope_scaling."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from _bind import Q4_K, Q6_K, Q8_0, rand_blocks
from _rope_cases import POSITIONS, ROWS, ROW_IDS, freq_factors, magnitude, rope_kw

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
T = 4
BOUND = 4e-6


@pytest.fixture(scope="module")
def P():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("GPU tests need a HIP device")
    import prima_cpp_amd.ops as ops
    ops.torch = torch
    return ops


def _dev(P, a):
    return None if a is None else P.torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def _bound(row, src_max):
    return BOUND * magnitude(row) * src_max


def _report(what, row, pos, err, src_max):
    """The share of the 4e-6 that the hardware uses (run with -s)."""
    print(f"\n[{what} {row.id} pos {pos}] max |got - oracle| / (ms max|src|) = {err / (magnitude(row) * src_max):.3e}")


def _half_f16_ulp(a, b):
    """Half an F16 ulp at the larger of |a|, |b| (f32 arrays): what rounding an f32 value in that binade to F16 may move it by."""
    m = np.maximum(np.abs(a), np.abs(b)).astype(np.float16)
    m = np.minimum(m, np.float16(65000))
    return 0.5 * np.spacing(m).astype(np.float32)


def _assert_f16_of(stored_bits, want, bound, what):
    """stored (F16 bits) is the F16 rounding of a value within `bound` of the oracle's f32 `want`."""
    got = np.ascontiguousarray(stored_bits).view(np.float16).astype(np.float32)
    excess = np.abs(got - want) - _half_f16_ulp(got, want) - bound
    assert excess.max() <= 0, (what, int(excess.argmax()), float(excess.max()))


# --------------------------------------------------------------------------------------------------------------------------------------------
# site 2: the per-token cos / sin table
# --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pos0", POSITIONS)
@pytest.mark.parametrize("row", ROWS, ids=ROW_IDS)
def test_rope_table_vs_oracle(P, oracle, row, pos0):
    """pm355_rope_table == the oracle's NORM rotation of the vector x[2i] = 1, x[2i + 1] = 0, which is (cos_i ms, sin_i ms); NEOX rows read the
    same table (it is indexed by pair, not by element), so the table of a NEOX row is bit-identical to the one built with mode 0."""
    torch = P.torch
    ff = freq_factors(row)
    kw = rope_kw(row)
    n = row.n_dims
    pos = np.arange(pos0, pos0 + T, dtype=np.int32)
    x = np.zeros((T, 1, n), dtype=np.float32)
    x[:, :, 0::2] = 1.0
    want = oracle.rope(x, pos, freq_factors=ff, **dict(kw, mode=0)).reshape(T, n)
    for t in range(T):
        pd = torch.tensor([int(pos[t])], dtype=torch.int32, device="cuda")
        tab = P.rope_table(pd, row.dh, freq_factors=_dev(P, ff), **kw)
        tab0 = P.rope_table(pd, row.dh, freq_factors=_dev(P, ff), **dict(kw, mode=0))
        assert tab.numel() == n and torch.equal(tab, tab0)
        err = float(np.abs(tab.cpu().numpy() - want[t]).max())
        _report("rope_table", row, int(pos[t]), err, 1.0)
        assert err <= _bound(row, 1.0), (int(pos[t]), err)


# --------------------------------------------------------------------------------------------------------------------------------------------
# site 1: multi-token rope + KV store
# --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pos0", POSITIONS)
@pytest.mark.parametrize("row", ROWS, ids=ROW_IDS)
def test_rope_kv_store_vs_oracle_params(P, oracle, row, pos0):
    """pm355_rope_kv_store on a 131072-cell cache: q_rot / k_rot against the oracle, elements [n_dims, head_dim) of every head bit-identical to the
    input, K cache rows = f16(k_rot) and V cache columns = f16(v) at cells pos0 .. pos0 + 3, both caches zero everywhere else."""
    torch = P.torch
    rng = np.random.default_rng(1000 + pos0)
    H, Hkv, dh, n_ctx = 4, 1, row.dh, 131072
    q = rng.normal(0, 1, (T, H * dh)).astype(np.float32)
    k = rng.normal(0, 1, (T, Hkv * dh)).astype(np.float32)
    v = rng.normal(0, 1, (T, Hkv * dh)).astype(np.float32)
    ff = freq_factors(row)
    kw = rope_kw(row)
    kc = torch.zeros(n_ctx * Hkv * dh, dtype=torch.int16, device="cuda")
    vc = torch.zeros(n_ctx * Hkv * dh, dtype=torch.int16, device="cuda")
    qr, kr = P.rope_kv_store(_dev(P, q), _dev(P, k), _dev(P, v), kc, vc, pos0, H, Hkv, dh, n_ctx, freq_factors=_dev(P, ff), **kw)
    qr, kr = qr.cpu().numpy(), kr.cpu().numpy()
    pos = np.arange(pos0, pos0 + T, dtype=np.int32)
    q_ref = oracle.rope(q.reshape(T, H, dh), pos, freq_factors=ff, **kw).reshape(T, -1)
    k_ref = oracle.rope(k.reshape(T, Hkv, dh), pos, freq_factors=ff, **kw).reshape(T, -1)
    for name, got, want, src in (("q", qr, q_ref, q), ("k", kr, k_ref, k)):
        err = float(np.abs(got - want).max())
        _report(f"rope_kv_store {name}", row, pos0, err, float(np.abs(src).max()))
        assert err <= _bound(row, float(np.abs(src).max())), (name, err)
        g3, s3 = got.reshape(T, -1, dh), src.reshape(T, -1, dh)
        assert np.array_equal(g3[:, :, row.n_dims:].view(np.uint32), s3[:, :, row.n_dims:].view(np.uint32)), name
    kc2, vc2 = kc.view(n_ctx, Hkv * dh), vc.view(Hkv * dh, n_ctx)
    assert np.array_equal(kc2[pos0:pos0 + T].cpu().numpy().view(np.uint16), kr.astype(np.float16).view(np.uint16))
    assert np.array_equal(vc2[:, pos0:pos0 + T].cpu().numpy().view(np.uint16), np.ascontiguousarray(v.T).astype(np.float16).view(np.uint16))
    kc2[pos0:pos0 + T] = 0
    vc2[:, pos0:pos0 + T] = 0
    assert not bool(kc.any()) and not bool(vc.any())


# --------------------------------------------------------------------------------------------------------------------------------------------
# site 3: the epilogue of the wq | wk | wv mat-vec launch
# --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", ROWS, ids=ROW_IDS)
def test_qkv_epilogue_rotation_vs_oracle(P, oracle, row):
    """pm355_mul_mat_vec_qkv with the row's table, n_rot = n_dims and the row's pairing, against the oracle's rotation of the RAW projections, which
    pm355_mul_mat_vec_fused (no epilogue) gives for the same weights: q and the stored K row are the F16 rounding of a value within the bound of
    the oracle's, V is f16(raw v) bit for bit, pass-through elements are f16(raw) bit for bit, nothing else in the caches is written.
    Head counts: every matrix needs N % (2 x CUs) == 0 rows for the epilogue (512 on this chip), so n_head_kv = 512 / head_dim and twice as many
    query heads - the smallest shape the epilogue serves (the check entry point must say so). NEOX with n_dims < head_dim is not served: the check
    says so, the launch is refused and leaves the query row and both caches untouched."""
    torch = P.torch
    K, n_ctx, pos = 1024, 512, 300
    dh = row.dh
    Hkv = 512 // dh
    H = 2 * Hkv
    Nq, Nkv = H * dh, Hkv * dh
    ff = freq_factors(row)
    kw = rope_kw(row)
    neox = row.mode == 2
    pd = torch.tensor([pos], dtype=torch.int32, device="cuda")
    tab = P.rope_table(pd, dh, freq_factors=_dev(P, ff), **kw)
    for tv in (Q4_K, Q6_K):
        rng = np.random.default_rng(300 + tv)
        blocks = [rand_blocks(Q4_K, Nq, K, rng), rand_blocks(Q4_K, Nkv, K, rng), rand_blocks(tv, Nkv, K, rng)]
        ws = [P.upload_weight(Q4_K, blocks[0], K, Nq), P.upload_weight(Q4_K, blocks[1], K, Nkv), P.upload_weight(tv, blocks[2], K, Nkv)]
        xd = _dev(P, rng.normal(0, 1, (1, K)).astype(np.float32))
        sentinel = 0x5A5A
        kc = torch.full((n_ctx, Nkv), sentinel, dtype=torch.int16, device="cuda")
        vc = torch.full((Nkv, n_ctx), sentinel, dtype=torch.int16, device="cuda")
        if neox and row.n_dims < dh:
            assert P.mul_mat_vec_qkv_check(ws, Hkv, dh, n_rot=row.n_dims, neox=True) != 0
            out = torch.full((Nq,), -77.0, dtype=torch.float32, device="cuda")
            with pytest.raises(RuntimeError):
                P.mul_mat_vec_qkv(ws, xd, tab, pd, kc, vc, Hkv, dh, n_ctx, n_rot=row.n_dims, neox=True, out=out)
            torch.cuda.synchronize()
            assert bool((out == -77.0).all()) and bool((kc == sentinel).all()) and bool((vc == sentinel).all())
            continue
        assert P.mul_mat_vec_qkv_check(ws, Hkv, dh, n_rot=row.n_dims, neox=neox) == 0
        raw = [y.cpu().numpy() for y in P.mul_mat_vec_fused(ws, xd)]
        q_got = P.mul_mat_vec_qkv(ws, xd, tab, pd, kc, vc, Hkv, dh, n_ctx, n_rot=row.n_dims, neox=neox).cpu().numpy()
        p1 = np.array([pos], dtype=np.int32)
        q_ref = oracle.rope(raw[0].reshape(1, H, dh), p1, freq_factors=ff, **kw).reshape(-1)
        k_ref = oracle.rope(raw[1].reshape(1, Hkv, dh), p1, freq_factors=ff, **kw).reshape(-1)
        kc_h = kc.cpu().numpy().view(np.uint16)
        vc_h = vc.cpu().numpy().view(np.uint16)
        assert np.array_equal(q_got, q_got.astype(np.float16).astype(np.float32))                  # the query row comes back F16-rounded
        _assert_f16_of(q_got.astype(np.float16).view(np.uint16), q_ref, _bound(row, float(np.abs(raw[0]).max())), "q")
        _assert_f16_of(kc_h[pos], k_ref, _bound(row, float(np.abs(raw[1]).max())), "k")
        assert np.array_equal(vc_h[:, pos], raw[2].astype(np.float16).view(np.uint16))
        f16 = lambda a: a.astype(np.float16).view(np.uint16)
        assert np.array_equal(f16(q_got).reshape(H, dh)[:, row.n_dims:], f16(raw[0]).reshape(H, dh)[:, row.n_dims:])
        assert np.array_equal(kc_h[pos].reshape(Hkv, dh)[:, row.n_dims:], f16(raw[1]).reshape(Hkv, dh)[:, row.n_dims:])
        kc_h[pos] = sentinel
        vc_h[:, pos] = sentinel
        assert (kc_h == sentinel).all() and (vc_h == sentinel).all()


# --------------------------------------------------------------------------------------------------------------------------------------------
# sites 5 - 8: pm355_attn_token in every form
# --------------------------------------------------------------------------------------------------------------------------------------------
FORMS = ["fused-vt", "fused-rowmajor", "flash", "three-launch", "q8_0", "q8_0-long"]
QB = 34                                         # bytes of a Q8_0 block


def _attn_token_form(P, oracle, row, form):
    """One form of pm355_attn_token on one row. The token's cache cell and its RoPE position are separate (d_cell_nkv): cell 5 of 6 attended at
    position 37 and at position 131071 (the context-shifted situation), the split forms also cell 693 of 700 (a span other than the first stores).
      1. the K row written at the cell = the oracle's rotation of raw k: F16 caches within half an F16 ulp + the bound; Q8_0 caches, dequantized,
         within 0.6 d_block + the bound, d_block = amax / 127 of the oracle row's block (half a quantization step, the F16 rounding of d:
         2^-11 x 127 = 0.062 d, slack to 0.6);
      2. the attention output = the same form on inputs the oracle rotated, called with pos = 0, ext_factor = 0, attn_factor = 1 (rope_cs then gives
         exactly (1, 0)): the two runs differ by device vs glibc cos / sin before the F16 / Q8_0 rounding - the attention bound 2e-3 max|want| + 1e-4;
      3. pass-through elements of the stored K row are f16(raw k) bit for bit; in a Q8_0 cache the blocks that hold pass-through elements only
         are quantize_row_q8_0(raw k) bit for bit;
    and the V store is f16(v) / quantize_row_q8_0(v) at the cell, every other cell of both caches keeps its bytes."""
    torch = P.torch
    H, Hkv, n_ctx, dh = 4, 2, 1024, row.dh
    Nkv = Hkv * dh
    q8 = form.startswith("q8_0")
    rowmajor = q8 or form == "fused-rowmajor"
    split = form in ("flash", "three-launch", "q8_0-long")
    flags = (P.ATTN_V_ROWMAJOR if rowmajor else 0) | ((P.ATTN_K_Q8_0 | P.ATTN_V_Q8_0) if q8 else 0)
    ff = freq_factors(row)
    kw = rope_kw(row)
    ident = dict(kw, ext_factor=0.0, attn_factor=1.0)
    scale = 1.0 / np.sqrt(dh)
    runs = [(5, 6, 37), (5, 6, 131071)] + ([(693, 700, 37), (693, 700, 131071)] if split else [])
    for cell, n_kv, pos in runs:
        rng = np.random.default_rng(7000 + 13 * cell + pos % 1000)
        q = rng.normal(0, 1, (1, H * dh)).astype(np.float32)
        k = rng.normal(0, 1, (1, Nkv)).astype(np.float32)
        v = rng.normal(0, 1, (1, Nkv)).astype(np.float32)
        if q8:                                   # native Q8_0 blocks, row-major K and V: [n_ctx][Nkv / 32 blocks]
            K0 = rand_blocks(Q8_0, n_ctx, Nkv, rng, scale=1.28).reshape(n_ctx, Nkv // 32 * QB).copy()
            V0 = rand_blocks(Q8_0, n_ctx, Nkv, rng, scale=1.28).reshape(n_ctx, Nkv // 32 * QB).copy()
            K0[n_kv:] = 0; V0[n_kv:] = 0
        else:
            K0 = rng.normal(0, 1, (n_ctx, Nkv)).astype(np.float16).view(np.uint16)
            V0 = rng.normal(0, 1, (n_ctx, Nkv)).astype(np.float16).view(np.uint16)
            K0[n_kv:] = 0; V0[n_kv:] = 0
            if not rowmajor:
                V0 = np.ascontiguousarray(V0.T)
        p1 = np.array([pos], dtype=np.int32)
        q_rot = oracle.rope(q.reshape(1, H, dh), p1, freq_factors=ff, **kw).reshape(1, -1)
        k_rot = oracle.rope(k.reshape(1, Hkv, dh), p1, freq_factors=ff, **kw).reshape(1, -1)
        dyn = torch.tensor([cell, n_kv], dtype=torch.int32, device="cuda")

        def run(qq, kk, pp, rp):
            up = lambda a: _dev(P, a.view(np.int16) if a.dtype == np.uint16 else a)
            kc, vc = up(K0), up(V0)
            extra = dict(scratch=P.attn_split_scratch(H, dh, n_ctx), max_keys=n_ctx) if split else {}
            out = P.attn_token(_dev(P, qq), _dev(P, kk), _dev(P, v), kc, vc, torch.tensor([pp], dtype=torch.int32, device="cuda"), dyn, H, Hkv, dh, n_ctx,
                               scale, flags=flags, freq_factors=_dev(P, ff), **extra, **rp)
            torch.cuda.synchronize()
            return out.cpu().numpy(), kc.cpu().numpy().view(K0.dtype), vc.cpu().numpy().view(V0.dtype)
        out, kc, vc = run(q, k, pos, kw)
        want, _, _ = run(q_rot, k_rot, 0, ident)
        tag = f"{form} {row.id} cell {cell}/{n_kv} pos {pos}"
        # (2) attention output
        d = float(np.abs(out - want).max())
        print(f"\n[attn_token {tag}] max |d out| {d:.3e}, max |out| {np.abs(want).max():.3e}")
        assert d <= 2e-3 * float(np.abs(want).max()) + 1e-4, (tag, d)
        # (1) + (3) the K row of the cell
        bound = _bound(row, float(np.abs(k).max()))
        passthrough = np.tile(np.arange(dh) >= row.n_dims, Hkv)
        if q8:
            deq = oracle.dequantize_row(Q8_0, kc[cell], Nkv)
            d_block = np.repeat(np.abs(k_rot[0]).reshape(-1, 32).max(axis=1) / 127.0, 32)
            excess = np.abs(deq - k_rot[0]) - 0.6 * d_block - bound
            print(f"[attn_token {tag}] Q8_0 K row: max (|deq - oracle| - bound) / d_block = {float(((np.abs(deq - k_rot[0]) - bound) / d_block).max()):.3f}")
            assert excess.max() <= 0, (tag, int(excess.argmax()), float(excess.max()))
            want_blocks = oracle.quantize_row_q8_0(k[0]).reshape(-1, QB)
            whole = passthrough.reshape(-1, 32).all(axis=1)
            assert np.array_equal(kc[cell].reshape(-1, QB)[whole], want_blocks[whole]), tag
            assert np.array_equal(vc[cell], oracle.quantize_row_q8_0(v[0])), tag
        else:
            _assert_f16_of(kc[cell], k_rot[0], bound, tag)
            assert np.array_equal(kc[cell][passthrough], k[0].astype(np.float16).view(np.uint16)[passthrough]), tag
            v_got = vc[cell] if rowmajor else vc[:, cell]
            assert np.array_equal(v_got, v[0].astype(np.float16).view(np.uint16)), tag
        # the other cells keep their bytes
        kc[cell] = K0[cell]
        if rowmajor:
            vc[cell] = V0[cell]
        else:
            vc[:, cell] = V0[:, cell]
        assert np.array_equal(kc, K0) and np.array_equal(vc, V0), tag


@pytest.fixture(scope="module")
def three_launch_results(tmp_path_factory):
    """PM355_ATTN_FLASH is read once per process: the three-launch split form (attn_split.hip) runs in ONE fresh child process for all rows."""
    out = str(tmp_path_factory.mktemp("three_launch") / "results.json")
    env = dict(os.environ, PM355_ATTN_FLASH="0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, cwd=HERE, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and os.path.exists(out), (r.stdout or "")[-3000:] + (r.stderr or "")[-3000:]
    print(r.stdout)
    with open(out) as f:
        return json.load(f)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("row", ROWS, ids=ROW_IDS)
def test_attn_token_rotation_every_form(P, oracle, request, row, form):
    if form == "three-launch":
        res = request.getfixturevalue("three_launch_results")
        verdict = res.get(row.id, "not run: an earlier row ended the child process")
        assert verdict == "ok", verdict
        return
    _attn_token_form(P, oracle, row, form)


# --------------------------------------------------------------------------------------------------------------------------------------------
# sites 1 + 5: the fused single-token kernel against rope_kv_store + attn_decode
# --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", ROWS, ids=ROW_IDS)
def test_attn_rope_fused_equals_two_kernel_path_params(P, row):
    """tests/test_gpu_ops.py::test_attn_rope_fused_equals_two_kernel_path with the row's parameters: caches bit-identical, outputs within
    2e-6 max(1, |w|) (summation order only)."""
    torch = P.torch
    H, Hkv, n_ctx, dh = 8, 2, 512, row.dh
    ff = freq_factors(row)
    kw = dict(rope_kw(row), freq_factors=_dev(P, ff))
    f16b = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda()
    for n_past in (0, 9, 300):
        rng = np.random.default_rng(44 + n_past)
        K0 = rng.normal(0, 1, (n_ctx, Hkv * dh)).astype(np.float16)
        V0 = rng.normal(0, 1, (Hkv * dh, n_ctx)).astype(np.float16)
        K0[n_past:] = 0; V0[:, n_past:] = 0
        q = rng.normal(0, 1, (1, H * dh)).astype(np.float32)
        k = rng.normal(0, 1, (1, Hkv * dh)).astype(np.float32)
        v = rng.normal(0, 1, (1, Hkv * dh)).astype(np.float32)
        kc1, vc1 = f16b(K0), f16b(V0)
        qr, _ = P.rope_kv_store(_dev(P, q), _dev(P, k), _dev(P, v), kc1, vc1, n_past, H, Hkv, dh, n_ctx, **kw)
        want = P.attn_decode(qr, kc1, vc1, n_past, H, Hkv, dh, n_ctx, 1.0 / np.sqrt(dh))
        kc2, vc2 = f16b(K0), f16b(V0)
        got = P.attn_rope_fused(_dev(P, q), _dev(P, k), _dev(P, v), kc2, vc2, n_past, H, Hkv, dh, n_ctx, 1.0 / np.sqrt(dh), **kw)
        assert torch.equal(kc1, kc2) and torch.equal(vc1, vc2), n_past
        w, g = want.cpu().numpy(), got.cpu().numpy()
        assert np.abs(w - g).max() <= 2e-6 * max(1.0, np.abs(w).max()), n_past


if __name__ == "__main__":
    # the child of three_launch_results: every row in the three-launch form, one verdict per row
    assert os.environ.get("PM355_ATTN_FLASH") == "0"
    import traceback
    import torch
    import prima_cpp_amd.ops as ops
    from _bind import Oracle
    ops.torch = torch
    orc = Oracle()
    verdicts = {}
    for r_ in ROWS:
        try:
            _attn_token_form(ops, orc, r_, "three-launch")
            verdicts[r_.id] = "ok"
        except AssertionError:                   # the verdict carries the traceback to the parent's assertion
            verdicts[r_.id] = traceback.format_exc()[-3000:]
        except Exception:                        # noqa: BLE001 - a launch that failed: nothing more on this device
            verdicts[r_.id] = traceback.format_exc()[-3000:]
            break
    with open(sys.argv[1], "w") as f_:
        json.dump(verdicts, f_)
