"""The single-token mat-vec after its entry was reordered and its row slices moved to the host plan (pm_gemv_fused_plan: GemvJob::rpw / rmul).

A workgroup now derives its rows [floor(N b / grid), floor(N (b + 1) / grid)) from two planned constants per job with a multiply and a multiply-high,
issues the activation loads and job 0's first weight loads on preloaded scalars alone, and only then reads the rest of its argument block. A wrong
slice shows as rows nobody wrote, rows written twice by neighbours with different partial results, or parked results read from the wrong LDS offset -
so every output buffer starts as NaN, and every launch is compared
  * bit for bit with the same product through the stand-alone rms_norm / quantize kernels and the pre-quantized launch
    (tests/test_gpu_ops.py::test_fused_prologue_equals_separate_kernels_bitexact), and
  * with the CPU oracle's mul_mat to rtol = atol = 2e-5 (tests/test_gpu_ops.py::test_fused_qkv_mixed_types_one_launch: identical integer partials,
    float summation order only).
Shapes: K = 256 (one Q4_K / Q6_K block per row), the grid taken from the plan; N = 2 grid (divisible: the multiply-only case of every decode launch),
grid + 1, 3 (fewer rows than workgroups: most slices are empty), 2 grid + 7."""
import ctypes as C

import numpy as np
import pytest

from _bind import Q4_K, Q6_K, rand_blocks

pytestmark = pytest.mark.gpu
RTOL = ATOL = 2e-5


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


def _plan(P, jobs, K, x_mode):
    """pm355_mul_mat_vec_fused_plan on the current device: the 25 values"""
    lib = P.L.load()
    f = lib.pm355_mul_mat_vec_fused_plan
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    out = (C.c_int32 * 25)()
    assert f(C.addressof(jobs), len(jobs), K, x_mode, None, 0, out, 25) == 0
    return list(out)


def _grid(P, t, K):
    jobs = (P.MatvecJob * 1)(P.MatvecJob(t, 0, 64, 4096, None, 4096, None, None))
    return _plan(P, jobs, K, 1)[0]


def _fused_nan(P, ws, x, norm_w=None, eps=0.0, w2s=None, resids=None):
    """pm355_mul_mat_vec_fused into outputs that start as NaN; returns (outputs, the plan's values for this list)"""
    torch = P.torch
    lib = P.L.load()
    lib.pm355_mul_mat_vec_fused.restype = C.c_int
    lib.pm355_mul_mat_vec_fused.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p]
    jobs = (P.MatvecJob * len(ws))()
    ys = [torch.full((w.N,), float("nan"), dtype=torch.float32, device="cuda") for w in ws]
    for j, w in enumerate(ws):
        jobs[j] = P.MatvecJob(w.type, 0, w.N, P.ptr(w.data), P.ptr(w2s[j].data) if w2s else None, P.ptr(ys[j]), None, P.ptr(resids[j]) if resids else None)
    P.check(lib.pm355_mul_mat_vec_fused(C.addressof(jobs), len(ws), ws[0].K, P.ptr(x), P.ptr(norm_w), float(eps), P.stream_ptr()), "mul_mat_vec_fused")
    return ys, _plan(P, jobs, ws[0].K, 2 if norm_w is not None else 1)


def _close(got, want):
    print(f"   max |got - oracle| = {np.abs(got - want).max():.3g} at max |oracle| = {np.abs(want).max():.3g}")
    return np.allclose(got, want, rtol=RTOL, atol=ATOL)


N_KINDS = ["2 grid", "grid + 1", "3", "2 grid + 7"]


def _n_of(kind, g):
    return {"2 grid": 2 * g, "grid + 1": g + 1, "3": 3, "2 grid + 7": 2 * g + 7}[kind]


@pytest.mark.parametrize("norm", [False, True], ids=["f32 row", "rms_norm"])
@pytest.mark.parametrize("kind", N_KINDS)
@pytest.mark.parametrize("t", [Q4_K, Q6_K], ids=["Q4_K", "Q6_K"])
def test_single_job_slices_with_residual(P, oracle, t, kind, norm):
    torch = P.torch
    K = 256
    g = _grid(P, t, K)
    N = _n_of(kind, g)
    rng = np.random.default_rng(1300 + t + N)
    blocks = rand_blocks(t, N, K, rng)
    w = P.upload_weight(t, blocks, K, N)
    x = rng.normal(0, 1.5, (1, K)).astype(np.float32)
    nw = (1 + rng.normal(0, 0.05, K)).astype(np.float32) if norm else None
    resid = rng.normal(0, 1, N).astype(np.float32)
    xd, nwd, rd = _dev(P, x), (_dev(P, nw) if norm else None), _dev(P, resid)
    (got,), pl = _fused_nan(P, [w], xd, norm_w=nwd, eps=1e-5, resids=[rd])
    assert pl[0] == g and pl[19] == N // g and (pl[22] == 0) == (N % g == 0)
    assert pl[18] == (0 if norm else 1)                                  # f32 row + residual: wo / ffn_down's HOT form, whatever N
    assert not bool(torch.isnan(got).any()), "rows no workgroup wrote"
    xn = P.rms_norm(xd, nwd, 1e-5) if norm else xd
    assert torch.equal(got, P.mul_mat_vec(w, x=xn, resid=rd.view(1, -1))[0])
    want = oracle.mul_mat(t, blocks, K, N, oracle.rms_norm(x, nw, 1e-5) if norm else x)[0] + resid
    assert _close(got.cpu().numpy(), want)


@pytest.mark.parametrize("t", [Q4_K, Q6_K], ids=["Q4_K", "Q6_K"])
def test_pair_form_slices(P, oracle, t):
    """ffn_gate | ffn_up at N = 2 grid: y = silu(Wg . xn) * (Wu . xn), the HOT pair form. Oracle bound: both products are within 2e-5 |.| + 2e-5 of the
    oracle's (the bound of a plain job), silu' is at most 1.1 in magnitude and device expf is good to a few ulp, so
    |y - want| <= 1.1 dg |u| + |silu(g)| du + 1e-6 |want| with dg = 2e-5 (|g| + 1), du = 2e-5 (|u| + 1)."""
    torch = P.torch
    K = 256
    g = _grid(P, t, K)
    N = 2 * g
    rng = np.random.default_rng(1400 + t)
    bg, bu = rand_blocks(t, N, K, rng), rand_blocks(t, N, K, rng)
    wg, wu = P.upload_weight(t, bg, K, N), P.upload_weight(t, bu, K, N)
    x = rng.normal(0, 1.5, (1, K)).astype(np.float32)
    nw = (1 + rng.normal(0, 0.05, K)).astype(np.float32)
    xd, nwd = _dev(P, x), _dev(P, nw)
    (got,), pl = _fused_nan(P, [wg], xd, norm_w=nwd, eps=1e-5, w2s=[wu])
    assert pl[0] == g and pl[4] == 1 and pl[18] == 1 and pl[19] == 2 and pl[22] == 0
    assert not bool(torch.isnan(got).any()), "rows no workgroup wrote"
    assert torch.equal(got, P.mul_mat_vec(wg, x=P.rms_norm(xd, nwd, 1e-5), w2=wu)[0])
    xn = oracle.rms_norm(x, nw, 1e-5)
    gate, up = oracle.mul_mat(t, bg, K, N, xn)[0].astype(np.float64), oracle.mul_mat(t, bu, K, N, xn)[0].astype(np.float64)
    silu = gate / (1 + np.exp(-gate))
    want = oracle.silu_mul(gate.astype(np.float32)[None], up.astype(np.float32)[None])[0]
    bound = 1.1 * RTOL * (np.abs(gate) + 1) * np.abs(up) + np.abs(silu) * RTOL * (np.abs(up) + 1) + 1e-6 * np.abs(want)
    err = np.abs(got.cpu().numpy() - want)
    print(f"   max |got - oracle| / bound = {(err / bound).max():.3g}, max |oracle| = {np.abs(want).max():.3g}")
    assert (err <= bound).all()


def _half_f16_ulp(a, b):
    m = np.minimum(np.maximum(np.abs(a), np.abs(b)).astype(np.float16), np.float16(65000))
    return 0.5 * np.spacing(m).astype(np.float32)


@pytest.mark.parametrize("pos", [0, 11])
def test_qkv_epilogue_at_its_smallest_shape(P, oracle, pos):
    """wq | wk | wv with RoPE + KV store at the smallest shape the epilogue serves: head_dim 64, n_head_kv * 64 = 2 grid rows in wk and wv, wq of the same
    size, Q4_K with a Q6_K wv, the token at cache cell `pos` (the engine's position-pointer mode: the HOT form), K = 256.
      * the raw projections (the same list without the epilogue, outputs from NaN) against oracle.mul_mat, rtol = atol = 2e-5;
      * q and the stored K row: the F16 rounding of a value within 4e-6 max|raw| (tests/test_gpu_rope.py: device cos / sin against glibc) of the
        oracle's rotation of the GPU's raw projections; the V column is f16(raw v) bit for bit; nothing else in the caches is written."""
    torch = P.torch
    K, dh, n_ctx = 256, 64, 16
    g = _grid(P, Q4_K, K)
    N = 2 * g
    Hkv = H = N // dh
    rng = np.random.default_rng(1500)
    ts = (Q4_K, Q4_K, Q6_K)
    blocks = [rand_blocks(t, N, K, rng) for t in ts]
    ws = [P.upload_weight(t, b, K, N) for t, b in zip(ts, blocks)]
    assert P.mul_mat_vec_qkv_check(ws, Hkv, dh) == 0
    x = rng.normal(0, 1, (1, K)).astype(np.float32)
    nw = (1 + rng.normal(0, 0.05, K)).astype(np.float32)
    xd, nwd = _dev(P, x), _dev(P, nw)
    raw, _ = _fused_nan(P, ws, xd, norm_w=nwd, eps=1e-5)
    xn = oracle.rms_norm(x, nw, 1e-5)
    for t, bl, y in zip(ts, blocks, raw):
        assert not bool(torch.isnan(y).any())
        assert _close(y.cpu().numpy(), oracle.mul_mat(t, bl, K, N, xn)[0])
    raw = [y.cpu().numpy() for y in raw]
    pd = torch.tensor([pos], dtype=torch.int32, device="cuda")
    tab = P.rope_table(pd, dh, freq_base=500000.0)
    sentinel = 0x5A5A
    kc = torch.full((n_ctx, N), sentinel, dtype=torch.int16, device="cuda")
    vc = torch.full((N, n_ctx), sentinel, dtype=torch.int16, device="cuda")
    q = torch.full((N,), float("nan"), dtype=torch.float32, device="cuda")
    P.mul_mat_vec_qkv(ws, xd, tab, pd, kc, vc, Hkv, dh, n_ctx, norm_w=nwd, eps=1e-5, out=q)
    q_got = q.cpu().numpy()
    assert not np.isnan(q_got).any(), "query rows no workgroup wrote"
    p1 = np.array([pos], dtype=np.int32)
    q_ref = oracle.rope(raw[0].reshape(1, H, dh), p1, mode=0, freq_base=500000.0).reshape(-1)
    k_ref = oracle.rope(raw[1].reshape(1, Hkv, dh), p1, mode=0, freq_base=500000.0).reshape(-1)
    kc_h, vc_h = kc.cpu().numpy().view(np.uint16), vc.cpu().numpy().view(np.uint16)
    assert np.array_equal(q_got, q_got.astype(np.float16).astype(np.float32))
    for name, got, want, src in (("q", q_got, q_ref, raw[0]), ("k", np.ascontiguousarray(kc_h[pos]).view(np.float16).astype(np.float32), k_ref, raw[1])):
        excess = np.abs(got - want) - _half_f16_ulp(got, want) - 4e-6 * np.abs(src).max()
        print(f"   {name}: max excess over half an F16 ulp + 4e-6 max|raw| = {excess.max():.3g}")
        assert excess.max() <= 0, name
    assert np.array_equal(vc_h[:, pos], raw[2].astype(np.float16).view(np.uint16))
    kc_h[pos] = sentinel
    vc_h[:, pos] = sentinel
    assert (kc_h == sentinel).all() and (vc_h == sentinel).all()
