"""The row slices of the single-token mat-vec as the host plan hands them to the kernels (pm_gemv_fused_plan, GemvJob::rpw / rmul), without a GPU.

Workgroup b of a launch of `grid` workgroups takes rows [floor(N b / grid), floor(N (b + 1) / grid)) of every job. The kernels used to compute that with
two 64-bit divisions per job by gridDim.x - a hidden kernel argument, fetched by a cold scalar load in front of the first memory instruction of every
workgroup. Now the plan computes rpw = N / grid and rmul = ceil(2^32 (N % grid) / grid) per job, and the kernel computes b * rpw + mulhi32(b, rmul).
pm355_mul_mat_vec_fused_plan reports both behind the 19 values it always wrote. Checked here:
  * the reported pair reproduces floor(N b / grid) for EVERY b in [0, grid] - the launch lists of the Llama-3 70B / 8B and Qwen2.5-72B decode steps, and
    lists whose rows the grid does not divide (N = grid + 1, 3, 2 grid + 7, N < grid, the lm_head on a doubled grid);
  * the multiply-only case (rmul == 0) is exactly the divisible one. Every launch of the Llama layers is multiply-only; Qwen2.5-72B's ffn_gate | ffn_up
    (29568 rows on 256 workgroups) is not, and keeps its HOT kernel form all the same: no form carries a division, so none needs divisibility
    (tests/test_matvec_plan.py pins the HOT forms for N = 33);
  * the multiplier is exact for every (rem, grid) the proof in pm_gemv_fused_plan covers that could matter - all remainders of the grids in use,
    and the worst cases near the bound of 65536 workgroups;
  * a caller that asks for 19 values sees what it saw before, and nothing behind them is written."""
import ctypes as C

import pytest

from test_matvec_plan import J, Q4_K, Q5_0, Q5_K, Q6_K, Q8_0, Qkv, c_jobs, c_store

N_OUT = 25


@pytest.fixture(scope="module")
def lib():
    import prima_cpp_amd
    return prima_cpp_amd.load()


def plan(lib, jobs, K, x_mode, qkv=None, cus=256, n_out=N_OUT, room=N_OUT):
    f = lib.pm355_mul_mat_vec_fused_plan
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    a, out = c_jobs(jobs), (C.c_int32 * room)(*([-12345] * room))
    st = c_store(qkv) if qkv else None
    rc = f(a, len(jobs), K, x_mode, C.addressof(st) if qkv else None, cus, out, n_out)
    return rc, list(out)


def slices_of(v):
    """(grid, first, [(rpw, rmul)] of the three jobs of the block)"""
    return v[0], v[5], [(v[19 + j], v[22 + j] & 0xffffffff) for j in range(3)]


def at(b, rpw, rmul):
    return b * rpw + ((b * rmul) >> 32)


def model_lists(E, H, Hkv, dh, F, V, wv, down, qkv_bias=False, neox=False, base=Q4_K):
    """the launches of one decoded token: wq | wk | wv with the epilogue, wo, ffn_gate | ffn_up, ffn_down (both types of the mixture), lm_head"""
    q = [J(base, H * dh, bias=qkv_bias), J(base, Hkv * dh, bias=qkv_bias), J(wv, Hkv * dh, bias=qkv_bias)]
    lists = [(q, E, 2, Qkv(Hkv, dh, neox=neox)), ([J(base, E, resid=True)], H * dh, 1, None), ([J(base, F, w2=True)], E, 2, None), ([J(Q6_K, V)], E, 2, None)]
    lists += [([J(t, E, resid=True)], F, 1, None) for t in down]
    return lists


LLAMA70 = model_lists(8192, 64, 8, 128, 28672, 128256, Q6_K, (Q4_K, Q6_K)) + model_lists(8192, 64, 8, 128, 28672, 128256, Q5_K, (Q4_K,))
LLAMA8 = model_lists(4096, 32, 8, 128, 14336, 128256, Q6_K, (Q4_K, Q6_K)) + model_lists(4096, 32, 8, 128, 14336, 128256, Q4_K, (Q4_K,))
QWEN72 = (model_lists(8192, 64, 8, 128, 29568, 152064, Q6_K, (Q5_0, Q8_0), qkv_bias=True, neox=True) +
          model_lists(8192, 64, 8, 128, 29568, 152064, Q6_K, (Q8_0,), qkv_bias=True, neox=True, base=Q6_K))


def odd_lists(grid):
    out = []
    for N in (grid + 1, 3, 2 * grid + 7, grid - 1, 1, 2 * grid):
        for t in (Q4_K, Q6_K):
            out.append(([J(t, N, resid=True)], 256, 1, None))              # wo / ffn_down's HOT form
            out.append(([J(t, N)], 256, 2, None))
            out.append(([J(t, N, w2=True)], 256, 2, None))                 # ffn_gate | ffn_up's HOT form
        out.append(([J(Q4_K, N), J(Q4_K, 2 * grid + 7), J(Q6_K, 3)], 256, 1, None))
        out.append(([J(Q6_K, N), J(Q4_K, grid + 1)], 256, 1, None))         # (the Q4_K job goes first: the reported values follow the kernel's order)
    out.append(([J(Q6_K, 128256)], 256, 2, None))                          # lm_heads: 501 / 594 rows per workgroup at 256 - the grid doubles for the second
    out.append(([J(Q6_K, 152064)], 256, 2, None))
    out.append(([J(Q6_K, 300000)], 256, 2, None))
    return out


@pytest.mark.parametrize("cus", [256, 64, 304])
def test_reported_slices_are_the_former_division(lib, cus):
    seen_div, seen_odd, hot_odd = 0, 0, 0
    models = LLAMA70 + LLAMA8 + QWEN72 if cus == 256 else [c for c in LLAMA70 + LLAMA8 + QWEN72 if c[3] is None]
    for jobs, K, x_mode, qkv in models + odd_lists(cus) + odd_lists(2 * cus):
        rc, v = plan(lib, jobs, K, x_mode, qkv, cus)
        assert rc == 0, (rc, jobs, K, x_mode, qkv)
        grid, first, sl = slices_of(v)
        order = list(range(len(jobs)))
        order[0], order[first] = order[first], order[0]                     # the job the kernel pre-issues went to the front
        Ns = [jobs[i]["N"] for i in order] + [0] * (3 - len(jobs))
        for N, (rpw, rmul) in zip(Ns, sl):
            assert rpw == N // grid and (rmul == 0) == (N % grid == 0), (jobs, grid, N, rpw, rmul)
            assert all(at(b, rpw, rmul) == N * b // grid for b in range(grid + 1)), (jobs, grid, N, rpw, rmul)
            seen_div += N > 0 and rmul == 0
            seen_odd += rmul != 0
            hot_odd += rmul != 0 and v[18] != 0
    assert seen_div and seen_odd and hot_odd


def test_llama_decode_launches_are_multiply_only_and_hot(lib):
    """what the 70B / 8B token pays for: every launch of the layer on 256 workgroups is divisible and takes a HOT form; the lm_head is divisible too"""
    for jobs, K, x_mode, qkv in LLAMA70 + LLAMA8:
        rc, v = plan(lib, jobs, K, x_mode, qkv, 256)
        assert rc == 0
        grid, _, sl = slices_of(v)
        assert grid == 256 and all(rmul == 0 for _, rmul in sl), (jobs, sl)
        if jobs[0]["N"] != 128256:
            assert v[18] != 0, jobs
    gate_up = QWEN72[2]
    rc, v = plan(lib, *gate_up, 256)
    assert rc == 0 and v[18] == 1 and slices_of(v)[2][0] == (115, 1 << 31)      # 29568 = 115.5 x 256: the HOT pair form with a remainder


def test_multiplier_is_exact_up_to_the_refused_grid():
    """rmul = ceil(2^32 rem / grid) restated; b * rmul >> 32 == floor(b * rem / grid) for every b <= grid: every remainder of the grids in use, and the
    remainders that come closest to failing (large rem, eps = rmul * grid - 2^32 rem close to grid) just below the refused 65536"""
    def check(grid, rem):
        rmul = ((rem << 32) + grid - 1) // grid
        assert rmul < 1 << 32
        assert all((b * rmul) >> 32 == b * rem // grid for b in range(grid + 1)), (grid, rem)
    for grid in (64, 256, 304, 512, 608, 1024):
        for rem in range(grid):
            check(grid, rem)
    for grid in (65535, 65521, 49152 + 1, 40000):
        worst = sorted(range(1, grid), key=lambda r: (-(((r << 32) + grid - 1) // grid * grid - (r << 32)), -r))[:6]
        for rem in worst + [1, grid - 1, grid // 2, grid // 3]:
            check(grid, rem)


def test_a_caller_of_19_values_sees_what_it_saw(lib):
    jobs, K, x_mode, qkv = LLAMA70[0]
    rc25, v25 = plan(lib, jobs, K, x_mode, qkv)
    rc19, v19 = plan(lib, jobs, K, x_mode, qkv, n_out=19)
    assert rc25 == 0 and rc19 == 0 and v19[:19] == v25[:19] and v19[19:] == [-12345] * 6
    assert v25[19:22] == [32, 4, 4] and v25[22:] == [0, 0, 0]
    rc, v = plan(lib, jobs, K, x_mode, qkv, n_out=40, room=40)               # more room than values: the rest stays untouched
    assert rc == 0 and v[:25] == v25 and v[25:] == [-12345] * 15


def test_a_grid_the_multiplier_cannot_serve_is_refused(lib):
    """65536 workgroups and more (over 33 million rows): refused with the shape code instead of planned with an inexact multiplier"""
    rc, _ = plan(lib, [J(Q6_K, 509 * 32768)], 256, 2, None, 256)
    assert rc == 0
    rc, _ = plan(lib, [J(Q6_K, 509 * 65536)], 256, 2, None, 256)
    assert rc == -2
