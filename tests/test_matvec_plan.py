"""The single-token mat-vec's host plan (pm_gemv_fused_plan, prima_cpp_amd/csrc/mmvq.hip), checked without a GPU through pm355_mul_mat_vec_fused_plan.

(a) The rules of the launcher in front of the plan - gemv_fill and the if-ladder launch_types() of the commit before this file - restated in Python
    (parent_plan below): the grid and its doubling past 512 rows per workgroup, what the RoPE + KV-store epilogue asks of the rows, the heads and the NEOX
    slices, `split`, the TA-first swap, the LDS bytes, and which of gemv_q_kernel<TA, TB, PAIR, DBG, EPI, NPRE, FEAT, XM, HOT>'s forms a launch takes - for
    every rung of the ladder and for every launch that just misses a HOT rung (a HOT kernel overwrites fields of its argument block: a launch that took
    one without matching its pattern would lose a bias, a residual or a job without a word). The attention-tail rungs need pointers the plan entry does not
    take; tests/test_gpu_experiments.py runs them.
(b) What the mat-vec entries of the C ABI refuse before anything is launched: codes and pm355_last_error texts as recorded from the build in front of the
    plan. Every pointer is a dummy that is never followed."""
import ctypes as C
import itertools
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q4_0, Q5_0, Q8_0, Q4_K, Q5_K, Q6_K = 2, 6, 8, 12, 13, 14
NV = {Q4_K: 64, Q5_K: 32, Q6_K: 64, Q8_0: 32, Q5_0: 32}                # values per unit of the mat-vec (pm355_types.h)
BLK = {Q4_K: 256, Q5_K: 256, Q6_K: 256, Q8_0: 32, Q5_0: 32}            # activation block the type multiplies with
PAIRS = [(Q4_K, Q4_K), (Q5_K, Q5_K), (Q6_K, Q6_K), (Q8_0, Q8_0), (Q5_0, Q5_0), (Q4_K, Q6_K), (Q4_K, Q5_K)]      # PM_GEMV_TYPE_PAIRS
MAX_ROWS_PER_WG, NW, CH64, CH32 = 512, 16, 1, 2
SS, TAIL, NEOX = 1, 2, 4
P = 4096                                                               # a non-null pointer nobody follows


def J(t, N, w2=False, bias=False, resid=False):
    return dict(t=t, N=N, w2=w2, bias=bias, resid=resid)


def Qkv(Hkv, dh, n_rot=None, neox=False, v_rowmajor=False, dyn=False):
    return dict(Hkv=Hkv, dh=dh, n_rot=dh if n_rot is None else n_rot, neox=neox, v_rowmajor=v_rowmajor, dyn=dyn)


def act_lds(K, blk):
    return ((K + 15) & ~15) + (K // 16) * 4 + ((K // blk + 3) & ~3) * 4


def parent_plan(jobs, K, x_mode, qkv=None, cus=256, xm_spec=True, hot_spec=True, experiments=False):
    """gemv_fill + launch_types of the parent, line by line. x_mode as pm355_mul_mat_vec_fused_plan takes it. A refusal code, or
    (grid, lds, ta, tb, pair, first, split[3], nx_s[3], (PAIR, DBG, EPI, NPRE, FEAT, XM, HOT))."""
    xmode, dbg, ss_out = x_mode & 3, bool(x_mode & 4), bool(x_mode & 8)
    hot_spec = hot_spec and xm_spec
    if ss_out and (len(jobs) != 1 or jobs[0]["w2"] or qkv or dbg):
        return -6
    ta = tb = jobs[0]["t"]
    pair = jobs[0]["w2"]
    for j in jobs:
        t = j["t"]
        if t not in NV:
            return -1
        if t != ta:
            if tb == ta:
                tb = t
            elif t != tb:
                return -1
        if j["w2"] != pair:
            return -1
    if (BLK[ta] == 32) != (BLK[tb] == 32):
        return -1
    if K % BLK[ta]:
        return -2
    if pair and ta != tb:
        return -1
    if (ta, tb) not in PAIRS:
        ta, tb = tb, ta
        if (ta, tb) not in PAIRS:
            return -1
    grid = cus
    tot = sum(j["N"] for j in jobs)
    while (tot + grid - 1) // grid + 3 > MAX_ROWS_PER_WG:
        grid *= 2
    blk = []
    for i, j in enumerate(jobs):
        g = dict(N=j["N"], is_b=j["t"] != ta, bias=j["bias"], resid=j["resid"], role=0, split=0, nx_s=0, src=i)
        if qkv:
            if pair or len(jobs) != 3 or j["N"] % (2 * grid) or dbg:
                return -5
            g["role"] = i + 1
            upl = (K // NV[j["t"]] + 63) >> 6
            ch = CH64 if NV[j["t"]] == 64 else CH32
            cpr = (upl + ch - 1) // ch
            g["split"] = int(i > 0 and j["N"] // grid < NW and cpr > 1)
            if qkv["neox"] and i < 2:
                sl, dh = j["N"] // grid, qkv["dh"]
                pow2 = lambda v: v > 0 and not (v & (v - 1))
                if qkv["n_rot"] != dh or not pow2(dh) or not pow2(sl) or sl < 2 or sl > dh:
                    return -5
                g["nx_s"] = sl.bit_length() - 1
        blk.append(g)
    while len(blk) < 3:
        blk.append(dict(N=0, is_b=False, bias=False, resid=False, role=0, split=0, nx_s=0, src=-1))
    if qkv:
        dh, kv = qkv["dh"], qkv["Hkv"] * qkv["dh"]
        if dh % 2 or qkv["n_rot"] % 2 or qkv["n_rot"] > dh or jobs[0]["N"] % dh or jobs[1]["N"] != kv or jobs[2]["N"] != kv:
            return -5
    first = 0
    if blk[0]["is_b"]:
        for i in (1, 2):
            if blk[i]["N"] > 0 and not blk[i]["is_b"]:
                blk[0], blk[i] = blk[i], blk[0]
                first = i
                break
    lds = act_lds(K, BLK[ta]) + MAX_ROWS_PER_WG * 4
    if lds > 150 * 1024:
        return -4
    # ---- launch_types<TA, TB>: the ladder
    epi = qkv is not None
    ss = ss_out or xmode == 3
    if not experiments and ss:
        return -8
    one_job = blk[1]["N"] == 0 and blk[2]["N"] == 0
    neox = epi and any(b["nx_s"] > 0 for b in blk)
    b0 = blk[0]
    if pair:
        if ta != tb:
            return -1
        if dbg:
            if ss:
                return -6
            form = (1, 1, 0, 1, 0, -1, 0)
        elif ss:
            form = (1, 0, 0, 1, SS, -1, 0)
        elif xmode == 2 and hot_spec and one_job and not b0["bias"] and not b0["resid"] and not b0["split"]:
            form = (1, 0, 0, 1, 0, 2, 1)
        elif xmode == 2 and xm_spec:
            form = (1, 0, 0, 1, 0, 2, 0)
        else:
            form = (1, 0, 0, 1, 0, -1, 0)
    elif epi:
        if dbg:
            return -1
        if neox and ss:
            form = (0, 0, 1, 2, NEOX | SS, -1, 0)
        elif ss:
            form = (0, 0, 1, 2, SS, -1, 0)
        elif neox:
            form = (0, 0, 1, 2, NEOX, -1, 0)
        elif (xmode == 2 and hot_spec and not any(b["bias"] for b in blk) and not qkv["v_rowmajor"] and [b["role"] for b in blk] == [1, 2, 3] and
              not blk[0]["is_b"] and not blk[1]["is_b"] and blk[2]["is_b"] == (ta != tb) and not b0["split"] and not any(b["resid"] for b in blk)):
            form = (0, 0, 1, 2, 0, 2, 2 if qkv["dyn"] else 1)
        elif xmode == 2 and xm_spec:
            form = (0, 0, 1, 2, 0, 2, 0)
        else:
            form = (0, 0, 1, 2, 0, -1, 0)
    else:
        if dbg:
            if ss:
                return -6
            form = (0, 1, 0, 1, 0, -1, 0)
        elif ss:
            form = (0, 0, 0, 2, SS, -1, 0)
        elif xmode == 1 and hot_spec and one_job and not b0["bias"] and b0["resid"] and not b0["split"] and not b0["is_b"]:
            form = (0, 0, 0, 2, 0, 1, 1)
        elif xmode == 1 and xm_spec:
            form = (0, 0, 0, 2, 0, 1, 0)
        elif xmode == 2 and xm_spec:
            form = (0, 0, 0, 2, 0, 2, 0)
        else:
            form = (0, 0, 0, 2, 0, -1, 0)
    return (grid, lds, ta, tb, int(pair), first, tuple(b["split"] for b in blk), tuple(b["nx_s"] for b in blk), form)


class MatvecJob(C.Structure):
    _fields_ = [("type", C.c_int32), ("pad_", C.c_int32), ("N", C.c_int64), ("W", C.c_void_p), ("W2", C.c_void_p), ("y", C.c_void_p), ("bias", C.c_void_p),
                ("resid", C.c_void_p)]


class QkvStore(C.Structure):
    _fields_ = [("rope_table", C.c_void_p), ("d_pos", C.c_void_p), ("d_cell_nkv", C.c_void_p), ("k_cache", C.c_void_p), ("v_cache", C.c_void_p),
                ("n_head_kv", C.c_int32), ("head_dim", C.c_int32), ("n_ctx", C.c_int32), ("n_rot", C.c_int32), ("v_rowmajor", C.c_int32), ("rope_neox", C.c_int32)]


def c_jobs(jobs):
    a = (MatvecJob * max(len(jobs), 1))()
    for i, j in enumerate(jobs):
        a[i] = MatvecJob(j["t"], 0, j["N"], P, P if j["w2"] else None, P, P if j["bias"] else None, P if j["resid"] else None)
    return a


def c_store(q, n_ctx=64):
    return QkvStore(P, None if q["dyn"] else P, P if q["dyn"] else None, P, P, q["Hkv"], q["dh"], n_ctx, q["n_rot"], int(q["v_rowmajor"]), int(q["neox"]))


def lib_plan(lib, jobs, K, x_mode, qkv=None, cus=256):
    f = lib.pm355_mul_mat_vec_fused_plan
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    a, out = c_jobs(jobs), (C.c_int32 * 19)()
    st = c_store(qkv) if qkv else None
    rc = f(a, len(jobs), K, x_mode, C.addressof(st) if qkv else None, cus, out, 19)
    v = list(out)
    return rc if rc else (v[0], v[1], v[2], v[3], v[4], v[5], tuple(v[6:9]), tuple(v[9:12]), tuple(v[12:19]))


def form_cases():
    """(jobs, K, x_mode, qkv): every rung of the ladder and the launches next to it"""
    cases = []
    flags = list(itertools.product((False, True), repeat=2))
    for t, K in itertools.product((Q4_K, Q5_K, Q6_K, Q8_0, Q5_0), (256, 768)):
        for x_mode, (bias, resid) in itertools.product((0, 1, 2, 3, 4, 5, 6, 7, 9, 10), flags):
            cases.append(([J(t, 33, bias=bias, resid=resid)], K, x_mode, None))                        # wo / ffn_down / lm_head and their near-misses
            cases.append(([J(t, 33, w2=True, bias=bias, resid=resid)], K, x_mode, None))               # ffn_gate | ffn_up
        for x_mode in (0, 1, 2, 3):                                                                   # a second / third job takes no HOT form
            cases.append(([J(t, 33, resid=True), J(t, 40, resid=True)], K, x_mode, None))
            cases.append(([J(t, 33, w2=True), J(t, 40, w2=True)], K, x_mode, None))
            cases.append(([J(t, 33, resid=True)] * 2, K, x_mode | 8, None))                            # sumsq_out on two jobs
    for mix in ((Q4_K, Q4_K, Q4_K), (Q4_K, Q4_K, Q6_K), (Q4_K, Q4_K, Q5_K), (Q6_K, Q6_K, Q6_K), (Q5_K, Q5_K, Q5_K), (Q8_0, Q8_0, Q8_0), (Q6_K, Q4_K, Q4_K),
                (Q4_K, Q6_K, Q4_K), (Q5_K, Q4_K, Q4_K), (Q6_K, Q6_K, Q4_K), (Q4_K, Q6_K, Q5_K), (Q6_K, Q5_K, Q5_K), (Q4_K, Q4_K, Q8_0), (Q8_0, Q8_0, Q5_0),
                (Q4_K, Q4_K, Q4_0)):
        for x_mode in (0, 1, 2, 3, 6):
            cases.append(([J(t, 512) for t in mix], 512, x_mode, None))                                # three plain jobs
            for kw in (dict(), dict(dyn=True), dict(v_rowmajor=True), dict(neox=True), dict(neox=True, dyn=True), dict(n_rot=32), dict(neox=True, n_rot=32)):
                cases.append(([J(t, 512) for t in mix], 512, x_mode, Qkv(8, 64, **kw)))               # wq | wk | wv with the epilogue
            for b in range(3):                                                                        # a bias on any job; a residual; a pair
                cases.append(([J(t, 512, bias=(i == b)) for i, t in enumerate(mix)], 512, x_mode, Qkv(8, 64)))
                cases.append(([J(t, 512, bias=(i == b)) for i, t in enumerate(mix)], 512, x_mode, Qkv(8, 64, dyn=True)))
            cases.append(([J(t, 512, w2=True) for t in mix], 512, x_mode, Qkv(8, 64)))
    # the epilogue's row, head and slice conditions; split; the 70B and Qwen2.5-72B layers
    for Ns, K, q in (((8192, 1024, 1024), 8192, Qkv(8, 128)), ((8192, 1024, 1024), 8192, Qkv(8, 128, neox=True)), ((4096, 1024, 1024), 4096, Qkv(8, 128)),
                     ((512, 512, 256), 512, Qkv(8, 64)), ((512, 256, 256), 512, Qkv(4, 64)), ((512, 512, 512), 512, Qkv(8, 64, n_rot=66)),
                     ((512, 512, 512), 512, Qkv(8, 64, n_rot=31)), ((1536, 1536, 1536), 512, Qkv(16, 96, neox=True)), ((1536, 512, 512), 512, Qkv(8, 64, neox=True)),
                     ((2048, 512, 512), 2048, Qkv(8, 64)), ((32768, 32768, 32768), 512, Qkv(256, 128, neox=True)), ((480, 512, 512), 512, Qkv(8, 64)),
                     ((65536, 1024, 1024), 512, Qkv(8, 128, neox=True))):
        for mix in ((Q4_K, Q4_K, Q4_K), (Q4_K, Q4_K, Q6_K), (Q4_K, Q4_K, Q5_K), (Q5_K, Q5_K, Q5_K), (Q8_0, Q8_0, Q8_0)):
            cases.append(([J(t, n) for t, n in zip(mix, Ns)], K, 2, q))
    cases.append(([J(Q4_K, 512), J(Q4_K, 512)], 512, 2, Qkv(8, 64)))                                   # the epilogue on two jobs
    # the grid doubles past 512 rows per workgroup; the activation must fit 150 KB of LDS next to the parked results
    for N in (33, 128256, 130000, 131072 - 3 * 256, 131072 - 3 * 256 + 1, 152064, 300000):
        cases.append(([J(Q6_K, N)], 256, 2, None))
        cases.append(([J(Q4_K, N), J(Q4_K, 1024)], 256, 1, None))
    for t in (Q4_K, Q5_K, Q8_0):
        for K in (8192, 28672, 29568 if t == Q8_0 else 29696, 118784, 119808, 122880, 110080, 110592):
            cases.append(([J(t, 64, resid=True)], K, 1, None))
    for K in (0, 128, 300, 8192 + 32):                                                                 # K against the block length
        cases.append(([J(Q4_K, 64)], K, 1, None))
        cases.append(([J(Q8_0, 64)], K, 1, None))
    return cases


CASES = form_cases()


@pytest.fixture(scope="module")
def lib():
    import prima_cpp_amd
    return prima_cpp_amd.load()              # (loads without a GPU, tests/test_abi.py)


@pytest.mark.parametrize("cus", [256, 64, 304])
def test_plan_is_the_former_launchers_arithmetic(lib, cus):
    seen, refusals = set(), set()
    for jobs, K, x_mode, qkv in CASES:
        want = parent_plan(jobs, K, x_mode, qkv, cus)
        assert lib_plan(lib, jobs, K, x_mode, qkv, cus) == want, (jobs, K, x_mode, qkv)
        (refusals if isinstance(want, int) else seen).add(want if isinstance(want, int) else want[8])
    if cus != 304:                           # (304 CUs: no shape here gives every workgroup whole rotation pairs - the epilogue forms are refused)
        assert len(seen) == 14, sorted(seen)     # every form of the product library was taken by some case ...
    assert refusals >= {-1, -2, -4, -5, -6, -8}


def test_plan_cases_reach_what_they_are_meant_to():
    """the cases above, against the restated rules alone: they double the grid, swap a TA job to the front, split wk / wv, and sit on both sides of every
    HOT rung"""
    plans = [(c, parent_plan(*c)) for c in CASES]
    ok = [(c, p) for c, p in plans if not isinstance(p, int)]
    assert {p[0] for _, p in ok} >= {256, 512, 1024} and {p[5] for _, p in ok} == {0, 1, 2}
    assert any(p[6] == (0, 1, 1) for _, p in ok) and any(p[6] == (0, 0, 0) and c[3] for c, p in ok)
    assert {p[7] for _, p in ok} >= {(0, 0, 0), (1, 1, 0), (5, 2, 0)}
    hot = {}
    for (jobs, K, x_mode, qkv), p in ok:
        key = (len(jobs), bool(jobs[0]["w2"]), qkv is not None)
        hot.setdefault(key, set()).add(p[8][6])
    assert hot[(1, False, False)] == {0, 1} and hot[(1, True, False)] == {0, 1} and hot[(3, False, True)] == {0, 1, 2}
    assert hot[(2, False, False)] == {0} and hot[(3, False, False)] == {0}
    # the near-misses of the HOT rungs named one by one: each takes the XM form (or the plain one) of its rung
    e = Qkv(8, 64)
    q3 = lambda **kw: [J(Q4_K, 512, **kw), J(Q4_K, 512), J(Q6_K, 512)]
    for jobs, x_mode, qkv, form in (
            ([J(Q4_K, 33, resid=True)], 1, None, (0, 0, 0, 2, 0, 1, 1)), ([J(Q4_K, 33)], 1, None, (0, 0, 0, 2, 0, 1, 0)),
            ([J(Q4_K, 33, resid=True, bias=True)], 1, None, (0, 0, 0, 2, 0, 1, 0)), ([J(Q4_K, 33, resid=True)], 2, None, (0, 0, 0, 2, 0, 2, 0)),
            ([J(Q4_K, 33, resid=True)], 0, None, (0, 0, 0, 2, 0, -1, 0)), ([J(Q4_K, 33, resid=True)] * 2, 1, None, (0, 0, 0, 2, 0, 1, 0)),
            ([J(Q4_K, 33, w2=True)], 2, None, (1, 0, 0, 1, 0, 2, 1)), ([J(Q4_K, 33, w2=True, resid=True)], 2, None, (1, 0, 0, 1, 0, 2, 0)),
            ([J(Q4_K, 33, w2=True, bias=True)], 2, None, (1, 0, 0, 1, 0, 2, 0)), ([J(Q4_K, 33, w2=True)], 1, None, (1, 0, 0, 1, 0, -1, 0)),
            ([J(Q4_K, 33, w2=True)] * 2, 2, None, (1, 0, 0, 1, 0, 2, 0)),
            (q3(), 2, e, (0, 0, 1, 2, 0, 2, 1)), (q3(), 2, Qkv(8, 64, dyn=True), (0, 0, 1, 2, 0, 2, 2)), (q3(bias=True), 2, e, (0, 0, 1, 2, 0, 2, 0)),
            (q3(), 2, Qkv(8, 64, v_rowmajor=True), (0, 0, 1, 2, 0, 2, 0)), (q3(), 1, e, (0, 0, 1, 2, 0, -1, 0)), (q3(), 0, e, (0, 0, 1, 2, 0, -1, 0)),
            ([J(Q6_K, 512), J(Q4_K, 512), J(Q4_K, 512)], 2, e, (0, 0, 1, 2, 0, 2, 0)), ([J(Q4_K, 512), J(Q6_K, 512), J(Q4_K, 512)], 2, e, (0, 0, 1, 2, 0, 2, 0)),
            (q3(), 2, Qkv(8, 64, neox=True), (0, 0, 1, 2, NEOX, -1, 0))):
        assert parent_plan(jobs, 512, x_mode, qkv)[8] == form, (jobs, x_mode, qkv)


SWITCH_CASES = [c for c in CASES if c[2] in (1, 2) and c[1] in (256, 512)]


@pytest.mark.parametrize("env,xm,hot", [({"PM355_XMODE_SPEC": "0"}, False, False), ({"PM355_HOT_SPEC": "0"}, True, False)], ids=["PM355_XMODE_SPEC=0", "PM355_HOT_SPEC=0"])
def test_plan_with_a_switch_off(env, xm, hot):
    """the A/B switches are read once per process: a process of its own plans the f32 / rms_norm cases with each of them off"""
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=dict(os.environ, **env), cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    got = json.loads(r.stdout.splitlines()[-1])
    assert len(got) == len(SWITCH_CASES) > 300
    forms = set()
    for (jobs, K, x_mode, qkv), g in zip(SWITCH_CASES, got):
        want = parent_plan(jobs, K, x_mode, qkv, 256, xm_spec=xm, hot_spec=hot)
        assert (g if isinstance(g, int) else tuple(g)) == (want if isinstance(want, int) else want[8]), (jobs, K, x_mode, qkv)
        if not isinstance(want, int):
            forms.add((want[8][5], want[8][6]))
    assert forms == ({(-1, 0)} if not xm else {(-1, 0), (1, 0), (2, 0)})


def test_experiments_library_plans_its_own_forms():
    """libprima_mi355_exp.so carries the sum-of-squares forms the product library answers -8 for (the attention tail's need pointers: GPU tests)"""
    path = os.path.join(ROOT, "prima_cpp_amd", "libprima_mi355_exp.so")
    assert os.path.exists(path), "prima_cpp_amd/libprima_mi355_exp.so not built (__graft_entry__.build() builds it)"
    import prima_cpp_amd  # noqa: F401  (the HIP runtime both libraries resolve)
    exp = C.CDLL(path)
    seen = set()
    for jobs, K, x_mode, qkv in CASES:
        want = parent_plan(jobs, K, x_mode, qkv, 256, experiments=True)
        assert lib_plan(exp, jobs, K, x_mode, qkv, 256) == want, (jobs, K, x_mode, qkv)
        if not isinstance(want, int):
            seen.add(want[8])
    assert len(seen) == 18 and {f[4] for f in seen} == {0, SS, NEOX, NEOX | SS}      # 20 forms less the two with the attention tail


# ---- (b) refusals in front of a launch, recorded from the parent build -----------------------------------------------------------------------------
UNSUPPORTED, SHAPE, RANGE, HIP = -1, -2, -4, -10
MSG = {
    "type": "mul_mat_vec_q: weight type",
    "block": "mul_mat_vec_q: K not a multiple of the block size",
    "lds": "mul_mat_vec_q: K too large",
    "exp": "mul_mat_vec_q: sum-of-squares partials / attention tail are built into libprima_mi355_exp.so only (PM_EXPERIMENTS)",
    "ncols": "mul_mat_vec_q: ncols must be 1..8",
    "fused_args": "mul_mat_vec_fused: 1..3 jobs and an f32 activation",
    "ss_args": "mul_mat_vec_fused_ss: 1..3 jobs and an f32 activation",
    "ss": "mul_mat_vec_fused_ss: sumsq_out needs ONE plain job; sumsq_in needs norm_w and 1..256 partials",
    "grid_args": "mul_mat_vec_fused_grid: 1..3 jobs",
    "check_args": "mul_mat_vec_fused: 1..3 jobs",
    "qkv_null": "mul_mat_vec_qkv: null pointer",
    "qkv": "mul_mat_vec_qkv: every workgroup's row slices must hold whole rotation pairs (N % (2 * CUs) == 0), N_k == N_v == n_head_kv * head_dim",
    "qkv_attn_null": "mul_mat_vec_qkv_attn: null pointer",
    "qkv_check_null": "mul_mat_vec_qkv_check: jobs",
    "launch": "mul_mat_vec_q: launch",       # (a refusal this entry has no text for: reported as a failed launch, with the runtime's last error behind it)
    "engine": "engine_run: the persistent decode engine is built into libprima_mi355_exp.so only (PM_EXPERIMENTS)",
}
vp, i32, i64, f32 = C.c_void_p, C.c_int, C.c_int64, C.c_float


def entry(lib, name, argtypes):
    f = getattr(lib, name)
    f.restype, f.argtypes = C.c_int, argtypes
    return f


def vec_q(t=Q4_K, K=4096, N=64, ncols=1, w2=None):
    return lambda lib: entry(lib, "pm355_mul_mat_vec_q", [i32, vp, vp, i64, i64, vp, i32, vp, i64, vp, vp, vp])(t, P, w2, K, N, P, ncols, P, N, None, None, None)


def vec_dbg(t=Q4_K, K=4096):
    return lambda lib: entry(lib, "pm355_mul_mat_vec_q_dbg", [i32, vp, i64, i64, vp, vp, vp, vp, vp])(t, P, K, 64, P, P, P, None, None)


def fused(jobs, K=4096, x=P, name="pm355_mul_mat_vec_fused", n=None, null_jobs=False):
    def call(lib):
        a = c_jobs(jobs)
        return entry(lib, name, [vp, i32, i64, vp, vp, f32, vp])(None if null_jobs else a, len(jobs) if n is None else n, K, x, None, 0.0, None)
    return call


def fused_ss(jobs, K=4096, x=P, norm_w=None, ss_out=None, ss_in=None, n_ss=0, n=None):
    def call(lib):
        a = c_jobs(jobs)
        return entry(lib, "pm355_mul_mat_vec_fused_ss", [vp, i32, i64, vp, vp, f32, vp, vp, i32, vp])(a, len(jobs) if n is None else n, K, x, norm_w, 0.0,
                                                                                                  ss_out, ss_in, n_ss, None)
    return call


def grid_or_check(name, jobs, K=4096, n=None, null_jobs=False):
    def call(lib):
        a = c_jobs(jobs)
        return entry(lib, name, [vp, i32, i64])(None if null_jobs else a, len(jobs) if n is None else n, K)
    return call


def qkv(jobs, K=512, q=None, x=P, null_store=False, ss_in=None, n_ss=0, norm_w=None, attn=None, name="pm355_mul_mat_vec_qkv_attn"):
    def call(lib):
        a, st = c_jobs(jobs), c_store(q or Qkv(8, 64))
        s = None if null_store else C.addressof(st)
        if name == "pm355_mul_mat_vec_qkv":
            return entry(lib, name, [vp, i64, vp, vp, f32, vp, vp])(a, K, x, norm_w, 0.0, s, None)
        if name == "pm355_mul_mat_vec_qkv_ss":
            return entry(lib, name, [vp, i64, vp, vp, f32, vp, vp, i32, vp])(a, K, x, norm_w, 0.0, s, ss_in, n_ss, None)
        at = (C.c_uint64 * 4)(*(attn or (0, 0, 0, 0)))       # pm355_qkv_attn {out, ticket, watchdog, {kq_scale, n_head}, max_keys}
        return entry(lib, name, [vp, i64, vp, vp, f32, vp, vp, i32, vp, vp])(a, K, x, norm_w, 0.0, s, ss_in, n_ss, C.addressof(at) if attn else None, None)
    return call


def qkv_check(jobs, K=512, Hkv=8, dh=64, n_rot=64, neox=0, null_jobs=False):
    def call(lib):
        a = c_jobs(jobs)
        return entry(lib, "pm355_mul_mat_vec_qkv_check_ex", [vp, i64, i32, i32, i32, i32])(None if null_jobs else a, K, Hkv, dh, n_rot, neox)
    return call


def q3(N=(512, 512, 512), mix=(Q4_K, Q4_K, Q6_K), **kw):
    return [J(t, n, **kw) for t, n in zip(mix, N)]


one = [J(Q4_K, 64)]
# (name, call, code, text; None: the entry leaves no text of its own)
REFUSALS = [
    ("vec_q: no columns", vec_q(ncols=0), RANGE, "ncols"),
    ("vec_q: nine columns", vec_q(ncols=9), RANGE, "ncols"),
    ("vec_q: unserved type", vec_q(t=Q4_0), UNSUPPORTED, "type"),
    ("vec_q: Q8_K is no weight", vec_q(t=15), UNSUPPORTED, "type"),
    ("vec_q: K % 256", vec_q(K=4096 + 64), SHAPE, "block"),
    ("vec_q: Q8_0 K % 32", vec_q(t=Q8_0, K=4096 + 16), SHAPE, "block"),
    ("vec_q: 8 columns, K % 256", vec_q(K=4096 + 64, ncols=8), SHAPE, "block"),
    ("vec_q: pair, K % 256", vec_q(K=4096 + 64, ncols=2, w2=P), SHAPE, "block"),
    ("vec_q: K beyond LDS", vec_q(K=122880), RANGE, "lds"),
    ("vec_q: 4 columns, K beyond LDS", vec_q(K=122880, ncols=4), RANGE, "lds"),
    ("vec_q_dbg: unserved type", vec_dbg(t=Q4_0), UNSUPPORTED, "type"),
    ("vec_q_dbg: K % 256", vec_dbg(K=4096 + 64), SHAPE, "block"),
    ("fused: no jobs", fused(one, n=0), RANGE, "fused_args"),
    ("fused: four jobs", fused(one, n=4), RANGE, "fused_args"),
    ("fused: null jobs", fused(one, null_jobs=True), RANGE, "fused_args"),
    ("fused: null activation", fused(one, x=None), RANGE, "fused_args"),
    ("fused: unserved type", fused([J(Q4_0, 64)]), UNSUPPORTED, "type"),
    ("fused: three types", fused([J(Q4_K, 64), J(Q6_K, 64), J(Q5_K, 64)]), UNSUPPORTED, "type"),
    ("fused: Q6_K next to Q5_K", fused([J(Q6_K, 64), J(Q5_K, 64)]), UNSUPPORTED, "type"),
    ("fused: K-quant next to Q8_0", fused([J(Q4_K, 64), J(Q8_0, 64)]), UNSUPPORTED, "type"),
    ("fused: Q8_0 next to Q5_0", fused([J(Q8_0, 64), J(Q5_0, 64)]), UNSUPPORTED, "type"),
    ("fused: pair next to plain", fused([J(Q4_K, 64, w2=True), J(Q4_K, 64)]), UNSUPPORTED, "type"),
    ("fused: pair of two types", fused([J(Q4_K, 64, w2=True), J(Q6_K, 64, w2=True)]), UNSUPPORTED, "type"),
    ("fused: K % 256", fused(one, K=4096 + 32), SHAPE, "block"),
    ("fused: K beyond LDS", fused(one, K=122880), RANGE, "lds"),
    ("fused_ss: no jobs", fused_ss(one, n=0), RANGE, "ss_args"),
    ("fused_ss: null activation", fused_ss(one, x=None), RANGE, "ss_args"),
    ("fused_ss: partials without norm_w", fused_ss(one, ss_in=P, n_ss=4), UNSUPPORTED, "ss"),
    ("fused_ss: no partials", fused_ss(one, norm_w=P, ss_in=P, n_ss=0), UNSUPPORTED, "ss"),
    ("fused_ss: 257 partials", fused_ss(one, norm_w=P, ss_in=P, n_ss=257), UNSUPPORTED, "ss"),
    ("fused_ss: sumsq_out on two jobs", fused_ss([J(Q4_K, 64)] * 2, ss_out=P), UNSUPPORTED, "ss"),
    ("fused_ss: sumsq_out on a pair", fused_ss([J(Q4_K, 64, w2=True)], ss_out=P), UNSUPPORTED, "ss"),
    ("fused_ss: sumsq_out asked of the product library", fused_ss(one, ss_out=P), UNSUPPORTED, "exp"),
    ("fused_ss: sumsq_in asked of the product library", fused_ss(one, norm_w=P, ss_in=P, n_ss=4), UNSUPPORTED, "exp"),
    ("fused_ss: unserved type", fused_ss([J(Q4_0, 64)]), UNSUPPORTED, "type"),
    ("fused_grid: no jobs", grid_or_check("pm355_mul_mat_vec_fused_grid", one, n=0), RANGE, "grid_args"),
    ("fused_grid: null jobs", grid_or_check("pm355_mul_mat_vec_fused_grid", one, null_jobs=True), RANGE, "grid_args"),
    ("fused_grid: unserved type", grid_or_check("pm355_mul_mat_vec_fused_grid", [J(Q4_0, 64)]), UNSUPPORTED, "type"),
    ("fused_grid: K % 256", grid_or_check("pm355_mul_mat_vec_fused_grid", one, K=300), SHAPE, "block"),
    ("fused_grid: K beyond LDS", grid_or_check("pm355_mul_mat_vec_fused_grid", one, K=122880), RANGE, "lds"),
    ("fused_check: four jobs", grid_or_check("pm355_mul_mat_vec_fused_check", one, n=4), RANGE, "check_args"),
    ("fused_check: three types", grid_or_check("pm355_mul_mat_vec_fused_check", [J(Q4_K, 64), J(Q6_K, 64), J(Q5_K, 64)]), UNSUPPORTED, "type"),
    ("fused_check: K % 256", grid_or_check("pm355_mul_mat_vec_fused_check", one, K=300), SHAPE, "block"),
    ("fused_check: K beyond LDS", grid_or_check("pm355_mul_mat_vec_fused_check", one, K=122880), RANGE, "lds"),
    ("qkv: null store", qkv(q3(), null_store=True, name="pm355_mul_mat_vec_qkv"), SHAPE, "qkv_null"),
    ("qkv: null activation", qkv(q3(), x=None, name="pm355_mul_mat_vec_qkv"), SHAPE, "qkv_null"),
    ("qkv: rows per workgroup", qkv(q3(N=(512, 256, 256)), q=Qkv(4, 64), name="pm355_mul_mat_vec_qkv"), UNSUPPORTED, "qkv"),
    ("qkv: wk rows against the heads", qkv(q3(), q=Qkv(4, 64), name="pm355_mul_mat_vec_qkv"), UNSUPPORTED, "qkv"),
    ("qkv: odd n_rot", qkv(q3(), q=Qkv(8, 64, n_rot=31), name="pm355_mul_mat_vec_qkv"), UNSUPPORTED, "qkv"),
    ("qkv: n_rot > head_dim", qkv(q3(), q=Qkv(8, 64, n_rot=66), name="pm355_mul_mat_vec_qkv"), UNSUPPORTED, "qkv"),
    ("qkv: NEOX with n_rot < head_dim", qkv(q3(), q=Qkv(8, 64, n_rot=32, neox=True), name="pm355_mul_mat_vec_qkv"), UNSUPPORTED, "qkv"),
    ("qkv: NEOX slices of 6 rows", qkv(q3(N=(1536, 1536, 1536)), q=Qkv(16, 96, neox=True), name="pm355_mul_mat_vec_qkv"), UNSUPPORTED, "qkv"),
    ("qkv: three types", qkv(q3(mix=(Q4_K, Q6_K, Q5_K)), name="pm355_mul_mat_vec_qkv"), UNSUPPORTED, "type"),
    ("qkv: K % 256", qkv(q3(), K=544, name="pm355_mul_mat_vec_qkv"), SHAPE, "block"),
    ("qkv_ss: partials asked of the product library", qkv(q3(), norm_w=P, ss_in=P, n_ss=4, name="pm355_mul_mat_vec_qkv_ss"), UNSUPPORTED, "exp"),
    ("qkv_ss: 257 partials", qkv(q3(), norm_w=P, ss_in=P, n_ss=257, name="pm355_mul_mat_vec_qkv_ss"), HIP, "launch"),
    ("qkv_attn: null output", qkv(q3(), attn=(0, P, 0, 0)), SHAPE, "qkv_attn_null"),
    ("qkv_attn: tail asked of the product library", qkv(q3(N=(512, 512, 512)), q=Qkv(8, 64), attn=(P, P, 0, 8 << 32)), UNSUPPORTED, "exp"),
    ("qkv_check: null jobs", qkv_check(q3(), null_jobs=True), SHAPE, "qkv_check_null"),
    ("qkv_check: three types", qkv_check(q3(mix=(Q4_K, Q6_K, Q5_K))), UNSUPPORTED, "type"),
    ("qkv_check: K % 256", qkv_check(q3(), K=544), SHAPE, "block"),
    ("qkv_check: rows per workgroup", qkv_check(q3(N=(512, 256, 256)), Hkv=4), UNSUPPORTED, None),
    ("qkv_check: NEOX with n_rot < head_dim", qkv_check(q3(), n_rot=32, neox=1), UNSUPPORTED, None),
    ("engine_run: the product library", lambda lib: entry(lib, "pm355_engine_run", [vp, i32, vp])(None, 0, None), UNSUPPORTED, "engine"),
]


@pytest.mark.parametrize("name,call,code,msg", REFUSALS, ids=[c[0] for c in REFUSALS])
def test_refused_before_any_launch(lib, name, call, code, msg):
    lib.pm355_last_error.restype = C.c_char_p
    marker = entry(lib, "pm355_mul_mat_vec_q", [i32, vp, vp, i64, i64, vp, i32, vp, i64, vp, vp, vp])
    assert marker(Q4_K, P, None, 4096, 64, P, 0, P, 64, None, None, None) == RANGE      # leaves "ncols must be 1..8": an entry without a text of its own keeps it
    rc = call(lib)
    text = lib.pm355_last_error().decode()
    print(f"{name}: rc {rc} ({code}), {text!r}")
    assert rc == code and (text.startswith(MSG[msg]) if msg == "launch" else text == MSG[msg or "ncols"])


def test_served_lists_pass_the_checks(lib):
    assert grid_or_check("pm355_mul_mat_vec_fused_check", one)(lib) == 0 and grid_or_check("pm355_mul_mat_vec_fused_check", q3())(lib) == 0
    assert grid_or_check("pm355_mul_mat_vec_fused_grid", one)(lib) == 256           # (no device: 256 CUs are assumed)
    assert grid_or_check("pm355_mul_mat_vec_fused_grid", [J(Q6_K, 300000)])(lib) == 1024
    assert qkv_check(q3())(lib) == 0 and qkv_check(q3(), neox=1)(lib) == 0 and qkv_check(q3(mix=(Q6_K, Q4_K, Q4_K)))(lib) == 0
    assert qkv_check(q3(w2=True))(lib) == 0                                         # (the epilogue entries read type, N, W, y and bias of a job: W2 / resid are ignored)
    assert lib_plan(lib, [], 4096, 1) == -9 and lib_plan(lib, one, 4096, 16) == -9   # the plan entry's own arguments: the job-count code, no text


if __name__ == "__main__":                   # test_plan_with_a_switch_off: the forms of SWITCH_CASES under this process's environment, one JSON line
    sys.path.insert(0, ROOT)
    import prima_cpp_amd
    lib_ = prima_cpp_amd.load()
    out_ = [lib_plan(lib_, *c) for c in SWITCH_CASES]
    print(json.dumps([p if isinstance(p, int) else list(p[8]) for p in out_]))
