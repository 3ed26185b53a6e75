"""Which single-token attention form serves a layer in ggml-graph mode (pm_attn_token_plan, prima_cpp_amd/csrc/attn_plan.hip), checked without a GPU
through pm355_attn_token_plan.

The plug-in's planner used to decide this itself (planner::try_attention_block of the commit before this file, the lines from `supported by the
kernels?` to the attention step): parent_rule below restates those lines. The library's plan is compared with it on the full product of GRID - form,
cells and whether scratch is needed. They may differ in ONE case: F16 caches, a shape no long-context form serves (so the score buffer is sized for
n_ctx), and n_ctx == 38392 - 4 * head_dim - (flash-attention layout ? 2048 : 256): the planner's LDS bound ((... + max_keys + 16) * 4 <= 150 KiB) was
one step of 8 cells stricter than the launchers' own (pm_attn_head_lds: ... + max_keys rounded to 8 + 8), so such a layer ran node by node where
pm_launch_attn_rope_fused / pm_launch_attn_cached serve it."""
import ctypes as C
import itertools
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE, ROPE_FUSED, FLASH, SPLIT3, Q8_TOKEN, Q8_LONG, CACHED, CACHED_LONG = range(8)          # PM355_ATTN_FORM_*
V_ROWMAJOR, MASK_F16, K_Q8_0, V_Q8_0 = 1, 2, 4, 8                                           # PM355_ATTN_*

HEADS = [(4, 2), (8, 1), (32, 8), (64, 8), (32, 32), (40, 40), (36, 4), (64, 2), (34, 2)]
DH = [64, 96, 128, 256]
N_CTX = [64, 1024, 32768, 32776, 36080, 36088, 37104, 37112, 37120, 37616, 37624, 37632, 37872, 37880, 37888, 131072]
CACHES = [(False, False, False)] + [(True, k, v) for k in (False, True) for v in (False, True)]      # (fa, k_q8, v_q8): Q8_0 only with fa
SPLIT_MIN = [32, 320]


class PlanIn(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("n_head", "n_head_kv", "head_dim", "n_ctx", "n_kv", "flags", "split_min", "attn_mfma", "rotated_q",
                                         "rope_mode", "rope_n_dims", "scratch", "n_cus")]


class PlanOut(C.Structure):
    _fields_ = [("form", C.c_int32), ("cells", C.c_int32), ("rotated_q", C.c_int32), ("pad_", C.c_int32), ("scratch_floats", C.c_int64)]


def grid():
    """(H, Hkv, dh, n_ctx, n_kv, fa, k_q8, v_q8, split_min, attn_mfma, rotated-q available, n_cus)"""
    for (H, Hkv), dh, n_ctx, (fa, kq8, vq8), sm in itertools.product(HEADS, DH, N_CTX, CACHES, SPLIT_MIN):
        for n_kv in sorted({v for v in (8, sm - 8, sm, sm + 32, n_ctx) if 1 <= v <= n_ctx}):
            for mfma, rot, cus in itertools.product((False, True), (False, True), (256, 32)):
                yield H, Hkv, dh, n_ctx, n_kv, fa, kq8, vq8, sm, mfma, rot, cus


def cached_long_check(H, Hkv, dh, n_ctx, cus):
    """pm355_attn_cached_long_check of the parent (attn_flash_mfma.hip)"""
    if dh not in (64, 128) or Hkv < 1 or H % Hkv or H // Hkv > 16 or n_ctx % 8 or Hkv > 16:
        return False
    return Hkv * min(64, max(16, 256 // Hkv)) <= 2 * cus


def parent_rule(H, Hkv, dh, n_ctx, n_kv, fa, kq8, vq8, split_min, mfma, rot, cus, mode=0, n_dims=None, scratch=True, three_launch=False):
    """try_attention_block of the parent, from `supported by the kernels?` on -> (form, max_keys, scratch needed, no LDS room for n_ctx alone).
    rot: rope_tab && one_launch && pm355_mul_mat_vec_qkv_check_ex(...) == 0 && the table matches - the planner's own facts."""
    n_dims = dh if n_dims is None else n_dims
    q8 = kq8 or vq8
    long_ok = cached_long_check(H, Hkv, dh, n_ctx, cus)
    can_split = dh in (64, 128) and H // Hkv <= 8 and (not q8 or (fa and mfma and long_ok))
    can_fused = dh in (64, 128) or (dh == 256 and not q8)
    split = n_kv >= split_min and can_split and scratch
    max_keys = split_min + 32 if can_split else (32768 if q8 and n_ctx > 32768 else n_ctx)
    if not split and not (can_fused and n_kv <= max_keys and (4 * dh + (2048 if fa else 256) + max_keys + 16) * 4 <= 150 * 1024):
        return NONE, 0, False, can_split
    epi = rot and not q8 and (not split or (mfma and long_ok)) and mode in (0, 2) and n_dims <= 256
    grid_cells = 1024
    while grid_cells < n_kv:
        grid_cells *= 2
    grid_cells = min(grid_cells, n_ctx)
    if epi:
        form = CACHED_LONG if split else CACHED
    elif q8:
        form = Q8_LONG if split else Q8_TOKEN
    else:
        form = (SPLIT3 if three_launch else FLASH) if split else ROPE_FUSED
    return form, grid_cells if split else max_keys, split, can_split


def lib_plan(lib, case, mode=0, n_dims=None, scratch=True):
    H, Hkv, dh, n_ctx, n_kv, fa, kq8, vq8, sm, mfma, rot, cus = case
    flags = (V_ROWMAJOR | MASK_F16 if fa else 0) | (K_Q8_0 if kq8 else 0) | (V_Q8_0 if vq8 else 0)
    i = PlanIn(H, Hkv, dh, n_ctx, n_kv, flags, sm, int(mfma), int(rot), mode, dh if n_dims is None else n_dims, int(scratch), cus)
    o = PlanOut()
    assert lib.pm355_attn_token_plan(C.byref(i), C.byref(o)) == 0
    return o


@pytest.fixture(scope="module")
def lib():
    import prima_cpp_amd
    lib = prima_cpp_amd.load()               # (loads without a GPU, tests/test_abi.py)
    lib.pm355_attn_token_plan.restype = C.c_int
    lib.pm355_attn_token_plan.argtypes = [C.c_void_p, C.c_void_p]
    lib.pm355_attn_split_scratch_floats.restype = C.c_size_t
    return lib


def permitted_difference(case, want, got):
    """the one case of the docstring: the planner said none, the library the per-head form over n_ctx cells"""
    H, Hkv, dh, n_ctx, n_kv, fa, kq8, vq8, sm, mfma, rot, cus = case
    form, _, _, can_split = want
    return (form == NONE and not kq8 and not vq8 and not can_split and n_ctx == 38392 - 4 * dh - (2048 if fa else 256) and
            got.form == (CACHED if rot else ROPE_FUSED) and got.cells == n_ctx and got.scratch_floats == 0 and n_kv <= n_ctx)


def test_plan_is_the_planners_former_rule(lib):
    three_launch = os.environ.get("PM355_ATTN_FLASH", "")[:1] == "0"
    n = 0
    forms, differ = set(), []
    for case in grid():
        n += 1
        want = parent_rule(*case, three_launch=three_launch)
        got = lib_plan(lib, case)
        forms.add(got.form)
        H, Hkv, dh, n_ctx = case[:4]
        floats = lib.pm355_attn_split_scratch_floats(H, dh, n_ctx) if want[2] else 0       # what the planner asked its scratch callback for
        if (got.form, got.cells if got.form else 0, got.scratch_floats) != (want[0], want[1], floats):
            assert permitted_difference(case, want, got), (case, want, (got.form, got.cells, got.scratch_floats))
            differ.append(case)
        assert got.rotated_q == int(got.form in (CACHED, CACHED_LONG))
    print(f"{n} cases, {len(differ)} take a per-head form where the planner had none: {sorted({(c[2], c[3], c[5]) for c in differ})} (dh, n_ctx, fa)")
    assert n == 224640
    assert differ
    assert forms == ({NONE, ROPE_FUSED, SPLIT3 if three_launch else FLASH, Q8_TOKEN, Q8_LONG, CACHED, CACHED_LONG})


def test_restated_rule_reaches_every_form():
    forms = {parent_rule(*case)[0] for case in grid()}
    assert forms == {NONE, ROPE_FUSED, FLASH, Q8_TOKEN, Q8_LONG, CACHED, CACHED_LONG}


SUBGRID = [c for c in grid() if c[3] in (1024, 37112, 131072) and c[11] == 256]


@pytest.mark.parametrize("mode,n_dims", [(1, None), (4, None), (8, None), (10, None), (0, 258), (2, 512)])
def test_no_rotated_rows_from_a_rotation_the_table_does_not_hold(lib, mode, n_dims):
    """RoPE modes other than NORM (0) / NEOX (2), or more than 256 rotated dimensions: the plan never asks for rotated q, whatever the caller offers"""
    asked = 0
    for case in SUBGRID:
        got = lib_plan(lib, case, mode=mode, n_dims=n_dims)
        raw = lib_plan(lib, case[:10] + (False,) + case[11:], mode=mode, n_dims=n_dims)
        assert not got.rotated_q and got.form not in (CACHED, CACHED_LONG), (case, got.form)
        assert (got.form, got.cells, got.scratch_floats) == (raw.form, raw.cells, raw.scratch_floats), case
        asked += case[10] and lib_plan(lib, case).rotated_q
    assert asked > 100                       # (the same cases with a rotation the table holds do take rotated rows)


def test_no_scratch_no_long_form(lib):
    """a caller without scratch memory gets the planner's answer for a failed allocation: the per-head form where split_min + 32 cells hold n_kv, else none"""
    long_forms = 0
    for case in SUBGRID:
        want = parent_rule(*case, scratch=False)
        got = lib_plan(lib, case, scratch=False)
        if not permitted_difference(case, want, got):
            assert (got.form, got.cells if got.form else 0, got.scratch_floats) == (want[0], want[1], 0), (case, want, got.form)
        long_forms += lib_plan(lib, case).scratch_floats > 0
    assert long_forms > 100


def test_three_launch_switch_turns_flash_into_split3_and_nothing_else(lib):
    """PM355_ATTN_FLASH is read once per process: a process of its own plans the grid with PM355_ATTN_FLASH=0 (this one's answers, FLASH read as SPLIT3)"""
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=dict(os.environ, PM355_ATTN_FLASH="0"), cwd=ROOT, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    got = r.stdout.splitlines()[-1].split(";")
    here = []
    for case in grid():
        o = lib_plan(lib, case)
        here.append(f"{SPLIT3 if o.form == FLASH else o.form},{o.cells},{o.scratch_floats}")
    assert len(got) == len(here) == 224640
    assert got == here
    assert sum(g.startswith(f"{SPLIT3},") for g in got) > 1000


if __name__ == "__main__":                   # the child of the test above
    sys.path.insert(0, ROOT)
    import prima_cpp_amd
    lib_ = prima_cpp_amd.load()
    lib_.pm355_attn_token_plan.restype = C.c_int
    lib_.pm355_attn_token_plan.argtypes = [C.c_void_p, C.c_void_p]
    out = []
    for case_ in grid():
        o_ = lib_plan(lib_, case_)
        out.append(f"{o_.form},{o_.cells},{o_.scratch_floats}")
    print(";".join(out))
