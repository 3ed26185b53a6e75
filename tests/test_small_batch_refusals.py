"""What the small-batch mat-mul's entry points of the C ABI refuse BEFORE anything is launched: the return code and the pm355_last_error text of each
case, recorded from the build in front of the one that gave the three launchers their common job-list entry (pm_launch_mmq_i8, pm355_kernels.h).
Host checks only: no GPU, every pointer is a dummy that is never dereferenced - so every case here must be refused on its own grounds, with or
without a device. pm355_mul_mat_q_small_check answers PM355_E_UNSUPPORTED for every shape it does not serve and leaves no text.

No case of the list had to be left out: every one is refused in front of the first device call (pm355_mul_mat_q_small and its siblings clear the
runtime's sticky error first, which fails quietly without a device)."""
import ctypes as C

import pytest

import prima_cpp_amd

UNSUPPORTED, SHAPE, RANGE = -1, -2, -4
P = 4096                                     # a non-null pointer nobody follows
Q4_0, Q8_0, Q4_K, Q5_K, Q6_K = 2, 8, 12, 13, 14

MSG = {
    "type": "mul_mat_q_small: weight type (Q4_K / Q5_K / Q6_K / Q8_0)",
    "shape": "mul_mat_q_small: 1 <= n_tokens <= 64, K % 256 == 0 (Q8_0: K % 32 == 0), K >= 512 required",
    "lds": "mul_mat_q_small: K too large for the LDS tiles",
    "no_x": "mul_mat_q_small: neither xq nor x given",
    "multi_args": "mul_mat_q_small_multi: 2..3 jobs, pre-quantized activations",
    "multi": "mul_mat_q_small_multi: Q4_K / Q6_K, n_tokens <= 64, K % 256 == 0 required",
    "mixed_args": "mul_mat_q_small_mixed: 2..3 jobs, pre-quantized activations",
    "mixed_mid": "mul_mat_q_small_mixed: only the LAST job may be of another type",
    "mixed": "mul_mat_q_small_mixed: Q4_K jobs + one Q6_K (n_tokens <= 32) / Q5_K (<= 16) job, K % 256 == 0 required",
}


def small(t=Q4_K, K=4096, N=64, T=8, xq=P, x=None):
    def call(lib):
        lib.pm355_mul_mat_q_small.restype = C.c_int
        lib.pm355_mul_mat_q_small.argtypes = [C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64] + [C.c_void_p] * 4
        return lib.pm355_mul_mat_q_small(t, P, K, N, xq, x, T, P, None, None, None)
    return call


def _lists(n, N):
    W, y = (C.c_void_p * 4)(*([P] * 4)), (C.c_void_p * 4)(*([P] * 4))
    Ns = (C.c_int64 * 4)(*([N] * 4))
    return W, Ns, y


def multi(t=Q4_K, n=3, K=4096, N=64, T=8, xq=P):
    def call(lib):
        lib.pm355_mul_mat_q_small_multi.restype = C.c_int
        lib.pm355_mul_mat_q_small_multi.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 5 + [C.c_int64, C.c_int64, C.c_void_p]
        W, Ns, y = _lists(n, N)
        return lib.pm355_mul_mat_q_small_multi(t, n, W, Ns, y, None, xq, K, T, None)
    return call


def mixed(types=(Q4_K, Q4_K, Q6_K), K=4096, N=64, T=8, xq=P):
    def call(lib):
        lib.pm355_mul_mat_q_small_mixed.restype = C.c_int
        lib.pm355_mul_mat_q_small_mixed.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 5 + [C.c_int64, C.c_int64, C.c_void_p]
        W, Ns, y = _lists(len(types), N)
        ts = (C.c_int * 4)(*(list(types) + [0] * (4 - len(types))))
        return lib.pm355_mul_mat_q_small_mixed(ts, len(types), W, Ns, y, None, xq, K, T, None)
    return call


# (name, what the single-matrix entry is asked, code, text, the same shape through pm355_mul_mat_q_small_check)
SMALL = [
    ("unserved type", dict(t=Q4_0), UNSUPPORTED, "type"),
    ("K % 256", dict(K=4096 + 64), SHAPE, "shape"),
    ("Q8_0: K % 32", dict(t=Q8_0, K=29568 + 16), SHAPE, "shape"),
    ("K < 512", dict(K=256), SHAPE, "shape"),
    ("Q8_0: K < 512", dict(t=Q8_0, K=256), SHAPE, "shape"),
    ("no tokens", dict(T=0), SHAPE, "shape"),
    ("65 tokens", dict(T=65), SHAPE, "shape"),
    ("no rows", dict(N=0), SHAPE, "shape"),
    ("tiles beyond LDS", dict(t=Q6_K, K=65536), RANGE, "lds"),
]
CASES = [("small: " + n, small(**kw), code, msg) for n, kw, code, msg in SMALL] + [
    ("small: neither xq nor x", small(xq=None), RANGE, "no_x"),
    ("multi: one job", multi(n=1), RANGE, "multi_args"),
    ("multi: four jobs", multi(n=4), RANGE, "multi_args"),
    ("multi: null xq", multi(xq=None), RANGE, "multi_args"),
    ("multi: a Q5_K list", multi(t=Q5_K), UNSUPPORTED, "multi"),
    ("multi: a Q8_0 list", multi(t=Q8_0), UNSUPPORTED, "multi"),
    ("multi: 65 tokens", multi(T=65), UNSUPPORTED, "multi"),
    ("multi: K % 256", multi(K=4096 + 64), UNSUPPORTED, "multi"),
    ("mixed: one job", mixed(types=(Q4_K,)), RANGE, "mixed_args"),
    ("mixed: null xq", mixed(xq=None), RANGE, "mixed_args"),
    ("mixed: first type other than Q4_K", mixed(types=(Q6_K, Q6_K, Q5_K)), UNSUPPORTED, "mixed"),
    ("mixed: last type equal to the first", mixed(types=(Q4_K, Q4_K, Q4_K)), UNSUPPORTED, "mixed"),
    ("mixed: two Q6_K jobs", mixed(types=(Q6_K, Q6_K)), UNSUPPORTED, "mixed"),
    ("mixed: differing middle type", mixed(types=(Q4_K, Q6_K, Q6_K)), UNSUPPORTED, "mixed_mid"),
    ("mixed: 33 tokens with Q6_K", mixed(T=33), UNSUPPORTED, "mixed"),
    ("mixed: 17 tokens with Q5_K", mixed(types=(Q4_K, Q4_K, Q5_K), T=17), UNSUPPORTED, "mixed"),
    ("mixed: last job Q8_0", mixed(types=(Q4_K, Q4_K, Q8_0)), UNSUPPORTED, "mixed"),
]


@pytest.fixture(scope="module")
def lib():
    return prima_cpp_amd.load()              # (loads without a GPU, tests/test_abi.py)


@pytest.mark.parametrize("name,call,code,msg", CASES, ids=[c[0] for c in CASES])
def test_refused_before_any_launch(lib, name, call, code, msg):
    rc = call(lib)
    text = lib.pm355_last_error().decode()
    print(f"{name}: rc {rc} ({code}), {text!r}")
    assert rc == code and text == MSG[msg]


@pytest.mark.parametrize("name,kw", [(n, kw) for n, kw, _, _ in SMALL], ids=[c[0] for c in SMALL])
def test_shape_check_refuses_the_same_shapes(lib, name, kw):
    a = dict(t=Q4_K, K=4096, N=64, T=8)
    a.update(kw)
    chk = lib.pm355_mul_mat_q_small_check
    chk.restype = C.c_int
    chk.argtypes = [C.c_int, C.c_int64, C.c_int64, C.c_int64]
    assert chk(Q4_K, 4096, 64, 8) == 0
    assert chk(a["t"], a["K"], a["N"], a["T"]) == UNSUPPORTED
