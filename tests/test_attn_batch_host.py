"""Host side of the multi-token attention and of the long-context scratch, checked without a GPU (every pointer is a dummy nobody follows).

1. What pm355_attn_prefill and pm355_attn_prefill_masked_ex refuse BEFORE anything is launched: return code and pm355_last_error text of each
   case, recorded from the build in front of the one that gave the launcher its argument block (pm_attn_batch, pm355_layer_ops.h).
2. The scratch layout of the long-context forms (pm_attn_flash_layout, pm355_layer_ops.h; read through pm355_attn_long_scratch_layout): the literals
   are the values of the formulas that stood in attn_flash.hip (launcher, pm_attn_flash_scratch_floats, pm_attn_flash_qrot_offset), attn_flash_mfma.hip
   (tickets at + Hkv + 16) and attn_split.hip / c_api.hip (the total of pm355_attn_split_scratch_floats, taken with n_head_kv = n_head) in front of it."""
import ctypes as C

import pytest

import prima_cpp_amd
from prima_cpp_amd.ops import ATTN_MASK_F16, ATTN_V_ROWMAJOR

UNSUPPORTED, SHAPE, RANGE = -1, -2, -4
P = 4096                                     # a non-null pointer nobody follows
H, HKV, SCALE = 4, 2, 0.125
MSG = {
    "prefill": "attn_prefill: head_dim must be 64 or 128 and n_ctx a multiple of 32",
    "masked": "attn_prefill_masked: head_dim 64/128, n_ctx % 32 == 0, n_kv % 4 == 0 <= n_ctx required",
    "masked_null": "attn_prefill_masked: mask required",
    "prefill_ptr": "attn_prefill: null pointer",
    "masked_ptr": "attn_prefill_masked: null pointer",
}


def prefill(dh=64, n_ctx=1024, n_tok=8, pos=P, out=P):
    def call(lib):
        lib.pm355_attn_prefill.restype = C.c_int
        lib.pm355_attn_prefill.argtypes = [C.c_void_p] * 5 + [C.c_int] * 5 + [C.c_float, C.c_void_p]
        return lib.pm355_attn_prefill(P, P, P, pos, out, n_tok, H, HKV, dh, n_ctx, SCALE, None)
    return call


def masked(dh=64, n_ctx=1024, n_tok=8, mask=P, mask_stride=1024, n_kv=256, flags=0, out=P):
    def call(lib):
        lib.pm355_attn_prefill_masked_ex.restype = C.c_int
        lib.pm355_attn_prefill_masked_ex.argtypes = [C.c_void_p] * 4 + [C.c_int64, C.c_void_p] + [C.c_int] * 6 + [C.c_float, C.c_int, C.c_void_p]
        return lib.pm355_attn_prefill_masked_ex(P, P, P, mask, mask_stride, out, n_tok, H, HKV, dh, n_ctx, n_kv, SCALE, flags, None)
    return call


CASES = [
    ("prefill: head_dim 96", prefill(dh=96), RANGE, "prefill"),
    ("prefill: n_ctx % 32", prefill(n_ctx=1032), RANGE, "prefill"),
    ("prefill: n_tokens 0", prefill(n_tok=0), RANGE, "prefill"),
    ("masked: head_dim 96", masked(dh=96), RANGE, "masked"),
    ("masked: n_ctx % 32", masked(n_ctx=1032), RANGE, "masked"),
    ("masked: n_tokens 0", masked(n_tok=0), RANGE, "masked"),
    ("masked: null mask", masked(mask=None), SHAPE, "masked_null"),
    ("masked: n_kv 0", masked(n_kv=0), RANGE, "masked"),
    ("masked: n_kv beyond n_ctx", masked(n_kv=1028), RANGE, "masked"),
    ("masked: n_kv % 4", masked(n_kv=254), RANGE, "masked"),
    ("masked: mask_stride % 4", masked(mask_stride=1022), RANGE, "masked"),
    ("masked: mask_stride % 4, flash-attention layout", masked(mask_stride=1022, flags=ATTN_V_ROWMAJOR | ATTN_MASK_F16), RANGE, "masked"),
]
# The mode rule of pm_attn_batch (exactly one of out / out_f16, exactly one of pos / mask) as far as the C ABI can break it: a served shape with neither
# positions nor a mask, or with no output. The build in front launched these and followed the null pointer; they are refused in words of their own.
# (Both outputs, positions AND a mask, seq without positions: no C entry can ask for them - the engine's builder and these two entries are the only callers.)
MODE_CASES = [
    ("prefill: neither positions nor mask", prefill(pos=None), SHAPE, "prefill_ptr"),
    ("prefill: no output", prefill(out=None), SHAPE, "prefill_ptr"),
    ("masked: no output", masked(out=None), SHAPE, "masked_ptr"),
]


@pytest.fixture(scope="module")
def lib():
    return prima_cpp_amd.load()              # (loads without a GPU, tests/test_abi.py)


@pytest.mark.parametrize("name,call,code,msg", CASES, ids=[c[0] for c in CASES])
def test_batch_attention_refused_before_any_launch(lib, name, call, code, msg):
    rc = call(lib)
    text = lib.pm355_last_error().decode()
    print(f"{name}: rc {rc} ({code}), {text!r}")
    assert rc == code and text == MSG[msg]


@pytest.mark.parametrize("name,call,code,msg", MODE_CASES, ids=[c[0] for c in MODE_CASES])
def test_batch_attention_mode_refused_before_any_launch(lib, name, call, code, msg):
    rc = call(lib)
    text = lib.pm355_last_error().decode()
    print(f"{name}: rc {rc} ({code}), {text!r}")
    assert rc == code and text == MSG[msg]


# (n_head, n_head_kv, head_dim, n_ctx) -> spans | M | L | P | tickets of attn_flash | tickets of attn_flash_mfma | query rows | total, then
# pm355_attn_split_scratch_floats(n_head, head_dim, n_ctx). (4, 1, 64, 136): a short context, two spans
LAYOUTS = {
    (64, 8, 128, 32768): ((256, 0, 16384, 32768, 2129920, 2129944, 2130056, 2138248), 4227072),
    (8, 2, 64, 1088): ((9, 0, 72, 144, 4752, 4770, 4882, 5394), 13456),
    (16, 16, 128, 8192): ((64, 0, 1024, 2048, 133120, 133152, 133264, 135312), 264192),
    (4, 1, 64, 136): ((2, 0, 8, 16, 528, 545, 657, 913), 1072),
}


def layout(lib, shape):
    f = lib.pm355_attn_long_scratch_layout
    f.restype, f.argtypes = C.c_int, [C.c_int] * 4 + [C.c_void_p, C.c_int]
    out = (C.c_int64 * 8)()
    assert f(*shape, out, 8) == 0
    return tuple(out)


@pytest.mark.parametrize("shape", list(LAYOUTS), ids=[str(s) for s in LAYOUTS])
def test_long_context_scratch_layout_is_the_recorded_one(lib, shape):
    want, want_total = LAYOUTS[shape]
    got = layout(lib, shape)
    lib.pm355_attn_split_scratch_floats.restype = C.c_size_t
    lib.pm355_attn_split_scratch_floats.argtypes = [C.c_int] * 3
    total = lib.pm355_attn_split_scratch_floats(shape[0], shape[2], shape[3])
    print(shape, got, total)
    assert got == want and total == want_total
    # what a C-ABI caller allocates (no n_head_kv: taken as n_head) holds the layout of every n_head_kv <= n_head
    assert total >= got[7] and total >= layout(lib, (shape[0], shape[0], shape[2], shape[3]))[7]


@pytest.mark.parametrize("shape", list(LAYOUTS), ids=[str(s) for s in LAYOUTS])
def test_long_context_scratch_regions_do_not_overlap(lib, shape):
    n_head, n_head_kv, dh, _ = shape
    nspan, m, l, p, tk, tk_mfma, qrot, total = layout(lib, shape)
    regions = [("M", m, n_head * nspan), ("L", l, n_head * nspan), ("P", p, nspan * n_head * dh), ("tickets", tk, n_head_kv),
               ("tickets_mfma", tk_mfma, 32), ("qrot", qrot, n_head * dh)]
    end = 0
    for name, at, n in regions:                     # in address order: each starts at or behind the end of the one in front, the last ends at the total
        print(name, at, at + n)
        assert at >= end, name
        end = at + n
    assert end <= total


def test_long_context_scratch_layout_refuses_a_short_buffer(lib):
    f = lib.pm355_attn_long_scratch_layout
    f.restype, f.argtypes = C.c_int, [C.c_int] * 4 + [C.c_void_p, C.c_int]
    out = (C.c_int64 * 8)()
    assert f(8, 2, 64, 1088, out, 7) == SHAPE and f(8, 2, 64, 1088, None, 8) == SHAPE


def test_long_context_check_without_a_device(lib):
    """pm355_attn_cached_long_check refuses on the shape alone, whatever the device's CU count"""
    f = lib.pm355_attn_cached_long_check
    f.restype, f.argtypes = C.c_int, [C.c_int] * 4
    assert f(8, 2, 96, 1088) == UNSUPPORTED and f(8, 2, 64, 1084) == UNSUPPORTED and f(64, 2, 64, 1088) == UNSUPPORTED and f(32, 32, 128, 4096) == UNSUPPORTED
