"""What the six single-token attention entry points of the C ABI refuse BEFORE anything is launched: the return code and the pm355_last_error text
of each case, recorded from the build in front of the one that gave the launchers their common argument block (pm_attn_tok, pm355_layer_ops.h).
Host checks only: no GPU, every pointer is a dummy that is never dereferenced - so every case here must be refused on its own grounds, with or
without a device.

Left out, because the entry point has no such check and would launch (that is its behaviour, and it stays):
  pm355_attn_decode        head_dim 96 (served: any multiple of 8), null pointers (not checked)
  pm355_attn_decode_split  null q / out (only the scratch is checked)
  pm355_attn_rope_fused    null q / k / v / out (not checked); it has no max_keys: the LDS case is an n_ctx of 40000
  pm355_attn_token, Q8_0   n_ctx % 8 != 0 (the Q8_0 one-workgroup-per-head kernel does not ask for it)
No entry point reaches the HIP runtime in front of these checks in a way that matters without a device (pm355_attn_token clears the runtime's
sticky error first, and pm355_attn_cached_long asks for the CU count: both just fail quietly), so all six have cases here."""
import ctypes as C
import os

import pytest

import prima_cpp_amd
from prima_cpp_amd.ops import ATTN_K_Q8_0, ATTN_MASK_F16, ATTN_V_Q8_0, ATTN_V_ROWMAJOR, AttnTokenArgs, RopeParams

UNSUPPORTED, SHAPE, RANGE = -1, -2, -4
P = 4096                                     # a non-null pointer nobody follows
H, HKV, NCTX, SCALE = 4, 2, 1088, 0.125

MSG = {
    "decode": "attn_decode: n_ctx/head_dim unsupported (LDS budget 150 KB, multiples of 8)",
    "split": "attn_decode_split: head_dim 64/128, at most 8 query heads per KV head, n_ctx % 8 == 0, scratch required",
    "fused": "attn_rope_fused: head_dim must be 64/128/256, n_ctx % 8 == 0 and fit LDS",
    "fused_rp": "attn_rope_fused: n_dims",
    "cached": "attn_cached: head_dim must be 64/128/256, n_ctx % 8 == 0 and max_keys fit LDS",
    "cached_null": "attn_cached: null pointer",
    "long": "attn_cached_long: head_dim must be 64/128, <= 16 query heads per KV head, n_ctx % 8 == 0; Q8_0 caches need row-major V",
    "long_null": "attn_cached_long: null pointer",
    "long_flag": "attn_cached_long: unknown flag",
    "tok": "attn_token: head_dim must be 64/128/256, n_ctx % 8 == 0 and max_keys fit LDS",
    "tok_rp": "attn_token: n_dims",
    "tok_null": "attn_token: null pointer",
    "tok_q8_layout": "attn_token: a quantized KV cache needs row-major V (flash-attention graphs)",
    "tok_q8": "attn_token(q8_0): head_dim 64/128 and max_keys must fit LDS",
    "tok_q8_scratch": "attn_token(q8_0, long): scratch",
    "tok_flash": "attn_token(flash): head_dim 64/128, at most 8 query heads per KV head, n_ctx % 8 == 0, scratch required",
    "tok_split": "attn_token(split): head_dim 64/128, at most 8 query heads per KV head, n_ctx % 8 == 0, scratch required",
}
# PM355_ATTN_FLASH=0 (read once by the library) sends the long-context token to the three-launch form, which refuses in its own words
TOK_LONG = "tok_split" if os.environ.get("PM355_ATTN_FLASH", "")[:1] == "0" else "tok_flash"
Q8 = ATTN_K_Q8_0 | ATTN_V_ROWMAJOR


def _rp(n_dims=64):
    return RopeParams(n_dims, 0, 8192, 10000.0, 1.0, 0.0, 1.0, 32.0, 1.0)


def decode(dh=64, n_ctx=NCTX):
    return lambda lib: lib.pm355_attn_decode(P, P, P, P, P, 1, H, HKV, dh, n_ctx, SCALE, None)


def decode_split(dh=64, n_ctx=NCTX, scratch=P, hkv=HKV, h=H):
    def call(lib):
        lib.pm355_attn_decode_split.restype = C.c_int
        lib.pm355_attn_decode_split.argtypes = [C.c_void_p] * 6 + [C.c_int] * 4 + [C.c_float, C.c_void_p]
        return lib.pm355_attn_decode_split(P, P, P, P, P, scratch, h, hkv, dh, n_ctx, SCALE, None)
    return call


def rope_fused(dh=64, n_ctx=NCTX, rp=True, n_dims=64):
    def call(lib):
        r = _rp(n_dims)
        return lib.pm355_attn_rope_fused(P, P, P, P, P, P, None, P, H, HKV, dh, n_ctx, SCALE, C.addressof(r) if rp else None, None)
    return call


def cached(dh=64, n_ctx=NCTX, out=P, max_keys=0, flags=0):
    def call(lib):
        lib.pm355_attn_cached.restype = C.c_int
        lib.pm355_attn_cached.argtypes = [C.c_void_p] * 7 + [C.c_int] * 4 + [C.c_float, C.c_int, C.c_int, C.c_void_p]
        return lib.pm355_attn_cached(P, P, P, P, None, None, out, H, HKV, dh, n_ctx, SCALE, max_keys, flags, None)
    return call


def cached_long(dh=64, n_ctx=NCTX, out=P, scratch=P, flags=0, h=H):
    def call(lib):
        lib.pm355_attn_cached_long.restype = C.c_int
        lib.pm355_attn_cached_long.argtypes = [C.c_void_p] * 8 + [C.c_int] * 4 + [C.c_float, C.c_int, C.c_int, C.c_void_p]
        return lib.pm355_attn_cached_long(P, P, P, P, None, None, out, scratch, h, HKV, dh, n_ctx, SCALE, 0, flags, None)
    return call


def token(dh=64, n_ctx=NCTX, out=P, scratch=None, split=0, max_keys=0, flags=0, n_dims=64, args=True):
    def call(lib):
        lib.pm355_attn_token.restype = C.c_int
        lib.pm355_attn_token.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        a = AttnTokenArgs(P, P, P, P, P, P, P, None, None, out, scratch, H, HKV, dh, n_ctx, split, max_keys, SCALE, flags)
        r = _rp(n_dims)
        return lib.pm355_attn_token(C.addressof(a) if args else None, C.addressof(r), None)
    return call


CASES = [
    ("decode: n_ctx % 8", decode(n_ctx=1004), RANGE, "decode"),
    ("decode: head_dim % 8", decode(dh=100), RANGE, "decode"),
    ("decode: scores beyond LDS", decode(dh=128, n_ctx=40000), RANGE, "decode"),
    ("decode_split: head_dim 96", decode_split(dh=96), RANGE, "split"),
    ("decode_split: n_ctx % 8", decode_split(n_ctx=1004), RANGE, "split"),
    ("decode_split: no scratch", decode_split(scratch=None), RANGE, "split"),
    ("decode_split: 16 query heads per KV head", decode_split(h=16, hkv=1), RANGE, "split"),
    ("rope_fused: no rope parameters", rope_fused(rp=False), SHAPE, "fused_rp"),
    ("rope_fused: odd n_dims", rope_fused(n_dims=63), SHAPE, "fused_rp"),
    ("rope_fused: n_dims > head_dim", rope_fused(n_dims=128), SHAPE, "fused_rp"),
    ("rope_fused: head_dim 96", rope_fused(dh=96), UNSUPPORTED, "fused"),
    ("rope_fused: n_ctx % 8", rope_fused(n_ctx=1004), UNSUPPORTED, "fused"),
    ("rope_fused: scores beyond LDS", rope_fused(dh=128, n_ctx=40000), UNSUPPORTED, "fused"),
    ("cached: null out", cached(out=None), SHAPE, "cached_null"),
    ("cached: head_dim 96", cached(dh=96), UNSUPPORTED, "cached"),
    ("cached: n_ctx % 8", cached(n_ctx=1004), UNSUPPORTED, "cached"),
    ("cached: max_keys beyond LDS", cached(dh=128, n_ctx=65536, max_keys=40000), UNSUPPORTED, "cached"),
    ("cached: max_keys beyond LDS, row-major V", cached(dh=128, n_ctx=65536, max_keys=37500, flags=ATTN_V_ROWMAJOR), UNSUPPORTED, "cached"),
    ("cached_long: null out", cached_long(out=None), SHAPE, "long_null"),
    ("cached_long: null scratch", cached_long(scratch=None), SHAPE, "long_null"),
    ("cached_long: unknown flag", cached_long(flags=16), UNSUPPORTED, "long_flag"),
    ("cached_long: unknown flag beside known ones", cached_long(flags=32 | ATTN_V_ROWMAJOR | ATTN_MASK_F16), UNSUPPORTED, "long_flag"),
    ("cached_long: head_dim 96", cached_long(dh=96), UNSUPPORTED, "long"),
    ("cached_long: n_ctx % 8", cached_long(n_ctx=1004), UNSUPPORTED, "long"),
    ("cached_long: 32 query heads per KV head", cached_long(h=64), UNSUPPORTED, "long"),
    ("cached_long: Q8_0 K cache, transposed V", cached_long(flags=ATTN_K_Q8_0), UNSUPPORTED, "long"),
    ("cached_long: Q8_0 V cache, transposed V", cached_long(flags=ATTN_V_Q8_0), UNSUPPORTED, "long"),
    ("token: no arguments", token(args=False), SHAPE, "tok_rp"),
    ("token: odd n_dims", token(n_dims=63), SHAPE, "tok_rp"),
    ("token: null out", token(out=None), SHAPE, "tok_null"),
    ("token: head_dim 96", token(dh=96, n_dims=32), UNSUPPORTED, "tok"),
    ("token: n_ctx % 8", token(n_ctx=1004), UNSUPPORTED, "tok"),
    ("token: max_keys beyond LDS", token(dh=128, n_ctx=65536, max_keys=40000), UNSUPPORTED, "tok"),
    ("token: Q8_0 K cache, transposed V", token(flags=ATTN_K_Q8_0), UNSUPPORTED, "tok_q8_layout"),
    ("token: Q8_0 V cache, transposed V, F16 mask", token(flags=ATTN_V_Q8_0 | ATTN_MASK_F16), UNSUPPORTED, "tok_q8_layout"),
    ("token: Q8_0, head_dim 96", token(dh=96, n_dims=32, flags=Q8), UNSUPPORTED, "tok_q8"),
    ("token: Q8_0, max_keys beyond LDS", token(dh=128, n_ctx=65536, max_keys=40000, flags=Q8), UNSUPPORTED, "tok_q8"),
    ("token: Q8_0, long context without scratch", token(split=1, flags=Q8), SHAPE, "tok_q8_scratch"),
    ("token: long context without scratch", token(split=1), UNSUPPORTED, TOK_LONG),
    ("token: long context, head_dim 256", token(dh=256, split=1, scratch=P), UNSUPPORTED, TOK_LONG),
    ("token: long context, n_ctx % 8", token(n_ctx=1004, split=1, scratch=P), UNSUPPORTED, TOK_LONG),
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
