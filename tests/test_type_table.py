"""The per-type table (prima_cpp_amd/csrc/pm355_types.h, prima_cpp_amd/gguf.py): row bytes and HBM row strides of every stored weight type,
from the built library, against the block layouts as documented (ggml/src/ggml-common.h; repack.hip for the row-SoA strides) written out
here once more as literals, and against the bytes the reference actually produced (the golden fixtures). Host arithmetic only: no GPU."""
import os

import numpy as np
import pytest

import prima_cpp_amd
from prima_cpp_amd import gguf as G
from _bind import TYPE_NAMES, Ref, have_ref

F32, F16, Q5_0, Q8_0, Q4_K, Q5_K, Q6_K, Q8_K = 0, 1, 6, 8, 12, 13, 14, 15
# values per block, bytes per block = the sum of the block's fields
LAYOUT = {
    F32: (1, 4),
    F16: (1, 2),
    Q5_0: (32, 2 + 4 + 16),                    # half d | u8 qh[4] | u8 qs[16]
    Q8_0: (32, 2 + 32),                        # half d | i8 qs[32]
    Q4_K: (256, 2 + 2 + 12 + 128),             # half d | half dmin | u8 scales[12] | u8 qs[128]
    Q5_K: (256, 2 + 2 + 12 + 32 + 128),        # half d | half dmin | u8 scales[12] | u8 qh[32] | u8 qs[128]
    Q6_K: (256, 128 + 64 + 16 + 2),            # u8 ql[128] | u8 qh[64] | i8 scales[16] | half d
}
# 96 / 2304 / 768: rows whose fp16 scale stream (and, Q5_0 at 96, the high-bit stream) does not end on a 16-byte boundary
KS = {1: (96, 256, 4096, 8192, 28672, 29568), 32: (96, 256, 2304, 4096, 8192, 28672, 29568), 256: (256, 768, 2304, 4096, 8192, 28672)}


def _up16(n):
    return (n + 15) // 16 * 16


def _stride(t, K):
    """HBM row stride: the row-SoA layouts pad their trailing stream(s) to 16 bytes, everything else keeps the GGUF row."""
    nb = K // LAYOUT[t][0]
    if t == Q8_0:
        return nb * 32 + _up16(nb * 2)                         # qa[nb][16] | qb[nb][16] | d[nb]
    if t == Q5_0:
        return nb * 16 + _up16(nb * 4) + _up16(nb * 2)         # qs[nb][16] | qh[nb][4] | d[nb]
    if t == Q6_K:
        return _up16(nb * 210)                                 # la | lb | qh (64 B per block each) | scales[nb][16] | d[nb]
    return nb * LAYOUT[t][1]


@pytest.fixture(scope="module")
def lib():
    return prima_cpp_amd.load()              # (loads without a GPU, tests/test_abi.py; lib.py declares the two signatures)


def test_python_table_is_the_documented_layout():
    assert {t: G.BLOCK[t] for t in LAYOUT} == LAYOUT and G.BLOCK[Q8_K] == (256, 4 + 256 + 2 * 16)
    assert (G.F32, G.F16, G.Q5_0, G.Q8_0, G.Q4_K, G.Q5_K, G.Q6_K, G.Q8_K) == (F32, F16, Q5_0, Q8_0, Q4_K, Q5_K, Q6_K, Q8_K)
    import _bind
    from prima_cpp_amd import lib as L
    assert _bind.BLOCK is G.BLOCK and _bind.row_size is G.row_size and L.row_size is G.row_size and L.Q8_K == 15


@pytest.mark.parametrize("t", sorted(LAYOUT))
def test_row_size_and_stride(lib, t):
    per, bs = LAYOUT[t]
    for K in KS[per]:
        want = K // per * bs
        size, stride = lib.pm355_row_size(t, K), lib.pm355_row_stride(t, K)
        print(f"type {t} K {K}: row {size} (table {G.row_size(t, K)}, layout {want}), stride {stride} (layout {_stride(t, K)})")
        assert size == want == G.row_size(t, K)
        assert stride == _stride(t, K) and stride >= size
        assert stride % 16 == 0 or stride == size


def test_strides_are_the_recorded_ones(lib):
    """What the library answered before the table existed (recorded from that build)."""
    recorded = {(Q5_0, 96): 80, (Q5_0, 29568): 20336, (Q8_0, 96): 112, (Q8_0, 4096): 4352, (Q8_0, 29568): 31424, (Q6_K, 768): 640,
                (Q6_K, 2304): 1904, (Q6_K, 8192): 6720, (Q6_K, 28672): 23520, (Q4_K, 2304): 1296, (Q5_K, 2304): 1584, (F32, 96): 384, (F16, 96): 192}
    for (t, K), want in recorded.items():
        assert lib.pm355_row_stride(t, K) == want == _stride(t, K), (t, K)
    # types the library does not store: no row, no stride
    for t in (-1, 2, 7, Q8_K, 16, 40):
        assert lib.pm355_row_size(t, 4096) == 0 and lib.pm355_row_stride(t, 4096) == 0, t


def test_row_size_is_what_the_reference_wrote(lib):
    """The golden fixtures hold blocks the reference quantized: 4 rows of K = 1024 per type, and the tiny models' tensors."""
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    ops = np.load(os.path.join(gold, "ops_golden.npz"))
    for t in (Q4_K, Q5_K, Q6_K, Q8_0):
        for tag in ("quantized", "random"):
            assert ops[f"w_{TYPE_NAMES[t]}_{tag}"].nbytes == 4 * lib.pm355_row_size(t, 1024), (t, tag)
    z = np.load(os.path.join(gold, "tiny_llama_decode.npz"))
    E, F, V = int(z["hp_n_embd"]), int(z["hp_n_ff"]), int(z["hp_n_vocab"])
    for key, K, N in (("attn_norm_0", E, 1), ("wq_0", E, E), ("wv_0", E, None), ("wv_1", E, None), ("ffn_down_0", F, E), ("tok_embd", E, V), ("output", E, V)):
        t, nbytes = int(z[f"y_{key}"]), z[f"t_{key}"].nbytes
        rs = lib.pm355_row_size(t, K)
        assert rs and nbytes % rs == 0 and (N is None or nbytes == N * rs), (key, t, nbytes, rs)
    if have_ref():                           # Q5_0 has no committed fixture: the reference's own quantizer, where it is built
        ref = Ref()
        for t in (Q5_0, Q8_0, Q4_K, Q5_K, Q6_K):
            K = 96 if LAYOUT[t][0] < 256 else 768
            assert ref.quantize_weights(t, np.ones((3, K), np.float32)).size == 3 * lib.pm355_row_size(t, K), t
