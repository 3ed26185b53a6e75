"""Q5_0 weights: the reference's fallback for Q4_K rows that are no multiple of 256 (llama_tensor_get_type, src/llama.cpp:19516-19548).
Qwen2.5-72B's n_ff = 29568 = 115.5 x 256, so ffn_down of its Q4_K_M file is Q5_0 in the 40 layers without use_more_bits and Q8_0 (the Q6_K
fallback) in the other 40. CPU-only: the type mixture, the fixture writer and the plug-in's graph lowering under the reference's own llama_decode
(GGML_MI355_PLAN_ONLY=1, as tests/test_plugin_plan.py)."""
import os
import re

import numpy as np
import pytest

from _bind import Ref, have_ref, llama_driver_path, run_llama_driver, write_gguf_from_arrays

HERE = os.path.dirname(os.path.abspath(__file__))
Q5_0, Q8_0, Q4_K, Q5_K, Q6_K = 6, 8, 12, 13, 14
PLAN = re.compile(r"ggml-mi355 plan: (\d+) nodes -> (\d+) launches \((\d+) fused mat-vec, (\d+) attention, (\d+) node-equivalent; (\d+) nodes fused\) "
                  r"single_token=(\d) cell=(\d+) n_kv=(\d+) graphable=(\d)")


def _more_bits(il, n):
    return il < n // 8 or il >= 7 * n // 8 or (il - n // 8) % 3 == 2


def test_q5_0_row_size():
    from prima_cpp_amd import gguf as G
    from prima_cpp_amd import lib as L
    assert G.BLOCK[G.Q5_0] == (32, 22) and G.Q5_0 == 6 and L.Q5_0 == 6
    assert G.row_size(G.Q5_0, 29568) == 924 * 22
    assert L.row_size(L.Q5_0, 29568) == 924 * 22


def test_q4_k_m_types_apply_the_reference_fallback():
    from prima_cpp_amd import engine as E
    hp = E.QWEN25_72B
    n = hp["n_layer"]
    downs = [E.q4_k_m_types(hp, il)[E.T_FFN_DOWN] for il in range(n)]
    assert downs.count(Q5_0) == 40 and downs.count(Q8_0) == 40
    for il in range(n):
        t = E.q4_k_m_types(hp, il)
        assert t[E.T_FFN_DOWN] == (Q8_0 if _more_bits(il, n) else Q5_0), il
        # K = n_embd = 8192 matrices keep their K-quants
        assert t[E.T_WQ] == Q4_K and t[E.T_FFN_GATE] == Q4_K and t[E.T_WV] in (Q4_K, Q5_K, Q6_K)
    # a MODEL_70B-shaped mixture whose n_embd is no multiple of 256 would need Q5_1 for its Q5_K wv: refused with a clear error
    with pytest.raises(ValueError):
        E.q4_k_m_types(dict(hp, n_embd=8320), 20)
    # Llama shapes (every K a multiple of 256) are untouched
    for hp in (E.LLAMA3_8B, E.LLAMA3_70B):
        for il in range(hp["n_layer"]):
            assert all(v in (Q4_K, Q5_K, Q6_K) for v in E.q4_k_m_types(hp, il).values())


def test_write_synthetic_model_reference_fallback(tmp_path):
    from prima_cpp_amd import gguf as G
    kw = dict(arch=1, n_layer=8, n_embd=256, n_head=4, n_head_kv=2, n_ff=640, n_vocab=300, distinct_layers=1)   # 640 % 256 == 128
    ref = G.GGUFFile(G.write_synthetic_model(str(tmp_path / "ref.gguf"), fallback="reference", **kw) or str(tmp_path / "ref.gguf"))
    old = G.GGUFFile(G.write_synthetic_model(str(tmp_path / "old.gguf"), **kw) or str(tmp_path / "old.gguf"))
    for il in range(8):
        name = f"blk.{il}.ffn_down.weight"
        t, shape, data = ref.tensors[name]
        assert t == (Q8_0 if _more_bits(il, 8) else Q5_0), (il, t)
        assert data.nbytes == G.row_size(t, 640) * 256
        assert old.tensors[name][0] == Q8_0                     # the default keeps every fallback on Q8_0: existing fixtures unchanged
        assert ref.tensors[f"blk.{il}.ffn_gate.weight"][0] == Q4_K
    # every Q5_0 block carries a finite, positive fp16 scale
    t, _, data = ref.tensors["blk.1.ffn_down.weight"]
    assert t == Q5_0
    d = np.frombuffer(np.ascontiguousarray(data).tobytes(), dtype=np.uint8).reshape(-1, 22)[:, :2].copy().view(np.float16).astype(np.float32)
    assert np.isfinite(d).all() and (d > 0).all()
    ref.close(); old.close()
    with pytest.raises(ValueError):
        G.fallback_type(Q5_K, 640, "reference")                # Q5_K -> Q5_1: not served


def _quantize_chunk(ref, t, w):
    """the reference's ggml_quantize_chunk (ggml.c:21826): f32 [nrows, k] -> packed blocks [nrows, row bytes]"""
    import ctypes as C
    from prima_cpp_amd import gguf as G
    w = np.ascontiguousarray(w, dtype=np.float32)
    nrows, k = w.shape
    out = np.zeros((nrows, G.row_size(t, k)), dtype=np.uint8)
    f = ref.fn("ggml_quantize_chunk", C.c_size_t, [C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p])
    assert f(t, w.ctypes.data, out.ctypes.data, 0, nrows, k, None) == out.size
    return out


@pytest.mark.skipif(llama_driver_path() is None or not have_ref("scalar"), reason="oracle/_ref (reference driver and library) not built")
def test_decode_graph_with_q5_0_ffn_down_lowers_to_five_launches_per_layer(tmp_path):
    """The tiny Qwen2 model with ffn_down re-quantized by the reference's ggml_quantize_chunk - Q5_0 in layer 0, Q8_0 in layer 1 (a Q4_K_M file's
    mixture at n_ff % 256 != 0) - plans every decode graph as 5 launches per layer + 3, every layer on the plug-in: the Q5_0 down projection + residual
    is one fused mat-vec launch like the Q8_0 one. Before Q5_0 was served, supports_op refused the Q5_0 MUL_MAT: the scheduler had to run a weight that
    lives in the plug-in's buffer on the CPU backend, and the layer graph never reached the plug-in in one piece (no 72-node decode plan)."""
    z = dict(np.load(os.path.join(HERE, "golden", "tiny_qwen2_decode.npz")))
    ref = Ref("scalar")
    K, N = int(z["hp_n_ff"]), int(z["hp_n_embd"])
    from prima_cpp_amd import gguf as G
    for il, t_new in ((0, Q5_0), (1, Q8_0)):
        t_old = int(z[f"y_ffn_down_{il}"])
        blocks = np.ascontiguousarray(z[f"t_ffn_down_{il}"]).view(np.uint8).reshape(N, -1)
        w = np.stack([ref.dequantize_row(t_old, blocks[r], K) for r in range(N)])
        z[f"t_ffn_down_{il}"] = _quantize_chunk(ref, t_new, w)
        z[f"y_ffn_down_{il}"] = np.int64(t_new)
    path = write_gguf_from_arrays(str(tmp_path / "tiny_qwen2_q5_0.gguf"), z)
    g = G.GGUFFile(path)
    assert g.tensors["blk.0.ffn_down.weight"][0] == Q5_0 and g.tensors["blk.1.ffn_down.weight"][0] == Q8_0
    g.close()
    _, _, st = run_llama_driver(path, z["prompt"][:3], 4, ngl=99, n_ctx=64, threads=1, extra_args=["--keep-out-in-cuda"],
                                env={"GGML_MI355_PLAN_ONLY": "1"}, flavour="avx2", timeout=120)
    plans = [tuple(int(x) for x in m.groups()) for m in PLAN.finditer(st["stderr"])]
    n_layer = int(z["hp_n_layer"])
    decode = [p for p in plans if p[0] == 72 and p[6] == 1]
    assert len(decode) >= 3, st["stderr"][-3000:]
    for p in decode:
        _, launches, gemv, attn, node_eq, fused, single, cell, n_kv, graphable = p
        assert attn == n_layer and gemv == 4 * n_layer and node_eq == 3 and launches == 5 * n_layer + 3 and graphable == 1, p
    # the layer window is one split on the plug-in: no node of it went to the CPU backend
    assert not [p for p in plans if p[6] == 1 and p[0] not in (72, 3)], plans
