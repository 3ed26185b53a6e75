"""Q5_0 measurements (Qwen2.5-72B Q4_K_M: ffn_down falls back to Q5_0 in the 40 layers without use_more_bits, src/llama.cpp:19516-19548).

  1. the ffn_down mat-vec at K = 29568, N = 8192 (f32 activation quantized to Q8_0 in the prologue, + residual: the decode launch) in Q5_0 and in
     Q8_0, hipGraph replay of back-to-back launches; bytes = the weight stream (row stride x N) + the activation row
  2. whole-token decode of a synthetic Qwen2.5-72B engine in the Q4_K_M mixture (engine.q4_k_m_types) next to the "Q6_K" file (q6_k_types):
     1 token (captured graph), 8-token steps (small-batch path) and a 2048-token prompt (F16 prompt GEMMs)

Every number comes with its byte / FLOP count from the shapes and the fraction of 8 TB/s HBM or of the 2.5 PFLOP/s dense F16 MFMA peak.
Prints one JSON document (and writes it to --out). Use with rocprofv3 --kernel-trace --stats for the per-kernel table."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import prima_cpp_amd.engine as E  # noqa: E402
import prima_cpp_amd.ops as P  # noqa: E402
from prima_cpp_amd import gguf as G  # noqa: E402

HBM = 8.0e12
MFMA_F16 = 2.5e15
Q5_0, Q8_0 = 6, 8


def matvec(qtype, K=29568, N=8192, iters=200):
    lib = P.L.load()
    lib.pm355_mul_mat_vec_fused.restype = C.c_int
    lib.pm355_mul_mat_vec_fused.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p]
    blocks = G.random_valid_blocks(qtype, N, K, np.random.default_rng(1))
    w = P.upload_weight(qtype, blocks, K, N)
    x = torch.randn(K, device="cuda")
    res = torch.randn(N, device="cuda")
    y = torch.empty(N, device="cuda")
    job = P.MatvecJob(qtype, 0, N, w.data.data_ptr(), None, y.data_ptr(), None, res.data_ptr())

    def run(n, st):
        for _ in range(n):
            P.check(lib.pm355_mul_mat_vec_fused(C.addressof(job), 1, K, x.data_ptr(), None, 0.0, st.cuda_stream), "mat-vec")
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        run(3, side)
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=side):
            run(iters, side)
        g.replay()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ts = []
        for _ in range(3):
            e0.record(side); g.replay(); e1.record(side)
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3 / iters)
    us = sorted(ts)[1]
    nbytes = w.data.numel() + K * 4
    return {"type": "Q5_0" if qtype == Q5_0 else "Q8_0", "K": K, "N": N, "weight_bytes": int(w.data.numel()), "us": round(us, 2),
            "tb_s": round(nbytes / us / 1e6, 3), "fraction_of_8TBs": round(nbytes / us / 1e6 / 8.0, 3)}


def token_bytes(win, mixture, hp):
    """weights one token streams: every weight but the token embedding (one row of it is read)"""
    emb_t = G.Q4_K if mixture is E.q4_k_m_types else G.Q6_K
    return int(win.weight_bytes) - G.row_size(emb_t, hp["n_embd"]) * hp["n_vocab"]


def model(mixture, name, prompt=2048, n_ctx=4096):
    hp = dict(E.QWEN25_72B)
    win = E.Window(hp, lo=0, hi=hp["n_layer"], flags=E.HAS_EMBD | E.HAS_HEAD, n_ctx=n_ctx)
    win.fill_synthetic(mixture, seed=1234)
    win.finalize(max_tokens=prompt, n_seq=1)
    wb = token_bytes(win, mixture, hp)
    rng = np.random.default_rng(3)
    toks = torch.from_numpy(rng.integers(0, hp["n_vocab"], prompt).astype(np.int32)).cuda()
    st = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = {"model": name, "weight_bytes": wb}
    # 2048-token prompt (first call warms up: allocations, plans)
    win.decode(tokens=toks, pos0=0, want_hidden=False)
    torch.cuda.synchronize()
    e0.record(st); win.decode(tokens=toks, pos0=0, want_hidden=False); e1.record(st)
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1)
    E_, F, Ekv = hp["n_embd"], hp["n_ff"], hp["n_head_kv"] * hp["head_dim"]
    flop = 2.0 * prompt * hp["n_layer"] * (E_ * (2 * E_ + 2 * Ekv) + 3 * E_ * F)
    out["prompt_2048"] = {"ms": round(ms, 2), "tokens_per_s": round(prompt / ms * 1e3, 1), "weight_gemm_flop": flop,
                          "fraction_of_mfma_f16_peak": round(flop / (ms / 1e3) / MFMA_F16, 3)}
    # 8-token steps (small-batch path)
    win.kv_clear()
    win.decode(tokens=toks[:8], pos0=0, want_hidden=False)
    torch.cuda.synchronize()
    e0.record(st)
    for i in range(4):
        win.decode(tokens=toks[:8], pos0=8 * (i + 1), want_hidden=False)
    e1.record(st)
    torch.cuda.synchronize()
    ms8 = e0.elapsed_time(e1) / 4
    out["batch_8"] = {"ms_per_step": round(ms8, 3), "tokens_per_s": round(8 / ms8 * 1e3, 1), "fraction_of_8TBs": round(wb / (ms8 / 1e3) / HBM, 3)}
    # single tokens through the captured graph
    win.kv_clear()
    win.decode(tokens=toks[:16], pos0=0, want_hidden=False)
    win.set_pos(16)
    tok = torch.zeros(1, dtype=torch.int32, device="cuda")
    lg = torch.empty(hp["n_vocab"], dtype=torch.float32, device="cuda")
    for _ in range(8):
        win.step(token=tok, logits=lg)
    torch.cuda.synchronize()
    n = 64
    e0.record(st)
    for _ in range(n):
        win.step(token=tok, logits=lg)
    e1.record(st)
    torch.cuda.synchronize()
    ms1 = e0.elapsed_time(e1) / n
    out["decode_1"] = {"ms_per_token": round(ms1, 3), "tokens_per_s": round(1e3 / ms1, 1), "roofline_ms": round(wb / HBM * 1e3, 3),
                       "fraction_of_8TBs": round(wb / (ms1 / 1e3) / HBM, 3)}
    win.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--part", default="all", choices=["all", "matvec", "models"])
    a = ap.parse_args()
    res = {}
    if a.part in ("all", "matvec"):
        res["ffn_down_matvec"] = [matvec(Q5_0), matvec(Q8_0)]
    if a.part in ("all", "models"):
        res["qwen25_72b"] = [model(E.q4_k_m_types, "Qwen2.5-72B Q4_K_M (ffn_down Q5_0 / Q8_0)"), model(E.q6_k_types, "Qwen2.5-72B Q6_K (ffn_down Q8_0)")]
    s = json.dumps(res, indent=1)
    print(s)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
