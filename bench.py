#!/usr/bin/env python
"""bench.py — decode tokens/s of the quantized decode hot path on MI355X.

Workload (BASELINE.json: metric quoted on Llama-3-70B Q4_K_M, which fits one GPU): synthetic
Llama-3-70B-shaped weights with the Q4_K_M type mixture generated directly in HBM, synthetic prompt,
batch-1 greedy decode. One "step" = every in-flight sequence advances by one token:
  N = 1 : one sequence, one token per step (whole model on the GPU, one hipGraph replay per token);
  N > 1 : piped-ring layer split, one rank per GPU, N sequences in flight staggered by one rank
          (N micro-steps per step; activations handed on with RCCL send/recv), N tokens per step.
Per-GPU HBM traffic per step is the same for every N (each rank streams its window N times) -> "weak".

Prints ONE JSON line on rank 0 (metric, value, unit, higher_is_better, dtype, ms_per_step, config). A plain run only sets up,
warms up, times --steps steps and prints that line. --dump-outputs DIR also writes the last timed step's output row (what
pm355_ring_decode_last_output hands a caller: float32 [n_embd], one file per rank) as DIR/last_output[_rank<r>].npy.
--full adds everything that takes runs of its own, among them:
  roofline     — dominant kernel (Q4_K gate/up mat-vec) timed live with HIP events on its launch stream
  cpu_baseline — the UNMODIFIED reference ggml CPU backend (oracle/_ref) timed on this host's cores on a
                 bounded sample of the same workload (N=1, rank 0 only)
  prefill / extra configs / plug-in decode / parity check / weight streaming (N=1), single stream + ring prefill (N>1)
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0          # MI355X HBM3E spec peak (MI355X_MICROARCH.md); measured copy ceiling ~6290 GB/s


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--model", default="llama3-70b", choices=["llama3-70b", "llama3-8b", "qwen2.5-72b"])
    ap.add_argument("--n-ctx", type=int, default=4096)
    ap.add_argument("--prompt", type=int, default=16)
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--prefill", type=int, default=2048, help="prompt length of the (untimed-for-the-metric) prefill probe, 0 = off")
    ap.add_argument("--cpu-seconds", type=float, default=12.0)
    ap.add_argument("--no-extras", action="store_true", help="skip extra_configs / plugin_decode / the llama_decode CPU baseline")
    ap.add_argument("--tmp", default=os.environ.get("TMPDIR", "/tmp"), help="where the synthetic GGUF files of the plug-in legs go")
    ap.add_argument("--section", default="", help="(internal) run ONE extra leg in this process and print its JSON: prefill_qwen | long_context[:model]")
    ap.add_argument("--full", action="store_true", help="also run every measurement beyond the headline (roofline probe, prefill, CPU baseline, "
                                                        "extra configs, plug-in decode, parity check; N>1: single stream, ring prefill)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="after the timed steps, write the last step's output row as DIR/*.npy (float32)")
    return ap.parse_args()


def model_cfg(name):
    import prima_cpp_amd.engine as E
    if name == "llama3-70b":
        return E.LLAMA3_70B, E.q4_k_m_types, "Llama-3-70B Q4_K_M"
    if name == "llama3-8b":
        return E.LLAMA3_8B, E.q4_k_m_types, "Llama-3-8B Q4_K_M"
    return E.QWEN25_72B, E.q6_k_types, "Qwen2.5-72B Q6_K"


def layer_bytes(hp, mixture):
    from prima_cpp_amd.lib import row_size
    import prima_cpp_amd.engine as E
    Ed, Eq, Ekv, F = hp["n_embd"], hp["head_dim"] * hp["n_head"], hp["head_dim"] * hp["n_head_kv"], hp["n_ff"]
    shape = {E.T_WQ: (Ed, Eq), E.T_WK: (Ed, Ekv), E.T_WV: (Ed, Ekv), E.T_WO: (Eq, Ed), E.T_FFN_GATE: (Ed, F),
             E.T_FFN_UP: (Ed, F), E.T_FFN_DOWN: (F, Ed)}
    out = []
    for il in range(hp["n_layer"]):
        t = mixture(hp, il)
        out.append(sum(row_size(t[k], kk) * n for k, (kk, n) in shape.items()) + 2 * Ed * 4)
    return out


def usable_cores():
    """Threads the CPU baseline may use: affinity mask capped by the cgroup CPU quota (the GPU box exposes 256 logical
    CPUs but a cpu.max quota of 16; oversubscribing ggml's spin-barrier thread pool is catastrophically slow)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            q, p = f.read().split()
            if q != "max":
                n = max(1, min(n, int(int(q) / int(p))))
    except (OSError, ValueError):
        pass
    return n


def cpu_baseline(hp, mixture, seconds):
    """Reference ggml CPU backend (unmodified sources, prebuilt under oracle/_ref) on this host's cores."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _bind as B
    import prima_cpp_amd.engine as E
    flavour = B.best_ref_flavour()
    if flavour is None:
        return None
    ref = B.Ref(flavour)
    cores = usable_cores()
    rng = np.random.default_rng(0)
    Ed, Eq, Ekv, F = hp["n_embd"], hp["head_dim"] * hp["n_head"], hp["head_dim"] * hp["n_head_kv"], hp["n_ff"]
    shape = {E.T_WQ: (Ed, Eq), E.T_WK: (Ed, Ekv), E.T_WV: (Ed, Ekv), E.T_WO: (Eq, Ed), E.T_FFN_GATE: (Ed, F),
             E.T_FFN_UP: (Ed, F), E.T_FFN_DOWN: (F, Ed)}
    # distinct layer compositions of the mixture, weighted by how often they occur
    comps = {}
    for il in range(hp["n_layer"]):
        key = tuple(sorted(mixture(hp, il).items()))
        comps[key] = comps.get(key, 0) + 1
    t_token, t_spent, desc = 0.0, 0.0, []
    budget = seconds / (len(comps) + 1)
    for key, count in comps.items():
        mats = [(t, shape[k][0], shape[k][1], B.rand_blocks(t, shape[k][1], shape[k][0], rng)) for k, t in key]
        t0 = time.time()
        one = ref.time_layer_matvecs(mats, cores, reps=2)
        reps = max(1, min(5000, int(budget / max(one, 1e-4))))     # ~cpu_seconds of reference CPU work in total
        best = min(one, ref.time_layer_matvecs(mats, cores, reps=reps))
        t_spent += time.time() - t0
        t_token += best * count
        desc.append(f"{count}x layer[{','.join(B.TYPE_NAMES[t] for _, t in key)}]")
        del mats
    out_t = B.Q6_K
    n_v = hp["n_vocab"]
    sub = 8                                                  # lm_head sampled on 1/8 of its rows
    mats = [(out_t, Ed, n_v // sub, B.rand_blocks(out_t, n_v // sub, Ed, rng))]
    one = ref.time_layer_matvecs(mats, cores, reps=2)
    t_token += min(one, ref.time_layer_matvecs(mats, cores, reps=max(1, min(5000, int(budget / max(one, 1e-4)))))) * sub
    desc.append(f"lm_head[q6_K] on 1/{sub} of its rows")
    return {"value": 1.0 / t_token, "unit": "tokens/s", "cores": cores, "kind": "reference",
            "sample": "7 quantized mat-vecs of one layer per distinct Q4_K_M layer composition (" + " + ".join(desc) +
                      f"), random valid blocks, reference ggml CPU backend ({ref.build_info()}), {cores} threads, "
                      "best of repeated passes, scaled by layer counts to one token (mat-vecs only: norms/rope/"
                      "attention excluded, which favours the CPU)"}


def kernel_source_sha16():
    import hashlib
    h = hashlib.sha256()
    d = os.path.join(os.path.dirname(os.path.abspath(__file__)), "prima_cpp_amd", "csrc")
    for f in ("mmvq.hip", "mmvq_device.h", "pm355_device.h"):
        with open(os.path.join(d, f), "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def pmc_traffic(bytes_per_launch):
    """HBM bytes per launch of the dominant kernel from the committed PMC pass of this round (profiles/rNN_pmc_traffic.json:
    rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE on tools/pmc_probe.py in separate passes, x1024 B and the gfx950 x2 correction of
    MI355X_MICROARCH.md; tools/collect_profiles.sh). Counters cannot be read from inside the timed process, so this is the recorded
    measurement - accepted only when it was taken on the SAME kernel sources (sha of mmvq.hip / mmvq_device.h / pm355_device.h recorded
    next to it) and the same launch shape; otherwise None (re-run tools/collect_profiles.sh)."""
    try:
        prof = os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles")
        names = sorted((n for n in os.listdir(prof) if n.endswith("_pmc_traffic.json")), reverse=True)
        for name in names:
            with open(os.path.join(prof, name)) as f:
                t = json.load(f)
            if t.get("kernel_source_sha16") == kernel_source_sha16() and int(t["algorithmic_bytes_per_launch"]) == int(bytes_per_launch):
                return int(t["hbm_read_bytes_per_launch"]) + int(t["hbm_write_bytes_per_launch_uncalibrated"])
    except Exception:
        pass
    return None


def probe_dominant_kernel(win, hp, iters=40):
    """Average duration of the dominant kernel (Q4_K gate/up mat-vec pair: 2 x [n_ff x n_embd] read once) measured with
    HIP events on the stream it is launched on, rotating over the real layers' weights (no cache reuse)."""
    import ctypes as C
    import prima_cpp_amd.engine as E
    import prima_cpp_amd.ops as P
    from prima_cpp_amd.lib import Q4_K, row_size
    lib = P.L.load()
    Ed, F = hp["n_embd"], hp["n_ff"]
    x = torch.randn(1, Ed, device="cuda")
    nw = torch.ones(Ed, device="cuda")
    y = torch.empty(F, dtype=torch.float32, device="cuda")
    tp = C.c_void_p
    lib.pm355_model_tensor_ptr.restype = tp
    lib.pm355_model_tensor_ptr.argtypes = [tp, C.c_int, C.c_int, C.POINTER(C.c_int)]
    lib.pm355_mul_mat_vec_fused.restype = C.c_int
    lib.pm355_mul_mat_vec_fused.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p]
    jobs = []
    for il in range(win.lo, win.hi):
        ty = C.c_int(0)
        g = lib.pm355_model_tensor_ptr(win.h, E.T_FFN_GATE, il, C.byref(ty))
        u = lib.pm355_model_tensor_ptr(win.h, E.T_FFN_UP, il, C.byref(ty))
        if ty.value == Q4_K:
            jobs.append(P.MatvecJob(Q4_K, 0, F, g, u, P.ptr(y), None, None))
    if not jobs:
        return None
    st = torch.cuda.current_stream()

    def run(n):
        # exactly the engine's launch: f32 activation, fused rms_norm * weight + Q8_K quantization, gate/up pair, silu*mul
        for i in range(n):
            P.check(lib.pm355_mul_mat_vec_fused(C.addressof(jobs[i % len(jobs)]), 1, Ed, P.ptr(x), P.ptr(nw), 1e-5, st.cuda_stream), "probe")
    run(len(jobs))
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    # launched the way the engine launches it: from a captured hipGraph (back-to-back dispatch, no host launch gaps)
    launch = "hipGraph replay"
    try:
        side = torch.cuda.Stream()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            st = torch.cuda.current_stream()
            with torch.cuda.graph(graph, stream=side):
                run(iters)
            graph.replay()
            torch.cuda.synchronize()
            e0.record(side)
            graph.replay()
            e1.record(side)
        torch.cuda.synchronize()
    except Exception:                                 # capture unavailable: eager launches (adds host launch gaps)
        launch = "eager launches"
        st = torch.cuda.current_stream()
        torch.cuda.synchronize()
        e0.record(st)
        run(iters)
        e1.record(st)
        torch.cuda.synchronize()
    st = torch.cuda.current_stream()
    us = e0.elapsed_time(e1) * 1e3 / iters
    nbytes = 2 * row_size(Q4_K, Ed) * F
    out = {"kernel": "gemv_q_kernel<Q4_K, PAIR> (rms_norm + Q8_K quantize + ffn_gate/ffn_up mat-vec + silu*mul, one launch)",
           "bytes_per_launch": nbytes, "avg_us": us, "gbs": nbytes / us / 1e3, "launch": launch}
    # what a pure streaming read of the same number of bytes achieves on this box (measured peak next to spec)
    try:
        plib = P.L.load_probe()                       # measurement helpers live in their own library (tools/csrc)
        span = ((nbytes + (1 << 20) - 1) >> 20) << 20
        nspan = 6                                     # > 1.5 GB rotated: nothing survives in the 256 MB infinity cache
        buf = torch.empty(nspan * span, dtype=torch.uint8, device="cuda")
        buf.random_(0, 255)
        sink = torch.zeros(4, dtype=torch.int32, device="cuda")
        ts = []
        for rep in range(2 * nspan):
            e0.record(st)
            P.check(plib.pm355_probe_stream_read(buf.data_ptr() + (rep % nspan) * span, nbytes, 1, 8, sink.data_ptr(), st.cuda_stream), "stream probe")
            e1.record(st)
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3)
        ts = sorted(ts[nspan:])
        out["stream_read_gbs"] = nbytes / ts[len(ts) // 2] / 1e3     # median single launch of the second round
    except Exception:
        out["stream_read_gbs"] = None
    return out


def probe_prefill(hp, mixture, n_tok, small_batches=(2, 3, 4, 8, 16, 32, 64)):
    """Prefill probe (reported as an extra, not the metric): an n_tok-token prompt through the WHOLE model (token embedding, every
    layer on the MFMA GEMM + MFMA attention path, result_norm + lm_head on the last token), plus `roofline` for its dominant kernel
    - the ffn gate / up GEMM - timed with HIP events on its launch stream."""
    import ctypes as C
    import prima_cpp_amd.engine as E
    import prima_cpp_amd.ops as P
    from prima_cpp_amd.lib import Q4_K, Q6_K
    win = E.Window(hp, lo=0, hi=hp["n_layer"], flags=E.HAS_EMBD | E.HAS_HEAD, n_ctx=max(1024, ((n_tok + 63) // 64) * 64))
    win.fill_synthetic(mixture, seed=4321)
    win.finalize(max_tokens=n_tok, n_seq=1)
    toks = torch.randint(0, hp["n_vocab"], (n_tok,), dtype=torch.int32, device="cuda")
    win.decode(tokens=toks, pos0=0, want_hidden=False, want_logits=True)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    st = torch.cuda.current_stream()
    win.kv_clear()
    e0.record(st)
    win.decode(tokens=toks, pos0=0, want_hidden=False, want_logits=True)
    e1.record(st)
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1)
    Ed, Eq, Ekv, F = hp["n_embd"], hp["head_dim"] * hp["n_head"], hp["head_dim"] * hp["n_head_kv"], hp["n_ff"]
    params = Ed * Eq * 2 + 2 * Ed * Ekv + 3 * Ed * F
    flop = 2.0 * params * n_tok * hp["n_layer"]
    out = {"prompt_tokens": n_tok, "layers_timed": hp["n_layer"], "tokens_per_s": round(n_tok / (ms / 1e3), 1), "ms": round(ms, 2),
           "gemm_tflops_whole_prompt": round(flop / (ms / 1e3) / 1e12, 1), "mfma_peak_tflops_f16_dense": 2500.0,
           "note": "token embedding + all layers (MFMA v_mfma_f32_32x32x16_f16 weight GEMMs with on-the-fly dequantization, MFMA causal "
                   "attention) + result_norm + lm_head on the last token; gemm_tflops_whole_prompt counts the weight-GEMM FLOPs over the whole time"}
    # the same prompt handed over in the reference's default micro-batches (n_ubatch = 512, common/common.h:178: what llama_decode passes to a backend
    # per graph when the prompt is longer) - every chunk a pass over all weights, the cells of the earlier chunks attended from the cache
    try:
        UB = 512
        if n_tok > UB and n_tok % UB == 0:
            win.kv_clear()
            e0.record(st)
            for c0 in range(0, n_tok, UB):
                win.decode(tokens=toks[c0:c0 + UB], pos0=c0, want_hidden=False, want_logits=(c0 + UB == n_tok))
            e1.record(st)
            torch.cuda.synchronize()
            ms_ub = e0.elapsed_time(e1)
            out["n_ubatch_512"] = {"tokens_per_s": round(n_tok / (ms_ub / 1e3), 1), "ms": round(ms_ub, 2), "chunks": n_tok // UB,
                                   "gemm_tflops_whole_prompt": round(flop / (ms_ub / 1e3) / 1e12, 1)}
    except Exception as e:
        out["n_ubatch_512"] = {"error": str(e)[:300]}
    # small batches through the same window (speculative decoding / parallel sequences / short prompts): 2..32 tokens per step take the
    # integer-matrix-core mat-mul (mmq_i8.hip: one weight pass per 32 tokens), whole model, KV positions advancing
    try:
        sb = {}
        for T in small_batches:
            if T > n_tok:
                continue
            win.kv_clear()
            win.decode(tokens=toks[:T], pos0=0, want_hidden=False, want_logits=True)
            torch.cuda.synchronize()
            e0.record(st)
            for i in range(3):
                win.decode(tokens=toks[:T], pos0=T * (i + 1), want_hidden=False, want_logits=True)
            e1.record(st)
            torch.cuda.synchronize()
            sb[str(T)] = {"ms_per_step": round(e0.elapsed_time(e1) / 3, 3), "tokens_per_s": round(3 * T / (e0.elapsed_time(e1) / 1e3), 1)}
        out["small_batch"] = sb
    except Exception as e:
        out["small_batch"] = {"error": str(e)[:300]}
    # dominant kernel: ffn_gate GEMM [n_tok x n_embd] x [n_ff x n_embd]^T of layer 0 (its type decides the instantiation)
    try:
        lib = P.L.load()
        lib.pm355_model_tensor_ptr.restype = C.c_void_p
        lib.pm355_model_tensor_ptr.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int)]
        ty = C.c_int(0)
        wp = lib.pm355_model_tensor_ptr(win.h, E.T_FFN_GATE, 0, C.byref(ty))
        x = torch.randn(n_tok, Ed, device="cuda") * 0.5
        y = torch.empty(n_tok, F, device="cuda")
        lib.pm355_mul_mat_q_mfma.argtypes = [C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        run = lambda: P.check(lib.pm355_mul_mat_q_mfma(ty.value, wp, Ed, F, x.data_ptr(), n_tok, y.data_ptr(), None, None, st.cuda_stream), "gemm probe")
        run(); torch.cuda.synchronize()
        iters = 10
        e0.record(st)
        for _ in range(iters):
            run()
        e1.record(st)
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / iters
        tf = 2.0 * n_tok * Ed * F / us / 1e6
        # what the vendor's plain F16 GEMM (no dequantization) reaches for the same shape on this box: the practical ceiling, measured
        a16, b16 = x.half(), torch.randn(F, Ed, device="cuda", dtype=torch.float16)
        for _ in range(2):
            (a16 @ b16.t())
        torch.cuda.synchronize()
        e0.record(st)
        for _ in range(iters):
            (a16 @ b16.t())
        e1.record(st)
        torch.cuda.synchronize()
        lib_tf = 2.0 * n_tok * Ed * F / (e0.elapsed_time(e1) * 1e3 / iters) / 1e6
        tname = {Q4_K: "Q4_K", Q6_K: "Q6_K"}.get(ty.value, str(ty.value))
        out["roofline"] = {"bound": "mfma", "achieved": round(tf, 1), "peak": 2500.0, "unit": "TFLOP/s", "frac": round(tf / 2500.0, 4),
                           "kernel": f"gemm_pf_kernel<{tname}> (mmq_pf.hip) ffn_gate [{n_tok} x {Ed}] x [{F} x {Ed}]^T incl. the f32->f16 conversion of the activations",
                           "flops_per_launch": 2.0 * n_tok * Ed * F, "avg_launch_us": round(us, 1),
                           "library_f16_gemm_same_shape_tflops": round(lib_tf, 1), "frac_of_library_f16_gemm": round(tf / lib_tf, 4),
                           "traffic": None,
                           "note": "peak = dense F16 MFMA at the nominal 2.4 GHz. With random operands the matrix pipe itself is power-throttled on this chip: "
                                   "back-to-back v_mfma_f32_32x32x16_f16 on every SIMD and nothing else take 25.5 ns each = 1.3 PFLOP/s (tools/r6/mfma_valu_probe.hip, "
                                   "profiles/r06_mfma_power_limit.txt); library_f16_gemm = torch.matmul (hipBLASLt) F16 x F16 of the same shape on this box, "
                                   "measured here only as the practical ceiling"}
        # the launches the layer really makes: wq | wk | wv as ONE launch of jobs, ffn_gate | ffn_up as ONE launch of pair tiles (silu(gate) * up inside the workgroup)
        try:
            class _Job(C.Structure):
                _fields_ = [("type", C.c_int32), ("N", C.c_int32), ("W", C.c_void_p), ("y", C.c_void_p), ("bias", C.c_void_p), ("resid", C.c_void_p)]
            jobs, outs, nq = (_Job * 3)(), [], 0
            for j, k in enumerate((E.T_WQ, E.T_WK, E.T_WV)):
                tj = C.c_int(0)
                wj = lib.pm355_model_tensor_ptr(win.h, k, 0, C.byref(tj))
                nj = Eq if k == E.T_WQ else Ekv
                outs.append(torch.empty(n_tok, nj, device="cuda"))
                jobs[j].type, jobs[j].N, jobs[j].W, jobs[j].y = tj.value, nj, wj, outs[-1].data_ptr()
                nq += nj
            lib.pm355_mul_mat_q_mfma_multi.restype = C.c_int
            lib.pm355_mul_mat_q_mfma_multi.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]
            runq = lambda: P.check(lib.pm355_mul_mat_q_mfma_multi(C.addressof(jobs), 3, Ed, x.data_ptr(), n_tok, st.cuda_stream), "qkv probe")
            tu = C.c_int(0)
            wu = lib.pm355_model_tensor_ptr(win.h, E.T_FFN_UP, 0, C.byref(tu))
            lib.pm355_mul_mat_q_mfma_pair.restype = C.c_int
            lib.pm355_mul_mat_q_mfma_pair.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
            runp = lambda: P.check(lib.pm355_mul_mat_q_mfma_pair(ty.value, wp, wu, Ed, F, x.data_ptr(), n_tok, y.data_ptr(), st.cuda_stream), "pair probe")
            for nm, fn, fl in (("qkv_one_launch", runq, 2.0 * n_tok * Ed * nq), ("gate_up_pair_launch", runp, 4.0 * n_tok * Ed * F)):
                if nm == "gate_up_pair_launch" and tu.value != ty.value:
                    continue
                fn(); torch.cuda.synchronize()
                e0.record(st)
                for _ in range(iters):
                    fn()
                e1.record(st)
                torch.cuda.synchronize()
                u2 = e0.elapsed_time(e1) * 1e3 / iters
                out["roofline"][nm] = {"avg_launch_us": round(u2, 1), "tflops": round(fl / u2 / 1e6, 1), "frac": round(fl / u2 / 1e6 / 2500.0, 4),
                                       "note": "incl. the f32->f16 conversion of the activations"}
        except Exception as e:
            out["roofline"]["launch_forms"] = {"error": str(e)[:300]}
    except Exception as e:
        out["roofline"] = {"error": str(e)[:300]}
    win.close()
    return out


def extra_config(name, steps=32, warmup=8, prompt=16, n_ctx=4096):
    """One more BASELINE.json config on the same engine path as the headline (batch-1 greedy decode, one hipGraph replay per
    token): tokens/s and fraction of that model's HBM roofline."""
    import prima_cpp_amd.engine as E
    from prima_cpp_amd.lib import Q6_K, row_size
    from prima_cpp_amd.ring import CRing
    hp, mixture, model_name = model_cfg(name)
    lb = layer_bytes(hp, mixture)
    total_w = sum(lb) + row_size(Q6_K, hp["n_embd"]) * hp["n_vocab"] + hp["n_embd"] * 4
    win = E.Window(hp, lo=0, hi=hp["n_layer"], flags=E.HAS_EMBD | E.HAS_HEAD, n_ctx=n_ctx)
    win.fill_synthetic(mixture, seed=1234)
    win.finalize(max_tokens=1, n_seq=1)
    ring = CRing(0, 1, transport="local")
    rng = np.random.default_rng(1234)
    toks = rng.integers(0, hp["n_vocab"], size=prompt)
    ring.decode_staggered(win, prompt + warmup, forced=[int(toks[s_]) if s_ < prompt else None for s_ in range(prompt + warmup)], reset=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ring.decode_staggered(win, steps)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    ring.wait()
    torch.cuda.synchronize()
    finite = bool(torch.isfinite(ring.last_output(hp["n_embd"])).all().item())
    ring.close()
    win.close()
    roof = HBM_PEAK_GBS * 1e9 / total_w
    return {"workload": f"{model_name} batch-1 greedy decode, {prompt}-token synthetic prompt, n_ctx {n_ctx}, F16 KV cache, 1 GPU",
            "tokens_per_s": round(steps / dt, 2), "ms_per_token": round(dt / steps * 1e3, 4), "weights_bytes_per_token": total_w, "activations_finite": finite,
            "hbm_roofline_tokens_per_s": round(roof, 1), "frac_of_hbm_roofline": round(steps / dt / roof, 4)}


def streaming_probe(name="llama3-8b", n_slots=4, steps=6):
    """Window streaming (north_star: async weight staging from host DRAM via pinned hipMemcpyAsync in place of prima.cpp's mmap
    prefetch): the layer tensors live in pinned host memory and are cycled through n_slots device slots while the compute stream
    decodes. Bounded by the host -> device link, not by HBM: reported as tokens/s and achieved H2D GB/s."""
    import prima_cpp_amd.engine as E
    hp, mixture, model_name = model_cfg(name)
    t0 = time.perf_counter()
    win = E.Window(hp, lo=0, hi=hp["n_layer"], flags=E.HAS_EMBD | E.HAS_HEAD, n_ctx=512)
    win.set_streaming(n_slots)
    win.fill_synthetic(mixture, seed=77)
    win.finalize(max_tokens=1, n_seq=1)
    torch.cuda.synchronize()
    t_load = time.perf_counter() - t0
    tok = torch.zeros(1, dtype=torch.int32, device="cuda")
    am = torch.zeros(1, dtype=torch.int32, device="cuda")
    win.set_pos(0)
    for _ in range(2):
        win.step(token=tok, argmax=am, advance=1)
    torch.cuda.synchronize()
    b0 = win.streamed_bytes()
    t0 = time.perf_counter()
    for _ in range(steps):
        win.step(token=tok, argmax=am, advance=1)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    moved = win.streamed_bytes() - b0
    win.close()
    return {"workload": f"{model_name} decode with the layer window streamed from pinned host memory through {n_slots} device layer slots "
                        f"(pm355_model_set_streaming), token embedding / head / KV resident",
            "tokens_per_s": round(steps / dt, 2), "h2d_GBps": round(moved / dt / 1e9, 1), "h2d_bytes_per_token": int(moved / steps),
            "park_and_setup_s": round(t_load, 2)}


def _driver(flavour_pref=None):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _bind as B
    return B, B.llama_driver_path(flavour_pref)


def plugin_decode(tmp, n_gen=64, prompt_len=16):
    """BASELINE.json config 1/2 through the DROP-IN boundary: a Llama-3-8B-shaped Q4_K_M GGUF (random valid blocks) decoded by
    the reference's unmodified llama_decode (oracle/_ref/llama-ref-driver-*, built from /root/reference with the committed gate
    patch) with every layer + the output layer in the MI355 buffer type (-ngl 99 --keep-out-in-cuda). The driver binary only
    orchestrates; all compute runs in libggml-mi355.so / libprima_mi355.so."""
    from prima_cpp_amd import gguf as G
    B, drv = _driver()
    if drv is None:
        return None, None
    path = os.path.join(tmp, "pm355_bench_llama3_8b_q4km.gguf")
    t0 = time.time()
    G.write_synthetic_model(path, arch=0, n_layer=32, n_embd=4096, n_head=32, n_head_kv=8, n_ff=14336, n_vocab=128256)
    t_gen = time.time() - t0
    prompt = np.random.default_rng(1234).integers(0, 128256, prompt_len)
    prompt[0] = 128000
    _, _, st = B.run_llama_driver(path, prompt, n_gen, ngl=99, n_ctx=4096, threads=usable_cores(), extra_args=["--keep-out-in-cuda"], timeout=150)
    total_w = 4617000000.0                       # bytes read per decoded token, Llama-3-8B Q4_K_M
    roof = HBM_PEAK_GBS * 1e9 / total_w
    out = {"workload": f"Llama-3-8B-shaped Q4_K_M GGUF ({os.path.getsize(path) / 1e9:.2f} GB, random valid blocks, no_vocab) through the reference's "
                       f"llama_decode + MI355 plug-in: -ngl 99 --keep-out-in-cuda, {prompt_len}-token prompt, {n_gen} greedy tokens, n_ctx 4096",
           "tokens_per_s": round(st["decode_tok_s"], 2), "ms_per_token": round(st["decode_ms_avg"], 4), "best_ms_per_token": round(st["decode_ms_min"], 4),
           "prompt_tokens_per_s": round(st["prompt_tok_s"], 1), "load_ms": round(st["load_ms"], 1), "gguf_write_s": round(t_gen, 1),
           "hbm_roofline_tokens_per_s": round(roof, 1), "frac_of_hbm_roofline": round(st["decode_tok_s"] / roof, 4),
           "timing": "wall clock around llama_decode + llama_synchronize per token, first 5 tokens dropped (llama_perf convention)"}
    # the same run with oracle/ref_patches/graph_reuse.patch switched on (LLAMA_MI355_GRAPH_REUSE=1: libllama keeps the previous single-token graph and
    # scheduler allocation; the headline figure above is the reference's unpatched per-token graph build)
    try:
        _, _, sr = B.run_llama_driver(path, prompt, n_gen, ngl=99, n_ctx=4096, threads=usable_cores(), extra_args=["--keep-out-in-cuda"], timeout=150,
                                      env={"LLAMA_MI355_GRAPH_REUSE": "1"})
        out["graph_reuse_patch"] = {"tokens_per_s": round(sr["decode_tok_s"], 2), "ms_per_token": round(sr["decode_ms_avg"], 4), "best_ms_per_token": round(sr["decode_ms_min"], 4),
                                    "frac_of_hbm_roofline": round(sr["decode_tok_s"] / roof, 4)}
    except Exception as e:                       # noqa: BLE001 - a bench leg, never fatal
        out["graph_reuse_patch"] = {"error": str(e)[:200]}
    # the same model with --flash-attn (FLASH_ATTN_EXT graphs: row-major V cache, F16 mask) - lowered to the same five launches
    try:
        _, _, sf = B.run_llama_driver(path, prompt, 32, ngl=99, n_ctx=4096, threads=usable_cores(), extra_args=["--keep-out-in-cuda", "-fa"], timeout=150)
        out["flash_attn"] = {"tokens_per_s": round(sf["decode_tok_s"], 2), "ms_per_token": round(sf["decode_ms_avg"], 4), "prompt_tokens_per_s": round(sf["prompt_tok_s"], 1)}
    except Exception as e:                       # noqa: BLE001 - a bench leg, never fatal
        out["flash_attn"] = {"error": str(e)[:200]}
    return out, path


def plugin_decode_70b(tmp, hp70, engine_ms_per_token, n_gen=48):
    """The HEADLINE shape through the drop-in boundary: Llama-3-70B-shaped Q4_K_M GGUFs of 8, 16 and 32 layers decoded by the reference's
    llama_decode + the MI355 plug-in (-ngl 99 --keep-out-in-cuda); per-layer and fixed cost from a line through the depths, the 80-layer token
    time they imply, and that against the resident engine's measured token (what the scheduler path costs at this shape)."""
    from prima_cpp_amd import gguf as G
    B, drv = _driver()
    if drv is None:
        return None
    prompt = np.random.default_rng(1234).integers(0, 128256, 16)
    prompt[0] = 128000
    ms, ms_reuse = {}, {}
    depths = (8, 16, 32)
    for L in depths:
        p = os.path.join(tmp, f"pm355_bench_llama3_70b_shape_{L}l.gguf")
        G.write_synthetic_model(p, arch=0, n_layer=L, n_embd=hp70["n_embd"], n_head=hp70["n_head"], n_head_kv=hp70["n_head_kv"],
                                n_ff=hp70["n_ff"], n_vocab=hp70["n_vocab"], is_70b=True)
        try:
            _, _, st = B.run_llama_driver(p, prompt, n_gen, ngl=99, n_ctx=4096, threads=usable_cores(), extra_args=["--keep-out-in-cuda"], timeout=300)
            ms[L] = (st["decode_ms_avg"], st["decode_ms_min"])
            try:                                     # the same file with oracle/ref_patches/graph_reuse.patch switched on
                _, _, sr = B.run_llama_driver(p, prompt, n_gen, ngl=99, n_ctx=4096, threads=usable_cores(), extra_args=["--keep-out-in-cuda"], timeout=300,
                                              env={"LLAMA_MI355_GRAPH_REUSE": "1"})
                ms_reuse[L] = sr["decode_ms_avg"]
            except Exception:                        # noqa: BLE001
                pass
        finally:
            os.unlink(p)
    # least-squares line through the depths (two points made the slope - and with it the 80-layer figure - swing by 10 % between boxes)
    A = np.stack([np.array(depths, dtype=np.float64), np.ones(len(depths))], axis=1)
    (per_layer, fixed), *_ = np.linalg.lstsq(A, np.array([ms[L][0] for L in depths]), rcond=None)
    per_layer, fixed = float(per_layer), float(fixed)
    tok_ms = fixed + hp70["n_layer"] * per_layer
    out = {"workload": f"Llama-3-70B-shaped Q4_K_M GGUFs of {' / '.join(str(L) for L in depths)} layers (random valid blocks, no_vocab) through the reference's llama_decode + MI355 "
                       f"plug-in: -ngl 99 --keep-out-in-cuda, 16-token prompt, {n_gen} greedy tokens, n_ctx 4096",
           "ms_per_token_at_depth": {str(L): round(ms[L][0], 4) for L in depths}, "best_ms_per_token_at_depth": {str(L): round(ms[L][1], 4) for L in depths},
           "ms_per_layer": round(per_layer, 4), "ms_fixed": round(fixed, 4), "ms_per_token_80_layers": round(tok_ms, 4), "tokens_per_s_80_layers": round(1e3 / tok_ms, 2),
           "timing": "wall clock around llama_decode + llama_synchronize per token, first 5 tokens dropped; least-squares line over the depths"}
    if engine_ms_per_token:
        out["engine_ms_per_token"] = round(engine_ms_per_token, 4)
        out["frac_of_engine"] = round(engine_ms_per_token / tok_ms, 4)
    if len(ms_reuse) == len(depths):
        (pl_r, fx_r), *_ = np.linalg.lstsq(A, np.array([ms_reuse[L] for L in depths]), rcond=None)
        tok_r = float(fx_r) + hp70["n_layer"] * float(pl_r)
        out["graph_reuse_patch"] = {"what": "the same files with oracle/ref_patches/graph_reuse.patch switched on (LLAMA_MI355_GRAPH_REUSE=1): libllama keeps the previous "
                                            "single-token ggml_cgraph + scheduler allocation while the KV bucket is unchanged",
                                    "ms_per_token_at_depth": {str(L): round(ms_reuse[L], 4) for L in depths}, "ms_per_layer": round(float(pl_r), 4), "ms_fixed": round(float(fx_r), 4),
                                    "ms_per_token_80_layers": round(tok_r, 4), "tokens_per_s_80_layers": round(1e3 / tok_r, 2)}
        if engine_ms_per_token:
            out["graph_reuse_patch"]["frac_of_engine"] = round(engine_ms_per_token / tok_r, 4)
    return out


def parity_bit(tmp, n_layer=8, n_gen=32, n_prompt=16):
    """The correctness bit the graded record carries: the peaked SURVEY-8d fixture at the Llama-3-70B shape with `n_layer` layers
    (tests/_fixtures8d.py: N(0, 1/K) weights through the reference's quantizer, Q4_K_M mixture), 16-token prompt + 32 greedy tokens, decoded by the
    reference's own llama_decode on this host's cores (oracle/_ref, -ngl 0: the checker) and by the resident engine (the thing measured): equal or not."""
    B, drv = _driver()
    if drv is None:
        return {"match": None, "reason": "oracle/_ref not built"}
    import _fixtures8d as F
    flavour = B.best_ref_flavour()
    shape = dict(n_layer=n_layer, n_embd=8192, n_head=64, n_head_kv=8, n_ff=28672, n_vocab=128256, is_70b=True)
    path = os.path.join(tmp, f"pm355_bench_parity_70b_{n_layer}l_peaked.gguf")
    t0 = time.time()
    F.write_model(path, B.Ref(flavour), tag=f"70b{n_layer}", peaked=True, **shape)
    t_gen = time.time() - t0
    try:
        prompt = F.prompt_tokens(shape["n_vocab"], n_prompt)
        tr, lr, _ = B.run_llama_driver(path, prompt, n_gen, ngl=0, n_ctx=256, threads=usable_cores(), flavour=flavour, timeout=600)
        te, le = F.engine_greedy(path, shape, prompt, n_gen, 256)
    finally:
        os.unlink(path)
    d = np.asarray(le, dtype=np.float64) - np.asarray(lr, dtype=np.float64)
    nmse = float((d ** 2).sum() / max((np.asarray(lr, dtype=np.float64) ** 2).sum(), 1e-30))
    n_same = int((np.asarray(te) == np.asarray(tr)).sum())
    return {"match": bool(n_same == n_gen), "tokens_identical": f"{n_same}/{n_gen}", "logits_nmse": float(f"{nmse:.3e}"),
            "fixture": f"peaked SURVEY-8d fixture, Llama-3-70B shape x {n_layer} layers, Q4_K_M through the reference's quantizer, {n_prompt}-token prompt + {n_gen} greedy tokens",
            "reference": f"llama_decode -ngl 0, oracle/_ref {flavour} build", "under_test": "resident engine (pm355_model_*), prompt batch + hipGraph single-token steps",
            "gguf_write_s": round(t_gen, 1)}


def cpu_llama_decode(tmp, path_8b, hp70):
    """The reference's own llama_decode on this host's cores (-ngl 0): (a) the 8B-shaped GGUF of plugin_decode, (b) the metric's
    model shape (Llama-3-70B Q4_K_M) at two reduced depths so that a whole-token time for 80 layers follows from the measured
    per-layer and fixed (embedding + head + graph) costs without writing a 42 GB file."""
    from prima_cpp_amd import gguf as G
    B, drv = _driver()
    if drv is None:
        return None
    cores = usable_cores()
    out = {"cores": cores, "kind": "reference", "binary": os.path.basename(drv),
           "timing": "llama_perf_context (t_eval_ms / n_eval) of llama_decode at -ngl 0"}
    prompt = np.random.default_rng(1234).integers(0, 128256, 16)
    if path_8b and os.path.exists(path_8b):
        _, _, st = B.run_llama_driver(path_8b, prompt, 12, ngl=0, n_ctx=512, threads=cores, timeout=240)
        out["llama3_8b_q4km"] = {"tokens_per_s": round(st["decode_tok_s"], 3), "prompt_tokens_per_s": round(st["prompt_tok_s"], 2)}
    # llama_perf_context (src/llama.cpp:23832-23851: t_eval_ms / n_eval of the single-token evals) on three depths; least-squares line
    depths, ms = (2, 6, 12), {}
    for L in depths:
        p = os.path.join(tmp, f"pm355_bench_llama3_70b_shape_{L}l.gguf")
        G.write_synthetic_model(p, arch=0, n_layer=L, n_embd=hp70["n_embd"], n_head=hp70["n_head"], n_head_kv=hp70["n_head_kv"],
                                n_ff=hp70["n_ff"], n_vocab=hp70["n_vocab"], is_70b=True)
        _, _, st = B.run_llama_driver(p, prompt, 10, ngl=0, n_ctx=512, threads=cores, timeout=300)
        ms[L] = st["perf_t_eval_ms"] / max(st["perf_n_eval"], 1) if st.get("perf_n_eval") else st["decode_ms_avg"]
        os.unlink(p)
    xs, ys = np.array(depths, dtype=np.float64), np.array([ms[L] for L in depths])
    per_layer, fixed = np.polyfit(xs, ys, 1)
    resid = float(np.abs(ys - (fixed + per_layer * xs)).max() / ys.max())
    tok_ms = fixed + hp70["n_layer"] * per_layer
    out["llama3_70b_q4km"] = {"tokens_per_s": round(1e3 / tok_ms, 3), "ms_per_layer": round(float(per_layer), 3), "ms_fixed": round(float(fixed), 3),
                              "fit_max_residual_rel": round(resid, 4), "ms_per_token_at_depth": {str(L): round(ms[L], 2) for L in depths},
                              "method": "llama_perf_context t_eval / n_eval of the reference's llama_decode on 70B-shaped GGUFs of 2, 6 and 12 layers; "
                                        f"least-squares line, token time for {hp70['n_layer']} layers = fixed + n_layer * per-layer (layers alternate the Q4_K_M type mixture with period 2)"}
    return out


def section_prefill_qwen():
    """BASELINE.json config 5's prompt pass on one GPU: Qwen2.5-72B Q6_K, 2048-token prompt (every weight GEMM the Q6_K instantiation)."""
    hq, mq, nq = model_cfg("qwen2.5-72b")
    pq = probe_prefill(hq, mq, 2048, small_batches=(8, 32))
    pq["workload"] = f"{nq}: 2048-token prompt, whole model, 1 GPU (config 5's prefill; the 8-GPU pipelined form is `ring_prefill` of --gpus N)"
    print(json.dumps(pq), flush=True)


def section_long_context(name="llama3-70b", ctxs=(8192, 32768)):
    """Decode at long contexts (engine, the captured per-token graph): the cache is filled by 2048-token prompt chunks on the prefill path, then
    24 greedy tokens are timed at each context; roofline = 8 TB/s over the weights + the F16 K / V^T bytes a token reads there. Next to it the
    single-token attention kernel of that regime alone (attn_flash_mfma.hip), HIP events over launches that rotate through caches of more
    than the 256 MB infinity cache: its achieved fraction of the 8 TB/s KV stream."""
    import prima_cpp_amd.engine as E
    import prima_cpp_amd.ops as P
    from prima_cpp_amd.lib import Q6_K, row_size
    hp, mixture, model_name = model_cfg(name)
    n_ctx = max(ctxs) + 256
    w = E.Window(hp, n_ctx=n_ctx)
    w.fill_synthetic(mixture, seed=1234)
    w.finalize(max_tokens=2048)
    total_w = sum(layer_bytes(hp, mixture)) + row_size(Q6_K, hp["n_embd"]) * hp["n_vocab"] + hp["n_embd"] * 4
    rng = np.random.default_rng(3)
    pos, out = 0, {"workload": f"{model_name} batch-1 greedy decode at long contexts, F16 KV cache, 1 GPU, cache filled by 2048-token prompt chunks", "contexts": {}}
    finite = True
    for ctx in ctxs:
        while pos < ctx - 32:
            n = min(2048, ctx - 32 - pos)
            toks = torch.from_numpy(rng.integers(0, hp["n_vocab"], n).astype(np.int32)).cuda()
            w.decode(tokens=toks, pos0=pos, want_hidden=False, want_logits=False)
            pos += n
        io = torch.zeros(64, dtype=torch.int32, device="cuda")
        io[0] = 7
        w.generate(io, pos, 8, use_graph=True)            # warm-up (captures the graph of this regime)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        w.generate(io, pos + 8, 24, use_graph=True)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / 24
        pos += 32
        finite = finite and bool(((io[:33] >= 0) & (io[:33] < hp["n_vocab"])).all().item())
        kv = hp["n_layer"] * 2 * hp["head_dim"] * hp["n_head_kv"] * 2 * pos
        roof = HBM_PEAK_GBS * 1e9 / (total_w + kv)
        out["contexts"][str(pos)] = {"tokens_per_s": round(1 / dt, 2), "ms_per_token": round(dt * 1e3, 4), "kv_bytes_per_token": kv,
                                     "hbm_roofline_tokens_per_s": round(roof, 1), "frac_of_hbm_roofline": round(1 / dt / roof, 4)}
    out["argmax_in_range"] = finite
    w.close()
    del w
    torch.cuda.empty_cache()
    # the attention kernel of this regime alone, at the model's head shape
    H, Hkv, dh = hp["n_head"], hp["n_head_kv"], hp["head_dim"]
    Nkv = Hkv * dh
    nbuf = max(2, int(600e6 / (n_ctx * Nkv * 4)) + 1)
    g = torch.Generator(device="cuda").manual_seed(5)
    kcs = [torch.randn(n_ctx * Nkv, device="cuda", generator=g).to(torch.float16).view(torch.int16) for _ in range(nbuf)]
    vcs = [torch.randn(n_ctx * Nkv, device="cuda", generator=g).to(torch.float16).view(torch.int16) for _ in range(nbuf)]
    q = torch.randn(1, H * dh, device="cuda", generator=g).to(torch.float16).float()
    scratch = P.attn_split_scratch(H, dh, n_ctx)
    kern = {}
    for ctx in ctxs:
        n_kv = ctx - 7
        pd = torch.tensor([n_kv - 1], dtype=torch.int32, device="cuda")
        grid = 1024
        while grid < n_kv:
            grid *= 2
        grid = min(grid, n_ctx)
        for i in range(nbuf):
            P.attn_cached(q, kcs[i], vcs[i], pd, H, Hkv, dh, n_ctx, dh ** -0.5, max_keys=grid, scratch=scratch)
        torch.cuda.synchronize()
        reps = 10 * nbuf
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(reps):
            P.attn_cached(q, kcs[i % nbuf], vcs[i % nbuf], pd, H, Hkv, dh, n_ctx, dh ** -0.5, max_keys=grid, scratch=scratch)
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / reps
        kvb = 2 * n_kv * Nkv * 2
        kern[str(ctx)] = {"us_per_launch": round(us, 2), "kv_bytes_per_launch": kvb,
                          "roofline": {"bound": "hbm", "achieved": round(kvb / us / 1e3, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(kvb / us / 1e3 / HBM_PEAK_GBS, 4)}}
    # the same kernel over Q8_0 K / V caches (-fa -ctk q8_0 -ctv q8_0: native 34-byte blocks, row-major V; random valid blocks)
    try:
        del kcs, vcs
        torch.cuda.empty_cache()
        row_b = Nkv // 32 * 34
        def q8_cache():
            b = torch.randint(-127, 128, (n_ctx * Nkv // 32, 34), dtype=torch.int8, device="cuda", generator=g)
            d = (torch.rand(n_ctx * Nkv // 32, device="cuda", generator=g) * 0.02 + 0.002).to(torch.float16).view(torch.int16)
            b[:, 0] = (d & 0xFF).to(torch.int8)
            b[:, 1] = ((d >> 8) & 0xFF).to(torch.int8)
            return b.view(-1)
        nb8 = max(2, int(600e6 / (n_ctx * row_b * 2)) + 1)
        k8 = [q8_cache() for _ in range(nb8)]
        v8 = [q8_cache() for _ in range(nb8)]
        flags = P.ATTN_V_ROWMAJOR | P.ATTN_K_Q8_0 | P.ATTN_V_Q8_0
        kern8 = {}
        for ctx in ctxs:
            n_kv = ctx - 7
            dyn = torch.tensor([n_kv - 1, n_kv], dtype=torch.int32, device="cuda")
            grid = 1024
            while grid < n_kv:
                grid *= 2
            grid = min(grid, n_ctx)
            run8 = lambda i: P.attn_cached(q, k8[i % nb8], v8[i % nb8], None, H, Hkv, dh, n_ctx, dh ** -0.5, cell_nkv=dyn, max_keys=grid, flags=flags, scratch=scratch)
            for i in range(nb8):
                run8(i)
            torch.cuda.synchronize()
            reps = 10 * nb8
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(reps):
                run8(i)
            e1.record()
            torch.cuda.synchronize()
            us = e0.elapsed_time(e1) * 1e3 / reps
            kvb = 2 * n_kv * row_b
            kern8[str(ctx)] = {"us_per_launch": round(us, 2), "kv_bytes_per_launch": kvb,
                               "roofline": {"bound": "hbm", "achieved": round(kvb / us / 1e3, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(kvb / us / 1e3 / HBM_PEAK_GBS, 4)}}
        out["attention_kernel_q8_0_kv"] = {"kernel": "attn_flash_mfma_kernel<.., K Q8_0, V Q8_0> (operand slices dequantized on the fly: q * d rounded to F16)", "cells": kern8}
    except Exception as e:
        out["attention_kernel_q8_0_kv"] = {"error": str(e)[:300]}
    out["attention_kernel"] = {"kernel": "attn_flash_mfma_kernel (scores and P.V of a GQA group on v_mfma_f32_16x16x32_f16, keys split over workgroups, in-launch merge)",
                               "shape": f"H {H} Hkv {Hkv} head_dim {dh}", "timing": "HIP events over eager launches on torch's current stream (the launch stream), caches rotated out of the infinity cache",
                               "cells": kern}
    print(json.dumps(out), flush=True)


def main():
    a = parse()
    if a.section == "prefill_qwen":
        assert torch.cuda.is_available(), "bench.py needs a HIP device (no CPU fallback)"
        section_prefill_qwen()
        return
    if a.section.startswith("long_context"):
        assert torch.cuda.is_available(), "bench.py needs a HIP device (no CPU fallback)"
        section_long_context(a.section.split(":")[1] if ":" in a.section else "llama3-70b")
        return
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    assert world == a.gpus, f"--gpus {a.gpus} but WORLD_SIZE={world}"
    assert torch.cuda.is_available(), "bench.py needs a HIP device (no CPU fallback)"
    local = local % torch.cuda.device_count()      # (PM355_DIST_BACKEND=gloo lets several ranks share one GPU for testing)
    torch.cuda.set_device(local)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        backend = os.environ.get("PM355_DIST_BACKEND", "nccl")      # "nccl" IS RCCL on ROCm
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local))
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)

    import prima_cpp_amd.engine as E
    from prima_cpp_amd.ring import partition_layers
    hp, mixture, model_name = model_cfg(a.model)
    from prima_cpp_amd.lib import Q6_K, row_size
    lb = layer_bytes(hp, mixture)
    head_b = row_size(Q6_K, hp["n_embd"]) * hp["n_vocab"] + hp["n_embd"] * 4
    wins = partition_layers(lb, head_b, world)
    lo, hi = wins[rank]
    flags = (E.HAS_EMBD | E.HAS_HEAD) if rank == 0 else 0
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        win = E.Window(hp, lo=lo, hi=hi, flags=flags, n_ctx=a.n_ctx)
        win.fill_synthetic(mixture, seed=1234)
        RING_UBATCH = 512                                  # tokens per hop of the pipelined prompt pass (the reference's n_ubatch)
        # sequences in flight: 2 per rank (round 6: the two-deep schedule of pm355_ring_decode_staggered - every hop travels under the other round's compute);
        # PM355_RING_DEPTH=1 is the lock-step schedule of rounds 4-5 (one sequence per rank, every hop exposed)
        ring_depth = 2 if (world > 1 and os.environ.get("PM355_RING_DEPTH", "2") != "1") else 1
        n_seq = ring_depth * world
        win.finalize(max_tokens=RING_UBATCH if world > 1 else 1, n_seq=n_seq)
        use_graph = not a.no_graph
        # N > 1 over RCCL: the transport is the C one (pm355_ring_*: ncclSend / ncclRecv on the library's communication stream, event
        # hand-off, no host wait per micro-step); PM355_RING_TRANSPORT=torch keeps torch.distributed's batch_isend_irecv instead
        # The ring itself is C (pm355_ring_*: multi-token hand-off, pipelined prompt pass, single-sequence loop); its exchanges travel over
        # RCCL (ncclSend / ncclRecv on the library's communication stream, event hand-off, no host wait per micro-step) or - PM355_DIST_BACKEND=gloo,
        # several ranks on one GPU, or PM355_RING_TRANSPORT=torch - over torch.distributed through the C API's transport callbacks
        c_ring = None
        ring_transport = None
        if world > 1:
            from prima_cpp_amd.ring import CRing
            want = "rccl" if (os.environ.get("PM355_DIST_BACKEND", "nccl") == "nccl" and os.environ.get("PM355_RING_TRANSPORT", "c") == "c") else "torch"
            ok = torch.ones(1, device="cuda" if dist.get_backend() != "gloo" else "cpu")
            if want == "rccl":
                try:
                    c_ring = CRing(rank, world, transport="rccl")
                except Exception as e:                       # every rank must take the same path: agree on it below
                    if os.environ.get("PM355_REQUIRE_RCCL") == "1":     # the first run on real multi-GPU hardware: fail loudly, never measure a fall-back by accident
                        raise RuntimeError(f"[rank {rank}] PM355_REQUIRE_RCCL=1 and the RCCL ring transport could not be created: {e}")
                    print(f"[rank {rank}] RCCL transport unavailable ({e}); falling back to torch.distributed", file=sys.stderr, flush=True)
                    ok.zero_()
                dist.all_reduce(ok, op=dist.ReduceOp.MIN)
                if ok.item() < 1 and os.environ.get("PM355_REQUIRE_RCCL") == "1":
                    raise RuntimeError(f"[rank {rank}] PM355_REQUIRE_RCCL=1: another rank could not create the RCCL ring transport")
                if ok.item() < 1:
                    if c_ring is not None:
                        c_ring.close()
                    c_ring = None
            ring_transport = "rccl" if c_ring is not None else "torch"
            if c_ring is None:
                c_ring = CRing(rank, world, transport="torch")
        if c_ring is None:
            from prima_cpp_amd.ring import CRing
            c_ring = CRing(0, 1, transport="local")          # one window: the same C loop, no communicator
        rng = np.random.default_rng(1234)
        prompt = rng.integers(0, hp["n_vocab"], size=(n_seq, a.prompt))
        prompt[:, 0] = 128000 % hp["n_vocab"]            # BOS first, like llama-bench

        # The decode loop is C (pm355_ring_decode_staggered): `world` sequences in flight one rank apart, a step = every sequence advances one
        # token = `world` micro-steps on every rank; one call enqueues all of them, no interpreter between the steps of the timed region.
        def sync():
            torch.cuda.synchronize()
            if world > 1:
                dist.barrier()
            torch.cuda.synchronize()

        # prompt + warmup, untimed. One GPU: token by token through the decode path. Ring: the prompts go through the ranks as
        # [n_tokens][n_embd] hand-offs, pipelined (pm355_ring_prefill), the last rank returns each prompt's last row to rank 0 for the head
        n_pre = a.prompt + a.warmup
        assert n_pre + 2 * a.steps + 2 <= a.n_ctx, "n_ctx too small for prompt+warmup+steps"
        # a STEP = `world` micro-steps on every rank = `world` tokens leaving rank 0's head (with two sequences per rank in flight every sequence advances one
        # token per two steps; the work per step and GPU is the same as with one)
        ring_prompt = None
        if world > 1:
            toks_d = torch.from_numpy(prompt.astype(np.int32)).cuda() if rank == 0 else None
            rows = torch.zeros((n_seq, hp["n_embd"]), dtype=torch.float32, device="cuda") if rank == 0 else None
            sync()
            tp0 = time.perf_counter()
            c_ring.prefill(win, toks_d, n_seq, a.prompt, min(RING_UBATCH, a.prompt), rows)
            sync()
            ring_prompt = time.perf_counter() - tp0
            first_tok = [None] * n_seq                     # the token each sequence starts its decode with (after the prompt pass)
            if rank == 0:
                am = torch.empty(1, dtype=torch.int32, device="cuda")
                for q in range(n_seq):
                    win.head(rows[q], argmax=am)
                    first_tok[q] = int(am.item())
            win.set_seq(0)                                  # the staggered decode meets the sequences in the order 0, 1, ...
            n_w = max(a.warmup, ring_depth) * world          # (at least one micro-step per sequence in flight: their first tokens are forced)
            c_ring.decode_staggered(win, n_w, forced=(first_tok + [None] * (n_w - n_seq)) if rank == 0 else None, reset=True, use_graph=use_graph)
        else:
            c_ring.decode_staggered(win, n_pre, forced=[int(prompt[0, s_]) if s_ < a.prompt else None for s_ in range(n_pre)], reset=True, use_graph=use_graph)
        sync()
        t0 = time.perf_counter()
        c_ring.decode_staggered(win, a.steps * world, use_graph=use_graph)
        sync()
        t1 = time.perf_counter()
        dt = t1 - t0
        if world > 1:
            t = torch.tensor([dt], dtype=torch.float64, device="cuda" if dist.get_backend() != "gloo" else "cpu")
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            dt = float(t.item())
        c_ring.wait()
        sync()
        # sanity of the synthetic workload: the activations the timed steps produced are finite (a fill that leaves NaNs behind times the
        # same kernels but is not a model)
        lo_ = c_ring.last_output(hp["n_embd"])
        finite = bool(lo_ is not None and torch.isfinite(lo_).all().item())
        # what the timed loop hands its caller after its last step: this rank's output row (seeded weights and prompt: the same from run to run)
        if a.dump_outputs:
            assert lo_ is not None, "no output row to dump (did any timed step run?)"
            os.makedirs(a.dump_outputs, exist_ok=True)
            name = "last_output.npy" if world == 1 else f"last_output_rank{rank}.npy"
            np.save(os.path.join(a.dump_outputs, name), lo_.cpu().numpy().astype(np.float32))

        # The reference's own mode next to the aggregate: ONE sequence in flight, every token once round the ring with the other ranks idle
        # (rank 0 blocked in recv until it returns, src/llama.cpp:18509) - what exposes the hop latency. And the pipelined prompt pass.
        single = ring_pf = None
        if world > 1 and a.full:
            tok1 = torch.tensor([1], dtype=torch.int32, device="cuda") if rank == 0 else None
            for _ in range(3):
                c_ring.single_token(win, 0, tok1)
            c_ring.wait(); sync()
            ts0 = time.perf_counter()
            for _ in range(a.steps):
                c_ring.single_token(win, 0, tok1)
            c_ring.wait(); sync()
            dts = time.perf_counter() - ts0
            n_pf = min(2048, a.n_ctx // 2)
            pf_tok = torch.from_numpy(rng.integers(0, hp["n_vocab"], size=(world, n_pf)).astype(np.int32)).cuda() if rank == 0 else None
            pf_rows = torch.zeros((world, hp["n_embd"]), dtype=torch.float32, device="cuda") if rank == 0 else None
            c_ring.prefill(win, pf_tok, world, n_pf, RING_UBATCH, pf_rows)          # warm: scratch growth, function attributes
            sync()
            tq0 = time.perf_counter()
            c_ring.prefill(win, pf_tok, world, n_pf, RING_UBATCH, pf_rows)
            sync()
            dtp = time.perf_counter() - tq0
            if world > 1:
                t2 = torch.tensor([dts, dtp], dtype=torch.float64, device="cuda" if dist.get_backend() != "gloo" else "cpu")
                dist.all_reduce(t2, op=dist.ReduceOp.MAX)
                dts, dtp = float(t2[0].item()), float(t2[1].item())
            single = {"tokens_per_s": round(a.steps / dts, 3), "ms_per_token": round(dts / a.steps * 1e3, 4), "steps": a.steps,
                      "note": "ONE sequence in flight (pm355_ring_single_token): a token visits every rank in turn, rank 0 waits for the last rank's row "
                              "before the head - the reference's llama_decode ring loop; no speed-up over one GPU is possible, the difference is the hops"}
            ring_pf = {"prompt_tokens": n_pf, "sequences": world, "ubatch": RING_UBATCH, "tokens_per_s": round(world * n_pf / dtp, 1), "ms": round(dtp * 1e3, 2),
                       "first_prompt_pass_s": round(ring_prompt, 4) if ring_prompt is not None else None,
                       "note": "pm355_ring_prefill: chunk g of the prompts on rank r at pipeline step g + r, [ubatch][n_embd] f32 per hop; aggregate over the sequences"}

        tokens = a.steps * world
        value = tokens / dt
        result = None
        if rank == 0:
            total_w = sum(lb) + head_b
            n_kv_mid = a.prompt + a.warmup + a.steps // 2
            kv_b = hp["n_layer"] * 2 * hp["head_dim"] * hp["n_head_kv"] * 2 * n_kv_mid
            result = {
                "metric": "decode_tokens_per_s", "value": round(value, 3), "unit": "tokens/s", "n_gpus": world,
                "steps": a.steps, "warmup": a.warmup, "ms_per_step": round(dt / a.steps * 1e3, 4),
                "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "int8xint4->int32, f32 accumulate",
                "data": "synthetic",
                "config": {"workload": f"{model_name} batch-1 greedy decode, {a.prompt}-token synthetic prompt, "
                                       f"{n_seq} sequence(s) in flight, n_ctx {a.n_ctx}, F16 KV cache",
                           "parallelism": "single GPU" if world == 1 else f"piped-ring layer split pp{world} "
                                          f"(windows {wins}; window bytes per token and rank {[int(sum(lb[lo_:hi_]) + (head_b if i_ == 0 else 0)) for i_, (lo_, hi_) in enumerate(wins)]}; "
                                          f"hop = {hp['n_embd'] * 4} bytes per micro-step and link), {n_seq} sequences in flight ({ring_depth} per rank: "
                                          f"{'a hop is consumed two micro-steps after it was sent' if ring_depth == 2 else 'lock-step, every hop exposed'}), ring in C (pm355_ring_*), "
                                          f"transport agreed on by all ranks: {'RCCL send/recv: comm stream + events, no host wait' if ring_transport == 'rccl' else 'torch.distributed ' + dist.get_backend() + ' through the transport callbacks'}",
                           "weights_bytes_per_token": total_w, "kv_bytes_per_token_mid_run": kv_b,
                           "hip_graph": use_graph, "activations_finite": finite},
                "hbm_roofline_tokens_per_s": round(HBM_PEAK_GBS * 1e9 / total_w * world, 2),
                "frac_of_hbm_roofline_weights_only": round(value * total_w / world / (HBM_PEAK_GBS * 1e9), 4),
                "frac_of_hbm_roofline_weights_plus_kv": round(value * (total_w + kv_b) / world / (HBM_PEAK_GBS * 1e9), 4),
            }
            if single:
                result["single_stream"] = single
                result["ring_prefill"] = ring_pf
            pr = probe_dominant_kernel(win, hp) if a.full else None
            if pr:
                result["roofline"] = {"bound": "hbm", "achieved": round(pr["gbs"], 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                      "frac": round(pr["gbs"] / HBM_PEAK_GBS, 4),
                                      "traffic": pmc_traffic(pr["bytes_per_launch"]),
                                      "kernel": pr["kernel"], "bytes_per_launch": pr["bytes_per_launch"],
                                      "avg_launch_us": round(pr["avg_us"], 2), "launched_as": pr["launch"],
                                      "measured_stream_read_peak": round(pr["stream_read_gbs"], 1) if pr.get("stream_read_gbs") else None,
                                      "frac_of_measured_peak": round(pr["gbs"] / pr["stream_read_gbs"], 4) if pr.get("stream_read_gbs") else None}
            if world == 1 and a.full and a.prefill > 0:
                try:
                    result["prefill"] = probe_prefill(hp, mixture, a.prefill)
                except Exception as e:
                    result["prefill"] = {"error": str(e)}
            if world == 1 and a.full and not a.no_cpu_baseline:
                try:
                    cb = cpu_baseline(hp, mixture, a.cpu_seconds)
                except Exception as e:                       # the baseline is a reported extra, never fatal
                    cb = {"value": None, "unit": "tokens/s", "cores": os.cpu_count(), "kind": "reference", "sample": f"failed: {e}"}
                if cb:
                    if cb.get("value"):
                        cb["value"] = round(cb["value"], 4)
                    result["cpu_baseline"] = cb
        win.close()
        win = None
        if rank == 0 and world == 1 and a.full and not a.no_extras:
            torch.cuda.empty_cache()
            extras = []
            for name in ("llama3-8b", "qwen2.5-72b"):
                if name == a.model:
                    continue
                try:
                    extras.append(extra_config(name))
                except Exception as e:
                    extras.append({"workload": name, "error": str(e)[:300]})
            result["extra_configs"] = extras
            # BASELINE.json config 5's prompt pass on one GPU: Qwen2.5-72B Q6_K, 2048-token prompt (every weight GEMM the Q6_K instantiation)
            # (in a process of its own: the newest leg must not be able to take the driver line down with it)
            try:
                import subprocess
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--section", "prefill_qwen"], capture_output=True, text=True, timeout=420)
                line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
                result["prefill_qwen25_72b_q6k"] = json.loads(line[-1]) if line else {"error": f"rc {r.returncode}: {r.stderr[-400:]}"}
            except Exception as e:
                result["prefill_qwen25_72b_q6k"] = {"error": str(e)[-400:]}
            # decode at 8k / 32k cells (70B and config 5's model) + the long-context attention kernel against its KV stream - each in a process of its own
            for key, mdl in (("long_context", "llama3-70b"), ("long_context_qwen25_72b", "qwen2.5-72b")):
                try:
                    import subprocess
                    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--section", "long_context:" + mdl], capture_output=True, text=True, timeout=420)
                    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
                    result[key] = json.loads(line[-1]) if line else {"error": f"rc {r.returncode}: {r.stderr[-400:]}"}
                except Exception as e:
                    result[key] = {"error": str(e)[-400:]}
            try:
                pb = parity_bit(a.tmp)
            except Exception as e:
                pb = {"match": None, "reason": str(e)[-400:]}
            result["config"]["greedy_tokens_match_reference"] = pb.get("match")
            result["parity_check"] = pb
            try:
                result["weight_streaming"] = streaming_probe()
            except Exception as e:
                result["weight_streaming"] = {"error": str(e)[-400:]}
            path_8b = None
            try:
                pd, path_8b = plugin_decode(a.tmp)
                if pd:
                    result["plugin_decode"] = pd
                    result["plugin_decode_tokens_per_s"] = pd["tokens_per_s"]
            except Exception as e:
                result["plugin_decode"] = {"error": str(e)[-600:]}
            try:
                import prima_cpp_amd.engine as E3
                p70 = plugin_decode_70b(a.tmp, E3.LLAMA3_70B, result["ms_per_step"] if a.model == "llama3-70b" else None)
                if p70:
                    result["plugin_decode_70b"] = p70
            except Exception as e:
                result["plugin_decode_70b"] = {"error": str(e)[-600:]}
            if not a.no_cpu_baseline:
                try:
                    import prima_cpp_amd.engine as E2
                    ld = cpu_llama_decode(a.tmp, path_8b, E2.LLAMA3_70B)
                    if ld and "cpu_baseline" in result:
                        result["cpu_baseline"]["llama_decode"] = ld
                        if ld.get("llama3_70b_q4km") and a.model == "llama3-70b":
                            # the whole-token number through the reference's own driver replaces the mat-vec-only estimate as `value`
                            result["cpu_baseline"]["matvec_only_tokens_per_s"] = result["cpu_baseline"]["value"]
                            result["cpu_baseline"]["value"] = ld["llama3_70b_q4km"]["tokens_per_s"]
                            result["cpu_baseline"]["sample"] = ("reference llama_decode (-ngl 0, unmodified libllama + ggml CPU backend built from /root/reference, "
                                                                f"{ld['cores']} threads, llama_perf_context timing) on Llama-3-70B-shaped Q4_K_M GGUFs of 2, 6 and 12 layers, least-squares line to 80 layers "
                                                                "(see llama_decode.llama3_70b_q4km.method); matvec_only_tokens_per_s = " + result["cpu_baseline"]["sample"])
                except Exception as e:
                    if "cpu_baseline" in result:
                        result["cpu_baseline"]["llama_decode"] = {"error": str(e)[-600:]}
            if path_8b and os.path.exists(path_8b):
                os.unlink(path_8b)
    if win is not None:
        win.close()
    if c_ring is not None:
        torch.cuda.synchronize()
        c_ring.close()
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
