"""Parity at BASELINE.json shapes: one Llama-3-70B-shaped and one Qwen2.5-72B-shaped LAYER
(E 8192, 64 heads / 8 KV heads, head_dim 128, F 28672 / 29568 with the Q8_0 ffn_down the reference falls back to for
K % 256 != 0, Q5_K / Q6_K attn_v) through the engine - single-token decode against the oracle, 80-token MFMA prefill + decode, 40-token small-batch step (integer matrix cores, two passes)
against the reference CPU backend itself (oracle/_ref, AVX2 build, multi-threaded: the scalar oracle needs ~50 s for 32 tokens
of a 70B layer) - and the two dominant decode launches (gate/up PAIR kernel, 3-job mixed-type QKV) at K = 8192 with the real
row counts against oracle.mul_mat."""
import os
import zlib

import numpy as np
import pytest

from _bind import Q4_K, Q5_K, Q6_K, Q8_0, Ref, have_ref, rand_blocks, tiny_model

pytestmark = pytest.mark.gpu


def _nmse(a, b):
    a = np.asarray(a, dtype=np.float64).ravel()
    b = np.asarray(b, dtype=np.float64).ravel()
    return float(((a - b) ** 2).sum() / max((b ** 2).sum(), 1e-30))


@pytest.fixture(scope="module")
def E():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    import prima_cpp_amd.engine as eng
    eng.torch = torch
    return eng


@pytest.fixture(scope="module")
def P():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    import prima_cpp_amd.ops as ops
    ops.torch = torch
    return ops


def _hp(d):
    return dict(arch=d.arch, n_layer=d.n_layer, n_embd=d.n_embd, n_head=d.n_head, n_head_kv=d.n_head_kv,
                head_dim=d.head_dim, n_ff=d.n_ff, n_vocab=d.n_vocab, rms_eps=d.rms_eps, rope_freq_base=d.rope_freq_base)


SHAPES = {
    # name: (arch, n_ff, attn_v type, ffn_down type, output type)
    "llama3_70b": (0, 28672, Q5_K, Q6_K, Q6_K),        # Q4_K_M: attn_v Q5_K (MODEL_70B) / Q6_K, ffn_down Q6_K on "more bits" layers
    "llama3_70b_morebits": (0, 28672, Q6_K, Q4_K, Q6_K),
    "qwen25_72b_q6k": (1, 29568, Q6_K, Q8_0, Q6_K),    # all Q6_K; ffn_down falls back to Q8_0 (29568 % 256 != 0, src/llama.cpp:19547)
}


@pytest.mark.parametrize("name", list(SHAPES) + ["llama3_70b+flash"])
def test_model_shaped_layer_decode_and_prefill(E, oracle, name, monkeypatch):
    torch = E.torch
    if name.endswith("+flash"):
        # the decode step at position 32 then runs the long-context path at the model's GQA shape (8 query heads per KV head): the matrix-core
        # kernel over cached cells (attn_flash_mfma.hip) where the QKV epilogue serves the rope mode, else the round-2 kernel (attn_flash.hip)
        monkeypatch.setenv("PM355_ATTN_SPLIT_MIN", "16")
        name = name[:-6]
    arch, n_ff, tv, td, tout = SHAPES[name]
    rng = np.random.default_rng(zlib.crc32(name.encode()) % 1000)     # (str hash() is salted per process: a different model every run)
    types = {"attn_v": tv, "ffn_down": td, "output": tout}
    if name.startswith("qwen"):
        types.update({k: Q6_K for k in ("attn_q", "attn_k", "attn_output", "ffn_gate", "ffn_up", "token_embd")})
    d = tiny_model(rng, arch=arch, n_layer=1, n_embd=8192, n_head=64, n_head_kv=8, n_ff=n_ff, n_vocab=512, n_ctx=128,
                   rope_freqs=(arch == 0), types=types)
    w = E.Window(_hp(d), n_ctx=128)
    w.load_desc(d)
    w.finalize(max_tokens=80)
    toks = rng.integers(0, d.n_vocab, 81).astype(np.int32)

    # (1) single-token decode (fused 5-launch path: 3-job QKV, fused attention, wo, PAIR gate/up, down) vs the ORACLE
    ho = oracle.model_new(d)
    hid, lg, _ = w.decode(tokens=torch.from_numpy(toks[:1]).cuda(), pos0=0, want_argmax=True)
    h_ref, l_ref = oracle.model_eval(ho, d, tokens=toks[:1], pos0=0)
    oracle.model_free(ho)
    n1, n2 = _nmse(hid.cpu().numpy(), h_ref), _nmse(lg.cpu().numpy(), l_ref)
    print(f"\n[{name}] decode vs oracle: hidden NMSE {n1:.2e}, logits NMSE {n2:.2e}")
    assert n1 < 1e-6 and n2 < 1e-4

    # (2) 80-token prefill (MFMA GEMMs + MFMA attention, GQA 8:1) then a decode step at position 80 (fused attention over 81
    #     cached keys) vs the REFERENCE CPU backend (unmodified ggml, AVX2 build) on the same weights
    if not have_ref("avx2"):
        pytest.skip("oracle/_ref/libggml_ref_avx2.so not built")
    ref = Ref("avx2")
    hr = ref.model_new(d)
    thr = max(1, min(16, len(os.sched_getaffinity(0))))
    w.kv_clear()
    hid_p, lg_p, _ = w.decode(tokens=torch.from_numpy(toks[:80]).cuda(), pos0=0, want_argmax=True)
    hp_ref, lp_ref = ref.model_eval(hr, d, tokens=toks[:80], pos0=0, n_threads=thr)
    hid_d, lg_d, _ = w.decode(tokens=torch.from_numpy(toks[80:]).cuda(), pos0=80, want_argmax=True)
    hd_ref, ld_ref = ref.model_eval(hr, d, tokens=toks[80:], pos0=80, n_threads=thr)
    ref.model_free(hr)
    a, b = _nmse(hid_p.cpu().numpy(), hp_ref), _nmse(lg_p.cpu().numpy(), lp_ref)
    c, e = _nmse(hid_d.cpu().numpy(), hd_ref), _nmse(lg_d.cpu().numpy(), ld_ref)
    print(f"[{name}] prefill(80) vs reference CPU: hidden NMSE {a:.2e}, logits NMSE {b:.2e}; decode@80: hidden {c:.2e}, logits {e:.2e}")
    # the MFMA path multiplies F16-rounded activations (no Q8_K re-quantization): the reference's own backend tolerance for
    # MUL_MAT is NMSE <= 5e-4 (tests/test-backend-ops.cpp:1660); whole layer + head stays far below it
    assert a < 5e-4 and b < 1e-3
    assert c < 5e-4 and e < 1e-3

    # (3) 24-token batch (up to 32 tokens take this path - speculative / parallel-sequence / short-prompt regime): mmq_i8.hip for the Q4_K / Q6_K matrices - the
    #     reference's integer arithmetic on Q8_K activations, so it sits at mat-vec distance from the CPU backend, not at F16-GEMM distance
    w.kv_clear()
    hr = ref.model_new(d)
    hid_s, lg_s, _ = w.decode(tokens=torch.from_numpy(toks[:24]).cuda(), pos0=0, want_argmax=True)
    hs_ref, ls_ref = ref.model_eval(hr, d, tokens=toks[:24], pos0=0, n_threads=thr)
    ref.model_free(hr)
    f, g2 = _nmse(hid_s.cpu().numpy(), hs_ref), _nmse(lg_s.cpu().numpy(), ls_ref)
    print(f"[{name}] small batch (24) vs reference CPU: hidden NMSE {f:.2e}, logits NMSE {g2:.2e}")
    # (what is left is the multi-token attention kernel's f32 softmax.V against the reference's F16-rounded probabilities: the distance
    #  is the same, 4.3e-6 / 1.3e-5, with PM355_NO_MMQ_I8=1, i.e. on the mat-vec path)
    # (the Qwen2.5-72B shape's Q8_0 ffn_down - K = 29568 is no multiple of 256 - is served by mmq_i8.hip's Q8_0 instantiation since round 4: Q8_0
    #  activations on the integer matrix cores, ggml_vec_dot_q8_0_q8_0's arithmetic, and the batch stays at the same distance)
    assert f < 2e-5 and g2 < 2e-4
    # (3b) 40-token batch: since round 6 batches of 33..64 tokens take the prompt GEMM with 64-token tiles (mmq_pf.hip: 25 ms against 30-36 for two integer
    #      passes on the 70B model) - F16 activations, the prompt's parity tier (the same bound as the 80-token prompt above)
    w.kv_clear()
    hr = ref.model_new(d)
    hid_m, lg_m, _ = w.decode(tokens=torch.from_numpy(toks[:40]).cuda(), pos0=0, want_argmax=True)
    hm_ref, lm_ref = ref.model_eval(hr, d, tokens=toks[:40], pos0=0, n_threads=thr)
    ref.model_free(hr)
    fm, gm = _nmse(hid_m.cpu().numpy(), hm_ref), _nmse(lg_m.cpu().numpy(), lm_ref)
    print(f"[{name}] 40-token batch (prompt GEMM, 64-token tiles) vs reference CPU: hidden NMSE {fm:.2e}, logits NMSE {gm:.2e}")
    assert fm < 5e-4 and gm < 1e-3
    # (4) 3-token step: wq | wk | wv and ffn_gate | ffn_up as one multi-job launch each (from 2 tokens), wo / down single launches (from 3)
    w.kv_clear()
    hr = ref.model_new(d)
    hid_3, lg_3, _ = w.decode(tokens=torch.from_numpy(toks[:3]).cuda(), pos0=0, want_argmax=True)
    h3_ref, l3_ref = ref.model_eval(hr, d, tokens=toks[:3], pos0=0, n_threads=thr)
    ref.model_free(hr)
    f3, g3 = _nmse(hid_3.cpu().numpy(), h3_ref), _nmse(lg_3.cpu().numpy(), l3_ref)
    print(f"[{name}] 3-token step vs reference CPU: hidden NMSE {f3:.2e}, logits NMSE {g3:.2e}")
    # (llama3_70b: 2.4e-6 - with wo / down on the multi-column mat-vec instead it was 8e-14, i.e. every Q8_K rounding decision identical to the
    #  CPU backend's; the small-batch kernel itself agrees with the mat-vec to NMSE 1e-14 on these shapes, tools/small_vs_vec_check.py, so what
    #  is left are activation roundings that flip on f32-summation-order noise. The reference's own MUL_MAT tolerance is NMSE 5e-4.)
    assert f3 < 5e-5 and g3 < 3e-4
    w.close()


def test_pair_and_qkv_kernels_at_model_k(P, oracle):
    """The dominant kernel (Q4_K gate/up PAIR, N = 28672) and the 3-job mixed-type QKV launch (Q4_K 8192 + Q4_K 1024 + Q5_K/Q6_K 1024
    rows) at K = 8192 against oracle.mul_mat (identical integer partials, float summation order only)."""
    torch = P.torch
    rng = np.random.default_rng(8192)
    K = 8192
    x = rng.normal(0, 1, (1, K)).astype(np.float32)
    nw = (1 + rng.normal(0, 0.05, K)).astype(np.float32)
    xn = oracle.rms_norm(x, nw, 1e-5)
    xd, nwd = torch.from_numpy(x).cuda(), torch.from_numpy(nw).cuda()
    # PAIR: y = silu(Wg.xn) * (Wu.xn)
    N = 28672
    bg, bu = rand_blocks(Q4_K, N, K, rng), rand_blocks(Q4_K, N, K, rng)
    wg, wu = P.upload_weight(Q4_K, bg, K, N), P.upload_weight(Q4_K, bu, K, N)
    y = P.mul_mat_vec_fused([wg], xd, norm_w=nwd, eps=1e-5, w2s=[wu])[0].cpu().numpy()
    want = oracle.silu_mul(oracle.mul_mat(Q4_K, bg, K, N, xn), oracle.mul_mat(Q4_K, bu, K, N, xn))[0]
    assert np.allclose(y, want, rtol=1e-4, atol=1e-4), np.abs(y - want).max()
    del wg, wu
    # QKV: three jobs, two quant types, bias on each (Qwen2 graph shape)
    for tv in (Q5_K, Q6_K):
        Ns = (8192, 1024, 1024)
        ts = (Q4_K, Q4_K, tv)
        blocks = [rand_blocks(t, n, K, rng) for t, n in zip(ts, Ns)]
        ws = [P.upload_weight(t, b, K, n) for t, b, n in zip(ts, blocks, Ns)]
        bias = [rng.normal(0, 1, n).astype(np.float32) for n in Ns]
        ys = P.mul_mat_vec_fused(ws, xd, norm_w=nwd, eps=1e-5, biases=[torch.from_numpy(b).cuda() for b in bias])
        for t, bl, n, b, yy in zip(ts, blocks, Ns, bias, ys):
            want = oracle.mul_mat(t, bl, K, n, xn)[0] + b
            assert np.allclose(yy.cpu().numpy(), want, rtol=2e-5, atol=2e-5), (t, np.abs(yy.cpu().numpy() - want).max())


@pytest.mark.parametrize("tv,T", [(Q5_K, 5), (Q5_K, 16), (Q6_K, 9), (Q6_K, 24), (Q4_K, 2), (Q4_K, 32)])
def test_small_batch_rope_and_kv_store_in_the_qkv_epilogue_same_bits(E, tv, T, monkeypatch):
    """Round 6: small batches (2..32 tokens, NORM rope) rotate q / k and store K / V in the epilogue of the wq | wk | wv small-batch launch (mmq_i8.hip EPI
    instantiations: the three-job launch, and the two-part grid when wv has another quant type) instead of a rope_kv_store launch of their own
    (ggml_compute_forward_rope_f32 ggml.c:14224 + llm_build_kv_store src/llama.cpp:9688): hidden rows and logits of the batch AND of the next single token -
    which reads the cache the batch wrote - are the same BITS as with PM355_SMALL_ROPE_EPI=0."""
    torch = E.torch
    arch, n_ff = 0, 28672
    rng = np.random.default_rng(1000 + 37 * tv + T)
    types = {"attn_v": tv, "ffn_down": Q6_K, "output": Q6_K}      # wv Q4_K: all three of one type = the three-job launch; Q5_K / Q6_K: the two-part grid
    d = tiny_model(rng, arch=arch, n_layer=1, n_embd=8192, n_head=64, n_head_kv=8, n_ff=n_ff, n_vocab=512, n_ctx=128, rope_freqs=True, types=types)
    toks = rng.integers(0, d.n_vocab, T + 1).astype(np.int32)
    outs = []
    for epi in ("1", "0"):
        monkeypatch.setenv("PM355_SMALL_ROPE_EPI", epi)
        w = E.Window(_hp(d), n_ctx=128)
        w.load_desc(d)
        w.finalize(max_tokens=32)
        w.decode(tokens=torch.from_numpy(toks[:3]).cuda(), pos0=0)                        # cells 0..2, so that the batch starts at a position > 0
        hb, lb, _ = w.decode(tokens=torch.from_numpy(toks[:T]).cuda(), pos0=3, want_argmax=True)
        h1, l1, _ = w.decode(tokens=torch.from_numpy(toks[T:T + 1]).cuda(), pos0=3 + T, want_argmax=True)
        outs.append((hb.clone(), lb.clone(), h1.clone(), l1.clone()))
        w.close()
    for a, b in zip(*outs):
        assert torch.isfinite(a).all()
        assert torch.equal(a, b)


def test_small_batch_tables_reused_across_wq_wk_and_then_wv_alone(E, monkeypatch):
    """A 20-token step through layers whose wv is Q5_K next to Q4_K wq / wk (K = 512): the two-part grid refuses it (Q5_K: 16 tokens), so wq | wk go out as one
    multi-job launch and wv alone, in two passes of 16 and 4 tokens over the SAME activation tables (tables_ready: no prologue launch in between; the second pass
    reads table slots 16..19). Same tokens, and hidden rows / logits at the distance of PM355_NO_MMQ_I8=1 - which sends 20 tokens to the F16 prompt GEMM, so the
    bound is that tier's (test_model_shaped_layer_decode_and_prefill (2), (3b): NMSE 5e-4 hidden, 1e-3 logits); the next single token reads the cache the step wrote."""
    torch = E.torch
    rng = np.random.default_rng(2020)
    d = tiny_model(rng, arch=0, n_layer=2, n_embd=512, n_head=4, n_head_kv=2, n_ff=1024, n_vocab=320, n_ctx=64,
                   types={"attn_v": Q5_K, "ffn_down": Q6_K, "output": Q6_K})
    toks = rng.integers(0, d.n_vocab, 21).astype(np.int32)
    outs = []
    for off in ("0", "1"):
        monkeypatch.setenv("PM355_NO_MMQ_I8", off)
        w = E.Window(_hp(d), n_ctx=64)
        w.load_desc(d)
        w.finalize(max_tokens=32)
        hb, lb, ab = w.decode(tokens=torch.from_numpy(toks[:20]).cuda(), pos0=0, want_argmax=True)
        h1, l1, a1 = w.decode(tokens=torch.from_numpy(toks[20:]).cuda(), pos0=20, want_argmax=True)
        outs.append([t.cpu().numpy().copy() for t in (hb, lb, ab, h1, l1, a1)])
        w.close()
    (hb, lb, ab, h1, l1, a1), (hb0, lb0, ab0, h10, l10, a10) = outs
    f, g = _nmse(hb, hb0), _nmse(lb, lb0)
    f1, g1 = _nmse(h1, h10), _nmse(l1, l10)
    print(f"\n20-token step vs PM355_NO_MMQ_I8=1: hidden NMSE {f:.2e}, logits NMSE {g:.2e}; next token: hidden {f1:.2e}, logits {g1:.2e}")
    assert np.isfinite(hb).all() and np.isfinite(lb).all()
    assert np.array_equal(ab, ab0) and np.array_equal(a1, a10)
    assert f < 5e-4 and g < 1e-3 and f1 < 5e-4 and g1 < 1e-3
