"""GPU parity of the engine (resident layer window) against the CPU oracle on tiny Llama / Qwen2
shaped models: prefill + decode, KV cache contents, window hand-off, graph replay, greedy loop."""
import numpy as np
import pytest

from _bind import Q4_K, Q6_K, Q8_0, tiny_model

pytestmark = pytest.mark.gpu


def _nmse(a, b):
    a = np.asarray(a, dtype=np.float64).ravel()
    b = np.asarray(b, dtype=np.float64).ravel()
    return float(((a - b) ** 2).sum() / max((b ** 2).sum(), 1e-30))


def _hp(d):
    return dict(arch=d.arch, n_layer=d.n_layer, n_embd=d.n_embd, n_head=d.n_head, n_head_kv=d.n_head_kv,
                head_dim=d.head_dim, n_ff=d.n_ff, n_vocab=d.n_vocab, rms_eps=d.rms_eps, rope_freq_base=d.rope_freq_base,
                rope_freq_scale=d.rope_freq_scale)


@pytest.fixture(scope="module")
def E():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    import prima_cpp_amd.engine as eng
    eng.torch = torch
    return eng


def _quantizer():
    from _bind import Ref, have_ref
    return Ref("scalar").quantize_weights if have_ref("scalar") else None


@pytest.mark.parametrize("arch", [0, 1])
def test_window_prefill_and_decode_vs_oracle(E, oracle, arch):
    torch = E.torch
    rng = np.random.default_rng(31 + arch)
    d = tiny_model(rng, arch=arch, n_layer=2, n_embd=256, n_head=4, n_head_kv=2, n_ff=512, n_vocab=320, n_ctx=64,
                   rope_freqs=(arch == 0), quantize=_quantizer())
    w = E.Window(_hp(d), n_ctx=64)
    w.load_desc(d)
    w.finalize(max_tokens=8)
    ho = oracle.model_new(d)
    toks = rng.integers(0, d.n_vocab, 9).astype(np.int32)
    steps = [(toks[:5], 0), (toks[5:6], 5), (toks[6:7], 6), (toks[7:9], 7)]
    for tk, p0 in steps:
        hid, lg, am = w.decode(tokens=torch.from_numpy(tk).cuda(), pos0=p0, want_argmax=True)
        h_ref, l_ref = oracle.model_eval(ho, d, tokens=tk, pos0=p0)
        # north_star: logits within 1e-3 relative; whole-stack metric = NMSE (reference: test-backend-ops)
        assert _nmse(hid.cpu().numpy(), h_ref) < 1e-3
        assert _nmse(lg.cpu().numpy(), l_ref) < 1e-3
        assert int(am.item()) == int(np.argmax(lg.cpu().numpy()))
    # layer-0 KV cache: K rows are rope(f32)->f16, V rows plain f16: compare as floats (cos/sin <= 2 ulp apart)
    for which in (0, 1):
        a = w.kv(0, which).view(np.float16).astype(np.float32)
        b = oracle.model_kv(ho, d, 0, which).view(np.float16).astype(np.float32)
        assert _nmse(a, b) < 1e-6
        if which == 1:
            assert np.array_equal(w.kv(0, 1), oracle.model_kv(ho, d, 0, 1))     # V path has no transcendental: bit-exact
    oracle.model_free(ho)
    w.close()


@pytest.mark.parametrize("arch", [0, 1])
def test_window_prefill_and_decode_with_linear_rope_scaling(E, oracle, arch):
    """test_window_prefill_and_decode_vs_oracle with rope_freq_scale = 0.25 (linear scaling by 4, `--rope-freq-scale`), under the same tolerances:
    that test's 5-token prefill, a small-batch step of 5 tokens at position 5 (the mmq_i8 QKV epilogue with a 5-token cos / sin table), then
    single-token steps (the mat-vec QKV epilogue with the per-token table). Then a prompt of 40 tokens in a fresh window (more than the small-batch
    path takes: rope_kv_store_kernel + the F16-tile GEMMs) under the tolerance of test_prefill_mfma_path_vs_oracle, 2e-3 - that path measures
    ~1e-3 with and without scaling. With freq_scale ignored anywhere, the K rows of that path are rotated by four times the angle."""
    torch = E.torch
    rng = np.random.default_rng(131 + arch)
    d = tiny_model(rng, arch=arch, n_layer=2, n_embd=256, n_head=4, n_head_kv=2, n_ff=512, n_vocab=320, n_ctx=64,
                   rope_freqs=(arch == 0), quantize=_quantizer(), rope_freq_scale=0.25)
    w = E.Window(_hp(d), n_ctx=64)
    w.load_desc(d)
    w.finalize(max_tokens=8)
    ho = oracle.model_new(d)
    toks = rng.integers(0, d.n_vocab, 41).astype(np.int32)
    steps = [(toks[:5], 0), (toks[5:10], 5), (toks[10:11], 10), (toks[11:12], 11), (toks[12:14], 12)]
    for tk, p0 in steps:
        hid, lg, am = w.decode(tokens=torch.from_numpy(tk).cuda(), pos0=p0, want_argmax=True)
        h_ref, l_ref = oracle.model_eval(ho, d, tokens=tk, pos0=p0)
        assert _nmse(hid.cpu().numpy(), h_ref) < 1e-3, p0
        assert _nmse(lg.cpu().numpy(), l_ref) < 1e-3, p0
        assert int(am.item()) == int(np.argmax(lg.cpu().numpy()))
    for which in (0, 1):
        a = w.kv(0, which).view(np.float16).astype(np.float32)
        b = oracle.model_kv(ho, d, 0, which).view(np.float16).astype(np.float32)
        assert _nmse(a, b) < 1e-6       # (V does not pass through the rotation: its bit-exactness is test_window_prefill_and_decode_vs_oracle's)
    k_scaled = w.kv(0, 0).view(np.float16).astype(np.float32)[:14 * d.head_dim * d.n_head_kv]
    w.close()
    # the prompt path
    w = E.Window(_hp(d), n_ctx=64)
    w.load_desc(d)
    w.finalize(max_tokens=40)
    oracle.model_kv_clear(ho)
    for tk, p0 in [(toks[:40], 0), (toks[40:41], 40)]:
        hid, lg, _ = w.decode(tokens=torch.from_numpy(tk).cuda(), pos0=p0)
        h_ref, l_ref = oracle.model_eval(ho, d, tokens=tk, pos0=p0)
        assert _nmse(hid.cpu().numpy(), h_ref) < 2e-3, p0
        assert _nmse(lg.cpu().numpy(), l_ref) < 2e-3, p0
    a = w.kv(0, 0).view(np.float16).astype(np.float32)
    b = oracle.model_kv(ho, d, 0, 0).view(np.float16).astype(np.float32)
    assert _nmse(a, b) < 2e-3
    oracle.model_free(ho)
    w.close()
    # the scaling is in effect: the same K rows without it are far away (a test that lost its parameter on the way would pass everything above)
    d.rope_freq_scale = 1.0
    h1 = oracle.model_new(d)
    for tk, p0 in steps:
        oracle.model_eval(h1, d, tokens=tk, pos0=p0)
    b1 = oracle.model_kv(h1, d, 0, 0).view(np.float16).astype(np.float32)[:k_scaled.size]
    assert _nmse(k_scaled, b1) > 1e-2
    oracle.model_free(h1)


def test_two_windows_hand_off_equals_single_window(E):
    """Piped-ring split: window A = layers [0,1) + embd, window B = layers [1,2) + head. The activation
    handed from A to B must reproduce the single-window result exactly (same kernels, same order)."""
    torch = E.torch
    rng = np.random.default_rng(33)
    d = tiny_model(rng, arch=0, n_layer=2, n_embd=256, n_head=4, n_head_kv=2, n_ff=512, n_vocab=320, n_ctx=64, rope_freqs=True)
    full = E.Window(_hp(d), n_ctx=64)
    full.load_desc(d); full.finalize(4)
    a = E.Window(_hp(d), lo=0, hi=1, flags=E.HAS_EMBD, n_ctx=64)
    a.load_desc(d); a.finalize(4)
    b = E.Window(_hp(d), lo=1, hi=2, flags=E.HAS_HEAD, n_ctx=64)
    b.load_desc(d); b.finalize(4)
    toks = torch.from_numpy(rng.integers(0, d.n_vocab, 4).astype(np.int32)).cuda()
    for tk, p0 in ((toks[:3], 0), (toks[3:4], 3)):
        hf, lf, _ = full.decode(tokens=tk, pos0=p0)
        ha, _, _ = a.decode(tokens=tk, pos0=p0, want_logits=False)
        hb, lb, _ = b.decode(x_in=ha, pos0=p0)
        assert torch.equal(hf, hb) and torch.equal(lf, lb)
    for w in (full, a, b):
        w.close()


def test_graph_replay_and_device_greedy_loop(E, oracle):
    torch = E.torch
    rng = np.random.default_rng(34)
    d = tiny_model(rng, arch=0, n_layer=2, n_embd=256, n_head=4, n_head_kv=2, n_ff=512, n_vocab=320, n_ctx=64, rope_freqs=True)
    w = E.Window(_hp(d), n_ctx=64)
    w.load_desc(d); w.finalize(4)
    n = 12
    first = int(rng.integers(0, d.n_vocab))
    outs = []
    for use_graph in (False, True):
        w.kv_clear()
        io = torch.zeros(n + 1, dtype=torch.int32, device="cuda")
        io[0] = first
        w.generate(io, 0, n, use_graph=use_graph)
        torch.cuda.synchronize()
        outs.append(io.cpu().numpy())
    assert np.array_equal(outs[0], outs[1])               # graph replay == eager launches, token for token
    # greedy parity with the CPU oracle; a flat synthetic logit distribution may flip near-ties, so
    # follow the oracle only while its top-1/top-2 margin is above the observed logit noise
    ho = oracle.model_new(d)
    tok = first
    for i in range(n):
        _, lg = oracle.model_eval(ho, d, tokens=np.array([tok], dtype=np.int32), pos0=i)
        top2 = np.sort(lg)[-2:]
        if top2[1] - top2[0] < 1e-2 * max(1.0, abs(top2[1])):
            break
        assert outs[0][i + 1] == int(np.argmax(lg)), (i, outs[0][: i + 2])
        tok = int(np.argmax(lg))
    oracle.model_free(ho)
    w.close()


def test_step_with_external_activation_buffers(E):
    """pm355_model_step: position in device memory, x_in/x_out owned by the caller (ring transport buffers)."""
    torch = E.torch
    rng = np.random.default_rng(35)
    d = tiny_model(rng, arch=1, n_layer=2, n_embd=256, n_head=4, n_head_kv=2, n_ff=512, n_vocab=320, n_ctx=64)
    w = E.Window(_hp(d), lo=0, hi=2, flags=0, n_ctx=64)
    w.load_desc(d); w.finalize(1)
    x = torch.randn(5, 1, d.n_embd, device="cuda")
    ref = []
    for i in range(5):
        h, _, _ = w.decode(x_in=x[i], pos0=i, want_logits=False)
        ref.append(h.clone())
    w.kv_clear()
    xin = torch.empty(1, d.n_embd, device="cuda"); xout = torch.empty(1, d.n_embd, device="cuda")
    w.set_pos(0)
    for i in range(5):
        xin.copy_(x[i])
        w.step(x_in=xin, x_out=xout, advance=1, use_graph=True)
        assert torch.equal(xout, ref[i])
    w.close()


@pytest.mark.parametrize("name", ["llama", "qwen2"])
def test_golden_greedy_decode_vs_reference(E, name):
    """The committed golden run of the REFERENCE CPU backend (tests/golden/tiny_*_decode.npz): same GGUF-order weights,
    same prompt; logits NMSE < 1e-3 per step (teacher-forced) and greedy-token parity wherever the reference's own
    top-1/top-2 margin is above the logit noise."""
    import os
    from _bind import desc_from_arrays
    torch = E.torch
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", f"tiny_{name}_decode.npz"))
    d = desc_from_arrays(z)
    w = E.Window(_hp(d), n_ctx=int(d.n_ctx))
    w.load_desc(d)
    w.finalize(max_tokens=8)
    prompt, toks, logits = z["prompt"], z["tokens"], z["logits"]
    _, lg, _ = w.decode(tokens=torch.from_numpy(prompt).cuda(), pos0=0)
    got, nm = [int(lg.argmax().item())], [_nmse(lg.cpu().numpy(), logits[0])]
    for i in range(len(toks) - 1):
        _, lg, am = w.decode(tokens=torch.tensor([int(toks[i])], dtype=torch.int32, device="cuda"), pos0=len(prompt) + i, want_argmax=True)
        got.append(int(am.item()))
        nm.append(_nmse(lg.cpu().numpy(), logits[i + 1]))
    w.close()
    assert max(nm) < 1e-3, nm
    for i, (a, b) in enumerate(zip(got, toks)):
        top2 = np.sort(logits[i])[-2:]
        if top2[1] - top2[0] > 2e-2 * max(1.0, abs(float(top2[1]))):
            assert a == int(b), (i, got, toks.tolist())


@pytest.mark.parametrize("arch", [0, 1])
def test_prefill_mfma_path_vs_oracle(E, oracle, arch):
    """n_tokens >= 16 goes through the MFMA GEMMs (f16 tiles, activations not re-quantized): logits NMSE vs the reference
    arithmetic stays within the reference's whole-layer backend tolerance (2e-3, tests/test-backend-ops.cpp:3000), and a
    following single-token decode step continues from the KV cache the prefill wrote."""
    torch = E.torch
    rng = np.random.default_rng(81 + arch)
    d = tiny_model(rng, arch=arch, n_layer=2, n_embd=256, n_head=4, n_head_kv=2, n_ff=512, n_vocab=320, n_ctx=64,
                   rope_freqs=(arch == 0), quantize=_quantizer())
    w = E.Window(_hp(d), n_ctx=64)
    w.load_desc(d)
    w.finalize(max_tokens=32)
    ho = oracle.model_new(d)
    toks = rng.integers(0, d.n_vocab, 25).astype(np.int32)
    hid, lg, _ = w.decode(tokens=torch.from_numpy(toks[:24]).cuda(), pos0=0)
    h_ref, l_ref = oracle.model_eval(ho, d, tokens=toks[:24], pos0=0)
    assert _nmse(hid.cpu().numpy(), h_ref) < 2e-3
    assert _nmse(lg.cpu().numpy(), l_ref) < 2e-3
    hid, lg, _ = w.decode(tokens=torch.from_numpy(toks[24:25]).cuda(), pos0=24)
    h_ref, l_ref = oracle.model_eval(ho, d, tokens=toks[24:25], pos0=24)
    assert _nmse(lg.cpu().numpy(), l_ref) < 2e-3
    oracle.model_free(ho)
    w.close()


@pytest.mark.parametrize("arch,types", [(0, None), (1, None), (0, {"ffn_gate": Q4_K, "ffn_up": Q6_K})])
def test_prompt_f16_layer_on_the_third_generation_gemm_vs_oracle(E, oracle, arch, types):
    """A 40-token prompt (above the 32-token small-batch limit) on a model whose every K is >= 512: the layer's GEMMs are the one-launch wq | wk | wv
    and the ffn_gate | ffn_up pair launch of mmq_pf.hip; with ffn_gate Q4_K and ffn_up Q6_K the pair falls back to two launches, ffn_up's epilogue
    reading the f32 gate. Hidden state and logits of the prompt and of a following decode step within the reference's whole-layer backend
    tolerance (NMSE 2e-3, the bound of test_prefill_mfma_path_vs_oracle).
    The decode step of the mixed gate / up case is left out: the engine's 1..32-token paths refuse a layer whose ffn_gate and ffn_up differ in type
    ("decode: ffn_gate and ffn_up of different types", run_layers_fused / small_ffn) - only the prompt path serves it, and that is what the case is for."""
    torch = E.torch
    rng = np.random.default_rng(91 + arch)
    d = tiny_model(rng, arch=arch, n_layer=2, n_embd=512, n_head=4, n_head_kv=2, n_ff=1024, n_vocab=320, n_ctx=64,
                   types=types, rope_freqs=(arch == 0), quantize=_quantizer())
    w = E.Window(_hp(d), n_ctx=64)
    w.load_desc(d)
    w.finalize(max_tokens=64)
    ho = oracle.model_new(d)
    toks = rng.integers(0, d.n_vocab, 41).astype(np.int32)
    for tk, p0 in ((toks[:40], 0), (toks[40:41], 40))[:2 if types is None else 1]:
        hid, lg, _ = w.decode(tokens=torch.from_numpy(tk).cuda(), pos0=p0)
        h_ref, l_ref = oracle.model_eval(ho, d, tokens=tk, pos0=p0)
        nh, nl = _nmse(hid.cpu().numpy(), h_ref), _nmse(lg.cpu().numpy(), l_ref)
        print(f"arch {arch} tokens {len(tk)}: hidden NMSE {nh:.3e} logits NMSE {nl:.3e}")
        assert nh < 2e-3 and nl < 2e-3, (len(tk), nh, nl)
    oracle.model_free(ho)
    w.close()


@pytest.mark.parametrize("flash,n_head,n_embd,n_head_kv", [("1", 8, 512, 2), ("1", 4, 512, 2), ("0", 8, 512, 2), ("1", 8, 1024, 4), ("1", 16, 1024, 8)])
def test_long_context_split_attention_path(E, monkeypatch, flash, n_head, n_embd, n_head_kv):
    """Beyond PM355_ATTN_SPLIT_MIN positions the engine switches from the one-workgroup-per-head attention kernel to the
    keys-split-over-workgroups path - one launch of flash-decoding with an in-launch merge (attn_flash.hip; head_dim 64 and 128, up to
    three spans merged here), or with PM355_ATTN_FLASH=0 the three-launch form (attn_split.hip) - in another captured graph: hidden
    state and logits agree at every position, through graph replay and through plain decode(). The n_embd 1024 shapes have wk / wv row
    slices that take the QKV epilogue (rope + KV store there), so their long-context regime is the matrix-core kernel over cached cells
    (attn_flash_mfma.hip, head_dim 128 and 64)."""
    torch = E.torch
    rng = np.random.default_rng(78)
    monkeypatch.setenv("PM355_ATTN_FLASH", flash)
    d = tiny_model(rng, arch=0, n_layer=2, n_embd=n_embd, n_head=n_head, n_head_kv=n_head_kv, n_ff=1024, n_vocab=320, n_ctx=320, rope_freqs=True)
    toks = rng.integers(0, d.n_vocab, 300).astype(np.int32)
    res = []
    for split_min in ("100000", "40"):
        monkeypatch.setenv("PM355_ATTN_SPLIT_MIN", split_min)
        w = E.Window(_hp(d), n_ctx=320)
        w.load_desc(d); w.finalize(4)
        out = []
        x_out = torch.empty((1, d.n_embd), dtype=torch.float32, device="cuda")
        lg = torch.empty(d.n_vocab, dtype=torch.float32, device="cuda")
        tok = torch.zeros(1, dtype=torch.int32, device="cuda")
        w.set_pos(0)
        for i, t in enumerate(toks):
            tok[0] = int(t)
            if i % 2 == 0:
                w.step(token=tok, x_out=x_out, logits=lg, advance=1, use_graph=True)       # device-side position, graph replay
            else:
                h, l, _ = w.decode(tokens=tok, pos0=i)                                     # host-given position, eager launches
                x_out.copy_(h); lg.copy_(l)
                w.set_pos(i + 1)
            if i in (0, 39, 40, 41, 100, 255, 256, 257, 299):
                torch.cuda.synchronize()
                out.append((x_out.cpu().numpy().copy(), lg.cpu().numpy().copy()))
        res.append(out)
        w.close()
    for (h0, l0), (h1, l1) in zip(*res):
        # not bit-identical: a different f32 summation order can flip an F16 / int8 re-quantization downstream, and the KV
        # caches of the two runs then differ by that much for all later tokens (same effect as between the reference's own builds)
        assert _nmse(h1, h0) < 1e-4 and _nmse(l1, l0) < 1e-3        # the whole-stack bound used against the reference itself


@pytest.mark.parametrize("flash,n_head,n_embd,n_head_kv", [("1", 4, 256, 2), ("0", 4, 256, 2), ("1", 8, 1024, 4)])
def test_long_context_attention_reads_its_own_sequence_slab(E, monkeypatch, flash, n_head, n_embd, n_head_kv):
    """Two sequences in one window, beyond PM355_ATTN_SPLIT_MIN: the long-context forms (attn_flash.hip, attn_split.hip with PM355_ATTN_FLASH=0, and
    - n_embd 1024: the QKV epilogue is served - attn_flash_mfma.hip, head_dim 128) must take the position and the KV slab of the CURRENT sequence.
    Sequence 0 is a decoy: other tokens, 20 positions ahead, stepped in turn with sequence 1. Sequence 1 must give what a window with ONE sequence
    gives for the same tokens through the same forms, under the bound of test_long_context_split_attention_path (a dropped sequence pointer or
    stride reads the decoy's slab: an error of order 1). n_ctx 1088: no power of two, no multiple of 1024.
    (The reference is the same form on purpose. Against the one-workgroup-per-head kernel - PM355_ATTN_SPLIT_MIN=100000, what that neighbour compares
    at n_embd >= 512 - this n_embd 256 model measures, before and after the argument block alike: attn_flash.hip nmse 0 up to position 39, then hidden
    1.02e-4 / logits 1.62e-4 at position 40, the first long-context step; attn_split.hip and attn_flash_mfma.hip stay under 1e-4 / 1e-3 throughout.
    That is the two kernels' summation order on a small model, not the sequence wiring.)"""
    torch = E.torch
    rng = np.random.default_rng(79)
    monkeypatch.setenv("PM355_ATTN_FLASH", flash)
    d = tiny_model(rng, arch=0, n_layer=2, n_embd=n_embd, n_head=n_head, n_head_kv=n_head_kv, n_ff=512, n_vocab=320, n_ctx=1088, rope_freqs=True)
    toks = rng.integers(0, d.n_vocab, 56).astype(np.int32)
    decoy = rng.integers(0, d.n_vocab, 56).astype(np.int32)
    at = (0, 39, 40, 41, 47, 55)
    x_out = torch.empty((1, d.n_embd), dtype=torch.float32, device="cuda")
    lg = torch.empty(d.n_vocab, dtype=torch.float32, device="cuda")
    tok = torch.zeros(1, dtype=torch.int32, device="cuda")
    res = []
    monkeypatch.setenv("PM355_ATTN_SPLIT_MIN", "40")
    for n_seq in (1, 2):
        w = E.Window(_hp(d), n_ctx=1088)
        w.load_desc(d); w.finalize(1, n_seq=n_seq)
        w.kv_clear()
        out = []
        if n_seq == 2:
            w.set_seq_pos(0, 20); w.set_seq_pos(1, 0); w.set_seq(0)
        else:
            w.set_pos(0)
        for i, t in enumerate(toks):
            if n_seq == 2:
                tok[0] = int(decoy[i])
                w.step_ex(token=tok, x_out=x_out, logits=lg, advance=1, rotate=1, use_graph=i % 2 == 0)      # sequence 0, then on to sequence 1
            tok[0] = int(t)
            w.step_ex(token=tok, x_out=x_out, logits=lg, advance=1, rotate=n_seq - 1, use_graph=i % 2 == 0)
            if i in at:
                torch.cuda.synchronize()
                out.append((x_out.cpu().numpy().copy(), lg.cpu().numpy().copy()))
        res.append(out)
        w.close()
    for i, ((h0, l0), (h1, l1)) in zip(at, zip(*res)):
        print(f"position {i}: nmse hidden {_nmse(h1, h0):.3g} logits {_nmse(l1, l0):.3g}")
        assert _nmse(h1, h0) < 1e-4 and _nmse(l1, l0) < 1e-3


def test_step_refuses_to_write_past_the_kv_slab(E):
    """pm355_model_step_ex / set_seq_pos must bound the position by n_ctx (llama_decode returns an error when no KV
    cell is left, src/llama.cpp:18445); a failed step must not move the host mirror of the device counters."""
    import prima_cpp_amd.lib as L
    torch = E.torch
    rng = np.random.default_rng(3)
    d = tiny_model(rng, arch=0, n_layer=1, n_embd=256, n_head=4, n_head_kv=2, n_ff=512, n_vocab=320, n_ctx=32, rope_freqs=True)
    w = E.Window(_hp(d), n_ctx=32)
    w.load_desc(d)
    w.finalize(max_tokens=1, n_seq=2)
    tok = torch.zeros(1, dtype=torch.int32, device="cuda")
    am = torch.zeros(1, dtype=torch.int32, device="cuda")
    w.set_pos(31)
    w.step(token=tok, argmax=am)                       # position 31 = last cell: fine
    torch.cuda.synchronize()
    for use_graph in (True, False):
        with pytest.raises(L.PM355Error):
            w.step(token=tok, argmax=am, use_graph=use_graph)    # position 32 == n_ctx: refused, nothing launched
    with pytest.raises(L.PM355Error):
        w.set_seq_pos(1, 33)
    with pytest.raises(L.PM355Error):
        w.set_seq_pos(1, -1)
    torch.cuda.synchronize()
    w.set_pos(5)
    w.step(token=tok, argmax=am)                       # still usable after the refusals
    torch.cuda.synchronize()
    w.close()


@pytest.mark.parametrize("n_slots", [1, 2, 3, 4])
def test_window_streaming_matches_resident(E, n_slots):
    """pm355_model_set_streaming: layer tensors parked in pinned host memory and cycled through n_slots device slots by the copy
    stream (the GPU-side form of prima.cpp's layer-window prefetch, src/llama.cpp:18152-18218) must give bit-identical results to the
    fully resident window: 20-token MFMA prefill, a short multi-token batch, and single-token steps wrapping around the slot ring."""
    torch = E.torch
    rng = np.random.default_rng(99)
    d = tiny_model(rng, arch=0, n_layer=4, n_embd=256, n_head=4, n_head_kv=2, n_ff=512, n_vocab=320, n_ctx=64, rope_freqs=True)
    toks = rng.integers(0, d.n_vocab, 30).astype(np.int32)
    outs = []
    for slots in (0, n_slots):
        w = E.Window(_hp(d), n_ctx=64)
        if slots:
            w.set_streaming(slots)
        w.load_desc(d)
        w.finalize(max_tokens=20)
        res = []
        h, lg, _ = w.decode(tokens=torch.from_numpy(toks[:20]).cuda(), pos0=0)
        res.append((h.cpu().numpy(), lg.cpu().numpy()))
        h, lg, _ = w.decode(tokens=torch.from_numpy(toks[20:23]).cuda(), pos0=20)
        res.append((h.cpu().numpy(), lg.cpu().numpy()))
        w.set_pos(23)
        x_out = torch.empty((1, d.n_embd), dtype=torch.float32, device="cuda")
        lgt = torch.empty(d.n_vocab, dtype=torch.float32, device="cuda")
        tok = torch.zeros(1, dtype=torch.int32, device="cuda")
        for t in toks[23:]:
            tok[0] = int(t)
            w.step(token=tok, x_out=x_out, logits=lgt, advance=1)
            torch.cuda.synchronize()
            res.append((x_out.cpu().numpy().copy(), lgt.cpu().numpy().copy()))
        if slots:
            assert w.streamed_bytes() > 0
        outs.append(res)
        w.close()
    for (h0, l0), (h1, l1) in zip(*outs):
        assert np.array_equal(h0, h1) and np.array_equal(l0, l1)


def test_qkv_epilogue_decode_form_matches_round2_form(E, oracle, monkeypatch):
    """PM355_QKV_EPI=0 (rope + KV store inside the attention kernel, the round-2 launch sequence) against the default (RoPE + KV store in
    the epilogue of the wq | wk | wv launch, attention over cached cells) through graph replay, on a window whose projections give every
    workgroup whole rotation pairs (N % 512 == 0), across the 64-cell boundary of the short attention kernel; both against the oracle."""
    torch = E.torch
    rng = np.random.default_rng(123)
    d = tiny_model(rng, arch=0, n_layer=2, n_embd=1024, n_head=8, n_head_kv=4, n_ff=2048, n_vocab=320, n_ctx=128, rope_freqs=True)
    assert d.head_dim == 128
    toks = rng.integers(0, d.n_vocab, 80).astype(np.int32)
    outs = []
    for flag in ("0", "1"):
        monkeypatch.setenv("PM355_QKV_EPI", flag)
        w = E.Window(_hp(d), n_ctx=128)
        w.load_desc(d)
        w.finalize(max_tokens=1)
        w.set_pos(0)
        x_out = torch.empty((1, d.n_embd), dtype=torch.float32, device="cuda")
        lg = torch.empty(d.n_vocab, dtype=torch.float32, device="cuda")
        tok = torch.zeros(1, dtype=torch.int32, device="cuda")
        res = []
        for t in toks:
            tok[0] = int(t)
            w.step(token=tok, x_out=x_out, logits=lg, advance=1, use_graph=True)
            torch.cuda.synchronize()
            res.append((x_out.cpu().numpy().copy(), lg.cpu().numpy().copy()))
        assert w.check() == 0
        outs.append(res)
        kv = [(w.kv(il, 0).copy(), w.kv(il, 1).copy()) for il in range(d.n_layer)]
        outs.append(kv)
        w.close()
    (r0, kv0, r1, kv1) = outs
    per = [_nmse(l1, l0) for (_, l0), (_, l1) in zip(r0, r1)]
    nm = max(per)
    print(f"\n[QKV epilogue form vs round-2 form] worst per-step logits NMSE {nm:.2e}; steps above 1e-9: {[(i, float(f'{v:.1e}')) for i, v in enumerate(per) if v > 1e-9]}")
    # summation order only (1e-13) - until a value that sits on an int8 / F16 rounding boundary tips the other way in one of the two runs:
    # that token differs by ~1e-4 and, through its K / V cache rows, every later token by ~1e-5 (observed: identical up to step 24 of 80).
    # The per-op comparison is tests/test_gpu_ops.py::test_qkv_epilogue_and_cached_attention_equal_the_fused_attention_path.
    assert nm < 1e-3 and max(per[:10]) < 1e-9, (nm, per[:10])
    # layer-0 caches (their inputs are identical in both runs): the same F16 bits except where the split wk / wv rows round differently
    for which in (0, 1):
        a, b = kv0[0][which], kv1[0][which]
        assert (a != b).mean() < 0.01
    # and against the oracle (teacher-forced)
    ho = oracle.model_new(d)
    worst = 0.0
    for i, t in enumerate(toks[:70]):
        _, l_ref = oracle.model_eval(ho, d, tokens=np.array([t], dtype=np.int32), pos0=i)
        worst = max(worst, _nmse(r1[i][1], l_ref))
    oracle.model_free(ho)
    print(f"[QKV epilogue form vs oracle] worst per-step logits NMSE {worst:.2e}")
    assert worst < 1e-3, worst


@pytest.mark.experiments
@pytest.mark.parametrize("arch", [0, 1])
def test_producer_side_sum_of_squares_decode_is_bit_identical(E, monkeypatch, arch):
    """PM355_SS=0 (every rms_norm prologue reduces its own row: the round-4 form) against the default (wo / ffn_down leave per-workgroup
    partials, the wq | wk | wv, ffn_gate | ffn_up and lm_head launches add them): hidden rows and logits of 40 graph-replayed tokens must be
    the same bits - the partial sums are exact in f64 for these magnitudes, and where they are not the f32 rounding of the mean hides it."""
    torch = E.torch
    rng = np.random.default_rng(321)
    d = tiny_model(rng, arch=arch, n_layer=3, n_embd=1024, n_head=8, n_head_kv=4, n_ff=2048, n_vocab=320, n_ctx=128, rope_freqs=(arch == 0))
    toks = rng.integers(0, d.n_vocab, 40).astype(np.int32)
    outs = []
    for flag in ("0", "1"):
        monkeypatch.setenv("PM355_SS", flag)
        w = E.Window(_hp(d), n_ctx=128)
        w.load_desc(d)
        w.finalize(max_tokens=1)
        w.set_pos(0)
        x_out = torch.empty((1, d.n_embd), dtype=torch.float32, device="cuda")
        lg = torch.empty(d.n_vocab, dtype=torch.float32, device="cuda")
        tok = torch.zeros(1, dtype=torch.int32, device="cuda")
        res = []
        for t in toks:
            tok[0] = int(t)
            w.step(token=tok, x_out=x_out, logits=lg, advance=1, use_graph=True)
            torch.cuda.synchronize()
            res.append((x_out.cpu().numpy().copy(), lg.cpu().numpy().copy()))
        assert w.check() == 0
        outs.append(res)
        w.close()
    for i, ((h0, l0), (h1, l1)) in enumerate(zip(*outs)):
        assert np.array_equal(h0, h1) and np.array_equal(l0, l1), i


@pytest.mark.experiments
@pytest.mark.parametrize("arch,n_tok", [(0, 90), (1, 70)])
def test_persistent_decode_engine_matches_the_five_launch_path(E, oracle, monkeypatch, arch, n_tok):
    """Round 5: csrc/decode_engine.hip (opt-in, PM355_ENGINE=1) - every phase of every layer of a single-token step as ONE persistent launch, device-wide
    barriers in place of kernel boundaries - against the default five launches per layer. The same row loops, prologue and epilogue code run in both:
    hidden rows and logits must be the same BITS, across the 64-cell boundary of the short attention path, NORM and NEOX rope, with the engine's
    watchdog clean (a stale hand-off between workgroups showed as 1e-4 while the engine was being built). Then against the oracle, teacher-forced."""
    torch = E.torch
    rng = np.random.default_rng(4321 + arch)
    d = tiny_model(rng, arch=arch, n_layer=3, n_embd=1024, n_head=8, n_head_kv=4, n_ff=2048, n_vocab=320, n_ctx=128, rope_freqs=(arch == 0))
    toks = rng.integers(0, d.n_vocab, n_tok).astype(np.int32)
    outs = []
    for flag in ("0", "1"):
        monkeypatch.setenv("PM355_ENGINE", flag)
        monkeypatch.setenv("PM355_ENGINE_VERBOSE", "1")
        w = E.Window(_hp(d), n_ctx=128)
        w.load_desc(d)
        w.finalize(max_tokens=1)
        w.set_pos(0)
        x_out = torch.empty((1, d.n_embd), dtype=torch.float32, device="cuda")
        lg = torch.empty(d.n_vocab, dtype=torch.float32, device="cuda")
        tok = torch.zeros(1, dtype=torch.int32, device="cuda")
        res = []
        for t in toks:
            tok[0] = int(t)
            w.step(token=tok, x_out=x_out, logits=lg, advance=1, use_graph=True)
            torch.cuda.synchronize()
            res.append((x_out.cpu().numpy().copy(), lg.cpu().numpy().copy()))
        assert w.check() == 0
        outs.append(res)
        w.close()
    per = [max(_nmse(h1, h0), _nmse(l1, l0)) for (h0, l0), (h1, l1) in zip(*outs)]
    print(f"\n[engine vs five launches, arch {arch}] worst per-step NMSE {max(per):.2e}; bit-identical steps {sum(int(np.array_equal(a[1], b[1])) for a, b in zip(*outs))}/{n_tok}")
    assert max(per) == 0.0, per
    ho = oracle.model_new(d)
    worst = 0.0
    for i, t in enumerate(toks[:40]):
        _, l_ref = oracle.model_eval(ho, d, tokens=np.array([t], dtype=np.int32), pos0=i)
        worst = max(worst, _nmse(outs[1][i][1], l_ref))
    oracle.model_free(ho)
    assert worst < 1e-3, worst


@pytest.mark.experiments
@pytest.mark.parametrize("arch", [0, 1])
def test_attention_tail_decode_is_bit_identical(E, monkeypatch, arch):
    """Round 5: PM355_ATTN_TAIL=1 - the attention computed in the tail of the wq | wk | wv launch by the last workgroups of each
    KV-head group (four launches per layer) - against the default five launches: the same hidden rows and logits, bit for bit, across the 64-cell
    boundary of the short attention path, NORM and NEOX rope, with the tail's watchdog clean."""
    torch = E.torch
    rng = np.random.default_rng(977 + arch)
    d = tiny_model(rng, arch=arch, n_layer=3, n_embd=1024, n_head=16, n_head_kv=8, n_ff=2048, n_vocab=320, n_ctx=128, rope_freqs=(arch == 0))
    toks = rng.integers(0, d.n_vocab, 80).astype(np.int32)
    outs = []
    for flag in ("0", "1"):
        monkeypatch.setenv("PM355_ATTN_TAIL", flag)
        w = E.Window(_hp(d), n_ctx=128)
        w.load_desc(d)
        w.finalize(max_tokens=1)
        w.set_pos(0)
        x_out = torch.empty((1, d.n_embd), dtype=torch.float32, device="cuda")
        lg = torch.empty(d.n_vocab, dtype=torch.float32, device="cuda")
        tok = torch.zeros(1, dtype=torch.int32, device="cuda")
        res = []
        for t in toks:
            tok[0] = int(t)
            w.step(token=tok, x_out=x_out, logits=lg, advance=1, use_graph=True)
            torch.cuda.synchronize()
            res.append((x_out.cpu().numpy().copy(), lg.cpu().numpy().copy()))
        assert w.check() == 0
        outs.append(res)
        w.close()
    for i, ((h0, l0), (h1, l1)) in enumerate(zip(*outs)):
        assert np.array_equal(h0, h1) and np.array_equal(l0, l1), i


def test_single_token_decode_with_three_types_in_wq_wk_wv_vs_oracle(E, oracle):
    """wq Q4_K, wk Q6_K, wv Q5_K: three types, so neither the epilogue nor the three-job launch serves wq | wk | wv and the step falls back to one
    mat-vec launch per matrix (run_layers_fused) - single tokens from an empty cache, at the tolerances of test_window_prefill_and_decode_vs_oracle."""
    from _bind import Q5_K
    torch = E.torch
    rng = np.random.default_rng(77)
    d = tiny_model(rng, arch=0, n_layer=2, n_embd=512, n_head=8, n_head_kv=8, n_ff=512, n_vocab=320, n_ctx=64, rope_freqs=True,
                   types={"attn_k": Q6_K, "attn_v": Q5_K}, quantize=_quantizer())
    w = E.Window(_hp(d), n_ctx=64)
    w.load_desc(d)
    w.finalize(max_tokens=1)
    ho = oracle.model_new(d)
    toks = rng.integers(0, d.n_vocab, 4).astype(np.int32)
    for p0, t in enumerate(toks):
        hid, lg, am = w.decode(tokens=torch.from_numpy(toks[p0:p0 + 1]).cuda(), pos0=p0, want_argmax=True)
        h_ref, l_ref = oracle.model_eval(ho, d, tokens=toks[p0:p0 + 1], pos0=p0)
        print(f"[three-type wq | wk | wv] token {p0}: NMSE hidden {_nmse(hid.cpu().numpy(), h_ref):.2e} logits {_nmse(lg.cpu().numpy(), l_ref):.2e}")
        assert _nmse(hid.cpu().numpy(), h_ref) < 1e-3
        assert _nmse(lg.cpu().numpy(), l_ref) < 1e-3
        assert int(am.item()) == int(np.argmax(lg.cpu().numpy()))
    for which in (0, 1):
        a = w.kv(0, which).view(np.float16).astype(np.float32)
        b = oracle.model_kv(ho, d, 0, which).view(np.float16).astype(np.float32)
        assert _nmse(a, b) < 1e-6
    oracle.model_free(ho)
    w.close()


# (path, prompt tokens, model, the two windows, NMSE bound). n_ctx 64 / 160: a multiple of 32, the matrix-core kernel (attn_prefill.hip) serves it where the
# path asks for it. n_ctx 72 / 136: a multiple of 8 only - that kernel refuses and the path's chain goes on (engine.hip: ATTN_SMALL, ATTN_PROMPT_F16, ATTN_PROMPT_I8)
# The forms are the indices of pm355_model_attn_forms: 1 matrix-core kernel (f32 rows), 2 the same with F16 rows, 3 attn_cached, 4 attn_decode
_CHAIN_CASES = [
    ("small-5", 5, dict(n_layer=2, n_embd=256, n_head=4, n_head_kv=2, n_ff=512), (64, 72), (3, 3), 1e-3),        # below SMALL_ATTN_MFMA_MIN: attn_cached in both windows
    # (n_embd 512: at 256 the small-batch mat-mul does not serve the layer and 20 tokens take the F16 prompt path - the count below told)
    ("small-20", 20, dict(n_layer=2, n_embd=512, n_head=4, n_head_kv=2, n_ff=1024), (64, 72), (1, 3), 2e-3),     # matrix-core kernel at 64, attn_cached at 72
    ("prompt-f16-40", 40, dict(n_layer=2, n_embd=512, n_head=4, n_head_kv=2, n_ff=1024), (64, 72), (2, 4), 2e-3),  # F16 rows at 64; at 72 attn_decode's f32 rows feed the wo GEMM
    ("prompt-i8-128", 128, dict(n_layer=1, n_embd=1024, n_head=8, n_head_kv=2, n_ff=1024), (160, 136), (1, 4), 2e-3),   # PM355_PROMPT_I8=1: f32 rows (the F16 prompt path would count form 2); attn_decode at 136
]


def _attn_forms(w):
    """pm355_model_attn_forms: layer passes of multi-token windows per attention form; None on a library in front of that entry (A/B runs)"""
    import ctypes as C
    if not hasattr(w.lib, "pm355_model_attn_forms"):
        return None
    f = w.lib.pm355_model_attn_forms
    f.restype, f.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_int]
    out = (C.c_int64 * 5)()
    assert f(w.h, out, 5) == 0
    return list(out)


@pytest.mark.parametrize("name,n_tok,shape,windows,forms,bound", _CHAIN_CASES, ids=[c[0] for c in _CHAIN_CASES])
def test_multi_token_attention_chain_with_and_without_the_matrix_core_kernel(E, oracle, monkeypatch, name, n_tok, shape, windows, forms, bound):
    """The attention of the three multi-token layer paths (engine.hip attend()) where its first kernel serves the window and where it refuses (n_ctx % 32 != 0)
    and the next form of the path's chain runs: the prompt, then one single-token step from the cache the prompt wrote, against the oracle; the engine's
    own count says that every layer of the prompt took the form the case is about and no other (the single token does not pass through attend()). Bounds: the
    project's own for these token counts - NMSE 1e-3 (test_window_prefill_and_decode_vs_oracle) at 5 tokens, 2e-3 (test_prefill_mfma_path_vs_oracle,
    test_prompt_f16_layer_on_the_third_generation_gemm_vs_oracle) at 20, 40 and 128."""
    torch = E.torch
    if name.startswith("prompt-i8"):
        monkeypatch.setenv("PM355_PROMPT_I8", "1")
    for n_ctx, form in zip(windows, forms):
        rng = np.random.default_rng(131)
        d = tiny_model(rng, arch=0, n_vocab=320, n_ctx=n_ctx, rope_freqs=True, quantize=_quantizer(), **shape)
        w = E.Window(_hp(d), n_ctx=n_ctx)
        w.load_desc(d)
        w.finalize(max_tokens=n_tok)
        ho = oracle.model_new(d)
        toks = rng.integers(0, d.n_vocab, n_tok + 1).astype(np.int32)
        for tk, p0 in ((toks[:n_tok], 0), (toks[n_tok:], n_tok)):
            hid, lg, am = w.decode(tokens=torch.from_numpy(tk).cuda(), pos0=p0, want_argmax=True)
            h_ref, l_ref = oracle.model_eval(ho, d, tokens=tk, pos0=p0)
            nh, nl = _nmse(hid.cpu().numpy(), h_ref), _nmse(lg.cpu().numpy(), l_ref)
            print(f"{name} n_ctx {n_ctx} tokens {len(tk)}: hidden NMSE {nh:.3e} logits NMSE {nl:.3e}")
            assert nh < bound and nl < bound, (n_ctx, len(tk), nh, nl)
            assert int(am.item()) == int(np.argmax(lg.cpu().numpy()))
        ran = _attn_forms(w)
        print(f"{name} n_ctx {n_ctx}: layer passes per attention form {ran}")
        assert ran is None or ran == [d.n_layer if i == form else 0 for i in range(5)], (n_ctx, ran)
        oracle.model_free(ho)
        w.close()
