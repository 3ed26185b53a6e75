"""GPU parity of the MASK mode of the MFMA batch attention (csrc/attn_prefill.hip through pm355_attn_prefill_masked_ex): the kernel every
multi-token batch of the plug-in runs (prompt chunks, speculative batches, parallel sequences), on masks that are NOT causal.

Reference: the float64 restatement of llm_build_kqv with the additive mask, on the same F16-rounded K / V and the F16-rounded query:
s = f32(K.q) * scale + mask_row, e = exp(s - max s), p = f16(e / sum e), out = V.p in float64, over cells [0, n_kv) only (_reference below; it
shares no code with the kernel or with ops.py). Bound: the causal test's, |out - want|.max() <= 2e-3 * |want|.max() + 1e-4 per (token, head),
checked for EVERY token and head.

Decoy cells: every cell no query of the case may attend - masked with -inf for all queries inside [0, n_kv), and all of [n_kv, n_ctx) - holds K
rows at 8x the live scale and V values of magnitude ~1000 with random sign, so that a leaked weight of 1e-6 already breaks the bound (live values
are at unit scale). The decoys are finite on purpose: a non-finite value in a masked cell inside n_kv poisons the reference's own 0 * NaN as
well, and real caches never hold one there (both caches are zeroed at allocation: engine.hip, ggml_backend_buffer_clear). Mask rows are
mask_stride elements apart with the gap [n_kv, mask_stride) filled with 0.0 (a kernel indexing rows by n_kv, or reading past n_kv, attends
decoys), and 32 rows of -inf follow row T - 1 like the padding llama_set_inputs writes."""
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BOUND_REL, BOUND_ABS = 2e-3, 1e-4          # test_attn_prefill_mfma_vs_exact's bound, unchanged
V_ROWMAJOR, MASK_F16 = 1, 2                # PM355_ATTN_V_ROWMAJOR, PM355_ATTN_MASK_F16 (include/prima_mi355.h)
E_SHAPE, E_RANGE = -2, -4                  # PM355_E_SHAPE, PM355_E_RANGE
GQA = [(8, 2), (4, 4)]


@pytest.fixture(scope="module")
def P():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("GPU tests need a HIP device")
    import prima_cpp_amd.ops as ops
    ops.torch = torch
    return ops


def _dev(P, a):
    return P.torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def _f16bits(P, a):
    return P.torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda()


def _roundup(x, m):
    return (x + m - 1) // m * m


def _reference(q, K, V, mask, n_kv, scale):
    """q [T, H, dh] f32; K [n_ctx, Hkv, dh] f16; V [Hkv, dh, n_ctx] f16; mask [T, >= n_kv] f32 -> float64 [T, H, dh]. Touches no cell >= n_kv."""
    T, H, dh = q.shape
    Hkv = K.shape[1]
    qh = q.astype(np.float16).astype(np.float64)
    m = mask[:T, :n_kv].astype(np.float32)
    want = np.empty((T, H, dh), dtype=np.float64)
    with np.errstate(invalid="raise"):         # a query without a visible cell would be a mistake of the case, not of the kernel
        for h in range(H):
            hk = h // (H // Hkv)
            s = (qh[:, h] @ K[:n_kv, hk].astype(np.float64).T).astype(np.float32) * np.float32(scale) + m          # [T, n_kv]
            e = np.exp(s - s.max(axis=1, keepdims=True)).astype(np.float32)
            inv = (1.0 / e.astype(np.float64).sum(axis=1, keepdims=True)).astype(np.float32)
            p = (e * inv).astype(np.float16).astype(np.float64)
            want[:, h] = p @ V[hk, :, :n_kv].astype(np.float64).T
    return want


def _worst(out, want):
    """(largest err / bound over all (token, head), its (t, h)) for the project's bound."""
    err = np.abs(out - want).max(axis=2)
    bound = BOUND_REL * np.abs(want).max(axis=2) + BOUND_ABS
    r = err / bound
    t, h = np.unravel_index(np.argmax(r), r.shape)
    return float(r[t, h]), (int(t), int(h), float(err[t, h]), float(bound[t, h]))


class Case:
    """Seeded inputs for one visibility matrix vis [T, n_kv] (True = query t may attend cell k)."""

    def __init__(self, vis, n_ctx, dh, H, Hkv, seed, stride_pad=0):
        rng = np.random.default_rng(seed)
        T, n_kv = vis.shape
        assert n_kv % 4 == 0 and n_kv <= n_ctx and n_ctx % 32 == 0 and vis.any(axis=1).all()
        self.T, self.n_kv, self.n_ctx, self.dh, self.H, self.Hkv = T, n_kv, n_ctx, dh, H, Hkv
        self.scale = 1.0 / np.sqrt(dh)
        self.q = rng.normal(0, 1, (T, H, dh)).astype(np.float32)
        decoy = np.ones(n_ctx, dtype=bool)
        decoy[:n_kv] = ~vis.any(axis=0)
        K = rng.normal(0, 1, (n_ctx, Hkv, dh))
        K[decoy] *= 8.0
        V = rng.normal(0, 1, (Hkv, dh, n_ctx))
        V[:, :, decoy] = (rng.uniform(800, 1200, V.shape) * rng.choice([-1.0, 1.0], V.shape))[:, :, decoy]
        self.K, self.V = K.astype(np.float16), V.astype(np.float16)
        self.stride = n_kv + stride_pad
        assert self.stride % 4 == 0
        self.mask = np.full((T + 32, self.stride), -np.inf, dtype=np.float32)
        self.mask[:T, :n_kv][vis] = 0.0
        self.mask[:T, n_kv:] = 0.0
        self.n_decoy = int(decoy.sum())

    def want(self):
        return _reference(self.q, self.K, self.V, self.mask, self.n_kv, self.scale)

    def run(self, P, flash=False):
        c = self
        q = _dev(P, c.q.reshape(c.T, -1))
        if flash:
            v = _f16bits(P, c.V.transpose(2, 0, 1))                    # [n_ctx][Hkv * dh] like K
            mask = _f16bits(P, c.mask.astype(np.float16))              # 0 and -inf are exact in F16
            flags = V_ROWMAJOR | MASK_F16
        else:
            v, mask, flags = _f16bits(P, c.V), _dev(P, c.mask), 0
        out = P.attn_prefill_masked(q, _f16bits(P, c.K), v, mask, c.T, c.H, c.Hkv, c.dh, c.n_ctx, c.n_kv, c.scale, mask_stride=c.stride, flags=flags)
        return out.cpu().numpy().reshape(c.T, c.H, c.dh)

    def run_causal(self, P, n_past):
        c = self
        out = P.attn_prefill(_dev(P, c.q.reshape(c.T, -1)), _f16bits(P, c.K), _f16bits(P, c.V), n_past, c.H, c.Hkv, c.dh, c.n_ctx, c.scale)
        return out.cpu().numpy().reshape(c.T, c.H, c.dh)


def _check(P, case, label, flash=False):
    want = case.want()
    out = case.run(P)
    assert np.isfinite(out).all(), label
    r, where = _worst(out, want)
    print(f"{label}: T={case.T} n_kv={case.n_kv} n_ctx={case.n_ctx} decoys={case.n_decoy} worst err/bound={r:.3f} at (t, h, err, bound)={where}")
    assert r <= 1.0, (label, where)
    if flash:
        out_fa = case.run(P, flash=True)
        r, where = _worst(out_fa, want)
        print(f"{label} [row-major V, F16 mask]: worst err/bound={r:.3f} at {where}")
        assert r <= 1.0, (label, "flash form", where)
        assert np.array_equal(out_fa, out), (label, "flash form differs from transposed V / F32 mask", float(np.abs(out_fa - out).max()))
    return out, want


# ---- visibility matrices ------------------------------------------------------------------------------------------------------------------

def _vis_causal(n_past, T):
    n_kv = _roundup(n_past + T, 4)
    return np.arange(n_kv)[None, :] <= (n_past + np.arange(T))[:, None]


def _vis_parallel(n_seq, P0, n_kv):
    """One token of each of n_seq sequences: P0 shared prompt cells, then cell P0 + i belongs to sequence i % n_seq (three rounds dealt)."""
    k = np.arange(n_kv)
    dealt = (k >= P0) & (k < P0 + 3 * n_seq)
    return (k < P0)[None, :] | (dealt[None, :] & (((k - P0) % n_seq)[None, :] == np.arange(n_seq)[:, None]))


def _vis_ragged(counts, pasts):
    """Sequences with counts[s] batch tokens on top of pasts[s] cached cells: causal inside a sequence, blind across sequences. Cell order: each
    past, followed by three stale cells nobody sees, then the batch's cells in token order (sequence after sequence)."""
    cell, past_cells = 0, []
    for n in pasts:
        past_cells.append((cell, cell + n))
        cell += n + 3
    batch0 = cell
    T = sum(counts)
    n_kv = _roundup(batch0 + T, 4)
    vis = np.zeros((T, n_kv), dtype=bool)
    t = 0
    for s, n in enumerate(counts):
        for i in range(n):
            vis[t, past_cells[s][0]:past_cells[s][1]] = True
            vis[t, batch0 + t - i:batch0 + t + 1] = True
            t += 1
    return vis


def _vis_hole(first_visible):
    """One sequence, 5 batch tokens behind 128 cached cells of which [32, 96) were removed (first_visible = 0) or everything below
    first_visible was (tiles 0 and 1 wholly masked, m still -inf when the first live tile arrives)."""
    T, n_past = 5, 128
    vis = _vis_causal(n_past, T)
    if first_visible:
        vis[:, :first_visible] = False
    else:
        vis[:, 32:96] = False
    return vis


def _vis_lane_halves(n_kv=100):
    """Accumulator registers of lane half 0 hold keys with k % 8 < 4, of half 1 those with k % 8 >= 4: a query seeing only one kind leaves the
    other half with m = -inf, l = 0 after pass 1. Plus queries that see exactly one cell: the last of n_kv, cell 0, and the first of the last
    (partial) tile."""
    k = np.arange(n_kv)
    return np.stack([(k % 8 < 4) & (k % 3 == 0), (k % 8 >= 4) & (k % 5 != 0), k == n_kv - 1, k == 0, k == n_kv // 32 * 32, (k % 8 < 4) & (k >= 64)])


def _vis_wrapped(T, n_kv):
    """Query t sees cells <= t % n_kv: lets T exceed n_kv (the kernel does not need the batch itself to be in the cache)."""
    return np.arange(n_kv)[None, :] <= (np.arange(T) % n_kv)[:, None]


# ---- 1. causal mask == causal mode -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H,Hkv", GQA)
@pytest.mark.parametrize("dh", [64, 128])
@pytest.mark.parametrize("n_past,T", [(0, 1), (0, 16), (0, 37), (5, 128), (40, 200), (96, 160), (0, 2), (7, 3), (31, 33), (100, 129)])
def test_causal_mask_equals_causal_mode_bitwise(P, n_past, T, dh, H, Hkv):
    """Both modes run the same MFMA sequence on the visible tiles, acc * scale + 0.0f == acc * scale, and the all-masked tiles mask mode walks in
    addition add exp(-inf) = 0 to the sum and 0 * finite to the output: the results must be identical bit for bit, decoys in the cache included
    (causal mode has to ignore the cells behind the batch as well). The float64 reference judges both sides, so a failure names the wrong one."""
    case = Case(_vis_causal(n_past, T), 256, dh, H, Hkv, seed=1000 + 7 * n_past + T)
    out, want = _check(P, case, f"causal n_past={n_past}")
    ref = case.run_causal(P, n_past)
    r, where = _worst(ref, want)
    assert r <= 1.0, ("causal MODE against float64", where)
    assert np.array_equal(out, ref), ("mask mode differs from causal mode", float(np.abs(out - ref).max()))


# ---- 2. parallel sequences -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H,Hkv", GQA)
@pytest.mark.parametrize("dh", [64, 128])
@pytest.mark.parametrize("big_n_kv", [False, True])
@pytest.mark.parametrize("P0", [0, 5, 40])
@pytest.mark.parametrize("n_seq", [2, 3, 8, 32])
def test_parallel_sequences_one_token_each(P, n_seq, P0, big_n_kv, dh, H, Hkv):
    """T = n_seq queries, one per sequence; with P0 = 0 cell 0 is invisible to every query but the first (the kernel's comment 'key 0 is always
    visible' is false here), and with 32 sequences a query's three cells lie in three different key tiles. mask_stride > n_kv."""
    n_kv = 256 if big_n_kv else _roundup(P0 + 3 * n_seq, 4)
    case = Case(_vis_parallel(n_seq, P0, n_kv), 512, dh, H, Hkv, seed=2000 + 100 * n_seq + P0, stride_pad=36)
    _check(P, case, f"parallel n_seq={n_seq} P0={P0}")


# ---- 3. ragged batches -----------------------------------------------------------------------------------------------------------------------

RAGGED = {"1+17": ((1, 17), (9, 30)), "17+60": ((17, 60), (3, 50)), "1+17+60": ((1, 17, 60), (20, 0, 41)), "60+17+53": ((60, 17, 53), (10, 33, 0))}


@pytest.mark.parametrize("H,Hkv", GQA)
@pytest.mark.parametrize("dh", [64, 128])
@pytest.mark.parametrize("name", list(RAGGED))
def test_ragged_batch(P, name, dh, H, Hkv):
    """Sequences of different lengths and pasts in one batch: the 32 queries of a wave, and the four waves of a workgroup (T = 130: two
    workgroups), need different cells of the same tiles."""
    counts, pasts = RAGGED[name]
    case = Case(_vis_ragged(counts, pasts), 512, dh, H, Hkv, seed=3000 + sum(counts), stride_pad=4)
    _check(P, case, f"ragged {name}")


# ---- 4. holes, empty tiles, empty lane halves ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H,Hkv", GQA)
@pytest.mark.parametrize("dh", [64, 128])
@pytest.mark.parametrize("name", ["hole_32_96", "first_visible_70", "lane_halves"])
def test_holes_and_empty_tiles(P, name, dh, H, Hkv):
    vis = {"hole_32_96": lambda: _vis_hole(0), "first_visible_70": lambda: _vis_hole(70), "lane_halves": _vis_lane_halves}[name]()
    case = Case(vis, 256, dh, H, Hkv, seed=4000 + len(name), stride_pad=8)
    _check(P, case, name)


# ---- 5. edges of n_kv ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H,Hkv", GQA)
@pytest.mark.parametrize("dh", [64, 128])
@pytest.mark.parametrize("n_ctx,n_kv,T", [(32, 4, 2), (32, 28, 127), (32, 32, 128), (256, 28, 128), (256, 36, 129), (256, 100, 300), (256, 256, 300),
                                          (1024, 36, 2), (1024, 100, 127), (1024, 1024, 300)])
def test_edges_of_n_kv(P, n_ctx, n_kv, T, dh, H, Hkv):
    """Partial last tile (the k0 + 3 < n_kv guard and the clamped fetch_k), n_kv == n_ctx, T around the 128-query workgroup."""
    case = Case(_vis_wrapped(T, n_kv), n_ctx, dh, H, Hkv, seed=5000 + n_ctx + n_kv + T, stride_pad=0 if n_kv == n_ctx else 12)
    _check(P, case, "edges")


# ---- 6. flash-attention form -----------------------------------------------------------------------------------------------------------------

FLASH = {
    "parallel_3_p5": lambda: (_vis_parallel(3, 5, 16), 512, 36),          # partial last tile
    "parallel_32_p0": lambda: (_vis_parallel(32, 0, 256), 512, 36),
    "ragged_60+17+53": lambda: (_vis_ragged(*RAGGED["60+17+53"]), 512, 4),
    "first_visible_70": lambda: (_vis_hole(70), 256, 8),
    "lane_halves": lambda: (_vis_lane_halves(), 256, 8),                # n_kv = 100: partial last tile
    "edge_32_28_127": lambda: (_vis_wrapped(127, 28), 32, 12),
    "edge_256_100_300": lambda: (_vis_wrapped(300, 100), 256, 12),
    "edge_1024_1024_300": lambda: (_vis_wrapped(300, 1024), 1024, 0),
}


@pytest.mark.parametrize("H,Hkv", GQA)
@pytest.mark.parametrize("dh", [64, 128])
@pytest.mark.parametrize("name", list(FLASH))
def test_flash_form_rowmajor_v_f16_mask(P, name, dh, H, Hkv):
    """flags = V_ROWMAJOR | MASK_F16 on a row-major V cache holding the same values and the same mask cast to F16: inside the bound of the
    float64 reference AND bit-identical to the transposed-V / F32-mask result. The second claim from the code: put_v writes element (key,
    channel c) of a row-major tile to vs[c * VS + key], the address the transposed staging writes the same value to, so both layouts leave the
    same LDS image and pass 2 issues the same MFMAs in the same order; h2f of an F16 0 / -inf is the F32 0 / -inf."""
    vis, n_ctx, pad = FLASH[name]()
    case = Case(vis, n_ctx, dh, H, Hkv, seed=6000 + len(name) + vis.shape[0], stride_pad=pad)
    _check(P, case, f"flash {name}", flash=True)


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,change,rc", [
    ("n_kv % 4", dict(n_kv=30), E_RANGE),
    ("n_kv > n_ctx", dict(n_kv=96), E_RANGE),
    ("mask_stride % 4", dict(mask_stride=34), E_RANGE),
    ("head_dim 96", dict(head_dim=96), E_RANGE),
    ("n_ctx % 32", dict(n_ctx=48), E_RANGE),
    ("mask NULL", dict(mask=None), E_SHAPE),
])
def test_refusals_leave_out_untouched(P, name, change, rc):
    """Host checks of pm355_attn_prefill_masked_ex / pm_launch_attn_prefill: the documented error comes back and nothing is launched (out keeps
    its sentinel). Every buffer is large enough for the refused shape anyway."""
    torch = P.torch
    a = dict(n_tokens=3, n_head=8, n_head_kv=2, head_dim=128, n_ctx=64, n_kv=32, mask_stride=32)
    a.update({k: v for k, v in change.items() if k != "mask"})
    q = torch.zeros((a["n_tokens"], a["n_head"] * 128), dtype=torch.float32, device="cuda")
    kc = torch.zeros(128 * a["n_head_kv"] * 128, dtype=torch.int16, device="cuda")
    vc = torch.zeros_like(kc)
    mask = None if "mask" in change else torch.zeros((a["n_tokens"] + 32, 128), dtype=torch.float32, device="cuda")
    out = torch.full((a["n_tokens"], a["n_head"] * 128), 12345.0, dtype=torch.float32, device="cuda")
    with pytest.raises(Exception) as ei:
        P.attn_prefill_masked(q, kc, vc, mask, a["n_tokens"], a["n_head"], a["n_head_kv"], a["head_dim"], a["n_ctx"], a["n_kv"], 0.125,
                              mask_stride=a["mask_stride"], out=out)
    assert type(ei.value).__name__ == "PM355Error", ei.value
    got = re.search(r"rc=(-?\d+)", str(ei.value))
    assert got and int(got.group(1)) == rc, (name, str(ei.value))
    torch.cuda.synchronize()
    assert bool((out == 12345.0).all()), name
