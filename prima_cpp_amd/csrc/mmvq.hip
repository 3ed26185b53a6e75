// mmvq.hip — batch-1 quantized mat-vec for gfx950 (the decode hot loop).
//
// Replaces, for tensors in our buffers, the reference's
//   ggml_compute_forward_mul_mat (ggml/src/ggml.c:12377) -> ggml_vec_dot_q4_K_q8_K (ggml-quants.c:7713),
//   ggml_vec_dot_q5_K_q8_K (:8281), ggml_vec_dot_q6_K_q8_K (:8918), ggml_vec_dot_q8_0_q8_0 (:5518), ggml_vec_dot_q5_0_q8_0 (:4789),
// and, fused into its prologue, the activation side of that function: quantize_row_q8_K (ggml-quants.c:3785) /
// quantize_row_q8_0 (:848) preceded, when asked, by ggml_compute_forward_rms_norm_f32 (ggml.c:11950) * weight.
// Integer arithmetic is identical to the reference (int8 x int4/5/6/8 products, int32 sums, 6-bit scales/mins,
// group sums of the int8 activations for the min / -32 terms) and is checked bit-for-bit against the oracle through the
// dbg output; the float scale-and-accumulate uses a fixed, deterministic order.
//
// Design: HBM-bound, 4.5-8.5 bits per weight, no reuse of W -> W goes straight from HBM to registers (no LDS staging).
//  * One 1024-thread workgroup (16 waves) per CU. Each workgroup quantizes the activation row ONCE (from f32, fused rms_norm
//    optional, bit-exact with the reference quantizers) into LDS: int8 values, 16-group sums, block scales.
//  * Each WAVE owns whole rows (2 at a time): lanes stride over the row's UNITS (16-48 contiguous weight bytes = 32/64
//    weights), so a wave instruction covers a contiguous 1-3 KB span of the row -> fully coalesced, every byte of every
//    fetched line is used. Q4_K/Q5_K blocks are 9/11 x 16 B; Q6_K/Q8_0 are stored row-SoA (repack.hip), so every field
//    stream is 16-B aligned. 8-20 independent 16-byte non-temporal loads (global_load_dwordx4 nt) are in flight per lane;
//    16 waves per CU hide the HBM latency. There is NO barrier and NO cross-wave reduction in the row loop.
//  * All weight loads are unconditional (clamped addresses) and the loop body contains no other VMEM operation (row
//    results are parked in LDS and written out coalesced afterwards): gfx9 counts loads and stores in ONE vmcnt and a
//    load in a divergent branch or a store in the stream makes the compiler fall back to s_waitcnt vmcnt(0).
//  * v_dot4_i32_i8 for the products against the LDS-resident activation, DPP reduction per row.
//  * Up to 3 weight matrices that share the activation (wq/wk/wv) are served by ONE launch ("jobs"), of at most two
//    different quant types (Q4_K_M: attn_v is Q6_K/Q5_K next to Q4_K q/k); every workgroup takes an equal slice of
//    the rows of every job.
#include "mmvq_device.h"
#include <stdlib.h>

using namespace pmv;

// what this file serves: every quantized weight type has a QT<> (mmvq_device.h)
constexpr uint32_t GEMV_TYPES = PM_QUANT_WEIGHTS;
// the instantiated (TA, TB) pairs of the fused launch, TA = the type of job 0 (the kernel pre-issues it): one type, or the Q4_K_M mixtures of wq | wk | wv
// (attn_v is Q6_K / Q5_K next to Q4_K). Q8_0 / Q5_0 jobs need Q8_0-quantized activations, the K-quants Q8_K, and one prologue serves one family:
// no pair across the two, and Q5_0 next to Q8_0 in one launch is not instantiated. pm_gemv_fused_plan validates against this list, gemv_kernel_of dispatches over it.
#define PM_GEMV_TYPE_PAIRS(X) X(PM_Q4_K, PM_Q4_K) X(PM_Q5_K, PM_Q5_K) X(PM_Q6_K, PM_Q6_K) X(PM_Q8_0, PM_Q8_0) X(PM_Q5_0, PM_Q5_0) X(PM_Q4_K, PM_Q6_K) X(PM_Q4_K, PM_Q5_K)

// (what the type table says about the mat-vec is what the kernels are compiled with; every type is the TA of some pair)
#define PM_QT_IS(TA_, TB_) static_assert(QT<TA_>::NV == pm_type_info(TA_).nv && QT<TA_>::ABLK == pm_block_len(TA_), "pm355_types.h and QT<> disagree");
PM_GEMV_TYPE_PAIRS(PM_QT_IS)
#undef PM_QT_IS

namespace {

// The first things a workgroup does - the activation loads and the pre-issued weight loads of job 0 - need these values of the argument block: the
// activation, job 0's matrix (its row stride as an int: a row of K <= 122880 values is far below 2 GB) and job 0's slice arithmetic (GemvJob::rpw /
// rmul) - fourteen dwords, all that can be preloaded: sixteen user SGPRs less the two of the kernarg segment pointer. They travel as LEADING
// scalar kernel arguments as well, which the dispatcher preloads into SGPRs (-mllvm -amdgpu-kernarg-preload-count, build.py): the wave issues its loads
// without first waiting for an s_load of the kernarg segment (a by-value struct is never preloaded; neither is gridDim.x, a hidden argument - the
// kernels do not read it). gemv_body issues them before it touches anything else of the block.
// FEAT (mmvq_device.h): PM_FEAT_SS / PM_FEAT_TAIL code lives in instantiations of its own - a launch that uses neither runs the plain kernel
// XM >= 0: the activation mode is a compile-time constant of the instantiation (the hot launches: 1 = f32 row, 2 = rms_norm of an f32 row) - the prologue
// keeps one mode's code instead of four behind scalar branches
// HOT: everything else the decode launches of the Llama-family layer never use is pinned too (no bias, one job outside wq | wk | wv, no residual on
// the pair launch, transposed V cache and - HOT 1: the engine - position-pointer mode / HOT 2: the plug-in - ggml-graph mode in the QKV epilogue):
// gemv_hot_of() checks that the argument block really looks like that
template <int TA, int TB, bool PAIR, bool DBG, bool EPI = false, int NPRE = 2, int FEAT = 0, int XM = -1, int HOT = 0>
#ifdef PM_NO_PRELOAD_ARGS
__global__ __launch_bounds__(PM_GEMV_BLOCK, 4) void gemv_q_kernel(GemvP p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ double nred[PM_GEMV_NW];
#else
__global__ __launch_bounds__(PM_GEMV_BLOCK, 4) void gemv_q_kernel(const float * xf, const float * norm_w, const uint8_t * W0, const uint8_t * W0b, int row_stride0,
                                                                  int K, int xmode, int U0, int rpw0, unsigned rmul0, GemvP p_in) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ double nred[PM_GEMV_NW];
    GemvP p = p_in;
    p.xf = xf; p.norm_w = norm_w; p.K = K; p.xmode = xmode;
    p.job[0].W = W0; p.job[0].W2 = W0b; p.job[0].row_stride = row_stride0; p.job[0].U = U0;
    p.job[0].rpw = rpw0; p.job[0].rmul = rmul0;
#endif
    if constexpr (XM >= 0) p.xmode = XM;
    if constexpr (HOT) {
        p.dbg = nullptr; p.job[0].bias = nullptr;
        if constexpr (EPI) {
            p.job[1].bias = nullptr; p.job[2].bias = nullptr; p.epi.v_rowmajor = 0;
            if constexpr (HOT == 1) p.epi.dyn = nullptr; else __builtin_assume(p.epi.dyn != nullptr);
            p.job[0].role = 1; p.job[1].role = 2; p.job[2].role = 3;                    // wq, wk, wv in this order (no TA-first swap happened)
            p.job[0].is_b = 0; p.job[1].is_b = 0; p.job[2].is_b = TA != TB ? 1 : 0;     // Q4_K_M: wq / wk of the first type, wv of the second (or all of one)
            p.job[0].split = 0; p.job[0].resid = nullptr; p.job[1].resid = nullptr; p.job[2].resid = nullptr;
        } else { p.job[1].N = 0; p.job[2].N = 0; p.job[1].rpw = 0; p.job[2].rpw = 0; p.job[1].rmul = 0; p.job[2].rmul = 0; p.job[0].split = 0; p.job[0].is_b = 0; p.job[0].role = 0; }
        if constexpr (PAIR) p.job[0].resid = nullptr;
        if constexpr (!PAIR && !EPI) __builtin_assume(p.job[0].resid != nullptr);     // wo / ffn_down: always + residual
    }
    // (Q5_K: two 32-weight units per lane and step = 24-VGPR sets with the high-bit plane; a second pre-issued set spills)
    gemv_body<TA, TB, PAIR, DBG, 1, EPI, (TA == PM_Q5_K && NPRE == 2) ? 1 : NPRE, FEAT>(p, smem, nred);
}
// The forms gemv_q_kernel is instantiated in, X(PAIR, DBG, EPI, NPRE, FEAT, XM, HOT), in the launcher's order of preference: gemv_form_of() takes the first row
// the argument block meets. A row requires the launch to be (not) a pair / debug / epilogue launch, to use exactly the features FEAT (gemv_feat_of), to have
// xmode == XM where XM >= 0 (and PM355_XMODE_SPEC not 0), and for HOT to hold already every value the kernel pins (gemv_hot_of; and PM355_HOT_SPEC not 0).
// NPRE asks nothing: 1 pre-issued step where two spill (pair launches: two sets of two matrices; the debug hook: Q6_K sat on the 128-VGPR cliff). Compiled
// (gemv_form_kernel) per pair of PM_GEMV_TYPE_PAIRS; PAIR rows for TA == TB only, TAIL rows for TA == Q4_K only (the Q4_K_M mixtures), SS / TAIL rows in the
// experiments library only - the product library answers -8 for what they serve.
#define PM_GEMV_FORMS(X) \
    X(true,  true,  false, 1, 0, -1, 0)            /* ffn_gate | ffn_up */ \
    X(true,  false, false, 1, PM_FEAT_SS, -1, 0) \
    X(true,  false, false, 1, 0, 2, 1) \
    X(true,  false, false, 1, 0, 2, 0) \
    X(true,  false, false, 1, 0, -1, 0) \
    X(false, false, true,  2, PM_FEAT_SS | PM_FEAT_TAIL, -1, 0)       /* wq | wk | wv with the RoPE + KV-store epilogue */ \
    X(false, false, true,  2, PM_FEAT_TAIL, -1, 0) \
    X(false, false, true,  2, PM_FEAT_NEOX | PM_FEAT_SS, -1, 0) \
    X(false, false, true,  2, PM_FEAT_SS, -1, 0) \
    X(false, false, true,  2, PM_FEAT_NEOX, -1, 0) \
    X(false, false, true,  2, 0, 2, 2) \
    X(false, false, true,  2, 0, 2, 1) \
    X(false, false, true,  2, 0, 2, 0) \
    X(false, false, true,  2, 0, -1, 0) \
    X(false, true,  false, 1, 0, -1, 0)            /* one to three plain jobs: wo, ffn_down, lm_head; wq | wk | wv without the epilogue */ \
    X(false, false, false, 2, PM_FEAT_SS, -1, 0) \
    X(false, false, false, 2, 0, 1, 1) \
    X(false, false, false, 2, 0, 1, 0) \
    X(false, false, false, 2, 0, 2, 0) \
    X(false, false, false, 2, 0, -1, 0)
#define PM_F(...) {__VA_ARGS__},
constexpr pm_gemv_form GEMV_FORMS[] = { PM_GEMV_FORMS(PM_F) };
#undef PM_F
constexpr int N_GEMV_FORMS = (int) (sizeof(GEMV_FORMS) / sizeof(GEMV_FORMS[0])), PM_FEAT_EXP = PM_FEAT_SS | PM_FEAT_TAIL;
typedef decltype(&gemv_q_kernel<PM_Q4_K, PM_Q4_K, false, false>) GemvKernel;
template <int TA, int TB, bool PAIR, bool DBG, bool EPI, int NPRE, int FEAT, int XM, int HOT>
GemvKernel gemv_form_kernel() {
    if constexpr ((PAIR && TA != TB) || ((FEAT & PM_FEAT_TAIL) && TA != PM_Q4_K) || ((FEAT & PM_FEAT_EXP) && !PM_EXPERIMENTS)) return nullptr;
    else return gemv_q_kernel<TA, TB, PAIR, DBG, EPI, NPRE, FEAT, XM, HOT>;
}
#define PM_K(...) gemv_form_kernel<TA, TB, __VA_ARGS__>(),
template <int TA, int TB> GemvKernel gemv_kernel_row(int row) { static const GemvKernel t[] = { PM_GEMV_FORMS(PM_K) }; return t[row]; }
#undef PM_K
GemvKernel gemv_kernel_of(int ta, int tb, int row) {
#define PM_L(TA_, TB_) if (ta == TA_ && tb == TB_) return gemv_kernel_row<TA_, TB_>(row);
    PM_GEMV_TYPE_PAIRS(PM_L)
#undef PM_L
    return nullptr;
}
bool pair_instantiated(int ta, int tb) {
#define PM_IS(TA_, TB_) || (ta == TA_ && tb == TB_)
    return false PM_GEMV_TYPE_PAIRS(PM_IS);
#undef PM_IS
}
// the FEAT a launch needs: producer or consumer of sum-of-squares partials, attention in the tail (its instantiations carry the NEOX row mapping), NEOX rope
int gemv_feat_of(const GemvP & p, bool epi) {
    const int ss = (p.ss_out != nullptr || p.xmode == 3) ? PM_FEAT_SS : 0;
    if (epi && p.epi.att_out != nullptr) return ss | PM_FEAT_TAIL;
    return ss | (epi && (p.job[0].nx_s > 0 || p.job[1].nx_s > 0 || p.job[2].nx_s > 0) ? PM_FEAT_NEOX : 0);
}
// the HOT a launch may take: 0, or the variant whose pinned values (gemv_q_kernel) the block holds anyway - else the kernel would drop a bias, a residual or a job
int gemv_hot_of(const GemvP & p, bool mixed, bool pair, bool epi) {
    const GemvJob * j = p.job;
    if (j[0].bias || j[0].split) return 0;
    // one job: ffn_gate | ffn_up without a residual; wo / ffn_down always with one
    if (!epi) return j[1].N == 0 && j[2].N == 0 && (pair ? !j[0].resid : j[0].resid && !j[0].is_b) ? 1 : 0;
    // wq, wk, wv in this order (no TA-first swap), wv alone of the second type, transposed V cache; 1: position pointer (the engine), 2: ggml-graph mode (the plug-in)
    if (j[1].bias || j[2].bias || j[0].resid || j[1].resid || j[2].resid || p.epi.v_rowmajor) return 0;
    if (j[0].role != 1 || j[1].role != 2 || j[2].role != 3 || j[0].is_b || j[1].is_b || j[2].is_b != (mixed ? 1 : 0)) return 0;
    return p.epi.dyn ? 2 : 1;
}
// Which row of PM_GEMV_FORMS a filled argument block launches, or the refusal (pm355_kernels.h). Pure host logic: the only place the launcher's conditions live
int gemv_form_of(const GemvP & p, int ta, int tb, bool pair, bool epi, bool dbg, bool xm_spec, bool hot_spec) {
    const int feat = gemv_feat_of(p, epi), hot = hot_spec ? gemv_hot_of(p, ta != tb, pair, epi) : 0;
    if (!PM_EXPERIMENTS && (feat & PM_FEAT_EXP)) return -8;
    if ((pair && ta != tb) || (epi && dbg)) return -1;
    if (dbg && (feat & PM_FEAT_SS)) return -6;
    if ((feat & PM_FEAT_TAIL) && ta != PM_Q4_K) return -7;
    for (int r = 0; r < N_GEMV_FORMS; ++r) {
        const pm_gemv_form & f = GEMV_FORMS[r];
        if (f.pair == pair && f.dbg == dbg && f.epi == epi && f.feat == feat && (f.xm < 0 || (xm_spec && p.xmode == f.xm)) && (!f.hot || f.hot == hot)) return r;
    }
    return -1;
}

} // namespace

static int g_num_cus_dev[16] = {};
int pm_device_cus() {
    const int dv = pm_cur_dev();
    if (!g_num_cus_dev[dv]) { hipDeviceProp_t pr; g_num_cus_dev[dv] = hipGetDeviceProperties(&pr, dv) == hipSuccess ? pr.multiProcessorCount : 256; }
    return g_num_cus_dev[dv];
}

// (a type the mat-vec does not serve answers K / 32 as it always did: the launch that follows refuses it)
int pm_gemv_units_per_row(int type, int64_t K) { const int nv = pm_type_info(type).nv; return (int) (K / (nv ? nv : 32)); }

size_t pm_weight_row_stride(int type, int64_t K) {
    if (!pm_type_info(type).pad) return pm_weight_row_bytes(type, K);
    const size_t nb = (size_t) (K / pm_block_len(type));            // the types with a padded stream, each with its layout's function (pm355_device.h)
    return type == PM_Q6_K ? pm_q6k_row_stride(nb) : type == PM_Q5_0 ? pm_q50_row_stride(nb) : pm_q80_row_stride(nb);
}

// Validates a fused job list, fills the kernel argument block and chooses the grid, the LDS bytes and the kernel form. (ta, tb) are the (at most two) quant
// types in the order of one of the instantiated kernels (PM_GEMV_TYPE_PAIRS); job 0 is always a `ta` job (the kernel pre-issues it).
int pm_gemv_fused_plan(const pm_gemv_fused & a, int cus, pm_gemv_plan & out) {
    if (a.njobs < 1 || a.njobs > 3) return -9;
    GemvP & p = out.p = GemvP{};
    p.K = a.K; p.xq = (const uint8_t *) a.xq; p.xf = a.xf; p.norm_w = a.norm_w; p.eps = a.eps; p.dbg = a.dbg_int;
    p.xmode = a.xq ? 0 : (a.norm_w ? (a.ss_in ? 3 : 2) : 1);
    if (a.ss_in && (!a.norm_w || a.xq || a.n_ss < 1 || a.n_ss > 256)) return -6;
    if (a.ss_out && (a.njobs != 1 || a.job[0].W2 || a.epi || a.dbg_int)) return -6;
    p.ss_out = a.ss_out; p.ss_in = a.ss_in; p.n_ss = a.n_ss;
    int ta = a.job[0].type, tb = ta;
    const bool pair = a.job[0].W2 != nullptr;
    for (int j = 0; j < a.njobs; ++j) {
        const int t = a.job[j].type;
        if (!pm_in_set(GEMV_TYPES, t)) return -1;
        if (t != ta) { if (tb == ta) tb = t; else if (t != tb) return -1; }
        if ((a.job[j].W2 != nullptr) != pair) return -1;
    }
    if (pm_q80_family(ta) != pm_q80_family(tb)) return -1;            // one prologue serves only one activation family
    if (a.K % pm_block_len(ta)) return -2;
    if (pair && ta != tb) return -1;
    if (!pair_instantiated(ta, tb)) {                                 // the jobs may come in the other order (wv first)
        const int t = ta; ta = tb; tb = t;
        if (!pair_instantiated(ta, tb)) return -1;
    }
    // one workgroup of 16 waves per CU; every workgroup takes an equal slice of the rows of EVERY job
    int grid = (1024 / PM_GEMV_BLOCK) * (cus > 0 ? cus : pm_device_cus());
    long tot_rows = 0;
    for (int j = 0; j < a.njobs; ++j) tot_rows += a.job[j].N;
    while ((tot_rows + grid - 1) / grid + 3 > PM_MAX_ROWS_PER_WG && grid < 65536) grid *= 2;
    if (grid >= 65536) return -2;                                     // (over 33 million rows: GemvJob::rmul is exact below that)
    for (int j = 0; j < 3; ++j) {
        GemvJob & g = p.job[j];
        if (j >= a.njobs) { g.N = 0; continue; }
        const pm_gemv_job & s = a.job[j];
        const int nv = pm_type_info(s.type).nv;
        g.W = (const uint8_t *) s.W; g.W2 = (const uint8_t *) s.W2; g.y = s.y; g.bias = s.bias; g.resid = s.resid;
        g.N = s.N; g.is_b = (s.type != ta); g.U = a.K / nv;
        // the slices [floor(N b / grid), floor(N (b + 1) / grid)) as a multiply and a multiply-high. With rem = N % grid and eps = rmul * grid - 2^32 * rem
        // (0 <= eps < grid): b * rmul / 2^32 = b * rem / grid + b * eps / (grid * 2^32), and the last term stays under 1 / grid - it cannot carry the
        // fraction of b * rem / grid (at most (grid - 1) / grid) over the next integer - as long as b * eps < 2^32, which b <= grid < 65536 guarantees
        g.rpw = s.N / grid; g.rmul = (unsigned) ((((unsigned long long) (s.N % grid) << 32) + (unsigned) grid - 1) / (unsigned) grid);
        g.row_stride = (long) pm_weight_row_stride(s.type, a.K);
        g.role = 0; g.split = 0;
        if (a.epi) {
            // wq | wk | wv with the RoPE + KV-store epilogue: every workgroup's slice must hold whole rotation pairs; a matrix that gives a
            // workgroup fewer rows than it has waves is dealt out step by step (row, chunk) so that all 16 waves share its rows
            if (pair || a.njobs != 3 || s.N % (2 * grid) || a.dbg_int) return -5;
            g.role = j + 1;
            const int upl = (g.U + 63) >> 6, ch = nv == 64 ? PM_CH64 : PM_CH32, cpr = (upl + ch - 1) / ch;
            g.split = (j > 0 && s.N / grid < PM_GEMV_NW && cpr > 1) ? 1 : 0;
            if (a.epi->neox && j < 2) {
                // NEOX pairs (i, i + n_rot / 2): the slice of every workgroup = two runs of sl / 2 rows, n_rot / 2 apart, inside one head
                const int sl = s.N / grid, dh = a.epi->dh;
                auto pow2 = [](int v) { return v > 0 && !(v & (v - 1)); };
                if (a.epi->n_rot != dh || !pow2(dh) || !pow2(sl) || sl < 2 || sl > dh) return -5;
                int ls = 0, ld = 0;
                while ((1 << ls) < sl) ++ls;
                while ((1 << ld) < dh) ++ld;
                g.nx_s = ls; g.nx_dh = ld; g.nx_hrot = a.epi->n_rot / 2;
            }
        }
    }
    size_t att_lds = 0;
    if (a.epi) {
        const pm_qkv_epi & e = *a.epi;
        if (e.dh % 2 || e.n_rot % 2 || e.n_rot > e.dh || a.job[0].N % e.dh || a.job[1].N != e.Hkv * e.dh || a.job[2].N != e.Hkv * e.dh) return -5;
        // (ggml-graph mode has no position pointer: the scalar loads of the un-taken branch may still be issued - give them a valid address)
        p.epi = QkvEpi{e.tab, e.pos ? e.pos : e.dyn, e.seq, e.dyn, e.seq_stride, (uint16_t *) e.kc, (uint16_t *) e.vc, e.Hkv * e.dh, e.dh, e.n_ctx, e.n_rot, e.v_rowmajor, e.neox,
                       nullptr, nullptr, nullptr, nullptr, 0.0f, 0, 0};
        if (e.att_out) {
            // attention in the tail: the workgroups of a KV-head group must be a power-of-two run of the grid, at least one per query head of the group
            const int wgs = e.Hkv > 0 && grid % e.Hkv == 0 ? grid / e.Hkv : 0, nh = e.Hkv > 0 ? e.n_head / e.Hkv : 0;
            const int mk = e.att_max_keys > 0 && e.att_max_keys < e.n_ctx ? e.att_max_keys : e.n_ctx;
            if (!e.pos || e.dyn || !e.att_ticket || e.v_rowmajor || wgs < 1 || (wgs & (wgs - 1)) || nh < 1 || nh > wgs || e.n_head != nh * e.Hkv || a.job[0].N != e.n_head * e.dh ||
                (e.dh != 64 && e.dh != 128) || e.n_ctx % 8 || e.n_ctx < 64) return -7;
            att_lds = 64 + attn_tail_lds(e.dh, mk);
            p.epi.att_out = e.att_out; p.epi.att_q = a.job[0].y; p.epi.att_ticket = e.att_ticket; p.epi.att_err = e.att_err; p.epi.att_scale = e.kq_scale;
            p.epi.att_H = e.n_head; p.epi.att_wgs = wgs;
        }
    }
    out.first = 0;
    if (p.job[0].is_b)                                // the kernel pre-issues job 0 with the TA code path: put a TA job first
        for (int j = 1; j < 3; ++j) if (p.job[j].N > 0 && !p.job[j].is_b) { const GemvJob t = p.job[0]; p.job[0] = p.job[j]; p.job[j] = t; out.first = j; break; }
    size_t lds = pm_gemv_act_lds(a.K, pm_block_len(ta)) + (size_t) PM_MAX_ROWS_PER_WG * 4;
    if (att_lds > lds) lds = att_lds;
    if (lds > 150 * 1024) return -4;
    static const bool xm_spec = [] { const char * e = getenv("PM355_XMODE_SPEC"); return !(e && e[0] == '0'); }();     // (A/B switches)
    static const bool hot_spec = xm_spec && [] { const char * e = getenv("PM355_HOT_SPEC"); return !(e && e[0] == '0'); }();
    if ((out.row = gemv_form_of(p, ta, tb, pair, a.epi != nullptr, a.dbg_int != nullptr, xm_spec, hot_spec)) < 0) return out.row;
    out.ta = ta; out.tb = tb; out.pair = pair; out.grid = grid; out.lds = lds; out.form = GEMV_FORMS[out.row];
    return 0;
}

static int gemv_launch_plan(pm_gemv_plan & pl, hipStream_t st) {
    const GemvKernel kern = gemv_kernel_of(pl.ta, pl.tb, pl.row); if (!kern) return -1;
    GemvP & p = pl.p; p.ts = pm_ts_next_slot();
    pm_allow_big_lds((const void *) kern, pl.lds);
#ifdef PM_NO_PRELOAD_ARGS
    hipLaunchKernelGGL(kern, dim3(pl.grid), dim3(PM_GEMV_BLOCK), pl.lds, st, p);
#else
    hipLaunchKernelGGL(kern, dim3(pl.grid), dim3(PM_GEMV_BLOCK), pl.lds, st, p.xf, p.norm_w, p.job[0].W, p.job[0].W2, (int) p.job[0].row_stride, p.K, p.xmode, p.job[0].U,
                       p.job[0].rpw, p.job[0].rmul, p);
#endif
    return 0;
}

// Fused launch: up to 3 matrices sharing one activation row.
int pm_launch_gemv_fused(const pm_gemv_fused & a, hipStream_t st) {
    pm_gemv_plan pl; const int rc = pm_gemv_fused_plan(a, 0, pl);
    return rc ? rc : gemv_launch_plan(pl, st);
}

// Column slots of a launch with `left` columns to go: 8 / 4 / 2 share one pass over the weights (gemv_q_cols_kernel), 1 = one launch per column
int pm_gemv_col_slots(int type, bool pair, int left) {
    if (left < 2) return 1;
    if (pair) return pm_in_set(GEMV_PAIR_COLS_TYPES, type) ? 2 : 1;  // pair launches: 2 columns, for Q4_K / Q6_K only (mmvq_device.h)
    if (left >= 8 && type != PM_Q5_K) return 8;                       // (8 Q5_K columns spill even at 256 VGPRs)
    return left >= 3 ? 4 : 2;                                         // (3 columns take the 4-slot form with one slot idle: one pass instead of 2 + 1)
}

// Single-matrix entry with ncols pre-quantized activation columns: groups of 8 / 4 / 2 columns share one pass over the
// weights (gemv_q_cols_kernel), a remaining single column - and pair / debug launches - go one launch per column.
int pm_launch_gemv(const pm_gemv_args & a, hipStream_t st) {
    const size_t xrow = pm_q80_family(a.type) ? pm_q80_row_bytes(a.K) : pm_q8k_row_bytes(a.K);
    int c = 0;
    while (c < a.ncols) {
        pm_gemv_fused f = {};
        f.K = a.K; f.njobs = 1; f.xq = (const uint8_t *) a.xq + (size_t) c * xrow; f.dbg_int = a.dbg_int;
        f.job[0].type = a.type; f.job[0].N = a.N; f.job[0].W = a.W; f.job[0].W2 = a.W2;
        f.job[0].y = a.y + (size_t) c * a.y_stride; f.job[0].bias = a.bias;
        f.job[0].resid = a.resid ? a.resid + (size_t) c * a.y_stride : nullptr;
        pm_gemv_plan pl;                                  // one plan per column group, whichever kernel takes it
        int rc = pm_gemv_fused_plan(f, 0, pl); if (rc) return rc;
        const int left = a.ncols - c;
        int nc = a.dbg_int ? 1 : pm_gemv_col_slots(a.type, pl.pair, left);
        // LDS: nc activation columns + nc results per row
        const size_t col = pm_gemv_act_lds(a.K, pm_block_len(pl.ta)), rows = (size_t) ((a.N + pl.grid - 1) / pl.grid + 4);
        while (nc > 1 && nc * col + rows * nc * 4 > 150 * 1024) nc /= 2;
        int served = 1;
        if (nc > 1) {
            served = left < nc ? left : nc;
            pl.p.ncols = served; pl.p.xq_stride = (long) xrow; pl.p.y_stride = (long) a.y_stride;
            rc = pm_launch_gemv_cols(pl.ta, pl.p, nc, pl.pair, pl.grid, nc * col + rows * nc * 4, st);      // mmvq_cols.hip (512-thread workgroups, 256-VGPR budget)
        } else rc = gemv_launch_plan(pl, st);
        if (rc) return rc;
        c += served;
    }
    return 0;
}
