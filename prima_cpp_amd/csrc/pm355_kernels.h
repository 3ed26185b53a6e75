// pm355_kernels.h — internal launcher prototypes (host side) for the gfx950 kernels.
#pragma once
// PM_EXPERIMENTS: round 5's three measured-slower forms of the decode layer - producer-side sums of squares, attention in the tail of the QKV launch, the persistent
// engine (decode_engine.hip) - are compiled ONLY into prima_cpp_amd/libprima_mi355_exp.so (build.py build_experiments(), -DPM_EXPERIMENTS=1), which their tests load.
// The product library libprima_mi355.so (what prima.cpp links) carries none of them: the entry points answer PM355_E_UNSUPPORTED there.
#ifndef PM_EXPERIMENTS
#define PM_EXPERIMENTS 0
#endif
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "pm355_types.h"

// index of the current HIP device for the per-device one-time state of the launchers (a process may drive up to 16 GPUs
// through the plug-in: hipFuncSetAttribute and the CU count are per device, not per process)
static inline int pm_cur_dev() { int d = 0; return (hipGetDevice(&d) == hipSuccess && d >= 0 && d < 16) ? d : 0; }

// THE opt-in to more than 48 KiB of dynamic LDS, for every launcher of the product sources: one hipFuncSetAttribute(MaxDynamicSharedMemorySize, limit) per (kernel, device),
// made by the first launch that needs it - later launches make no runtime call (none inside a stream capture either). Keyed on the kernel POINTER: a `static bool` inside a
// generic lambda is shared by every instantiation that decays to the same function-pointer type, so only the first kernel launched would get it. No lock: the call is idempotent,
// a lost race sets it twice. The table is one copy per translation unit (static inline): a kernel is launched only from the file that defines it, so no two copies hold one pointer.
static inline void pm_allow_big_lds(const void * kern, size_t lds, size_t limit = 150 * 1024) {
    if (lds <= 48 * 1024) return;
    struct E { const void * k; int dev; };
    static E done[256]; static int n_done = 0;
    static hipError_t (*set)(const void *, hipFuncAttribute, int) = hipFuncSetAttribute;
    const int dev = pm_cur_dev();
    for (int i = 0; i < n_done && i < 256; ++i) if (done[i].k == kern && done[i].dev == dev) return;
    (void) set(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int) limit);
    if (n_done < 256) { done[n_done].k = kern; done[n_done].dev = dev; ++n_done; }
}

// bytes of one quantized ACTIVATION row in the library's internal row-SoA layout (quantize.hip)
static inline size_t pm_q8k_row_bytes(int K) { return (size_t) K + (size_t) (K / 256) * 4 + (size_t) (K / 16) * 2; }
static inline size_t pm_q80_row_bytes(int K) { return (size_t) K + (size_t) (K / 32) * 2; }

// (bytes of one WEIGHT row in GGUF order: pm_weight_row_bytes, pm355_types.h)
// row STRIDE in HBM: == row bytes except that the trailing fp16 scale stream of the row-SoA layouts
// (Q6_K, Q8_0, Q5_0) is padded to 16 B so every row (and every field stream) starts 16-B aligned for any K
size_t pm_weight_row_stride(int type, int64_t K);
int pm_gemv_units_per_row(int type, int64_t K);
  // units of the mat-vec's per-(row, unit) debug partials

// optional second output of the Q8_K quantizers: the activation tables of the small-batch mat-mul (mmq_i8.hip: per 32-row pass, the F16
// 16-value sums in MFMA operand order | the transposed block scales) - that mat-mul then needs no prologue launch. base == null: off
// qbase (optional third table, mmq_i8.hip): the int8 values themselves in the matrix cores' A-operand order, nsb * 8192 bytes per 32 rows -
// [super-block][32-value sub-block s][operand lane = 32 * (k / 16 % 2) + row % 32][16 bytes]: one coalesced load per sub-block instead of one
// cache line per token
struct pm_q8k_tables { uint8_t * base = nullptr; size_t tab_bytes = 0; int nsb = 0; uint8_t * qbase = nullptr; };
// bytes of one 32-row pass of the first two tables: per 256-value super-block 64 lanes x 8 F16 sums | 32 f32 scales
static inline size_t pm_q8k_tab_bytes(int K) { return (size_t) (K / 256) * (1024 + 128); }
static inline pm_q8k_tables pm_q8k_tables_at(void * base, int K, void * qbase = nullptr) { return {(uint8_t *) base, pm_q8k_tab_bytes(K), K / 256, (uint8_t *) qbase}; }
void pm_launch_quantize_q8k(const float * x, void * y, int K, int rows, hipStream_t st, pm_q8k_tables tab = {});
void pm_launch_quantize_q80(const float * x, void * y, int K, int rows, hipStream_t st);
// silu(gate) * up -> Q8_0, written into the Q8_0 small-batch mat-mul's activation tables (pm_mmq_i8_q80_tables); then pm_launch_mmq_i8 with tables_ready
void pm_launch_silu_mul_q80_tab(const float * gate, const float * up, void * tab, size_t qtab_bytes, size_t dtab_bytes, int K, int rows, hipStream_t st);
int pm_mmq_i8_q80_tables(int K, hipStream_t st, void ** tab, size_t * qtab_bytes, size_t * dtab_bytes);
// Q8_K rows of silu(gate) * up (the ffn_down activations of a small batch), no f32 product in HBM
void pm_launch_silu_mul_q8k(const float * gate, const float * up, void * y, int K, int rows, hipStream_t st, pm_q8k_tables tab = {});
void pm_launch_rmsnorm_q8k(const float * x, const float * w, float * ynorm, void * yq, int K, int rows, float eps, hipStream_t st, void * ynorm_f16 = nullptr,
                           pm_q8k_tables tab = {});

// weight repack (row-local, bijective):  GGUF block order <-> HBM row-SoA (Q4_K, Q6_K, Q8_0, Q5_0); identity for the rest
void pm_launch_repack(int type, const void * src, void * dst, int64_t K, int64_t nrows, int to_device_layout, hipStream_t st);

// y[N] = W[N,K] . xq (+bias)(+resid);  optional second matrix W2 (same type/shape): y = silu(W.x) * (W2.x)
struct pm_gemv_args {
    int type; int K; int N;
    const void * W; const void * W2;
    const void * xq;            // quantized activation row(s) (Q8_K row-SoA, or Q8_0 row-SoA for Q8_0 / Q5_0 weights)
    int ncols;                  // 1..8 activation columns (rows of xq, stride = row bytes)
    float * y; size_t y_stride; // y[col * y_stride + n]
    const float * bias;         // [N] or null
    const float * resid;        // same indexing as y, or null
    int32_t * dbg_int;          // debug: per (row, unit) {isum, msum} pairs, or null
};
int pm_launch_gemv(const pm_gemv_args & a, hipStream_t st);
// activation columns one launch of pm_launch_gemv takes in one pass over the weights when `left` columns remain: 8 / 4 / 2, or 1 (one launch per column)
int pm_gemv_col_slots(int type, bool pair, int left);

// Fused single-token launch: up to 3 matrices (same K) sharing ONE activation row, which is either pre-quantized
// (xq) or given in f32 (xf) and quantized in the kernel prologue, optionally after rms_norm(xf, eps) * norm_w.
struct pm_gemv_job {
    int type; int N;
    const void * W; const void * W2;    // W2 != null: y = silu(W.x) * (W2.x) (all jobs of a launch alike)
    float * y; const float * bias; const float * resid;
};
// RoPE + KV store in the epilogue of a wq | wk | wv launch (jobs in that order). Served for NORM-mode rope when every workgroup's row
// slices start and end on even rows (pm_gemv_fused_plan tells); tab = this token's cos / sin table (pm_launch_rope_table)
struct pm_qkv_epi {
    const float * tab; const int32_t * pos, * seq, * dyn; long seq_stride;
    void * kc, * vc; int Hkv, dh, n_ctx, n_rot, v_rowmajor;
    int neox;                           // rope mode 2 (build_qwen2): pairs (i, i + n_rot / 2); needs n_rot == head_dim and power-of-two slices
    // attention in the launch's tail (round 5): att_out != null - the workgroups of one KV-head group (its query rows, its K rows and its V rows all
    // live in the same grid / Hkv workgroups) take a ticket after their RoPE / KV stores; the last n_head / Hkv of them wait for the group to be
    // complete and compute one query head each over the cached cells (attn_tail_device.h: attn_cached.hip's arithmetic, the same bits) - the
    // attention launch and its boundary disappear. att_ticket: Hkv counters (zeroed once, monotonic), att_err: watchdog word (a bounded wait gave up).
    // Position-pointer mode only (pos != null, dyn == null); -7 when the shape is not served (then launch pm_launch_attn_cached as before)
    float * att_out; unsigned * att_ticket; int * att_err; float kq_scale; int n_head, att_max_keys;
};
struct pm_gemv_fused {
    int K; int njobs;
    pm_gemv_job job[3];
    const void * xq;                    // pre-quantized activation row, or null
    const float * xf; const float * norm_w; float eps;
    int32_t * dbg_int;
    const pm_qkv_epi * epi;             // null: plain outputs
    // producer-side sum of squares for the NEXT launch's rms_norm (round 5): ss_out != null (single job, no pair, no epilogue) - every workgroup
    // stores the f64 sum of the f32-rounded squares of the output rows it wrote into ss_out[workgroup] (pm_gemv_plan::grid of them);
    // ss_in != null (with norm_w): the n_ss <= 256 partials a producer left for THIS launch's input row replace the in-kernel reduction
    double * ss_out; const double * ss_in; int n_ss;
};
namespace pmv {     // the kernel argument block of the mat-vec: mmvq_device.h reads it, pm_gemv_fused_plan fills it, pm_gemv_plan holds it
struct GemvJob {
    const uint8_t * W; const uint8_t * W2; float * y; const float * bias; const float * resid;
    long row_stride;
    int N, is_b /*uses TB*/, U /*units per row*/;
    int role;    // QKV epilogue (GemvP::epi): 0 none, 1 = query rows (rotate, round to F16), 2 = key rows (rotate, store in the K cache), 3 = value rows (store in the V cache)
    int split;   // items of this job are (row, chunk) steps instead of whole rows: a few long rows spread over all waves (wk / wv next to wq)
    // NEOX rope in the QKV epilogue (build_qwen2): a rotation pair is (i, i + n_rot / 2) of one head (ggml.c:14238-14253), so a workgroup's slice of
    // s = 2^nx_s rows is made of TWO runs of s / 2 rows, n_rot / 2 apart: logical row L of the job (what the item loops count in) is matrix row
    // job_row(L). nx_s == 0: identity (NORM rope pairs adjacent rows; every other job).
    int nx_s, nx_dh /*log2 head_dim*/, nx_hrot /*n_rot / 2*/;
    // This job's slice of workgroup b is [at(b), at(b + 1)), at(b) = floor(N * b / grid) = b * rpw + mulhi32(b, rmul) with rpw = N / grid and
    // rmul = ceil(2^32 * (N % grid) / grid): exact for 0 <= b <= grid < 65536 (pm_gemv_fused_plan proves it and refuses larger grids). N % grid == 0 - every
    // launch of a decode layer - gives rmul = 0, a plain multiply. The kernels neither divide nor read the grid size (pmv::slice_at, mmvq_device.h).
    int rpw; unsigned rmul;
};
// RoPE + F16 KV store in the epilogue of the wq | wk | wv launch (NORM-mode rope: a pair = two adjacent rows of one workgroup's slice).
// tab[i] = (cos, sin) of rotation pair i at this token's position, built once per token by rope_table_kernel (layer_ops.hip) with the
// reference's running product (ggml_rope_cache_init, ggml.c:14117-14131); cell / sequence as in attn_device.h (dyn: ggml-graph mode).
struct QkvEpi {
    const float * tab; const int32_t * pos_ptr, * seq_ptr, * dyn; long seq_stride;
    uint16_t * kc, * vc; int kv_dim /*Hkv * dh*/, dh, n_ctx, n_rot, v_rowmajor;
    int neox;    // rotation pairs (i, i + n_rot / 2) instead of (2 i, 2 i + 1): the q / k jobs carry the row mapping (GemvJob::nx_s)
    // attention in the tail (pm_qkv_epi::att_out): q = the rotated query rows this launch stores, wgs = workgroups per KV-head group (power of two)
    float * att_out; const float * att_q; unsigned * att_ticket; int * att_err; float att_scale; int att_H, att_wgs;
};
struct GemvP {
    GemvJob job[3];
    const uint8_t * xq;                     // xmode 0: pre-quantized activation row (row-SoA Q8_K / Q8_0)
    const float * xf; const float * norm_w; // xmode 1: f32 activation; xmode 2: rms_norm(xf) * norm_w first; xmode 3: the same with the
                                            // sum of squares of xf taken from the PRODUCER's per-workgroup partials (ss_in[n_ss], see ss_out)
    float eps;
    // producer-side sum of squares (round 5): a single-job launch whose output row is the next launch's rms_norm input stores, per workgroup,
    // the f64 sum of the f32-rounded squares of the rows it wrote (ss_out[blockIdx.x]); the consuming launch (xmode 3) adds the n_ss partials
    // instead of reducing the row itself - its prologue loses the reduction pass and one workgroup barrier (ggml.c:11975-11980: the reference
    // sums (ggml_float)(x[i] * x[i]) in f64; any order of these <= 2^15 terms agrees after the final rounding to f32, as for xmode 2)
    double * ss_out; const double * ss_in; int n_ss;
    int xmode, K;
    int32_t * dbg;
    int ncols;                              // activation columns served by one launch (xmode 0 only when > 1)
    long xq_stride, y_stride;               // bytes between quantized activation rows; floats between output columns
    unsigned long long * ts;                // measurement builds (-DPM_TS): this launch's timestamp slot, else null
    QkvEpi epi;                             // used by the EPI instantiation only
};
}
struct pm_gemv_form { int pair, dbg, epi, npre, feat, xm, hot; };      // gemv_q_kernel<TA, TB, PAIR, DBG, EPI, NPRE, FEAT, XM, HOT>: a row of PM_GEMV_FORMS (mmvq.hip)
// What pm_launch_gemv_fused will launch for a job list: the filled argument block, the (ta, tb) pair of PM_GEMV_TYPE_PAIRS (job 0 of the block is a `ta` job;
// `first` = the input job that went there), the grid, the dynamic LDS bytes and the kernel form. Host arithmetic only, no pointer is followed.
struct pm_gemv_plan { pmv::GemvP p; int ta, tb, pair, grid, first, row /*of PM_GEMV_FORMS*/; size_t lds; pm_gemv_form form; };
// LDS bytes of one quantized activation column of K values with ablk-value scale blocks: int8 values | 16-group sums | block scales
static inline size_t pm_gemv_act_lds(int K, int ablk) { return (size_t) ((K + 15) & ~15) + (size_t) (K / 16) * 4 + (size_t) ((K / ablk + 3) & ~3) * 4; }
// Return codes of the mat-vec launchers (pm_gemv_fused_plan, pm_launch_gemv_fused, pm_launch_gemv; pm_eng_plan_add_matvec passes them on): 0 served;
//   -1 a weight type or type mix no kernel is instantiated for, pair jobs next to plain ones, a debug launch with the epilogue; -2 K is no multiple of the
//   type's block length, or so many rows that the grid reaches 65536 workgroups (the slice arithmetic, GemvJob::rmul); -4 the activation (or the attention tail) does not fit 150 KB of LDS; -5 the RoPE + KV-store epilogue does not serve the list (not
//   three plain jobs, rows per workgroup not whole rotation pairs, head / NEOX slice conditions); -6 sum-of-squares arguments (ss_in without norm_w / with xq /
//   n_ss outside 1..256, ss_out on anything but ONE plain job, either with a debug launch); -7 attention tail (grid no power-of-two run per KV head, head_dim,
//   position-pointer mode, transposed V cache, wq Q4_K); -8 sum of squares / tail asked of the product library (PM_EXPERIMENTS only); -9 njobs outside 1..3
int pm_gemv_fused_plan(const pm_gemv_fused & a, int cus, pm_gemv_plan & out);     // cus <= 0: the current device's CU count
int pm_launch_gemv_fused(const pm_gemv_fused & a, hipStream_t st);     // plan, then launch the plan

// batched (prefill) GEMM on MFMA: up to 4 matrices W_j [N_j][K] (quantized, HBM layout) over the same activations x [T][K]. Job: Y[t * ldy + n] (f32) or, when
// Yh != null, Yh[t * ldy + n] (F16; Y is not written) = W . x (+ bias[n]) (+ resid[t * ldy + n]) (* silu(silu_gate[t * ldy + n])); ldy == 0 means N.
// pair != 0: jobs = {ffn_gate, ffn_up}, jobs[1]'s output = silu(W0 . x) * (W1 . x). The routing between the kernel generations is written at pm_launch_gemm
// (mmq.hip). 0, or -1 type / -2 shape / -3 device or scratch / -5 a pair launch that is not served and has no f32 gate buffer (jobs[0].Y) to fall back on
struct pm_gemm_job { int type; int N; const void * W; float * Y; void * Yh; const float * bias; const float * resid; const float * silu_gate; long ldy; };
struct pm_gemm_acts { const float * f32; const void * f16; };      // exactly one is non-null; f32 is converted once per call into a per-device F16 scratch
int pm_launch_gemm(const pm_gemm_job * jobs, int njobs, pm_gemm_acts x, int K, int T, int pair, hipStream_t st);

// the third generation (mmq_pf.hip; Q4_K / Q5_K / Q6_K / Q8_0, at most two types per launch) behind pm_launch_gemm: pm_gemm_pf_check: 0 when (type, K, N, T)
// is served, -1 type, -2 shape; pm_launch_gemm_pf_ex: ONE launch over jobs that all pass it, xh = the F16 activations
struct pm_gemm_pf_plan_t { int nt, nt_t, splitk, full, grid; double cost; };
void pm_gemm_pf_plan(int tiles, int K, int T, int cus, int force_nt, int force_s, int allow_mixed, pm_gemm_pf_plan_t * out);   // host arithmetic only (mmq_pf.hip)
int pm_gemm_pf_check(int type, int K, int N, int T);
int pm_launch_gemm_pf_ex(const pm_gemm_job * jobs, int njobs, const void * xh, int K, int T, int pair, hipStream_t st);

int pm_device_cus();
struct pm_rope_cfg;

// small-batch (1..64 tokens) quantized mat-mul on the integer matrix cores (mmq_i8.hip): quantized weights x Q8_K activations (Q8_0 / Q5_0 weights: Q8_0
// activations). ONE entry over a job list - the routing between its three forms (single, multi-job, two-part grid) is written at pm_launch_mmq_i8
// (mmq_i8.hip). 0, or -1 type / -2 shape / -4 LDS (one job), -3 device or scratch, -5 a list (or epilogue) no form serves: the caller splits it
struct pm_mmq_job  { int type; int N; const void * W; float * y; const float * bias; const float * resid; };
struct pm_mmq_acts { const void * xq; const float * f32; int tables_ready; };   // xq: quantized rows, or null and f32 [T][K]; tables_ready: no prologue launch
int pm_launch_mmq_i8(const pm_mmq_job * jobs, int njobs, pm_mmq_acts x, int K, int T, const pm_qkv_epi * epi, hipStream_t st);
int pm_mmq_i8_check(int type, int K, int N, int T);                    // 0 when ONE job of this shape is served
int pm_mmq_i8_tables(int K, hipStream_t st, pm_q8k_tables * out);      // where a quantizer writes the tables for K (<= 64 rows); then tables_ready = 1
int pm_launch_mmq_i8_prep(const void * xq, int K, int T, hipStream_t st);      // the activation tables alone (then tables_ready = 1)
// the launcher's own arithmetic for a list on a device of `cus` CUs, host only: per pass the form, the tokens, the result registers per lane of the
// instantiation (NV: 4 / 8 / 16) and grid / rgb_log2 of each part ([1]: part b of the two-part grid, else 0). 0, or the launcher's refusal
enum { PM_MMQ_SINGLE = 0, PM_MMQ_MULTI = 1, PM_MMQ_DUAL = 2 };
struct pm_mmq_pass { int form, t0, tn, nv, grid[2], rgb_log2[2]; };
struct pm_mmq_plan_t { int npass; pm_mmq_pass pass[4]; };
int pm_mmq_i8_plan(const pm_mmq_job * jobs, int njobs, int K, int T, int epi, int cus, pm_mmq_plan_t * out);

// prompt-sized batches (>= 128 tokens) on the integer matrix cores (mmq_big.hip): Q4_K / Q6_K weights x Q8_K activations, the CPU reference's
// integer arithmetic. xq = T rows of row-SoA Q8_K, tab = the activation tables a quantizer wrote for them (pm_q8k_tables{tab, (K / 256) * 1152, K / 256};
// pm_mmq_big_table_bytes(K, T) bytes). 0, or -1 type / -2 shape / -3 device
int pm_mmq_big_check(int type, int K, int N, int T);
size_t pm_mmq_big_table_bytes(int K, int T);
int pm_launch_mmq_big(int type, const void * W, const void * xq, const void * tab, float * Y, int K, int N, int T,
                      const float * bias, const float * resid, hipStream_t st);
int pm_launch_mmq_big_f32(int type, const void * W, const float * X, float * Y, int K, int N, int T, const float * bias, const float * resid,
                          int reuse_x, hipStream_t st);
