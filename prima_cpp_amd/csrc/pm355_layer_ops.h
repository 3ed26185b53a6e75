// pm355_layer_ops.h — host launchers of the layer operations: layer_ops.hip, the attention forms (attn_cached / attn_split / attn_flash /
// attn_flash_mfma / attn_prefill / attn_q8 .hip) and the RoPE configuration they share. Argument blocks: pm_attn_tok (one token), pm_attn_batch (many tokens),
// pm_rope_store (RoPE + KV store in front of them); pm_attn_flash_layout: the one layout of the long-context scratch
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include "../../include/prima_mi355.h"
#include "pm355_types.h"

struct pm_rope_cfg {
    int n_dims, mode /*0 = NORM, 2 = NEOX*/, n_ctx_orig;
    float freq_base, freq_scale, ext_factor, attn_factor, beta_fast, beta_slow;
    float theta_scale, corr0, corr1;     // filled by pm_rope_params()
};
void pm_rope_params(pm_rope_cfg & c);
pm_rope_cfg pm_rope_cfg_of(const pm355_rope_params & rp);      // the C ABI's parameters with the derived constants filled in

// type: one the embedding row lookup decodes (pm_embed_type_ok, pm355_types.h; pm355_get_rows and the engine's token embedding refuse the others)
void pm_launch_embed(int type, const void * table, int K, const int32_t * tokens, int n_tok, float * out, hipStream_t st);
// RoPE of n_tok tokens' raw q / k projections, their K rows / V columns stored in the F16 caches (transposed V); engine mode as below:
// token t sits at position pos[seq ? *seq : 0] + t = its cell
struct pm_rope_store {
    const float * q, * k, * v; float * q_out, * k_out_f32;     // raw projections; rotated queries (may be q) and, optionally, the rotated keys in f32
    void * kc, * vc; const int32_t * pos, * seq; long seq_stride; const float * freq_factors;
    int n_tok, H, Hkv, dh, n_ctx; const pm_rope_cfg * rope;
    bool round_q;                          // q_out rounded to F16 (what MUL_MAT(k, q) does to its src1): the form pm_launch_attn_cached reads
};
void pm_launch_rope_kv_store(const pm_rope_store & a, hipStream_t st);
// ---- single-token attention: every form takes the same argument block -----------------------------------------------------------------
// Engine mode: the token's position is pos[seq ? *seq : 0], its cache slab starts seq_stride elements per sequence further on, cell == position
// and cells [0, pos] are attended. ggml-graph mode: dyn = device int32[2] {cache cell the token is stored in, cells attended}, the RoPE position
// is pos[0], mask = additive KQ-mask row [cells attended] (f32, or F16 with mask_f16) or null.
// A launcher returns -1 for a shape it does not serve and for a MODE it does not serve (rope present or absent, dyn / mask, seq, a flag, cells,
// n_tok): it never drops one. Input buffers its form does not read (k, v, freq_factors, scratch) are not looked at, nor is mask_f16 without a mask.
struct pm_attn_tok {
    const float * q, * k, * v;             // raw projections (rope != null), or q = rotated queries of a form that finds the caches already written
    void * kc, * vc;
    const int32_t * pos, * seq; long seq_stride;
    const int32_t * dyn; const void * mask;
    const float * freq_factors; float * out, * scratch;
    int H, Hkv, dh, n_ctx; float scale;
    const pm_rope_cfg * rope;              // null: no rotation and no KV store in this launch
    bool v_rowmajor;                       // the V cache is [n_ctx][n_embd_v_gqa] (flash-attention graphs, with their rounding points) instead of transposed
    bool mask_f16, k_q8, v_q8;             // k_q8 / v_q8: that cache holds native 34-byte Q8_0 blocks
    int cells;                             // > 0: keys the LDS score buffer (per-head forms) / the grid (flash forms) is sized for; the caller guarantees cells attended <= cells
    int n_tok = 1;                         // decode and cached forms, engine mode: token t attends cells [0, pos + t], q / out rows t
};
// Every form has its predicate next to its launcher: what pm_X_ok(a) accepts pm_launch_X(a) launches, and the launcher refuses (-1) exactly what
// the predicate refuses. pm_attn_token_plan (attn_plan.hip) chooses among the forms with the same predicates.
// dynamic LDS bytes of the per-head kernels (rope_fused, cached); beyond PM_ATTN_LDS_MAX the launchers refuse
constexpr size_t PM_ATTN_LDS_MAX = 150 * 1024;
inline size_t pm_attn_head_lds(int dh, int n_ctx, bool v_rowmajor, int cells) {
    return (size_t) (4 * dh + (v_rowmajor ? 2048 : 256) + (cells > 0 ? ((cells + 7) & ~7) : n_ctx) + 8) * 4;
}
inline bool pm_attn_head_shape_ok(const pm_attn_tok & a) {          // head_dim list and score buffer of the two per-head kernels
    return (a.dh == 64 || a.dh == 128 || a.dh == 256) && a.n_ctx % 8 == 0 && pm_attn_head_lds(a.dh, a.n_ctx, a.v_rowmajor, a.cells) <= PM_ATTN_LDS_MAX;
}
int  pm_launch_attn_decode(const pm_attn_tok & a, hipStream_t st);       // cached cells, scores in LDS sized for n_ctx, q rounded to F16 by the kernel (layer_ops.hip)
bool pm_attn_rope_fused_ok(const pm_attn_tok & a);
int  pm_launch_attn_rope_fused(const pm_attn_tok & a, hipStream_t st);   // raw projections: RoPE + KV store + attention, one workgroup per head (layer_ops.hip)
// decode path with the RoPE + KV-store epilogue in the wq | wk | wv launch (mmvq_device.h QkvEpi): q = rotated, F16-rounded rows (attn_cached.hip)
bool pm_attn_cached_ok(const pm_attn_tok & a);
int  pm_launch_attn_cached(const pm_attn_tok & a, hipStream_t st);
// long context over raw projections or rotated rows, keys split over workgroups (attn_split.hip, attn_flash.hip): a workgroup serves the whole group
// of query heads of its KV head, at most PM_ATTN_GROUP_MAX of them (RMAX of both files); head_dim 64 / 128
constexpr int PM_ATTN_GROUP_MAX = 8;
inline bool pm_attn_split_heads_ok(int H, int Hkv, int dh) { return (dh == 64 || dh == 128) && Hkv >= 1 && H % Hkv == 0 && H / Hkv <= PM_ATTN_GROUP_MAX; }
// three launches (attn_split.hip). rope == null: q = ROTATED queries and the caches are already
// updated; else q / k / v are the raw projections and rope + KV store happen inside the first kernel
size_t pm_attn_split_scratch_floats(int H, int dh, int n_ctx);
bool pm_attn_split_ok(const pm_attn_tok & a);
int  pm_launch_attn_split(const pm_attn_tok & a, hipStream_t st);
// The scratch of the two one-launch long-context forms and of the Q8_0 path in front of the second, in floats.
// Both kernels may run on one scratch in one process: each has ticket words of its own
constexpr int PM_FLASH_CK = 128;           // keys per span of both kernels at their shortest: the partials are sized for ceil(n_ctx / CK) spans
struct pm_flash_scratch {
    int nspan;                             // rows of M / L / P: spans of PM_FLASH_CK keys over n_ctx (a launch that grows its spans uses fewer)
    size_t M, L;                           // [H][nspan] each: running max / sum of exp of every (head, span)
    size_t P;                              // [nspan][H][dh]: the spans' partial outputs
    size_t tickets;                        // attn_flash.hip: Hkv arrival counters straight behind P; its last workgroup leaves them 0 for its next launch
    size_t tickets_mfma;                   // attn_flash_mfma.hip: 32 words ([g], [16 + g], g < 16 KV heads) that count on from launch to launch, so never
                                           // the other kernel's Hkv words, which must read 0: 16 words behind those, up to tickets + Hkv + 48
    size_t qrot;                           // H * dh floats: the rotated (Q8_0 K cache: quantized) query rows pm_launch_q8_token_prep leaves for the cached
                                           // kernel, Hkv + 64 + 64 words behind the first tickets: clear of the 48 above with a cache line to spare
    size_t total;
};
inline pm_flash_scratch pm_attn_flash_layout(int H, int Hkv, int dh, int n_ctx) {
    pm_flash_scratch s;
    s.nspan = (n_ctx + PM_FLASH_CK - 1) / PM_FLASH_CK; s.M = 0; s.L = s.M + (size_t) H * s.nspan; s.P = s.L + (size_t) H * s.nspan;
    s.tickets = s.P + (size_t) s.nspan * H * dh; s.tickets_mfma = s.tickets + Hkv + 16; s.qrot = s.tickets + Hkv + 64 + 64; s.total = s.qrot + (size_t) H * dh;
    return s;
}
// floats of scratch that serve ANY long-context form (attn_split.hip included): what the engine or a C-ABI caller allocates and zeroes once (tickets start at 0)
inline size_t pm_attn_long_scratch_floats(int H, int Hkv, int dh, int n_ctx) {
    return std::max(pm_attn_split_scratch_floats(H, dh, n_ctx), pm_attn_flash_layout(H, Hkv, dh, n_ctx).total);
}
// long context in ONE launch (flash-decoding with an in-launch merge, attn_flash.hip); q / k / v raw projections
bool pm_attn_flash_ok(const pm_attn_tok & a);
int  pm_launch_attn_flash(const pm_attn_tok & a, hipStream_t st);
// long context over cached cells on the matrix cores (attn_flash_mfma.hip); F16 or Q8_0 caches. The shape rule reads the CU count: n_cus <= 0 = the device's
bool pm_attn_flash_cached_shape_ok(int H, int Hkv, int dh, int n_ctx, int n_cus = 0);
bool pm_attn_flash_cached_ok(const pm_attn_tok & a, int n_cus = 0);
int  pm_launch_attn_flash_cached(const pm_attn_tok & a, hipStream_t st);
// ---- multi-token attention over cached cells on MFMA (attn_prefill.hip) -----------------------------------------------------------------------
// q = rotated query rows [n_tok][H * dh], the caches already hold the tokens. Engine mode (pos): token t attends cells [0, pos[seq ? *seq : 0] + t], causal.
// ggml-graph mode (mask): cells [0, n_kv) plus the additive mask row of each token (mask_stride elements apart; f32, or F16 with mask_f16).
// The rule above holds: -1 for a shape it does not serve (head_dim 64 / 128, n_ctx % 32 == 0, n_tok >= 1; with a mask n_kv in 1 .. n_ctx, n_kv % 4 == 0,
// mask_stride % 4 == 0) and for a mode it does not serve: exactly one of out / out_f16, exactly one of pos / mask, seq only with pos, v_rowmajor and
// mask_f16 (the flash-attention graphs) only with a mask.
struct pm_attn_batch {
    const float * q; const void * kc, * vc; const int32_t * pos, * seq; long seq_stride; const void * mask; long mask_stride; int n_kv;
    float * out; void * out_f16;           // the result as f32, or as F16 (the activations of the wo GEMM)
    int n_tok, H, Hkv, dh, n_ctx; float scale; bool v_rowmajor, mask_f16;
};
int  pm_launch_attn_prefill(const pm_attn_batch & a, hipStream_t st);
// the per-token cos / sin table the QKV epilogue reads (tab[2 i], tab[2 i + 1] for rotation pair i; position = pos[seq ? *seq : 0])
constexpr int PM_ROPE_TABLE_DIMS_MAX = 256;          // n_dims the table (and the buffers its callers keep for it) holds
void pm_launch_rope_table(const pm_rope_cfg & c, const int32_t * pos, const int32_t * seq, const float * freq_factors, float * tab, hipStream_t st,
                          int n_tok = 1);    // n_tok > 1: tables of the tokens pos .. pos + n_tok - 1, n_dims floats each
void pm_launch_set_i32x2(int32_t * p, int a, int b, hipStream_t st);
// dynamic LDS bytes of the two FLASH_ATTN_EXT node kernels (ggml_ops.hip; Q8_0 K / V: attn_q8.hip): the padded query row, one query's scores, the slots' partial rows
inline size_t pm_flash_attn_ext_lds(int64_t head_dim, int64_t n_kv) {
    const size_t Dp = ((size_t) head_dim + 7) & ~(size_t) 7;
    return (Dp + (((size_t) n_kv + 3) & ~(size_t) 3) + 256 / (Dp / 8) * Dp) * 4;
}
// quantized (Q8_0) KV cache, native 34-byte blocks (attn_q8.hip)
int  pm_launch_cpy_f32_q8_0(const pm355_tensor * src, void * dst, hipStream_t st);
int  pm_launch_flash_attn_ext_q8(const pm355_tensor * q, const pm355_tensor * k, const pm355_tensor * v, const pm355_tensor * mask,
                                 const pm355_tensor * dst, float scale, float softcap, hipStream_t st);
// Q8_0 caches (row-major V), ggml-graph mode, raw projections. prep: RoPE + quantizing KV store, a.out receives the operand rows of the K.q product
// (then pm_launch_attn_flash_cached runs over the cached cells); token: the same plus the attention, one workgroup per head
bool pm_attn_q8_token_prep_ok(const pm_attn_tok & a);
int  pm_launch_q8_token_prep(const pm_attn_tok & a, hipStream_t st);
bool pm_attn_q8_token_ok(const pm_attn_tok & a);
int  pm_launch_attn_q8_token(const pm_attn_tok & a, hipStream_t st);
constexpr int PM_ATTN_Q8_TOKEN_CELLS_MAX = 32768;      // ggml-graph mode: the per-head Q8_0 kernel's score buffer is never sized for more cells than this
// ---- ggml-graph mode: which single-token form serves a layer, and the one switch that runs a form (attn_plan.hip) ------------------------------
// The plan follows no pointer and needs no device. A form it names is accepted by that form's predicate above, so pm_attn_token_run cannot be
// refused for the shape or mode the plan saw (it still refuses null pointers).
void pm_attn_token_plan(const pm355_attn_plan_in & in, pm355_attn_plan_out & out);
int  pm_attn_long_raw_form();                           // PM355_ATTN_FORM_FLASH, or _SPLIT3 with PM355_ATTN_FLASH=0 in the environment (read once)
// runs `form` (PM355_ATTN_FORM_*) on the C ABI's argument block; 0, or the refusal as a PM355_E_* code with its text in *why
int  pm_attn_token_run(int form, const pm355_attn_token_args & a, const pm355_rope_params * rp, hipStream_t st, const char ** why);
void pm_launch_argmax(const float * x, int n, int32_t * idx, float * val, hipStream_t st);
void pm_launch_add(const float * a, const float * b, float * y, long n, long nb, hipStream_t st);
void pm_launch_mul(const float * a, const float * b, float * y, long n, long nb, hipStream_t st);
void pm_launch_silu_mul(const float * g, const float * u, float * y, long n, hipStream_t st);
void pm_launch_scale(const float * a, float * y, float s, long n, hipStream_t st);
void pm_launch_set_i32(int32_t * p, int v, hipStream_t st);
void pm_launch_advance(int32_t * pos, int32_t * ctl, int by, int rotate, hipStream_t st);
void pm_launch_fill_random_blocks(int type, void * dst, int64_t K, int64_t nrows, uint64_t seed, float scale, hipStream_t st);
void pm_launch_fill_random_f32(float * dst, int64_t n, uint64_t seed, float mean, float amp, hipStream_t st);
