// pm355_layer_ops.h — host launchers of the layer operations: layer_ops.hip, the attention forms (attn_cached / attn_split / attn_flash /
// attn_flash_mfma / attn_prefill / attn_q8 .hip) and the RoPE configuration they share
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
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
void pm_launch_rope_kv_store(const float * q, const float * k, const float * v, float * q_out, float * k_out_f32,
                             void * kc, void * vc, const int32_t * pos0, const int32_t * seq, long seq_stride,
                             const float * freq_factors,
                             int n_tok, int H, int Hkv, int dh, int n_ctx, const pm_rope_cfg & c, hipStream_t st,
                             int round_q = 0);       // q_out rounded to F16 (what MUL_MAT(k, q) does to its src1): the form pm_launch_attn_cached reads
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
// dynamic LDS bytes of the per-head kernels (rope_fused, cached); beyond PM_ATTN_LDS_MAX the launchers refuse.
// ggml_graph_plan.h keeps a bound of its own (the plug-in links only the C ABI): it must stay at least as strict as this one.
constexpr size_t PM_ATTN_LDS_MAX = 150 * 1024;
inline size_t pm_attn_head_lds(int dh, int n_ctx, bool v_rowmajor, int cells) {
    return (size_t) (4 * dh + (v_rowmajor ? 2048 : 256) + (cells > 0 ? ((cells + 7) & ~7) : n_ctx) + 8) * 4;
}
int  pm_launch_attn_decode(const pm_attn_tok & a, hipStream_t st);       // cached cells, scores in LDS sized for n_ctx, q rounded to F16 by the kernel (layer_ops.hip)
int  pm_launch_attn_rope_fused(const pm_attn_tok & a, hipStream_t st);   // raw projections: RoPE + KV store + attention, one workgroup per head (layer_ops.hip)
// decode path with the RoPE + KV-store epilogue in the wq | wk | wv launch (mmvq_device.h QkvEpi): q = rotated, F16-rounded rows (attn_cached.hip)
int  pm_launch_attn_cached(const pm_attn_tok & a, hipStream_t st);
// long context, keys split over workgroups, three launches (attn_split.hip). rope == null: q = ROTATED queries and the caches are already
// updated; else q / k / v are the raw projections and rope + KV store happen inside the first kernel
size_t pm_attn_split_scratch_floats(int H, int dh, int n_ctx);
int  pm_launch_attn_split(const pm_attn_tok & a, hipStream_t st);
// long context in ONE launch (flash-decoding with an in-launch merge, attn_flash.hip); q / k / v raw projections
size_t pm_attn_flash_scratch_floats(int H, int Hkv, int dh, int n_ctx);
int  pm_launch_attn_flash(const pm_attn_tok & a, hipStream_t st);
// long context over cached cells on the matrix cores (attn_flash_mfma.hip); F16 or Q8_0 caches
int  pm_attn_flash_cached_ok(int H, int Hkv, int dh, int n_ctx);      // 0: served by the matrix-core long-context kernel
int  pm_launch_attn_flash_cached(const pm_attn_tok & a, hipStream_t st);
// where the long-context Q8_0 path parks the token's rotated (and, for a Q8_0 K cache, Q8_0-quantized) query rows inside the attention scratch
size_t pm_attn_flash_qrot_offset(int H, int Hkv, int dh, int n_ctx);
// causal multi-token attention on MFMA (attn_prefill.hip); -1: unsupported shape (head_dim 64/128, n_ctx % 32 == 0)
int  pm_launch_attn_prefill(const float * q, const void * kc, const void * vc, const int32_t * pos0, const int32_t * seq,
                            long seq_stride, float * out, int n_tok, int H, int Hkv, int dh, int n_ctx, float scale, hipStream_t st,
                            const float * mask = nullptr, long mask_stride = 0, int n_kv = 0,   // mask != null: ggml-graph mode (cells [0, n_kv) + additive mask row per token)
                            int v_rowmajor = 0, int mask_f16 = 0,                              // flash-attention graphs: row-major V cache, F16 mask rows
                            void * out_f16 = nullptr);                                         // result as F16 (activations of the wo GEMM) instead of `out`
// the per-token cos / sin table the QKV epilogue reads (tab[2 i], tab[2 i + 1] for rotation pair i; position = pos[seq ? *seq : 0])
void pm_launch_rope_table(const pm_rope_cfg & c, const int32_t * pos, const int32_t * seq, const float * freq_factors, float * tab, hipStream_t st,
                          int n_tok = 1);    // n_tok > 1: tables of the tokens pos .. pos + n_tok - 1, n_dims floats each
void pm_launch_set_i32x2(int32_t * p, int a, int b, hipStream_t st);
// quantized (Q8_0) KV cache, native 34-byte blocks (attn_q8.hip)
int  pm_launch_cpy_f32_q8_0(const pm355_tensor * src, void * dst, hipStream_t st);
int  pm_launch_flash_attn_ext_q8(const pm355_tensor * q, const pm355_tensor * k, const pm355_tensor * v, const pm355_tensor * mask,
                                 const pm355_tensor * dst, float scale, float softcap, hipStream_t st);
// Q8_0 caches (row-major V), ggml-graph mode, raw projections. prep: RoPE + quantizing KV store, a.out receives the operand rows of the K.q product
// (then pm_launch_attn_flash_cached runs over the cached cells); token: the same plus the attention, one workgroup per head
int  pm_launch_q8_token_prep(const pm_attn_tok & a, hipStream_t st);
int  pm_launch_attn_q8_token(const pm_attn_tok & a, hipStream_t st);
void pm_launch_argmax(const float * x, int n, int32_t * idx, float * val, hipStream_t st);
void pm_launch_add(const float * a, const float * b, float * y, long n, long nb, hipStream_t st);
void pm_launch_mul(const float * a, const float * b, float * y, long n, long nb, hipStream_t st);
void pm_launch_silu_mul(const float * g, const float * u, float * y, long n, hipStream_t st);
void pm_launch_scale(const float * a, float * y, float s, long n, hipStream_t st);
void pm_launch_set_i32(int32_t * p, int v, hipStream_t st);
void pm_launch_advance(int32_t * pos, int32_t * ctl, int by, int rotate, hipStream_t st);
void pm_launch_fill_random_blocks(int type, void * dst, int64_t K, int64_t nrows, uint64_t seed, float scale, hipStream_t st);
void pm_launch_fill_random_f32(float * dst, int64_t n, uint64_t seed, float mean, float amp, hipStream_t st);
