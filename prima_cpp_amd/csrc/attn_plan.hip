// attn_plan.hip — ggml-graph mode, one token: which attention form serves a layer (pm_attn_token_plan) and the one switch that runs a form
// (pm_attn_token_run). Host code only. Both build the form's pm_attn_tok with tok_of() and ask the predicate that sits next to the form's
// launcher, so what the plan names the switch launches.
#include "pm355_layer_ops.h"
#include <stdlib.h>

namespace {

const int F16_FLAGS = PM355_ATTN_V_ROWMAJOR | PM355_ATTN_MASK_F16, Q8_FLAGS = PM355_ATTN_K_Q8_0 | PM355_ATTN_V_Q8_0;

bool raw_form(int form) { return form != PM355_ATTN_FORM_CACHED && form != PM355_ATTN_FORM_CACHED_LONG; }

// the argument block of `form`: the raw-projection forms rotate and store (rope), the cached forms find q rotated and the caches written
pm_attn_tok tok_of(int form, const pm355_attn_token_args & a, const pm_rope_cfg * rope) {
    pm_attn_tok t = {};
    t.q = a.q; t.kc = a.k_cache; t.vc = a.v_cache; t.pos = a.d_pos; t.dyn = a.d_cell_nkv; t.mask = a.mask; t.out = a.out; t.scratch = a.scratch;
    t.H = a.n_head; t.Hkv = a.n_head_kv; t.dh = a.head_dim; t.n_ctx = a.n_ctx; t.scale = a.kq_scale;
    t.cells = form == PM355_ATTN_FORM_SPLIT3 ? 0 : a.max_keys;       // (the three-launch form has nothing max_keys would size)
    t.v_rowmajor = a.flags & PM355_ATTN_V_ROWMAJOR; t.mask_f16 = a.flags & PM355_ATTN_MASK_F16;
    t.k_q8 = a.flags & PM355_ATTN_K_Q8_0; t.v_q8 = a.flags & PM355_ATTN_V_Q8_0;
    if (raw_form(form)) { t.k = a.k; t.v = a.v; t.freq_factors = a.freq_factors; t.rope = rope; }
    return t;
}
// q8_long is two launches: RoPE + quantizing KV store that leaves the operand rows of K.q in the scratch, then the matrix-core kernel over the cached cells
void q8_long_parts(const pm_attn_tok & t, pm_attn_tok & prep, pm_attn_tok & cached) {
    prep = t; cached = t;
    prep.out = t.scratch ? t.scratch + pm_attn_flash_layout(t.H, t.Hkv, t.dh, t.n_ctx).qrot : nullptr;
    cached.q = prep.out; cached.k = cached.v = nullptr; cached.pos = nullptr; cached.freq_factors = nullptr; cached.rope = nullptr;
}
bool form_ok(int form, const pm_attn_tok & t, int n_cus) {
    switch (form) {
        case PM355_ATTN_FORM_ROPE_FUSED:  return pm_attn_rope_fused_ok(t);
        case PM355_ATTN_FORM_FLASH:       return pm_attn_flash_ok(t);
        case PM355_ATTN_FORM_SPLIT3:      return pm_attn_split_ok(t);
        case PM355_ATTN_FORM_Q8_TOKEN:    return pm_attn_q8_token_ok(t);
        case PM355_ATTN_FORM_Q8_LONG:     { pm_attn_tok p, c; q8_long_parts(t, p, c); return pm_attn_q8_token_prep_ok(p) && pm_attn_flash_cached_ok(c, n_cus); }
        case PM355_ATTN_FORM_CACHED:      return pm_attn_cached_ok(t);
        case PM355_ATTN_FORM_CACHED_LONG: return pm_attn_flash_cached_ok(t, n_cus);
        default:                          return false;
    }
}
// what a form's refusal reads like (the texts of the entries that used to own one form each)
const char * refusal_text(int form) {
    switch (form) {
        case PM355_ATTN_FORM_ROPE_FUSED:  return "attn_token: head_dim must be 64/128/256, n_ctx % 8 == 0 and max_keys fit LDS";
        case PM355_ATTN_FORM_FLASH:       return "attn_token(flash): head_dim 64/128, at most 8 query heads per KV head, n_ctx % 8 == 0, scratch required";
        case PM355_ATTN_FORM_SPLIT3:      return "attn_token(split): head_dim 64/128, at most 8 query heads per KV head, n_ctx % 8 == 0, scratch required";
        case PM355_ATTN_FORM_Q8_TOKEN:    return "attn_token(q8_0): head_dim 64/128 and max_keys must fit LDS";
        case PM355_ATTN_FORM_Q8_LONG:     return "attn_token(q8_0, long): head_dim 64/128, <= 16 query heads per KV head, <= 16 KV heads, n_ctx % 8 == 0";
        case PM355_ATTN_FORM_CACHED:      return "attn_cached: head_dim must be 64/128/256, n_ctx % 8 == 0 and max_keys fit LDS";
        case PM355_ATTN_FORM_CACHED_LONG: return "attn_cached_long: head_dim must be 64/128, <= 16 query heads per KV head, n_ctx % 8 == 0; Q8_0 caches need row-major V";
        default:                          return "attn_token_run: form";
    }
}

} // namespace

// the long-context form over raw F16 projections: one launch, or three with PM355_ATTN_FLASH=0 (read once)
int pm_attn_long_raw_form() {
    static const bool three_launch = [] { const char * e = getenv("PM355_ATTN_FLASH"); return e && e[0] == '0'; }();
    return three_launch ? PM355_ATTN_FORM_SPLIT3 : PM355_ATTN_FORM_FLASH;
}

void pm_attn_token_plan(const pm355_attn_plan_in & in, pm355_attn_plan_out & out) {
    out = {};                                                         // PM355_ATTN_FORM_NONE: the layer runs node by node
    if (in.n_kv < 1 || in.n_kv > in.n_ctx || in.split_min < 1) return;
    const bool q8 = in.flags & Q8_FLAGS;
    float * const dp = (float *) 16;                                  // stands for every buffer: never followed
    pm355_attn_token_args a = {};
    a.q = a.k = a.v = a.out = a.scratch = dp; a.k_cache = a.v_cache = dp; a.d_pos = a.d_cell_nkv = (const int32_t *) dp;
    a.n_head = in.n_head; a.n_head_kv = in.n_head_kv; a.head_dim = in.head_dim; a.n_ctx = in.n_ctx; a.flags = in.flags;
    const pm_rope_cfg rope = {};
    auto serves = [&](int form, int cells) { a.max_keys = cells; return form_ok(form, tok_of(form, a, &rope), in.n_cus); };
    // rotated query rows, caches written: F16 caches, and a rotation the cos / sin table holds
    const bool rot = in.rotated_q && !q8 && (in.rope_mode == 0 || in.rope_mode == 2) && in.rope_n_dims <= PM_ROPE_TABLE_DIMS_MAX;
    // long contexts (keys split over workgroups, from split_min cells attended on): the shapes of the split kernels; a quantized cache has the
    // matrix-core kernel only. The grid is sized for a power-of-two bucket of the cells attended, so that a plan (and its captured hipGraph)
    // survives the steps of n_kv inside a bucket
    int64_t bucket = 1024;
    while (bucket < in.n_kv) bucket *= 2;
    if (bucket > in.n_ctx) bucket = in.n_ctx;
    int long_form = !pm_attn_split_heads_ok(in.n_head, in.n_head_kv, in.head_dim) ? PM355_ATTN_FORM_NONE :
                    !q8 ? pm_attn_long_raw_form() : in.attn_mfma ? PM355_ATTN_FORM_Q8_LONG : PM355_ATTN_FORM_NONE;
    if (long_form && !serves(long_form, (int) bucket)) long_form = PM355_ATTN_FORM_NONE;
    if (long_form && in.n_kv >= in.split_min && in.scratch) {
        out.form = rot && in.attn_mfma && serves(PM355_ATTN_FORM_CACHED_LONG, (int) bucket) ? PM355_ATTN_FORM_CACHED_LONG : long_form;
        out.cells = (int32_t) bucket;
        out.scratch_floats = (int64_t) pm_attn_long_scratch_floats(in.n_head, in.n_head, in.head_dim, in.n_ctx);   // (n_head: what the C ABI's callers allocate)
    } else {
        // one workgroup per head: the score buffer lives in LDS, sized for split_min (+ one padding step of the cache) or, when no long form
        // serves this shape, for the whole cache
        const int cells = long_form ? in.split_min + 32 : q8 && in.n_ctx > PM_ATTN_Q8_TOKEN_CELLS_MAX ? PM_ATTN_Q8_TOKEN_CELLS_MAX : in.n_ctx;
        const int form = rot ? PM355_ATTN_FORM_CACHED : q8 ? PM355_ATTN_FORM_Q8_TOKEN : PM355_ATTN_FORM_ROPE_FUSED;
        if (in.n_kv > cells || !serves(form, cells)) return;
        out.form = form; out.cells = cells;
    }
    out.rotated_q = !raw_form(out.form);
}

int pm_attn_token_run(int form, const pm355_attn_token_args & a, const pm355_rope_params * rp, hipStream_t st, const char ** why) {
    auto refuse = [&](int code, const char * text) { *why = text; return code; };
    pm_rope_cfg c = {};
    if (raw_form(form)) {
        if (!rp || rp->n_dims % 2 || rp->n_dims > a.head_dim) return refuse(PM355_E_SHAPE, "attn_token: n_dims");
        if (!a.d_pos || !a.d_cell_nkv || !a.q || !a.k || !a.v || !a.k_cache || !a.v_cache || !a.out) return refuse(PM355_E_SHAPE, "attn_token: null pointer");
        if ((a.flags & Q8_FLAGS) && !(a.flags & PM355_ATTN_V_ROWMAJOR))
            return refuse(PM355_E_UNSUPPORTED, "attn_token: a quantized KV cache needs row-major V (flash-attention graphs)");
        if (form == PM355_ATTN_FORM_Q8_LONG && !a.scratch) return refuse(PM355_E_SHAPE, "attn_token(q8_0, long): scratch");
        c = pm_rope_cfg_of(*rp);
    } else {
        const bool lng = form == PM355_ATTN_FORM_CACHED_LONG;
        if (!a.q || !a.k_cache || !a.v_cache || !a.out || (lng && !a.scratch) || (!a.d_pos && !a.d_cell_nkv))
            return refuse(PM355_E_SHAPE, lng ? "attn_cached_long: null pointer" : "attn_cached: null pointer");
        if (lng && (a.flags & ~(F16_FLAGS | Q8_FLAGS))) return refuse(PM355_E_UNSUPPORTED, "attn_cached_long: unknown flag");
    }
    const pm_attn_tok t = tok_of(form, a, &c);
    int rc;
    switch (form) {
        case PM355_ATTN_FORM_ROPE_FUSED:  rc = pm_launch_attn_rope_fused(t, st); break;
        case PM355_ATTN_FORM_FLASH:       rc = pm_launch_attn_flash(t, st); break;         // scratch zeroed once after its allocation (ticket words)
        case PM355_ATTN_FORM_SPLIT3:      rc = pm_launch_attn_split(t, st); break;
        case PM355_ATTN_FORM_Q8_TOKEN:    rc = pm_launch_attn_q8_token(t, st); break;
        case PM355_ATTN_FORM_Q8_LONG:     { pm_attn_tok p, k; q8_long_parts(t, p, k); rc = pm_launch_q8_token_prep(p, st) || pm_launch_attn_flash_cached(k, st) ? -1 : 0; break; }
        case PM355_ATTN_FORM_CACHED:      rc = pm_launch_attn_cached(t, st); break;
        case PM355_ATTN_FORM_CACHED_LONG: rc = pm_launch_attn_flash_cached(t, st); break;
        default:                          rc = -1;
    }
    return rc ? refuse(PM355_E_UNSUPPORTED, refusal_text(form)) : 0;
}
