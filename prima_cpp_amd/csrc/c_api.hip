// c_api.hip — extern "C" surface of libprima_mi355.so (see include/prima_mi355.h).
#include "../../include/prima_mi355.h"
#include "pm355_device.h"
#include "pm355_kernels.h"
#include "pm355_engine.h"
#include "pm355_layer_ops.h"
#include <stdio.h>
#include <string.h>
#include <atomic>
#include <mutex>

static thread_local char g_err[256] = "";
static int fail(int code, const char * what, hipError_t e = hipSuccess) {
    snprintf(g_err, sizeof(g_err), "%s%s%s", what, e != hipSuccess ? ": " : "", e != hipSuccess ? hipGetErrorString(e) : "");
    return code;
}
#define HIP_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return fail(PM355_E_HIP, #expr, e_); } while (0)
static inline hipStream_t S(pm355_stream_t s) { return (hipStream_t) s; }

extern "C" {

const char * pm355_version(void) { return "prima_mi355 0.1 (gfx950)"; }
const char * pm355_last_error(void) { return g_err; }

int pm355_device_count(void) { int n = 0; return hipGetDeviceCount(&n) == hipSuccess ? n : 0; }
int pm355_set_device(int d) { HIP_TRY(hipSetDevice(d)); return 0; }
int pm355_device_info(int d, char * name, size_t name_len, size_t * free_b, size_t * total_b, int * cus) {
    hipDeviceProp_t p;
    HIP_TRY(hipGetDeviceProperties(&p, d));
    if (name && name_len) { strncpy(name, p.name, name_len - 1); name[name_len - 1] = 0; }
    if (cus) *cus = p.multiProcessorCount;
    if (free_b || total_b) {
        int cur = 0; hipGetDevice(&cur); hipSetDevice(d);
        size_t f = 0, t = 0; hipError_t e = hipMemGetInfo(&f, &t); hipSetDevice(cur);
        if (e != hipSuccess) return fail(PM355_E_HIP, "hipMemGetInfo", e);
        if (free_b) *free_b = f;
        if (total_b) *total_b = t;
    }
    return 0;
}
// Is `p` page-locked host memory? Asked for every small upload of a token (positions, mask, ...). Only POSITIVE verdicts are cached (per 4 KiB page,
// direct-mapped, flushed whenever this library allocates or frees pinned memory itself - pm355_host_malloc / pm355_host_free, the plug-in's host
// buffer type): a stale "pinned" costs one wait, but a cached "pageable" for a page somebody pins later (hipHostRegister, another library's pinned
// allocator) would let set_tensor return while the DMA still reads the source - pageable pages ask the runtime every time.
namespace { struct PinE { uintptr_t page; }; PinE g_pin[256] = {}; std::atomic<unsigned> g_pin_gen{1}; unsigned g_pin_seen = 0; std::mutex g_pin_mu; }
int pm355_host_is_pinned(const void * p) {
    const uintptr_t page = ((uintptr_t) p >> 12) + 1;                 // (+1: 0 marks an empty slot)
    {
        std::lock_guard<std::mutex> lk(g_pin_mu);
        const unsigned gen = g_pin_gen.load(std::memory_order_acquire);
        if (gen != g_pin_seen) { memset(g_pin, 0, sizeof(g_pin)); g_pin_seen = gen; }
        if (g_pin[page & 255].page == page) return 1;
    }
    const unsigned gen0 = g_pin_gen.load(std::memory_order_acquire);
    hipPointerAttribute_t a;
    int pinned = 0;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) (void) hipGetLastError();                   // unknown to the runtime: pageable
    else pinned = a.type == hipMemoryTypeHost ? 1 : 0;
    if (pinned) {
        std::lock_guard<std::mutex> lk(g_pin_mu);
        if (g_pin_gen.load(std::memory_order_acquire) == gen0 && g_pin_seen == gen0) g_pin[page & 255].page = page;   // (an allocation raced the query: do not cache)
    }
    return pinned;
}
int pm355_sync_null_stream(void) { HIP_TRY(hipStreamSynchronize(nullptr)); return 0; }
int pm355_sync(pm355_stream_t s) { HIP_TRY(s ? hipStreamSynchronize(S(s)) : hipDeviceSynchronize()); return 0; }

pm355_stream_t pm355_stream_create(void) { hipStream_t s = nullptr; return hipStreamCreateWithFlags(&s, hipStreamNonBlocking) == hipSuccess ? (pm355_stream_t) s : nullptr; }
void pm355_stream_destroy(pm355_stream_t s) { if (s) (void) hipStreamDestroy(S(s)); }
pm355_event_t pm355_event_create(void) { hipEvent_t e = nullptr; return hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess ? (pm355_event_t) e : nullptr; }
void pm355_event_destroy(pm355_event_t e) { if (e) (void) hipEventDestroy((hipEvent_t) e); }
int pm355_event_record(pm355_event_t e, pm355_stream_t s) { HIP_TRY(hipEventRecord((hipEvent_t) e, S(s))); return 0; }
int pm355_event_wait(pm355_stream_t s, pm355_event_t e) { HIP_TRY(hipStreamWaitEvent(S(s), (hipEvent_t) e, 0)); return 0; }
int pm355_event_sync(pm355_event_t e) { HIP_TRY(hipEventSynchronize((hipEvent_t) e)); return 0; }

void * pm355_malloc(size_t n) { void * p = nullptr; return hipMalloc(&p, n) == hipSuccess ? p : nullptr; }
void   pm355_free(void * p) { if (p) (void) hipFree(p); }
// (the generation moves AFTER the runtime has changed the status of the pages: a query that overlaps the call re-asks the runtime next time)
void * pm355_host_malloc(size_t n) { void * p = nullptr; const bool ok = hipHostMalloc(&p, n, hipHostMallocDefault) == hipSuccess; g_pin_gen.fetch_add(1, std::memory_order_release); return ok ? p : nullptr; }
void   pm355_host_free(void * p) { if (p) (void) hipHostFree(p); g_pin_gen.fetch_add(1, std::memory_order_release); }
int pm355_memcpy_h2d(void * d, const void * s, size_t n, pm355_stream_t st) { HIP_TRY(hipMemcpyAsync(d, s, n, hipMemcpyHostToDevice, S(st))); return 0; }
int pm355_memcpy_d2h(void * d, const void * s, size_t n, pm355_stream_t st) { HIP_TRY(hipMemcpyAsync(d, s, n, hipMemcpyDeviceToHost, S(st))); return 0; }
int pm355_memcpy_d2d(void * d, const void * s, size_t n, pm355_stream_t st) { HIP_TRY(hipMemcpyAsync(d, s, n, hipMemcpyDeviceToDevice, S(st))); return 0; }
int pm355_memset(void * d, int v, size_t n, pm355_stream_t st) { HIP_TRY(hipMemsetAsync(d, v, n, S(st))); return 0; }

size_t pm355_row_size(int type, int64_t K) { return pm_weight_row_bytes(type, K); }
size_t pm355_row_stride(int type, int64_t K) { return pm_weight_row_stride(type, K); }
size_t pm355_q8_K_row_size(int64_t K) { return pm_q8k_row_bytes((int) K); }
size_t pm355_q8_0_row_size(int64_t K) { return pm_q80_row_bytes((int) K); }

int pm355_repack_rows(int type, const void * src, void * dst, int64_t K, int64_t nrows, int to_dev, pm355_stream_t st) {
    if (pm_weight_row_bytes(type, K) == 0) return fail(PM355_E_UNSUPPORTED, "repack: type");
    pm_launch_repack(type, src, dst, K, nrows, to_dev, S(st));
    HIP_TRY(hipGetLastError());
    return 0;
}

int pm355_quantize_q8_K(const float * x, void * yq, int64_t K, int64_t rows, pm355_stream_t st) {
    if (K <= 0 || K % 256) return fail(PM355_E_SHAPE, "quantize_q8_K: K % 256");
    pm_launch_quantize_q8k(x, yq, (int) K, (int) rows, S(st));
    HIP_TRY(hipGetLastError());
    return 0;
}
int pm355_quantize_q8_0(const float * x, void * yq, int64_t K, int64_t rows, pm355_stream_t st) {
    if (K <= 0 || K % 32) return fail(PM355_E_SHAPE, "quantize_q8_0: K % 32");
    pm_launch_quantize_q80(x, yq, (int) K, (int) rows, S(st));
    HIP_TRY(hipGetLastError());
    return 0;
}

// row-SoA activation -> reference block layout (test hook; tiny)
__global__ void act_to_blocks_kernel(int act_type, const uint8_t * yq, uint8_t * out, int K, int rows, size_t in_row) {
    const long i = (long) blockIdx.x * blockDim.x + threadIdx.x;
    if (act_type == PM_Q8_K) {
        const int nblk = K / 256;
        if (i >= (long) rows * nblk) return;
        const int row = (int) (i / nblk), b = (int) (i % nblk);
        const uint8_t * r = yq + (size_t) row * in_row;
        uint8_t * o = out + ((size_t) row * nblk + b) * PM_BS_Q8_K;
        *(float *) o = ((const float *) (r + K))[b];
        for (int j = 0; j < 256; ++j) o[4 + j] = r[b * 256 + j];
        for (int j = 0; j < 16; ++j) ((int16_t *) (o + 260))[j] = ((const int16_t *) (r + K + nblk * 4))[b * 16 + j];
    } else {
        const int nblk = K / 32;
        if (i >= (long) rows * nblk) return;
        const int row = (int) (i / nblk), b = (int) (i % nblk);
        const uint8_t * r = yq + (size_t) row * in_row;
        uint8_t * o = out + ((size_t) row * nblk + b) * PM_BS_Q8_0;
        *(uint16_t *) o = ((const uint16_t *) (r + K))[b];
        for (int j = 0; j < 32; ++j) o[2 + j] = r[b * 32 + j];
    }
}
int pm355_act_to_ggml_blocks(int act_type, const void * yq, void * out, int64_t K, int64_t rows, pm355_stream_t st) {
    if (act_type != PM_Q8_K && act_type != PM_Q8_0) return fail(PM355_E_UNSUPPORTED, "act_to_ggml_blocks: type");
    const long n = rows * (act_type == PM_Q8_K ? K / 256 : K / 32);
    const size_t in_row = act_type == PM_Q8_K ? pm_q8k_row_bytes((int) K) : pm_q80_row_bytes((int) K);
    hipLaunchKernelGGL(act_to_blocks_kernel, dim3((unsigned) ((n + 63) / 64)), dim3(64), 0, S(st),
                       act_type, (const uint8_t *) yq, (uint8_t *) out, (int) K, (int) rows, in_row);
    HIP_TRY(hipGetLastError());
    return 0;
}

int pm355_rms_norm(const float * x, const float * w, float * y, void * yq, int64_t K, int64_t rows, float eps, pm355_stream_t st) {
    if (K <= 0 || K % 256) return fail(PM355_E_SHAPE, "rms_norm: K % 256");
    pm_launch_rmsnorm_q8k(x, w, y, yq, (int) K, (int) rows, eps, S(st));
    HIP_TRY(hipGetLastError());
    return 0;
}

// The mat-vec launchers' return codes (pm355_kernels.h) as the C ABI's, for every mat-vec entry. -5, -6 and -7 have a text with the entry that can ask for what they
// refuse and are a failed launch elsewhere (as is the job count, -9: every entry checks or fixes it first); the epilogue check answers -5 without a text
enum { MV_ANY, MV_SS, MV_QKV, MV_QKV_CHECK };
static const struct { int rc, entry, code; const char * text; } GEMV_RC[] = {
    {-1, MV_ANY, PM355_E_UNSUPPORTED, "mul_mat_vec_q: weight type"},
    {-2, MV_ANY, PM355_E_SHAPE, "mul_mat_vec_q: K not a multiple of the block size"},
    {-3, MV_ANY, PM355_E_ALIGN, "mul_mat_vec_q: K not a multiple of 32 for Q8_0"},
    {-4, MV_ANY, PM355_E_RANGE, "mul_mat_vec_q: K too large"},
    {-5, MV_QKV_CHECK, PM355_E_UNSUPPORTED, nullptr},
    {-5, MV_QKV, PM355_E_UNSUPPORTED, "mul_mat_vec_qkv: every workgroup's row slices must hold whole rotation pairs (N % (2 * CUs) == 0), N_k == N_v == n_head_kv * head_dim"},
    {-6, MV_SS, PM355_E_UNSUPPORTED, "mul_mat_vec_fused_ss: sumsq_out needs ONE plain job; sumsq_in needs norm_w and 1..256 partials"},
    {-7, MV_QKV, PM355_E_UNSUPPORTED, "mul_mat_vec_qkv_attn: the workgroups of a KV-head group must be a power-of-two run of the grid (CUs % n_head_kv == 0), head_dim 64 / 128, position-pointer mode, transposed V cache"},
    {-8, MV_ANY, PM355_E_UNSUPPORTED, "mul_mat_vec_q: sum-of-squares partials / attention tail are built into libprima_mi355_exp.so only (PM_EXPERIMENTS)"},
};
static int gemv_rc(int rc, int entry = MV_ANY) {
    if (rc == 0) return 0;
    for (const auto & r : GEMV_RC) if (r.rc == rc && (r.entry == MV_ANY || r.entry == entry)) return r.text ? fail(r.code, r.text) : r.code;
    return fail(PM355_E_HIP, "mul_mat_vec_q: launch", hipGetLastError());
}
// a job list of the C ABI as the launcher's; qkv: wq | wk | wv for the epilogue entries - three plain jobs whatever the caller left in W2 / resid
static pm_gemv_fused fused_of(const pm355_matvec_job * jobs, int njobs, int64_t K, const float * x, const float * norm_w, float eps, bool qkv = false) {
    pm_gemv_fused f = {};
    f.K = (int) K; f.njobs = qkv ? 3 : njobs; f.xf = x; f.norm_w = norm_w; f.eps = eps;
    for (int j = 0; j < f.njobs; ++j) f.job[j] = {jobs[j].type, (int) jobs[j].N, jobs[j].W, qkv ? nullptr : jobs[j].W2, jobs[j].y, jobs[j].bias, qkv ? nullptr : jobs[j].resid};
    return f;
}
static pm_qkv_epi qkv_epi_of(const pm355_qkv_store & s) {
    pm_qkv_epi e = {};
    e.tab = s.rope_table; e.pos = s.d_pos; e.dyn = s.d_cell_nkv; e.kc = s.k_cache; e.vc = s.v_cache;
    e.Hkv = s.n_head_kv; e.dh = s.head_dim; e.n_ctx = s.n_ctx; e.n_rot = s.n_rot; e.v_rowmajor = s.v_rowmajor; e.neox = s.rope_neox;
    return e;
}
// pm_launch_gemm's return codes (pm355_kernels.h); what = the entry's name
static int gemm_rc(int rc, const char * what) {
    if (rc == 0) return 0;
    char msg[160];
    snprintf(msg, sizeof(msg), "%s: %s", what, rc == -1 ? "weight type" : rc == -2 ? "K % 256 (K % 64 for Q8_0) and N % 4 required"
                                             : rc == -5 ? "type / shape not served by the prompt kernel" : "scratch allocation");
    return fail(rc == -1 || rc == -5 ? PM355_E_UNSUPPORTED : rc == -2 ? PM355_E_SHAPE : PM355_E_HIP, msg);
}
int pm355_mul_mat_vec_q(int type, const void * W, const void * W2, int64_t K, int64_t N, const void * xq, int ncols,
                        float * y, int64_t y_stride, const float * bias, const float * resid, pm355_stream_t st) {
    if (ncols < 1 || ncols > 8) return fail(PM355_E_RANGE, "mul_mat_vec_q: ncols must be 1..8");
    pm_gemv_args a = {};
    a.type = type; a.K = (int) K; a.N = (int) N; a.W = W; a.W2 = W2; a.xq = xq; a.ncols = ncols;
    a.y = y; a.y_stride = (size_t) y_stride; a.bias = bias; a.resid = resid; a.dbg_int = nullptr;
    return gemv_rc(pm_launch_gemv(a, S(st)));
}
int pm355_mul_mat_vec_fused(const pm355_matvec_job * jobs, int njobs, int64_t K, const float * x_f32, const float * norm_w,
                            float eps, pm355_stream_t st) {
    if (njobs < 1 || njobs > 3 || !jobs || !x_f32) return fail(PM355_E_RANGE, "mul_mat_vec_fused: 1..3 jobs and an f32 activation");
    return pm355_mul_mat_vec_fused_ss(jobs, njobs, K, x_f32, norm_w, eps, nullptr, nullptr, 0, st);
}
int pm355_mul_mat_vec_fused_ss(const pm355_matvec_job * jobs, int njobs, int64_t K, const float * x_f32, const float * norm_w, float eps,
                               double * sumsq_out, const double * sumsq_in, int n_sumsq_in, pm355_stream_t st) {
    if (njobs < 1 || njobs > 3 || !jobs || !x_f32) return fail(PM355_E_RANGE, "mul_mat_vec_fused_ss: 1..3 jobs and an f32 activation");
    pm_gemv_fused f = fused_of(jobs, njobs, K, x_f32, norm_w, eps);
    f.ss_out = sumsq_out; f.ss_in = sumsq_in; f.n_ss = n_sumsq_in;
    (void) hipGetLastError();
    const int rc = gemv_rc(pm_launch_gemv_fused(f, S(st)), MV_SS);
    if (rc) return rc;
    HIP_TRY(hipGetLastError());
    return 0;
}
namespace {
struct ScatterP { pm355_scatter_seg seg[16]; };
__global__ __launch_bounds__(256) void scatter_bytes_kernel(const uint8_t * __restrict__ src, ScatterP p) {
    const pm355_scatter_seg sg = p.seg[blockIdx.x];
    const uint8_t * s_ = src + sg.src_off;
    uint8_t * d_ = (uint8_t *) sg.dst;
    if ((((uintptr_t) d_ | (uintptr_t) s_ | sg.bytes) & 3) == 0) {
        for (uint32_t i = threadIdx.x; i < sg.bytes / 4; i += 256) ((uint32_t *) d_)[i] = ((const uint32_t *) s_)[i];
    } else {
        for (uint32_t i = threadIdx.x; i < sg.bytes; i += 256) d_[i] = s_[i];
    }
}
} // namespace
int pm355_scatter_bytes(const void * src_dev, const pm355_scatter_seg * segs, int n, pm355_stream_t st) {
    if (!src_dev || !segs || n < 1 || n > 16) return fail(PM355_E_RANGE, "scatter_bytes: 1..16 segments");
    ScatterP p = {};
    for (int i = 0; i < n; ++i) { if (!segs[i].dst) return fail(PM355_E_SHAPE, "scatter_bytes: null destination"); p.seg[i] = segs[i]; }
    (void) hipGetLastError();
    hipLaunchKernelGGL(scatter_bytes_kernel, dim3(n), dim3(256), 0, S(st), (const uint8_t *) src_dev, p);
    HIP_TRY(hipGetLastError());
    return 0;
}
int pm355_q6k_tail_grouped(void) { return PM_Q6K_SCD ? 1 : 0; }
int pm355_experiments_built(void) { return PM_EXPERIMENTS ? 1 : 0; }
int pm355_mul_mat_vec_fused_grid(const pm355_matvec_job * jobs, int njobs, int64_t K) {
    if (njobs < 1 || njobs > 3 || !jobs) return fail(PM355_E_RANGE, "mul_mat_vec_fused_grid: 1..3 jobs");
    pm_gemv_plan pl; const int rc = pm_gemv_fused_plan(fused_of(jobs, njobs, K, (const float *) 16, nullptr, 0.0f), 0, pl);
    return rc ? gemv_rc(rc) : pl.grid;
}
int pm355_mul_mat_vec_fused_check(const pm355_matvec_job * jobs, int njobs, int64_t K) {
    if (njobs < 1 || njobs > 3 || !jobs) return fail(PM355_E_RANGE, "mul_mat_vec_fused: 1..3 jobs");
    pm_gemv_plan pl; return gemv_rc(pm_gemv_fused_plan(fused_of(jobs, njobs, K, (const float *) 16, nullptr, 0.0f), 0, pl));
}
int pm355_mul_mat_q_mfma(int type, const void * W, int64_t K, int64_t N, const float * x, int64_t n_tokens, float * y,
                         const float * bias, const float * resid, pm355_stream_t st) {
    (void) hipGetLastError();
    const pm_gemm_job jb = {type, (int) N, W, y, nullptr, bias, resid, nullptr, 0};
    const int rc = gemm_rc(pm_launch_gemm(&jb, 1, {x, nullptr}, (int) K, (int) n_tokens, 0, S(st)), "mul_mat_q_mfma");
    if (rc) return rc;
    HIP_TRY(hipGetLastError());
    return 0;
}
int pm355_mul_mat_q_mfma_multi(const pm355_gemm_job * jobs, int njobs, int64_t K, const float * x, int64_t n_tokens, pm355_stream_t st) {
    (void) hipGetLastError();
    if (!jobs || njobs < 1 || njobs > 4 || !x) return fail(PM355_E_RANGE, "mul_mat_q_mfma_multi: 1..4 jobs");
    pm_gemm_job jb[4];
    for (int j = 0; j < njobs; ++j) jb[j] = {jobs[j].type, (int) jobs[j].N, jobs[j].W, jobs[j].y, nullptr, jobs[j].bias, jobs[j].resid, nullptr, 0};
    const int rc = gemm_rc(pm_launch_gemm(jb, njobs, {x, nullptr}, (int) K, (int) n_tokens, 0, S(st)), "mul_mat_q_mfma_multi");
    if (rc) return rc;
    HIP_TRY(hipGetLastError());
    return 0;
}
int pm355_mul_mat_q_mfma_pair(int type, const void * W_gate, const void * W_up, int64_t K, int64_t N, const float * x, int64_t n_tokens, float * y, pm355_stream_t st) {
    (void) hipGetLastError();
    if (!W_gate || !W_up || !x || !y) return fail(PM355_E_SHAPE, "mul_mat_q_mfma_pair: null pointer");
    // (no f32 gate buffer: one launch of pair tiles, or refused)
    const pm_gemm_job jb[2] = {{type, (int) N, W_gate, nullptr, nullptr, nullptr, nullptr, nullptr, 0}, {type, (int) N, W_up, y, nullptr, nullptr, nullptr, nullptr, 0}};
    const int rc = gemm_rc(pm_launch_gemm(jb, 2, {x, nullptr}, (int) K, (int) n_tokens, 1, S(st)), "mul_mat_q_mfma_pair");
    if (rc) return rc;
    HIP_TRY(hipGetLastError());
    return 0;
}
int pm355_mul_mat_q_i8(int type, const void * W, int64_t K, int64_t N, const float * x, int64_t n_tokens, float * y,
                       const float * bias, const float * resid, pm355_stream_t st) {
    if (!W || !x || !y) return fail(PM355_E_SHAPE, "mul_mat_q_i8: null pointer");
    const int rc = pm_launch_mmq_big_f32(type, W, x, y, (int) K, (int) N, (int) n_tokens, bias, resid, 0, S(st));
    if (rc == -1) return fail(PM355_E_UNSUPPORTED, "mul_mat_q_i8: weight type (Q4_K / Q6_K)");
    if (rc == -2) return fail(PM355_E_SHAPE, "mul_mat_q_i8: K % 1024 == 0 required");
    if (rc) return fail(PM355_E_HIP, "mul_mat_q_i8: scratch allocation");
    HIP_TRY(hipGetLastError());
    return 0;
}
int pm355_mul_mat_q_i8_check(int type, int64_t K, int64_t N, int64_t n_tokens) { return pm_mmq_big_check(type, (int) K, (int) N, (int) n_tokens) ? PM355_E_UNSUPPORTED : 0; }
// pm_launch_mmq_i8's return codes (pm355_kernels.h); what = the entry's name, unserved = what the entry says to a list no form serves (-5)
static int mmq_rc(int rc, const char * what, const char * unserved) {
    if (rc == 0) return 0;
    char msg[200];
    snprintf(msg, sizeof(msg), "%s: %s", what, rc == -1 ? "weight type (Q4_K / Q5_K / Q6_K / Q8_0)"
                                             : rc == -2 ? "1 <= n_tokens <= 64, K % 256 == 0 (Q8_0: K % 32 == 0), K >= 512 required"
                                             : rc == -4 ? "K too large for the LDS tiles" : rc == -5 ? unserved : "scratch allocation");
    return fail(rc == -1 || rc == -5 ? PM355_E_UNSUPPORTED : rc == -2 ? PM355_E_SHAPE : rc == -4 ? PM355_E_RANGE : PM355_E_HIP, msg);
}
// a job list of the C ABI's parallel arrays (types: one per job, or null and `type` for all)
static void mmq_jobs(pm_mmq_job * jb, int njobs, const int * types, int type, const void * const * W, const int64_t * N, float * const * y, const float * const * bias) {
    for (int j = 0; j < njobs; ++j) jb[j] = {types ? types[j] : type, (int) N[j], W[j], y[j], bias ? bias[j] : nullptr, nullptr};
}
int pm355_mul_mat_q_small(int type, const void * W, int64_t K, int64_t N, const void * xq, const float * x, int64_t n_tokens, float * y,
                          const float * bias, const float * resid, pm355_stream_t st) {
    (void) hipGetLastError();
    if (!xq && !x) return fail(PM355_E_RANGE, "mul_mat_q_small: neither xq nor x given");
    const pm_mmq_job jb = {type, (int) N, W, y, bias, resid};
    const int rc = mmq_rc(pm_launch_mmq_i8(&jb, 1, {xq, x, 0}, (int) K, (int) n_tokens, nullptr, S(st)), "mul_mat_q_small", "");
    if (rc) return rc;
    HIP_TRY(hipGetLastError());
    return 0;
}
int pm355_mul_mat_q_small_multi(int type, int njobs, const void * const * W, const int64_t * N, float * const * y, const float * const * bias,
                                const void * xq, int64_t K, int64_t n_tokens, pm355_stream_t st) {
    (void) hipGetLastError();
    if (njobs < 2 || njobs > 3 || !W || !N || !y || !xq) return fail(PM355_E_RANGE, "mul_mat_q_small_multi: 2..3 jobs, pre-quantized activations");
    pm_mmq_job jb[3];
    mmq_jobs(jb, njobs, nullptr, type, W, N, y, bias);
    const int rc = mmq_rc(pm_launch_mmq_i8(jb, njobs, {xq, nullptr, 0}, (int) K, (int) n_tokens, nullptr, S(st)), "mul_mat_q_small_multi",
                          "Q4_K / Q6_K, n_tokens <= 64, K % 256 == 0 required");
    if (rc) return rc;
    HIP_TRY(hipGetLastError());
    return 0;
}
int pm355_mul_mat_q_small_mixed(const int * types, int njobs, const void * const * W, const int64_t * N, float * const * y, const float * const * bias,
                                const void * xq, int64_t K, int64_t n_tokens, pm355_stream_t st) {
    (void) hipGetLastError();
    if (njobs < 2 || njobs > 3 || !types || !W || !N || !y || !xq) return fail(PM355_E_RANGE, "mul_mat_q_small_mixed: 2..3 jobs, pre-quantized activations");
    for (int j = 1; j < njobs - 1; ++j) if (types[j] != types[0]) return fail(PM355_E_UNSUPPORTED, "mul_mat_q_small_mixed: only the LAST job may be of another type");
    pm_mmq_job jb[3];
    mmq_jobs(jb, njobs, types, 0, W, N, y, bias);
    // (a last job of the first job's type is pm355_mul_mat_q_small_multi's list: this entry keeps refusing it)
    const int lrc = types[njobs - 1] == types[0] ? -5 : pm_launch_mmq_i8(jb, njobs, {xq, nullptr, 0}, (int) K, (int) n_tokens, nullptr, S(st));
    const int rc = mmq_rc(lrc, "mul_mat_q_small_mixed", "Q4_K jobs + one Q6_K (n_tokens <= 32) / Q5_K (<= 16) job, K % 256 == 0 required");
    if (rc) return rc;
    HIP_TRY(hipGetLastError());
    return 0;
}
int pm355_mul_mat_q_small_plan(const int * types, const int64_t * N, int njobs, int64_t K, int64_t n_tokens, int with_epilogue, int n_cus, int32_t * out, int max_passes) {
    if (!types || !N || njobs < 1 || njobs > 4 || n_cus < 1 || !out || max_passes < 1) return fail(PM355_E_RANGE, "mul_mat_q_small_plan: 1..4 jobs, n_cus >= 1, out required");
    pm_mmq_job jb[4];
    for (int j = 0; j < njobs; ++j) jb[j] = {types[j], (int) N[j], nullptr, nullptr, nullptr, nullptr};
    pm_mmq_plan_t pl;
    if (pm_mmq_i8_plan(jb, njobs, (int) K, (int) n_tokens, with_epilogue, n_cus, &pl)) return fail(PM355_E_UNSUPPORTED, "mul_mat_q_small_plan: no form of the small-batch mat-mul serves this list");
    for (int i = 0; i < pl.npass && i < max_passes; ++i) {
        const pm_mmq_pass & p = pl.pass[i];
        const int32_t v[8] = {p.form, p.t0, p.tn, p.nv, p.grid[0], p.rgb_log2[0], p.grid[1], p.rgb_log2[1]};
        memcpy(out + 8 * i, v, sizeof(v));
    }
    return pl.npass;
}
int pm355_gemm_plan(int64_t n_row_tiles, int64_t K, int64_t n_tokens, int n_cus, int allow_tail_split, int32_t * out5) {
    if (n_row_tiles < 1 || K < 256 || n_tokens < 1 || n_cus < 8 || !out5) return fail(PM355_E_RANGE, "gemm_plan: n_row_tiles >= 1, K >= 256, n_tokens >= 1, n_cus >= 8");
    pm_gemm_pf_plan_t pl;
    pm_gemm_pf_plan((int) n_row_tiles, (int) K, (int) n_tokens, n_cus, 0, 0, allow_tail_split, &pl);
    out5[0] = pl.nt * 32; out5[1] = pl.nt_t; out5[2] = pl.splitk; out5[3] = pl.full; out5[4] = pl.grid;
    return 0;
}
int pm355_mul_mat_q_small_check(int type, int64_t K, int64_t N, int64_t n_tokens) {
    return pm_mmq_i8_check(type, (int) K, (int) N, (int) n_tokens) == 0 ? 0 : PM355_E_UNSUPPORTED;
}
int pm355_mul_mat_vec_q_dbg(int type, const void * W, int64_t K, int64_t N, const void * xq, float * y,
                            int32_t * ip, int64_t * upr, pm355_stream_t st) {
    if (upr) *upr = pm_gemv_units_per_row(type, K);
    if (!ip && !y) return 0;                          // query of the unit count only
    pm_gemv_args a = {};
    a.type = type; a.K = (int) K; a.N = (int) N; a.W = W; a.xq = xq; a.ncols = 1; a.y = y; a.y_stride = (size_t) N; a.dbg_int = ip;
    return gemv_rc(pm_launch_gemv(a, S(st)));
}

int pm355_get_rows(int type, const void * table, int64_t K, const int32_t * d_tokens, int n_tokens, float * out, pm355_stream_t st) {
    if (!pm_weight_row_bytes(type, K) || !pm_embed_type_ok(type)) return fail(PM355_E_UNSUPPORTED, "get_rows: type (Q5_0 embedding rows are not served)");
    pm_launch_embed(type, table, (int) K, d_tokens, n_tokens, out, S(st));
    HIP_TRY(hipGetLastError());
    return 0;
}
int pm355_rope_kv_store(const float * q, const float * k, const float * v, float * q_out, float * k_out_f32,
                        void * kc, void * vc, const int32_t * d_pos0, const float * ff, int n_tokens, int H, int Hkv, int dh,
                        int n_ctx, const pm355_rope_params * rp, pm355_stream_t st) {
    if (!rp || rp->n_dims % 2 || rp->n_dims > dh || dh % 2) return fail(PM355_E_SHAPE, "rope: n_dims");
    const pm_rope_cfg c = pm_rope_cfg_of(*rp);
    pm_rope_store r = {};
    r.q = q; r.k = k; r.v = v; r.q_out = q_out; r.k_out_f32 = k_out_f32; r.kc = kc; r.vc = vc; r.pos = d_pos0; r.freq_factors = ff;
    r.n_tok = n_tokens; r.H = H; r.Hkv = Hkv; r.dh = dh; r.n_ctx = n_ctx; r.rope = &c;
    pm_launch_rope_kv_store(r, S(st));
    HIP_TRY(hipGetLastError());
    return 0;
}
int pm355_attn_decode(const float * q, const void * kc, const void * vc, const int32_t * d_pos0, float * out, int n_tokens,
                      int H, int Hkv, int dh, int n_ctx, float kq_scale, pm355_stream_t st) {
    pm_attn_tok t = {};
    t.q = q; t.kc = (void *) kc; t.vc = (void *) vc; t.pos = d_pos0; t.out = out; t.n_tok = n_tokens; t.H = H; t.Hkv = Hkv; t.dh = dh; t.n_ctx = n_ctx; t.scale = kq_scale;
    if (pm_launch_attn_decode(t, S(st)))
        return fail(PM355_E_RANGE, "attn_decode: n_ctx/head_dim unsupported (LDS budget 150 KB, multiples of 8)");
    HIP_TRY(hipGetLastError());
    return 0;
}
size_t pm355_attn_split_scratch_floats(int H, int dh, int n_ctx) { return pm_attn_long_scratch_floats(H, H, dh, n_ctx); }     // (every long-context form; no n_head_kv here: n_head is the upper bound)
int pm355_attn_long_scratch_layout(int H, int Hkv, int dh, int n_ctx, int64_t * out, int n_out) {
    if (!out || n_out < 8 || H < 1 || Hkv < 1 || dh < 1 || n_ctx < 1) return fail(PM355_E_SHAPE, "attn_long_scratch_layout: arguments");
    const pm_flash_scratch s = pm_attn_flash_layout(H, Hkv, dh, n_ctx);
    const int64_t v[8] = {s.nspan, (int64_t) s.M, (int64_t) s.L, (int64_t) s.P, (int64_t) s.tickets, (int64_t) s.tickets_mfma, (int64_t) s.qrot, (int64_t) s.total};
    memcpy(out, v, sizeof v); return 0;
}
int pm355_attn_decode_split(const float * q_rot, const void * kc, const void * vc, const int32_t * d_pos0, float * out, float * scratch,
                            int H, int Hkv, int dh, int n_ctx, float kq_scale, pm355_stream_t st) {
    pm_attn_tok t = {};
    t.q = q_rot; t.kc = (void *) kc; t.vc = (void *) vc; t.pos = d_pos0; t.out = out; t.scratch = scratch;
    t.H = H; t.Hkv = Hkv; t.dh = dh; t.n_ctx = n_ctx; t.scale = kq_scale;
    if (pm_launch_attn_split(t, S(st)))
        return fail(PM355_E_RANGE, "attn_decode_split: head_dim 64/128, at most 8 query heads per KV head, n_ctx % 8 == 0, scratch required");
    HIP_TRY(hipGetLastError());
    return 0;
}
int pm355_attn_prefill(const float * q, const void * kc, const void * vc, const int32_t * d_pos0, float * out, int n_tokens,
                       int H, int Hkv, int dh, int n_ctx, float kq_scale, pm355_stream_t st) {
    pm_attn_batch a = {};
    a.q = q; a.kc = kc; a.vc = vc; a.pos = d_pos0; a.out = out; a.n_tok = n_tokens; a.H = H; a.Hkv = Hkv; a.dh = dh; a.n_ctx = n_ctx; a.scale = kq_scale;
    if (pm_launch_attn_prefill(a, S(st)))
        return !d_pos0 || !out ? fail(PM355_E_SHAPE, "attn_prefill: null pointer")
                               : fail(PM355_E_RANGE, "attn_prefill: head_dim must be 64 or 128 and n_ctx a multiple of 32");
    HIP_TRY(hipGetLastError());
    return 0;
}
int pm355_attn_prefill_masked_ex(const float * q, const void * kc, const void * vc, const void * mask, int64_t mask_stride, float * out,
                                 int n_tokens, int H, int Hkv, int dh, int n_ctx, int n_kv, float kq_scale, int flags, pm355_stream_t st) {
    if (!mask) return fail(PM355_E_SHAPE, "attn_prefill_masked: mask required");
    pm_attn_batch a = {};
    a.q = q; a.kc = kc; a.vc = vc; a.mask = mask; a.mask_stride = (long) mask_stride; a.n_kv = n_kv; a.out = out; a.n_tok = n_tokens; a.H = H; a.Hkv = Hkv;
    a.dh = dh; a.n_ctx = n_ctx; a.scale = kq_scale; a.v_rowmajor = flags & PM355_ATTN_V_ROWMAJOR; a.mask_f16 = flags & PM355_ATTN_MASK_F16;
    if (pm_launch_attn_prefill(a, S(st)))
        return !out ? fail(PM355_E_SHAPE, "attn_prefill_masked: null pointer")
                    : fail(PM355_E_RANGE, "attn_prefill_masked: head_dim 64/128, n_ctx % 32 == 0, n_kv % 4 == 0 <= n_ctx required");
    HIP_TRY(hipGetLastError());
    return 0;
}
int pm355_attn_prefill_masked(const float * q, const void * kc, const void * vc, const float * mask, int64_t mask_stride, float * out,
                              int n_tokens, int H, int Hkv, int dh, int n_ctx, int n_kv, float kq_scale, pm355_stream_t st) {
    return pm355_attn_prefill_masked_ex(q, kc, vc, mask, mask_stride, out, n_tokens, H, Hkv, dh, n_ctx, n_kv, kq_scale, 0, st);
}
int pm355_attn_rope_fused(const float * q, const float * k, const float * v, void * kc, void * vc, const int32_t * d_pos0,
                          const float * ff, float * out, int H, int Hkv, int dh, int n_ctx, float kq_scale,
                          const pm355_rope_params * rp, pm355_stream_t st) {
    if (!rp || rp->n_dims % 2 || rp->n_dims > dh) return fail(PM355_E_SHAPE, "attn_rope_fused: n_dims");
    const pm_rope_cfg c = pm_rope_cfg_of(*rp);
    pm_attn_tok t = {};
    t.q = q; t.k = k; t.v = v; t.kc = kc; t.vc = vc; t.pos = d_pos0; t.freq_factors = ff; t.out = out;
    t.H = H; t.Hkv = Hkv; t.dh = dh; t.n_ctx = n_ctx; t.scale = kq_scale; t.rope = &c;
    if (pm_launch_attn_rope_fused(t, S(st)))
        return fail(PM355_E_UNSUPPORTED, "attn_rope_fused: head_dim must be 64/128/256, n_ctx % 8 == 0 and fit LDS");
    HIP_TRY(hipGetLastError());
    return 0;
}
int pm355_rope_table(const pm355_rope_params * rp, const int32_t * d_pos, const float * ff, float * table, pm355_stream_t st) {
    if (!rp || rp->n_dims % 2 || rp->n_dims > PM_ROPE_TABLE_DIMS_MAX || !d_pos || !table) return fail(PM355_E_SHAPE, "rope_table: n_dims (even, <= 256), d_pos and table required");
    pm_launch_rope_table(pm_rope_cfg_of(*rp), d_pos, nullptr, ff, table, S(st));
    HIP_TRY(hipGetLastError());
    return 0;
}
int pm355_mul_mat_vec_qkv(const pm355_matvec_job * jobs, int64_t K, const float * x_f32, const float * norm_w, float eps,
                          const pm355_qkv_store * s, pm355_stream_t st) {
    return pm355_mul_mat_vec_qkv_ss(jobs, K, x_f32, norm_w, eps, s, nullptr, 0, st);
}
int pm355_mul_mat_vec_qkv_ss(const pm355_matvec_job * jobs, int64_t K, const float * x_f32, const float * norm_w, float eps,
                             const pm355_qkv_store * s, const double * sumsq_in, int n_sumsq_in, pm355_stream_t st) {
    return pm355_mul_mat_vec_qkv_attn(jobs, K, x_f32, norm_w, eps, s, sumsq_in, n_sumsq_in, nullptr, st);
}
int pm355_mul_mat_vec_qkv_attn(const pm355_matvec_job * jobs, int64_t K, const float * x_f32, const float * norm_w, float eps,
                               const pm355_qkv_store * s, const double * sumsq_in, int n_sumsq_in, const pm355_qkv_attn * at, pm355_stream_t st) {
    if (!jobs || !x_f32 || !s || !s->rope_table || !s->k_cache || !s->v_cache || (!s->d_pos && !s->d_cell_nkv)) return fail(PM355_E_SHAPE, "mul_mat_vec_qkv: null pointer");
    pm_gemv_fused f = fused_of(jobs, 3, K, x_f32, norm_w, eps, true);
    if (sumsq_in && n_sumsq_in > 0 && norm_w) { f.ss_in = sumsq_in; f.n_ss = n_sumsq_in; }
    pm_qkv_epi e = qkv_epi_of(*s);
    if (at) {
        if (!at->out || !at->ticket) return fail(PM355_E_SHAPE, "mul_mat_vec_qkv_attn: null pointer");
        e.att_out = at->out; e.att_ticket = at->ticket; e.att_err = at->watchdog; e.kq_scale = at->kq_scale; e.n_head = at->n_head; e.att_max_keys = at->max_keys;
    }
    f.epi = &e;
    (void) hipGetLastError();
    const int rc = pm_launch_gemv_fused(f, S(st));
    if (rc) return gemv_rc(rc, MV_QKV);
    HIP_TRY(hipGetLastError());
    return 0;
}
#if PM_EXPERIMENTS
int pm355_engine_run(const pm355_engine_phase * phs, int n, pm355_stream_t st) {
    if (!phs || n < 1) return fail(PM355_E_SHAPE, "engine_run: phases");
    pm_eng_plan * pl = pm_eng_plan_new();
    int rc = 0;
    for (int i = 0; i < n && !rc; ++i) {
        const pm355_engine_phase & e = phs[i];
        if (e.kind == 0) {
            if (e.njobs < 1 || e.njobs > 3 || !e.jobs || !e.x_f32) { rc = -100; break; }
            pm_gemv_fused f = fused_of(e.jobs, e.njobs, e.K, e.x_f32, e.norm_w, e.eps);
            f.ss_out = e.sumsq_out; f.ss_in = e.sumsq_in; f.n_ss = e.n_sumsq_in;
            pm_qkv_epi qe = {};
            if (e.qkv) {
                const pm355_qkv_store * s = e.qkv;
                if (s->d_cell_nkv || !s->d_pos || e.njobs != 3) { rc = -100; break; }
                qe = qkv_epi_of(*s);
                f.epi = &qe;
            }
            rc = pm_eng_plan_add_matvec(pl, f);
        } else if (e.kind == 1) {
            rc = pm_eng_plan_add_attention(pl, e.q_rot, e.k_cache, e.v_cache, e.d_pos, nullptr, 0, e.out, e.n_head, e.n_head_kv, e.head_dim, e.n_ctx, e.kq_scale, e.max_keys);
        } else rc = -100;
    }
    if (!rc) rc = pm_eng_plan_finish(pl);
    if (rc) { pm_eng_plan_free(pl); (void) hipGetLastError(); char msg[96]; snprintf(msg, sizeof(msg), "engine_run: phase list not served (code %d)", rc); return fail(PM355_E_UNSUPPORTED, msg); }
    (void) hipGetLastError();
    pm_eng_plan_launch(pl, S(st));
    const hipError_t le = hipGetLastError();
    const hipError_t se = hipStreamSynchronize(S(st));
    const int w = pm_eng_plan_status(pl);
    pm_eng_plan_free(pl);
    if (le != hipSuccess) return fail(PM355_E_HIP, "engine_run: launch", le);
    if (se != hipSuccess) return fail(PM355_E_HIP, "engine_run: synchronize", se);
    if (w) { char msg[96]; snprintf(msg, sizeof(msg), "engine_run: watchdog code %d", w); return fail(PM355_E_HIP, msg); }
    return 0;
}
#else
int pm355_engine_run(const pm355_engine_phase *, int, pm355_stream_t) { return fail(PM355_E_UNSUPPORTED, "engine_run: the persistent decode engine is built into libprima_mi355_exp.so only (PM_EXPERIMENTS)"); }
#endif
int pm355_mul_mat_vec_qkv_check_ex(const pm355_matvec_job * jobs, int64_t K, int n_head_kv, int head_dim, int n_rot, int rope_neox) {
    if (!jobs) return fail(PM355_E_SHAPE, "mul_mat_vec_qkv_check: jobs");
    pm_gemv_fused f = fused_of(jobs, 3, K, (const float *) 16, nullptr, 0.0f, true);
    pm_qkv_epi e = {};
    e.tab = (const float *) 16; e.pos = (const int32_t *) 16; e.kc = (void *) 16; e.vc = (void *) 16;
    e.Hkv = n_head_kv; e.dh = head_dim; e.n_ctx = 8; e.n_rot = n_rot; e.neox = rope_neox ? 1 : 0;
    f.epi = &e;
    pm_gemv_plan pl; return gemv_rc(pm_gemv_fused_plan(f, 0, pl), MV_QKV_CHECK);
}
int pm355_mul_mat_vec_fused_plan(const pm355_matvec_job * jobs, int njobs, int64_t K, int x_mode, const pm355_qkv_store * qkv, int n_cus, int32_t * out, int n_out) {
    if (njobs < 1 || njobs > 3 || !jobs || x_mode < 0 || x_mode > 15 || !out) return -9;
    const float * const dx = (const float *) 16;             // stands for an activation, a weight vector, partial sums: never followed
    const int xm = x_mode & 3;
    pm_gemv_fused f = fused_of(jobs, njobs, K, xm ? dx : nullptr, xm >= 2 ? dx : nullptr, 0.0f);
    if (xm == 0) f.xq = dx;
    if (xm == 3) { f.ss_in = (const double *) dx; f.n_ss = 1; }
    if (x_mode & 4) f.dbg_int = (int32_t *) dx;
    if (x_mode & 8) f.ss_out = (double *) dx;
    pm_qkv_epi e = {}; if (qkv) { e = qkv_epi_of(*qkv); f.epi = &e; }
    pm_gemv_plan pl;
    if (const int rc = pm_gemv_fused_plan(f, n_cus, pl)) return rc;
    const pmv::GemvJob * j = pl.p.job;
    // [19..24]: the slice arithmetic of the three jobs of the block (GemvJob::rpw, then GemvJob::rmul as its bit pattern): workgroup b starts job j at row
    // b * rpw[j] + ((uint64) b * rmul[j] >> 32)
    const int32_t v[25] = {pl.grid, (int32_t) pl.lds, pl.ta, pl.tb, pl.pair, pl.first, j[0].split, j[1].split, j[2].split, j[0].nx_s, j[1].nx_s, j[2].nx_s,
                           pl.form.pair, pl.form.dbg, pl.form.epi, pl.form.npre, pl.form.feat, pl.form.xm, pl.form.hot,
                           j[0].rpw, j[1].rpw, j[2].rpw, (int32_t) j[0].rmul, (int32_t) j[1].rmul, (int32_t) j[2].rmul};
    for (int i = 0; i < n_out && i < 25; ++i) out[i] = v[i];
    return 0;
}
int pm355_mul_mat_vec_qkv_check(const pm355_matvec_job * jobs, int64_t K, int n_head_kv, int head_dim, int n_rot) {
    return pm355_mul_mat_vec_qkv_check_ex(jobs, K, n_head_kv, head_dim, n_rot, 0);
}
// the single-token attention entries: each fixes the form and its argument block, pm_attn_token_run (attn_plan.hip) holds the one switch
int pm355_attn_token_run(int form, const pm355_attn_token_args * a, const pm355_rope_params * rp, pm355_stream_t st) {
    if (!a) return fail(PM355_E_SHAPE, "attn_token_run: arguments");
    const char * why = nullptr;
    if (const int rc = pm_attn_token_run(form, *a, rp, S(st), &why)) return fail(rc, why);
    HIP_TRY(hipGetLastError());
    return 0;
}
int pm355_op_flash_attn_ext_fits(int64_t head_dim, int64_t n_kv) { return head_dim >= 8 && n_kv >= 0 && pm_flash_attn_ext_lds(head_dim, n_kv) <= PM_ATTN_LDS_MAX; }
int pm355_attn_token_plan(const pm355_attn_plan_in * in, pm355_attn_plan_out * out) {
    if (!in || !out) return fail(PM355_E_SHAPE, "attn_token_plan: arguments");
    pm_attn_token_plan(*in, *out);
    return 0;
}
static pm355_attn_token_args cached_args(const float * q_rot, void * kc, void * vc, const int32_t * d_pos, const int32_t * d_cell_nkv, const void * mask, float * out,
                                         float * scratch, int H, int Hkv, int dh, int n_ctx, float kq_scale, int max_keys, int flags) {
    pm355_attn_token_args a = {};
    a.q = q_rot; a.k_cache = kc; a.v_cache = vc; a.d_pos = d_pos; a.d_cell_nkv = d_cell_nkv; a.mask = mask; a.out = out; a.scratch = scratch;
    a.n_head = H; a.n_head_kv = Hkv; a.head_dim = dh; a.n_ctx = n_ctx; a.max_keys = max_keys; a.kq_scale = kq_scale; a.flags = flags;
    return a;
}
int pm355_attn_cached(const float * q_rot, void * kc, void * vc, const int32_t * d_pos, const int32_t * d_cell_nkv, const void * mask,
                      float * out, int H, int Hkv, int dh, int n_ctx, float kq_scale, int max_keys, int flags, pm355_stream_t st) {
    const pm355_attn_token_args a = cached_args(q_rot, kc, vc, d_pos, d_cell_nkv, mask, out, nullptr, H, Hkv, dh, n_ctx, kq_scale, max_keys,
                                                flags & (PM355_ATTN_V_ROWMAJOR | PM355_ATTN_MASK_F16));      // (this entry never read another flag)
    return pm355_attn_token_run(PM355_ATTN_FORM_CACHED, &a, nullptr, st);
}
int pm355_attn_cached_long(const float * q_rot, void * kc, void * vc, const int32_t * d_pos, const int32_t * d_cell_nkv, const void * mask,
                           float * out, float * scratch, int H, int Hkv, int dh, int n_ctx, float kq_scale, int max_cells, int flags, pm355_stream_t st) {
    const pm355_attn_token_args a = cached_args(q_rot, kc, vc, d_pos, d_cell_nkv, mask, out, scratch, H, Hkv, dh, n_ctx, kq_scale, max_cells, flags);
    return pm355_attn_token_run(PM355_ATTN_FORM_CACHED_LONG, &a, nullptr, st);
}
int pm355_attn_cached_long_check(int H, int Hkv, int dh, int n_ctx) { return pm_attn_flash_cached_shape_ok(H, Hkv, dh, n_ctx) ? 0 : PM355_E_UNSUPPORTED; }
int pm355_attn_token(const pm355_attn_token_args * a, const pm355_rope_params * rp, pm355_stream_t st) {
    if (!a) return fail(PM355_E_SHAPE, "attn_token: n_dims");
    (void) hipGetLastError();
    const bool q8 = a->flags & (PM355_ATTN_K_Q8_0 | PM355_ATTN_V_Q8_0);
    const int form = q8 ? (a->split ? PM355_ATTN_FORM_Q8_LONG : PM355_ATTN_FORM_Q8_TOKEN) : a->split ? pm_attn_long_raw_form() : PM355_ATTN_FORM_ROPE_FUSED;
    return pm355_attn_token_run(form, a, rp, st);
}
int pm355_set_i32x2(int32_t * d_p, int32_t a, int32_t b, pm355_stream_t st) { pm_launch_set_i32x2(d_p, a, b, S(st)); HIP_TRY(hipGetLastError()); return 0; }

int pm355_capture_begin(pm355_stream_t st) { HIP_TRY(hipStreamBeginCapture(S(st), hipStreamCaptureModeRelaxed)); return 0; }
pm355_graph_t pm355_capture_end(pm355_stream_t st) {
    hipGraph_t g = nullptr;
    hipError_t e = hipStreamEndCapture(S(st), &g);
    if (e != hipSuccess || !g) { fail(PM355_E_HIP, "hipStreamEndCapture", e); if (g) (void) hipGraphDestroy(g); return nullptr; }
    hipGraphExec_t x = nullptr;
    e = hipGraphInstantiate(&x, g, nullptr, nullptr, 0);
    (void) hipGraphDestroy(g);
    if (e != hipSuccess) { fail(PM355_E_HIP, "hipGraphInstantiate", e); return nullptr; }
    return (pm355_graph_t) x;
}
int pm355_graph_launch(pm355_graph_t g, pm355_stream_t st) { HIP_TRY(hipGraphLaunch((hipGraphExec_t) g, S(st))); return 0; }
void pm355_graph_free(pm355_graph_t g) { if (g) (void) hipGraphExecDestroy((hipGraphExec_t) g); }

int pm355_argmax(const float * x, int64_t n, int32_t * d_index, float * d_value, pm355_stream_t st) {
    pm_launch_argmax(x, (int) n, d_index, d_value, S(st)); HIP_TRY(hipGetLastError()); return 0;
}
int pm355_add(const float * a, const float * b, float * y, int64_t n, int64_t nb, pm355_stream_t st) { pm_launch_add(a, b, y, n, nb, S(st)); HIP_TRY(hipGetLastError()); return 0; }
int pm355_mul(const float * a, const float * b, float * y, int64_t n, int64_t nb, pm355_stream_t st) { pm_launch_mul(a, b, y, n, nb, S(st)); HIP_TRY(hipGetLastError()); return 0; }
int pm355_silu_mul(const float * g, const float * u, float * y, int64_t n, pm355_stream_t st) { pm_launch_silu_mul(g, u, y, n, S(st)); HIP_TRY(hipGetLastError()); return 0; }
int pm355_scale(const float * a, float * y, float s, int64_t n, pm355_stream_t st) { pm_launch_scale(a, y, s, n, S(st)); HIP_TRY(hipGetLastError()); return 0; }
int pm355_fill_random_blocks(int type, void * dst, int64_t K, int64_t nrows, uint64_t seed, float scale, pm355_stream_t st) {
    if (!pm_weight_row_bytes(type, K)) return fail(PM355_E_UNSUPPORTED, "fill_random_blocks: type");
    pm_launch_fill_random_blocks(type, dst, K, nrows, seed, scale, S(st)); HIP_TRY(hipGetLastError()); return 0;
}
} // extern "C"
