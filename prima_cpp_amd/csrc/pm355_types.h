// pm355_types.h — the facts about each weight type, written down once. Plain C++17 with no HIP header: the kernels, their host launchers and the
// ggml plug-in (compiled with g++) all read this table. Everything here is constexpr, so kernels may use the accessors on template parameters.
//
// Adding a weight type: one row below, its pm355_device.h stride function if a stream is padded, then the per-launcher sets at the top of
// mmvq.hip / mmq.hip / mmq_i8.hip / mmq_pf.hip / mmq_big.hip (DESIGN.md "Adding a weight type").
#pragma once
#include <stddef.h>
#include <stdint.h>

// the values of ggml_type (ggml_graph_plan.h asserts it): a tensor's type crosses the C ABI as a plain int
enum pm_type : int { PM_F32 = 0, PM_F16 = 1, PM_Q5_0 = 6, PM_Q8_0 = 8, PM_Q4_K = 12, PM_Q5_K = 13, PM_Q6_K = 14, PM_Q8_K = 15 };

// GGUF block bytes (block layouts: pm355_device.h)
#define PM_BS_Q5_0 22
#define PM_BS_Q8_0 34
#define PM_BS_Q4_K 144
#define PM_BS_Q5_K 176
#define PM_BS_Q6_K 210
#define PM_BS_Q8_K 292

struct pm_type_rec {
    int  block;       // values per GGUF block: 1, 32 or 256; 0 = not a weight type this library stores
    int  bytes;       // GGUF bytes per block
    bool soa;         // the HBM image is row-SoA, not GGUF block order (repack.hip)
    int  pad;         // granule the trailing scale stream(s) of a row are padded to: row stride != row bytes (pm_weight_row_stride); 0 = none
    bool q80_act;     // multiplies with Q8_0 activations (32-value blocks, ggml.c type_traits vec_dot_type); else Q8_K
    int  nv;          // values per unit of the mat-vec (mmvq_device.h QT<>::NV); 0 = not a quantized weight matrix
    bool embed;       // the embedding row lookup decodes it (layer_ops.hip pm_dequant_elem)
};
// indexed by pm_type. Q8_K (15) is the activation format of the K-quants, never a weight: no row
constexpr int PM_N_TYPES = 16;
inline constexpr pm_type_rec PM_TYPES[PM_N_TYPES] = {
    /*  0 F32  */ {1,   4,          false, 0,  false, 0,  true},
    /*  1 F16  */ {1,   2,          false, 0,  false, 0,  true},
    {}, {}, {}, {},
    /*  6 Q5_0 */ {32,  PM_BS_Q5_0, true,  16, true,  32, false},    // (embedding rows: not built, the callers refuse them instead of returning zeros)
    {},
    /*  8 Q8_0 */ {32,  PM_BS_Q8_0, true,  16, true,  32, true},
    {}, {}, {},
    /* 12 Q4_K */ {256, PM_BS_Q4_K, true,  0,  false, 64, true},     // (144-byte blocks: every stream of the row is 16-byte aligned without padding)
    /* 13 Q5_K */ {256, PM_BS_Q5_K, false, 0,  false, 32, true},
    /* 14 Q6_K */ {256, PM_BS_Q6_K, true,  16, false, 64, true},
    {},
};
static_assert(PM_TYPES[PM_Q5_0].bytes == 22 && PM_TYPES[PM_Q8_0].bytes == 34 && PM_TYPES[PM_Q4_K].bytes == 144 && PM_TYPES[PM_Q5_K].bytes == 176 &&
              PM_TYPES[PM_Q6_K].bytes == 210 && PM_TYPES[PM_F16].bytes == 2 && PM_TYPES[PM_Q8_K].block == 0, "a row of PM_TYPES sits at the wrong index");

constexpr pm_type_rec pm_type_info(int t) { return t >= 0 && t < PM_N_TYPES ? PM_TYPES[t] : pm_type_rec{}; }

// values per block; for a quantized weight also the block length of the activations it multiplies with (K must be a multiple)
constexpr int  pm_block_len(int t) { return pm_type_info(t).block; }
// bytes of one WEIGHT row in GGUF order (== ggml_row_size); 0: not a stored type
constexpr size_t pm_weight_row_bytes(int t, int64_t K) { return pm_block_len(t) ? (size_t) (K / pm_block_len(t)) * pm_type_info(t).bytes : 0; }
// HBM layout != GGUF block order
constexpr bool pm_type_is_repacked(int t) { return pm_type_info(t).soa; }
// weights whose vec_dot_type is Q8_0: one activation family in every kernel
constexpr bool pm_q80_family(int t) { return pm_type_info(t).q80_act; }
// a quantized weight matrix the mat-vec / mat-mul launchers know (each launcher's own set says which of them it serves)
constexpr bool pm_is_quant_weight(int t) { return pm_type_info(t).nv != 0; }
constexpr bool pm_embed_type_ok(int t) { return pm_type_info(t).embed; }

// sets of types as bit masks over pm_type: what a launcher serves is one named constant at the top of its file
template <typename... T> constexpr uint32_t pm_type_set(T... t) { return ((1u << t) | ...); }
constexpr bool pm_in_set(uint32_t set, int t) { return t >= 0 && t < PM_N_TYPES && ((set >> t) & 1u); }
constexpr uint32_t pm_quant_weight_set() { uint32_t s = 0; for (int t = 0; t < PM_N_TYPES; ++t) if (PM_TYPES[t].nv) s |= 1u << t; return s; }
constexpr uint32_t PM_QUANT_WEIGHTS = pm_quant_weight_set();       // Q5_0, Q8_0, Q4_K, Q5_K, Q6_K
