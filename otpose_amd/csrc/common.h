// Shared helpers for the gfx950 kernels of libotpose_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <atomic>

#include "../../include/otpose_hip.h"

#define OTP_LDS_LIMIT (160 * 1024)

static inline int otp_launch_status() {
    return hipGetLastError() == hipSuccess ? OTP_OK : OTP_ERR_LAUNCH;
}

// Raise the dynamic-LDS limit of a kernel once per DEVICE and per kernel instantiation (the flags live in the
// enclosing template instantiation): hipFuncSetAttribute applies to the device that is current at the call, so a
// process driving several GPUs must set it on each.  Set-once, so launches stay graph-capturable; the flag is an
// atomic bit per device (two threads racing both set the attribute, which is idempotent).
#define OTP_MAX_DEVICES 64
#define OTP_ALLOW_BIG_LDS(kern, bytes)                                                                      \
    do {                                                                                                    \
        if ((bytes) > 64 * 1024) {                                                                          \
            static std::atomic<uint64_t> otp_done_{0};                                                      \
            int otp_dev_ = 0;                                                                               \
            (void)hipGetDevice(&otp_dev_);                                                                  \
            const uint64_t otp_bit_ = 1ull << (otp_dev_ & (OTP_MAX_DEVICES - 1));                           \
            if (!(otp_done_.load(std::memory_order_acquire) & otp_bit_)) {                                  \
                (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern),                              \
                                          hipFuncAttributeMaxDynamicSharedMemorySize, OTP_LDS_LIMIT);       \
                otp_done_.fetch_or(otp_bit_, std::memory_order_release);                                    \
            }                                                                                               \
        }                                                                                                   \
    } while (0)

static inline int otp_ceil_div(int a, int b) { return (a + b - 1) / b; }

// the vector types of every kernel file (16-bit element vectors: otp_x3x2 / otp_x3x8 below; csrc/h16_kernels.h takes its element
// type from a traits parameter, csrc/nhwc.h is bfloat16 only)
typedef float otp_f32x4 __attribute__((ext_vector_type(4)));
typedef float otp_f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int otp_u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int otp_u32x2 __attribute__((ext_vector_type(2)));

// ---- index arithmetic --------------------------------------------------------------------------------------------------------
// floor(i / d) for i * d < 2^32 with magic = floor(2^32 / d) + 1 (0 encodes d == 1); the host side computes the magic number
__device__ __forceinline__ uint32_t otp_magic_div(uint32_t i, uint32_t magic) { return magic ? __umulhi(i, magic) : i; }
static inline uint32_t otp_magic(uint32_t d) { return d <= 1 ? 0u : (uint32_t)((1ull << 32) / d) + 1u; }   // exact while i * d < 2^32
// a * b for per-lane index arithmetic whose operands stay below 2^24 (checked by the plans): v_mul_u32_u24 issues at full rate,
// v_mul_lo_u32 at a quarter of it - 40 of them sat in the set-up of every tile of csrc/h16.hip
__device__ __forceinline__ int otp_mul24(int a, int b) { return (int)__umul24((unsigned)a, (unsigned)b); }

// wave64 reductions (DPP-lowered __shfl_xor)
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ float otp_kslot_sum(float v) {  // sum over the four k-slot lane groups (lanes n, n+16, n+32, n+48)
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    return v;
}
// sum over the 16 lanes of a DPP row (one MFMA pixel column group) with four VALU adds; every lane ends with the total.
// (__shfl_xor with offsets 4 and 8 lowers to ds_bpermute on gfx950: 96 LDS round trips in the old epilogue of csrc/nhwc_conv.hip)
template <int CTRL>
__device__ __forceinline__ float otp_dpp_mov(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, false));
}
__device__ __forceinline__ float otp_row16_sum(float v) {
    v += otp_dpp_mov<0xB1>(v);    // quad_perm [1,0,3,2]
    v += otp_dpp_mov<0x4E>(v);    // quad_perm [2,3,0,1]
    v += otp_dpp_mov<0x124>(v);   // row_ror:4
    v += otp_dpp_mov<0x128>(v);   // row_ror:8
    return v;
}

// ---- counter-based dropout draws ------------------------------------------------------------------------------------------------
// A hash of (element pair, 64-bit seed) with the lowbias32 finaliser: two 16-bit uniforms per 32-bit hash, keep <=> u16 >= round(65536 p).
// Users: the bf16 training path (csrc/hb.h: otp_drop_keep8) and the attention-probability dropout below.
__device__ __forceinline__ uint32_t otp_drop_hash(size_t pair, uint32_t s0, uint32_t s1) {
    uint32_t h = (uint32_t)pair * 0x9E3779B1u + s0;
    h ^= ((uint32_t)(pair >> 32) + s1) * 0x85EBCA77u;
    h ^= h >> 16; h *= 0x21F0AAADu; h ^= h >> 15; h *= 0x735A2D97u; h ^= h >> 15;
    return h;
}
// Attention-probability dropout (include/otpose_hip.h, "attention dropout mask"): the probability matrix of an attention is
// (G groups, R rows, Ccols columns); entry (g, i, j) draws from pair ((g R + i) ceil(Ccols / 2) + j / 2), the low half of the hash
// for an even j, the high half for an odd one.  A pure function of (seed, g, i, j, p): every kernel that needs the mask - forward,
// both backward passes, the mask writer - evaluates it in place through these three functions.
struct otp_attn_drop {
    uint32_t s0, s1, thr;
    float keep_scale;                                              // 65536 / (65536 - thr): what a survivor is multiplied by
};
// a rate is p in [0, 1) whose threshold stays below 65536 (p < 1 - 2^-17: from there on every entry would be dropped); false for NaN
static inline bool otp_attn_drop_rate_ok(float p) { return p >= 0.f && p < 1.f && (uint32_t)(p * 65536.f + 0.5f) < 65536u; }
static inline otp_attn_drop otp_attn_drop_make(float p, unsigned long long seed) {   // p: otp_attn_drop_rate_ok
    const uint32_t thr = (uint32_t)(p * 65536.f + 0.5f);
    return otp_attn_drop{(uint32_t)seed, (uint32_t)(seed >> 32), thr, 65536.f / (float)(65536u - thr)};
}
// first pair of row (g R + i): add j / 2 for the pair of column j
__device__ __forceinline__ uint64_t otp_attn_drop_row(uint64_t row, int Ccols) { return row * (uint64_t)((Ccols + 1) >> 1); }
__device__ __forceinline__ uint32_t otp_attn_drop_draw(const otp_attn_drop& d, uint64_t pair) {
    return otp_drop_hash((size_t)pair, d.s0, d.s1);
}
// the factor of column j (only its parity counts) from its pair's hash: keep_scale for a survivor, 0 for a dropped entry
__device__ __forceinline__ float otp_attn_drop_factor(const otp_attn_drop& d, uint32_t h, int j) {
    return ((j & 1) ? (h >> 16) : (h & 0xFFFFu)) >= d.thr ? d.keep_scale : 0.f;
}
__device__ __forceinline__ float otp_attn_drop_at(const otp_attn_drop& d, uint64_t row_pair, int j) {
    return otp_attn_drop_factor(d, otp_attn_drop_draw(d, row_pair + (uint64_t)(j >> 1)), j);
}

// ---- GELU ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float otp_gelu_erf(float x) { return 0.5f * x * (1.f + erff(x * 0.70710678118654752440f)); }
// erf-GELU on a pair of accumulator values, branch-free and in packed-f32 form (v_pk_fma_f32): erf(t) = t P(t^2) / Q(t^2)
// on |t| <= 4 (the classic single-precision rational fit; erf is 1 - 1.5e-8 beyond), max abs error 4.2e-7 on erf and
// 7e-7 on gelu(x) over the whole real line - checked against fp64 in tests/test_gpu_ops.py.  The libm erff the other
// epilogues call has two data-dependent paths, and both would run for every accumulator register of a wave in the MLP
// kernels (csrc/mlp.hip, csrc/mlpx.hip).
__device__ __forceinline__ otp_f32x2 otp_gelu2(otp_f32x2 x) {
    otp_f32x2 t = x * 0.70710678118654752440f;
    t.x = __builtin_amdgcn_fmed3f(t.x, -4.f, 4.f);
    t.y = __builtin_amdgcn_fmed3f(t.y, -4.f, 4.f);
    const otp_f32x2 t2 = t * t;
    otp_f32x2 p = t2 * -2.72614225801306e-10f + 2.77068142495902e-08f;
    p = p * t2 + -2.10102402082508e-06f;
    p = p * t2 + -5.69250639462346e-05f;
    p = p * t2 + -7.34990630326855e-04f;
    p = p * t2 + -2.95459980854025e-03f;
    p = p * t2 + -1.60960333262415e-02f;
    p = p * t;
    otp_f32x2 q = t2 * -1.45660718464996e-05f + -2.13374055278905e-04f;
    q = q * t2 + -1.68282697438203e-03f;
    q = q * t2 + -7.37332916720468e-03f;
    q = q * t2 + -1.42647390514189e-02f;
    otp_f32x2 r;
    r.x = __builtin_amdgcn_rcpf(q.x);
    r.y = __builtin_amdgcn_rcpf(q.y);
    const otp_f32x2 e = p * r, hx = x * 0.5f;
    return hx * e + hx;
}

// ---- buffer (SRSRC) addressing: one VGPR byte offset + one SGPR byte offset per access -------------
// gfx9-family dword3 (DST_SEL/format) constant for raw buffers
#define OTP_BUFFER_DWORD3 0x00020000
typedef __amdgpu_buffer_rsrc_t otp_rsrc;
constexpr int OTP_OOB = -16;              // byte offset outside every descriptor: a load returns zeros, the LDS-DMA writes zeros, a store is dropped
__device__ __forceinline__ otp_rsrc make_rsrc(const void* p, size_t bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0,
                                             (int)(bytes > 0xffffffffull ? 0xffffffffull : bytes), OTP_BUFFER_DWORD3);
}
// same with a 32-bit size known to fit (no 64-bit clamp arithmetic)
__device__ __forceinline__ otp_rsrc make_rsrc32(const void* p, unsigned bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, (int)bytes, OTP_BUFFER_DWORD3);
}
__device__ __forceinline__ float bload(otp_rsrc r, int voff_bytes, int soff_bytes) {
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, voff_bytes, soff_bytes, 0));
}

// ---- the 16-bit operand type of the split ("x3") products ------------------------------------------------------------------
// Every fp32 operand a of the convolutions / projections / MLPs / attention products of the eval path is carried as two 16-bit
// pieces, hi = rne(a), lo = rne(a - hi), and a product is accumulated in fp32 as a_lo*b_hi + a_hi*b_lo + a_hi*b_hi on the
// 16x16x32 MFMA (csrc/convx.hip).  Rounds 2-3 used bfloat16 pieces: 8 significand bits each, a = hi + lo to 2^-17.  Round 4
// switched to IEEE half: 11 bits each, a = hi + lo to max(2^-22 |a|, 2^-25) - the f16 MFMA of gfx950 has the same rate as the
// bf16 one and takes SUBNORMAL f16 inputs exactly (tools/micro/mfma_f16_denorm.hip), which the small `lo` pieces need.  Range:
// operands above 65504 become infinities (BatchNorm-folded weights and heat-map activations are orders of magnitude below).
// The piece type is a traits parameter of the kernels that exist for both (csrc/densex.hip, the attention products of
// csrc/chanattn.hip: bfloat16 pieces for the GRADIENT operands of the training backward); every other file uses the half
// aliases below.
struct otp_half_pieces {
    typedef _Float16 elem;
    typedef _Float16 x2 __attribute__((ext_vector_type(2)));
    typedef _Float16 x8 __attribute__((ext_vector_type(8)));
    static constexpr float range_limit = 65504.f;
    static __device__ __forceinline__ otp_f32x4 mfma(x8 a, x8 b, otp_f32x4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
    }
    // the two pieces of a packed pair back as fp32
    static __device__ __forceinline__ otp_f32x2 widen(uint32_t pair) {
        return __builtin_convertvector(__builtin_bit_cast(x2, pair), otp_f32x2);
    }
};
struct otp_bf16_pieces {
    typedef __bf16 elem;
    typedef __bf16 x2 __attribute__((ext_vector_type(2)));
    typedef __bf16 x8 __attribute__((ext_vector_type(8)));
    static constexpr float range_limit = 3.0e38f;                  // fp32's own range
    static __device__ __forceinline__ otp_f32x4 mfma(x8 a, x8 b, otp_f32x4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
    }
    static __device__ __forceinline__ otp_f32x2 widen(uint32_t pair) {
        return __builtin_convertvector(__builtin_bit_cast(x2, pair), otp_f32x2);
    }
};
typedef otp_half_pieces::elem otp_x3_t;
typedef otp_half_pieces::x2 otp_x3x2;
typedef otp_half_pieces::x8 otp_x3x8;
#define OTP_X3_MFMA __builtin_amdgcn_mfma_f32_16x16x32_f16       /* what otp_half_pieces::mfma wraps, with its three modifiers */
__device__ __forceinline__ otp_f32x2 otp_x3_widen(uint32_t pair) { return otp_half_pieces::widen(pair); }

// ---- range guard of the 16-bit-operand kernels (csrc/range.hip) ----------------------------------------------------------------
// A half piece overflows at 65504: hi = rne(a) = inf, lo = rne(a - hi) = -inf, every product with it NaN - and a ReLU (v_max_f32
// drops a quiet NaN) or the DCN's open-interval test can swallow that NaN silently.  Every kernel that forms such pieces
// therefore tests ITS RESULTS before the activation - a NaN accumulator is an operand that overflowed, |v| >= 65504 is a value
// the next consumer could not split - and stores a code word through `otp_range_word()` (one word of pinned host memory, visible
// to every device of the process; written only on a violation, so the guard costs a compare per result and no memory traffic).
// include/otpose_hip.h: otp_range_flag_read / otp_range_poison.
enum {
    OTP_RANGE_CONVX = 1, OTP_RANGE_CONVS = 2, OTP_RANGE_CONVS2 = 3, OTP_RANGE_POINTX = 4, OTP_RANGE_STEM = 5, OTP_RANGE_S8PASS = 6,
    OTP_RANGE_MLPX = 7, OTP_RANGE_DENSEX = 8, OTP_RANGE_ATTN = 9, OTP_RANGE_DCNF = 10, OTP_RANGE_H16 = 11,
    OTP_RANGE_TOKATTN_H = 12
};
unsigned* otp_range_word();                                        // host side: the word's address (NULL without a GPU)
template <typename P>                                              // P: the piece traits above, whose range_limit is the bound
__device__ __forceinline__ bool otp_out_of_range(float v) {
#ifdef OTP_NO_RANGE_GUARD                                          /* development A/B only (tools/lib_variant.sh): what the guard costs */
    return false;
#else
    return !(__builtin_fabsf(v) < P::range_limit);                 // true for NaN too
#endif
}
__device__ __forceinline__ bool otp_out_of_range(float v) { return otp_out_of_range<otp_half_pieces>(v); }
__device__ __forceinline__ void otp_range_report(unsigned* word, bool bad, unsigned code) {
    if (bad && word) __hip_atomic_store(word, code, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
// max(x, 0) as ONE instruction.  fmaxf lowers to v_max_f32 x, x (the IEEE quieting of a signalling NaN) + v_max_f32 x, 0: two vector
// instructions per value in epilogues that are bound by vector issue (48 values per lane and tile in the conv kernels).
__device__ __forceinline__ float otp_relu(float x) {
    float y;
    asm("v_max_f32 %0, 0, %1" : "=v"(y) : "v"(x));
    return y;
}
// 16-byte buffer load: offsets at or past the descriptor's size return zeros (hardware range check)
__device__ __forceinline__ otp_f32x4 bload4(otp_rsrc r, int voff_bytes) {
    return __builtin_bit_cast(otp_f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, voff_bytes, 0, 0));
}
__device__ __forceinline__ void bstore(float v, otp_rsrc r, int voff_bytes, int soff_bytes) {
    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, v), r, voff_bytes, soff_bytes, 0);
}

// ---- LDS-DMA ----------------------------------------------------------------------------------------------------------------------
// copy one block of BLKB bytes (a multiple of 1 KB) global -> LDS with the LDS-DMA (global_load_lds, no staging registers), all NTHR
// threads of the workgroup: unit u (16 bytes) lands at lds + 16 u; a wave-instruction covers 64 units, so it is inside the block
// or past it, and the bound test exists only when the last pass of the workgroup is partial
template <int NTHR, int BLKB>
__device__ __forceinline__ void otp_lds_stage(const unsigned char* __restrict__ src, unsigned char* lds) {
    constexpr int UNITS = BLKB / 16, NST = (UNITS + NTHR - 1) / NTHR;
    static_assert(BLKB % 1024 == 0, "whole wave-instructions");
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
#pragma unroll
    for (int i = 0; i < NST; ++i) {
        const int u0 = i * NTHR + wave * 64;                       // wave-uniform first unit of this wave-instruction
        if (UNITS % NTHR != 0 && u0 * 16 >= BLKB) break;
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + (size_t)(u0 + lane) * 16),
                                         (__attribute__((address_space(3))) void*)(lds + u0 * 16), 16, 0, 0);
    }
}
