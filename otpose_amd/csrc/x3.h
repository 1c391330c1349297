// What the split-product ("x3") kernels share beyond csrc/common.h: the 8-float split into hi / lo records, and the conventions of
// the record-format 3x3 convolutions - S8 (csrc/convs.hip, csrc/convs2.hip: split fp32) and H8 (csrc/h16_kernels.h in csrc/h16.hip and csrc/hb.hip, with
// csrc/nhwc_conv.hip's packer: one 16-bit piece).  A weight packer and the kernels that read its image must agree on these, so they are
// written once, here.
#pragma once
#include "common.h"

// 8 floats -> hi / lo records of 8 pieces each: hi = rne(a), lo = rne(a - hi); P: the piece traits of common.h
template <typename P = otp_half_pieces>
__device__ __forceinline__ void otp_x3_split8(const float (&v)[8], otp_u32x4& hi, otp_u32x4& lo) {
    uint32_t h[4], l[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const otp_f32x2 a = {v[2 * i], v[2 * i + 1]};
        const uint32_t hb = __builtin_bit_cast(uint32_t, __builtin_convertvector(a, typename P::x2));
        const otp_f32x2 af = P::widen(hb);
        h[i] = hb;
        l[i] = __builtin_bit_cast(uint32_t, __builtin_convertvector(a - af, typename P::x2));
    }
    hi = (otp_u32x4){h[0], h[1], h[2], h[3]};
    lo = (otp_u32x4){l[0], l[1], l[2], l[3]};
}
// the same as MFMA operand vectors
template <typename P = otp_half_pieces>
__device__ __forceinline__ void otp_x3_split8(const float (&v)[8], typename P::x8& hi, typename P::x8& lo) {
    otp_u32x4 h, l;
    otp_x3_split8<P>(v, h, l);
    hi = __builtin_bit_cast(typename P::x8, h);
    lo = __builtin_bit_cast(typename P::x8, l);
}
// 4 floats -> the hi and the lo pieces as one 64-bit word each
template <typename P>
__device__ __forceinline__ void otp_x3_split4(otp_f32x4 v, unsigned long long& hi, unsigned long long& lo) {
    uint32_t h[2], l[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const otp_f32x2 a = {v[2 * i], v[2 * i + 1]};
        const uint32_t hb = __builtin_bit_cast(uint32_t, __builtin_convertvector(a, typename P::x2));
        const otp_f32x2 af = P::widen(hb);
        h[i] = hb;
        l[i] = __builtin_bit_cast(uint32_t, __builtin_convertvector(a - af, typename P::x2));
    }
    hi = (unsigned long long)h[0] | ((unsigned long long)h[1] << 32);
    lo = (unsigned long long)l[0] | ((unsigned long long)l[1] << 32);
}

// ---- weight image and row order of the S8 / H8 3x3 convolutions --------------------------------------------------------------------
constexpr int OTP_S8_KS = 5;              // k-steps per 16-channel chunk: 18 (tap, group) slots of 8 channels in 5 x 4 (2 zero-weight slots)
// 1 KB pieces of a chunk's packed S8 weights: 4 full k-steps x NTW tiles x (hi, lo) + the half-filled fifth (512 bytes per fragment)
__host__ __device__ constexpr int otp_s8_wch(int ntw) { return 8 * ntw + ntw; }

// Output-channel row of an MFMA tile <-> channel.  A lane's accumulator registers of a tile are rows 4 kl .. 4 kl + 3 (kl =
// lane / 16) of one pixel.  Cout tiles go in pairs (2 tp, 2 tp + 1): row 4 kl + r of the even tile is channel 8 kl + r of the
// pair's 32, of the odd tile channel 8 kl + 4 + r - a lane then holds 8 CONSECUTIVE channels of its pixel = one S8 record
// group (one H8 record), and the epilogue splits and stores them without any cross-lane traffic.  A tile without a partner (odd
// tile count, or the partner past Cout) keeps the identity: 4 consecutive channels per lane, stored as half records.
__host__ __device__ inline bool otp_tile_paired(int co_blk, int t, int ntw, int Cout) {
    const int tb = t | 1;
    return tb < ntw && co_blk + 16 * tb < Cout;
}
__host__ __device__ inline int otp_row2ch(int co_blk, int t, int row, int ntw, int Cout) {
    return otp_tile_paired(co_blk, t, ntw, Cout) ? co_blk + 32 * (t >> 1) + 8 * (row >> 2) + 4 * (t & 1) + (row & 3)
                                                 : co_blk + 16 * t + row;
}

// instruction order of one (k-step, pixel tile) block of the S8 kernels: NM MFMAs and NR LDS reads - [MFMA, read] pairs while
// reads remain (two MFMAs first when there are few), then the remaining MFMAs
template <int NM, int NR>
__device__ __forceinline__ void otp_s8_block_sched() {
    if constexpr (NR == 0) {
        __builtin_amdgcn_sched_group_barrier(0x008, NM, 0);
    } else if constexpr (NR == 1) {
        __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, NM - 2, 0);
    } else if constexpr (NR >= NM - 1) {
#pragma unroll
        for (int g = 0; g < NM - 1; ++g) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        }
        if constexpr (NR > NM - 1) __builtin_amdgcn_sched_group_barrier(0x100, NR - (NM - 1), 0);
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
    } else {
        __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, NM / 2 - 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, NR - 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, NM - 1 - NM / 2, 0);
    }
}
