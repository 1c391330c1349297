// The 16-bit record kernels two translation units instantiate: the 3x3 window / weight-stream convolution and the register-resident
// 1x1 convolution, with their plans and launches.  csrc/h16.hip runs them on IEEE half H8 images (the fp16 eval engine: folded
// BatchNorm, range guard), csrc/hb.hip on bfloat16 NHWC tensors (the training step's forward / input-gradient convolutions, reached
// through csrc/nhwc_conv.hip: per-tile channel statistics instead of the folded BatchNorm).  Same window, weight stream and MFMA schedule;
// the records' addresses are (pixel stride, group stride) pairs, and what differs is the element traits T below.  Internal linkage
// throughout, as in the .hip files: each translation unit gets its own copies.
#pragma once
#include "common.h"
#include "hb.h"
#include <cstdlib>

namespace {

// ---- element traits: T::x8 (an MFMA operand = one record), T::mfma, T::widen, T::pack8, T::training -----------------------------
template <typename E>
struct HElem {
    typedef E x2 __attribute__((ext_vector_type(2)));
    typedef E x8 __attribute__((ext_vector_type(8)));
    static __device__ __forceinline__ otp_u32x4 pack8(const float (&v)[8]) {        // one rounding per value
        uint32_t h[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) h[i] = __builtin_bit_cast(uint32_t, (x2){(E)v[2 * i], (E)v[2 * i + 1]});
        return (otp_u32x4){h[0], h[1], h[2], h[3]};
    }
};
struct Half : HElem<_Float16> {               // eval: out = act(post * sum + shift (+ res)), one rounding, range guard
    static constexpr bool training = false;
    static __device__ __forceinline__ otp_f32x4 mfma(x8 a, x8 b, otp_f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ otp_f32x2 widen(uint32_t pair) { return __builtin_convertvector(__builtin_bit_cast(x2, pair), otp_f32x2); }
};
struct Bf16 : HElem<__bf16> {                 // training: out = bf16(sum + bias) (+ res as a separate bf16 add), statistics of the stored values
    static constexpr bool training = true;
    static __device__ __forceinline__ otp_f32x4 mfma(x8 a, x8 b, otp_f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ otp_f32x2 widen(uint32_t pair) {
        return (otp_f32x2){__builtin_bit_cast(float, pair << 16), __builtin_bit_cast(float, pair & 0xffff0000u)};
    }
};

#ifdef OTP_H16_TIMING
// development build only (tools/h16_timing.sh): per-workgroup phase stamps, never in libotpose_hip.so
__device__ unsigned long long otp_h16_stamps[8192 * 32];
#define HSTAMP(slot)                                                                                                       \
    do {                                                                                                                   \
        if (threadIdx.x == 0 && blockIdx.x < 8192) otp_h16_stamps[blockIdx.x * 32 + (slot)] = __builtin_readcyclecounter(); \
    } while (0)
#else
#define HSTAMP(slot)
#endif

// packed weights of a (cout block, 16-channel chunk): 4 full k-steps x NTW tiles x 1 KB, then the half-filled fifth (k-slots 16, 17
// on lanes 0 .. 31: 512 bytes per tile)
__host__ __device__ constexpr int hwb(int ntw) { return otp_hb_wb(ntw); }
// training: the four waves' partial channel sums behind the weight image
template <typename T>
__host__ __device__ constexpr int hsred(int ntw) { return T::training ? 4 * 2 * ntw * 16 * 4 : 0; }

// instruction order of one (k-step, pixel tile) block: NM MFMAs and NR LDS reads interleaved (another order than
// csrc/x3.h: otp_s8_block_sched - with one product per multiply there are fewer MFMAs per read)
template <int NM, int NR>
__device__ __forceinline__ void hblock_sched() {
    if constexpr (NR == 0) {
        __builtin_amdgcn_sched_group_barrier(0x008, NM, 0);
    } else if constexpr (NR >= NM) {
        // [MFMA, read] pairs, the surplus reads behind the last MFMA's pair
#pragma unroll
        for (int g = 0; g < NM - 1; ++g) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        }
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, NR - (NM - 1), 0);
    } else {
#pragma unroll
        for (int g = 0; g < NR; ++g) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        }
        __builtin_amdgcn_sched_group_barrier(0x008, NM - NR, 0);
    }
}

// ================================================================================================================================
// 3x3 / pad 1 convolution, stride 1 or 2, H8 -> H8 (+ H8 residual) (+ ReLU)
// ================================================================================================================================
struct HPlan {
    int N, C, H, W, HW, Ho, Wo, HWo, Cout, total;      // total = N * Ho * Wo output pixels
    int act;
    // where records live, in bytes: record (image n, channel group g, pixel p) of a tensor is at base + n imgB + g gS + p pS.
    // H8: pS = 16, gS = 16 HW, imgB = 16 gtot HW, base = 16 goff HW.  NHWC with CS channels: pS = 2 CS, gS = 16, imgB = 2 CS HW
    int in_pS, in_gS, in_imgB, out_pS, out_gS, out_imgB, res_pS, res_gS, res_imgB;
    size_t in_base, out_base, res_base;
    float* stats;                                      // training: per-tile channel sums [nTiles][2][Cout] of the stored values, or NULL
    float pre, post;                                   // weights carry 2^k = pre; the sum is multiplied by post = 2^-k
    int NTW, nN, nTiles, nChunks, tpx, NPT;
    int CK;                                            // input channels per WINDOW stage (a multiple of 16 that divides Cin)
    int VR, W1, NIW, NV, pl;                           // virtual rows per image (H + 1), records per virtual row (W + 1), 64-record
                                                       // pieces / records / bytes of a window plane
    uint32_t mHWo, mWo, mW1, mVR;
    unsigned* rflag;
};

// Workgroup = 64 NPT flattened output pixels x 16 NTW output channels, 4 waves; K = input channels x 9 taps.
// LDS: [CK / 8 window planes | one 16-channel weight chunk].  Window (stride 1, csrc/convs.hip): record index = (virtual row) *
// (W + 1) + 1 + x from the first record a tap of the tile reads, one zero record between rows, one zero row above every image;
// (stride 2, csrc/convs2.hip): a virtual row is [0 | odd columns | even columns] so that consecutive output pixels read consecutive
// records.  The window arrives by LDS-DMA; padding = lanes whose source offset is outside the descriptor.
// With ONE product per multiply a 16-channel chunk is ~1 k cycles of MFMA against a ~4 k cycle HBM round trip, and a ring of
// 16-channel stages measured no better than no ring at all (profiles/r05_h16_ring_sweep.txt: what hides latency is other
// workgroups, and every stage costs them LDS).  So the WINDOW of CK = 48 .. 96 channels is staged at once - one round trip per CK
// channels instead of one per 16 - and only the weights (L2-resident, 13.5 KB per 16 channels) stream: the next chunk's
// weights are loaded into registers under the current chunk's MFMAs and written to the LDS behind them.
#ifndef OTP_H16_MINWG
#define OTP_H16_MINWG 3                   /* development A/B (tools/lib_variant.sh): waves per SIMD the register budget is cut for */
#endif
// MODE (compile time - as run-time branches the statistics / residual forms cost the plain one registers): 0 plain, 1 per-tile
// channel statistics (training only), 2 residual
template <typename T, int NTW, int NPT, int STRIDE, int MODE = 0>
__global__ __launch_bounds__(256, STRIDE == 1 ? OTP_H16_MINWG : 2) void h16_conv3x3_kernel(const unsigned char* __restrict__ xs,
                                                                                const unsigned char* __restrict__ wpk,
                                                                                const float* __restrict__ shift,
                                                                                const unsigned char* res, unsigned char* out,
                                                                                const HPlan P) {
    constexpr int BM = 64 * NPT, WB = hwb(NTW), WU = WB / 16, NWJ = (WU + 255) / 256, NBLK = OTP_S8_KS * NPT, MAXJ = STRIDE == 1 ? 2 : 4;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int PL = P.pl, NPL = P.CK >> 3, SUB = P.CK >> 4;          // bytes of a window plane, planes / weight chunks per stage
    unsigned char* const wl = smem + NPL * PL;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i16 = lane & 15, kl = lane >> 4;
    const bool upper = kl >= 2;

    // workgroup -> (pixel tile, cout block): XCD x walks a contiguous tile range, the blocks of a tile back to back (shared L2 lines)
    const int xcd = (int)blockIdx.x & 7, jb = (int)blockIdx.x >> 3;
    const int tl = jb / P.nN, cb = jb - tl * P.nN;
    const int tile = xcd * P.tpx + tl;
    if (tile >= P.nTiles) return;
    HSTAMP(0);
#ifdef OTP_H16_TIMING
    if (threadIdx.x == 0 && blockIdx.x < 8192) otp_h16_stamps[blockIdx.x * 32 + 30] = __builtin_amdgcn_s_memrealtime();
#endif
    const int P0 = tile * BM;
    const int n0 = P0 / P.HWo, p0 = P0 - n0 * P.HWo;               // (uniform, once per workgroup)
    const int y0 = (int)otp_magic_div((uint32_t)p0, P.mWo);
    const int x0 = STRIDE == 1 ? p0 - y0 * P.Wo : 0;               // stride 1: the window starts at record x0 of its first row
    const int Vf = n0 * P.VR + STRIDE * y0;                        // first virtual row of the window
    const int imgB = P.in_imgB;                                    // bytes of one image of the input tensor
    const int co_blk = cb * NTW * 16;

    // ---- window pieces of this wave: piece k = wave + 4 j covers window records 64 k .. 64 k + 63 of every plane ----------------
    // (arrays of a fixed bound: with a template-dependent bound captured by the lambda below hipcc 7.2's host pass emits no kernel stub)
    int voff[4];
    bool vlive[4];
#pragma unroll
    for (int j = 0; j < MAXJ; ++j) {
        const int v = 64 * (wave + 4 * j) + lane;
        vlive[j] = v < P.NV;
        const int vv = v + x0;
        const int r = (int)otp_magic_div((uint32_t)vv, P.mW1), i = vv - otp_mul24(r, P.W1);
        const int V = Vf + r;
        const int n = (int)otp_magic_div((uint32_t)V, P.mVR), yy = V - otp_mul24(n, P.VR);
        const int col = STRIDE == 1 ? i - 1 : (i <= P.Wo ? 2 * (i - 1) + 1 : 2 * (i - P.Wo - 1));   // stride 2: odd columns, then even
        const bool ok = i >= 1 && yy >= 1 && n < P.N;
        voff[j] = ok ? (n - n0) * imgB + otp_mul24(otp_mul24(yy - 1, P.W) + col, P.in_pS) : OTP_OOB;    // (imgB may pass 2^24: a full multiply)
    }
    const size_t left = (size_t)(P.N - n0) * imgB - P.in_base;
    const otp_rsrc rin = make_rsrc32(xs + (size_t)n0 * imgB + P.in_base, left > 0x7fffff00ull ? 0x7fffff00u : (unsigned)left);
    const otp_rsrc rw = make_rsrc32(wpk, (unsigned)((size_t)P.nN * P.nChunks * WB));

    // the window of window-stage sc: planes of channels CK sc .. CK sc + CK - 1
    auto stage_window = [&](int sc) __attribute__((always_inline)) {
        const int so0 = sc * NPL * P.in_gS, dso = P.in_gS;
#pragma unroll
        for (int j = 0; j < MAXJ; ++j) {
            const int k = wave + 4 * j;
            // (piece outermost: its lane mask - a plane's last piece is partial, lanes past it write nothing - is set once for all the
            //  planes; inside, a plane costs two scalar adds and the DMA instruction)
            if (k < P.NIW && vlive[j]) {
                int so = so0, ld = k * 1024;
                for (int pl = 0; pl < NPL; ++pl, so += dso, ld += PL)
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(rin, (__attribute__((address_space(3))) void*)(smem + ld), 16, voff[j], so, 0, 0);
            }
        }
    };
    // the weights of 16-channel chunk c: global -> registers (under the previous chunk's MFMAs) -> LDS; unit u = tid + 256 j
    otp_u32x4 wr[4];                                                   // (fixed bound, NWJ <= 4: see voff above)
    static_assert(NWJ <= 4, "weight units per thread");
    auto wload = [&](int c) __attribute__((always_inline)) {
        const int wb = (cb * P.nChunks + c) * WB;
#pragma unroll
        for (int j = 0; j < NWJ; ++j)
            wr[j] = __builtin_bit_cast(otp_u32x4, __builtin_amdgcn_raw_buffer_load_b128(rw, tid + 256 * j < WU ? (tid + 256 * j) * 16 : OTP_OOB, wb, 0));
    };
    auto wstore = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < NWJ; ++j)
            if (tid + 256 * j < WU) *reinterpret_cast<otp_u32x4*>(wl + (tid + 256 * j) * 16) = wr[j];
    };
    stage_window(0);
    wload(0);
    HSTAMP(1);

    // ---- per pixel tile: fragment address, lane offsets into the output / residual images --------------------------------------
    const unsigned obytes = (unsigned)((size_t)P.N * P.out_imgB - P.out_base);
    const otp_rsrc ro = make_rsrc32(out + P.out_base, obytes);
    const otp_rsrc rr = make_rsrc32(res ? res + P.res_base : xs, res ? (unsigned)((size_t)P.N * P.res_imgB - P.res_base) : 0u);
    const otp_rsrc rsh = make_rsrc32(shift ? shift : reinterpret_cast<const float*>(xs), shift ? (unsigned)(P.Cout * 4) : 0u);
    int pb[NPT], toff[OTP_S8_KS], offO[NPT], offR[NPT], ch0[NTW];
    otp_f32x4 acc[NTW][NPT];
    {
#pragma unroll
        for (int s = 0; s < OTP_S8_KS; ++s) {
            const int q = 4 * s + kl;
            int tap = q >> 1;
            if (tap > 8) tap = 8;                                  // zero weights: any finite data
            const int dy = tap / 3, dx = tap - dy * 3;
            // record of the tap relative to the pixel's record of tap row dy = 0 (stride 2: parity de-interleaved virtual rows)
            const int rx = STRIDE == 1 ? dx - x0 : (dx == 0 ? 0 : (dx == 1 ? P.Wo + 1 : 1));
            toff[s] = (otp_mul24(dy, P.W1) + rx) * 16 + (q & 1) * PL;
        }
        otp_f32x4 sh[NTW];
#pragma unroll
        for (int t = 0; t < NTW; ++t) {
            ch0[t] = otp_row2ch(co_blk, t, 4 * kl, NTW, P.Cout);
            sh[t] = __builtin_bit_cast(otp_f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsh, co_blk + 16 * t < P.Cout ? ch0[t] * 4 : OTP_OOB, 0, 0));
        }
#pragma unroll
        for (int p = 0; p < NPT; ++p) {
            int m = (wave * NPT + p) * 16 + i16;
            const bool pv = P0 + m < P.total;
            if (!pv) m = P.total - 1 - P0;                         // tail tile: a finite address, the result is dropped
            const int q = p0 + m;
            const int dn = (int)otp_magic_div((uint32_t)q, P.mHWo), pi = q - otp_mul24(dn, P.HWo);
            const int y = (int)otp_magic_div((uint32_t)pi, P.mWo), x = pi - otp_mul24(y, P.Wo);
            pb[p] = (otp_mul24(otp_mul24(n0 + dn, P.VR) + STRIDE * y - Vf, P.W1) + x) * 16;
            offO[p] = pv ? (n0 + dn) * P.out_imgB + otp_mul24(pi, P.out_pS) : OTP_OOB;
            offR[p] = (pv && res) ? (n0 + dn) * P.res_imgB + otp_mul24(pi, P.res_pS) : OTP_OOB;
#pragma unroll
            for (int t = 0; t < NTW; ++t) acc[t][p] = sh[t] * P.pre;
        }
    }

    // One 16-channel chunk: NBLK (k-step, pixel tile) blocks of NTW MFMAs; B fragments are read two blocks ahead (ring of three),
    // the weight fragments of the next k-step two blocks before it starts (csrc/convs.hip)
    auto mfma_phase = [&](int sub) __attribute__((always_inline)) {
        const unsigned char* win = smem + sub * 2 * PL;            // the two planes of this chunk
        typename T::x8 a[2][NTW], b[3];
        auto load_a = [&](int ab, int s) __attribute__((always_inline)) {
#pragma unroll
            for (int t = 0; t < NTW; ++t) {
                if (s < OTP_S8_KS - 1) {
                    a[ab][t] = *reinterpret_cast<const typename T::x8*>(wl + (s * NTW + t) * 1024 + lane * 16);
                } else {
                    // last k-step: k-slots 16, 17 (tap 8) on the lanes kl = 0, 1; kl = 2, 3 multiply zeros (not stored)
                    const typename T::x8 h = *reinterpret_cast<const typename T::x8*>(wl + (OTP_S8_KS - 1) * NTW * 1024 + t * 512 + (lane & 31) * 16);
                    const typename T::x8 z = __builtin_bit_cast(typename T::x8, (otp_u32x4){0u, 0u, 0u, 0u});
                    a[ab][t] = upper ? z : h;
                }
            }
        };
        auto load_b = [&](int bb, int blk) __attribute__((always_inline)) {
            b[bb] = *reinterpret_cast<const typename T::x8*>(win + (pb[blk % NPT] + toff[blk / NPT]));
        };
        load_a(0, 0);
        load_b(0, 0);
        if (NBLK > 1) load_b(1, 1);
#pragma unroll
        for (int blk = 0; blk < NBLK; ++blk) {
            const int s = blk / NPT, p = blk % NPT, cur = blk % 3, sa = s & 1;
            const bool nb = blk + 2 < NBLK;
            const bool na = (NPT >= 2 ? p == NPT - 2 : true) && s + 1 < OTP_S8_KS;
            if (nb) load_b((blk + 2) % 3, blk + 2);
            if (na) load_a(sa ^ 1, s + 1);
#pragma unroll
            for (int t = 0; t < NTW; ++t) acc[t][p] = T::mfma(a[sa][t], b[cur], acc[t][p]);
            if (!nb && !na) hblock_sched<NTW, 0>();
            else if (nb && na) hblock_sched<NTW, 1 + NTW>();
            else if (na) hblock_sched<NTW, NTW>();
            else hblock_sched<NTW, 1>();
            __builtin_amdgcn_sched_barrier(0);
        }
    };

    HSTAMP(2);
    const int nStages = P.C / P.CK;
    for (int sc = 0; sc < nStages; ++sc) {
        if (sc > 0) {
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();                          // every wave is done with the previous window (and weight chunk)
            asm volatile("" ::: "memory");
            stage_window(sc);
            wload(sc * SUB);
        }
        for (int sub = 0; sub < SUB; ++sub) {
            if (sub > 0) {
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();                      // every wave is done with the previous chunk's weight image
                asm volatile("" ::: "memory");
            } else {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's pieces of the window (and its weight units) have landed
            }
            if (sc == 0 && sub < 3) HSTAMP(3 + 4 * sub);
            wstore();
            asm volatile("" ::: "memory");
            if (sub + 1 < SUB) wload(sc * SUB + sub + 1);          // the next chunk's weights fly under this chunk's MFMAs
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();                          // the weight image (and everybody's window pieces) are in the LDS
            asm volatile("" ::: "memory");
            if (sc == 0 && sub < 3) HSTAMP(4 + 4 * sub);
            mfma_phase(sub);
            if (sc == 0 && sub < 3) HSTAMP(5 + 4 * sub);
        }
    }
    HSTAMP(16);

    // ---- epilogue ---------------------------------------------------------------------------------------------------------------
    // (the residual records are loaded here, not held across the chunk loop: 24 registers less is a fourth workgroup per CU, and
    //  another workgroup's MFMAs cover the round trip)
    otp_u32x4 rres[(NTW + 1) / 2][NPT];
    constexpr bool load_res = MODE == 2;                           // (a template variant: the plain form carries no residual loads / adds)
#pragma unroll
    for (int t = 0; load_res && t < NTW; t += 2) {
        const bool tav = ch0[t] < P.Cout;                          // (per lane: Cout % 8 == 0, a lane's record exists or does not)
        const int go = otp_mul24(ch0[t] >> 3, P.res_gS);
        if (otp_tile_paired(co_blk, t, NTW, P.Cout)) {
#pragma unroll
            for (int p = 0; p < NPT; ++p)
                rres[t >> 1][p] = __builtin_bit_cast(otp_u32x4, __builtin_amdgcn_raw_buffer_load_b128(
                    rr, (tav && offR[p] != OTP_OOB) ? offR[p] + go : OTP_OOB, 0, 0));
        } else {
            const int half = (ch0[t] >> 2) & 1;
#pragma unroll
            for (int p = 0; p < NPT; ++p) {
                const otp_u32x2 h = __builtin_bit_cast(otp_u32x2, __builtin_amdgcn_raw_buffer_load_b64(
                    rr, (tav && offR[p] != OTP_OOB) ? offR[p] + go + 8 * half : OTP_OOB, 0, 0));
                rres[t >> 1][p] = (otp_u32x4){h[0], h[1], 0u, 0u};
            }
        }
    }
    HSTAMP(17);
    if constexpr (T::training) {
        // training form (csrc/nhwc_conv.hip's contract): out = bf16(conv + bias); the per-tile channel sums / sums of squares are those of
        // the ROUNDED values (what BatchNorm will normalise); a residual is added to the rounded result and the sum rounded again -
        // bit for bit a separate bf16 add.  Sums: 16 lanes of a DPP row hold the 16 pixels of a tile -> row sum -> the four waves'
        // partials through the LDS behind the weight image, added in a fixed order.
        constexpr int CB = NTW * 16;
        float* sred = reinterpret_cast<float*>(wl + WB);               // [4 waves][2][CB]
#pragma unroll
        for (int t = 0; t < NTW; t += 2) {
            const bool paired = otp_tile_paired(co_blk, t, NTW, P.Cout);       // (uniform)
            const int t1 = t + 1 < NTW ? t + 1 : t;
            const bool tav = ch0[t] < P.Cout;                          // (per lane)
            const int go = otp_mul24(ch0[t] >> 3, P.out_gS);
            float s1[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, s2[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int p = 0; p < NPT; ++p) {
                float f[8] = {acc[t][p][0], acc[t][p][1], acc[t][p][2], acc[t][p][3], paired ? acc[t1][p][0] : 0.f,
                              paired ? acc[t1][p][1] : 0.f, paired ? acc[t1][p][2] : 0.f, paired ? acc[t1][p][3] : 0.f};
                otp_u32x4 rec = T::pack8(f);
                const bool pv = offO[p] != OTP_OOB;
                if constexpr (MODE != 0) {
                    const otp_f32x2 w0 = T::widen(rec[0]), w1 = T::widen(rec[1]), w2 = T::widen(rec[2]), w3 = T::widen(rec[3]);
                    float fr[8] = {w0.x, w0.y, w1.x, w1.y, w2.x, w2.y, w3.x, w3.y};
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const float v = pv ? fr[e] : 0.f;
                        s1[e] += v;
                        s2[e] += v * v;
                    }
                    if constexpr (MODE == 2) {
                        const otp_u32x4 rq = rres[t >> 1][p];
                        const otp_f32x2 r0 = T::widen(rq[0]), r1 = T::widen(rq[1]), r2 = T::widen(rq[2]), r3 = T::widen(rq[3]);
                        float g[8] = {fr[0] + r0.x, fr[1] + r0.y, fr[2] + r1.x, fr[3] + r1.y, fr[4] + r2.x, fr[5] + r2.y, fr[6] + r3.x, fr[7] + r3.y};
                        rec = T::pack8(g);
                    }
                }
                if (paired) {
                    __builtin_amdgcn_raw_buffer_store_b128(rec, ro, (tav && pv) ? offO[p] + go : OTP_OOB, 0, 0);
                } else {
                    const int half = (ch0[t] >> 2) & 1;
                    __builtin_amdgcn_raw_buffer_store_b64((otp_u32x2){rec[0], rec[1]}, ro, (tav && pv) ? offO[p] + go + 8 * half : OTP_OOB, 0, 0);
                }
            }
            if constexpr (MODE == 1) {
                const int cl = ch0[t] - co_blk;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    if (e < 4 || paired) {
                        const float a = otp_row16_sum(s1[e]), b = otp_row16_sum(s2[e]);
                        if (i16 == 0) {
                            sred[(wave * 2 + 0) * CB + cl + e] = a;
                            sred[(wave * 2 + 1) * CB + cl + e] = b;
                        }
                    }
                }
            }
        }
        if constexpr (MODE == 1) {
            __syncthreads();
            for (int i = tid; i < 2 * CB; i += 256) {
                const int which = i / CB, c = i - which * CB, co = co_blk + c;
                if (co < P.Cout) {
                    float v = 0.f;
#pragma unroll
                    for (int w = 0; w < 4; ++w) v += sred[(w * 2 + which) * CB + c];
                    P.stats[((size_t)tile * 2 + which) * P.Cout + co] = v;
                }
            }
        }
    } else {
        bool bad = false;
#pragma unroll
        for (int t = 0; t < NTW; t += 2) {
            const bool paired = otp_tile_paired(co_blk, t, NTW, P.Cout);       // (uniform)
            const int t1 = t + 1 < NTW ? t + 1 : t;
            const bool tav = ch0[t] < P.Cout;                          // (per lane)
            const int go = otp_mul24(ch0[t] >> 3, P.out_gS);
#pragma unroll
            for (int p = 0; p < NPT; ++p) {
                const otp_u32x4 rq = load_res ? rres[t >> 1][p] : (otp_u32x4){0u, 0u, 0u, 0u};
                const otp_f32x2 r0 = T::widen(rq[0]), r1 = T::widen(rq[1]), r2 = T::widen(rq[2]), r3 = T::widen(rq[3]);
                float f[8] = {acc[t][p][0] * P.post + r0.x, acc[t][p][1] * P.post + r0.y, acc[t][p][2] * P.post + r1.x,
                              acc[t][p][3] * P.post + r1.y,
                              paired ? acc[t1][p][0] * P.post + r2.x : 0.f, paired ? acc[t1][p][1] * P.post + r2.y : 0.f,
                              paired ? acc[t1][p][2] * P.post + r3.x : 0.f, paired ? acc[t1][p][3] * P.post + r3.y : 0.f};
#pragma unroll
                for (int e = 0; e < 8; ++e) bad |= otp_out_of_range(f[e]);
                if (P.act == OTP_ACT_RELU) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) f[e] = otp_relu(f[e]);
                }
                const otp_u32x4 rec = T::pack8(f);
                if (paired) {
                    __builtin_amdgcn_raw_buffer_store_b128(rec, ro, (tav && offO[p] != OTP_OOB) ? offO[p] + go : OTP_OOB, 0, 0);
                } else {
                    const int half = (ch0[t] >> 2) & 1;
                    __builtin_amdgcn_raw_buffer_store_b64((otp_u32x2){rec[0], rec[1]}, ro, (tav && offO[p] != OTP_OOB) ? offO[p] + go + 8 * half : OTP_OOB,
                                                          0, 0);
                }
            }
        }
        otp_range_report(P.rflag, bad, OTP_RANGE_H16);
    }
    HSTAMP(19);
#ifdef OTP_H16_TIMING
    if (threadIdx.x == 0 && blockIdx.x < 8192) otp_h16_stamps[blockIdx.x * 32 + 31] = __builtin_amdgcn_s_memrealtime();
#endif
}

inline int h16_ntw(int Cout) { return otp_hb_ntw(Cout); }

inline int h16_window_records(const HPlan& P, int bm, int stride) {
    int NV = 0;
    for (int t = 0; t < P.nTiles; ++t) {
        const int a = t * bm, b = (a + bm < P.total ? a + bm : P.total) - 1;
        const int na = a / P.HWo, ya = (a % P.HWo) / P.Wo, xa = (a % P.HWo) % P.Wo;
        const int nb = b / P.HWo, yb = (b % P.HWo) / P.Wo, xb = (b % P.HWo) % P.Wo;
        int v;
        if (stride == 1) {
            const int rows = (nb * P.VR + yb + 1) - (na * P.VR + ya);   // virtual rows between the window's first and the last pixel's
            v = (rows + 1) * P.W1 + xb - xa + 3;
        } else {
            const int rows = (nb * P.VR + 2 * yb + 2) - (na * P.VR + 2 * ya) + 1;
            v = rows * P.W1;
        }
        if (v > NV) NV = v;
    }
    return NV;
}

// nhwc: the tensors are NHWC with exactly Cin / Cout channels (csrc/hb.hip: HPlan's strides are those of 2-byte NHWC elements);
// otherwise H8 images, channel-group slices from the descriptor
template <typename T>
bool h16_conv_plan(const otp_h16_conv_desc& d, HPlan& P, bool nhwc = false) {
    if (d.stride != 1 && d.stride != 2) return false;
    if (d.N <= 0 || d.Cin <= 0 || d.Cout <= 0 || d.H <= 0 || d.W <= 0) return false;
    if (d.Cin % 16 || d.Cout % 8 || (d.act != OTP_ACT_NONE && d.act != OTP_ACT_RELU)) return false;
    if (d.stride == 2 && ((d.H & 1) || (d.W & 1))) return false;
    const int S = d.stride, Ho = d.H / S, Wo = d.W / S;
    P.N = d.N; P.C = d.Cin; P.H = d.H; P.W = d.W; P.HW = d.H * d.W; P.Ho = Ho; P.Wo = Wo; P.HWo = Ho * Wo; P.Cout = d.Cout;
    P.total = d.N * P.HWo;
    const int in_gtot = d.in_gtot > 0 ? d.in_gtot : d.Cin / 8, in_goff = d.in_gtot > 0 ? d.in_goff : 0;
    const int out_gtot = d.out_gtot > 0 ? d.out_gtot : d.Cout / 8, out_goff = d.out_gtot > 0 ? d.out_goff : 0;
    const int res_gtot = d.res_gtot > 0 ? d.res_gtot : d.Cout / 8, res_goff = d.res_gtot > 0 ? d.res_goff : 0;
    if (in_goff < 0 || in_goff + d.Cin / 8 > in_gtot || out_goff < 0 || out_goff + d.Cout / 8 > out_gtot || res_goff < 0 ||
        res_goff + d.Cout / 8 > res_gtot)
        return false;
    if ((size_t)in_gtot * P.HW * 16 >= (1ull << 31) || (size_t)out_gtot * P.HWo * 16 >= (1ull << 31) || (size_t)res_gtot * P.HWo * 16 >= (1ull << 31))
        return false;
    if (nhwc) {
        if (d.in_gtot > 0 || d.out_gtot > 0 || d.res_gtot > 0) return false;
        P.in_pS = d.Cin * 2; P.in_gS = 16; P.in_imgB = P.HW * d.Cin * 2; P.in_base = 0;
        P.out_pS = P.res_pS = d.Cout * 2; P.out_gS = P.res_gS = 16; P.out_imgB = P.res_imgB = P.HWo * d.Cout * 2;
        P.out_base = P.res_base = 0;
    } else {
        P.in_pS = 16; P.in_gS = P.HW * 16; P.in_imgB = in_gtot * P.HW * 16; P.in_base = (size_t)in_goff * P.HW * 16;
        P.out_pS = 16; P.out_gS = P.HWo * 16; P.out_imgB = out_gtot * P.HWo * 16; P.out_base = (size_t)out_goff * P.HWo * 16;
        P.res_pS = 16; P.res_gS = P.HWo * 16; P.res_imgB = res_gtot * P.HWo * 16; P.res_base = (size_t)res_goff * P.HWo * 16;
    }
    P.stats = nullptr;
    P.act = d.act;
    P.post = d.out_scale > 0.f ? d.out_scale : 1.f;
    P.pre = 1.f / P.post;
    P.NTW = h16_ntw(d.Cout);
    P.nN = ((d.Cout + 15) / 16 + P.NTW - 1) / P.NTW;
    P.nChunks = d.Cin / 16;
    P.VR = d.H + 1;
    P.W1 = d.W + 1;
    const int maxrec = S == 1 ? 512 : 1024;                        // 2 / 4 pieces of 64 records per wave and plane
    // the pixel tile: 256 pixels, or 128 for launches that would leave the CUs with fewer than three workgroups each; smaller while
    // the window planes do not fit.
    bool found = false;
    int npt0 = 4;
    if (const char* e = getenv("OTPOSE_H16_NPT")) {                // development override of the largest pixel tile (1 / 2 / 4)
        const int v = atoi(e);
        if (v == 1 || v == 2 || v == 4) npt0 = v;
    }
    for (int npt = npt0; npt >= 1; npt >>= 1) {
        const int bm = 64 * npt;
        P.NPT = npt;
        P.nTiles = (P.total + bm - 1) / bm;
        const int NV = h16_window_records(P, bm, S);
        if (NV > maxrec) continue;
        const size_t st = (size_t)2 * NV * 16 + hwb(P.NTW) + hsred<T>(P.NTW);   // the smallest stage: 16 channels
        if (st > 80 * 1024) continue;
        P.NV = NV;
        found = true;
        if ((long)P.nTiles * P.nN >= 3 * 256 || npt == 1) break;
    }
    if (!found) return false;
    {
        const int bm = 64 * P.NPT;
        P.nTiles = (P.total + bm - 1) / bm;
        P.NV = h16_window_records(P, bm, S);
        if (P.NV > maxrec) return false;
    }
    P.pl = P.NV * 16;
    // channels per window stage: the largest multiple of 16 dividing Cin whose planes + one weight chunk let three workgroups share a
    // CU's 160 KB (two when nothing else fits) - one HBM round trip per CK channels
    {
        const size_t wbytes = hwb(P.NTW) + hsred<T>(P.NTW);
        int best = 0;
        for (size_t budget : {(size_t)(160 * 1024) / 3, (size_t)80 * 1024, (size_t)160 * 1024}) {
            for (int ck = 96; ck >= 16 && !best; ck -= 16)
                if (d.Cin % ck == 0 && (size_t)(ck / 8) * P.pl + wbytes <= budget) best = ck;
            if (best) break;
        }
        if (!best) return false;
        P.CK = best;
        if (const char* e = getenv("OTPOSE_H16_CK")) {             // development override
            const int v = atoi(e);
            if (v >= 16 && v <= 96 && v % 16 == 0 && d.Cin % v == 0 && (size_t)(v / 8) * P.pl + wbytes <= 160 * 1024) P.CK = v;
        }
    }
    P.tpx = (P.nTiles + 7) / 8;
    P.NIW = (P.NV + 63) / 64;
    P.mHWo = otp_magic(P.HWo); P.mWo = otp_magic(Wo); P.mW1 = otp_magic(P.W1); P.mVR = otp_magic(P.VR);
    // exactness of the magic divisions (numerator * divisor < 2^32) and 31-bit byte offsets
    if ((long)(P.HWo + 256) * P.HWo >= (1l << 32) || (long)P.HWo * Wo >= (1l << 32)) return false;
    if ((long)(d.N + 2) * P.VR * P.VR >= (1l << 32) || (long)(maxrec + d.W + 2) * P.W1 >= (1l << 32)) return false;
    if ((long)P.in_imgB * 20 >= (1l << 31)) return false;                 // a tile spans few images: per-lane offsets stay 31-bit
    if ((size_t)d.N * P.out_imgB >= (1ull << 31) || (size_t)d.N * P.res_imgB >= (1ull << 31)) return false;
    if ((size_t)P.nN * P.nChunks * hwb(P.NTW) >= (1ull << 31)) return false;
    if (P.HWo < 16) return false;
    // operands of the 24-bit multiplies of the kernel's index arithmetic (otp_mul24)
    if (P.HW >= (1 << 24) || (long)(d.N + 2) * P.VR >= (1l << 24) || (long)(maxrec + 2 * d.W + 8) >= (1l << 24) ||
        (long)(d.N + 2) * P.VR * 2 + 2 * d.H >= (1l << 24) || P.in_pS >= (1 << 24) || P.out_pS >= (1 << 24) || P.in_gS >= (1 << 24) ||
        P.out_gS >= (1 << 24) || d.Cout / 8 >= (1 << 24))
        return false;
    // images a tile's window may touch: (n - n0) * imgB must stay below 2^31
    {
        const long span = (long)(64 * P.NPT) / P.HWo + 2;
        if (span * P.in_imgB >= (1l << 31)) return false;
    }
    return true;
}

template <typename T, int NTW, int NPT, int STRIDE, int MODE>
int h16_conv_launch(const void* xs, const void* wpk, const float* shift, const void* res, void* out, const HPlan& P, hipStream_t st) {
    auto kern = h16_conv3x3_kernel<T, NTW, NPT, STRIDE, MODE>;
    const size_t need = (size_t)(P.CK / 8) * P.pl + hwb(NTW) + hsred<T>(NTW);
    OTP_ALLOW_BIG_LDS(kern, need);
    hipLaunchKernelGGL(kern, dim3(8 * P.tpx * P.nN), dim3(256), need, st, static_cast<const unsigned char*>(xs),
                       static_cast<const unsigned char*>(wpk), shift, static_cast<const unsigned char*>(res),
                       static_cast<unsigned char*>(out), P);
    return otp_launch_status();
}

// NTW {2, 3} x NPT {4, 2, 1} x stride {1, 2} x MODE {0, 2; training: 1 when the plan carries a statistics buffer}
template <typename T>
int h16_conv_dispatch(const void* xs, const void* wpk, const float* fs, const void* res, void* out, const HPlan& P, int stride,
                      hipStream_t st) {
#define OTP_H16_GO(NTW_, NPT_, S_)                                                                          \
    {                                                                                                       \
        if constexpr (T::training)                                                                          \
            if (P.stats) return h16_conv_launch<T, NTW_, NPT_, S_, 1>(xs, wpk, fs, res, out, P, st);        \
        return res ? h16_conv_launch<T, NTW_, NPT_, S_, 2>(xs, wpk, fs, res, out, P, st)                    \
                   : h16_conv_launch<T, NTW_, NPT_, S_, 0>(xs, wpk, fs, res, out, P, st);                   \
    }
#define OTP_H16_NPT(NPT_, S_)                                  \
    if (P.NPT == NPT_) {                                       \
        if (P.NTW == 2) OTP_H16_GO(2, NPT_, S_);               \
        OTP_H16_GO(3, NPT_, S_);                               \
    }
    if (stride == 1) {
        OTP_H16_NPT(4, 1)
        OTP_H16_NPT(2, 1)
        OTP_H16_NPT(1, 1)
    } else {
        OTP_H16_NPT(4, 2)
        OTP_H16_NPT(2, 2)
        OTP_H16_NPT(1, 2)
    }
#undef OTP_H16_NPT
#undef OTP_H16_GO
    return OTP_ERR_UNSUPPORTED;
}

// ================================================================================================================================
// 1x1 convolution on H8 records: out = act(W . x + shift (+ res)), H8 (+ H8 residual) -> H8, or -> a channel slice of fp32 NCHW
// ================================================================================================================================
// Register-resident input (csrc/pointx.hip's design, minus the split): a wave owns 32 flattened pixels and holds their Cin
// channels as B-operand fragments - lane (pixel i16 of tile h, kq) loads record (group 4 ks + kq, pixel) straight from global
// memory, 16 bytes, no conversion; the weights stream through the LDS in blocks of one cout-tile pair (32 output channels: 2 KS
// KB, LDS-DMA, double buffered); a pair's two 16 x 16 results per pixel tile are 8 consecutive channels per lane = one record.
// (csrc/hb.hip: the same kernel on bfloat16 NHWC tensors - the TransformerBlock MLP's two projections and their input gradients in
//  the training step, reached through csrc/nhwc_conv.hip's otp_nhwc_conv_* - with the bias as a separate fp32 vector.)
struct HPw {
    const unsigned char* x;
    const unsigned char* packed;
    const unsigned char* res;
    unsigned char* out;
    const float* shift;                                           // Cout floats or NULL
    int total, HW, Cin, Cout, nblk, relu, f32out;
    // record (image n, channel group g, pixel p) of a tensor: base + n imgB + g gS + p pS bytes (see HPlan)
    size_t x_imgB, x_gS, x_pS, x_base, r_imgB, r_gS, r_pS, r_base, o_imgB, o_gS, o_pS, o_base;
    int o_tot, o_off;                                             // fp32 NCHW output: channels of the tensor / first channel
    float post;
    unsigned* rflag;
    float* stats;                                                 // training: per-tile channel sums [tiles of 128 pixels][2][Cout] of the stored values, or NULL
    otp_hbpw_epi epi;                                             // training: the MLP epilogues (csrc/hb.h); mode 0: none
};

constexpr int HPW_MAXC = 1024;            // shift table: output channels
// KS k-steps of 32 input channels (Cin padded with zero weights and masked loads); a weight block = one tile pair x KS x 1 KB each
// = 2 KS KB, rounded up to whole 4 KB passes of the 256 threads
__host__ __device__ constexpr int hpw_blkb(int KS) { return otp_hbpw_blkb(KS); }

// EPI (training only; compile time, so that the plain form keeps its registers - as run-time branches the two MLP epilogues cost
// the projections 19 registers and 41 -> 58 us): 0 plain, 1 per-tile channel statistics, 2 / 3 the MLP epilogues of csrc/hb.h
template <typename T, int KS, int EPI = 0>
__global__ __launch_bounds__(256, KS <= 4 ? 4 : (KS <= 8 ? 3 : 2)) void h16_pointwise_kernel(HPw A) {
    constexpr int BLKB = hpw_blkb(KS);
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];     // 2 BLKB + HPW_MAXC * 4 (+ training: 4 waves x 2 x 32 floats, twice)
    float* shl = reinterpret_cast<float*>(lds + 2 * BLKB);
    float* sred = shl + HPW_MAXC;                                            // (training, EPI 1) [2 buffers][4 waves][2][32]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, kq = lane >> 4, n16 = lane & 15;
    otp_lds_stage<256, BLKB>(A.packed, lds);
    for (int i = tid; i < HPW_MAXC; i += 256) shl[i] = (A.shift && i < A.Cout) ? A.shift[i] : 0.f;
    // the lane's two pixels (tile h: flattened pixel base + 16 h + n16), their image and in-image index
    int img[2], pix[2];
    bool pv[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        int P = (int)blockIdx.x * 128 + wave * 32 + 16 * h + n16;
        pv[h] = P < A.total;
        if (!pv[h]) P = A.total - 1;
        img[h] = P / A.HW;                                                     // (exact: P * HW may pass 2^32, twice per lane)
        pix[h] = P - img[h] * A.HW;
    }
    const int Gin = A.Cin >> 3;
    otp_u32x4 X[KS][2];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int g = 4 * ks + kq;
            const bool live = g < Gin;                                         // groups past Cin: zero operands (and zero weights)
            const otp_u32x4* src = reinterpret_cast<const otp_u32x4*>(A.x + A.x_base + img[h] * A.x_imgB + (live ? g : 0) * A.x_gS + pix[h] * A.x_pS);
            const otp_u32x4 v = *src;
            X[ks][h] = live ? v : (otp_u32x4){0u, 0u, 0u, 0u};
        }
    const float lo_clamp = A.relu ? 0.f : -__builtin_inff();
    bool bad = false;
    __syncthreads();                                   // weight block 0 and the shift table landed
#pragma unroll 1
    for (int blk = 0; blk < A.nblk; ++blk) {
        // (the last trip re-stages block 0, which nobody reads: every wave issues the same instructions on every trip)
        otp_lds_stage<256, BLKB>(A.packed + (size_t)(blk + 1 < A.nblk ? blk + 1 : 0) * BLKB, lds + ((blk + 1) & 1) * BLKB);
        asm volatile("" ::: "memory");
        const unsigned char* Pw = lds + (blk & 1) * BLKB;
        const int c8 = 32 * blk + 8 * kq;                                     // the lane's 8 output channels of this block
        const bool cl = c8 < A.Cout;
        otp_u32x4 rq[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            rq[h] = (otp_u32x4){0u, 0u, 0u, 0u};
            if (A.res && cl && pv[h])
                rq[h] = *reinterpret_cast<const otp_u32x4*>(A.res + A.r_base + img[h] * A.r_imgB + (c8 >> 3) * A.r_gS + pix[h] * A.r_pS);
        }
        otp_f32x4 acc[2][2];                                                       // [tile of the pair][pixel tile]
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            otp_f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                const typename T::x8 aw = *reinterpret_cast<const typename T::x8*>(Pw + (m * KS + ks) * 1024 + lane * 16);
                a0 = T::mfma(aw, __builtin_bit_cast(typename T::x8, X[ks][0]), a0);
                a1 = T::mfma(aw, __builtin_bit_cast(typename T::x8, X[ks][1]), a1);
            }
            acc[m][0] = a0;
            acc[m][1] = a1;
        }
        const otp_f32x4 sh0 = *reinterpret_cast<const otp_f32x4*>(shl + (c8 & (HPW_MAXC - 1)));
        const otp_f32x4 sh1 = *reinterpret_cast<const otp_f32x4*>(shl + ((c8 + 4) & (HPW_MAXC - 1)));
        float st1[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, st2[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const otp_f32x2 r0 = T::widen(rq[h][0]), r1 = T::widen(rq[h][1]), r2 = T::widen(rq[h][2]), r3 = T::widen(rq[h][3]);
            // eval: post * sum + shift + residual in fp32; training: sum + bias
            float f[8];
            if constexpr (T::training) {
                f[0] = acc[0][h][0] + sh0[0], f[1] = acc[0][h][1] + sh0[1], f[2] = acc[0][h][2] + sh0[2], f[3] = acc[0][h][3] + sh0[3];
                f[4] = acc[1][h][0] + sh1[0], f[5] = acc[1][h][1] + sh1[1], f[6] = acc[1][h][2] + sh1[2], f[7] = acc[1][h][3] + sh1[3];
            } else {
                f[0] = acc[0][h][0] * A.post + sh0[0] + r0.x, f[1] = acc[0][h][1] * A.post + sh0[1] + r0.y;
                f[2] = acc[0][h][2] * A.post + sh0[2] + r1.x, f[3] = acc[0][h][3] * A.post + sh0[3] + r1.y;
                f[4] = acc[1][h][0] * A.post + sh1[0] + r2.x, f[5] = acc[1][h][1] * A.post + sh1[1] + r2.y;
                f[6] = acc[1][h][2] * A.post + sh1[2] + r3.x, f[7] = acc[1][h][3] * A.post + sh1[3] + r3.y;
            }
            if constexpr (T::training) {
                if (A.res) {
                    // csrc/nhwc_conv.hip's contract: the residual is added to the ROUNDED result and the sum rounded again (a separate bf16 add)
                    const otp_u32x4 q = T::pack8((const float(&)[8])f);
                    const otp_f32x2 w0 = T::widen(q[0]), w1 = T::widen(q[1]), w2 = T::widen(q[2]), w3 = T::widen(q[3]);
                    const float g[8] = {w0.x, w0.y, w1.x, w1.y, w2.x, w2.y, w3.x, w3.y};
                    const float rr[8] = {r0.x, r0.y, r1.x, r1.y, r2.x, r2.y, r3.x, r3.y};
#pragma unroll
                    for (int e = 0; e < 8; ++e) f[e] = g[e] + rr[e];
                }
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                bad |= otp_out_of_range(f[e]);
                f[e] = fmaxf(f[e], lo_clamp);
            }
            if constexpr (EPI == 3) {
                // input gradient of the MLP's down-projection: times gelu'(pre-activation) and the dropout factor of the forward
                const size_t eo = A.o_base + img[h] * A.o_imgB + (c8 >> 3) * A.o_gS + pix[h] * A.o_pS;
                const bool lv = cl && pv[h];
                const otp_u32x4 hq = lv ? *reinterpret_cast<const otp_u32x4*>(static_cast<const unsigned char*>(A.epi.aux) + eo) : (otp_u32x4){0u, 0u, 0u, 0u};
                const unsigned bits = lv ? A.epi.keep[eo >> 4] : 0u;
                const otp_f32x2 h0 = T::widen(hq[0]), h1 = T::widen(hq[1]), h2 = T::widen(hq[2]), h3 = T::widen(hq[3]);
                const float hv[8] = {h0.x, h0.y, h1.x, h1.y, h2.x, h2.y, h3.x, h3.y};
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float x = hv[e];
                    const float d = otp_phi_fast(x) + x * 0.39894228040143267794f * __expf(-0.5f * x * x);
                    f[e] = ((bits >> e) & 1u) ? f[e] * A.epi.scale * d : 0.f;
                }
            }
            if constexpr (EPI == 1) {
                // per-tile channel sums of the ROUNDED values (csrc/nhwc_conv.hip's contract: what BatchNorm will normalise): the 16 lanes of
                // a DPP row hold 16 pixels of the lane's 8 channels
                const otp_u32x4 qv = T::pack8((const float(&)[8])f);
                const otp_f32x2 w0 = T::widen(qv[0]), w1 = T::widen(qv[1]), w2 = T::widen(qv[2]), w3 = T::widen(qv[3]);
                const float g[8] = {w0.x, w0.y, w1.x, w1.y, w2.x, w2.y, w3.x, w3.y};
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float v = pv[h] ? g[e] : 0.f;
                    st1[e] += v;
                    st2[e] += v * v;
                }
            }
            if (cl && pv[h]) {
                if (A.f32out) {
                    float* o = reinterpret_cast<float*>(A.out) + ((size_t)img[h] * A.o_tot + A.o_off + c8) * A.HW + pix[h];
#pragma unroll
                    for (int e = 0; e < 8; ++e)
                        if (c8 + e < A.Cout) o[(size_t)e * A.HW] = f[e];
                } else {
                    const size_t eo = A.o_base + img[h] * A.o_imgB + (c8 >> 3) * A.o_gS + pix[h] * A.o_pS;
                    const otp_u32x4 rec = T::pack8(f);
                    *reinterpret_cast<otp_u32x4*>(A.out + eo) = rec;
                    if constexpr (EPI == 2) {
                        // dropout(gelu(.)) of the ROUNDED result (what a separate pass over the stored tensor computes), one rounding
                        const otp_f32x2 w0 = T::widen(rec[0]), w1 = T::widen(rec[1]), w2 = T::widen(rec[2]), w3 = T::widen(rec[3]);
                        const float hv[8] = {w0.x, w0.y, w1.x, w1.y, w2.x, w2.y, w3.x, w3.y};
                        const unsigned bits = otp_drop_keep8(eo >> 4, A.epi.s0, A.epi.s1, A.epi.thr);
                        float g[8];
#pragma unroll
                        for (int e = 0; e < 8; ++e) g[e] = ((bits >> e) & 1u) ? hv[e] * otp_phi_fast(hv[e]) * A.epi.scale : 0.f;
                        *reinterpret_cast<otp_u32x4*>(static_cast<unsigned char*>(A.epi.out2) + eo) = T::pack8(g);
                        A.epi.keep[eo >> 4] = (unsigned char)bits;
                    }
                }
            }
        }
        if constexpr (EPI == 1) {
            float* sr = sred + (blk & 1) * 256;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float a = otp_row16_sum(st1[e]), b = otp_row16_sum(st2[e]);
                if (n16 == 0) {
                    sr[(wave * 2 + 0) * 32 + 8 * kq + e] = a;
                    sr[(wave * 2 + 1) * 32 + 8 * kq + e] = b;
                }
            }
        }
        // the next block has landed, this block's stores (training: and its partial sums) have left
        if constexpr (T::training) asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        if constexpr (EPI == 1) if (tid < 64) {
            // the four waves' partials in a fixed order; the buffer alternates, so the next block's writes cannot overtake these reads
            const float* sr = sred + (blk & 1) * 256;
            const int which = tid >> 5, c = tid & 31, co = 32 * blk + c;
            if (co < A.Cout)
                A.stats[((size_t)blockIdx.x * 2 + which) * A.Cout + co] =
                    sr[(0 * 2 + which) * 32 + c] + sr[(1 * 2 + which) * 32 + c] + sr[(2 * 2 + which) * 32 + c] + sr[(3 * 2 + which) * 32 + c];
        }
    }
    if constexpr (!T::training) otp_range_report(A.rflag, bad, OTP_RANGE_H16);
    else (void)bad;
}

template <typename T, int KS, int EPI = 0>
int hpw_launch(const HPw& a, hipStream_t st) {
    auto kern = h16_pointwise_kernel<T, KS, EPI>;
    const size_t need = 2 * (size_t)hpw_blkb(KS) + HPW_MAXC * 4 + (T::training ? 2 * 256 * 4 : 0);
    OTP_ALLOW_BIG_LDS(kern, need);
    hipLaunchKernelGGL(kern, dim3((unsigned)((a.total + 127) / 128)), dim3(256), need, st, a);
    return otp_launch_status();
}

}  // namespace
