// fp16-storage eval kernels of the HRNet backbone (BASELINE.json configs[4]: "fp16"; cfg.MODEL.DTYPE = "fp16").
//
// The reference's own native op dispatches half (thirdparty/deform_conv/src/deform_conv_cuda_kernel.cu:719,
// AT_DISPATCH_FLOATING_TYPES_AND_HALF) but its model code never runs below fp32 (no AMP anywhere), so an fp16 forward
// is an extension, validated against the fp32 HIP engine and the oracle with a stated tolerance (tests/test_gpu_h16.py).
// What these kernels compute is model/HRNet.py:116-152 with BatchNorm (eval) folded: conv3x3 (stride 1: BasicBlock :500-530,
// Bottleneck conv2 :551-571, transition :213-229; stride 2: fuse chains :442-470, transitions, stem conv2 :66-72), conv1x1
// (Bottleneck conv1 / conv3, fuse up-sampling paths :426-439, final_layer :108-114), the stem conv (:118-120) and the fuse rows'
// upsample-accumulate (:487-494).
//
// Arithmetic: operands are IEEE half - activations AS STORED, weights rounded once (times a per-layer power of two so small
// BatchNorm-folded weights stay normal numbers) - ONE v_mfma_f32_16x16x32_f16 per product where the fp32 engine spends three
// (csrc/convs.hip), fp32 accumulation, shift / residual / ReLU in fp32, one rounding to half per stored value.
//
// Storage: "H8" images.  A logical (N, C, H, W) tensor, C % 8 == 0, is [N][C / 8][H * W] records of 16 bytes = the 8 halves of
// channels 8 g .. 8 g + 7 at pixel p - 2 bytes per element.  A record IS one lane's B operand of a k-slot of the MFMA, a plane
// (n, g) is contiguous in p, so a conv stages its window with the LDS-DMA only (csrc/convs.hip's design with half the planes) and
// a 1x1 conv loads its operand fragments straight from global memory.  (gtot, goff): a tensor may be a range of channel groups
// of a wider H8 tensor - channel concatenations cost nothing.
//
// The 3x3 and 1x1 kernels, their plans and launches are csrc/h16_kernels.h instantiated with the Half traits (csrc/hb.hip holds the
// bfloat16 training instantiation); this file adds the weight packers, the stem, the element-wise H8 passes and the C ABI.
#include "h16_kernels.h"

namespace {

// packed weights: [cout block][chunk][k-step][cout tile][lane] 16-byte A fragments, lane (i16, kl): row i16 of the tile = channel
// otp_row2ch(block, tile, i16), k-slot q = 4 s + kl -> tap q / 2, input channels 16 chunk + 8 (q % 2) .. + 7; the fifth k-step holds
// k-slots 16, 17 only (32 lanes per tile)
__global__ void h16_wpack_kernel(const float* __restrict__ w, const float* __restrict__ scale, otp_u32x4* __restrict__ out, int Cout,
                                 int Cin, int NTW, int nN, int nChunks, float pre) {
    const int total = nN * nChunks * OTP_S8_KS * NTW * 64;
    const int WU = hwb(NTW) / 16;                                   // 16-byte units of one (cout block, chunk) image
    for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gridDim.x * blockDim.x) {
        const int lane = idx & 63;
        int r = idx >> 6;
        const int t = r % NTW; r /= NTW;
        const int s = r % OTP_S8_KS; r /= OTP_S8_KS;
        const int chunk = r % nChunks, cb = r / nChunks;
        const int cout = otp_row2ch(cb * NTW * 16, t, lane & 15, NTW, Cout), kl = lane >> 4;
        const int q = 4 * s + kl, tap = q >> 1, ci0 = chunk * 16 + 8 * (q & 1);
        if (tap > 8) continue;
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int ci = ci0 + j;
            v[j] = (cout < Cout && ci < Cin) ? w[((size_t)cout * Cin + ci) * 9 + tap] * (scale ? scale[cout] : 1.f) * pre : 0.f;
        }
        const size_t base = (size_t)(cb * nChunks + chunk) * WU;
        const size_t o = s < OTP_S8_KS - 1 ? base + (s * NTW + t) * 64 + lane : base + (OTP_S8_KS - 1) * NTW * 64 + t * 32 + lane;
        out[o] = Half::pack8(v);
    }
}

// packed: nblk blocks of [tile of the pair][ks][lane] 16-byte A fragments (rows permuted: row r16 of tile m of pair p = channel
// 32 p + 8 (r16 >> 2) + 4 m + (r16 & 3)), padded to hpw_blkb(KS), then shift[HPW_MAXC] floats, then {post, 0, 0, 0}
__global__ void h16_pw_pack_kernel(const float* __restrict__ w, const float* __restrict__ scale, const float* __restrict__ shift,
                                   unsigned char* __restrict__ packed, int Cin, int Cout, int KS, int nblk, int blkb, float pre) {
    const int units = blkb / 16;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx < nblk * units) {
        const int blk = idx / units, u = idx - blk * units;
        otp_u32x4 o = {0u, 0u, 0u, 0u};
        if (u < 2 * KS * 64) {
            const int frag = u >> 6, lane = u & 63, m = frag / KS, ks = frag - m * KS, r16 = lane & 15, kq = lane >> 4;
            const int row = 32 * blk + 8 * (r16 >> 2) + 4 * m + (r16 & 3);
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int c = 32 * ks + 8 * kq + j;
                v[j] = (row < Cout && c < Cin) ? w[(size_t)row * Cin + c] * (scale ? scale[row] : 1.f) * pre : 0.f;
            }
            o = Half::pack8(v);
        }
        reinterpret_cast<otp_u32x4*>(packed)[idx] = o;
    } else if (idx < nblk * units + HPW_MAXC / 4 + 1) {
        const int q = idx - nblk * units;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (q < HPW_MAXC / 4) {
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = (4 * q + i < Cout && shift) ? shift[4 * q + i] : 0.f;
        } else {
            v[0] = 1.f / pre;
        }
        reinterpret_cast<otp_u32x4*>(packed)[idx] = (otp_u32x4){__builtin_bit_cast(uint32_t, v[0]), __builtin_bit_cast(uint32_t, v[1]),
                                                        __builtin_bit_cast(uint32_t, v[2]), __builtin_bit_cast(uint32_t, v[3])};
    }
}

int hpw_ks(int Cin) {
    const int k = (Cin + 31) / 32;
    return k <= 2 ? 2 : (k <= 4 ? 4 : (k <= 8 ? 8 : (k <= 12 ? 12 : 0)));
}

// ================================================================================================================================
// stem: Conv2d(3, Cout <= 64, 3x3, stride 2, pad 1) + BN + ReLU on the frames of the fp32 clip tensor -> H8 (csrc/stem.hip)
// ================================================================================================================================
constexpr int HST_CT = 4;                 // 16-channel output tiles (Cout <= 64)
struct HSt {
    const float* in;
    const otp_u32x4* packed;
    otp_u32x4* out;
    int B, F, H, W, Ho, Wo, HoWo, Cout, total;
    uint32_t mWo;
    unsigned* rflag;
};

// packed: [cout tile][64 lanes] A fragments (lane (row i16, kq): k slots 8 kq .. 8 kq + 7, k = 3 tap + channel; rows of a tile pair
// permuted like everywhere in this file), then shift[64], then {post, 0, 0, 0}
__global__ void h16_stem_pack_kernel(const float* __restrict__ w, const float* __restrict__ scale, const float* __restrict__ shift,
                                     otp_u32x4* __restrict__ packed, int Cout) {
    __shared__ float wmax[4];
    float m = 0.f;
    for (int i = threadIdx.x; i < Cout * 27; i += blockDim.x) m = fmaxf(m, fabsf(w[i] * (scale ? scale[i / 27] : 1.f)));
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = m;
    __syncthreads();
    m = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
    int e = 0;
    (void)frexpf(m, &e);
    const int kx = (m > 0.f && m < 3e38f) ? min(40, max(-40, 14 - e)) : 0;
    const float pre = ldexpf(1.f, kx), post = ldexpf(1.f, -kx);
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx == HST_CT * 64 + 16) packed[idx] = (otp_u32x4){__builtin_bit_cast(uint32_t, post), 0u, 0u, 0u};
    if (idx < HST_CT * 64) {
        const int t = idx >> 6, lane = idx & 63, r16 = lane & 15, kq = lane >> 4;
        const int co = 32 * (t >> 1) + 8 * (r16 >> 2) + 4 * (t & 1) + (r16 & 3);
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int k = 8 * kq + j, tap = k / 3, c = k - tap * 3;               // reference weight layout (Cout, 3, 3, 3): [co][c][dy][dx]
            v[j] = (k < 27 && co < Cout) ? w[(co * 3 + c) * 9 + tap] * (scale ? scale[co] : 1.f) * pre : 0.f;
        }
        packed[idx] = Half::pack8(v);
    } else if (idx < HST_CT * 64 + 16) {
        const int q = idx - HST_CT * 64;
        float v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = (4 * q + i < Cout && shift) ? shift[4 * q + i] : 0.f;
        packed[idx] = (otp_u32x4){__builtin_bit_cast(uint32_t, v[0]), __builtin_bit_cast(uint32_t, v[1]), __builtin_bit_cast(uint32_t, v[2]),
                              __builtin_bit_cast(uint32_t, v[3])};
    }
}

// a wave: NPT tiles of 16 consecutive output pixels (all frames, row-major); lane (pixel i16, kq) gathers k slots 8 kq .. + 7 of its
// pixel (the B operand); A = the weights, so a lane's accumulators of a tile pair are 8 consecutive channels of ITS pixel
template <int NPT>
__global__ __launch_bounds__(256) void h16_stem_kernel(HSt A) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i16 = lane & 15, kq = lane >> 4;
    Half::x8 Wf[HST_CT];
#pragma unroll
    for (int t = 0; t < HST_CT; ++t) Wf[t] = __builtin_bit_cast(Half::x8, A.packed[t * 64 + lane]);
    const float* shp = reinterpret_cast<const float*>(A.packed + HST_CT * 64);
    otp_f32x4 sh[HST_CT];                                               // shift of the lane's channels: pair tp, tile m: 32 tp + 8 kq + 4 m ..
#pragma unroll
    for (int t = 0; t < HST_CT; ++t) sh[t] = *reinterpret_cast<const otp_f32x4*>(shp + 32 * (t >> 1) + 8 * kq + 4 * (t & 1));
    const float post = reinterpret_cast<const float*>(A.packed + HST_CT * 64 + 16)[0];
    const size_t clip = (size_t)3 * A.F * A.H * A.W;
    const otp_rsrc rin = make_rsrc(A.in, (size_t)A.B * clip * sizeof(float));
    const int G = (A.Cout + 7) >> 3;
    bool bad = false;
#pragma unroll 2
    for (int p = 0; p < NPT; ++p) {
        int px = ((int)blockIdx.x * 4 + wave) * (16 * NPT) + 16 * p + i16;
        const bool pv = px < A.total;
        if (!pv) px = A.total - 1;
        const int n = px / A.HoWo, pi = px - n * A.HoWo;                         // (exact division: px * HoWo passes 2^32 at cfg2)
        const int yo = (int)otp_magic_div((uint32_t)pi, A.mWo), xo = pi - yo * A.Wo;
        const int b = n % A.B, f = n / A.B;                                   // frame n = f B + b (model/OTPose.py:317)
        const int base = (b * 3 * A.F + 3 * f) * A.H * A.W;
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int k = 8 * kq + j, tap = k / 3, c = k - tap * 3, dy = tap / 3, dx = tap - dy * 3;
            const int iy = 2 * yo + dy - 1, ix = 2 * xo + dx - 1;
            const bool ok = k < 27 && iy >= 0 && iy < A.H && ix >= 0 && ix < A.W;
            v[j] = bload(rin, ok ? (base + (c * A.H + iy) * A.W + ix) * 4 : -16, 0);
        }
        const Half::x8 bx = __builtin_bit_cast(Half::x8, Half::pack8(v));
#pragma unroll
        for (int tp = 0; tp < HST_CT / 2; ++tp) {
            otp_f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
            a0 = Half::mfma(Wf[2 * tp], bx, a0);
            a1 = Half::mfma(Wf[2 * tp + 1], bx, a1);
            float o[8];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                o[r] = a0[r] * post + sh[2 * tp][r];
                o[4 + r] = a1[r] * post + sh[2 * tp + 1][r];
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                bad |= otp_out_of_range(o[e]);
                o[e] = fmaxf(o[e], 0.f);
            }
            const int g = 4 * tp + kq;
            if (pv && g < G) A.out[((size_t)n * G + g) * A.HoWo + pi] = Half::pack8(o);
        }
    }
    otp_range_report(A.rflag, bad, OTP_RANGE_H16);
}

// ================================================================================================================================
// element-wise passes on H8 images
// ================================================================================================================================
// fp32 NCHW channel slice -> H8 (one rounding); a thread owns one pixel of one 8-channel group (1 KB store runs per wave)
__global__ __launch_bounds__(256) void h8_pack_kernel(const float* __restrict__ in, otp_u32x4* __restrict__ out, int N, int C, int HW,
                                                       int ctot, int coff, int gtot, int goff, unsigned* rflag) {
    const int G8 = C >> 3;
    const size_t items = (size_t)N * G8 * HW;
    bool bad = false;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < items; i += (size_t)gridDim.x * 256) {
        const int p = (int)(i % HW);
        const size_t r = i / HW;
        const int g = (int)(r % G8), n = (int)(r / G8);
        const float* src = in + ((size_t)n * ctot + coff + 8 * g) * HW + p;
        float f[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) f[e] = src[(size_t)e * HW];
#pragma unroll
        for (int e = 0; e < 8; ++e) bad |= otp_out_of_range(f[e]);
        out[((size_t)n * gtot + goff + g) * HW + p] = Half::pack8(f);
    }
    otp_range_report(rflag, bad, OTP_RANGE_H16);
}

__global__ __launch_bounds__(256) void h8_unpack_kernel(const otp_u32x4* __restrict__ in, float* __restrict__ out, int N, int C, int HW,
                                                         int gtot, int goff) {
    const int G8 = C >> 3;
    const size_t items = (size_t)N * G8 * HW;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < items; i += (size_t)gridDim.x * 256) {
        const int p = (int)(i % HW);
        const size_t r = i / HW;
        const int g = (int)(r % G8), n = (int)(r / G8);
        const otp_u32x4 v = in[((size_t)n * gtot + goff + g) * HW + p];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const otp_f32x2 a = Half::widen(v[e]);
            out[((size_t)n * C + 8 * g + 2 * e) * HW + p] = a.x;
            out[((size_t)n * C + 8 * g + 2 * e + 1) * HW + p] = a.y;
        }
    }
}

// a fuse row's tail (model/HRNet.py:487-494): out = act(res + up_f0(low0) + up_f1(low1) + ...), nearest up-sampling, all H8; the
// terms are added in fp32 in that order and rounded once
struct H8Up {
    const otp_u32x4* low[3];
    int f[3];
    int n;
};
__global__ __launch_bounds__(256) void h8_upsample_add_kernel(H8Up U, const otp_u32x4* __restrict__ res, otp_u32x4* __restrict__ out, int N,
                                                               int G8, int Hh, int Wh, int relu, unsigned* rflag) {
    const int HW = Hh * Wh;
    const size_t items = (size_t)N * G8 * HW;
    bool bad = false;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < items; i += (size_t)gridDim.x * 256) {
        const int p = (int)(i % HW);
        const size_t r = i / HW;                                    // (n, g) plane
        const int y = p / Wh, x = p - y * Wh;
        const otp_u32x4 rv = res[i];
        float f[8];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const otp_f32x2 a = Half::widen(rv[e]);
            f[2 * e] = a.x;
            f[2 * e + 1] = a.y;
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (k < U.n) {
                const int fk = U.f[k], Wl = Wh / fk, Hl = Hh / fk;
                const otp_u32x4 lv = U.low[k][r * (size_t)(Hl * Wl) + (y / fk) * Wl + x / fk];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const otp_f32x2 a = Half::widen(lv[e]);
                    f[2 * e] += a.x;
                    f[2 * e + 1] += a.y;
                }
            }
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            bad |= otp_out_of_range(f[e]);
            if (relu) f[e] = fmaxf(f[e], 0.f);
        }
        out[i] = Half::pack8(f);
    }
    otp_range_report(rflag, bad, OTP_RANGE_H16);
}

}  // namespace

// ---- C ABI ---------------------------------------------------------------------------------------------------------------------
#ifdef OTP_H16_TIMING
extern "C" int otp_h16_read_stamps(void* host_out, size_t bytes) {
    return hipMemcpyFromSymbol(host_out, HIP_SYMBOL(otp_h16_stamps), bytes) == hipSuccess ? OTP_OK : OTP_ERR_LAUNCH;
}
#endif
extern "C" size_t otp_h8_bytes(int N, int C, int H, int W) {
    if (N <= 0 || C <= 0 || H <= 0 || W <= 0 || C % 8) return 0;
    return (size_t)N * C * H * W * 2;
}

extern "C" int otp_h8_pack(const void* in, void* out, int N, int C, int H, int W, int in_ctot, int in_coff, int out_gtot,
                           int out_goff, void* stream) {
    if (!in || !out || N <= 0 || C <= 0 || H <= 0 || W <= 0 || in_coff < 0 || in_ctot < in_coff + C) return OTP_ERR_BAD_ARG;
    if (C % 8 || (reinterpret_cast<uintptr_t>(out) & 15) || (reinterpret_cast<uintptr_t>(in) & 3)) return OTP_ERR_UNSUPPORTED;
    if (out_gtot <= 0) out_gtot = C / 8, out_goff = 0;
    if (out_goff < 0 || out_goff + C / 8 > out_gtot) return OTP_ERR_BAD_ARG;
    const size_t items = (size_t)N * (C / 8) * (H * W);
    const int grid = (int)((items + 255) / 256 > 16384 ? 16384 : (items + 255) / 256);
    hipLaunchKernelGGL(h8_pack_kernel, dim3(grid), dim3(256), 0, static_cast<hipStream_t>(stream), static_cast<const float*>(in),
                       static_cast<otp_u32x4*>(out), N, C, H * W, in_ctot, in_coff, out_gtot, out_goff, otp_range_word());
    return otp_launch_status();
}

extern "C" int otp_h8_unpack(const void* in, void* out, int N, int C, int H, int W, int in_gtot, int in_goff, void* stream) {
    if (!in || !out || N <= 0 || C <= 0 || H <= 0 || W <= 0) return OTP_ERR_BAD_ARG;
    if (C % 8 || (reinterpret_cast<uintptr_t>(in) & 15)) return OTP_ERR_UNSUPPORTED;
    if (in_gtot <= 0) in_gtot = C / 8, in_goff = 0;
    if (in_goff < 0 || in_goff + C / 8 > in_gtot) return OTP_ERR_BAD_ARG;
    const size_t items = (size_t)N * (C / 8) * (H * W);
    const int grid = (int)((items + 255) / 256 > 16384 ? 16384 : (items + 255) / 256);
    hipLaunchKernelGGL(h8_unpack_kernel, dim3(grid), dim3(256), 0, static_cast<hipStream_t>(stream), static_cast<const otp_u32x4*>(in),
                       static_cast<float*>(out), N, C, H * W, in_gtot, in_goff);
    return otp_launch_status();
}

extern "C" int otp_h16_upsample_add(const void* const* lows, const int* factors, int nlow, const void* res, void* out, int N, int C,
                                    int Hh, int Wh, int relu, void* stream) {
    if (!lows || !factors || !res || !out || nlow < 1 || nlow > 3 || N <= 0 || C <= 0 || Hh <= 0 || Wh <= 0) return OTP_ERR_BAD_ARG;
    if (C % 8) return OTP_ERR_UNSUPPORTED;
    H8Up U{};
    U.n = nlow;
    for (int k = 0; k < nlow; ++k) {
        const int f = factors[k];
        if (!lows[k]) return OTP_ERR_BAD_ARG;
        if (f < 2 || (f & (f - 1)) || Hh % f || Wh % f) return OTP_ERR_UNSUPPORTED;
        if (reinterpret_cast<uintptr_t>(lows[k]) & 15) return OTP_ERR_UNSUPPORTED;
        U.low[k] = static_cast<const otp_u32x4*>(lows[k]);
        U.f[k] = f;
    }
    if ((reinterpret_cast<uintptr_t>(res) | reinterpret_cast<uintptr_t>(out)) & 15) return OTP_ERR_UNSUPPORTED;
    const size_t items = (size_t)N * (C / 8) * (Hh * Wh);
    const int grid = (int)((items + 255) / 256 > 16384 ? 16384 : (items + 255) / 256);
    hipLaunchKernelGGL(h8_upsample_add_kernel, dim3(grid), dim3(256), 0, static_cast<hipStream_t>(stream), U,
                       static_cast<const otp_u32x4*>(res), static_cast<otp_u32x4*>(out), N, C / 8, Hh, Wh, relu, otp_range_word());
    return otp_launch_status();
}

extern "C" int otp_h16_conv3x3_supported(const otp_h16_conv_desc* desc) {
    if (!desc) return 0;
    HPlan P{};
    return h16_conv_plan<Half>(*desc, P) ? 1 : 0;
}

extern "C" size_t otp_h16_conv3x3_weight_bytes(int Cout, int Cin) {
    if (Cout <= 0 || Cin <= 0 || Cin % 16) return 0;
    const int NTW = h16_ntw(Cout), nN = ((Cout + 15) / 16 + NTW - 1) / NTW;
    return (size_t)nN * (Cin / 16) * hwb(NTW);
}

extern "C" int otp_h16_conv3x3_pack_weight(const void* weight, const void* scale, void* wpacked, int Cout, int Cin, float pre,
                                           void* stream) {
    if (!weight || !wpacked || Cout <= 0 || Cin <= 0 || !(pre > 0.f)) return OTP_ERR_BAD_ARG;
    if (!otp_h16_conv3x3_weight_bytes(Cout, Cin)) return OTP_ERR_UNSUPPORTED;
    const int NTW = h16_ntw(Cout), nN = ((Cout + 15) / 16 + NTW - 1) / NTW, nChunks = Cin / 16;
    const int total = nN * nChunks * OTP_S8_KS * NTW * 64;
    hipLaunchKernelGGL(h16_wpack_kernel, dim3(otp_ceil_div(total, 256) > 2048 ? 2048 : otp_ceil_div(total, 256)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), static_cast<const float*>(weight), static_cast<const float*>(scale),
                       static_cast<otp_u32x4*>(wpacked), Cout, Cin, NTW, nN, nChunks, pre);
    return otp_launch_status();
}

extern "C" int otp_h16_conv3x3(const void* in_h8, const void* wpacked, const void* shift, const void* res_h8, void* out_h8,
                               const otp_h16_conv_desc* desc, void* stream) {
    if (!in_h8 || !wpacked || !out_h8 || !desc) return OTP_ERR_BAD_ARG;
    if ((reinterpret_cast<uintptr_t>(in_h8) | reinterpret_cast<uintptr_t>(wpacked) | reinterpret_cast<uintptr_t>(out_h8) |
         reinterpret_cast<uintptr_t>(res_h8) | reinterpret_cast<uintptr_t>(shift)) & 15)
        return OTP_ERR_UNSUPPORTED;
    HPlan P{};
    if (!h16_conv_plan<Half>(*desc, P)) return OTP_ERR_UNSUPPORTED;
    P.rflag = otp_range_word();
    return h16_conv_dispatch<Half>(in_h8, wpacked, static_cast<const float*>(shift), res_h8, out_h8, P, desc->stride, static_cast<hipStream_t>(stream));
}

extern "C" int otp_h16_pointwise_supported(int Cin, int Cout) {
    return (Cin > 0 && Cin % 8 == 0 && hpw_ks(Cin) > 0 && Cout > 0 && Cout <= HPW_MAXC) ? 1 : 0;
}

extern "C" size_t otp_h16_pointwise_weight_bytes(int Cin, int Cout) {
    if (!otp_h16_pointwise_supported(Cin, Cout)) return 0;
    const int KS = hpw_ks(Cin), nblk = (Cout + 31) / 32;
    return (size_t)nblk * hpw_blkb(KS) + HPW_MAXC * 4 + 16;
}

extern "C" int otp_h16_pointwise_pack(const void* w, const void* scale, const void* shift, void* packed, int Cin, int Cout, float pre,
                                      void* stream) {
    if (!w || !packed || !(pre > 0.f)) return OTP_ERR_BAD_ARG;
    const size_t bytes = otp_h16_pointwise_weight_bytes(Cin, Cout);
    if (!bytes) return OTP_ERR_UNSUPPORTED;
    const int KS = hpw_ks(Cin), nblk = (Cout + 31) / 32, total = (int)(bytes / 16);
    hipLaunchKernelGGL(h16_pw_pack_kernel, dim3(otp_ceil_div(total, 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const float*>(w), static_cast<const float*>(scale), static_cast<const float*>(shift),
                       static_cast<unsigned char*>(packed), Cin, Cout, KS, nblk, hpw_blkb(KS), pre);
    return otp_launch_status();
}

extern "C" int otp_h16_pointwise(const void* in_h8, const void* packed, const void* res_h8, void* out, int out_f32_nchw, int N, int Cin,
                                 int Cout, int HW, int in_gtot, int in_goff, int res_gtot, int res_goff, int out_tot, int out_off,
                                 int relu, float out_scale, void* stream) {
    if (!in_h8 || !packed || !out || N <= 0 || HW <= 0) return OTP_ERR_BAD_ARG;
    if (!otp_h16_pointwise_supported(Cin, Cout)) return OTP_ERR_UNSUPPORTED;
    if (!out_f32_nchw && Cout % 8) return OTP_ERR_UNSUPPORTED;
    if ((reinterpret_cast<uintptr_t>(in_h8) | reinterpret_cast<uintptr_t>(packed) | reinterpret_cast<uintptr_t>(res_h8)) & 15 ||
        reinterpret_cast<uintptr_t>(out) & (out_f32_nchw ? 3 : 15))
        return OTP_ERR_BAD_ARG;
    if (in_gtot <= 0) in_gtot = Cin / 8, in_goff = 0;
    if (res_gtot <= 0) res_gtot = Cout / 8, res_goff = 0;
    if (out_tot <= 0) out_tot = out_f32_nchw ? Cout : Cout / 8, out_off = 0;
    if (in_goff < 0 || in_goff + Cin / 8 > in_gtot || out_off < 0 || out_off + (out_f32_nchw ? Cout : Cout / 8) > out_tot ||
        (res_h8 && (Cout % 8 || res_goff < 0 || res_goff + Cout / 8 > res_gtot)))
        return OTP_ERR_BAD_ARG;
    if ((size_t)N * HW >= (1ull << 31)) return OTP_ERR_UNSUPPORTED;
    HPw a{};
    a.x = static_cast<const unsigned char*>(in_h8);
    a.packed = static_cast<const unsigned char*>(packed);
    a.res = static_cast<const unsigned char*>(res_h8);
    a.out = static_cast<unsigned char*>(out);
    a.total = N * HW, a.HW = HW, a.Cin = Cin, a.Cout = Cout, a.nblk = (Cout + 31) / 32, a.relu = relu ? 1 : 0, a.f32out = out_f32_nchw ? 1 : 0;
    const size_t hw16 = (size_t)HW * 16;
    a.x_imgB = in_gtot * hw16, a.x_gS = hw16, a.x_pS = 16, a.x_base = in_goff * hw16;
    a.r_imgB = res_gtot * hw16, a.r_gS = hw16, a.r_pS = 16, a.r_base = res_goff * hw16;
    a.o_imgB = out_tot * hw16, a.o_gS = hw16, a.o_pS = 16, a.o_base = out_off * hw16;
    a.o_tot = out_tot, a.o_off = out_off;
    a.post = out_scale > 0.f ? out_scale : 1.f;
    a.rflag = otp_range_word();
    const int KS = hpw_ks(Cin);
    a.shift = reinterpret_cast<const float*>(a.packed + (size_t)a.nblk * hpw_blkb(KS));
    hipStream_t st = static_cast<hipStream_t>(stream);
    switch (KS) {
        case 2: return hpw_launch<Half, 2>(a, st);
        case 4: return hpw_launch<Half, 4>(a, st);
        case 8: return hpw_launch<Half, 8>(a, st);
        default: return hpw_launch<Half, 12>(a, st);
    }
}

extern "C" int otp_h16_stem_supported(int B, int F, int H, int W, int Cout) {
    if (B <= 0 || F <= 0 || H < 2 || W < 2 || Cout <= 0 || Cout > 16 * HST_CT || Cout % 8) return 0;
    const int Wo = (W - 1) / 2 + 1, Ho = (H - 1) / 2 + 1;
    if ((size_t)B * 3 * F * H * W * 4 >= (1ull << 31) || (size_t)B * F * Ho * Wo >= (1ull << 31) ||
        (size_t)(Ho * Wo) * (size_t)(Ho * Wo) >= (1ull << 32))
        return 0;
    return 1;
}

extern "C" size_t otp_h16_stem_weight_bytes(int Cout) { return (Cout <= 0 || Cout > 16 * HST_CT) ? 0 : (HST_CT * 64 + 17) * 16; }

extern "C" int otp_h16_stem_pack(const void* w, const void* scale, const void* shift, void* packed, int Cout, void* stream) {
    if (!w || !packed) return OTP_ERR_BAD_ARG;
    if (!otp_h16_stem_weight_bytes(Cout)) return OTP_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(h16_stem_pack_kernel, dim3(otp_ceil_div(HST_CT * 64 + 17, 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const float*>(w), static_cast<const float*>(scale), static_cast<const float*>(shift),
                       static_cast<otp_u32x4*>(packed), Cout);
    return otp_launch_status();
}

/* out_h8 (F * B, Cout, Ho, Wo) = relu(conv3x3 s2 p1 of the frames of in (B, 3 F, H, W) fp32 + shift), frame n = f B + b */
extern "C" int otp_h16_stem(const void* in, const void* packed, void* out_h8, int B, int F, int H, int W, int Cout, void* stream) {
    if (!in || !packed || !out_h8) return OTP_ERR_BAD_ARG;
    if (!otp_h16_stem_supported(B, F, H, W, Cout)) return OTP_ERR_UNSUPPORTED;
    if ((reinterpret_cast<uintptr_t>(in) & 3) || ((reinterpret_cast<uintptr_t>(packed) | reinterpret_cast<uintptr_t>(out_h8)) & 15))
        return OTP_ERR_BAD_ARG;
    HSt a{};
    a.in = static_cast<const float*>(in);
    a.packed = static_cast<const otp_u32x4*>(packed);
    a.out = static_cast<otp_u32x4*>(out_h8);
    a.B = B, a.F = F, a.H = H, a.W = W, a.Ho = (H - 1) / 2 + 1, a.Wo = (W - 1) / 2 + 1, a.HoWo = a.Ho * a.Wo, a.Cout = Cout;
    a.total = B * F * a.HoWo;
    a.mWo = otp_magic((uint32_t)a.Wo);
    a.rflag = otp_range_word();
    constexpr int NPT = 4;
    hipLaunchKernelGGL(h16_stem_kernel<NPT>, dim3((unsigned)((a.total + 64 * NPT - 1) / (64 * NPT))), dim3(256), 0,
                       static_cast<hipStream_t>(stream), a);
    return otp_launch_status();
}
