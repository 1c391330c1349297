// HBM-bound passes of the bf16 NHWC training path (csrc/nhwc.h) besides BatchNorm (16-byte accesses, fp32 arithmetic):
// upsample_add_* (HRNet fuse rows), the NCHW fp32 <-> NHWC bf16 layout conversions, zero-insertion, per-channel sums,
// GELU and GELU + dropout.
#include "nhwc.h"
#include "hb.h"

// ---------------------------------------------------------------------------------------------------------------------
// nearest-upsample-accumulate (HRNet fuse rows, model/HRNet.py:426-439, 488-494) and layout converters
// ---------------------------------------------------------------------------------------------------------------------
namespace {

// out[n, y, x, c] = act(res[n, y, x, c] + low[n, y/f, x/f, c])
__global__ __launch_bounds__(256) void upsample_add_nhwc_kernel(const bf16* __restrict__ low, const bf16* __restrict__ res,
                                                                 bf16* __restrict__ out, int N, int H, int W, int C8, int f,
                                                                 int relu) {
    const size_t units = (size_t)N * H * W * C8;
    const int Hl = H / f, Wl = W / f;
    for (size_t u = blockIdx.x * (size_t)blockDim.x + threadIdx.x; u < units; u += (size_t)gridDim.x * blockDim.x) {
        size_t r = u;
        const int cg = r % C8; r /= C8;
        const int xx = r % W; r /= W;
        const int yy = r % H;
        const int n = (int)(r / H);
        const bf16x8 a = *reinterpret_cast<const bf16x8*>(res + u * 8);
        const bf16x8 b = *reinterpret_cast<const bf16x8*>(low + ((((size_t)n * Hl + yy / f) * Wl + xx / f) * C8 + cg) * 8);
        bf16x8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float v = bf2f(a[j]) + bf2f(b[j]);
            if (relu) v = fmaxf(v, 0.f);
            o[j] = (bf16)v;
        }
        *reinterpret_cast<bf16x8*>(out + u * 8) = o;
    }
}

// gres = gy * mask, glow[n, yl, xl, c] = sum over the f x f block of gy * mask   (mask = out > 0 when relu)
__global__ __launch_bounds__(256) void upsample_add_nhwc_bwd_kernel(const bf16* __restrict__ gy, const bf16* __restrict__ out,
                                                                     bf16* __restrict__ gres, bf16* __restrict__ glow, int N,
                                                                     int Hl, int Wl, int C8, int f, int relu) {
    const size_t units = (size_t)N * Hl * Wl * C8;
    const int H = Hl * f, W = Wl * f;
    for (size_t u = blockIdx.x * (size_t)blockDim.x + threadIdx.x; u < units; u += (size_t)gridDim.x * blockDim.x) {
        size_t r = u;
        const int cg = r % C8; r /= C8;
        const int xl = r % Wl; r /= Wl;
        const int yl = r % Hl;
        const int n = (int)(r / Hl);
        float s[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) s[j] = 0.f;
        for (int dy = 0; dy < f; ++dy)
            for (int dx = 0; dx < f; ++dx) {
                const size_t o = ((((size_t)n * H + yl * f + dy) * W + xl * f + dx) * C8 + cg) * 8;
                const bf16x8 g8 = *reinterpret_cast<const bf16x8*>(gy + o);
                bf16x8 y8, gr;
                if (relu) y8 = *reinterpret_cast<const bf16x8*>(out + o);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    float g = bf2f(g8[j]);
                    if (relu && !(bf2f(y8[j]) > 0.f)) g = 0.f;
                    s[j] += g;
                    gr[j] = (bf16)g;
                }
                *reinterpret_cast<bf16x8*>(gres + o) = gr;
            }
        bf16x8 o8;
#pragma unroll
        for (int j = 0; j < 8; ++j) o8[j] = (bf16)s[j];
        *reinterpret_cast<bf16x8*>(glow + u * 8) = o8;
    }
}

}  // namespace

extern "C" int otp_nhwc_upsample_add(const void* low, const void* res, void* out, int N, int H, int W, int CS, int f, int relu,
                                     void* stream) {
    if (!low || !res || !out || f <= 0 || H % f || W % f || CS % 8) return OTP_ERR_BAD_ARG;
    upsample_add_nhwc_kernel<<<grid_for((size_t)N * H * W * (CS / 8)), 256, 0, static_cast<hipStream_t>(stream)>>>(
        static_cast<const bf16*>(low), static_cast<const bf16*>(res), static_cast<bf16*>(out), N, H, W, CS / 8, f, relu);
    return otp_launch_status();
}

extern "C" int otp_nhwc_upsample_add_backward(const void* gy, const void* out, void* gres, void* glow, int N, int Hl, int Wl,
                                              int CS, int f, int relu, void* stream) {
    if (!gy || !gres || !glow || (relu && !out) || f <= 0 || CS % 8) return OTP_ERR_BAD_ARG;
    upsample_add_nhwc_bwd_kernel<<<grid_for((size_t)N * Hl * Wl * (CS / 8)), 256, 0, static_cast<hipStream_t>(stream)>>>(
        static_cast<const bf16*>(gy), static_cast<const bf16*>(out), static_cast<bf16*>(gres), static_cast<bf16*>(glow), N, Hl, Wl,
        CS / 8, f, relu);
    return otp_launch_status();
}

namespace {

// (N, C, H, W) fp32 -> (N, H, W, CS) bf16, padding channels zero.  frame_split = B > 0 reads the (B, 5*C, H, W) clip tensor
// as (5B, C, H, W) with image n = f*B + b from channels [f*C, (f+1)*C) of sample b (model/OTPose.py:317).
__global__ __launch_bounds__(256) void nchw_to_nhwc_kernel(const float* __restrict__ in, bf16* __restrict__ out, int N, int C,
                                                            int HW, int CS, int frame_split) {
    const size_t total = (size_t)N * HW;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int n = (int)(i / HW), px = (int)(i - (size_t)n * HW);
        const float* src;
        if (frame_split > 0) {
            const int fr = n / frame_split, b = n - fr * frame_split;
            src = in + (((size_t)b * (N / frame_split) + fr) * C) * HW + px;
        } else {
            src = in + (size_t)n * C * HW + px;
        }
        for (int c0 = 0; c0 < CS; c0 += 8) {
            bf16x8 o;
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] = (bf16)(c0 + j < C ? src[(size_t)(c0 + j) * HW] : 0.f);
            *reinterpret_cast<bf16x8*>(out + i * CS + c0) = o;
        }
    }
}

// The same conversion for tensors with many channels (the (B, C, T) sequences of the temporal encoders: C = 136): a workgroup moves
// 64 pixels x all channels through the LDS - reads are 256-byte runs of one channel plane, writes 16-byte units of the tile's
// CONTIGUOUS 64 x CS x 2 bytes (the kernel above scatters a 16-byte piece per thread at the pixel stride: 46 us for 16 x 136 x 6912
// against 16 us for the opposite direction).  LDS rows of CS / 2 | 1 dwords (channel pairs): an odd stride, no bank conflicts.
__global__ __launch_bounds__(256) void nchw_to_nhwc_tile_kernel(const float* __restrict__ in, bf16* __restrict__ out, int C, int HW,
                                                                 int CS) {
    extern __shared__ unsigned int ttile[];
    const int tilesPerImg = (HW + 63) / 64;
    const int n = blockIdx.x / tilesPerImg, p0 = (blockIdx.x - n * tilesPerImg) * 64;
    const int RS = (CS / 2) | 1;
    const int px = threadIdx.x & 63, g = threadIdx.x >> 6;
    const bool pv = p0 + px < HW;
    const float* src = in + (size_t)n * C * HW + p0 + (pv ? px : 0);
#pragma unroll 4
    for (int cp = g; cp < CS / 2; cp += 4) {
        const int c = 2 * cp;
        const float a = (pv && c < C) ? src[(size_t)c * HW] : 0.f, b = (pv && c + 1 < C) ? src[(size_t)(c + 1) * HW] : 0.f;
        typedef bf16 bf16x2_t __attribute__((ext_vector_type(2)));
        ttile[px * RS + cp] = __builtin_bit_cast(unsigned int, (bf16x2_t){(bf16)a, (bf16)b});
    }
    __syncthreads();
    const int U = CS / 8, npx = HW - p0 < 64 ? HW - p0 : 64;
    typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
    for (int u = threadIdx.x; u < npx * U; u += 256) {
        const int q = u / U, k = u - q * U;
        const unsigned int* r = ttile + q * RS + 4 * k;
        *reinterpret_cast<u32x4_t*>(out + ((size_t)n * HW + p0 + q) * CS + 8 * k) = (u32x4_t){r[0], r[1], r[2], r[3]};
    }
}

}  // namespace

// (N, C, H, W) fp32 gradient -> (N, H, W, CS) bf16 (same as nchw_to_nhwc without frame_split) is reused for grads.
extern "C" int otp_nchw_f32_to_nhwc_bf16(const void* in, void* out, int N, int C, int H, int W, int frame_split, void* stream) {
    if (!in || !out || N <= 0 || C <= 0 || (frame_split > 0 && N % frame_split)) return OTP_ERR_BAD_ARG;
    const int CS = (C + 7) / 8 * 8;
    if (frame_split <= 0 && CS >= 32 && CS <= 4096 && (size_t)N * ((H * W + 63) / 64) < (1ull << 31)) {
        nchw_to_nhwc_tile_kernel<<<N * ((H * W + 63) / 64), 256, (size_t)64 * ((CS / 2) | 1) * 4, static_cast<hipStream_t>(stream)>>>(
            static_cast<const float*>(in), static_cast<bf16*>(out), C, H * W, CS);
        return otp_launch_status();
    }
    nchw_to_nhwc_kernel<<<grid_for((size_t)N * H * W), 256, 0, static_cast<hipStream_t>(stream)>>>(
        static_cast<const float*>(in), static_cast<bf16*>(out), N, C, H * W, CS, frame_split);
    return otp_launch_status();
}

namespace {

// (N, H, W, CS) bf16 -> (N, C, H, W) fp32: a workgroup moves 64 pixels x all channels through LDS, so that the reads are
// 16-byte units of whole pixel rows and the writes 256-byte runs of one channel plane
__global__ __launch_bounds__(256) void nhwc_to_nchw_kernel(const bf16* __restrict__ in, float* __restrict__ out, int N, int C,
                                                            int HW, int CS) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    bf16* sT = reinterpret_cast<bf16*>(smem);                 // [64][CS + 8]
    const int CP = CS + 8, C8 = CS / 8;
    const int tilesPerImg = (HW + 63) / 64;
    const int n = blockIdx.x / tilesPerImg, p0 = (blockIdx.x - n * tilesPerImg) * 64;
    const int npx = min(64, HW - p0);
    for (int u = threadIdx.x; u < 64 * C8; u += 256) {
        const int px = u / C8, cg = u - px * C8;
        otp_u32x4 v = {0u, 0u, 0u, 0u};
        if (px < npx) v = *reinterpret_cast<const otp_u32x4*>(in + ((size_t)n * HW + p0 + px) * CS + cg * 8);
        *reinterpret_cast<otp_u32x4*>(sT + px * CP + cg * 8) = v;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane < npx)
        for (int c = wave; c < C; c += 4) out[((size_t)n * C + c) * HW + p0 + lane] = bf2f(sT[lane * CP + c]);
}

}  // namespace

extern "C" int otp_nhwc_bf16_to_nchw_f32(const void* in, void* out, int N, int C, int H, int W, void* stream) {
    if (!in || !out || N <= 0 || C <= 0) return OTP_ERR_BAD_ARG;
    const int CS = (C + 7) / 8 * 8;
    if (CS > 2048) return OTP_ERR_UNSUPPORTED;
    const int tiles = N * ((H * W + 63) / 64);
    nhwc_to_nchw_kernel<<<tiles, 256, (size_t)64 * (CS + 8) * 2, static_cast<hipStream_t>(stream)>>>(
        static_cast<const bf16*>(in), static_cast<float*>(out), N, C, H * W, CS);
    return otp_launch_status();
}

namespace {

// zero-insertion for the input gradient of a strided conv: out (N, H, W, C) = 0 except out[:, y*s, x*s] = in[:, y, x]
__global__ __launch_bounds__(256) void dilate_nhwc_kernel(const bf16* __restrict__ in, bf16* __restrict__ out, int N, int Hi,
                                                           int Wi, int s, int H, int W, int C8) {
    const size_t units = (size_t)N * H * W * C8;
    for (size_t u = blockIdx.x * (size_t)blockDim.x + threadIdx.x; u < units; u += (size_t)gridDim.x * blockDim.x) {
        size_t r = u;
        const int cg = r % C8; r /= C8;
        const int xx = r % W; r /= W;
        const int yy = r % H;
        const int n = (int)(r / H);
        otp_u32x4 v = {0u, 0u, 0u, 0u};
        if (yy % s == 0 && xx % s == 0 && yy / s < Hi && xx / s < Wi)
            v = *reinterpret_cast<const otp_u32x4*>(in + ((((size_t)n * Hi + yy / s) * Wi + xx / s) * C8 + cg) * 8);
        *reinterpret_cast<otp_u32x4*>(out + u * 8) = v;
    }
}

}  // namespace

extern "C" int otp_nhwc_dilate(const void* in, void* out, int N, int Hi, int Wi, int s, int H, int W, int CS, void* stream) {
    if (!in || !out || s <= 0 || CS % 8) return OTP_ERR_BAD_ARG;
    dilate_nhwc_kernel<<<grid_for((size_t)N * H * W * (CS / 8)), 256, 0, static_cast<hipStream_t>(stream)>>>(
        static_cast<const bf16*>(in), static_cast<bf16*>(out), N, Hi, Wi, s, H, W, CS / 8);
    return otp_launch_status();
}

namespace {

// per-channel sums over the pixels of an NHWC bf16 tensor (bias gradients): partial rows [wg][C] -> out[c]
__global__ __launch_bounds__(256) void channel_sum_nhwc_kernel(const bf16* __restrict__ g, float* __restrict__ part, size_t npix,
                                                                int C8, int pixPerWg) {
    extern __shared__ float sred[];                       // [ppw][C8*8]
    const int ppw = 256 / C8;
    const int pl = threadIdx.x / C8, cg = threadIdx.x - pl * C8;
    const int C = C8 * 8;
    float s[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) s[j] = 0.f;
    if (pl < ppw) {
        const size_t pbeg = (size_t)blockIdx.x * pixPerWg;
        const size_t pend = pbeg + pixPerWg < npix ? pbeg + pixPerWg : npix;
        for (size_t px = pbeg + pl; px < pend; px += ppw) {
            const bf16x8 g8 = *reinterpret_cast<const bf16x8*>(g + px * C + cg * 8);
#pragma unroll
            for (int j = 0; j < 8; ++j) s[j] += bf2f(g8[j]);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) sred[(pl * C8 + cg) * 8 + j] = s[j];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < C; i += 256) {
        float v = 0.f;
        for (int k = 0; k < ppw; ++k) v += sred[k * C + i];
        part[(size_t)blockIdx.x * C + i] = v;
    }
}

__global__ __launch_bounds__(256) void channel_sum_nhwc_finish_kernel(const float* __restrict__ part, float* __restrict__ out,
                                                                       int rows, int C, int Ctrue) {
    __shared__ double red[32][8];
    const int cl = threadIdx.x & 7, rq = threadIdx.x >> 3, c = blockIdx.x * 8 + cl;
    double s = 0.0;
    if (c < C)
        for (int r = rq; r < rows; r += 32) s += (double)part[(size_t)r * C + c];
    red[rq][cl] = s;
    __syncthreads();
    if (rq == 0 && c < Ctrue) {
        for (int k = 1; k < 32; ++k) s += red[k][cl];
        out[c] = (float)s;
    }
}

}  // namespace

extern "C" size_t otp_nhwc_channel_sum_workspace(size_t pixels, int CS) {
    int ppw;
    const int rows = bn_bwd_rows(pixels, &ppw);
    return (size_t)rows * CS * sizeof(float);
}

// out[c] (C floats) = sum over pixels of g[pixel][c], g NHWC bf16 with channel stride CS (bias gradients)
extern "C" int otp_nhwc_channel_sum(const void* g, void* out, void* workspace, size_t workspace_bytes, size_t pixels, int C,
                                    int CS, void* stream) {
    if (!g || !out || !workspace || C <= 0 || CS < C || CS % 8 || CS > 2048) return OTP_ERR_BAD_ARG;
    if (workspace_bytes < otp_nhwc_channel_sum_workspace(pixels, CS)) return OTP_ERR_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    int ppw;
    const int rows = bn_bwd_rows(pixels, &ppw);
    const int C8 = CS / 8;
    channel_sum_nhwc_kernel<<<rows, 256, (size_t)(256 / C8) * CS * sizeof(float), st>>>(
        static_cast<const bf16*>(g), static_cast<float*>(workspace), pixels, C8, ppw);
    channel_sum_nhwc_finish_kernel<<<(CS + 7) / 8, 256, 0, st>>>(static_cast<const float*>(workspace), static_cast<float*>(out),
                                                                 rows, CS, C);
    return otp_launch_status();
}

namespace {

// exact-erf GELU on bf16 (nn.GELU of the TransformerBlock MLP, model/blocks.py:248-254), fp32 arithmetic
__global__ __launch_bounds__(256) void gelu_bf16_fwd_kernel(const bf16* __restrict__ x, bf16* __restrict__ y, size_t units) {
    for (size_t u = blockIdx.x * (size_t)blockDim.x + threadIdx.x; u < units; u += (size_t)gridDim.x * blockDim.x) {
        const bf16x8 v = *reinterpret_cast<const bf16x8*>(x + u * 8);
        bf16x8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float f = bf2f(v[j]);
            o[j] = (bf16)(0.5f * f * (1.f + erff(f * 0.70710678118654752440f)));
        }
        *reinterpret_cast<bf16x8*>(y + u * 8) = o;
    }
}
__global__ __launch_bounds__(256) void gelu_bf16_bwd_kernel(const bf16* __restrict__ x, const bf16* __restrict__ dy,
                                                             bf16* __restrict__ dx, size_t units) {
    for (size_t u = blockIdx.x * (size_t)blockDim.x + threadIdx.x; u < units; u += (size_t)gridDim.x * blockDim.x) {
        const bf16x8 v = *reinterpret_cast<const bf16x8*>(x + u * 8), g = *reinterpret_cast<const bf16x8*>(dy + u * 8);
        bf16x8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float f = bf2f(v[j]);
            const float cdf = 0.5f * (1.f + erff(f * 0.70710678118654752440f));
            const float pdf = 0.39894228040143267794f * expf(-0.5f * f * f);
            o[j] = (bf16)(bf2f(g[j]) * (cdf + f * pdf));
        }
        *reinterpret_cast<bf16x8*>(dx + u * 8) = o;
    }
}

}  // namespace

extern "C" int otp_gelu_bf16_forward(const void* x, void* y, size_t n, void* stream) {
    if (!x || !y || n % 8) return OTP_ERR_BAD_ARG;
    gelu_bf16_fwd_kernel<<<grid_for(n / 8), 256, 0, static_cast<hipStream_t>(stream)>>>(static_cast<const bf16*>(x),
                                                                                          static_cast<bf16*>(y), n / 8);
    return otp_launch_status();
}

extern "C" int otp_gelu_bf16_backward(const void* x, const void* grad_y, void* grad_x, size_t n, void* stream) {
    if (!x || !grad_y || !grad_x || n % 8) return OTP_ERR_BAD_ARG;
    gelu_bf16_bwd_kernel<<<grid_for(n / 8), 256, 0, static_cast<hipStream_t>(stream)>>>(
        static_cast<const bf16*>(x), static_cast<const bf16*>(grad_y), static_cast<bf16*>(grad_x), n / 8);
    return otp_launch_status();
}

namespace {

// GELU followed by Dropout(p) (model/blocks.py:250-251) as one pass: y = keep ? gelu(x) / (1 - p) : 0, one rounding, plus the keep
// decisions as one bit per element (a byte per 8-element unit) for the backward - the separate launches cost a 240 MB pass forward
// (fused_dropout) and a 360 MB one backward (masked_scale) per MLP.  Draws: a counter-based hash of (element pair, seed), two 16-bit
// uniforms per 32-bit hash (csrc/hb.h: otp_drop_keep8), keep <=> u16 >= round(65536 p); the seed comes from PyTorch's CUDA generator
// (bf16_ops.gelu_dropout), so torch.manual_seed reproduces a step.
__global__ __launch_bounds__(256) void gelu_dropout_bf16_fwd_kernel(const bf16* __restrict__ x, bf16* __restrict__ y,
                                                                     unsigned char* __restrict__ keep, size_t units, uint32_t s0, uint32_t s1,
                                                                     uint32_t thr, float scale) {
    for (size_t u = blockIdx.x * (size_t)blockDim.x + threadIdx.x; u < units; u += (size_t)gridDim.x * blockDim.x) {
        const bf16x8 v = *reinterpret_cast<const bf16x8*>(x + u * 8);
        const unsigned bits = otp_drop_keep8(u, s0, s1, thr);
        bf16x8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float f = bf2f(v[j]);
            const float g = 0.5f * f * (1.f + erff(f * 0.70710678118654752440f)) * scale;
            o[j] = (bf16)(((bits >> j) & 1u) ? g : 0.f);
        }
        *reinterpret_cast<bf16x8*>(y + u * 8) = o;
        keep[u] = (unsigned char)bits;
    }
}
__global__ __launch_bounds__(256) void gelu_dropout_bf16_bwd_kernel(const bf16* __restrict__ x, const bf16* __restrict__ dy,
                                                                     const unsigned char* __restrict__ keep, bf16* __restrict__ dx,
                                                                     size_t units, float scale) {
    for (size_t u = blockIdx.x * (size_t)blockDim.x + threadIdx.x; u < units; u += (size_t)gridDim.x * blockDim.x) {
        const bf16x8 v = *reinterpret_cast<const bf16x8*>(x + u * 8), g = *reinterpret_cast<const bf16x8*>(dy + u * 8);
        const unsigned bits = keep[u];
        bf16x8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float f = bf2f(v[j]);
            const float cdf = 0.5f * (1.f + erff(f * 0.70710678118654752440f));
            const float pdf = 0.39894228040143267794f * expf(-0.5f * f * f);
            o[j] = (bf16)(((bits >> j) & 1u) ? bf2f(g[j]) * scale * (cdf + f * pdf) : 0.f);
        }
        *reinterpret_cast<bf16x8*>(dx + u * 8) = o;
    }
}

}  // namespace

extern "C" int otp_gelu_dropout_bf16_forward(const void* x, void* y, void* keep_bits, size_t n, float p, unsigned long long seed,
                                             void* stream) {
    if (!x || !y || !keep_bits || n % 8 || !(p >= 0.f) || !(p < 1.f)) return OTP_ERR_BAD_ARG;
    const uint32_t thr = (uint32_t)(p * 65536.f + 0.5f);
    gelu_dropout_bf16_fwd_kernel<<<grid_for(n / 8), 256, 0, static_cast<hipStream_t>(stream)>>>(
        static_cast<const bf16*>(x), static_cast<bf16*>(y), static_cast<unsigned char*>(keep_bits), n / 8, (uint32_t)seed,
        (uint32_t)(seed >> 32), thr, 65536.f / (float)(65536u - thr));
    return otp_launch_status();
}

extern "C" int otp_gelu_dropout_bf16_backward(const void* x, const void* grad_y, const void* keep_bits, void* grad_x, size_t n, float p,
                                              void* stream) {
    if (!x || !grad_y || !keep_bits || !grad_x || n % 8 || !(p >= 0.f) || !(p < 1.f)) return OTP_ERR_BAD_ARG;
    const uint32_t thr = (uint32_t)(p * 65536.f + 0.5f);
    gelu_dropout_bf16_bwd_kernel<<<grid_for(n / 8), 256, 0, static_cast<hipStream_t>(stream)>>>(
        static_cast<const bf16*>(x), static_cast<const bf16*>(grad_y), static_cast<const unsigned char*>(keep_bits),
        static_cast<bf16*>(grad_x), n / 8, 65536.f / (float)(65536u - thr));
    return otp_launch_status();
}
