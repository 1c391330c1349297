// BatchNorm (batch statistics) of the bf16 NHWC training path (csrc/nhwc.h), forward and backward: HBM-bound NHWC passes (16-byte
// accesses, fp32 arithmetic) around two small finalize kernels that fold per-tile / per-workgroup partial rows in fp64.
#include "nhwc.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------------
// BatchNorm (batch statistics) on NHWC bf16, fp32 arithmetic
// ---------------------------------------------------------------------------------------------------------------------
constexpr int BNF_RL = 128;                 // row lanes of the two finalize kernels (8 channels x BNF_RL rows = 1024 threads)

// The opening of both finalize kernels: the two sums over partial rows [rows][2][C] of channel c = blockIdx.x * 8 + (threadIdx.x & 7).
// 8 channels x 128 row lanes per workgroup: the partial rows (up to N * tiles of the conv, 2160 at 96x72 x 80) are the long
// axis - with 32 row lanes the backward's launch, between the two HBM passes of every layer's BatchNorm backward, was a 15 us chain.
// The totals are valid in row lane 0 (threadIdx.x < 8) of channels c < C.  The order of the additions is fixed (determinism, and
// the fp64 comparisons of the tests): four-way unrolled rows, tail rows, 128 -> 16 row lanes, then one thread per channel.
// Contains workgroup barriers; every thread of the workgroup must call it.
__device__ __forceinline__ void bnf_row_sums(const float* __restrict__ part, int rows, int C, double& s1, double& s2) {
    __shared__ double red[2][BNF_RL][8];
    const int cl = threadIdx.x & 7, rq = threadIdx.x >> 3, c = blockIdx.x * 8 + cl;
    s1 = 0.0, s2 = 0.0;
    if (c < C) {
        int r = rq;
        for (; r + 3 * BNF_RL < rows; r += 4 * BNF_RL) {
            float a[4], b[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                a[j] = part[((size_t)(r + BNF_RL * j) * 2) * C + c];
                b[j] = part[((size_t)(r + BNF_RL * j) * 2 + 1) * C + c];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) s1 += (double)a[j], s2 += (double)b[j];
        }
        for (; r < rows; r += BNF_RL) {
            s1 += (double)part[((size_t)r * 2) * C + c];
            s2 += (double)part[((size_t)r * 2 + 1) * C + c];
        }
    }
    red[0][rq][cl] = s1, red[1][rq][cl] = s2;
    __syncthreads();
    if (rq < 16) {                                  // fixed-order fold: 128 -> 16 row lanes, then one thread per channel
        for (int k = rq + 16; k < BNF_RL; k += 16) s1 += red[0][k][cl], s2 += red[1][k][cl];
        red[0][rq][cl] = s1, red[1][rq][cl] = s2;
    }
    __syncthreads();
    if (rq == 0 && c < C)
        for (int k = 1; k < 16; ++k) s1 += red[0][k][cl], s2 += red[1][k][cl];
}

// partial sums [rows][2][C] -> mean / rstd, scale = gamma*rstd, shift = beta - mean*scale, running statistics update
__global__ __launch_bounds__(8 * BNF_RL) void bn_finalize_kernel(const float* __restrict__ part, int rows, int C, int Ctrue, float count,
                                                           const float* __restrict__ gamma, const float* __restrict__ beta,
                                                           float* __restrict__ mean_o, float* __restrict__ rstd_o,
                                                           float* __restrict__ scale_o, float* __restrict__ shift_o,
                                                           float* __restrict__ run_mean, float* __restrict__ run_var, float eps,
                                                           float momentum) {
    const int rq = threadIdx.x >> 3, c = blockIdx.x * 8 + (threadIdx.x & 7);
    double s1, s2;
    bnf_row_sums(part, rows, C, s1, s2);
    if (rq == 0 && c < C) {
        const double m = s1 / count;
        double var = s2 / count - m * m;
        if (var < 0.0) var = 0.0;
        const float rstd = (float)(1.0 / sqrt(var + (double)eps));
        const bool live = c < Ctrue;
        const float g = live ? gamma[c] : 0.f, b = live ? beta[c] : 0.f;
        mean_o[c] = (float)m, rstd_o[c] = rstd;
        scale_o[c] = g * rstd;
        shift_o[c] = b - (float)m * g * rstd;
        if (live && run_mean) {
            run_mean[c] = (1.f - momentum) * run_mean[c] + momentum * (float)m;
            const double unb = count > 1.f ? var * (double)count / ((double)count - 1.0) : var;
            run_var[c] = (1.f - momentum) * run_var[c] + momentum * (float)unb;
        }
    }
}

}  // namespace

extern "C" int otp_nhwc_bn_finalize(const void* partials, int rows, int C, int CS, float count, const void* gamma,
                                    const void* beta, void* mean, void* rstd, void* scale, void* shift, void* running_mean,
                                    void* running_var, float eps, float momentum, void* stream) {
    if (!partials || !gamma || !beta || !mean || !rstd || !scale || !shift || rows <= 0 || C <= 0 || CS < C)
        return OTP_ERR_BAD_ARG;
    bn_finalize_kernel<<<(CS + 7) / 8, 8 * BNF_RL, 0, static_cast<hipStream_t>(stream)>>>(
        static_cast<const float*>(partials), rows, CS, C, count, static_cast<const float*>(gamma), static_cast<const float*>(beta),
        static_cast<float*>(mean), static_cast<float*>(rstd), static_cast<float*>(scale), static_cast<float*>(shift),
        static_cast<float*>(running_mean), static_cast<float*>(running_var), eps, momentum);
    return otp_launch_status();
}

namespace {

// y = act(x*scale[c] + shift[c] (+ res)); 8 channels per thread
template <bool HAS_RES>
__global__ __launch_bounds__(256) void bn_apply_kernel(const bf16* __restrict__ x, const float* __restrict__ scale,
                                                        const float* __restrict__ shift, const bf16* __restrict__ res,
                                                        bf16* __restrict__ y, unsigned char* __restrict__ mask, size_t units,
                                                        int C8, int relu) {
    for (size_t u = blockIdx.x * (size_t)blockDim.x + threadIdx.x; u < units; u += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(u % C8) * 8;
        const bf16x8 v = *reinterpret_cast<const bf16x8*>(x + u * 8);
        bf16x8 r8;
        if constexpr (HAS_RES) r8 = *reinterpret_cast<const bf16x8*>(res + u * 8);
        const otp_f32x4 sa = *reinterpret_cast<const otp_f32x4*>(scale + c), sb = *reinterpret_cast<const otp_f32x4*>(scale + c + 4);
        const otp_f32x4 ha = *reinterpret_cast<const otp_f32x4*>(shift + c), hb = *reinterpret_cast<const otp_f32x4*>(shift + c + 4);
        bf16x8 o;
        unsigned bits = 0;                                     // ReLU mask of the 8 channels (1 bit each): what backward needs of y
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float f = bf2f(v[j]) * (j < 4 ? sa[j] : sb[j - 4]) + (j < 4 ? ha[j] : hb[j - 4]);
            if constexpr (HAS_RES) f += bf2f(r8[j]);
            if (relu) {
                bits |= (f > 0.f ? 1u : 0u) << j;
                f = fmaxf(f, 0.f);
            }
            o[j] = (bf16)f;
        }
        *reinterpret_cast<bf16x8*>(y + u * 8) = o;
        if (mask) mask[u] = (unsigned char)bits;
    }
}

}  // namespace

extern "C" int otp_nhwc_bn_apply(const void* x, const void* scale, const void* shift, const void* res, void* y, void* relu_mask,
                                 size_t pixels, int CS, int relu, void* stream) {
    if (!x || !scale || !shift || !y || CS <= 0 || CS % 8) return OTP_ERR_BAD_ARG;
    const size_t units = pixels * (CS / 8);
    if (res)
        bn_apply_kernel<true><<<grid_for(units), 256, 0, static_cast<hipStream_t>(stream)>>>(
            static_cast<const bf16*>(x), static_cast<const float*>(scale), static_cast<const float*>(shift),
            static_cast<const bf16*>(res), static_cast<bf16*>(y), static_cast<unsigned char*>(relu_mask), units, CS / 8, relu);
    else
        bn_apply_kernel<false><<<grid_for(units), 256, 0, static_cast<hipStream_t>(stream)>>>(
            static_cast<const bf16*>(x), static_cast<const float*>(scale), static_cast<const float*>(shift), nullptr,
            static_cast<bf16*>(y), static_cast<unsigned char*>(relu_mask), units, CS / 8, relu);
    return otp_launch_status();
}

namespace {

// backward pass 1: per-workgroup partial sums of g and g*xhat over a pixel range, g = gy * (y > 0 when relu)
// threads: (pixel lane pl, channel group cg); partial rows [wg][2][C]
template <int RELU>    // 0: no activation, 1: y tensor, 2: bit mask (compile time: a runtime branch around a load makes hipcc drain every outstanding load)
__global__ __launch_bounds__(256) void bn_bwd_reduce_kernel(const bf16* __restrict__ gy, const bf16* __restrict__ y,
                                                             const bf16* __restrict__ x, const float* __restrict__ mean,
                                                             const float* __restrict__ rstd, float* __restrict__ part,
                                                             size_t npix, int C8, int pixPerWg, int relu) {
    extern __shared__ float sred[];                       // [ppw][C8*16]
    const int ppw = 256 / C8;
    const int pl = threadIdx.x / C8, cg = threadIdx.x - pl * C8;
    const int C = C8 * 8;
    float s1[8], s2[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) s1[j] = s2[j] = 0.f;
    if (pl < ppw) {
        float mu[8], rs[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) mu[j] = mean[cg * 8 + j], rs[j] = rstd[cg * 8 + j];
        const size_t pbeg = (size_t)blockIdx.x * pixPerWg;
        const size_t pend = pbeg + pixPerWg < npix ? pbeg + pixPerWg : npix;
        for (size_t px = pbeg + pl; px < pend; px += ppw) {
            const size_t o = px * C + cg * 8;
            const bf16x8 g8 = *reinterpret_cast<const bf16x8*>(gy + o);
            const bf16x8 x8 = *reinterpret_cast<const bf16x8*>(x + o);
            bf16x8 y8;
            unsigned bits = 0xffu;
            if constexpr (RELU == 1) y8 = *reinterpret_cast<const bf16x8*>(y + o);
            if constexpr (RELU == 2) bits = reinterpret_cast<const unsigned char*>(y)[px * C8 + cg];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                float g = bf2f(g8[j]);
                if constexpr (RELU == 1) { if (!(bf2f(y8[j]) > 0.f)) g = 0.f; }
                if constexpr (RELU == 2) { if (!((bits >> j) & 1u)) g = 0.f; }
                s1[j] += g;
                s2[j] += g * (bf2f(x8[j]) - mu[j]) * rs[j];
            }
        }
    }
    if (pl < ppw) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            sred[(pl * C8 + cg) * 16 + j] = s1[j];
            sred[(pl * C8 + cg) * 16 + 8 + j] = s2[j];
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < C8 * 16; i += 256) {
        float v = 0.f;
        for (int k = 0; k < ppw; ++k) v += sred[k * C8 * 16 + i];
        const int cgi = i / 16, j = i & 15;
        part[((size_t)blockIdx.x * 2 + (j >> 3)) * C + cgi * 8 + (j & 7)] = v;
    }
}

// partials -> dgamma, dbeta, and the three per-channel coefficients of pass 2
__global__ __launch_bounds__(8 * BNF_RL) void bn_bwd_finalize_kernel(const float* __restrict__ part, int rows, int C, int Ctrue,
                                                                      float count, const float* __restrict__ gamma,
                                                                      const float* __restrict__ rstd, float* __restrict__ dgamma,
                                                                      float* __restrict__ dbeta, float* __restrict__ coef) {
    const int rq = threadIdx.x >> 3, c = blockIdx.x * 8 + (threadIdx.x & 7);
    double s1, s2;
    bnf_row_sums(part, rows, C, s1, s2);
    if (rq == 0 && c < C) {
        const bool live = c < Ctrue;
        if (live) dbeta[c] = (float)s1, dgamma[c] = (float)s2;
        const float k1 = live ? gamma[c] * rstd[c] : 0.f;
        coef[c] = k1;                                     // gx = k1 * (g - mg - xhat * mgx)
        coef[C + c] = (float)(s1 / count);
        coef[2 * C + c] = (float)(s2 / count);
    }
}

template <int RELU>
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const bf16* __restrict__ gy, const bf16* __restrict__ y,
                                                            const bf16* __restrict__ x, const float* __restrict__ mean,
                                                            const float* __restrict__ rstd, const float* __restrict__ coef,
                                                            bf16* __restrict__ gx, bf16* __restrict__ gres, size_t units, int C8,
                                                            int relu) {
    const int C = C8 * 8;
    for (size_t u = blockIdx.x * (size_t)blockDim.x + threadIdx.x; u < units; u += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(u % C8) * 8;
        const bf16x8 g8 = *reinterpret_cast<const bf16x8*>(gy + u * 8);
        const bf16x8 x8 = *reinterpret_cast<const bf16x8*>(x + u * 8);
        bf16x8 y8;
        unsigned bits = 0xffu;
        if constexpr (RELU == 1) y8 = *reinterpret_cast<const bf16x8*>(y + u * 8);
        if constexpr (RELU == 2) bits = reinterpret_cast<const unsigned char*>(y)[u];
        bf16x8 o, gr;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float g = bf2f(g8[j]);
            if constexpr (RELU == 1) { if (!(bf2f(y8[j]) > 0.f)) g = 0.f; }
            if constexpr (RELU == 2) { if (!((bits >> j) & 1u)) g = 0.f; }
            const float xh = (bf2f(x8[j]) - mean[c + j]) * rstd[c + j];
            o[j] = (bf16)(coef[c + j] * (g - coef[C + c + j] - xh * coef[2 * C + c + j]));
            gr[j] = (bf16)g;
        }
        *reinterpret_cast<bf16x8*>(gx + u * 8) = o;
        if (gres) *reinterpret_cast<bf16x8*>(gres + u * 8) = gr;
    }
}

}  // namespace

extern "C" size_t otp_nhwc_bn_backward_workspace(size_t pixels, int CS) {
    int ppw;
    const int rows = bn_bwd_rows(pixels, &ppw);
    return ((size_t)rows * 2 * CS + 3 * (size_t)CS) * sizeof(float);
}

// gx (and gres = gy * relu-mask when not NULL) from gy; dgamma / dbeta (C floats) overwritten.  y may be NULL when relu == 0.
extern "C" int otp_nhwc_bn_backward(const void* gy, const void* y, const void* x, const void* mean, const void* rstd,
                                    const void* gamma, void* gx, void* gres, void* dgamma, void* dbeta, void* workspace,
                                    size_t workspace_bytes, size_t pixels, int C, int CS, int relu, void* stream) {
    if (!gy || !x || !mean || !rstd || !gamma || !gx || !dgamma || !dbeta || !workspace || (relu && !y) || CS % 8 || CS > 2048)
        return OTP_ERR_BAD_ARG;
    if (workspace_bytes < otp_nhwc_bn_backward_workspace(pixels, CS)) return OTP_ERR_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    int ppw;
    const int rows = bn_bwd_rows(pixels, &ppw);
    float* part = static_cast<float*>(workspace);
    float* coef = part + (size_t)rows * 2 * CS;
    const int C8 = CS / 8;
    if (C8 > 256) return OTP_ERR_UNSUPPORTED;
    const size_t lds = (size_t)(256 / C8) * C8 * 16 * sizeof(float);
#define OTP_BN_BWD(R)                                                                                               \
    {                                                                                                                \
        bn_bwd_reduce_kernel<R><<<rows, 256, lds, st>>>(static_cast<const bf16*>(gy), static_cast<const bf16*>(y),    \
                                                        static_cast<const bf16*>(x), static_cast<const float*>(mean), \
                                                        static_cast<const float*>(rstd), part, pixels, C8, ppw, relu); \
        bn_bwd_finalize_kernel<<<(CS + 7) / 8, 8 * BNF_RL, 0, st>>>(part, rows, CS, C, (float)pixels,                         \
                                                             static_cast<const float*>(gamma),                        \
                                                             static_cast<const float*>(rstd), static_cast<float*>(dgamma), \
                                                             static_cast<float*>(dbeta), coef);                       \
        bn_bwd_apply_kernel<R><<<grid_for(units), 256, 0, st>>>(                                                      \
            static_cast<const bf16*>(gy), static_cast<const bf16*>(y), static_cast<const bf16*>(x),                   \
            static_cast<const float*>(mean), static_cast<const float*>(rstd), coef, static_cast<bf16*>(gx),           \
            static_cast<bf16*>(gres), units, C8, relu);                                                               \
    }
    const size_t units = pixels * C8;
    if (relu == 0) OTP_BN_BWD(0)
    else if (relu == 1) OTP_BN_BWD(1)
    else OTP_BN_BWD(2)
#undef OTP_BN_BWD
    return otp_launch_status();
}
