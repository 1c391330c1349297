// Forward passes of the ConvTransformer encoder for gfx950: channel LayerNorm (+ MaxPool1d skip), the three depthwise
// convs of MaskedMHCA each with its LayerNorm in one launch (dwconv_ln3), MaxPool1d(3, 2, 1), linear up-sampling.  Their
// backwards are in transformer_bwd.hip; the channel attention that consumes q, k, v is csrc/chanattn.hip.
// Reference: model/blocks.py:95-110 (LayerNorm), :234-238 (pool_skip), :400-415 (the q / k / v convs and norms of
// MaskedMHCA.forward), model/ConvVideoTransformer.py:108,163-184 (nn.Upsample linear).
//
// All tensors are (B, C, T) with T contiguous, so a thread owns one time step t and walks the C
// channels: every global access of a wave is a coalesced 256-byte run along T.
#include "common.h"

namespace {

// ---- channel LayerNorm ---------------------------------------------------------------------------
// CREG > 0: the C <= CREG channel values of a time step are held in registers (one HBM read).
template <int CREG>
__global__ __launch_bounds__(256) void ln_channel_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                          const float* __restrict__ beta, float* __restrict__ y,
                                                          int C, int T, float eps) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= T) return;
    const size_t base = (size_t)blockIdx.y * C * T + t;
    const float inv_c = 1.f / (float)C;
    if (CREG > 0) {
        float v[CREG > 0 ? CREG : 1];
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < CREG; ++c) {
            v[c] = c < C ? x[base + (size_t)c * T] : 0.f;
            s += v[c];
        }
        const float mu = s * inv_c;
        float q = 0.f;
#pragma unroll
        for (int c = 0; c < CREG; ++c) {
            v[c] -= mu;
            q += c < C ? v[c] * v[c] : 0.f;
        }
        const float rs = 1.f / sqrtf(q * inv_c + eps);
#pragma unroll
        for (int c = 0; c < CREG; ++c)
            if (c < C) y[base + (size_t)c * T] = v[c] * rs * gamma[c] + beta[c];
    } else {
        float s = 0.f;
        for (int c = 0; c < C; ++c) s += x[base + (size_t)c * T];
        const float mu = s * inv_c;
        float q = 0.f;
        for (int c = 0; c < C; ++c) {
            float dlt = x[base + (size_t)c * T] - mu;
            q += dlt * dlt;
        }
        const float rs = 1.f / sqrtf(q * inv_c + eps);
        for (int c = 0; c < C; ++c) y[base + (size_t)c * T] = (x[base + (size_t)c * T] - mu) * rs * gamma[c] + beta[c];
    }
}

// The same LayerNorm for wide channel counts (C = 136 of the temporal encoders): workgroup = 64 time steps x 4 waves that
// split the channels (lane = time step: 256-byte coalesced rows), statistics reduced across the waves through LDS, mean first,
// then the biased variance of the centred values.  One thread walking all 136 channels (ln_channel_kernel<136>) left the chip
// with 432 workgroups of dependent loads: 34 us for a 120 MB pass; this form runs 1728 workgroups.
template <int CW>
__global__ __launch_bounds__(256) void ln_channel_split_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                                const float* __restrict__ beta, float* __restrict__ y,
                                                                int C, int T, float eps) {
    __shared__ float red[2][4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int t = blockIdx.x * 64 + lane;
    const bool live = t < T;
    const size_t base = (size_t)blockIdx.y * C * T + (live ? t : 0);
    const float inv_c = 1.f / (float)C;
    const int cw = (C + 3) / 4, cbeg = wave * cw;
    float v[CW];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < CW; ++i) {
        const int c = cbeg + i;
        v[i] = (i < cw && c < C) ? x[base + (size_t)c * T] : 0.f;
        s += v[i];
    }
    red[0][wave][lane] = s;
    __syncthreads();
    const float mu = ((red[0][0][lane] + red[0][1][lane]) + (red[0][2][lane] + red[0][3][lane])) * inv_c;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < CW; ++i) {
        const int c = cbeg + i;
        if (i < cw && c < C) {
            v[i] -= mu;
            q += v[i] * v[i];
        }
    }
    red[1][wave][lane] = q;
    __syncthreads();
    const float rs = 1.f / sqrtf(((red[1][0][lane] + red[1][1][lane]) + (red[1][2][lane] + red[1][3][lane])) * inv_c + eps);
    if (!live) return;
#pragma unroll
    for (int i = 0; i < CW; ++i) {
        const int c = cbeg + i;
        if (i < cw && c < C) y[base + (size_t)c * T] = v[i] * rs * gamma[c] + beta[c];
    }
}

// MaxPool1d(kernel 3, stride 2, padding 1): To = (T + 2 - 3) / 2 + 1
__global__ void maxpool3s2_kernel(const float* __restrict__ x, float* __restrict__ y, int T, int To) {
    const int to = blockIdx.x * blockDim.x + threadIdx.x;
    if (to >= To) return;
    const float* xr = x + (size_t)blockIdx.y * T;
    const int t = 2 * to;
    float m = xr[t];
    if (t - 1 >= 0) m = fmaxf(m, xr[t - 1]);
    if (t + 1 < T) m = fmaxf(m, xr[t + 1]);
    y[(size_t)blockIdx.y * To + to] = m;
}

// ---- three depthwise convs (k=3, pad 1, stride s) each followed by a channel LayerNorm -------------
// Workgroup = 64 output time steps (lane = time step: 256-byte coalesced rows) x 4 waves that split the channels;
// every conv output is computed once and kept in registers (CW channels x 3 per lane), the channel statistics are
// reduced across the four waves through LDS: mean first, then the biased variance of the centred values
// (the two-pass form of blocks.py:100-103).
template <int CW>
__global__ __launch_bounds__(256) void dwconv_ln3_kernel(
    const float* __restrict__ x, const float* __restrict__ dwq, const float* __restrict__ dwk,
    const float* __restrict__ dwv, const float* __restrict__ gq, const float* __restrict__ bq,
    const float* __restrict__ gk, const float* __restrict__ bk, const float* __restrict__ gv,
    const float* __restrict__ bv, float* __restrict__ q, float* __restrict__ k, float* __restrict__ v,
    int C, int T, int To, int stride, float eps) {
    __shared__ float red[3][4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int to = blockIdx.x * 64 + lane;
    const bool live = to < To;
    const float* xb = x + (size_t)blockIdx.y * C * T;
    const size_t ob = (size_t)blockIdx.y * C * To + to;
    const int t0 = (live ? to : 0) * stride - 1;
    const bool l_ok = t0 >= 0, r_ok = t0 + 2 < T;
    const float inv_c = 1.f / (float)C;
    const int cw = (C + 3) / 4;                 // channels per wave (<= CW)
    const int cbeg = wave * cw;
    float dq[CW], dk[CW], dv[CW];
    float sq = 0.f, sk = 0.f, sv = 0.f;
#pragma unroll
    for (int i = 0; i < CW; ++i) {
        const int c = cbeg + i;
        dq[i] = dk[i] = dv[i] = 0.f;
        if (i < cw && c < C) {
            const float* xr = xb + (size_t)c * T + t0;
            const float a = l_ok ? xr[0] : 0.f, b = xr[1], cc = r_ok ? xr[2] : 0.f;
            dq[i] = dwq[c * 3] * a + dwq[c * 3 + 1] * b + dwq[c * 3 + 2] * cc;
            dk[i] = dwk[c * 3] * a + dwk[c * 3 + 1] * b + dwk[c * 3 + 2] * cc;
            dv[i] = dwv[c * 3] * a + dwv[c * 3 + 1] * b + dwv[c * 3 + 2] * cc;
            sq += dq[i]; sk += dk[i]; sv += dv[i];
        }
    }
    red[0][wave][lane] = sq; red[1][wave][lane] = sk; red[2][wave][lane] = sv;
    __syncthreads();
    const float mq = (red[0][0][lane] + red[0][1][lane] + red[0][2][lane] + red[0][3][lane]) * inv_c;
    const float mk = (red[1][0][lane] + red[1][1][lane] + red[1][2][lane] + red[1][3][lane]) * inv_c;
    const float mv = (red[2][0][lane] + red[2][1][lane] + red[2][2][lane] + red[2][3][lane]) * inv_c;
    __syncthreads();
    float vq = 0.f, vk = 0.f, vv = 0.f;
#pragma unroll
    for (int i = 0; i < CW; ++i) {
        const int c = cbeg + i;
        if (i < cw && c < C) {
            dq[i] -= mq; dk[i] -= mk; dv[i] -= mv;
            vq += dq[i] * dq[i]; vk += dk[i] * dk[i]; vv += dv[i] * dv[i];
        }
    }
    red[0][wave][lane] = vq; red[1][wave][lane] = vk; red[2][wave][lane] = vv;
    __syncthreads();
    const float rq = 1.f / sqrtf((red[0][0][lane] + red[0][1][lane] + red[0][2][lane] + red[0][3][lane]) * inv_c + eps);
    const float rk = 1.f / sqrtf((red[1][0][lane] + red[1][1][lane] + red[1][2][lane] + red[1][3][lane]) * inv_c + eps);
    const float rv = 1.f / sqrtf((red[2][0][lane] + red[2][1][lane] + red[2][2][lane] + red[2][3][lane]) * inv_c + eps);
    if (!live) return;
#pragma unroll
    for (int i = 0; i < CW; ++i) {
        const int c = cbeg + i;
        if (i < cw && c < C) {
            q[ob + (size_t)c * To] = dq[i] * rq * gq[c] + bq[c];
            k[ob + (size_t)c * To] = dk[i] * rk * gk[c] + bk[c];
            v[ob + (size_t)c * To] = dv[i] * rv * gv[c] + bv[c];
        }
    }
}

// any channel count: one thread per time step, three passes over the channels
__global__ __launch_bounds__(256) void dwconv_ln3_generic_kernel(
    const float* __restrict__ x, const float* __restrict__ dwq, const float* __restrict__ dwk,
    const float* __restrict__ dwv, const float* __restrict__ gq, const float* __restrict__ bq,
    const float* __restrict__ gk, const float* __restrict__ bk, const float* __restrict__ gv,
    const float* __restrict__ bv, float* __restrict__ q, float* __restrict__ k, float* __restrict__ v,
    int C, int T, int To, int stride, float eps) {
    const int to = blockIdx.x * blockDim.x + threadIdx.x;
    if (to >= To) return;
    const float* xb = x + (size_t)blockIdx.y * C * T;
    const size_t ob = (size_t)blockIdx.y * C * To + to;
    const int t0 = to * stride - 1;
    const bool l_ok = t0 >= 0, r_ok = t0 + 2 < T;
    const float inv_c = 1.f / (float)C;
    float sq = 0.f, sk = 0.f, sv = 0.f;
    for (int c = 0; c < C; ++c) {
        const float* xr = xb + (size_t)c * T + t0;
        const float a = l_ok ? xr[0] : 0.f, b = xr[1], cc = r_ok ? xr[2] : 0.f;
        sq += dwq[c * 3] * a + dwq[c * 3 + 1] * b + dwq[c * 3 + 2] * cc;
        sk += dwk[c * 3] * a + dwk[c * 3 + 1] * b + dwk[c * 3 + 2] * cc;
        sv += dwv[c * 3] * a + dwv[c * 3 + 1] * b + dwv[c * 3 + 2] * cc;
    }
    const float mq = sq * inv_c, mk = sk * inv_c, mv = sv * inv_c;
    float vq = 0.f, vk = 0.f, vv = 0.f;
    for (int c = 0; c < C; ++c) {
        const float* xr = xb + (size_t)c * T + t0;
        const float a = l_ok ? xr[0] : 0.f, b = xr[1], cc = r_ok ? xr[2] : 0.f;
        float d1 = dwq[c * 3] * a + dwq[c * 3 + 1] * b + dwq[c * 3 + 2] * cc - mq;
        float d2 = dwk[c * 3] * a + dwk[c * 3 + 1] * b + dwk[c * 3 + 2] * cc - mk;
        float d3 = dwv[c * 3] * a + dwv[c * 3 + 1] * b + dwv[c * 3 + 2] * cc - mv;
        vq += d1 * d1; vk += d2 * d2; vv += d3 * d3;
    }
    const float rq = 1.f / sqrtf(vq * inv_c + eps), rk = 1.f / sqrtf(vk * inv_c + eps), rv = 1.f / sqrtf(vv * inv_c + eps);
    for (int c = 0; c < C; ++c) {
        const float* xr = xb + (size_t)c * T + t0;
        const float a = l_ok ? xr[0] : 0.f, b = xr[1], cc = r_ok ? xr[2] : 0.f;
        float d1 = dwq[c * 3] * a + dwq[c * 3 + 1] * b + dwq[c * 3 + 2] * cc - mq;
        float d2 = dwk[c * 3] * a + dwk[c * 3 + 1] * b + dwk[c * 3 + 2] * cc - mk;
        float d3 = dwv[c * 3] * a + dwv[c * 3 + 1] * b + dwv[c * 3 + 2] * cc - mv;
        q[ob + (size_t)c * To] = d1 * rq * gq[c] + bq[c];
        k[ob + (size_t)c * To] = d2 * rk * gk[c] + bk[c];
        v[ob + (size_t)c * To] = d3 * rv * gv[c] + bv[c];
    }
}

// ---- nn.Upsample(scale_factor = f, mode = 'linear', align_corners = False) on (B, C, T) ------------
__global__ void upsample_linear_kernel(const float* __restrict__ x, float* __restrict__ out, int C, int T, int f,
                                       int out_ctot, int out_coff) {
    const int To = T * f;
    const int to = blockIdx.x * blockDim.x + threadIdx.x;
    if (to >= To) return;
    const int c = blockIdx.y % C, b = blockIdx.y / C;
    const float* xr = x + ((size_t)b * C + c) * T;
    float r;
    if (f == 1) {
        r = xr[to];
    } else {
        float src = ((float)to + 0.5f) * (1.f / (float)f) - 0.5f;
        src = src < 0.f ? 0.f : src;
        int i0 = (int)src;
        int i1 = i0 + (i0 < T - 1 ? 1 : 0);
        float l1 = src - (float)i0, l0 = 1.f - l1;
        r = l0 * xr[i0] + l1 * xr[i1];
    }
    out[((size_t)b * out_ctot + out_coff + c) * To + to] = r;
}

// four consecutive outputs per thread, one 16-byte store (rows of To = T f floats, To % 4 == 0, 16-byte aligned rows): the
// scalar form above moves the 60 MB pyramid levels of a temporal encoder at 2 TB/s
__global__ void upsample_linear4_kernel(const float* __restrict__ x, float* __restrict__ out, int C, int T, int f,
                                        int out_ctot, int out_coff) {
    const int To = T * f;
    const int t4 = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (t4 >= To) return;
    const int c = blockIdx.y % C, b = blockIdx.y / C;
    const float* xr = x + ((size_t)b * C + c) * T;
    otp_f32x4 r;
    if (f == 1) {
        r = *reinterpret_cast<const otp_f32x4*>(xr + t4);
    } else {
        const float inv = 1.f / (float)f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float src = ((float)(t4 + k) + 0.5f) * inv - 0.5f;
            src = src < 0.f ? 0.f : src;
            const int i0 = (int)src;
            const int i1 = i0 + (i0 < T - 1 ? 1 : 0);
            const float l1 = src - (float)i0, l0 = 1.f - l1;
            r[k] = l0 * xr[i0] + l1 * xr[i1];
        }
    }
    *reinterpret_cast<otp_f32x4*>(out + ((size_t)b * out_ctot + out_coff + c) * To + t4) = r;
}

}  // namespace

extern "C" int otp_ln_channel(const void* x, const void* gamma, const void* beta, void* y, void* pool, int B,
                              int C, int T, float eps, void* stream) {
    if (!x || !gamma || !beta || !y || B <= 0 || C <= 0 || T <= 0) return OTP_ERR_BAD_ARG;
    auto st = static_cast<hipStream_t>(stream);
    auto xf = static_cast<const float*>(x);
    auto gf = static_cast<const float*>(gamma);
    auto bf = static_cast<const float*>(beta);
    auto yf = static_cast<float*>(y);
    dim3 grid(otp_ceil_div(T, 256), B);
    if (C <= 17) hipLaunchKernelGGL(ln_channel_kernel<17>, grid, dim3(256), 0, st, xf, gf, bf, yf, C, T, eps);
    else if (C <= 136)
        hipLaunchKernelGGL(ln_channel_split_kernel<34>, dim3(otp_ceil_div(T, 64), B), dim3(256), 0, st, xf, gf, bf, yf, C, T, eps);
    else if (C <= 204)                                   // 12 x 17 stacked maps: the 7-frame window of BASELINE configs[4]
        hipLaunchKernelGGL(ln_channel_split_kernel<51>, dim3(otp_ceil_div(T, 64), B), dim3(256), 0, st, xf, gf, bf, yf, C, T, eps);
    else hipLaunchKernelGGL(ln_channel_kernel<0>, grid, dim3(256), 0, st, xf, gf, bf, yf, C, T, eps);
    if (pool) {
        int To = (T + 2 - 3) / 2 + 1;
        hipLaunchKernelGGL(maxpool3s2_kernel, dim3(otp_ceil_div(To, 256), B * C), dim3(256), 0, st, xf,
                           static_cast<float*>(pool), T, To);
    }
    return otp_launch_status();
}

extern "C" int otp_dwconv_ln3(const void* x, const void* dwq, const void* dwk, const void* dwv, const void* gq,
                              const void* bq, const void* gk, const void* bk, const void* gv, const void* bv,
                              void* q, void* k, void* v, int B, int C, int T, int stride, float eps, void* stream) {
    if (!x || !dwq || !dwk || !dwv || !gq || !bq || !gk || !bk || !gv || !bv || !q || !k || !v) return OTP_ERR_BAD_ARG;
    if (B <= 0 || C <= 0 || T <= 0 || stride <= 0) return OTP_ERR_BAD_ARG;
    const int To = (T + 2 - 3) / stride + 1;
    auto f = [](const void* p) { return static_cast<const float*>(p); };
    auto st = static_cast<hipStream_t>(stream);
#define OTP_DW_ARGS f(x), f(dwq), f(dwk), f(dwv), f(gq), f(bq), f(gk), f(bk), f(gv), f(bv), static_cast<float*>(q), \
                    static_cast<float*>(k), static_cast<float*>(v), C, T, To, stride, eps
    if (C <= 4 * 5)
        hipLaunchKernelGGL(dwconv_ln3_kernel<5>, dim3(otp_ceil_div(To, 64), B), dim3(256), 0, st, OTP_DW_ARGS);
    else if (C <= 4 * 34)
        hipLaunchKernelGGL(dwconv_ln3_kernel<34>, dim3(otp_ceil_div(To, 64), B), dim3(256), 0, st, OTP_DW_ARGS);
    else if (C <= 4 * 51)                                          // C = 204: the 7-frame window (the generic kernel took 370-450 us)
        hipLaunchKernelGGL(dwconv_ln3_kernel<51>, dim3(otp_ceil_div(To, 64), B), dim3(256), 0, st, OTP_DW_ARGS);
    else
        hipLaunchKernelGGL(dwconv_ln3_generic_kernel, dim3(otp_ceil_div(To, 256), B), dim3(256), 0, st, OTP_DW_ARGS);
#undef OTP_DW_ARGS
    return otp_launch_status();
}

extern "C" int otp_maxpool3s2_forward(const void* x, void* y, int rows, int T, void* stream) {
    if (!x || !y || rows <= 0 || T <= 0) return OTP_ERR_BAD_ARG;
    const int To = (T + 2 - 3) / 2 + 1;
    hipLaunchKernelGGL(maxpool3s2_kernel, dim3(otp_ceil_div(To, 256), rows), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const float*>(x), static_cast<float*>(y), T, To);
    return otp_launch_status();
}

extern "C" int otp_upsample_linear(const void* x, void* out, int B, int C, int T, int f, int out_ctot, int out_coff,
                                   void* stream) {
    if (!x || !out || B <= 0 || C <= 0 || T <= 0 || f <= 0 || out_ctot < out_coff + C) return OTP_ERR_BAD_ARG;
    const bool vec = (T * f) % 4 == 0 && (f > 1 || T % 4 == 0) &&
                     ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
    if (vec)
        hipLaunchKernelGGL(upsample_linear4_kernel, dim3(otp_ceil_div(T * f / 4, 256), B * C), dim3(256), 0,
                           static_cast<hipStream_t>(stream), static_cast<const float*>(x), static_cast<float*>(out), C, T,
                           f, out_ctot, out_coff);
    else
        hipLaunchKernelGGL(upsample_linear_kernel, dim3(otp_ceil_div(T * f, 256), B * C), dim3(256), 0,
                           static_cast<hipStream_t>(stream), static_cast<const float*>(x), static_cast<float*>(out), C, T,
                           f, out_ctot, out_coff);
    return otp_launch_status();
}
