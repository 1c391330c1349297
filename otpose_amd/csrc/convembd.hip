// Conv embedding of ConvTransformer (reference model/ConvVideoTransformer.py:60-78, 129-135): per embedding layer
//   z = Conv2d(Cin, Cout, ks, stride 1, padding ks / 2)(x)              x (B, Cin, H, W), zero padding
//   v = z (+ bias);  y = relu(LayerNorm_c(v)) (+ pe[c][t])               LayerNorm of model/blocks.py:95-110 over the channels
// as ONE launch that writes (B, Cout, T = H W) fp32: the convolution result never reaches HBM before the norm.
//
// GEMM view as in csrc/conv.hip: D[co][pixel] = sum_{tap, ci} Wp[tap][ci][co] X[ci][pixel shifted by tap] on the exact-fp32
// matrix cores (v_mfma_f32_16x16x4_f32: bit-equal to an fmaf chain, no split products - the LayerNorm divides by a standard
// deviation that is small when the weights are small).
//   * A workgroup (256 threads) owns CE_PT = 128 consecutive flattened pixels of one image and ALL output channels: the
//     LayerNorm is a reduction over the output-channel axis.  Its four waves are WM (over 16-channel blocks) x WP (over
//     16-pixel blocks); a wave holds MBW x PBW accumulator tiles, PBW = 2 WM.  Six instances cover Cout <= 16 .. 256.
//   * The input is staged in the LDS CE_CK = 8 channels at a time: per channel and tap ROW dy one segment of the flattened
//     plane, positions q0 + dy W - pad .. q0 + dy W + 127 + pad (zero outside [0, H W): the rows above / below the image).  The
//     staged size is ks (128 + 2 pad) words per channel whatever W is; a tap that crosses the left / right image edge is
//     masked per lane when the B fragment is read (one bit per pixel block and tap column, computed once).
//   * Weights come straight from L2 in the packed layout [tap][Cin4][CoutP] (zeros in the padding): a wave reads only the
//     rows of its own channel blocks, 64 bytes per lane group, and every fragment feeds PBW MFMAs.
//   * Epilogue on the accumulators: optional z store, bias, then mean first and centred sum of squares second like the
//     reference; the channel sums run over a lane's registers, the four k-slot lane groups, then the WM waves through the
//     LDS in a fixed order.
//
// Backward in front of the convolution's own gradients (otp_conv_embd_backward_pre): per token recompute mean, rstd, xhat from
// z, mask = gamma xhat + beta > 0, g' = gamma grad_y mask, grad_z = rstd (g' - mean_c g' - xhat mean_c(g' xhat)); a
// workgroup owns 64 tokens (lanes) x all channels (wave w: channels w, w + 4, ..), writes its partial sums of
// grad_gamma = sum g xhat and grad_beta = sum g, and a fold adds the partials in a fixed order: no atomics, bit-equal runs.
#include "common.h"

namespace {

constexpr int CE_THREADS = 256;
constexpr int CE_PT = 128;                         // pixels of a workgroup
constexpr int CE_CK = 8;                           // input channels staged at a time
constexpr int CE_MAXC = 256;

template <int KS>
struct ce_dims {
    static constexpr int PAD = KS / 2;
    static constexpr int SEGW = CE_PT + 2 * PAD;                   // staged positions of one (channel, tap row)
    static constexpr int SEGR = (SEGW + 3) & ~3;
    static constexpr int CS0 = KS * SEGR;
    static constexpr int CS = CS0 + (16 - CS0 % 64 + 64) % 64;     // channel stride = 16 mod 64: the four k-slot groups of a B read hit disjoint banks
    static constexpr int ITEMS = CE_CK * KS * SEGW;
    static constexpr int NIT = (ITEMS + CE_THREADS - 1) / CE_THREADS;
};

// channels c0 .. c0 + CE_CK - 1 of image `img` (rows of HW words) -> lds[cc][dy][j] = plane[q0 + (dy - PAD) W - PAD + j]
template <int KS>
__device__ __forceinline__ void ce_stage(const float* __restrict__ img, float* lds, int c0, int Cin, int W, int HW, int q0) {
    typedef ce_dims<KS> D;
    float r[D::NIT];
#pragma unroll
    for (int n = 0; n < D::NIT; ++n) {
        const int idx = n * CE_THREADS + (int)threadIdx.x;
        const int row = idx / D::SEGW, j = idx - row * D::SEGW;    // compile-time divisors
        const int cc = row / KS, dy = row - cc * KS;
        const int p = q0 + (dy - D::PAD) * W - D::PAD + j;
        const bool ok = idx < D::ITEMS && c0 + cc < Cin && p >= 0 && p < HW;
        r[n] = ok ? img[(size_t)(c0 + cc) * HW + p] : 0.f;
    }
#pragma unroll
    for (int n = 0; n < D::NIT; ++n) {
        const int idx = n * CE_THREADS + (int)threadIdx.x;
        const int row = idx / D::SEGW, j = idx - row * D::SEGW;
        const int cc = row / KS, dy = row - cc * KS;
        if (idx < D::ITEMS) lds[cc * D::CS + dy * D::SEGR + j] = r[n];
    }
}

// grid: B * tiles workgroups, tile = 128 flattened pixels of one image
template <int KS, int WM, int MBW>
__global__ __launch_bounds__(CE_THREADS) void conv_embd_kernel(const float* __restrict__ x, const float* __restrict__ wp,
                                                               const float* __restrict__ bias, const float* __restrict__ gamma,
                                                               const float* __restrict__ beta, const float* __restrict__ pe,
                                                               float* __restrict__ out, float* __restrict__ zout, int Cin, int Cin4,
                                                               int Cout, int W, int HW, int tiles, float eps) {
    typedef ce_dims<KS> D;
    constexpr int WP = 4 / WM, PBW = 2 * WM, CoutP = WM * MBW * 16;
    static_assert(WP * PBW * 16 == CE_PT, "the waves cover the pixel tile");
    __shared__ __attribute__((aligned(16))) float lds[CE_CK * D::CS];
    __shared__ float red[WM][CE_PT];
    const int lane = threadIdx.x & 63, i16 = lane & 15, kl = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wm = wave / WP, wpi = wave - wm * WP;
    const int b = blockIdx.x / tiles, q0 = (blockIdx.x - b * tiles) * CE_PT;
    const float* __restrict__ img = x + (size_t)b * Cin * HW;
    const int n0 = wpi * PBW * 16 + i16;                           // the lane's pixel of block 0 inside the tile

    // bit dx of cmask[pb]: tap column dx stays inside the image row for this lane's pixel of block pb
    unsigned cmask[PBW];
#pragma unroll
    for (int pb = 0; pb < PBW; ++pb) {
        const int xc = (q0 + n0 + pb * 16) % W;
        unsigned m = 0;
#pragma unroll
        for (int dx = 0; dx < KS; ++dx) m |= (xc + dx - D::PAD >= 0 && xc + dx - D::PAD < W) ? 1u << dx : 0u;
        cmask[pb] = m;
    }

    // blocked summation: the products of one staged chunk (CE_CK ks^2 terms) run as an MFMA chain in `part`, and the chunk sums
    // are added into `acc` - one chain over all Cin ks^2 terms (3400 at 136 channels and 5x5) carries several times the rounding
    // error of a vectorised fp32 convolution
    otp_f32x4 acc[MBW][PBW], part[MBW][PBW];
#pragma unroll
    for (int i = 0; i < MBW; ++i)
#pragma unroll
        for (int pb = 0; pb < PBW; ++pb) acc[i][pb] = otp_f32x4{0.f, 0.f, 0.f, 0.f};

    const size_t tap_stride = (size_t)Cin4 * CoutP;
    for (int c0 = 0; c0 < Cin4; c0 += CE_CK) {
        __syncthreads();                                           // the previous chunk's readers are done
        ce_stage<KS>(img, lds, c0, Cin, W, HW, q0);
        __syncthreads();
        const int nc4 = (Cin4 - c0 < CE_CK ? Cin4 - c0 : CE_CK) / 4;
#pragma unroll
        for (int i = 0; i < MBW; ++i)
#pragma unroll
            for (int pb = 0; pb < PBW; ++pb) part[i][pb] = otp_f32x4{0.f, 0.f, 0.f, 0.f};
        for (int c4 = 0; c4 < nc4; ++c4) {
            const float* lrow = lds + (c4 * 4 + kl) * D::CS + n0;
            const float* __restrict__ wrow = wp + (size_t)(c0 + c4 * 4 + kl) * CoutP + wm * 16 + i16;
#pragma unroll 1                                                     // (the tap rows stay a loop: 25 unrolled taps cost 5x5 a hundred registers)
            for (int dy = 0; dy < KS; ++dy)
#pragma unroll
                for (int dx = 0; dx < KS; ++dx) {
                    float a[MBW], bf[PBW];
#pragma unroll
                    for (int i = 0; i < MBW; ++i) a[i] = wrow[(dy * KS + dx) * tap_stride + i * WM * 16];
#pragma unroll
                    for (int pb = 0; pb < PBW; ++pb) {
                        const float v = lrow[dy * D::SEGR + pb * 16 + dx];
                        bf[pb] = (dx == D::PAD || ((cmask[pb] >> dx) & 1u)) ? v : 0.f;
                    }
#pragma unroll
                    for (int i = 0; i < MBW; ++i)
#pragma unroll
                        for (int pb = 0; pb < PBW; ++pb)
                            part[i][pb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], bf[pb], part[i][pb], 0, 0, 0);
                }
        }
#pragma unroll
        for (int i = 0; i < MBW; ++i)
#pragma unroll
            for (int pb = 0; pb < PBW; ++pb) acc[i][pb] += part[i][pb];
    }

    // ---- epilogue: acc[i][pb][r] is channel (wm + i WM) 16 + 4 kl + r of pixel q0 + n0 + 16 pb ---------------------------------
    const size_t obase = (size_t)b * Cout * HW;
    if (zout) {
#pragma unroll
        for (int i = 0; i < MBW; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int ch = (wm + i * WM) * 16 + 4 * kl + r;
#pragma unroll
                for (int pb = 0; pb < PBW; ++pb) {
                    const int q = q0 + n0 + pb * 16;
                    if (ch < Cout && q < HW) zout[obase + (size_t)ch * HW + q] = acc[i][pb][r];
                }
            }
    }
    if (bias) {
#pragma unroll
        for (int i = 0; i < MBW; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int ch = (wm + i * WM) * 16 + 4 * kl + r;
                const float bv = ch < Cout ? bias[ch] : 0.f;
#pragma unroll
                for (int pb = 0; pb < PBW; ++pb) acc[i][pb][r] += bv;
            }
    }
    if (gamma) {
        const float inv_c = 1.f / (float)Cout;
        float mean[PBW], rstd[PBW];
        // mean first (the padded channels hold exact zeros: zero weights, no bias)
#pragma unroll
        for (int pb = 0; pb < PBW; ++pb) {
            float s = 0.f;
#pragma unroll
            for (int i = 0; i < MBW; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r) s += acc[i][pb][r];
            s = otp_kslot_sum(s);
            if (kl == 0) red[wm][n0 + pb * 16] = s;
        }
        __syncthreads();
#pragma unroll
        for (int pb = 0; pb < PBW; ++pb) {
            float s = red[0][n0 + pb * 16];
#pragma unroll
            for (int m = 1; m < WM; ++m) s += red[m][n0 + pb * 16];
            mean[pb] = s * inv_c;
        }
        __syncthreads();
        // then the centred sum of squares
#pragma unroll
        for (int pb = 0; pb < PBW; ++pb) {
            float s = 0.f;
#pragma unroll
            for (int i = 0; i < MBW; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int ch = (wm + i * WM) * 16 + 4 * kl + r;
                    const float d = ch < Cout ? acc[i][pb][r] - mean[pb] : 0.f;
                    acc[i][pb][r] = d;
                    s = __builtin_fmaf(d, d, s);
                }
            s = otp_kslot_sum(s);
            if (kl == 0) red[wm][n0 + pb * 16] = s;
        }
        __syncthreads();
#pragma unroll
        for (int pb = 0; pb < PBW; ++pb) {
            float s = red[0][n0 + pb * 16];
#pragma unroll
            for (int m = 1; m < WM; ++m) s += red[m][n0 + pb * 16];
            rstd[pb] = 1.f / sqrtf(s * inv_c + eps);
        }
#pragma unroll
        for (int i = 0; i < MBW; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int ch = (wm + i * WM) * 16 + 4 * kl + r;
                const float g = ch < Cout ? gamma[ch] : 0.f, bt = ch < Cout ? beta[ch] : 0.f;
#pragma unroll
                for (int pb = 0; pb < PBW; ++pb) acc[i][pb][r] = acc[i][pb][r] * rstd[pb] * g + bt;
            }
    }
#pragma unroll
    for (int i = 0; i < MBW; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int ch = (wm + i * WM) * 16 + 4 * kl + r;
#pragma unroll
            for (int pb = 0; pb < PBW; ++pb) {
                const int q = q0 + n0 + pb * 16;
                if (ch < Cout && q < HW) {
                    float y = fmaxf(acc[i][pb][r], 0.f);
                    if (pe) y += pe[(size_t)ch * HW + q];
                    out[obase + (size_t)ch * HW + q] = y;
                }
            }
        }
}

// (Cout, Cin, ks, ks) -> [tap][Cin4][CoutP], zeros in the padding
__global__ void conv_embd_pack_kernel(const float* __restrict__ w, float* __restrict__ wp, int Cin, int Cin4, int Cout, int CoutP,
                                      int KK, size_t total) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int co = (int)(i % CoutP);
    const size_t row = i / CoutP;
    const int ci = (int)(row % Cin4), tap = (int)(row / Cin4);
    wp[i] = (ci < Cin && co < Cout) ? w[((size_t)co * Cin + ci) * KK + tap] : 0.f;
}

// ---- backward in front of the convolution's gradients ----------------------------------------------------------------------------
// grid (ceil(T / 64), B); lane = token, wave w owns channels w, w + 4, ...; partial[(wg * 2 + {0, 1}) * C + c]
__global__ __launch_bounds__(256) void conv_embd_bwd_ln_kernel(const float* __restrict__ z, const float* __restrict__ bias,
                                                               const float* __restrict__ gamma, const float* __restrict__ beta,
                                                               const float* __restrict__ gy, float* __restrict__ gz,
                                                               float* __restrict__ partial, int C, int T, float eps) {
    __shared__ float red[2][4][64];
    const int lane = threadIdx.x & 63;
    const int cg = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int t = blockIdx.x * 64 + lane;
    const bool ok = t < T;
    const size_t base = (size_t)blockIdx.y * C * T + (ok ? t : 0);
    const size_t wg = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
    const float inv_c = 1.f / (float)C;
    auto fold4 = [&](int k) { return ((red[k][0][lane] + red[k][1][lane]) + red[k][2][lane]) + red[k][3][lane]; };

    float s = 0.f;
    for (int c = cg; c < C; c += 4) s += z[base + (size_t)c * T] + (bias ? bias[c] : 0.f);
    red[0][cg][lane] = s;
    __syncthreads();
    const float mean = fold4(0) * inv_c;
    s = 0.f;
    for (int c = cg; c < C; c += 4) {
        const float d = z[base + (size_t)c * T] + (bias ? bias[c] : 0.f) - mean;
        s = __builtin_fmaf(d, d, s);
    }
    red[1][cg][lane] = s;
    __syncthreads();
    const float rstd = 1.f / sqrtf(fold4(1) * inv_c + eps);
    __syncthreads();                                               // both slots are read: reuse them
    float sa = 0.f, sb = 0.f;
    for (int c = cg; c < C; c += 4) {
        const float xh = (z[base + (size_t)c * T] + (bias ? bias[c] : 0.f) - mean) * rstd;
        const float g = (xh * gamma[c] + beta[c] > 0.f) ? gy[base + (size_t)c * T] : 0.f;
        const float gp = g * gamma[c];
        sa += gp;
        sb = __builtin_fmaf(gp, xh, sb);
    }
    red[0][cg][lane] = sa;
    red[1][cg][lane] = sb;
    __syncthreads();
    const float ma = fold4(0) * inv_c, mb = fold4(1) * inv_c;
    for (int c = cg; c < C; c += 4) {                              // wave-uniform trip count: the wave sums below are whole
        const float xh = (z[base + (size_t)c * T] + (bias ? bias[c] : 0.f) - mean) * rstd;
        float g = (xh * gamma[c] + beta[c] > 0.f) ? gy[base + (size_t)c * T] : 0.f;
        if (!ok) g = 0.f;
        const float gp = g * gamma[c];
        if (ok) gz[base + (size_t)c * T] = rstd * (gp - ma - xh * mb);
        const float pg = wave_sum(g * xh), pb = wave_sum(g);
        if (lane == 0) {
            partial[(wg * 2 + 0) * C + c] = pg;
            partial[(wg * 2 + 1) * C + c] = pb;
        }
    }
}

// grid C, 64 threads: lane l adds workgroups l, l + 64, ... in order, then the wave sum (fixed order)
__global__ __launch_bounds__(64) void conv_embd_bwd_fold_kernel(const float* __restrict__ partial, float* __restrict__ ggamma,
                                                                float* __restrict__ gbeta, int C, int nwg) {
    const int c = blockIdx.x;
    float a = 0.f, b = 0.f;
    for (int w = threadIdx.x; w < nwg; w += 64) {
        a += partial[((size_t)w * 2 + 0) * C + c];
        b += partial[((size_t)w * 2 + 1) * C + c];
    }
    a = wave_sum(a);
    b = wave_sum(b);
    if (threadIdx.x == 0) {
        if (ggamma) ggamma[c] = a;
        if (gbeta) gbeta[c] = b;
    }
}

// no LayerNorm: grad_z = grad_y * (z + bias > 0)
__global__ void conv_embd_bwd_relu_kernel(const float* __restrict__ z, const float* __restrict__ bias, const float* __restrict__ gy,
                                          float* __restrict__ gz, int C, int T, size_t total) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int c = (int)((i / T) % C);
    gz[i] = (z[i] + (bias ? bias[c] : 0.f) > 0.f) ? gy[i] : 0.f;
}

bool ce_channels_ok(int Cin, int Cout, int ks) {
    return (ks == 1 || ks == 3 || ks == 5) && Cin >= 1 && Cin <= CE_MAXC && Cout >= 1 && Cout <= CE_MAXC;
}
bool ce_shape_ok(int B, int Cin, int H, int W, int Cout, int ks) {
    if (!ce_channels_ok(Cin, Cout, ks) || B < 1 || H < 1 || W < 1) return false;
    const long long hw = (long long)H * W;                         // pixel indices, q0 + dy W and the grid stay inside an int
    return hw <= (1ll << 30) && (long long)B * ((hw + CE_PT - 1) / CE_PT) <= 0x7fffffffll;
}
// the instance of a Cout: WM, MBW (CoutP = 16 WM MBW)
void ce_config(int Cout, int& WM, int& MBW) {
    if (Cout <= 16) WM = 1, MBW = 1;
    else if (Cout <= 32) WM = 2, MBW = 1;
    else WM = 4, MBW = (Cout + 63) / 64;
}

struct ce_args {
    const float *x, *wp, *bias, *gamma, *beta, *pe;
    float *out, *z;
    int Cin, Cin4, Cout, W, HW, tiles;
    float eps;
    dim3 grid;
    hipStream_t st;
};

template <int KS, int WM, int MBW>
void ce_launch(const ce_args& a) {
    hipLaunchKernelGGL((conv_embd_kernel<KS, WM, MBW>), a.grid, dim3(CE_THREADS), 0, a.st, a.x, a.wp, a.bias, a.gamma, a.beta, a.pe,
                       a.out, a.z, a.Cin, a.Cin4, a.Cout, a.W, a.HW, a.tiles, a.eps);
}
template <int KS>
void ce_dispatch(const ce_args& a) {
    int WM, MBW;
    ce_config(a.Cout, WM, MBW);
    if (WM == 1) ce_launch<KS, 1, 1>(a);
    else if (WM == 2) ce_launch<KS, 2, 1>(a);
    else if (MBW == 1) ce_launch<KS, 4, 1>(a);
    else if (MBW == 2) ce_launch<KS, 4, 2>(a);
    else if (MBW == 3) ce_launch<KS, 4, 3>(a);
    else ce_launch<KS, 4, 4>(a);
}

}  // namespace

extern "C" int otp_conv_embd_supported(int B, int Cin, int H, int W, int Cout, int ks) { return ce_shape_ok(B, Cin, H, W, Cout, ks); }

extern "C" size_t otp_conv_embd_weight_bytes(int Cin, int Cout, int ks) {
    if (!ce_channels_ok(Cin, Cout, ks)) return 0;
    int WM, MBW;
    ce_config(Cout, WM, MBW);
    return (size_t)ks * ks * ((Cin + 3) & ~3) * (WM * MBW * 16) * sizeof(float);
}

extern "C" int otp_conv_embd_pack_weight(const void* weight, void* wpacked, int Cin, int Cout, int ks, void* stream) {
    if (!weight || !wpacked || !ce_channels_ok(Cin, Cout, ks)) return OTP_ERR_BAD_ARG;
    int WM, MBW;
    ce_config(Cout, WM, MBW);
    const int Cin4 = (Cin + 3) & ~3, CoutP = WM * MBW * 16;
    const size_t total = (size_t)ks * ks * Cin4 * CoutP;
    hipLaunchKernelGGL(conv_embd_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const float*>(weight), static_cast<float*>(wpacked), Cin, Cin4, Cout, CoutP, ks * ks, total);
    return otp_launch_status();
}

extern "C" int otp_conv_embd(const void* x, const void* wpacked, const void* bias, const void* gamma, const void* beta,
                             const void* pe, void* out, void* z, int B, int Cin, int H, int W, int Cout, int ks, float eps,
                             void* stream) {
    if (!x || !wpacked || !out || (gamma == nullptr) != (beta == nullptr) || !ce_shape_ok(B, Cin, H, W, Cout, ks) || !(eps >= 0.f))
        return OTP_ERR_BAD_ARG;
    ce_args a;
    a.x = static_cast<const float*>(x), a.wp = static_cast<const float*>(wpacked), a.bias = static_cast<const float*>(bias);
    a.gamma = static_cast<const float*>(gamma), a.beta = static_cast<const float*>(beta), a.pe = static_cast<const float*>(pe);
    a.out = static_cast<float*>(out), a.z = static_cast<float*>(z);
    a.Cin = Cin, a.Cin4 = (Cin + 3) & ~3, a.Cout = Cout, a.W = W, a.HW = H * W, a.tiles = otp_ceil_div(H * W, CE_PT), a.eps = eps;
    a.grid = dim3((unsigned)(B * a.tiles));
    a.st = static_cast<hipStream_t>(stream);
    if (ks == 1) ce_dispatch<1>(a);
    else if (ks == 3) ce_dispatch<3>(a);
    else ce_dispatch<5>(a);
    return otp_launch_status();
}

static bool ce_bwd_shape_ok(int B, int C, int T) {
    return B >= 1 && B <= 65535 && C >= 1 && C <= CE_MAXC && T >= 1 && T <= (1 << 30);
}

// the per-workgroup partial sums of grad_gamma and grad_beta
extern "C" size_t otp_conv_embd_backward_pre_workspace(int B, int C, int T) {
    if (!ce_bwd_shape_ok(B, C, T)) return 0;
    return (size_t)B * otp_ceil_div(T, 64) * 2 * C * sizeof(float);
}

extern "C" int otp_conv_embd_backward_pre(const void* z, const void* bias, const void* gamma, const void* beta, const void* grad_y,
                                          void* grad_z, void* grad_gamma, void* grad_beta, void* ws, size_t ws_bytes, int B, int C,
                                          int T, float eps, void* stream) {
    if (!z || !grad_y || !grad_z || (gamma == nullptr) != (beta == nullptr) || !ce_bwd_shape_ok(B, C, T) || !(eps >= 0.f))
        return OTP_ERR_BAD_ARG;
    auto st = static_cast<hipStream_t>(stream);
    const float *zf = static_cast<const float*>(z), *bf = static_cast<const float*>(bias), *gf = static_cast<const float*>(grad_y);
    if (!gamma) {
        if (grad_gamma || grad_beta) return OTP_ERR_BAD_ARG;
        const size_t total = (size_t)B * C * T;
        if ((total + 255) / 256 > 0x7fffffffull) return OTP_ERR_BAD_ARG;
        hipLaunchKernelGGL(conv_embd_bwd_relu_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, zf, bf, gf,
                           static_cast<float*>(grad_z), C, T, total);
        return otp_launch_status();
    }
    if (!ws) return OTP_ERR_BAD_ARG;
    if (ws_bytes < otp_conv_embd_backward_pre_workspace(B, C, T)) return OTP_ERR_WORKSPACE;
    const int tiles = otp_ceil_div(T, 64);
    hipLaunchKernelGGL(conv_embd_bwd_ln_kernel, dim3(tiles, B), dim3(256), 0, st, zf, bf, static_cast<const float*>(gamma),
                       static_cast<const float*>(beta), gf, static_cast<float*>(grad_z), static_cast<float*>(ws), C, T, eps);
    if (grad_gamma || grad_beta)
        hipLaunchKernelGGL(conv_embd_bwd_fold_kernel, dim3(C), dim3(64), 0, st, static_cast<const float*>(ws),
                           static_cast<float*>(grad_gamma), static_cast<float*>(grad_beta), C, B * tiles);
    return otp_launch_status();
}
