// RSN attention (Pose Refine Machine) and weight vector, reference model/RSB.py:142-203, behind include/otpose_hip.h.  Exact fp32,
// no float atomics: every sum runs in a fixed order, so two runs are bit-equal.
//
// Inference (BatchNorm folded into a per-channel scale / shift):
//   otp_prm_gate   per-(n, c) mean of f over H W, two 1x1 conv + BN + ReLU layers on the C-vector, sigmoid         -> gate_c (N, C)
//   otp_prm_apply  t = ReLU(BN(1x1(f))) on a tile with a 4-pixel halo IN THE LDS ONLY, depthwise 9x9 + BN + ReLU + sigmoid from the
//                  LDS, out = f (1 + gate_c gate_s): neither t nor the spatial gate reaches HBM
// Training (batch statistics, layer by layer): spatial mean, depthwise k x k conv (k = 9) and the combine, forward and backward.
#include "common.h"

namespace {

constexpr int PRM_MAXC = 64;
// the output tile of otp_prm_apply and of the depthwise kernels: 8 rows of 32 pixels, one pixel per thread.  A 32-lane half of a
// wave reads 32 consecutive dwords of one LDS row at every tap: ds_read_b32 banks are (a / 4) % 32 per half, so no tap conflicts.
constexpr int PRM_TH = 8, PRM_TW = 32, PRM_K = 9, PRM_HALO = PRM_K / 2;
constexpr int PRM_LH = PRM_TH + 2 * PRM_HALO, PRM_LW = PRM_TW + 2 * PRM_HALO, PRM_LPIX = PRM_LH * PRM_LW;   // 16 x 40 = 640
constexpr int PRM_THREADS = PRM_TH * PRM_TW;                                                                // 256
constexpr int PRM_TAPS = PRM_K * PRM_K;

__device__ __forceinline__ float prm_sigmoid(float v) { return 1.f / (1.f + expf(-v)); }

// sum over the 256 threads of a workgroup in a fixed order: wave sums, then the four wave results in order.  `red`: 4 doubles of LDS.
// Every thread returns the total.  The sums that feed the channel gate run in double: the gate's BatchNorm normalises N values per
// channel in training, and its 1 / sigma multiplies every rounding error of the means in front of it.
__device__ __forceinline__ double prm_block_sum(double v, double* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();                                               // (red may still be read from the previous call)
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// ---- spatial mean: grid (C, N), 256 threads; thread t adds elements t, t + 256, ... in order, in double ---------------------------------------
__global__ __launch_bounds__(PRM_THREADS) void prm_mean_kernel(const float* __restrict__ f, float* __restrict__ mean, int C, int HW,
                                                               float hw) {
    __shared__ double red[4];
    const float* p = f + ((size_t)blockIdx.y * C + blockIdx.x) * HW;
    double s = 0.0;
    for (int i = threadIdx.x; i < HW; i += PRM_THREADS) s += (double)p[i];
    s = prm_block_sum(s, red);
    if (threadIdx.x == 0) mean[(size_t)blockIdx.y * C + blockIdx.x] = (float)(s / (double)hw);
}

// the two 1x1 layers on the C-vector that `gate` holds (the means), in place: grid N, 64 threads, thread o owns output channel o
__global__ __launch_bounds__(64) void prm_gate_kernel(float* __restrict__ gate, const float* __restrict__ w1, const float* __restrict__ sc1,
                                                      const float* __restrict__ sh1, const float* __restrict__ w2,
                                                      const float* __restrict__ sc2, const float* __restrict__ sh2, int C, int residual) {
    __shared__ float v0[PRM_MAXC], v1[PRM_MAXC];
    const int o = threadIdx.x;
    float* g = gate + (size_t)blockIdx.x * C;
    if (o < C) v0[o] = g[o];
    __syncthreads();
    if (o < C) {
        float a = 0.f;
        for (int i = 0; i < C; ++i) a = fmaf(w1[o * C + i], v0[i], a);
        const float y = fmaxf(fmaf(sc1[o], a, sh1[o]), 0.f);
        v1[o] = residual ? y + v0[o] : y;                          // out_1 + out_0 of RSN_WEIGHT_VECTOR (RSB.py:162)
    }
    __syncthreads();
    if (o < C) {
        float a = 0.f;
        for (int i = 0; i < C; ++i) a = fmaf(w2[o * C + i], v1[i], a);
        g[o] = prm_sigmoid(fmaxf(fmaf(sc2[o], a, sh2[o]), 0.f));
    }
}

// ---- the fused spatial gate ---------------------------------------------------------------------------------------------------------
// grid (tiles, N), 256 threads.  The output channels go through the LDS in chunks of OC: for a chunk, every halo pixel's OC values of
// t are formed from the C input channels of f (OC register accumulators, the chunk's 1x1 weights in the LDS as [Cin][OC], f read
// through the cache: a tile's f is 640 pixels x C channels, re-read once per chunk), pixels outside the image are 0 - the zero
// padding of the 9x9 applies to t, not to f.  Then thread (ty, tx) runs the 81 taps of its pixel for each channel of the chunk.
template <int OC>
__global__ __launch_bounds__(PRM_THREADS) void prm_apply_kernel(const float* __restrict__ f, const float* __restrict__ gate,
                                                                const float* __restrict__ w31, const float* __restrict__ sc31,
                                                                const float* __restrict__ sh31, const float* __restrict__ w32,
                                                                const float* __restrict__ sc32, const float* __restrict__ sh32,
                                                                float* __restrict__ out, int C, int H, int W, int tiles_x) {
    __shared__ float t[OC * PRM_LPIX];
    __shared__ float wl[PRM_MAXC * OC];
    __shared__ float wd[OC * PRM_TAPS];
    const int tid = threadIdx.x, n = blockIdx.y;
    const int y0 = (blockIdx.x / tiles_x) * PRM_TH, x0 = (blockIdx.x % tiles_x) * PRM_TW;
    const int ty = tid / PRM_TW, tx = tid % PRM_TW;
    const int oy = y0 + ty, ox = x0 + tx;
    const bool valid = oy < H && ox < W;
    const size_t HW = (size_t)H * W;
    const float* fn = f + (size_t)n * C * HW;
    for (int c0 = 0; c0 < C; c0 += OC) {
        __syncthreads();                                           // the previous chunk's taps are done with t and wd
        for (int e = tid; e < C * OC; e += PRM_THREADS) {
            const int i = e / OC, oo = e % OC;
            wl[e] = (c0 + oo < C) ? w31[(c0 + oo) * C + i] : 0.f;
        }
        for (int e = tid; e < OC * PRM_TAPS; e += PRM_THREADS) wd[e] = (c0 + e / PRM_TAPS < C) ? w32[c0 * PRM_TAPS + e] : 0.f;
        __syncthreads();
        for (int p = tid; p < PRM_LPIX; p += PRM_THREADS) {
            const int gy = y0 - PRM_HALO + p / PRM_LW, gx = x0 - PRM_HALO + p % PRM_LW;
            const bool inside = gy >= 0 && gy < H && gx >= 0 && gx < W;
            float acc[OC];
#pragma unroll
            for (int oo = 0; oo < OC; ++oo) acc[oo] = 0.f;
            if (inside) {
                const float* fp = fn + (size_t)gy * W + gx;
                for (int i = 0; i < C; ++i) {
                    const float v = fp[(size_t)i * HW];
#pragma unroll
                    for (int oo = 0; oo < OC; ++oo) acc[oo] = fmaf(wl[i * OC + oo], v, acc[oo]);
                }
            }
#pragma unroll
            for (int oo = 0; oo < OC; ++oo) {
                const int c = min(c0 + oo, C - 1);                 // (slots past C hold zero weights; their t is never read)
                t[oo * PRM_LPIX + p] = inside ? fmaxf(fmaf(sc31[c], acc[oo], sh31[c]), 0.f) : 0.f;
            }
        }
        __syncthreads();
        const int nc = min(OC, C - c0);
        for (int oo = 0; oo < nc; ++oo) {
            const float* tp = t + oo * PRM_LPIX + ty * PRM_LW + tx;
            const float* wp = wd + oo * PRM_TAPS;
            float s = 0.f;
#pragma unroll
            for (int dy = 0; dy < PRM_K; ++dy) {                   // one fmaf chain per row of taps, the nine rows added in order
                float r = 0.f;
#pragma unroll
                for (int dx = 0; dx < PRM_K; ++dx) r = fmaf(wp[dy * PRM_K + dx], tp[dy * PRM_LW + dx], r);
                s += r;
            }
            if (valid) {
                const int c = c0 + oo;
                const float gs = prm_sigmoid(fmaxf(fmaf(sc32[c], s, sh32[c]), 0.f));
                const size_t at = ((size_t)n * C + c) * HW + (size_t)oy * W + ox;
                out[at] = f[at] * fmaf(gate[(size_t)n * C + c], gs, 1.f);
            }
        }
    }
}

// ---- depthwise 9x9, pad 4: grid (tiles, N C).  FLIP: the taps reversed (the input gradient as a gather) ------------------------------
__global__ __launch_bounds__(PRM_THREADS) void prm_dwconv_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                                 const float* __restrict__ bias, float* __restrict__ y, int C, int H,
                                                                 int W, int tiles_x, int flip) {
    __shared__ float xs[PRM_LPIX];
    __shared__ float wd[PRM_TAPS];
    const int tid = threadIdx.x, c = blockIdx.y % C;
    const int y0 = (blockIdx.x / tiles_x) * PRM_TH, x0 = (blockIdx.x % tiles_x) * PRM_TW;
    const float* xp = x + (size_t)blockIdx.y * H * W;
    if (tid < PRM_TAPS) wd[tid] = w[c * PRM_TAPS + (flip ? PRM_TAPS - 1 - tid : tid)];
    for (int p = tid; p < PRM_LPIX; p += PRM_THREADS) {
        const int gy = y0 - PRM_HALO + p / PRM_LW, gx = x0 - PRM_HALO + p % PRM_LW;
        xs[p] = (gy >= 0 && gy < H && gx >= 0 && gx < W) ? xp[(size_t)gy * W + gx] : 0.f;
    }
    __syncthreads();
    const int ty = tid / PRM_TW, tx = tid % PRM_TW, oy = y0 + ty, ox = x0 + tx;
    const float* tp = xs + ty * PRM_LW + tx;
    float s = 0.f;
#pragma unroll
    for (int dy = 0; dy < PRM_K; ++dy) {
        float r = 0.f;
#pragma unroll
        for (int dx = 0; dx < PRM_K; ++dx) r = fmaf(wd[dy * PRM_K + dx], tp[dy * PRM_LW + dx], r);
        s += r;
    }
    if (oy < H && ox < W) y[(size_t)blockIdx.y * H * W + (size_t)oy * W + ox] = bias ? s + bias[c] : s;
}

// weight gradient, per-workgroup partials: grid (tiles, N C); partial[c][n tiles + tile][81] = sum over the tile of gy x(shifted)
__global__ __launch_bounds__(PRM_THREADS) void prm_dwconv_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ gy,
                                                                       float* __restrict__ partial, int C, int H, int W, int tiles_x,
                                                                       int slots) {
    __shared__ float xs[PRM_LPIX];
    __shared__ float red[4 * PRM_TAPS];
    const int tid = threadIdx.x, c = blockIdx.y % C, n = blockIdx.y / C;
    const int y0 = (blockIdx.x / tiles_x) * PRM_TH, x0 = (blockIdx.x % tiles_x) * PRM_TW;
    const float* xp = x + (size_t)blockIdx.y * H * W;
    for (int p = tid; p < PRM_LPIX; p += PRM_THREADS) {
        const int py = y0 - PRM_HALO + p / PRM_LW, px = x0 - PRM_HALO + p % PRM_LW;
        xs[p] = (py >= 0 && py < H && px >= 0 && px < W) ? xp[(size_t)py * W + px] : 0.f;
    }
    __syncthreads();
    const int ty = tid / PRM_TW, tx = tid % PRM_TW, oy = y0 + ty, ox = x0 + tx;
    const float g = (oy < H && ox < W) ? gy[(size_t)blockIdx.y * H * W + (size_t)oy * W + ox] : 0.f;
    const float* tp = xs + ty * PRM_LW + tx;
    const int wave = tid >> 6, lane = tid & 63;
    for (int k = 0; k < PRM_TAPS; ++k) {
        const float v = wave_sum(g * tp[(k / PRM_K) * PRM_LW + k % PRM_K]);
        if (lane == 0) red[wave * PRM_TAPS + k] = v;
    }
    __syncthreads();
    if (tid < PRM_TAPS) {
        const size_t slot = (size_t)n * gridDim.x + blockIdx.x;
        partial[((size_t)c * slots + slot) * PRM_TAPS + tid] =
            ((red[tid] + red[PRM_TAPS + tid]) + red[2 * PRM_TAPS + tid]) + red[3 * PRM_TAPS + tid];
    }
}

// grid (81, C), 64 threads: lane l adds slots l, l + 64, ... in order, then the wave sum
__global__ __launch_bounds__(64) void prm_dwconv_wgrad_fold_kernel(const float* __restrict__ partial, float* __restrict__ gw, int slots) {
    const int k = blockIdx.x, c = blockIdx.y;
    float a = 0.f;
    for (int s = threadIdx.x; s < slots; s += 64) a += partial[((size_t)c * slots + s) * PRM_TAPS + k];
    a = wave_sum(a);
    if (threadIdx.x == 0) gw[c * PRM_TAPS + k] = a;
}

// ---- spatial mean backward: grid (N C, ceil(HW / 256)) ------------------------------------------------------------------------------
__global__ __launch_bounds__(PRM_THREADS) void prm_mean_bwd_kernel(const float* __restrict__ g, float* __restrict__ gx, int HW, float hw) {
    const int i = blockIdx.y * PRM_THREADS + threadIdx.x;
    if (i < HW) gx[(size_t)blockIdx.x * HW + i] = g[blockIdx.x] / hw;
}

// ---- combine: out = f (1 + sigmoid(a[n, c]) sigmoid(s)); grid N C, 256 threads walking the plane ------------------------------------
__global__ __launch_bounds__(PRM_THREADS) void prm_combine_kernel(const float* __restrict__ f, const float* __restrict__ a,
                                                                  const float* __restrict__ s, float* __restrict__ out, int HW) {
    const size_t base = (size_t)blockIdx.x * HW;
    const float sa = prm_sigmoid(a[blockIdx.x]);
    for (int i = threadIdx.x; i < HW; i += PRM_THREADS) out[base + i] = f[base + i] * fmaf(sa, prm_sigmoid(s[base + i]), 1.f);
}

// grad_f = g (1 + sa ss), grad_s = g f sa ss (1 - ss), grad_a[n, c] = sa (1 - sa) sum_hw g f ss (thread-strided sums, then the
// workgroup sum in a fixed order)
__global__ __launch_bounds__(PRM_THREADS) void prm_combine_bwd_kernel(const float* __restrict__ f, const float* __restrict__ a,
                                                                      const float* __restrict__ s, const float* __restrict__ g,
                                                                      float* __restrict__ gf, float* __restrict__ ga,
                                                                      float* __restrict__ gs, int HW) {
    __shared__ double red[4];
    const size_t base = (size_t)blockIdx.x * HW;
    const float sa = prm_sigmoid(a[blockIdx.x]);
    double acc = 0.0;
    for (int i = threadIdx.x; i < HW; i += PRM_THREADS) {
        const float ss = prm_sigmoid(s[base + i]), gv = g[base + i], gfv = gv * f[base + i];
        gf[base + i] = gv * fmaf(sa, ss, 1.f);
        gs[base + i] = gfv * sa * ss * (1.f - ss);
        acc += (double)gfv * (double)ss;
    }
    acc = prm_block_sum(acc, red);
    if (threadIdx.x == 0) ga[blockIdx.x] = (float)((double)(sa * (1.f - sa)) * acc);
}

// planes of H x W and tiles of 8 x 32 whose counts fit the grid; every in-plane offset fits an int
bool prm_plane_ok(long long planes, int H, int W) {
    if (planes < 1 || H < 1 || W < 1 || (long long)H * W > (1ll << 30)) return false;
    const long long tiles = (long long)otp_ceil_div(H, PRM_TH) * otp_ceil_div(W, PRM_TW);
    return planes <= 65535 && tiles <= 0x7fffffffll;
}
// one workgroup per (n, c) plane in grid.x, the plane in 256-element steps in grid.y
bool prm_flat_ok(long long planes, long long HW) {
    return planes >= 1 && planes <= 0x7fffffffll && HW >= 1 && HW <= (1ll << 30) && (HW + PRM_THREADS - 1) / PRM_THREADS <= 65535;
}
int prm_chunk(int C) {                                              // 8 or 16 output channels per pass: the fewer padded slots
    return ((C + 7) / 8) * 8 < ((C + 15) / 16) * 16 ? 8 : 16;
}

}  // namespace

extern "C" int otp_prm_supported(int C, int H, int W) { return C >= 1 && C <= PRM_MAXC && prm_plane_ok(1, H, W); }

extern "C" int otp_spatial_mean(const void* x, void* mean, int N, int C, int HW, void* stream) {
    if (!x || !mean || N < 1 || C < 1 || N > 65535 || !prm_flat_ok((long long)N * C, HW)) return OTP_ERR_BAD_ARG;
    hipLaunchKernelGGL(prm_mean_kernel, dim3(C, N), dim3(PRM_THREADS), 0, static_cast<hipStream_t>(stream),
                       static_cast<const float*>(x), static_cast<float*>(mean), C, HW, (float)HW);
    return otp_launch_status();
}

extern "C" int otp_spatial_mean_backward(const void* grad_mean, void* grad_x, int N, int C, int HW, void* stream) {
    if (!grad_mean || !grad_x || N < 1 || C < 1 || !prm_flat_ok((long long)N * C, HW)) return OTP_ERR_BAD_ARG;
    hipLaunchKernelGGL(prm_mean_bwd_kernel, dim3(N * C, otp_ceil_div(HW, PRM_THREADS)), dim3(PRM_THREADS), 0,
                       static_cast<hipStream_t>(stream), static_cast<const float*>(grad_mean), static_cast<float*>(grad_x), HW,
                       (float)HW);
    return otp_launch_status();
}

extern "C" int otp_prm_gate(const void* f, const void* w1, const void* scale1, const void* shift1, const void* w2, const void* scale2,
                            const void* shift2, void* gate, int N, int C, int HW, int residual, void* stream) {
    if (!f || !w1 || !scale1 || !shift1 || !w2 || !scale2 || !shift2 || !gate || C < 1 || C > PRM_MAXC || N < 1 || N > 65535 ||
        !prm_flat_ok((long long)N * C, HW))
        return OTP_ERR_BAD_ARG;
    auto st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(prm_mean_kernel, dim3(C, N), dim3(PRM_THREADS), 0, st, static_cast<const float*>(f), static_cast<float*>(gate),
                       C, HW, (float)HW);
    hipLaunchKernelGGL(prm_gate_kernel, dim3(N), dim3(64), 0, st, static_cast<float*>(gate), static_cast<const float*>(w1),
                       static_cast<const float*>(scale1), static_cast<const float*>(shift1), static_cast<const float*>(w2),
                       static_cast<const float*>(scale2), static_cast<const float*>(shift2), C, residual ? 1 : 0);
    return otp_launch_status();
}

extern "C" int otp_prm_apply(const void* f, const void* gate, const void* w31, const void* scale31, const void* shift31,
                             const void* w32, const void* scale32, const void* shift32, void* out, int N, int C, int H, int W,
                             void* stream) {
    if (!f || !gate || !w31 || !scale31 || !shift31 || !w32 || !scale32 || !shift32 || !out || f == out || N < 1 || N > 65535 ||
        !otp_prm_supported(C, H, W))
        return OTP_ERR_BAD_ARG;
    const int tiles_x = otp_ceil_div(W, PRM_TW);
    const dim3 grid(tiles_x * otp_ceil_div(H, PRM_TH), N);
    auto st = static_cast<hipStream_t>(stream);
#define PRM_APPLY(OC)                                                                                                              \
    hipLaunchKernelGGL(prm_apply_kernel<OC>, grid, dim3(PRM_THREADS), 0, st, static_cast<const float*>(f),                          \
                       static_cast<const float*>(gate), static_cast<const float*>(w31), static_cast<const float*>(scale31),         \
                       static_cast<const float*>(shift31), static_cast<const float*>(w32), static_cast<const float*>(scale32),      \
                       static_cast<const float*>(shift32), static_cast<float*>(out), C, H, W, tiles_x)
    if (prm_chunk(C) == 8) PRM_APPLY(8);
    else PRM_APPLY(16);
#undef PRM_APPLY
    return otp_launch_status();
}

extern "C" int otp_dwconv2d(const void* x, const void* weight, const void* bias, void* y, int N, int C, int H, int W, int ks, int flip,
                            void* stream) {
    if (!x || !weight || !y || x == y || ks != PRM_K || N < 1 || C < 1 || !prm_plane_ok((long long)N * C, H, W)) return OTP_ERR_BAD_ARG;
    const int tiles_x = otp_ceil_div(W, PRM_TW);
    hipLaunchKernelGGL(prm_dwconv_kernel, dim3(tiles_x * otp_ceil_div(H, PRM_TH), N * C), dim3(PRM_THREADS), 0,
                       static_cast<hipStream_t>(stream), static_cast<const float*>(x), static_cast<const float*>(weight),
                       static_cast<const float*>(bias), static_cast<float*>(y), C, H, W, tiles_x, flip ? 1 : 0);
    return otp_launch_status();
}

extern "C" size_t otp_dwconv2d_wgrad_workspace(int N, int C, int H, int W, int ks) {
    if (ks != PRM_K || N < 1 || C < 1 || !prm_plane_ok((long long)N * C, H, W)) return 0;
    return (size_t)C * N * otp_ceil_div(W, PRM_TW) * otp_ceil_div(H, PRM_TH) * PRM_TAPS * sizeof(float);
}

extern "C" int otp_dwconv2d_wgrad(const void* x, const void* grad_y, void* grad_weight, void* ws, size_t ws_bytes, int N, int C, int H,
                                  int W, int ks, void* stream) {
    if (!x || !grad_y || !grad_weight || !ws) return OTP_ERR_BAD_ARG;
    const size_t need = otp_dwconv2d_wgrad_workspace(N, C, H, W, ks);
    if (!need) return OTP_ERR_BAD_ARG;
    if (ws_bytes < need) return OTP_ERR_WORKSPACE;
    const int tiles_x = otp_ceil_div(W, PRM_TW), tiles = tiles_x * otp_ceil_div(H, PRM_TH);
    if ((long long)N * tiles > 0x7fffffffll) return OTP_ERR_BAD_ARG;
    auto st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(prm_dwconv_wgrad_kernel, dim3(tiles, N * C), dim3(PRM_THREADS), 0, st, static_cast<const float*>(x),
                       static_cast<const float*>(grad_y), static_cast<float*>(ws), C, H, W, tiles_x, N * tiles);
    hipLaunchKernelGGL(prm_dwconv_wgrad_fold_kernel, dim3(PRM_TAPS, C), dim3(64), 0, st, static_cast<const float*>(ws),
                       static_cast<float*>(grad_weight), N * tiles);
    return otp_launch_status();
}

extern "C" int otp_prm_combine(const void* f, const void* a, const void* s, void* out, int N, int C, int HW, void* stream) {
    if (!f || !a || !s || !out || N < 1 || C < 1 || !prm_flat_ok((long long)N * C, HW)) return OTP_ERR_BAD_ARG;
    hipLaunchKernelGGL(prm_combine_kernel, dim3(N * C), dim3(PRM_THREADS), 0, static_cast<hipStream_t>(stream),
                       static_cast<const float*>(f), static_cast<const float*>(a), static_cast<const float*>(s),
                       static_cast<float*>(out), HW);
    return otp_launch_status();
}

extern "C" int otp_prm_combine_backward(const void* f, const void* a, const void* s, const void* grad_out, void* grad_f, void* grad_a,
                                        void* grad_s, int N, int C, int HW, void* stream) {
    if (!f || !a || !s || !grad_out || !grad_f || !grad_a || !grad_s || N < 1 || C < 1 || !prm_flat_ok((long long)N * C, HW))
        return OTP_ERR_BAD_ARG;
    hipLaunchKernelGGL(prm_combine_bwd_kernel, dim3(N * C), dim3(PRM_THREADS), 0, static_cast<hipStream_t>(stream),
                       static_cast<const float*>(f), static_cast<const float*>(a), static_cast<const float*>(s),
                       static_cast<const float*>(grad_out), static_cast<float*>(grad_f), static_cast<float*>(grad_a),
                       static_cast<float*>(grad_s), HW);
    return otp_launch_status();
}
