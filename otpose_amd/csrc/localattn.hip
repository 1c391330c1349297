// Local-window (banded) attention of LocalMaskedMHCA (reference model/blocks.py:479-833), forward and backward.
//
// q, k, v (B, C, T) fp32 viewed as (B, nh, hs, T); w = window / 2, W = 2w + 1.  Token t attends to positions t - w .. t + w:
//   S[t][j] = scale * sum_c q[c][t] k[c][t + j - w] (+ rel_pe[h][j]),  P = softmax over the positions inside [0, T),
//   O[c][t] = sum_j P[t][j] v[c][t + j - w]                                        (natural (B, C, T) layout)
// Every kernel here is the same two loops around a per-token transform of the W band values a thread keeps in registers:
//   band_scores  coef[m][j] += a[c][t_m] * x[c][t_m + j - w]     a: the thread's own tokens (global, 16 bytes per lane)
//   band_apply   out[c][t_m] = f * sum_j coef[m][j] * x[c][t_m + j - w]
// with x staged in the LDS in chunks of LA_CC channels: a tile's LA_TILE positions plus a w-wide halo on each side (18 KB, so
// the LDS never bounds occupancy).  A thread owns LA_TPT = 4 consecutive tokens: one staged word serves up to four products
// (6 ds_read_b128 per 76 FMAs at window 19), and lanes run along T, so the global reads and writes are 16 bytes per lane and
// contiguous across a wave.
//   forward      scores(q, k) -> softmax (max subtracted) -> [P out] -> apply(P, v)
//   backward A   scores(dO, v) = dP -> dS = P (dP - sum_j P dP) -> dS out, per-workgroup column sums of dS -> apply(dS, k) = dq
//   backward B   gather form: dk[c][u] = scale sum_j' dS[u + j' - w][2w - j'] q[c][u + j' - w], dv likewise from P and dO:
//                the transposed band of a token is read once into registers (W words per token, every word of dS / P read by
//                exactly one thread), then two apply loops.  No atomics anywhere: every output word has one writer, and
//                d rel_pe adds the workgroup partials in a fixed order.
// Exact fp32 FMAs throughout (the op is memory bound: no split products).
#include "common.h"

namespace {

constexpr int LA_THREADS = 128;
constexpr int LA_TPT = 4;                          // consecutive tokens of a thread
constexpr int LA_TILE = LA_THREADS * LA_TPT;       // tokens of a workgroup
constexpr int LA_CC = 8;                           // channels staged at a time
constexpr int LA_WMIN = 2, LA_WMAX = 16;           // w = window / 2

template <int w>
struct la_dims {
    static constexpr int W = 2 * w + 1;
    static constexpr int NWIN = (LA_TPT + 2 * w + 3) & ~3;     // words a thread reads of a staged row (whole 16-byte reads)
    static constexpr int LROW = LA_TILE + NWIN;                // staged positions tile0 - w .. (the tail past 2w is zero fill)
    static constexpr int LDS_WORDS = LA_CC * LROW;
    static_assert(LDS_WORDS >= W * LA_THREADS, "the column-sum reduction of backward A reuses the staging buffer");
};

// four consecutive fp32 words at row[t .. t + 3]: one 16-byte access when `vec` (T % 4 == 0 and 16-byte aligned bases), else
// word by word; words at or past T read as zero / are not written
__device__ __forceinline__ otp_f32x4 la_load4(const float* __restrict__ row, int t, int T, bool vec) {
    otp_f32x4 r = {0.f, 0.f, 0.f, 0.f};
    if (vec) {
        if (t < T) r = *reinterpret_cast<const otp_f32x4*>(row + t);
    } else {
#pragma unroll
        for (int m = 0; m < 4; ++m)
            if (t + m < T) r[m] = row[t + m];
    }
    return r;
}
__device__ __forceinline__ void la_store4(float* __restrict__ row, int t, int T, bool vec, otp_f32x4 r) {
    if (vec) {
        if (t < T) *reinterpret_cast<otp_f32x4*>(row + t) = r;
    } else {
#pragma unroll
        for (int m = 0; m < 4; ++m)
            if (t + m < T) row[t + m] = r[m];
    }
}

// channels c0 .. c0 + LA_CC - 1 of one head of x (rows of T words), positions tile0 - w .. tile0 - w + LROW - 1 -> lds[cc][LROW];
// zero outside the sequence and past the head's last channel
template <int w>
__device__ __forceinline__ void la_stage(const float* __restrict__ x, float* lds, int c0, int hs, int T, int tile0) {
    typedef la_dims<w> D;
    constexpr int NI = (D::LROW + LA_THREADS - 1) / LA_THREADS;
    // every load of the chunk is issued before the first LDS write: one memory latency per chunk, not one per word
    float r[LA_CC][NI];
#pragma unroll
    for (int cc = 0; cc < LA_CC; ++cc) {
        const bool row_ok = c0 + cc < hs;
        const float* __restrict__ row = x + (size_t)(c0 + cc) * T;
#pragma unroll
        for (int n = 0; n < NI; ++n) {
            const int p = tile0 - w + n * LA_THREADS + (int)threadIdx.x;
            r[cc][n] = (row_ok && p >= 0 && p < T) ? row[p] : 0.f;
        }
    }
#pragma unroll
    for (int cc = 0; cc < LA_CC; ++cc)
#pragma unroll
        for (int n = 0; n < NI; ++n) {
            const int i = n * LA_THREADS + (int)threadIdx.x;
            if (i < D::LROW) lds[cc * D::LROW + i] = r[cc][n];
        }
}

// the NWIN staged words of row cc a thread's four tokens touch: win[m + j] is position t_m + j - w
template <int w>
__device__ __forceinline__ void la_window(const float* lds, int cc, float (&win)[la_dims<w>::NWIN]) {
    typedef la_dims<w> D;
    const otp_f32x4* p = reinterpret_cast<const otp_f32x4*>(lds + cc * D::LROW + threadIdx.x * LA_TPT);
#pragma unroll
    for (int i = 0; i < D::NWIN / 4; ++i) {
        const otp_f32x4 v = p[i];
        win[4 * i] = v[0], win[4 * i + 1] = v[1], win[4 * i + 2] = v[2], win[4 * i + 3] = v[3];
    }
}

// coef[m][j] = sum_c a[c][t0 + m] * x[c][t0 + m + j - w] over the hs channels of one head
template <int w>
__device__ __forceinline__ void la_band_scores(const float* __restrict__ a, const float* __restrict__ x, float* lds,
                                               float (&coef)[LA_TPT][la_dims<w>::W], int hs, int T, int tile0, int t0, bool vec) {
    typedef la_dims<w> D;
#pragma unroll
    for (int m = 0; m < LA_TPT; ++m)
#pragma unroll
        for (int j = 0; j < D::W; ++j) coef[m][j] = 0.f;
    for (int c0 = 0; c0 < hs; c0 += LA_CC) {
        otp_f32x4 av[LA_CC];
#pragma unroll
        for (int cc = 0; cc < LA_CC; ++cc)
            av[cc] = c0 + cc < hs ? la_load4(a + (size_t)(c0 + cc) * T, t0, T, vec) : otp_f32x4{0.f, 0.f, 0.f, 0.f};
        __syncthreads();                                   // the previous chunk's (or phase's) readers are done
        la_stage<w>(x, lds, c0, hs, T, tile0);
        __syncthreads();
#pragma unroll
        for (int cc = 0; cc < LA_CC; ++cc) {
            if (c0 + cc >= hs) break;                      // workgroup-uniform
            float win[D::NWIN];
            la_window<w>(lds, cc, win);
#pragma unroll
            for (int m = 0; m < LA_TPT; ++m)
#pragma unroll
                for (int j = 0; j < D::W; ++j) coef[m][j] = __builtin_fmaf(av[cc][m], win[m + j], coef[m][j]);
        }
    }
}

// out[c][t0 + m] = f * sum_j coef[m][j] * x[c][t0 + m + j - w]
template <int w>
__device__ __forceinline__ void la_band_apply(const float (&coef)[LA_TPT][la_dims<w>::W], const float* __restrict__ x, float* lds,
                                              float* __restrict__ out, float f, int hs, int T, int tile0, int t0, bool vec) {
    typedef la_dims<w> D;
    for (int c0 = 0; c0 < hs; c0 += LA_CC) {
        __syncthreads();
        la_stage<w>(x, lds, c0, hs, T, tile0);
        __syncthreads();
#pragma unroll
        for (int cc = 0; cc < LA_CC; ++cc) {
            if (c0 + cc >= hs) break;
            float win[D::NWIN];
            la_window<w>(lds, cc, win);
            otp_f32x4 o;
#pragma unroll
            for (int m = 0; m < LA_TPT; ++m) {
                float s = 0.f;
#pragma unroll
                for (int j = 0; j < D::W; ++j) s = __builtin_fmaf(coef[m][j], win[m + j], s);
                o[m] = s * f;
            }
            la_store4(out + (size_t)(c0 + cc) * T, t0, T, vec, o);
        }
    }
}

// the thread's LA_TPT * W consecutive words of a (BH, T, W) band tensor (rows t0 .. t0 + 3 of `band`, which points at row 0)
template <int w>
__device__ __forceinline__ void la_band_load(const float* __restrict__ band, float (&r)[LA_TPT][la_dims<w>::W], int T, int t0, bool vec) {
    typedef la_dims<w> D;
    const float* __restrict__ p = band + (size_t)t0 * D::W;
    if (vec) {                                             // 4 W words from a 16-byte aligned address
        float flat[LA_TPT * D::W];
#pragma unroll
        for (int i = 0; i < D::W; ++i) {
            const otp_f32x4 v = t0 < T ? reinterpret_cast<const otp_f32x4*>(p)[i] : otp_f32x4{0.f, 0.f, 0.f, 0.f};
            flat[4 * i] = v[0], flat[4 * i + 1] = v[1], flat[4 * i + 2] = v[2], flat[4 * i + 3] = v[3];
        }
#pragma unroll
        for (int m = 0; m < LA_TPT; ++m)
#pragma unroll
            for (int j = 0; j < D::W; ++j) r[m][j] = flat[m * D::W + j];
    } else {
#pragma unroll
        for (int m = 0; m < LA_TPT; ++m)
#pragma unroll
            for (int j = 0; j < D::W; ++j) r[m][j] = t0 + m < T ? p[m * D::W + j] : 0.f;
    }
}
template <int w>
__device__ __forceinline__ void la_band_store(float* __restrict__ band, const float (&r)[LA_TPT][la_dims<w>::W], int T, int t0, bool vec) {
    typedef la_dims<w> D;
    float* __restrict__ p = band + (size_t)t0 * D::W;
    if (vec) {
        if (t0 >= T) return;
        float flat[LA_TPT * D::W];
#pragma unroll
        for (int m = 0; m < LA_TPT; ++m)
#pragma unroll
            for (int j = 0; j < D::W; ++j) flat[m * D::W + j] = r[m][j];
#pragma unroll
        for (int i = 0; i < D::W; ++i)
            reinterpret_cast<otp_f32x4*>(p)[i] = otp_f32x4{flat[4 * i], flat[4 * i + 1], flat[4 * i + 2], flat[4 * i + 3]};
    } else {
#pragma unroll
        for (int m = 0; m < LA_TPT; ++m)
            if (t0 + m < T)
#pragma unroll
                for (int j = 0; j < D::W; ++j) p[m * D::W + j] = r[m][j];
    }
}

// Attention-probability dropout (csrc/common.h: otp_attn_drop): the band is entry (g = bh, i = t, j = slot) of a (B nh, T, W)
// matrix, slots outside the sequence included (P is zero there).  band[m][j] *= the factor of (bh, t0 + m, j): W / 2 + 1 hashes a row
template <int w>
__device__ __forceinline__ void la_band_drop(float (&band)[LA_TPT][la_dims<w>::W], const otp_attn_drop& drop, int bh, int T, int t0) {
    typedef la_dims<w> D;
#pragma unroll
    for (int m = 0; m < LA_TPT; ++m) {
        const uint64_t row = otp_attn_drop_row((uint64_t)bh * T + (uint64_t)(t0 + m), D::W);
#pragma unroll
        for (int j2 = 0; j2 <= w; ++j2) {
            const uint32_t h = otp_attn_drop_draw(drop, row + j2);
            band[m][2 * j2] *= otp_attn_drop_factor(drop, h, 0);
            if (2 * j2 + 1 < D::W) band[m][2 * j2 + 1] *= otp_attn_drop_factor(drop, h, 1);
        }
    }
}

// The three kernels are bodies with a DROP flag under two __global__ wrappers each (grid (tiles, B * n_head)): DROP = false is the
// code without a hash in it, under the kernel name and arguments it always had.
template <int w, bool DROP>
__device__ __forceinline__ void local_attn_fwd_body(float* lds, const float* __restrict__ q, const float* __restrict__ k,
                                                    const float* __restrict__ v, const float* __restrict__ rel_pe,
                                                    float* __restrict__ out, float* __restrict__ probs, int hs,
                                                    int T, int n_head, float scale, int vec_i, const otp_attn_drop& drop) {
    typedef la_dims<w> D;
    const bool vec = vec_i != 0;
    const int bh = blockIdx.y, head = bh % n_head;
    const int tile0 = blockIdx.x * LA_TILE, t0 = tile0 + threadIdx.x * LA_TPT;
    const size_t base = (size_t)bh * hs * T;               // (b * C + head * hs) * T
    float s[LA_TPT][D::W];
    la_band_scores<w>(q + base, k + base, lds, s, hs, T, tile0, t0, vec);
#pragma unroll
    for (int m = 0; m < LA_TPT; ++m) {
        const int t = t0 + m;
        float mx = -3.0e38f;
#pragma unroll
        for (int j = 0; j < D::W; ++j) {
            const int p = t + j - w;
            const bool in = p >= 0 && p < T;
            float x = s[m][j] * scale;
            if (rel_pe) x += rel_pe[head * D::W + j];
            s[m][j] = in ? x : -3.0e38f;
            mx = fmaxf(mx, s[m][j]);
        }
        float sum = 0.f;
#pragma unroll
        for (int j = 0; j < D::W; ++j) {
            const int p = t + j - w;
            const float e = (p >= 0 && p < T) ? expf(s[m][j] - mx) : 0.f;
            s[m][j] = e;
            sum += e;
        }
        const float inv = t < T ? 1.f / sum : 0.f;         // (a token past T has no position inside: sum = 0, nothing stored)
#pragma unroll
        for (int j = 0; j < D::W; ++j) s[m][j] *= inv;
    }
    if (probs) la_band_store<w>(probs + (size_t)bh * T * D::W, s, T, t0, vec);     // the undropped band
    if (DROP) la_band_drop<w>(s, drop, bh, T, t0);
    la_band_apply<w>(s, v + base, lds, out + base, 1.f, hs, T, tile0, t0, vec);
}
template <int w>
__global__ __launch_bounds__(LA_THREADS) void local_attn_fwd_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                                    const float* __restrict__ v, const float* __restrict__ rel_pe,
                                                                    float* __restrict__ out, float* __restrict__ probs, int hs,
                                                                    int T, int n_head, float scale, int vec_i) {
    __shared__ __attribute__((aligned(16))) float lds[la_dims<w>::LDS_WORDS];
    local_attn_fwd_body<w, false>(lds, q, k, v, rel_pe, out, probs, hs, T, n_head, scale, vec_i, otp_attn_drop{});
}
template <int w>
__global__ __launch_bounds__(LA_THREADS) void local_attn_fwd_drop_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                                         const float* __restrict__ v, const float* __restrict__ rel_pe,
                                                                         float* __restrict__ out, float* __restrict__ probs, int hs,
                                                                         int T, int n_head, float scale, int vec_i, otp_attn_drop drop) {
    __shared__ __attribute__((aligned(16))) float lds[la_dims<w>::LDS_WORDS];
    local_attn_fwd_body<w, true>(lds, q, k, v, rel_pe, out, probs, hs, T, n_head, scale, vec_i, drop);
}

// backward A: dS (BH, T, W), dq, and partial[(bh * tiles + tile) * W + j] = sum over the tile's tokens of dS[.][j] when non-null
// with DROP: dS = P (m dP - sum_j P m dP)
template <int w, bool DROP>
__device__ __forceinline__ void local_attn_bwd_a_body(float* lds, const float* __restrict__ k, const float* __restrict__ v,
                                                      const float* __restrict__ probs, const float* __restrict__ gout,
                                                      float* __restrict__ gq, float* __restrict__ ds,
                                                      float* __restrict__ partial, int hs, int T, float scale,
                                                      int vec_i, const otp_attn_drop& drop) {
    typedef la_dims<w> D;
    const bool vec = vec_i != 0;
    const int bh = blockIdx.y;
    const int tile0 = blockIdx.x * LA_TILE, t0 = tile0 + threadIdx.x * LA_TPT;
    const size_t base = (size_t)bh * hs * T, band = (size_t)bh * T * D::W;
    float d[LA_TPT][D::W];
    la_band_scores<w>(gout + base, v + base, lds, d, hs, T, tile0, t0, vec);           // dP
    if (DROP) la_band_drop<w>(d, drop, bh, T, t0);
    {
        float p[LA_TPT][D::W];
        la_band_load<w>(probs + band, p, T, t0, vec);      // zero at positions outside the sequence and for tokens past T
#pragma unroll
        for (int m = 0; m < LA_TPT; ++m) {
            float dot = 0.f;
#pragma unroll
            for (int j = 0; j < D::W; ++j) dot = __builtin_fmaf(p[m][j], d[m][j], dot);
#pragma unroll
            for (int j = 0; j < D::W; ++j) d[m][j] = p[m][j] * (d[m][j] - dot);
        }
    }
    la_band_store<w>(ds + band, d, T, t0, vec);
    if (partial) {                                         // column sums of the tile in a fixed order: thread 0 .. 127 per column
        __syncthreads();
#pragma unroll
        for (int j = 0; j < D::W; ++j) lds[j * LA_THREADS + threadIdx.x] = (d[0][j] + d[1][j]) + (d[2][j] + d[3][j]);
        __syncthreads();
        if (threadIdx.x < D::W) {
            float sum = 0.f;
            for (int i = 0; i < LA_THREADS; ++i) sum += lds[threadIdx.x * LA_THREADS + i];
            partial[((size_t)bh * gridDim.x + blockIdx.x) * D::W + threadIdx.x] = sum;
        }
    }
    la_band_apply<w>(d, k + base, lds, gq + base, scale, hs, T, tile0, t0, vec);
}
template <int w>
__global__ __launch_bounds__(LA_THREADS) void local_attn_bwd_a_kernel(const float* __restrict__ k, const float* __restrict__ v,
                                                                      const float* __restrict__ probs, const float* __restrict__ gout,
                                                                      float* __restrict__ gq, float* __restrict__ ds,
                                                                      float* __restrict__ partial, int hs, int T, float scale,
                                                                      int vec_i) {
    __shared__ __attribute__((aligned(16))) float lds[la_dims<w>::LDS_WORDS];
    local_attn_bwd_a_body<w, false>(lds, k, v, probs, gout, gq, ds, partial, hs, T, scale, vec_i, otp_attn_drop{});
}
template <int w>
__global__ __launch_bounds__(LA_THREADS) void local_attn_bwd_a_drop_kernel(const float* __restrict__ k, const float* __restrict__ v,
                                                                           const float* __restrict__ probs,
                                                                           const float* __restrict__ gout, float* __restrict__ gq,
                                                                           float* __restrict__ ds, float* __restrict__ partial, int hs,
                                                                           int T, float scale, int vec_i, otp_attn_drop drop) {
    __shared__ __attribute__((aligned(16))) float lds[la_dims<w>::LDS_WORDS];
    local_attn_bwd_a_body<w, true>(lds, k, v, probs, gout, gq, ds, partial, hs, T, scale, vec_i, drop);
}

// the transposed band of the thread's tokens: r[m][j'] = band[u + j' - w][2w - j'] with u = t0 + m, zero where that row is
// outside the sequence (the entry itself then refers to position u, which is inside whenever u < T)
template <int w>
__device__ __forceinline__ void la_band_gather(const float* __restrict__ band, float (&r)[LA_TPT][la_dims<w>::W], int T, int t0) {
    typedef la_dims<w> D;
#pragma unroll
    for (int m = 0; m < LA_TPT; ++m)
#pragma unroll
        for (int j = 0; j < D::W; ++j) {
            const int u = t0 + m, t = u + j - w;
            r[m][j] = (u < T && t >= 0 && t < T) ? band[(size_t)t * D::W + (2 * w - j)] : 0.f;
        }
}

// the factors of the transposed band: r[m][j'] *= the factor of (bh, u + j' - w, 2w - j'), one hash each (rows outside the
// sequence hold zeros already)
template <int w>
__device__ __forceinline__ void la_band_gather_drop(float (&r)[LA_TPT][la_dims<w>::W], const otp_attn_drop& drop, int bh, int T, int t0) {
    typedef la_dims<w> D;
#pragma unroll
    for (int m = 0; m < LA_TPT; ++m) {
        const uint64_t row0 = otp_attn_drop_row((uint64_t)bh * T + (uint64_t)(t0 + m) - (uint64_t)w, D::W);     // row u - w (wraps below 0: unused)
#pragma unroll
        for (int j = 0; j < D::W; ++j) {
            const int t = t0 + m + j - w;
            if (t >= 0 && t < T) r[m][j] *= otp_attn_drop_at(drop, row0 + (uint64_t)(j * (w + 1)), 2 * w - j);
        }
    }
}

// backward B: dk and dv in gather form; with DROP dv gathers m P
template <int w, bool DROP>
__device__ __forceinline__ void local_attn_bwd_b_body(float* lds, const float* __restrict__ q, const float* __restrict__ probs,
                                                      const float* __restrict__ ds, const float* __restrict__ gout,
                                                      float* __restrict__ gk, float* __restrict__ gv, int hs, int T,
                                                      float scale, int vec_i, const otp_attn_drop& drop) {
    typedef la_dims<w> D;
    const bool vec = vec_i != 0;
    const int bh = blockIdx.y;
    const int tile0 = blockIdx.x * LA_TILE, t0 = tile0 + threadIdx.x * LA_TPT;
    const size_t base = (size_t)bh * hs * T, band = (size_t)bh * T * D::W;
    float c[LA_TPT][D::W];
    la_band_gather<w>(ds + band, c, T, t0);
    la_band_apply<w>(c, q + base, lds, gk + base, scale, hs, T, tile0, t0, vec);
    la_band_gather<w>(probs + band, c, T, t0);
    if (DROP) la_band_gather_drop<w>(c, drop, bh, T, t0);
    la_band_apply<w>(c, gout + base, lds, gv + base, 1.f, hs, T, tile0, t0, vec);
}
template <int w>
__global__ __launch_bounds__(LA_THREADS) void local_attn_bwd_b_kernel(const float* __restrict__ q, const float* __restrict__ probs,
                                                                      const float* __restrict__ ds, const float* __restrict__ gout,
                                                                      float* __restrict__ gk, float* __restrict__ gv, int hs, int T,
                                                                      float scale, int vec_i) {
    __shared__ __attribute__((aligned(16))) float lds[la_dims<w>::LDS_WORDS];
    local_attn_bwd_b_body<w, false>(lds, q, probs, ds, gout, gk, gv, hs, T, scale, vec_i, otp_attn_drop{});
}
template <int w>
__global__ __launch_bounds__(LA_THREADS) void local_attn_bwd_b_drop_kernel(const float* __restrict__ q, const float* __restrict__ probs,
                                                                           const float* __restrict__ ds, const float* __restrict__ gout,
                                                                           float* __restrict__ gk, float* __restrict__ gv, int hs,
                                                                           int T, float scale, int vec_i, otp_attn_drop drop) {
    __shared__ __attribute__((aligned(16))) float lds[la_dims<w>::LDS_WORDS];
    local_attn_bwd_b_body<w, true>(lds, q, probs, ds, gout, gk, gv, hs, T, scale, vec_i, drop);
}

// grel[head][j] = sum over b, then tile, of the workgroup partials (one thread per word, fixed order)
__global__ void local_attn_grel_kernel(const float* __restrict__ partial, float* __restrict__ grel, int B, int n_head, int tiles, int W) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_head * W) return;
    const int head = i / W, j = i % W;
    float sum = 0.f;
    for (int b = 0; b < B; ++b)
        for (int tl = 0; tl < tiles; ++tl) sum += partial[((size_t)(b * n_head + head) * tiles + tl) * W + j];
    grel[i] = sum;
}

bool la_window_ok(int window) { return (window & 1) && window >= 2 * LA_WMIN + 1 && window <= 2 * LA_WMAX + 1; }

bool la_shape_ok(int B, int C, int T, int n_head, int window) {
    return B > 0 && C > 0 && T > 0 && n_head > 0 && C % n_head == 0 && la_window_ok(window) && T % (window - 1) == 0 &&
           (long long)B * n_head <= 65535;
}

bool la_aligned16(std::initializer_list<const void*> ptrs) {
    uintptr_t bits = 0;
    for (const void* p : ptrs) bits |= reinterpret_cast<uintptr_t>(p);
    return (bits & 15) == 0;
}

// one case per w: the band arrays are indexed by compile-time constants only, so they stay in registers
#define LA_DISPATCH(w_, CALL)                                                                                          \
    switch (w_) {                                                                                                      \
        case 2: { constexpr int LW = 2; CALL; } break;   case 3: { constexpr int LW = 3; CALL; } break;                \
        case 4: { constexpr int LW = 4; CALL; } break;   case 5: { constexpr int LW = 5; CALL; } break;                \
        case 6: { constexpr int LW = 6; CALL; } break;   case 7: { constexpr int LW = 7; CALL; } break;                \
        case 8: { constexpr int LW = 8; CALL; } break;   case 9: { constexpr int LW = 9; CALL; } break;                \
        case 10: { constexpr int LW = 10; CALL; } break; case 11: { constexpr int LW = 11; CALL; } break;              \
        case 12: { constexpr int LW = 12; CALL; } break; case 13: { constexpr int LW = 13; CALL; } break;              \
        case 14: { constexpr int LW = 14; CALL; } break; case 15: { constexpr int LW = 15; CALL; } break;              \
        default: { constexpr int LW = 16; CALL; } break;                                                               \
    }

}  // namespace

extern "C" int otp_local_attn_supported(int hs, int t, int window) {
    return hs > 0 && t > 0 && la_window_ok(window) && t % (window - 1) == 0;
}

extern "C" int otp_local_attn(const void* q, const void* k, const void* v, const void* rel_pe, void* out, void* probs, int B, int C,
                              int T, int n_head, int window, float scale, void* stream) {
    if (!q || !k || !v || !out || !la_shape_ok(B, C, T, n_head, window)) return OTP_ERR_BAD_ARG;
    const int hs = C / n_head, w = window / 2;
    const int vec = T % 4 == 0 && la_aligned16({q, k, v, out, probs});
    const dim3 grid(otp_ceil_div(T, LA_TILE), B * n_head);
    auto st = static_cast<hipStream_t>(stream);
    LA_DISPATCH(w, hipLaunchKernelGGL(local_attn_fwd_kernel<LW>, grid, dim3(LA_THREADS), 0, st, static_cast<const float*>(q),
                                      static_cast<const float*>(k), static_cast<const float*>(v), static_cast<const float*>(rel_pe),
                                      static_cast<float*>(out), static_cast<float*>(probs), hs, T, n_head, scale, vec));
    return otp_launch_status();
}

extern "C" int otp_local_attn_dropout(const void* q, const void* k, const void* v, const void* rel_pe, void* out, void* probs, int B,
                                      int C, int T, int n_head, int window, float scale, float p, unsigned long long seed,
                                      void* stream) {
    if (!q || !k || !v || !out || !la_shape_ok(B, C, T, n_head, window) || !otp_attn_drop_rate_ok(p)) return OTP_ERR_BAD_ARG;
    const otp_attn_drop drop = otp_attn_drop_make(p, seed);
    if (!drop.thr) return otp_local_attn(q, k, v, rel_pe, out, probs, B, C, T, n_head, window, scale, stream);
    const int hs = C / n_head, w = window / 2;
    const int vec = T % 4 == 0 && la_aligned16({q, k, v, out, probs});
    const dim3 grid(otp_ceil_div(T, LA_TILE), B * n_head);
    auto st = static_cast<hipStream_t>(stream);
    LA_DISPATCH(w, hipLaunchKernelGGL(local_attn_fwd_drop_kernel<LW>, grid, dim3(LA_THREADS), 0, st, static_cast<const float*>(q),
                                      static_cast<const float*>(k), static_cast<const float*>(v), static_cast<const float*>(rel_pe),
                                      static_cast<float*>(out), static_cast<float*>(probs), hs, T, n_head, scale, vec, drop));
    return otp_launch_status();
}

// dS (B nh, T, window) and the per-workgroup column sums of dS (B nh, tiles, window), both fp32
extern "C" size_t otp_local_attn_backward_workspace(int B, int C, int T, int n_head, int window) {
    if (!la_shape_ok(B, C, T, n_head, window)) return 0;
    const size_t BH = (size_t)B * n_head;
    return (BH * T + BH * otp_ceil_div(T, LA_TILE)) * window * sizeof(float);
}

extern "C" int otp_local_attn_backward(const void* q, const void* k, const void* v, const void* probs, const void* gout, void* gq,
                                       void* gk, void* gv, void* grel, void* ws, size_t ws_bytes, int B, int C, int T, int n_head,
                                       int window, float scale, void* stream) {
    if (!q || !k || !v || !probs || !gout || !gq || !gk || !gv || !ws || !la_shape_ok(B, C, T, n_head, window))
        return OTP_ERR_BAD_ARG;
    if (ws_bytes < otp_local_attn_backward_workspace(B, C, T, n_head, window)) return OTP_ERR_WORKSPACE;
    const int hs = C / n_head, w = window / 2, tiles = otp_ceil_div(T, LA_TILE);
    float* ds = static_cast<float*>(ws);
    float* partial = ds + (size_t)B * n_head * T * window;
    const int vec = T % 4 == 0 && la_aligned16({q, k, v, probs, gout, gq, gk, gv, ws});
    const dim3 grid(tiles, B * n_head);
    auto st = static_cast<hipStream_t>(stream);
    const float *qf = static_cast<const float*>(q), *kf = static_cast<const float*>(k), *vf = static_cast<const float*>(v),
                *pf = static_cast<const float*>(probs), *gf = static_cast<const float*>(gout);
    LA_DISPATCH(w, {
        hipLaunchKernelGGL(local_attn_bwd_a_kernel<LW>, grid, dim3(LA_THREADS), 0, st, kf, vf, pf, gf, static_cast<float*>(gq), ds,
                           grel ? partial : nullptr, hs, T, scale, vec);
        hipLaunchKernelGGL(local_attn_bwd_b_kernel<LW>, grid, dim3(LA_THREADS), 0, st, qf, pf, static_cast<const float*>(ds), gf,
                           static_cast<float*>(gk), static_cast<float*>(gv), hs, T, scale, vec);
    });
    if (grel)
        hipLaunchKernelGGL(local_attn_grel_kernel, dim3(otp_ceil_div(n_head * window, 64)), dim3(64), 0, st,
                           static_cast<const float*>(partial), static_cast<float*>(grel), B, n_head, tiles, window);
    return otp_launch_status();
}

extern "C" int otp_local_attn_backward_dropout(const void* q, const void* k, const void* v, const void* probs, const void* gout,
                                               void* gq, void* gk, void* gv, void* grel, void* ws, size_t ws_bytes, int B, int C, int T,
                                               int n_head, int window, float scale, float p, unsigned long long seed, void* stream) {
    if (!q || !k || !v || !probs || !gout || !gq || !gk || !gv || !ws || !la_shape_ok(B, C, T, n_head, window) ||
        !otp_attn_drop_rate_ok(p))
        return OTP_ERR_BAD_ARG;
    const otp_attn_drop drop = otp_attn_drop_make(p, seed);
    if (!drop.thr)
        return otp_local_attn_backward(q, k, v, probs, gout, gq, gk, gv, grel, ws, ws_bytes, B, C, T, n_head, window, scale, stream);
    if (ws_bytes < otp_local_attn_backward_workspace(B, C, T, n_head, window)) return OTP_ERR_WORKSPACE;
    const int hs = C / n_head, w = window / 2, tiles = otp_ceil_div(T, LA_TILE);
    float* ds = static_cast<float*>(ws);
    float* partial = ds + (size_t)B * n_head * T * window;
    const int vec = T % 4 == 0 && la_aligned16({q, k, v, probs, gout, gq, gk, gv, ws});
    const dim3 grid(tiles, B * n_head);
    auto st = static_cast<hipStream_t>(stream);
    const float *qf = static_cast<const float*>(q), *kf = static_cast<const float*>(k), *vf = static_cast<const float*>(v),
                *pf = static_cast<const float*>(probs), *gf = static_cast<const float*>(gout);
    LA_DISPATCH(w, {
        hipLaunchKernelGGL(local_attn_bwd_a_drop_kernel<LW>, grid, dim3(LA_THREADS), 0, st, kf, vf, pf, gf, static_cast<float*>(gq),
                           ds, grel ? partial : nullptr, hs, T, scale, vec, drop);
        hipLaunchKernelGGL(local_attn_bwd_b_drop_kernel<LW>, grid, dim3(LA_THREADS), 0, st, qf, pf, static_cast<const float*>(ds), gf,
                           static_cast<float*>(gk), static_cast<float*>(gv), hs, T, scale, vec, drop);
    });
    if (grel)
        hipLaunchKernelGGL(local_attn_grel_kernel, dim3(otp_ceil_div(n_head * window, 64)), dim3(64), 0, st,
                           static_cast<const float*>(partial), static_cast<float*>(grel), B, n_head, tiles, window);
    return otp_launch_status();
}
