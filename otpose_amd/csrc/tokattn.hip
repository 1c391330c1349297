// Token x token self-attention of the DETR-style TransformerEncoder (reference model/OTPose.py:26-159), flash style:
//   S[i][j] = scale * sum_c q[c][i] k[c][j],  P = softmax_j(S),  O[c][i] = sum_j P[i][j] v[c][j]
// on (B, C, T) fp32 operands viewed as (B, n_head, hd, T), without a T x T buffer anywhere but the explicit attention map.
// Every product runs on the exact-fp32 MFMA (16x16x4: bit for bit a k-ordered fmaf chain); no split half-precision products.
//
// One tile shape serves all five kernels: a workgroup of 4 waves holds TA_TILE = 64 tokens of one side in registers (16 per
// wave, the MFMA's column index n = lane & 15) and walks the other side in 64-token tiles staged in the LDS, channel-major
// [16 NCB channels][64 tokens] with a row stride of 68 words; hd is zero-padded to 16 NCB rows there, never in HBM.
//
// The first product is computed TRANSPOSED, staged side x register side: its accumulators then hold, per lane, one register-side
// token and 16 staged-side tokens - exactly the B operand of the second product (which sums over the staged side), so P never
// leaves the registers.  The staged token of accumulator acc[kb][r] in lane group g = lane >> 4 is 16 g + 4 r + kb: with that
// numbering every LDS read is one ds_read_b128 of four neighbouring tokens,
//   first product,  k-step s:  lds[4 s + g][4 n .. 4 n + 3]                    -> the A operands of the four blocks kb
//   second product, (cb, r):   lds[16 cb + n][16 g + 4 r .. 16 g + 4 r + 3]    -> the A operands of its four k-steps kb
// and the 16 lanes of a group touch 16 different 16-byte slots (68 / 4 = 17 is odd).
//
//   forward     per (b, h, query tile): loop over key tiles, running maximum / sum / O in registers
//   backward A  per (b, h, query tile): D = sum_c dO O (kept for B in the workspace), loop over key tiles, dq
//   backward B  per (b, h, key tile):   loop over query tiles, dk and dv
//   map         per (b, query tile, key tile): loop over heads, mean_h exp(S - lse)
// Every output word has one writer; there are no atomics.
#include "common.h"

#include <math.h>

namespace {

constexpr int TA_TILE = 64, TA_STRIDE = 68, TA_THREADS = 256, TA_MAX_HD = 136;
constexpr int TA_MAX_T = 1 << 30;

template <int NCB>
constexpr int ta_lds_bytes() { return (2 * 16 * NCB * TA_STRIDE + 2 * TA_TILE) * (int)sizeof(float); }

__device__ __forceinline__ otp_f32x4 ta_mfma(float a, float b, otp_f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// columns t0 .. t0 + 63 of the hd rows of one head (src: its first channel) into lds[16 NCB][TA_STRIDE]; zeros past hd and past T
template <int NCB>
__device__ __forceinline__ void ta_stage(float* lds, const float* __restrict__ src, int hd, int T, int t0) {
    const int col = threadIdx.x & 63, t = t0 + col;
    const bool tv = t < T;
#pragma unroll 4
    for (int r = threadIdx.x >> 6; r < 16 * NCB; r += TA_THREADS / 64)
        lds[r * TA_STRIDE + col] = (tv && r < hd) ? src[(size_t)r * T + t] : 0.f;
}

// the B operands of the first product: f[s] = x[4 s + g][t] for this lane's token t; zeros past hd and past T
template <int NCB>
__device__ __forceinline__ void ta_frags(float (&f)[4 * NCB], const float* __restrict__ src, int hd, int T, int t) {
    const int g = (threadIdx.x & 63) >> 4;
#pragma unroll
    for (int s = 0; s < 4 * NCB; ++s) {
        const int c = 4 * s + g;
        f[s] = (c < hd && t < T) ? src[(size_t)c * T + t] : 0.f;
    }
}

// acc[kb][r] (lane n, g) += sum_c lds[c][16 g + 4 r + kb] f[c][n]
template <int NCB>
__device__ __forceinline__ void ta_first(otp_f32x4 (&acc)[4], const float* lds, const float (&f)[4 * NCB]) {
    const int lane = threadIdx.x & 63, n = lane & 15, g = lane >> 4;
    const float* base = lds + g * TA_STRIDE + 4 * n;
#pragma unroll
    for (int s = 0; s < 4 * NCB; ++s) {
        const otp_f32x4 a = *reinterpret_cast<const otp_f32x4*>(base + 4 * s * TA_STRIDE);
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) acc[kb] = ta_mfma(a[kb], f[s], acc[kb]);
    }
}

// o[cb][r'] (lane n, g: channel 16 cb + 4 g + r', token n) += sum over the 64 staged tokens j of lds[channel][j] p[j][n]
template <int NCB>
__device__ __forceinline__ void ta_second(otp_f32x4 (&o)[NCB], const float* lds, const otp_f32x4 (&p)[4]) {
    const int lane = threadIdx.x & 63, n = lane & 15, g = lane >> 4;
    const float* base = lds + n * TA_STRIDE + 16 * g;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb) {
            const otp_f32x4 a = *reinterpret_cast<const otp_f32x4*>(base + 16 * cb * TA_STRIDE + 4 * r);
#pragma unroll
            for (int kb = 0; kb < 4; ++kb) o[cb] = ta_mfma(a[kb], p[kb][r], o[cb]);
        }
    }
}

// o[cb][r'] -> dst[16 cb + 4 g + r'][t] (dst: the head's first channel), times mul
template <int NCB>
__device__ __forceinline__ void ta_store(float* __restrict__ dst, const otp_f32x4 (&o)[NCB], float mul, int hd, int T, int t) {
    const int g = (threadIdx.x & 63) >> 4;
    if (t >= T) return;
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int c = 16 * cb + 4 * g + r;
            if (c < hd) dst[(size_t)c * T + t] = o[cb][r] * mul;
        }
}

// whether key t0 + lane of the tile is live (inside T and not masked): the 64 keys of a tile are the 64 lanes of EVERY wave, so
// __ballot of it is the same word in all four waves - a decision on it is uniform over the workgroup and needs no LDS
__device__ __forceinline__ bool ta_key_live(const unsigned char* __restrict__ mask_row, int T, int t0) {
    const int t = t0 + (threadIdx.x & 63);
    return t < T && !(mask_row && mask_row[t]);
}
// kbias[j] = 0 for a live key of the tile, -inf for a masked one or one past T (first wave); read after the next barrier
__device__ __forceinline__ void ta_stage_keys(float* kbias, bool live) {
    if (threadIdx.x < TA_TILE) kbias[threadIdx.x] = live ? 0.f : -INFINITY;
}

// The three training kernels are bodies with a DROP flag (attention-probability dropout, csrc/common.h: otp_attn_drop) under two
// __global__ wrappers each: DROP = false is the code without a hash in it, under the kernel name and arguments it always had.
// The mask of P[i][j] of head bh is entry (g = bh, i, j) of a (B nh, T, T) matrix; a lane's 16 staged tokens 16 g + 4 r + kb of a
// tile are consecutive, so where the staged side is the key side (forward, backward A) one hash serves kb = 0, 1 and one kb = 2, 3.
template <int NCB, bool DROP>
__device__ __forceinline__ void tokattn_fwd_body(const float* __restrict__ q, const float* __restrict__ k,
                                                 const float* __restrict__ v, const unsigned char* __restrict__ mask,
                                                 float* __restrict__ out, float* __restrict__ lse, int C, int nh,
                                                 int T, float scale, int tiles, const otp_attn_drop& drop) {
    extern __shared__ __attribute__((aligned(16))) float ta_smem[];
    float* Ks = ta_smem;
    float* Vs = Ks + 16 * NCB * TA_STRIDE;
    float* kbias = Vs + 16 * NCB * TA_STRIDE;
    const int hd = C / nh, bh = blockIdx.x / tiles, b = bh / nh, h = bh - b * nh;
    const int lane = threadIdx.x & 63, n = lane & 15, g = lane >> 4;
    const int tq = (blockIdx.x - bh * tiles) * TA_TILE + (threadIdx.x >> 6) * 16 + n;
    const size_t head = ((size_t)b * C + (size_t)h * hd) * T;
    const unsigned char* mask_row = mask ? mask + (size_t)b * T : nullptr;

    float qf[4 * NCB];
    ta_frags<NCB>(qf, q + head, hd, T, tq);
    otp_f32x4 o[NCB];
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) o[cb] = otp_f32x4{0.f, 0.f, 0.f, 0.f};
    float m = -INFINITY, l = 0.f;
    const uint64_t drop_row = DROP ? otp_attn_drop_row((uint64_t)bh * T + tq, T) : 0;

    for (int kt = 0; kt < tiles; ++kt) {
        const bool live = ta_key_live(mask_row, T, kt * TA_TILE);
        if (!__ballot(live)) continue;        // a tile without a live key: no load, no barrier, m, l and O untouched (uniform)
        __syncthreads();                                           // the previous tile has been read
        ta_stage<NCB>(Ks, k + head, hd, T, kt * TA_TILE);
        ta_stage<NCB>(Vs, v + head, hd, T, kt * TA_TILE);
        ta_stage_keys(kbias, live);
        __syncthreads();
        otp_f32x4 s[4];
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) s[kb] = otp_f32x4{0.f, 0.f, 0.f, 0.f};
        ta_first<NCB>(s, Ks, qf);
        float mt = -INFINITY;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const otp_f32x4 kb4 = *reinterpret_cast<const otp_f32x4*>(kbias + 16 * g + 4 * r);
#pragma unroll
            for (int kb = 0; kb < 4; ++kb) {
                s[kb][r] = __fadd_rn(__fmul_rn(s[kb][r], scale), kb4[kb]);
                mt = fmaxf(mt, s[kb][r]);
            }
        }
        mt = fmaxf(mt, __shfl_xor(mt, 16, 64));
        mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
        // the tile has a live key, so mt is finite and so is the new maximum: exp(-inf - (-inf)) cannot appear
        const float m_new = fmaxf(m, mt);
        const float alpha = expf(m - m_new);                       // m = -inf before the first live tile: 0
        float rs = 0.f;
#pragma unroll
        for (int kb = 0; kb < 4; ++kb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                s[kb][r] = expf(s[kb][r] - m_new);                 // -inf for a dead key: 0
                rs += s[kb][r];
            }
        rs = otp_kslot_sum(rs);
        l = fmaf(l, alpha, rs);
        m = m_new;
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb) o[cb] *= alpha;
        if (DROP) {                                                // l and m above are the undropped ones: only the operand of P v
            const uint64_t pair0 = drop_row + (uint64_t)((kt * TA_TILE + 16 * g) >> 1);
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int h2 = 0; h2 < 2; ++h2) {
                    const uint32_t h = otp_attn_drop_draw(drop, pair0 + 2 * r + h2);
                    s[2 * h2][r] *= otp_attn_drop_factor(drop, h, 0);
                    s[2 * h2 + 1][r] *= otp_attn_drop_factor(drop, h, 1);
                }
        }
        ta_second<NCB>(o, Vs, s);
    }
    ta_store<NCB>(out + head, o, 1.f / l, hd, T, tq);
    if (lse && g == 0 && tq < T) lse[(size_t)bh * T + tq] = m + logf(l);
}
template <int NCB>
__global__ __launch_bounds__(TA_THREADS) void tokattn_fwd_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                                 const float* __restrict__ v, const unsigned char* __restrict__ mask,
                                                                 float* __restrict__ out, float* __restrict__ lse, int C, int nh,
                                                                 int T, float scale, int tiles) {
    tokattn_fwd_body<NCB, false>(q, k, v, mask, out, lse, C, nh, T, scale, tiles, otp_attn_drop{});
}
template <int NCB>
__global__ __launch_bounds__(TA_THREADS) void tokattn_fwd_drop_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                                      const float* __restrict__ v,
                                                                      const unsigned char* __restrict__ mask, float* __restrict__ out,
                                                                      float* __restrict__ lse, int C, int nh, int T, float scale,
                                                                      int tiles, otp_attn_drop drop) {
    tokattn_fwd_body<NCB, true>(q, k, v, mask, out, lse, C, nh, T, scale, tiles, drop);
}

// with DROP: dP[i][j] = m[i][j] (dO_i . v_j); D = sum_c dO O is the row sum of P m dP already, O being the dropped output
template <int NCB, bool DROP>
__device__ __forceinline__ void tokattn_bwd_a_body(const float* __restrict__ q, const float* __restrict__ k,
                                                   const float* __restrict__ v, const unsigned char* __restrict__ mask,
                                                   const float* __restrict__ out, const float* __restrict__ lse,
                                                   const float* __restrict__ dout, float* __restrict__ dq,
                                                   float* __restrict__ dsum, int C, int nh, int T, float scale,
                                                   int tiles, const otp_attn_drop& drop) {
    extern __shared__ __attribute__((aligned(16))) float ta_smem[];
    float* Ks = ta_smem;
    float* Vs = Ks + 16 * NCB * TA_STRIDE;
    float* kbias = Vs + 16 * NCB * TA_STRIDE;
    const int hd = C / nh, bh = blockIdx.x / tiles, b = bh / nh, h = bh - b * nh;
    const int lane = threadIdx.x & 63, n = lane & 15, g = lane >> 4;
    const int tq = (blockIdx.x - bh * tiles) * TA_TILE + (threadIdx.x >> 6) * 16 + n;
    const size_t head = ((size_t)b * C + (size_t)h * hd) * T;
    const unsigned char* mask_row = mask ? mask + (size_t)b * T : nullptr;

    float qf[4 * NCB], gf[4 * NCB];
    ta_frags<NCB>(qf, q + head, hd, T, tq);
    ta_frags<NCB>(gf, dout + head, hd, T, tq);
    float dsum_q = 0.f;                                            // D[i] = sum_c dO[c][i] O[c][i]
#pragma unroll
    for (int s = 0; s < 4 * NCB; ++s) {
        const int c = 4 * s + g;
        if (c < hd && tq < T) dsum_q = fmaf(gf[s], out[head + (size_t)c * T + tq], dsum_q);
    }
    dsum_q = otp_kslot_sum(dsum_q);
    const float lse_q = tq < T ? lse[(size_t)bh * T + tq] : 0.f;
    if (g == 0 && tq < T) dsum[(size_t)bh * T + tq] = dsum_q;
    otp_f32x4 acc[NCB];
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) acc[cb] = otp_f32x4{0.f, 0.f, 0.f, 0.f};
    const uint64_t drop_row = DROP ? otp_attn_drop_row((uint64_t)bh * T + tq, T) : 0;

    for (int kt = 0; kt < tiles; ++kt) {
        const bool live = ta_key_live(mask_row, T, kt * TA_TILE);
        if (!__ballot(live)) continue;                             // P = 0 on the whole tile (uniform over the workgroup)
        __syncthreads();
        ta_stage<NCB>(Ks, k + head, hd, T, kt * TA_TILE);
        ta_stage<NCB>(Vs, v + head, hd, T, kt * TA_TILE);
        ta_stage_keys(kbias, live);
        __syncthreads();
        otp_f32x4 s[4], dp[4];
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) s[kb] = dp[kb] = otp_f32x4{0.f, 0.f, 0.f, 0.f};
        ta_first<NCB>(s, Ks, qf);
        ta_first<NCB>(dp, Vs, gf);
        if (DROP) {
            const uint64_t pair0 = drop_row + (uint64_t)((kt * TA_TILE + 16 * g) >> 1);
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int h2 = 0; h2 < 2; ++h2) {
                    const uint32_t h = otp_attn_drop_draw(drop, pair0 + 2 * r + h2);
                    dp[2 * h2][r] *= otp_attn_drop_factor(drop, h, 0);
                    dp[2 * h2 + 1][r] *= otp_attn_drop_factor(drop, h, 1);
                }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const otp_f32x4 kb4 = *reinterpret_cast<const otp_f32x4*>(kbias + 16 * g + 4 * r);
#pragma unroll
            for (int kb = 0; kb < 4; ++kb) {
                const float p = expf(__fadd_rn(__fmul_rn(s[kb][r], scale), kb4[kb]) - lse_q);     // exactly 0 for a dead key
                s[kb][r] = p * (dp[kb][r] - dsum_q);
            }
        }
        ta_second<NCB>(acc, Ks, s);
    }
    ta_store<NCB>(dq + head, acc, scale, hd, T, tq);
}
template <int NCB>
__global__ __launch_bounds__(TA_THREADS) void tokattn_bwd_a_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                                   const float* __restrict__ v, const unsigned char* __restrict__ mask,
                                                                   const float* __restrict__ out, const float* __restrict__ lse,
                                                                   const float* __restrict__ dout, float* __restrict__ dq,
                                                                   float* __restrict__ dsum, int C, int nh, int T, float scale,
                                                                   int tiles) {
    tokattn_bwd_a_body<NCB, false>(q, k, v, mask, out, lse, dout, dq, dsum, C, nh, T, scale, tiles, otp_attn_drop{});
}
template <int NCB>
__global__ __launch_bounds__(TA_THREADS) void tokattn_bwd_a_drop_kernel(
    const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v, const unsigned char* __restrict__ mask,
    const float* __restrict__ out, const float* __restrict__ lse, const float* __restrict__ dout, float* __restrict__ dq,
    float* __restrict__ dsum, int C, int nh, int T, float scale, int tiles, otp_attn_drop drop) {
    tokattn_bwd_a_body<NCB, true>(q, k, v, mask, out, lse, dout, dq, dsum, C, nh, T, scale, tiles, drop);
}

// with DROP: the staged side is the query side, so a lane's 16 entries of a tile are 16 rows of the mask at its own key column -
// one hash each; dv sums P m dO, dk the same dS as pass A
template <int NCB, bool DROP>
__device__ __forceinline__ void tokattn_bwd_b_body(const float* __restrict__ q, const float* __restrict__ k,
                                                   const float* __restrict__ v, const unsigned char* __restrict__ mask,
                                                   const float* __restrict__ lse, const float* __restrict__ dout,
                                                   const float* __restrict__ dsum, float* __restrict__ dk,
                                                   float* __restrict__ dv, int C, int nh, int T, float scale,
                                                   int tiles, const otp_attn_drop& drop) {
    extern __shared__ __attribute__((aligned(16))) float ta_smem[];
    float* Qs = ta_smem;
    float* Gs = Qs + 16 * NCB * TA_STRIDE;
    float* lse_s = Gs + 16 * NCB * TA_STRIDE;
    float* dsum_s = lse_s + TA_TILE;
    const int hd = C / nh, bh = blockIdx.x / tiles, b = bh / nh, h = bh - b * nh;
    const int lane = threadIdx.x & 63, n = lane & 15, g = lane >> 4;
    const int tk = (blockIdx.x - bh * tiles) * TA_TILE + (threadIdx.x >> 6) * 16 + n;
    const size_t head = ((size_t)b * C + (size_t)h * hd) * T;
    const bool key_live = tk < T && !(mask && mask[(size_t)b * T + tk]);

    float kf[4 * NCB], vf[4 * NCB];
    ta_frags<NCB>(kf, k + head, hd, T, tk);
    ta_frags<NCB>(vf, v + head, hd, T, tk);
    otp_f32x4 gk[NCB], gv[NCB];
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) gk[cb] = gv[cb] = otp_f32x4{0.f, 0.f, 0.f, 0.f};

    for (int qt = 0; qt < tiles; ++qt) {
        __syncthreads();
        ta_stage<NCB>(Qs, q + head, hd, T, qt * TA_TILE);
        ta_stage<NCB>(Gs, dout + head, hd, T, qt * TA_TILE);
        if (threadIdx.x < TA_TILE) {
            const int t = qt * TA_TILE + threadIdx.x;
            lse_s[threadIdx.x] = t < T ? lse[(size_t)bh * T + t] : INFINITY;      // a query past T: P = exp(-inf) = 0
            dsum_s[threadIdx.x] = t < T ? dsum[(size_t)bh * T + t] : 0.f;
        }
        __syncthreads();
        otp_f32x4 s[4], dp[4];
#pragma unroll
        for (int qb = 0; qb < 4; ++qb) s[qb] = dp[qb] = otp_f32x4{0.f, 0.f, 0.f, 0.f};
        ta_first<NCB>(s, Qs, kf);
        ta_first<NCB>(dp, Gs, vf);
        // the pair of (first query of this lane group, own key); one row further is ceil(T / 2) pairs further
        const uint64_t pair0 = DROP ? otp_attn_drop_row((uint64_t)bh * T + (uint64_t)(qt * TA_TILE + 16 * g), T) + (uint64_t)(tk >> 1) : 0;
        const uint64_t row_pairs = (uint64_t)((T + 1) >> 1);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const otp_f32x4 l4 = *reinterpret_cast<const otp_f32x4*>(lse_s + 16 * g + 4 * r);
            const otp_f32x4 d4 = *reinterpret_cast<const otp_f32x4*>(dsum_s + 16 * g + 4 * r);
#pragma unroll
            for (int qb = 0; qb < 4; ++qb) {
                const float p = key_live ? expf(__fmul_rn(s[qb][r], scale) - l4[qb]) : 0.f;
                if (DROP) {
                    const float f = otp_attn_drop_factor(drop, otp_attn_drop_draw(drop, pair0 + (4 * r + qb) * row_pairs), tk);
                    s[qb][r] = p * f;
                    dp[qb][r] = p * (f * dp[qb][r] - d4[qb]);
                } else {
                    s[qb][r] = p;
                    dp[qb][r] = p * (dp[qb][r] - d4[qb]);
                }
            }
        }
        ta_second<NCB>(gv, Gs, s);
        ta_second<NCB>(gk, Qs, dp);
    }
    ta_store<NCB>(dk + head, gk, scale, hd, T, tk);
    ta_store<NCB>(dv + head, gv, 1.f, hd, T, tk);
}
template <int NCB>
__global__ __launch_bounds__(TA_THREADS) void tokattn_bwd_b_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                                   const float* __restrict__ v, const unsigned char* __restrict__ mask,
                                                                   const float* __restrict__ lse, const float* __restrict__ dout,
                                                                   const float* __restrict__ dsum, float* __restrict__ dk,
                                                                   float* __restrict__ dv, int C, int nh, int T, float scale,
                                                                   int tiles) {
    tokattn_bwd_b_body<NCB, false>(q, k, v, mask, lse, dout, dsum, dk, dv, C, nh, T, scale, tiles, otp_attn_drop{});
}
template <int NCB>
__global__ __launch_bounds__(TA_THREADS) void tokattn_bwd_b_drop_kernel(
    const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v, const unsigned char* __restrict__ mask,
    const float* __restrict__ lse, const float* __restrict__ dout, const float* __restrict__ dsum, float* __restrict__ dk,
    float* __restrict__ dv, int C, int nh, int T, float scale, int tiles, otp_attn_drop drop) {
    tokattn_bwd_b_body<NCB, true>(q, k, v, mask, lse, dout, dsum, dk, dv, C, nh, T, scale, tiles, drop);
}

template <int NCB>
__global__ __launch_bounds__(TA_THREADS) void tokattn_map_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                                 const unsigned char* __restrict__ mask, const float* __restrict__ lse,
                                                                 float* __restrict__ map, int C, int nh, int T, float scale,
                                                                 int tiles) {
    extern __shared__ __attribute__((aligned(16))) float ta_smem[];
    float* Ks = ta_smem;
    float* kbias = Ks + 2 * 16 * NCB * TA_STRIDE;
    const int hd = C / nh, b = blockIdx.x / (tiles * tiles), rest = blockIdx.x - b * tiles * tiles, qt = rest / tiles,
              kt = rest - qt * tiles;
    const int lane = threadIdx.x & 63, n = lane & 15, g = lane >> 4;
    const int tq = qt * TA_TILE + (threadIdx.x >> 6) * 16 + n;
    ta_stage_keys(kbias, ta_key_live(mask ? mask + (size_t)b * T : nullptr, T, kt * TA_TILE));
    otp_f32x4 mean[4];
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) mean[kb] = otp_f32x4{0.f, 0.f, 0.f, 0.f};
    for (int h = 0; h < nh; ++h) {
        const size_t head = ((size_t)b * C + (size_t)h * hd) * T;
        __syncthreads();
        ta_stage<NCB>(Ks, k + head, hd, T, kt * TA_TILE);
        __syncthreads();
        float qf[4 * NCB];
        ta_frags<NCB>(qf, q + head, hd, T, tq);
        const float lse_q = tq < T ? lse[((size_t)b * nh + h) * T + tq] : 0.f;
        otp_f32x4 s[4];
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) s[kb] = otp_f32x4{0.f, 0.f, 0.f, 0.f};
        ta_first<NCB>(s, Ks, qf);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const otp_f32x4 kb4 = *reinterpret_cast<const otp_f32x4*>(kbias + 16 * g + 4 * r);
#pragma unroll
            for (int kb = 0; kb < 4; ++kb)
                mean[kb][r] += expf(__fadd_rn(__fmul_rn(s[kb][r], scale), kb4[kb]) - lse_q);
        }
    }
    if (tq >= T) return;
    float* row = map + ((size_t)b * T + tq) * T;
    const float div = (float)nh;
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) {
            const int tk = kt * TA_TILE + 16 * g + 4 * r + kb;
            if (tk < T) row[tk] = mean[kb][r] / div;
        }
}

bool ta_shape_ok(int B, int C, int nh, int T) { return B > 0 && otp_token_attn_supported(C, nh, T); }

// workgroups of a launch over `tiles` tiles of `groups` groups, 0 when the count does not fit a grid
unsigned ta_grid(size_t groups, size_t tiles) {
    const size_t n = groups * tiles;
    return n < (1ull << 31) ? (unsigned)n : 0u;
}

// one case per head-size class: the accumulator arrays are indexed by compile-time constants only, so they stay in registers
#define TA_DISPATCH(ncb_, CALL)                                                                                        \
    switch (ncb_) {                                                                                                    \
        case 1: { constexpr int N = 1; CALL; } break; case 2: { constexpr int N = 2; CALL; } break;                    \
        case 3: { constexpr int N = 3; CALL; } break; case 4: { constexpr int N = 4; CALL; } break;                    \
        case 5: { constexpr int N = 5; CALL; } break; case 6: { constexpr int N = 6; CALL; } break;                    \
        case 7: { constexpr int N = 7; CALL; } break; case 8: { constexpr int N = 8; CALL; } break;                    \
        default: { constexpr int N = 9; CALL; } break;                                                                 \
    }

#define TA_LAUNCH(kern, grid, st, ...)                                                                                 \
    do {                                                                                                               \
        OTP_ALLOW_BIG_LDS(kern<N>, ta_lds_bytes<N>());                                                                 \
        hipLaunchKernelGGL(kern<N>, dim3(grid), dim3(TA_THREADS), ta_lds_bytes<N>(), st, __VA_ARGS__);                 \
    } while (0)

}  // namespace

extern "C" int otp_token_attn_supported(int C, int nh, int T) {
    return C > 0 && nh > 0 && C % nh == 0 && C / nh <= TA_MAX_HD && T >= 1 && T <= TA_MAX_T;
}

extern "C" size_t otp_token_attn_workspace(int B, int nh, int T, int hd) {
    if (B <= 0 || nh <= 0 || T <= 0 || hd <= 0 || hd > TA_MAX_HD) return 0;
    return (size_t)B * nh * T * sizeof(float);                     // D = rowsum(dO o O), written by pass A for pass B
}

extern "C" int otp_token_attn_forward(const void* q, const void* k, const void* v, const void* key_mask, void* out, void* lse,
                                      int B, int C, int nh, int T, float scale, void* stream) {
    if (!q || !k || !v || !out || !ta_shape_ok(B, C, nh, T)) return OTP_ERR_BAD_ARG;
    const int tiles = otp_ceil_div(T, TA_TILE);
    const unsigned grid = ta_grid((size_t)B * nh, tiles);
    if (!grid) return OTP_ERR_UNSUPPORTED;
    auto st = static_cast<hipStream_t>(stream);
    TA_DISPATCH(otp_ceil_div(C / nh, 16),
                TA_LAUNCH(tokattn_fwd_kernel, grid, st, static_cast<const float*>(q), static_cast<const float*>(k),
                          static_cast<const float*>(v), static_cast<const unsigned char*>(key_mask), static_cast<float*>(out),
                          static_cast<float*>(lse), C, nh, T, scale, tiles));
    return otp_launch_status();
}

extern "C" int otp_token_attn_backward(const void* q, const void* k, const void* v, const void* key_mask, const void* out,
                                       const void* lse, const void* dout, void* dq, void* dk, void* dv, void* workspace, int B,
                                       int C, int nh, int T, float scale, void* stream) {
    if (!q || !k || !v || !out || !lse || !dout || !dq || !dk || !dv || !workspace || !ta_shape_ok(B, C, nh, T))
        return OTP_ERR_BAD_ARG;
    const int tiles = otp_ceil_div(T, TA_TILE);
    const unsigned grid = ta_grid((size_t)B * nh, tiles);
    if (!grid) return OTP_ERR_UNSUPPORTED;
    auto st = static_cast<hipStream_t>(stream);
    const float *qf = static_cast<const float*>(q), *kf = static_cast<const float*>(k), *vf = static_cast<const float*>(v),
                *lf = static_cast<const float*>(lse), *gf = static_cast<const float*>(dout);
    const unsigned char* mf = static_cast<const unsigned char*>(key_mask);
    float* dsum = static_cast<float*>(workspace);
    TA_DISPATCH(otp_ceil_div(C / nh, 16), {
        TA_LAUNCH(tokattn_bwd_a_kernel, grid, st, qf, kf, vf, mf, static_cast<const float*>(out), lf, gf, static_cast<float*>(dq),
                  dsum, C, nh, T, scale, tiles);
        TA_LAUNCH(tokattn_bwd_b_kernel, grid, st, qf, kf, vf, mf, lf, gf, static_cast<const float*>(dsum), static_cast<float*>(dk),
                  static_cast<float*>(dv), C, nh, T, scale, tiles);
    });
    return otp_launch_status();
}

extern "C" int otp_token_attn_forward_dropout(const void* q, const void* k, const void* v, const void* key_mask, void* out, void* lse,
                                              int B, int C, int nh, int T, float scale, float p, unsigned long long seed,
                                              void* stream) {
    if (!q || !k || !v || !out || !ta_shape_ok(B, C, nh, T) || !otp_attn_drop_rate_ok(p)) return OTP_ERR_BAD_ARG;
    const otp_attn_drop drop = otp_attn_drop_make(p, seed);
    if (!drop.thr) return otp_token_attn_forward(q, k, v, key_mask, out, lse, B, C, nh, T, scale, stream);
    const int tiles = otp_ceil_div(T, TA_TILE);
    const unsigned grid = ta_grid((size_t)B * nh, tiles);
    if (!grid) return OTP_ERR_UNSUPPORTED;
    auto st = static_cast<hipStream_t>(stream);
    TA_DISPATCH(otp_ceil_div(C / nh, 16),
                TA_LAUNCH(tokattn_fwd_drop_kernel, grid, st, static_cast<const float*>(q), static_cast<const float*>(k),
                          static_cast<const float*>(v), static_cast<const unsigned char*>(key_mask), static_cast<float*>(out),
                          static_cast<float*>(lse), C, nh, T, scale, tiles, drop));
    return otp_launch_status();
}

extern "C" int otp_token_attn_backward_dropout(const void* q, const void* k, const void* v, const void* key_mask, const void* out,
                                               const void* lse, const void* dout, void* dq, void* dk, void* dv, void* workspace,
                                               int B, int C, int nh, int T, float scale, float p, unsigned long long seed,
                                               void* stream) {
    if (!q || !k || !v || !out || !lse || !dout || !dq || !dk || !dv || !workspace || !ta_shape_ok(B, C, nh, T) ||
        !otp_attn_drop_rate_ok(p))
        return OTP_ERR_BAD_ARG;
    const otp_attn_drop drop = otp_attn_drop_make(p, seed);
    if (!drop.thr) return otp_token_attn_backward(q, k, v, key_mask, out, lse, dout, dq, dk, dv, workspace, B, C, nh, T, scale, stream);
    const int tiles = otp_ceil_div(T, TA_TILE);
    const unsigned grid = ta_grid((size_t)B * nh, tiles);
    if (!grid) return OTP_ERR_UNSUPPORTED;
    auto st = static_cast<hipStream_t>(stream);
    const float *qf = static_cast<const float*>(q), *kf = static_cast<const float*>(k), *vf = static_cast<const float*>(v),
                *lf = static_cast<const float*>(lse), *gf = static_cast<const float*>(dout);
    const unsigned char* mf = static_cast<const unsigned char*>(key_mask);
    float* dsum = static_cast<float*>(workspace);
    TA_DISPATCH(otp_ceil_div(C / nh, 16), {
        TA_LAUNCH(tokattn_bwd_a_drop_kernel, grid, st, qf, kf, vf, mf, static_cast<const float*>(out), lf, gf,
                  static_cast<float*>(dq), dsum, C, nh, T, scale, tiles, drop);
        TA_LAUNCH(tokattn_bwd_b_drop_kernel, grid, st, qf, kf, vf, mf, lf, gf, static_cast<const float*>(dsum),
                  static_cast<float*>(dk), static_cast<float*>(dv), C, nh, T, scale, tiles, drop);
    });
    return otp_launch_status();
}

extern "C" int otp_token_attn_map(const void* q, const void* k, const void* key_mask, const void* lse, void* map, int B, int C,
                                  int nh, int T, float scale, void* stream) {
    if (!q || !k || !lse || !map || !ta_shape_ok(B, C, nh, T)) return OTP_ERR_BAD_ARG;
    const int tiles = otp_ceil_div(T, TA_TILE);
    const unsigned grid = ta_grid((size_t)B * tiles, tiles);
    if (!grid) return OTP_ERR_UNSUPPORTED;
    auto st = static_cast<hipStream_t>(stream);
    TA_DISPATCH(otp_ceil_div(C / nh, 16),
                TA_LAUNCH(tokattn_map_kernel, grid, st, static_cast<const float*>(q), static_cast<const float*>(k),
                          static_cast<const unsigned char*>(key_mask), static_cast<const float*>(lse), static_cast<float*>(map), C,
                          nh, T, scale, tiles));
    return otp_launch_status();
}
