// Token x token self-attention with IEEE-half products: the arithmetic mode `products = "half"` of otpose_amd/token_attn.py.
//   S[i][j] = sum_c h(scale q[c][i]) h(k[c][j]),  P = softmax_j(S),  O[c][i] = sum_j h(P[i][j]) h(v[c][j]) / sum_j P[i][j]
// h() = round to nearest even IEEE half; every sum is an fp32 MFMA accumulator (D = sum_c h(dO) h(O) among them: see backward A),
// the online softmax, lse and every store are fp32.  Same operands as csrc/tokattn.hip: fp32 (B, C, T) tensors, the uint8 key
// mask, lse (B, nh, T), a workspace that grows with T only.  Nothing is converted in HBM: the halves exist in the LDS tiles and in
// registers only.
//
// Shape of the products: v_mfma_f32_16x16x16_f16 (4 halves per lane and operand).  Its accumulator holds, in lane (n = lane & 15,
// g = lane >> 4), rows 4 g .. 4 g + 3 of column n; its B operand holds k = 4 g .. 4 g + 3 of column n.  With the first product
// transposed, S^T = K Q^T (rows: staged tokens, columns: the wave's 16 register-side tokens), the four accumulator words of a lane
// ARE the B fragment of the second product O^T = V P^T after one packed conversion: P never leaves the registers and needs no
// lane movement.  The k = 32 shape holds 8 consecutive k per lane, so the same hand-over would need a permute between lane
// groups (or a trip through the LDS) per key block; at the widths of this model (hd = 17 .. 136) the products are a small part
// of a tile next to the exponentials and the LDS reads, so the shape that keeps P in place was chosen.
//
// Tile scheme (as the fp32 family): a workgroup of 4 waves holds 64 tokens of one side in registers, 16 per wave, and walks the
// other side in 64-token tiles staged in the LDS as halves.  The A operand of a product is 4 consecutive halves (one ds_read_b64)
//   first product  (sums over channels):      token-major image   xt[64 tokens][16 NCB + 8],  lane reads xt[16 kb + n][16 s + 4 g ..]
//   second product (sums over staged tokens): channel-major image xc[16 NCB channels][72],    lane reads xc[16 cb + n][16 kb + 4 g ..]
// Row strides 16 NCB + 8 and 72 halves are 4 x odd dwords: the 16 lanes of a group start 4 banks apart modulo 64 and the second
// group of a half-wave sits 2 banks further, so the 32 lanes of one ds_read_b64 cycle cover the 64 banks once.  A tensor that
// feeds both products (K in backward A; Q and dO in backward B) is staged into both images from one HBM read.
//
//   forward     per (b, h, query tile): key tiles of K (token-major) and V (channel-major)              40.4 KB at hd = 136
//   backward A  per (b, h, query tile): K (both images), V (token-major); D and dq                      59.8 KB
//   backward B  per (b, h, key tile):   Q scale and dO (both images each); dk and dv                    80.9 KB
// Every output word has one writer; there are no atomics.  Masking is the fp32 family's: -inf before the maximum, a tile without
// a live key skipped before its loads and barriers on a workgroup-uniform ballot, exactly zero dk / dv for a masked key.
// Gradient scale: dO enters the products times 2^e, one e per 64-query tile (backward A), so that a small gradient does not
// fall into a half's subnormal range; dP, D and dS live at that scale and dq, dk, dv are scaled back at their stores.
// Range guard: scale q, k, v, dO and the scaled dS are tested against a half's range while they are converted (common.h:
// otp_out_of_range); a violation stores OTP_RANGE_TOKATTN_H into the guard word.
#include "common.h"

#include <math.h>

namespace {

constexpr int TH_TILE = 64, TH_CSTRIDE = 72, TH_THREADS = 256, TH_MAX_HD = 136;
constexpr int TH_MAX_T = 1 << 30;
constexpr int TH_GEXP_MAX = 40;                                    // |e| of a query tile's gradient scale 2^e

typedef _Float16 th_h4 __attribute__((ext_vector_type(4)));

template <int NCB> constexpr int th_tstride() { return 16 * NCB + 8; }                    // halves per token row
template <int NCB> constexpr int th_timage() { return TH_TILE * th_tstride<NCB>(); }      // halves of a token-major image
template <int NCB> constexpr int th_cimage() { return 16 * NCB * TH_CSTRIDE; }            // halves of a channel-major image
// NT token-major and NC channel-major images and two 64-word fp32 rows
template <int NCB, int NT, int NC>
constexpr int th_lds_bytes() { return (NT * th_timage<NCB>() + NC * th_cimage<NCB>()) * 2 + 2 * TH_TILE * (int)sizeof(float); }

__device__ __forceinline__ otp_f32x4 th_mfma(th_h4 a, th_h4 b, otp_f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x16f16(a, b, c, 0, 0, 0);
}
// e with amax 2^e in [1, 2), 0 for an all-zero (or non-finite) tile, clamped so that moving an accumulator between two tiles'
// scales stays inside fp32
__device__ __forceinline__ int th_grad_exponent(float amax) {
    if (!(amax > 0.f) || !(amax < INFINITY)) return 0;
    return min(max(-ilogbf(amax), -TH_GEXP_MAX), TH_GEXP_MAX);
}
__device__ __forceinline__ th_h4 th_round(otp_f32x4 x) { return __builtin_convertvector(x, th_h4); }

// columns t0 .. t0 + 63 of the hd rows of one head (src: its first channel), times mul, as halves into the token-major image xt
// (TM) and / or the channel-major image xc (CM); zeros past hd and past T.  One thread: one token, four neighbouring channels.
template <int NCB, bool TM, bool CM>
__device__ __forceinline__ void th_stage(_Float16* xt, _Float16* xc, const float* __restrict__ src, int hd, int T, int t0,
                                         float mul, bool& bad) {
    const int col = threadIdx.x & 63, t = t0 + col;
    const bool tv = t < T;
#pragma unroll 2
    for (int cg = threadIdx.x >> 6; cg < 4 * NCB; cg += TH_THREADS / 64) {
        otp_f32x4 x;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = 4 * cg + j;
            x[j] = (tv && c < hd) ? src[(size_t)c * T + t] * mul : 0.f;
            bad |= otp_out_of_range(x[j]);
        }
        const th_h4 h = th_round(x);
        if (TM) *reinterpret_cast<th_h4*>(xt + col * th_tstride<NCB>() + 4 * cg) = h;
        if (CM) {
#pragma unroll
            for (int j = 0; j < 4; ++j) xc[(4 * cg + j) * TH_CSTRIDE + col] = h[j];
        }
    }
}

// the B operands of the first product: f[s][j] = h(mul x[16 s + 4 g + j][t]) for this lane's token t; zeros past hd and past T
template <int NCB>
__device__ __forceinline__ void th_frags(th_h4 (&f)[NCB], const float* __restrict__ src, int hd, int T, int t, float mul,
                                         bool& bad) {
    const int g = (threadIdx.x & 63) >> 4;
#pragma unroll
    for (int s = 0; s < NCB; ++s) {
        otp_f32x4 x;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = 16 * s + 4 * g + j;
            x[j] = (c < hd && t < T) ? src[(size_t)c * T + t] * mul : 0.f;
            bad |= otp_out_of_range(x[j]);
        }
        f[s] = th_round(x);
    }
}

// acc[kb][r] (lane n, g: staged token 16 kb + 4 g + r, register-side token n) += sum_c xt[token][c] f[c][n]
template <int NCB>
__device__ __forceinline__ void th_first(otp_f32x4 (&acc)[4], const _Float16* xt, const th_h4 (&f)[NCB]) {
    const int lane = threadIdx.x & 63, n = lane & 15, g = lane >> 4;
    const _Float16* base = xt + n * th_tstride<NCB>() + 4 * g;
#pragma unroll
    for (int s = 0; s < NCB; ++s)
#pragma unroll
        for (int kb = 0; kb < 4; ++kb)
            acc[kb] = th_mfma(*reinterpret_cast<const th_h4*>(base + 16 * kb * th_tstride<NCB>() + 16 * s), f[s], acc[kb]);
}

// o[cb][r] (lane n, g: channel 16 cb + 4 g + r, token n) += sum over the 64 staged tokens j of xc[channel][j] h(p[j][n])
template <int NCB>
__device__ __forceinline__ void th_second(otp_f32x4 (&o)[NCB], const _Float16* xc, const otp_f32x4 (&p)[4]) {
    const int lane = threadIdx.x & 63, n = lane & 15, g = lane >> 4;
    const _Float16* base = xc + n * TH_CSTRIDE + 4 * g;
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) {
        const th_h4 b = th_round(p[kb]);
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb)
            o[cb] = th_mfma(*reinterpret_cast<const th_h4*>(base + 16 * cb * TH_CSTRIDE + 16 * kb), b, o[cb]);
    }
}

// o[cb][r] -> dst[16 cb + 4 g + r][t] (dst: the head's first channel), times mul
template <int NCB>
__device__ __forceinline__ void th_store(float* __restrict__ dst, const otp_f32x4 (&o)[NCB], float mul, int hd, int T, int t) {
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

// whether key t0 + lane of the tile is live: the 64 keys of a tile are the 64 lanes of EVERY wave, so __ballot of it is the same
// word in all four waves - a decision on it is uniform over the workgroup
__device__ __forceinline__ bool th_key_live(const unsigned char* __restrict__ mask_row, int T, int t0) {
    const int t = t0 + (threadIdx.x & 63);
    return t < T && !(mask_row && mask_row[t]);
}
__device__ __forceinline__ void th_stage_keys(float* kbias, bool live) {
    if (threadIdx.x < TH_TILE) kbias[threadIdx.x] = live ? 0.f : -INFINITY;
}

// Attention-probability dropout (common.h: otp_attn_drop), applied to the fp32 P in front of its conversion.  A lane's staged
// tokens 16 kb + 4 g + r of a tile: r = 0, 1 share one hash and r = 2, 3 the next where the staged side is the key side.
template <int NCB, bool DROP>
__global__ __launch_bounds__(TH_THREADS) void tokattn_h_fwd_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                                   const float* __restrict__ v,
                                                                   const unsigned char* __restrict__ mask, float* __restrict__ out,
                                                                   float* __restrict__ lse, int C, int nh, int T, float scale,
                                                                   int tiles, otp_attn_drop drop, unsigned* rword) {
    extern __shared__ __attribute__((aligned(16))) unsigned char th_smem[];
    _Float16* Kt = reinterpret_cast<_Float16*>(th_smem);
    _Float16* Vc = Kt + th_timage<NCB>();
    float* kbias = reinterpret_cast<float*>(Vc + th_cimage<NCB>());
    const int hd = C / nh, bh = blockIdx.x / tiles, b = bh / nh, h = bh - b * nh;
    const int lane = threadIdx.x & 63, n = lane & 15, g = lane >> 4;
    const int tq = (blockIdx.x - bh * tiles) * TH_TILE + (threadIdx.x >> 6) * 16 + n;
    const size_t head = ((size_t)b * C + (size_t)h * hd) * T;
    const unsigned char* mask_row = mask ? mask + (size_t)b * T : nullptr;
    bool bad = false;

    th_h4 qf[NCB];
    th_frags<NCB>(qf, q + head, hd, T, tq, scale, bad);
    otp_f32x4 o[NCB];
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) o[cb] = otp_f32x4{0.f, 0.f, 0.f, 0.f};
    float m = -INFINITY, l = 0.f;
    const uint64_t drop_row = DROP ? otp_attn_drop_row((uint64_t)bh * T + tq, T) : 0;

    for (int kt = 0; kt < tiles; ++kt) {
        const bool live = th_key_live(mask_row, T, kt * TH_TILE);
        if (!__ballot(live)) continue;        // a tile without a live key: no load, no barrier, m, l and O untouched (uniform)
        __syncthreads();                                           // the previous tile has been read
        th_stage<NCB, true, false>(Kt, nullptr, k + head, hd, T, kt * TH_TILE, 1.f, bad);
        th_stage<NCB, false, true>(nullptr, Vc, v + head, hd, T, kt * TH_TILE, 1.f, bad);
        th_stage_keys(kbias, live);
        __syncthreads();
        otp_f32x4 s[4];
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) s[kb] = otp_f32x4{0.f, 0.f, 0.f, 0.f};
        th_first<NCB>(s, Kt, qf);
        float mt = -INFINITY;
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) {
            const otp_f32x4 kb4 = *reinterpret_cast<const otp_f32x4*>(kbias + 16 * kb + 4 * g);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                s[kb][r] = __fadd_rn(s[kb][r], kb4[r]);
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
            const uint64_t pair0 = drop_row + (uint64_t)((kt * TH_TILE + 4 * g) >> 1);
#pragma unroll
            for (int kb = 0; kb < 4; ++kb)
#pragma unroll
                for (int h2 = 0; h2 < 2; ++h2) {
                    const uint32_t hh = otp_attn_drop_draw(drop, pair0 + 8 * kb + h2);
                    s[kb][2 * h2] *= otp_attn_drop_factor(drop, hh, 0);
                    s[kb][2 * h2 + 1] *= otp_attn_drop_factor(drop, hh, 1);
                }
        }
        th_second<NCB>(o, Vc, s);
    }
    th_store<NCB>(out + head, o, 1.f / l, hd, T, tq);
    if (lse && g == 0 && tq < T) lse[(size_t)bh * T + tq] = m + logf(l);
    otp_range_report(rword, bad, OTP_RANGE_TOKATTN_H);
}

// with DROP: dP[i][j] = m[i][j] (dO_i . v_j); D = sum_c dO O is the row sum of P m dP already, O being the dropped output
template <int NCB, bool DROP>
__global__ __launch_bounds__(TH_THREADS) void tokattn_h_bwd_a_kernel(
    const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v, const unsigned char* __restrict__ mask,
    const float* __restrict__ out, const float* __restrict__ lse, const float* __restrict__ dout, float* __restrict__ dq,
    float* __restrict__ dsum, float* __restrict__ gexp, int C, int nh, int T, float scale, int tiles, otp_attn_drop drop,
    unsigned* rword) {
    extern __shared__ __attribute__((aligned(16))) unsigned char th_smem[];
    _Float16* Kt = reinterpret_cast<_Float16*>(th_smem);
    _Float16* Vt = Kt + th_timage<NCB>();
    _Float16* Kc = Vt + th_timage<NCB>();
    float* kbias = reinterpret_cast<float*>(Kc + th_cimage<NCB>());
    const int hd = C / nh, bh = blockIdx.x / tiles, b = bh / nh, h = bh - b * nh;
    const int lane = threadIdx.x & 63, n = lane & 15, g = lane >> 4;
    const int tq = (blockIdx.x - bh * tiles) * TH_TILE + (threadIdx.x >> 6) * 16 + n;
    const size_t head = ((size_t)b * C + (size_t)h * hd) * T;
    const unsigned char* mask_row = mask ? mask + (size_t)b * T : nullptr;
    bool bad = false;

    th_h4 qf[NCB], gf[NCB];
    th_frags<NCB>(qf, q + head, hd, T, tq, scale, bad);
    // dO is a gradient: behind a mean-reduced loss its entries sit far below 2^-14, where a half is subnormal (or zero) and keeps
    // no relative precision.  The query tile therefore carries one power of two, 2^e with max|dO| 2^e in [1, 2): h(2^e dO) goes
    // into the products, dP, D and dS are formed at that scale (exact: a power of two commutes with every rounding above the
    // subnormals) and dq is scaled back at its store.  e is kept for pass B behind D in the workspace.
    float amax = 0.f;
#pragma unroll
    for (int s = 0; s < NCB; ++s)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = 16 * s + 4 * g + j;
            const float x = (c < hd && tq < T) ? dout[head + (size_t)c * T + tq] : 0.f;
            bad |= otp_out_of_range(x);
            amax = fmaxf(amax, __builtin_fabsf(x));
        }
    amax = wave_max(amax);
    if (lane == 0) kbias[TH_TILE + (threadIdx.x >> 6)] = amax;
    __syncthreads();
    amax = fmaxf(fmaxf(kbias[TH_TILE], kbias[TH_TILE + 1]), fmaxf(kbias[TH_TILE + 2], kbias[TH_TILE + 3]));
    const int ge = th_grad_exponent(amax);
    const float gup = ldexpf(1.f, ge), gdown = ldexpf(1.f, -ge);
    if (threadIdx.x == 0) gexp[blockIdx.x] = (float)ge;
    {
        bool unused = false;                                       // the unscaled dO was tested above
        th_frags<NCB>(gf, dout + head, hd, T, tq, gup, unused);
    }
    // D[i] = sum_c dO[c][i] O[c][i] on the same instruction, from the same h(dO) and in the same channel order as dP below: the
    // diagonal of O^T dO over the wave's 16 tokens (fp32 accumulator).  dS = P (dP - D) cancels: where P is one-hot (a single live
    // key) O is h(v) of that key exactly, D equals dP bit for bit and dq, dk are exact zeros - a D summed in fp32 from the
    // unrounded dO differs from the half-product dP by the rounding of dO, which the cancellation would amplify.
    th_h4 of[NCB];
    {
        bool unused = false;                                       // |O| <= max|v|, which the forward has tested
        th_frags<NCB>(of, out + head, hd, T, tq, 1.f, unused);
    }
    otp_f32x4 dd = otp_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < NCB; ++s) dd = th_mfma(of[s], gf[s], dd);  // dd[r] (lane n, g) = sum_c O[c][token 4 g + r] dO[c][token n]
    const int dr = n & 3;
    const float diag = dr == 0 ? dd[0] : dr == 1 ? dd[1] : dr == 2 ? dd[2] : dd[3];
    const float dsum_q = __shfl(diag, 16 * (n >> 2) + n, 64);      // the lane that holds row n of column n
    const float lse_q = tq < T ? lse[(size_t)bh * T + tq] : 0.f;
    if (g == 0 && tq < T) dsum[(size_t)bh * T + tq] = dsum_q * gdown;       // dsum_q itself stays at the tile's scale
    otp_f32x4 acc[NCB];
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) acc[cb] = otp_f32x4{0.f, 0.f, 0.f, 0.f};
    const uint64_t drop_row = DROP ? otp_attn_drop_row((uint64_t)bh * T + tq, T) : 0;

    for (int kt = 0; kt < tiles; ++kt) {
        const bool live = th_key_live(mask_row, T, kt * TH_TILE);
        if (!__ballot(live)) continue;                             // P = 0 on the whole tile (uniform over the workgroup)
        __syncthreads();
        th_stage<NCB, true, true>(Kt, Kc, k + head, hd, T, kt * TH_TILE, 1.f, bad);
        th_stage<NCB, true, false>(Vt, nullptr, v + head, hd, T, kt * TH_TILE, 1.f, bad);
        th_stage_keys(kbias, live);
        __syncthreads();
        otp_f32x4 s[4], dp[4];
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) s[kb] = dp[kb] = otp_f32x4{0.f, 0.f, 0.f, 0.f};
        th_first<NCB>(s, Kt, qf);
        th_first<NCB>(dp, Vt, gf);
        if (DROP) {
            const uint64_t pair0 = drop_row + (uint64_t)((kt * TH_TILE + 4 * g) >> 1);
#pragma unroll
            for (int kb = 0; kb < 4; ++kb)
#pragma unroll
                for (int h2 = 0; h2 < 2; ++h2) {
                    const uint32_t hh = otp_attn_drop_draw(drop, pair0 + 8 * kb + h2);
                    dp[kb][2 * h2] *= otp_attn_drop_factor(drop, hh, 0);
                    dp[kb][2 * h2 + 1] *= otp_attn_drop_factor(drop, hh, 1);
                }
        }
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) {
            const otp_f32x4 kb4 = *reinterpret_cast<const otp_f32x4*>(kbias + 16 * kb + 4 * g);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float p = expf(__fadd_rn(s[kb][r], kb4[r]) - lse_q);                       // exactly 0 for a dead key
                s[kb][r] = p * (dp[kb][r] - dsum_q);
                bad |= otp_out_of_range(s[kb][r]);                 // dS at the tile's scale is an operand too
            }
        }
        th_second<NCB>(acc, Kc, s);
    }
    th_store<NCB>(dq + head, acc, scale * gdown, hd, T, tq);
    otp_range_report(rword, bad, OTP_RANGE_TOKATTN_H);
}

// with DROP: the staged side is the query side, so a lane's 16 entries of a tile are 16 rows of the mask at its own key column -
// one hash each; dv sums h(P m) h(dO), dk h(dS) h(scale q): the scale is in the staged operand, nothing is multiplied at the store
template <int NCB, bool DROP>
__global__ __launch_bounds__(TH_THREADS) void tokattn_h_bwd_b_kernel(
    const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v, const unsigned char* __restrict__ mask,
    const float* __restrict__ lse, const float* __restrict__ dout, const float* __restrict__ dsum, const float* __restrict__ gexp,
    float* __restrict__ dk, float* __restrict__ dv, int C, int nh, int T, float scale, int tiles, otp_attn_drop drop,
    unsigned* rword) {
    extern __shared__ __attribute__((aligned(16))) unsigned char th_smem[];
    _Float16* Qt = reinterpret_cast<_Float16*>(th_smem);
    _Float16* Gt = Qt + th_timage<NCB>();
    _Float16* Qc = Gt + th_timage<NCB>();
    _Float16* Gc = Qc + th_cimage<NCB>();
    float* lse_s = reinterpret_cast<float*>(Gc + th_cimage<NCB>());
    float* dsum_s = lse_s + TH_TILE;
    const int hd = C / nh, bh = blockIdx.x / tiles, b = bh / nh, h = bh - b * nh;
    const int lane = threadIdx.x & 63, n = lane & 15, g = lane >> 4;
    const int tk = (blockIdx.x - bh * tiles) * TH_TILE + (threadIdx.x >> 6) * 16 + n;
    const size_t head = ((size_t)b * C + (size_t)h * hd) * T;
    const bool key_live = tk < T && !(mask && mask[(size_t)b * T + tk]);
    bool bad = false;

    th_h4 kf[NCB], vf[NCB];
    th_frags<NCB>(kf, k + head, hd, T, tk, 1.f, bad);
    th_frags<NCB>(vf, v + head, hd, T, tk, 1.f, bad);
    otp_f32x4 gk[NCB], gv[NCB];
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) gk[cb] = gv[cb] = otp_f32x4{0.f, 0.f, 0.f, 0.f};
    const uint64_t row_pairs = (uint64_t)((T + 1) >> 1);

    int ge_prev = 0;
    for (int qt = 0; qt < tiles; ++qt) {
        // pass A's power of two of this query tile: dO and D enter at 2^ge, and the accumulators, which sum over tiles of
        // different scales, move to the new tile's scale first (an exact multiplication, like alpha of the online softmax)
        const int ge = (int)gexp[(size_t)bh * tiles + qt];
        const float gup = ldexpf(1.f, ge);
        if (ge != ge_prev) {
            const float move = ldexpf(1.f, ge - ge_prev);
#pragma unroll
            for (int cb = 0; cb < NCB; ++cb) { gk[cb] *= move; gv[cb] *= move; }
            ge_prev = ge;
        }
        __syncthreads();
        th_stage<NCB, true, true>(Qt, Qc, q + head, hd, T, qt * TH_TILE, scale, bad);
        {
            bool unused = false;                                   // pass A has tested the unscaled dO
            th_stage<NCB, true, true>(Gt, Gc, dout + head, hd, T, qt * TH_TILE, gup, unused);
        }
        if (threadIdx.x < TH_TILE) {
            const int t = qt * TH_TILE + threadIdx.x;
            lse_s[threadIdx.x] = t < T ? lse[(size_t)bh * T + t] : INFINITY;      // a query past T: P = exp(-inf) = 0
            dsum_s[threadIdx.x] = t < T ? dsum[(size_t)bh * T + t] * gup : 0.f;
        }
        __syncthreads();
        otp_f32x4 s[4], dp[4];
#pragma unroll
        for (int qb = 0; qb < 4; ++qb) s[qb] = dp[qb] = otp_f32x4{0.f, 0.f, 0.f, 0.f};
        th_first<NCB>(s, Qt, kf);
        th_first<NCB>(dp, Gt, vf);
        // the pair of (first query of this lane group, own key); one row further is ceil(T / 2) pairs further
        const uint64_t pair0 = DROP ? otp_attn_drop_row((uint64_t)bh * T + (uint64_t)(qt * TH_TILE + 4 * g), T) + (uint64_t)(tk >> 1) : 0;
#pragma unroll
        for (int qb = 0; qb < 4; ++qb) {
            const otp_f32x4 l4 = *reinterpret_cast<const otp_f32x4*>(lse_s + 16 * qb + 4 * g);
            const otp_f32x4 d4 = *reinterpret_cast<const otp_f32x4*>(dsum_s + 16 * qb + 4 * g);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float p = key_live ? expf(s[qb][r] - l4[r]) : 0.f;
                if (DROP) {
                    const float f = otp_attn_drop_factor(drop, otp_attn_drop_draw(drop, pair0 + (16 * qb + r) * row_pairs), tk);
                    s[qb][r] = p * f;
                    dp[qb][r] = p * (f * dp[qb][r] - d4[r]);
                } else {
                    s[qb][r] = p;
                    dp[qb][r] = p * (dp[qb][r] - d4[r]);
                }
                bad |= otp_out_of_range(dp[qb][r]);                // dS at the tile's scale is an operand too
            }
        }
        th_second<NCB>(gv, Gc, s);
        th_second<NCB>(gk, Qc, dp);
    }
    const float gdown = ldexpf(1.f, -ge_prev);
    th_store<NCB>(dk + head, gk, gdown, hd, T, tk);
    th_store<NCB>(dv + head, gv, gdown, hd, T, tk);
    otp_range_report(rword, bad, OTP_RANGE_TOKATTN_H);
}

bool th_shape_ok(int B, int C, int nh, int T) { return B > 0 && otp_token_attn_h1_supported(C, nh, T); }

// workgroups of a launch over `tiles` tiles of `groups` groups, 0 when the count does not fit a grid
unsigned th_grid(size_t groups, size_t tiles) {
    const size_t n = groups * tiles;
    return n < (1ull << 31) ? (unsigned)n : 0u;
}

// one case per head-size class: the accumulator arrays are indexed by compile-time constants only, so they stay in registers
#define TH_DISPATCH(ncb_, CALL)                                                                                        \
    switch (ncb_) {                                                                                                    \
        case 1: { constexpr int N = 1; CALL; } break; case 2: { constexpr int N = 2; CALL; } break;                    \
        case 3: { constexpr int N = 3; CALL; } break; case 4: { constexpr int N = 4; CALL; } break;                    \
        case 5: { constexpr int N = 5; CALL; } break; case 6: { constexpr int N = 6; CALL; } break;                    \
        case 7: { constexpr int N = 7; CALL; } break; case 8: { constexpr int N = 8; CALL; } break;                    \
        default: { constexpr int N = 9; CALL; } break;                                                                 \
    }

#define TH_LAUNCH(kern, NT, NC, grid, st, ...)                                                                         \
    do {                                                                                                               \
        constexpr int bytes_ = th_lds_bytes<N, NT, NC>();                                                              \
        OTP_ALLOW_BIG_LDS(kern, bytes_);                                                                               \
        hipLaunchKernelGGL(kern, dim3(grid), dim3(TH_THREADS), bytes_, st, __VA_ARGS__);                               \
    } while (0)

// the guard word of a launch: the caller's, or the library's sticky one (csrc/range.hip)
unsigned* th_word(void* range_word) { return range_word ? static_cast<unsigned*>(range_word) : otp_range_word(); }

}  // namespace

extern "C" int otp_token_attn_h1_supported(int C, int nh, int T) {
    return C > 0 && nh > 0 && C % nh == 0 && C / nh <= TH_MAX_HD && T >= 1 && T <= TH_MAX_T;
}

extern "C" size_t otp_token_attn_h1_workspace(int B, int nh, int T, int hd) {
    if (B <= 0 || nh <= 0 || T <= 0 || hd <= 0 || hd > TH_MAX_HD) return 0;
    // D = rowsum(dO o O) per query and the gradient exponent per query tile, written by pass A for pass B
    return ((size_t)B * nh * T + (size_t)B * nh * otp_ceil_div(T, TH_TILE)) * sizeof(float);
}

extern "C" int otp_token_attn_forward_h1(const void* q, const void* k, const void* v, const void* key_mask, void* out, void* lse,
                                         int B, int C, int nh, int T, float scale, float p, unsigned long long seed,
                                         void* range_word, void* stream) {
    if (!q || !k || !v || !out || !th_shape_ok(B, C, nh, T) || !otp_attn_drop_rate_ok(p)) return OTP_ERR_BAD_ARG;
    const otp_attn_drop drop = otp_attn_drop_make(p, seed);
    const int tiles = otp_ceil_div(T, TH_TILE);
    const unsigned grid = th_grid((size_t)B * nh, tiles);
    if (!grid) return OTP_ERR_UNSUPPORTED;
    auto st = static_cast<hipStream_t>(stream);
    unsigned* word = th_word(range_word);
#define TH_FWD(DROP_)                                                                                                  \
    TH_LAUNCH((tokattn_h_fwd_kernel<N, DROP_>), 1, 1, grid, st, static_cast<const float*>(q), static_cast<const float*>(k), \
              static_cast<const float*>(v), static_cast<const unsigned char*>(key_mask), static_cast<float*>(out),     \
              static_cast<float*>(lse), C, nh, T, scale, tiles, drop, word)
    if (drop.thr) {
        TH_DISPATCH(otp_ceil_div(C / nh, 16), TH_FWD(true));
    } else {
        TH_DISPATCH(otp_ceil_div(C / nh, 16), TH_FWD(false));
    }
#undef TH_FWD
    return otp_launch_status();
}

extern "C" int otp_token_attn_backward_h1(const void* q, const void* k, const void* v, const void* key_mask, const void* out,
                                          const void* lse, const void* dout, void* dq, void* dk, void* dv, void* workspace, int B,
                                          int C, int nh, int T, float scale, float p, unsigned long long seed, void* range_word,
                                          void* stream) {
    if (!q || !k || !v || !out || !lse || !dout || !dq || !dk || !dv || !workspace || !th_shape_ok(B, C, nh, T) ||
        !otp_attn_drop_rate_ok(p))
        return OTP_ERR_BAD_ARG;
    const otp_attn_drop drop = otp_attn_drop_make(p, seed);
    const int tiles = otp_ceil_div(T, TH_TILE);
    const unsigned grid = th_grid((size_t)B * nh, tiles);
    if (!grid) return OTP_ERR_UNSUPPORTED;
    auto st = static_cast<hipStream_t>(stream);
    const float *qf = static_cast<const float*>(q), *kf = static_cast<const float*>(k), *vf = static_cast<const float*>(v),
                *lf = static_cast<const float*>(lse), *gf = static_cast<const float*>(dout);
    const unsigned char* mf = static_cast<const unsigned char*>(key_mask);
    float* dsum = static_cast<float*>(workspace);
    float* gexp = dsum + (size_t)B * nh * T;
    unsigned* word = th_word(range_word);
#define TH_BWD(DROP_)                                                                                                  \
    {                                                                                                                  \
        TH_LAUNCH((tokattn_h_bwd_a_kernel<N, DROP_>), 2, 1, grid, st, qf, kf, vf, mf, static_cast<const float*>(out), lf, gf, \
                  static_cast<float*>(dq), dsum, gexp, C, nh, T, scale, tiles, drop, word);                                  \
        TH_LAUNCH((tokattn_h_bwd_b_kernel<N, DROP_>), 2, 2, grid, st, qf, kf, vf, mf, lf, gf, static_cast<const float*>(dsum), \
                  static_cast<const float*>(gexp), static_cast<float*>(dk), static_cast<float*>(dv), C, nh, T, scale, tiles, drop, word);               \
    }
    if (drop.thr) {
        TH_DISPATCH(otp_ceil_div(C / nh, 16), TH_BWD(true));
    } else {
        TH_DISPATCH(otp_ceil_div(C / nh, 16), TH_BWD(false));
    }
#undef TH_BWD
    return otp_launch_status();
}
