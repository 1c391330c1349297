// Channel attention of MaskedMHCA (reference model/blocks.py:400-453), forward and the pieces its backward is assembled from.
//
// q, k, v (B, C, T) fp32 with T contiguous, viewed as (B, n_head, hs, T).  Per (b, head) the attention matrix is hs x hs and the
// contraction of the scores runs over T:
//   S[i][j] = scale * sum_t q[i][t] k[j][t],  P = softmax_j(S),  O[i][t] = sum_j P[i][j] v[j][t]
// with O stored as out[bh][t][i], the memory image of `out.transpose(2,3).contiguous()` (blocks.py:447).  hs is zero-padded to
// HSP = 16 NB (NB <= 7, hs <= 112) in the slabs and matrices of the workspace, never in q, k, v or out.
//
//   phase 1  scores   per (b, head, slice of T): a partial q k^T slab (HSP x HSP), NS slices so that every CU has a workgroup
//   phase 2  softmax  per (b, head, row): sum of the NS slabs, scale, row softmax -> P; with dropout also m P
//   phase 3  apply    per (b, head, token tile): O^T = v^T P^T (with dropout: m P in the place of P)
// The backward (ChanAttnFunction.backward in otpose_amd/train_ops.py) runs phases 1 and 3 again on other operands
// (dP = dO v^T; dq, dk, dv = dS k, dS^T q, (m P)^T dO) around the helpers of the second half of this file: the layout transpose
// between (t, i) and (i, t) images and the softmax backward.
//
// Phases 1 and 3 come in two forms, chosen by otp_chan_attn_set_split: the f32 matrix cores (v_mfma_f32_16x16x4_f32) and, the
// default, split products on the 16-bit matrix cores.  The two split-product kernels are templates over
// the piece traits P (csrc/common.h): otp_half_pieces for
// the forward, otp_bf16_pieces for otp_chan_attn_scores_bf16p / otp_chan_attn_apply_bf16p, the two attention products of the
// training backward, whose operands are GRADIENTS of unknown magnitude (a half piece flushes 1e-8 to zero; a bfloat16 pair
// keeps 16-17 bits at any magnitude).
#include "x3.h"
#include <atomic>
#include <type_traits>

namespace {

// ---- channel attention ---------------------------------------------------------------------------
// Phase 1: partial scores.  grid (B*nh, NS); a workgroup (4 waves) owns a chunk of T, stages q and k
// tiles [HSP][64] through LDS (coalesced rows) and accumulates the NB x NB 16x16 score tiles with
// v_mfma_f32_16x16x4_f32 (A = q rows, B = k rows, K = time).  Wave w owns tiles w, w+4, ...
constexpr int ATT_TC = 64;            // time steps per staged tile
constexpr int ATT_TCP = ATT_TC + 2;   // LDS row pitch: (row*2 + k) mod 32 distinct inside each half wave

template <int NB>                     // NB = HSP / 16 (5 for hs = 68, 2 for hs = 17)
__global__ __launch_bounds__(256) void attn_scores_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                           float* __restrict__ slabs, int hs, int T, int chunk) {
    constexpr int HSP = NB * 16, NT = NB * NB, TPW = (NT + 3) / 4;
    // float4 items of one [HSP][64] tile: 16 per row; NQ per thread and matrix
    constexpr int NQ = (HSP * (ATT_TC / 4) + 255) / 256;
    __shared__ float ql[HSP * ATT_TCP];
    __shared__ float kl[HSP * ATT_TCP];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int bh = blockIdx.x, s = blockIdx.y;
    const float* qb = q + (size_t)bh * hs * T;
    const float* kb = k + (size_t)bh * hs * T;
    const int t_begin = s * chunk, t_end = min(T, t_begin + chunk);
    otp_f32x4 acc[TPW];
#pragma unroll
    for (int i = 0; i < TPW; ++i) acc[i] = (otp_f32x4){0.f, 0.f, 0.f, 0.f};
    const int r16 = lane & 15, kk = lane >> 4;
    // rows are T floats apart; 16-byte vectors need T % 4 == 0 (and the chunk start is a multiple of 64)
    const bool vec = (T & 3) == 0 && ((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(k)) & 15) == 0;
    otp_f32x4 pq[NQ], pk[NQ];
    auto load_tile = [&](int t0) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < NQ; ++j) {
            const int idx = tid + j * 256;
            const int row = idx / (ATT_TC / 4), t = t0 + 4 * (idx - row * (ATT_TC / 4));
            otp_f32x4 a = {0.f, 0.f, 0.f, 0.f}, b = {0.f, 0.f, 0.f, 0.f};
            if (row < hs && idx < HSP * (ATT_TC / 4)) {
                const float* qp = qb + (size_t)row * T + t;
                const float* kp = kb + (size_t)row * T + t;
                if (vec && t + 3 < t_end) {
                    a = *reinterpret_cast<const otp_f32x4*>(qp);
                    b = *reinterpret_cast<const otp_f32x4*>(kp);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (t + e < t_end) { a[e] = qp[e]; b[e] = kp[e]; }
                }
            }
            pq[j] = a;
            pk[j] = b;
        }
    };
    auto store_tile = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < NQ; ++j) {
            const int idx = tid + j * 256;
            if (idx < HSP * (ATT_TC / 4)) {
                const int row = idx / (ATT_TC / 4), tt = 4 * (idx - row * (ATT_TC / 4));
#pragma unroll
                for (int e = 0; e < 4; ++e) {                  // pitch ATT_TCP = 66 floats: rows are not 16-byte aligned
                    ql[row * ATT_TCP + tt + e] = pq[j][e];
                    kl[row * ATT_TCP + tt + e] = pk[j][e];
                }
            }
        }
    };
    // tile pipeline: the global loads of tile i+1 are in flight while tile i is multiplied
    load_tile(t_begin);
    for (int t0 = t_begin; t0 < t_end; t0 += ATT_TC) {
        __syncthreads();                                       // previous tile fully read
        store_tile();
        __syncthreads();
        if (t0 + ATT_TC < t_end) load_tile(t0 + ATT_TC);
#pragma unroll
        for (int i = 0; i < TPW; ++i) {
            const int tile = wave + 4 * i;
            if (tile < NT) {
                const int ib = tile / NB, jb = tile - ib * NB;
                const float* qa = ql + (ib * 16 + r16) * ATT_TCP + kk;
                const float* ka = kl + (jb * 16 + r16) * ATT_TCP + kk;
#pragma unroll
                for (int ks = 0; ks < ATT_TC; ks += 4)
                    acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(qa[ks], ka[ks], acc[i], 0, 0, 0);
            }
        }
    }
    float* slab = slabs + ((size_t)bh * gridDim.y + s) * HSP * HSP;
#pragma unroll
    for (int i = 0; i < TPW; ++i) {
        const int tile = wave + 4 * i;
        if (tile < NT) {
            const int ib = tile / NB, jb = tile - ib * NB;
#pragma unroll
            for (int r = 0; r < 4; ++r) slab[(ib * 16 + kk * 4 + r) * HSP + jb * 16 + r16] = acc[i][r];
        }
    }
}

// Phase 1 with split-bf16 products: the same partial scores on v_mfma_f32_16x16x32_bf16.  The staged
// q / k tiles are split once into bf16 hi / lo images [row][64 tokens] (row pitch 144 B: an odd multiple of 16 B, so the 16
// rows of a fragment read hit 16 distinct bank groups); a fragment is one ds_read_b128 (8 consecutive tokens of a row), a
// 16 x 16 score tile takes 3 MFMAs per 32 tokens instead of 8 f32 ones at twice the cycles.
constexpr int SX_PITCH = ATT_TC * 2 + 16;          // bytes per LDS row

template <typename P, int NB>
__global__ __launch_bounds__(256) void attn_scores_x3_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                              float* __restrict__ slabs, int hs, int T, int chunk) {
    constexpr int HSP = NB * 16, NT = NB * NB, TPW = (NT + 3) / 4;
    constexpr int NQ = (HSP * (ATT_TC / 4) + 255) / 256;
    // (dynamic: 4 HSP SX_PITCH bytes - 64.5 KB at HSP = 112, the 102-wide heads of the 7-frame window, past the static limit)
    extern __shared__ __attribute__((aligned(16))) unsigned char sxs[];
    unsigned char *qh = sxs, *ql = sxs + HSP * SX_PITCH, *kh = sxs + 2 * HSP * SX_PITCH, *kl_ = sxs + 3 * HSP * SX_PITCH;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int bh = blockIdx.x, s = blockIdx.y;
    const float* qb = q + (size_t)bh * hs * T;
    const float* kb = k + (size_t)bh * hs * T;
    const int t_begin = s * chunk, t_end = min(T, t_begin + chunk);
    otp_f32x4 acc[TPW];
#pragma unroll
    for (int i = 0; i < TPW; ++i) acc[i] = (otp_f32x4){0.f, 0.f, 0.f, 0.f};
    const int r16 = lane & 15, kk = lane >> 4;
    const bool vec = (T & 3) == 0 && ((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(k)) & 15) == 0;
    otp_f32x4 pq[NQ], pk[NQ];
    auto load_tile = [&](int t0) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < NQ; ++j) {
            const int idx = tid + j * 256;
            const int row = idx / (ATT_TC / 4), t = t0 + 4 * (idx - row * (ATT_TC / 4));
            otp_f32x4 a = {0.f, 0.f, 0.f, 0.f}, b = {0.f, 0.f, 0.f, 0.f};
            if (row < hs && idx < HSP * (ATT_TC / 4)) {
                const float* qp = qb + (size_t)row * T + t;
                const float* kp = kb + (size_t)row * T + t;
                if (vec && t + 3 < t_end) {
                    a = *reinterpret_cast<const otp_f32x4*>(qp);
                    b = *reinterpret_cast<const otp_f32x4*>(kp);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (t + e < t_end) { a[e] = qp[e]; b[e] = kp[e]; }
                }
            }
            pq[j] = a;
            pk[j] = b;
        }
    };
    auto store_tile = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < NQ; ++j) {
            const int idx = tid + j * 256;
            if (idx < HSP * (ATT_TC / 4)) {
                const int row = idx / (ATT_TC / 4), tt = 4 * (idx - row * (ATT_TC / 4));
                unsigned long long h, l;
                otp_x3_split4<P>(pq[j], h, l);
                *reinterpret_cast<unsigned long long*>(qh + row * SX_PITCH + tt * 2) = h;
                *reinterpret_cast<unsigned long long*>(ql + row * SX_PITCH + tt * 2) = l;
                otp_x3_split4<P>(pk[j], h, l);
                *reinterpret_cast<unsigned long long*>(kh + row * SX_PITCH + tt * 2) = h;
                *reinterpret_cast<unsigned long long*>(kl_ + row * SX_PITCH + tt * 2) = l;
            }
        }
    };
    load_tile(t_begin);
    for (int t0 = t_begin; t0 < t_end; t0 += ATT_TC) {
        __syncthreads();                                       // previous tile fully read
        store_tile();
        __syncthreads();
        if (t0 + ATT_TC < t_end) load_tile(t0 + ATT_TC);
#pragma unroll
        for (int i = 0; i < TPW; ++i) {
            const int tile = wave + 4 * i;
            if (tile < NT) {
                const int ib = tile / NB, jb = tile - ib * NB;
                const int qo = (ib * 16 + r16) * SX_PITCH + kk * 16, ko = (jb * 16 + r16) * SX_PITCH + kk * 16;
#pragma unroll
                for (int ks = 0; ks < ATT_TC / 32; ++ks) {
                    const typename P::x8 a_h = *reinterpret_cast<const typename P::x8*>(qh + qo + ks * 64);
                    const typename P::x8 a_l = *reinterpret_cast<const typename P::x8*>(ql + qo + ks * 64);
                    const typename P::x8 b_h = *reinterpret_cast<const typename P::x8*>(kh + ko + ks * 64);
                    const typename P::x8 b_l = *reinterpret_cast<const typename P::x8*>(kl_ + ko + ks * 64);
                    acc[i] = P::mfma(a_l, b_h, acc[i]);
                    acc[i] = P::mfma(a_h, b_l, acc[i]);
                    acc[i] = P::mfma(a_h, b_h, acc[i]);
                }
            }
        }
    }
    float* slab = slabs + ((size_t)bh * gridDim.y + s) * HSP * HSP;
#pragma unroll
    for (int i = 0; i < TPW; ++i) {
        const int tile = wave + 4 * i;
        if (tile < NT) {
            const int ib = tile / NB, jb = tile - ib * NB;
#pragma unroll
            for (int r = 0; r < 4; ++r) slab[(ib * 16 + kk * 4 + r) * HSP + jb * 16 + r16] = acc[i][r];
        }
    }
}

// Phase 2: sum the slabs, scale, row softmax (one wave per row, shuffles for max / sum).
// P (B*nh, HSP, HSP) with zero padding columns.  grid (B*nh, ceil(HSP / 4)): every wave of the chip gets a row
// (a grid of B*nh workgroups alone left 7/8 of the CUs idle for 120 us).
// A body with a DROP flag under two __global__ wrappers: with DROP (attention-probability dropout, csrc/common.h: otp_attn_drop, the
// matrix is entry (g = bh, i = row, j = col) of (B nh, hs, hs)) PM receives m P for the apply step and P stays the undropped matrix.
template <bool DROP>
__device__ __forceinline__ void attn_softmax_body(const float* __restrict__ slabs, float* __restrict__ P, float* __restrict__ PM,
                                                  int hs, int HSP, int NS, float scale, const otp_attn_drop& drop) {
    const int bh = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row = blockIdx.y * 4 + wave;
    if (row >= HSP) return;
    const float* sb = slabs + (size_t)bh * NS * HSP * HSP;
    float* pb = P + (size_t)bh * HSP * HSP;
    float v[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int col = lane + 64 * h;
        // the NS partial slabs: independent loads, eight in flight (one after the other they were a 40 us latency chain);
        // a masked lane re-reads element 0 of its slab, same summation order as before for the live ones
        const bool live = row < hs && col < hs;
        const float* sp = sb + (live ? (size_t)row * HSP + col : 0);
        float a = 0.f;
        int s = 0;
        for (; s + 8 <= NS; s += 8) {
            float t[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) t[j] = sp[(size_t)(s + j) * HSP * HSP];
#pragma unroll
            for (int j = 0; j < 8; ++j) a += t[j];
        }
        for (; s < NS; ++s) a += sp[(size_t)s * HSP * HSP];
        v[h] = live ? a * scale : -INFINITY;
    }
    const float m = wave_max(fmaxf(v[0], v[1]));
    float e0 = (row < hs && lane < hs) ? expf(v[0] - m) : 0.f;
    float e1 = (row < hs && lane + 64 < hs) ? expf(v[1] - m) : 0.f;
    const float den = wave_sum(e0 + e1);
    const float p0 = row < hs ? e0 / den : 0.f, p1 = row < hs ? e1 / den : 0.f;
    if (lane < HSP) pb[row * HSP + lane] = p0;
    if (lane + 64 < HSP) pb[row * HSP + lane + 64] = p1;
    if (DROP) {
        float* mb = PM + (size_t)bh * HSP * HSP;
        const uint64_t rp = otp_attn_drop_row((uint64_t)bh * hs + row, hs);
        if (lane < HSP) mb[row * HSP + lane] = p0 * otp_attn_drop_at(drop, rp, lane);
        if (lane + 64 < HSP) mb[row * HSP + lane + 64] = p1 * otp_attn_drop_at(drop, rp, lane + 64);
    }
}
__global__ __launch_bounds__(256) void attn_softmax_kernel(const float* __restrict__ slabs, float* __restrict__ P,
                                                            int hs, int HSP, int NS, float scale) {
    attn_softmax_body<false>(slabs, P, nullptr, hs, HSP, NS, scale, otp_attn_drop{});
}
__global__ __launch_bounds__(256) void attn_softmax_drop_kernel(const float* __restrict__ slabs, float* __restrict__ P,
                                                                 float* __restrict__ PM, int hs, int HSP, int NS, float scale,
                                                                 otp_attn_drop drop) {
    attn_softmax_body<true>(slabs, P, PM, hs, HSP, NS, scale, drop);
}

// Phase 3: O^T[t, i] = sum_j v[j, t] P[i, j], stored as out[bh][t][i] (i contiguous) - exactly the memory
// image of `out.transpose(2,3).contiguous()` (blocks.py:447).  grid (B*nh, ceil(T / 256)); each wave owns
// 64 time steps (4 row blocks) x all NB column blocks.  A = v^T from an LDS tile, B = P^T from LDS.
// time steps per workgroup: 256, 128 once HSP > 96 (the v tile must fit in LDS)
constexpr int pv_tt(int nb) { return nb > 6 ? 128 : 256; }
template <int NB>
__global__ __launch_bounds__(256) void attn_pv_kernel(const float* __restrict__ v, const float* __restrict__ P,
                                                       float* __restrict__ out, int hs, int T) {
    constexpr int HSP = NB * 16, TT = pv_tt(NB), TB = TT / 64;   // TB 16-row time blocks per wave
    constexpr int PS = HSP + 2;       // P row pitch: (i*2 + k) distinct banks
    constexpr int VS = TT + 16;    // v row pitch == 16 (mod 32)
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* pl = smem;                 // [HSP][PS]
    float* vl = smem + HSP * PS;      // [HSP][VS]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int bh = blockIdx.x, t0 = blockIdx.y * TT;
    const float* vb = v + (size_t)bh * hs * T;
    const float* pb = P + (size_t)bh * HSP * HSP;
    // 16-byte vector loads, all issued before the first LDS write (one memory round trip for the whole tile)
    {
        constexpr int NP4 = (HSP * HSP / 4 + 255) / 256, NV4 = (HSP * (TT / 4) + 255) / 256;
        const bool vecv = (T & 3) == 0 && (reinterpret_cast<uintptr_t>(v) & 15) == 0;
        otp_f32x4 rp[NP4], rv[NV4];
#pragma unroll
        for (int j = 0; j < NP4; ++j) {
            const int idx = tid + j * 256;
            rp[j] = idx < HSP * HSP / 4 ? reinterpret_cast<const otp_f32x4*>(pb)[idx] : (otp_f32x4){0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int j = 0; j < NV4; ++j) {
            const int idx = tid + j * 256;
            const int row = idx / (TT / 4), t = t0 + 4 * (idx - row * (TT / 4));
            otp_f32x4 a = {0.f, 0.f, 0.f, 0.f};
            if (row < hs && idx < HSP * (TT / 4)) {
                const float* vp = vb + (size_t)row * T + t;
                if (vecv && t + 3 < T) {
                    a = *reinterpret_cast<const otp_f32x4*>(vp);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (t + e < T) a[e] = vp[e];
                }
            }
            rv[j] = a;
        }
#pragma unroll
        for (int j = 0; j < NP4; ++j) {
            const int idx = tid + j * 256;
            if (idx < HSP * HSP / 4) {
                const int i = (4 * idx) / HSP, jj = 4 * idx - i * HSP;    // HSP % 4 == 0: a float4 stays in one row
#pragma unroll
                for (int e = 0; e < 4; ++e) pl[i * PS + jj + e] = rp[j][e];
            }
        }
#pragma unroll
        for (int j = 0; j < NV4; ++j) {
            const int idx = tid + j * 256;
            if (idx < HSP * (TT / 4)) {
                const int row = idx / (TT / 4), tt = 4 * (idx - row * (TT / 4));
                *reinterpret_cast<otp_f32x4*>(vl + row * VS + tt) = rv[j];
            }
        }
    }
    __syncthreads();
    const int r16 = lane & 15, kk = lane >> 4;
    otp_f32x4 acc[TB][NB];
#pragma unroll
    for (int tb = 0; tb < TB; ++tb)
#pragma unroll
        for (int ib = 0; ib < NB; ++ib) acc[tb][ib] = (otp_f32x4){0.f, 0.f, 0.f, 0.f};
    const float* va = vl + kk * VS + wave * (TT / 4) + r16;          // A[t][j]: lane (t = r16, k = kk)
    const float* pa = pl + r16 * PS + kk;                      // B[j][i]: lane (k = kk, i = r16)
    for (int j0 = 0; j0 < HSP; j0 += 4) {
        float a[TB], b[NB];
#pragma unroll
        for (int tb = 0; tb < TB; ++tb) a[tb] = va[j0 * VS + tb * 16];
#pragma unroll
        for (int ib = 0; ib < NB; ++ib) b[ib] = pa[ib * 16 * PS + j0];
#pragma unroll
        for (int tb = 0; tb < TB; ++tb)
#pragma unroll
            for (int ib = 0; ib < NB; ++ib)
                acc[tb][ib] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[tb], b[ib], acc[tb][ib], 0, 0, 0);
    }
    float* ob = out + (size_t)bh * T * hs;
#pragma unroll
    for (int tb = 0; tb < TB; ++tb)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int t = t0 + wave * (TT / 4) + tb * 16 + kk * 4 + r;
            if (t < T) {
#pragma unroll
                for (int ib = 0; ib < NB; ++ib) {
                    const int i = ib * 16 + r16;
                    if (i < hs) ob[(size_t)t * hs + i] = acc[tb][ib][r];
                }
            }
        }
}

// Phase 3 with split-bf16 products: O^T[t, i] = sum_j v[j, t] P[i, j] on v_mfma_f32_16x16x32_bf16 (M = 256 tokens per
// workgroup, N = i, K = j).  Both operands want 8 consecutive j per lane: P rows have them; the v tile is transposed while it
// is staged (a thread loads 8 rows j x 4 tokens and writes four per-token records of 8 j each, hi and lo), like the window
// staging of csrc/convx.hip.  Records: [HSP j hi | HSP j lo | 16 B pad] (an odd multiple of 16 bytes).
// Eight waves own 256 tokens and ONE workgroup owns its CU: the launch asks for PVX_LDS bytes of LDS whatever the records need.
// Sharing a CU with a workgroup of this kernel changed results of the LDS-DMA fed projection kernel (csrc/densex.hip: one
// accumulator row of one 16-token tile, a few times per launch, only while the two temporal encoders ran side by side - found
// as replay-to-replay differences of the batch-16 forward, tools/dbg notes in DESIGN.md section 4); with the CU to itself
// neither kernel's results depend on what else is running.
// PVX_WAVES: 8 up to HSP = 80; 4 for the 96 / 112-wide heads of the 7-frame window (the records of 256 tokens would not fit)
constexpr size_t PVX_LDS = 138 * 1024;
constexpr int pvx_waves(int NB) { return NB <= 5 ? 8 : 4; }
constexpr size_t pvx_lds(int NB) {
    return NB <= 5 ? PVX_LDS : (size_t)(32 * pvx_waves(NB) + NB * 16) * (NB * 16 * 4 + 16) + 16;
}
template <typename P, int NB>
__global__ __launch_bounds__(64 * pvx_waves(NB), 2) void attn_pv_x3_kernel(const float* __restrict__ v, const float* __restrict__ M,
                                                                      float* __restrict__ out, int hs, int T, unsigned* rflag) {
    constexpr int PVX_WAVES = pvx_waves(NB), PVX_TH = 64 * PVX_WAVES, PVX_TT = 32 * PVX_WAVES;
    constexpr int HSP = NB * 16, KS = (HSP + 31) / 32, G = HSP / 8;
    constexpr int REC = HSP * 4 + 16;                              // bytes of a token (v) / row (P) record
    constexpr int NVI = (G * (PVX_TT / 4) + PVX_TH - 1) / PVX_TH;            // v items (8 rows x 4 tokens) per thread
    constexpr int NP4 = (HSP * HSP / 4 + PVX_TH - 1) / PVX_TH;
    extern __shared__ __attribute__((aligned(16))) unsigned char pvs[];
    unsigned char* vrec = pvs;                                     // [PVX_TT][REC]
    unsigned char* prec = pvs + PVX_TT * REC;                      // [HSP][REC]
    unsigned char* zrec = prec + HSP * REC;                        // 16 zero bytes
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int bh = blockIdx.x, t0 = blockIdx.y * PVX_TT;
    const float* vb = v + (size_t)bh * hs * T;
    const float* pb = M + (size_t)bh * HSP * HSP;
    if (tid < 4) reinterpret_cast<uint32_t*>(zrec)[tid] = 0u;
    // M (HSP x HSP fp32, zero padded) -> rows of hi / lo pieces
    {
        otp_f32x4 rp[NP4];
#pragma unroll
        for (int j = 0; j < NP4; ++j) {
            const int idx = tid + j * PVX_TH;
            rp[j] = idx < HSP * HSP / 4 ? reinterpret_cast<const otp_f32x4*>(pb)[idx] : (otp_f32x4){0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int j = 0; j < NP4; ++j) {
            const int idx = tid + j * PVX_TH;
            if (idx < HSP * HSP / 4) {
                const int i = (4 * idx) / HSP, jj = 4 * idx - i * HSP;
                unsigned long long h, l;
                otp_x3_split4<P>(rp[j], h, l);
                *reinterpret_cast<unsigned long long*>(prec + i * REC + jj * 2) = h;
                *reinterpret_cast<unsigned long long*>(prec + i * REC + HSP * 2 + jj * 2) = l;
            }
        }
    }
    // v tile, transposed: item = (8-row group g, 4 tokens)
    const bool vecv = (T & 3) == 0 && (reinterpret_cast<uintptr_t>(v) & 15) == 0;
#pragma unroll
    for (int it = 0; it < NVI; ++it) {
        const int idx = tid + it * PVX_TH;
        const int g = idx / (PVX_TT / 4), f4 = idx - g * (PVX_TT / 4);
        const int t = t0 + 4 * f4;
        otp_f32x4 x[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int row = 8 * g + e;
            otp_f32x4 a = {0.f, 0.f, 0.f, 0.f};
            if (idx < G * (PVX_TT / 4) && row < hs) {
                const float* vp = vb + (size_t)row * T + t;
                if (vecv && t + 3 < T) {
                    a = *reinterpret_cast<const otp_f32x4*>(vp);
                } else {
#pragma unroll
                    for (int c = 0; c < 4; ++c)
                        if (t + c < T) a[c] = vp[c];
                }
            }
            x[e] = a;
        }
        if (idx < G * (PVX_TT / 4)) {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                unsigned long long h0, l0, h1, l1;
                otp_x3_split4<P>((otp_f32x4){x[0][c], x[1][c], x[2][c], x[3][c]}, h0, l0);
                otp_x3_split4<P>((otp_f32x4){x[4][c], x[5][c], x[6][c], x[7][c]}, h1, l1);
                unsigned char* r = vrec + (4 * f4 + c) * REC + g * 16;
                *reinterpret_cast<unsigned long long*>(r) = h0;
                *reinterpret_cast<unsigned long long*>(r + 8) = h1;
                *reinterpret_cast<unsigned long long*>(r + HSP * 2) = l0;
                *reinterpret_cast<unsigned long long*>(r + HSP * 2 + 8) = l1;
            }
        }
    }
    __syncthreads();
    const int r16 = lane & 15, kk = lane >> 4;
    otp_f32x4 acc[2][NB];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < NB; ++nt) acc[mt][nt] = (otp_f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        const int kg = 4 * ks + kk;                                // 8-wide j group of this lane
        const bool kv = kg < G;
        typename P::x8 ah[2], al[2];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            const unsigned char* a = kv ? vrec + ((wave * 2 + mt) * 16 + r16) * REC + kg * 16 : zrec;
            ah[mt] = *reinterpret_cast<const typename P::x8*>(a);
            al[mt] = *reinterpret_cast<const typename P::x8*>(kv ? a + HSP * 2 : zrec);
        }
#pragma unroll
        for (int nt = 0; nt < NB; ++nt) {
            const unsigned char* b = kv ? prec + (nt * 16 + r16) * REC + kg * 16 : zrec;
            const typename P::x8 b_h = *reinterpret_cast<const typename P::x8*>(b);
            const typename P::x8 b_l = *reinterpret_cast<const typename P::x8*>(kv ? b + HSP * 2 : zrec);
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) {
                acc[mt][nt] = P::mfma(al[mt], b_h, acc[mt][nt]);
                acc[mt][nt] = P::mfma(ah[mt], b_l, acc[mt][nt]);
                acc[mt][nt] = P::mfma(ah[mt], b_h, acc[mt][nt]);
            }
        }
    }
    {   // range guard (common.h): q, k or v beyond the pieces' range has made these sums NaN (through the scores and the softmax)
        bool bad = false;
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int nt = 0; nt < NB; ++nt)
#pragma unroll
                for (int r = 0; r < 4; ++r) bad |= otp_out_of_range<P>(acc[mt][nt][r]);
        otp_range_report(rflag, bad, OTP_RANGE_ATTN);
    }
    float* ob = out + (size_t)bh * T * hs;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int t = t0 + (wave * 2 + mt) * 16 + kk * 4 + r;
            if (t < T) {
#pragma unroll
                for (int nt = 0; nt < NB; ++nt) {
                    const int i = nt * 16 + r16;
                    if (i < hs) ob[(size_t)t * hs + i] = acc[mt][nt][r];
                }
            }
        }
}

// ---- attention backward helpers ------------------------------------------------------------------------
// per (b, head): in (R, Cc) row-major -> out (Cc, R) row-major, scaled (the O <-> out.transpose(2,3).contiguous() image)
__global__ void transpose_scale_kernel(const float* __restrict__ in, float* __restrict__ out, int R, int Cc, float scale) {
    __shared__ float tile[32][33];
    const float* ib = in + (size_t)blockIdx.z * R * Cc;
    float* ob = out + (size_t)blockIdx.z * R * Cc;
    const int r0 = blockIdx.y * 32, c0 = blockIdx.x * 32;
    for (int j = threadIdx.y; j < 32; j += 8) {
        const int r = r0 + j, c = c0 + threadIdx.x;
        tile[j][threadIdx.x] = (r < R && c < Cc) ? ib[(size_t)r * Cc + c] : 0.f;
    }
    __syncthreads();
    for (int j = threadIdx.y; j < 32; j += 8) {
        const int c = c0 + j, r = r0 + threadIdx.x;
        if (c < Cc && r < R) ob[(size_t)c * R + r] = tile[threadIdx.x][j] * scale;
    }
}

// dP = sum of the NS score slabs (padded HSP x HSP); dS = P o (dP - rowsum(dP o P)); also writes dS^T and P^T.
// With DROP (attention-probability dropout, csrc/common.h: otp_attn_drop, entry (g = bh, i = row, j = col) of (B nh, hs, hs)): dP is
// multiplied by the mask m first and PT receives (m P)^T, the matrix dv is formed with.
template <bool DROP>
__device__ __forceinline__ void softmax_bwd_body(const float* __restrict__ slabs, const float* __restrict__ P,
                                                 float* __restrict__ dS, float* __restrict__ dST,
                                                 float* __restrict__ PT, int hs, int HSP, int NS, const otp_attn_drop& drop) {
    const int bh = blockIdx.x, row = blockIdx.y, lane = threadIdx.x;
    const float* sb = slabs + (size_t)bh * NS * HSP * HSP;
    const float* pb = P + (size_t)bh * HSP * HSP;
    float dp[2], pv[2], mf[2], acc = 0.f;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int col = lane + 64 * h;
        dp[h] = 0.f;
        pv[h] = 0.f;
        mf[h] = 1.f;
        if (row < hs && col < hs) {
            for (int s = 0; s < NS; ++s) dp[h] += sb[((size_t)s * HSP + row) * HSP + col];
            pv[h] = pb[row * HSP + col];
            if (DROP) {
                mf[h] = otp_attn_drop_at(drop, otp_attn_drop_row((uint64_t)bh * hs + row, hs), col);
                dp[h] *= mf[h];
            }
        }
        acc += dp[h] * pv[h];
    }
    acc = wave_sum(acc);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int col = lane + 64 * h;
        if (col < HSP) {
            const float v = (row < hs && col < hs) ? pv[h] * (dp[h] - acc) : 0.f;
            dS[((size_t)bh * HSP + row) * HSP + col] = v;
            dST[((size_t)bh * HSP + col) * HSP + row] = v;
            PT[((size_t)bh * HSP + col) * HSP + row] = (row < hs && col < hs) ? (DROP ? pv[h] * mf[h] : pv[h]) : 0.f;
        }
    }
}
__global__ __launch_bounds__(64) void softmax_bwd_kernel(const float* __restrict__ slabs, const float* __restrict__ P,
                                                          float* __restrict__ dS, float* __restrict__ dST,
                                                          float* __restrict__ PT, int hs, int HSP, int NS) {
    softmax_bwd_body<false>(slabs, P, dS, dST, PT, hs, HSP, NS, otp_attn_drop{});
}
__global__ __launch_bounds__(64) void softmax_bwd_drop_kernel(const float* __restrict__ slabs, const float* __restrict__ P,
                                                               float* __restrict__ dS, float* __restrict__ dST,
                                                               float* __restrict__ PT, int hs, int HSP, int NS, otp_attn_drop drop) {
    softmax_bwd_body<true>(slabs, P, dS, dST, PT, hs, HSP, NS, drop);
}

// ---- host code ---------------------------------------------------------------------------------------------------------
// 1: the attention products as split products (default), 0: f32 MFMA (otp_chan_attn_set_split)
std::atomic<int> g_attn_split{1};

int attn_splits(int BH, int T) {
    int ns = 1;
    while (BH * ns < 768 && T / (ns * 2) >= 2 * ATT_TC) ns *= 2;
    return ns;
}

// f(std::integral_constant<int, NB>) for the NB = ceil(hs / 16) <= 7 of a head; the callers have checked the bound
template <typename F>
void with_nb(int hs, F f) {
    switch ((hs + 15) / 16) {
        case 1: f(std::integral_constant<int, 1>{}); break;
        case 2: f(std::integral_constant<int, 2>{}); break;
        case 3: f(std::integral_constant<int, 3>{}); break;
        case 4: f(std::integral_constant<int, 4>{}); break;
        case 5: f(std::integral_constant<int, 5>{}); break;
        case 6: f(std::integral_constant<int, 6>{}); break;
        default: f(std::integral_constant<int, 7>{}); break;
    }
}

// slabs[bh][s] = partial a . b^T over the s-th of NS slices of T (chunk steps each): split products on pieces P, or the f32 kernel.
// (OTP_ALLOW_BIG_LDS in a body instantiated per P and NB: one flag per kernel instantiation)
template <typename P>
void launch_scores(const float* a, const float* b, float* slabs, int BH, int hs, int T, int NS, int chunk, hipStream_t st) {
    const bool split = g_attn_split.load(std::memory_order_relaxed);
    with_nb(hs, [&](auto nb) {
        constexpr int NB = decltype(nb)::value;
        if (split) {
            auto kern = attn_scores_x3_kernel<P, NB>;
            const size_t lds = (size_t)4 * NB * 16 * SX_PITCH;
            OTP_ALLOW_BIG_LDS(kern, lds);
            hipLaunchKernelGGL(kern, dim3(BH, NS), dim3(256), lds, st, a, b, slabs, hs, T, chunk);
        } else {
            hipLaunchKernelGGL(attn_scores_kernel<NB>, dim3(BH, NS), dim3(256), 0, st, a, b, slabs, hs, T, chunk);
        }
    });
}

// the f32 kernel of launch_apply: independent of the piece type, so its LDS flag is one per NB
template <int NB>
void launch_pv_f32(const float* v, const float* M, float* out, int BH, int hs, int T, hipStream_t st) {
    constexpr int HSP = NB * 16, TT = pv_tt(NB);
    const size_t lds = ((size_t)HSP * (HSP + 2) + (size_t)HSP * (TT + 16)) * sizeof(float);
    auto kern = attn_pv_kernel<NB>;
    OTP_ALLOW_BIG_LDS(kern, lds);
    hipLaunchKernelGGL(kern, dim3(BH, otp_ceil_div(T, TT)), dim3(256), lds, st, v, M, out, hs, T);
}

// out[bh][t][i] = sum_j M[bh][i][j] * v[bh][j][t]: split products on pieces P, or the f32 kernel
template <typename P>
void launch_apply(const float* v, const float* M, float* out, int BH, int hs, int T, hipStream_t st) {
    const bool split = g_attn_split.load(std::memory_order_relaxed);
    with_nb(hs, [&](auto nb) {
        constexpr int NB = decltype(nb)::value;
        if (split) {
            auto kern = attn_pv_x3_kernel<P, NB>;
            const size_t lds = pvx_lds(NB);                        // >= (tokens + HSP) * (HSP * 4 + 16) + 16
            OTP_ALLOW_BIG_LDS(kern, lds);
            hipLaunchKernelGGL(kern, dim3(BH, otp_ceil_div(T, 32 * pvx_waves(NB))), dim3(64 * pvx_waves(NB)), lds, st, v, M, out, hs,
                               T, otp_range_word());
        } else {
            launch_pv_f32<NB>(v, M, out, BH, hs, T, st);
        }
    });
}

template <typename P>
int scores_entry(const void* a, const void* b, void* slabs, int BH, int hs, int T, void* stream) {
    if (!a || !b || !slabs || BH <= 0 || hs <= 0 || T <= 0) return OTP_ERR_BAD_ARG;
    if (hs > 7 * 16) return OTP_ERR_UNSUPPORTED;
    const int NS = attn_splits(BH, T);
    const int chunk = otp_ceil_div(otp_ceil_div(T, NS), ATT_TC) * ATT_TC;
    launch_scores<P>(static_cast<const float*>(a), static_cast<const float*>(b), static_cast<float*>(slabs), BH, hs, T, NS, chunk,
                     static_cast<hipStream_t>(stream));
    return otp_launch_status();
}

template <typename P>
int apply_entry(const void* v, const void* M, void* out, int BH, int hs, int T, void* stream) {
    if (!v || !M || !out || BH <= 0 || hs <= 0 || T <= 0) return OTP_ERR_BAD_ARG;
    if (hs > 7 * 16) return OTP_ERR_UNSUPPORTED;
    launch_apply<P>(static_cast<const float*>(v), static_cast<const float*>(M), static_cast<float*>(out), BH, hs, T,
                    static_cast<hipStream_t>(stream));
    return otp_launch_status();
}

// The forward's workspace, the one statement of its layout: three regions of floats,
//   slabs (BH NS matrices) | P (BH matrices) | m P (BH matrices, with_mask only),   a matrix = HSP x HSP floats, zero padded.
// Both size queries and the forward read it from here; outside C only ChanAttnFunction.forward (otpose_amd/train_ops.py)
// knows it, where it copies P out of the workspace.  (B, C, T, n_head) positive and C % n_head == 0: the callers have checked.
struct attn_workspace {
    int hs, HSP, BH, NS;
    size_t slabs, P, mP;                   // float offsets of the regions (without a mask mP is the end of the workspace)
    size_t bytes;
};
attn_workspace attn_workspace_of(int B, int C, int T, int n_head, bool with_mask) {
    attn_workspace w;
    w.hs = C / n_head;
    w.HSP = (w.hs + 15) & ~15;
    w.BH = B * n_head;
    w.NS = attn_splits(w.BH, T);
    const size_t mat = (size_t)w.HSP * w.HSP;
    w.slabs = 0;
    w.P = (size_t)w.BH * w.NS * mat;
    w.mP = w.P + (size_t)w.BH * mat;
    w.bytes = (with_mask ? w.mP + (size_t)w.BH * mat : w.mP) * sizeof(float);
    return w;
}

size_t attn_workspace_bytes(int B, int C, int T, int n_head, bool with_mask) {
    if (B <= 0 || C <= 0 || T <= 0 || n_head <= 0 || C % n_head) return 0;
    return attn_workspace_of(B, C, T, n_head, with_mask).bytes;
}

// the forward of otp_chan_attn (drop == nullptr: P is applied) and otp_chan_attn_dropout (m P is written next to P and applied)
int chan_attn_forward(const void* q, const void* k, const void* v, void* out, void* workspace, size_t workspace_bytes, int B, int C,
                      int T, int n_head, float scale, const otp_attn_drop* drop, void* stream) {
    if (!q || !k || !v || !out || !workspace || B <= 0 || C <= 0 || T <= 0 || n_head <= 0) return OTP_ERR_BAD_ARG;
    if (C % n_head) return OTP_ERR_BAD_ARG;
    const attn_workspace w = attn_workspace_of(B, C, T, n_head, drop != nullptr);
    if (w.HSP > 7 * 16) return OTP_ERR_UNSUPPORTED;                      // hs <= 112
    if (workspace_bytes < w.bytes) return OTP_ERR_WORKSPACE;
    const int chunk = otp_ceil_div(otp_ceil_div(T, w.NS), ATT_TC) * ATT_TC;
    auto st = static_cast<hipStream_t>(stream);
    float* slabs = static_cast<float*>(workspace) + w.slabs;
    float* P = static_cast<float*>(workspace) + w.P;
    float* PM = static_cast<float*>(workspace) + w.mP;
    launch_scores<otp_half_pieces>(static_cast<const float*>(q), static_cast<const float*>(k), slabs, w.BH, w.hs, T, w.NS, chunk, st);
    if (drop)
        hipLaunchKernelGGL(attn_softmax_drop_kernel, dim3(w.BH, otp_ceil_div(w.HSP, 4)), dim3(256), 0, st, slabs, P, PM, w.hs, w.HSP,
                           w.NS, scale, *drop);
    else
        hipLaunchKernelGGL(attn_softmax_kernel, dim3(w.BH, otp_ceil_div(w.HSP, 4)), dim3(256), 0, st, slabs, P, w.hs, w.HSP, w.NS,
                           scale);
    launch_apply<otp_half_pieces>(static_cast<const float*>(v), drop ? PM : P, static_cast<float*>(out), w.BH, w.hs, T, st);
    return otp_launch_status();
}
}  // namespace

extern "C" size_t otp_chan_attn_workspace(int B, int C, int T, int n_head) { return attn_workspace_bytes(B, C, T, n_head, false); }

extern "C" int otp_chan_attn(const void* q, const void* k, const void* v, void* out, void* workspace,
                             size_t workspace_bytes, int B, int C, int T, int n_head, float scale, void* stream) {
    return chan_attn_forward(q, k, v, out, workspace, workspace_bytes, B, C, T, n_head, scale, nullptr, stream);
}

// the same with attention-probability dropout: the workspace holds one more matrix per (b, head), m P, behind P
extern "C" size_t otp_chan_attn_dropout_workspace(int B, int C, int T, int n_head) {
    return attn_workspace_bytes(B, C, T, n_head, true);
}

// a rate whose threshold is 0 keeps everything: the plain path, held to the plain workspace size
extern "C" int otp_chan_attn_dropout(const void* q, const void* k, const void* v, void* out, void* workspace, size_t workspace_bytes,
                                     int B, int C, int T, int n_head, float scale, float p, unsigned long long seed, void* stream) {
    if (!otp_attn_drop_rate_ok(p)) return OTP_ERR_BAD_ARG;
    const otp_attn_drop drop = otp_attn_drop_make(p, seed);
    return chan_attn_forward(q, k, v, out, workspace, workspace_bytes, B, C, T, n_head, scale, drop.thr ? &drop : nullptr, stream);
}

// ---- pieces of the channel attention exposed for its backward (otpose_amd/train_ops.py) -------------------------
// 1 (default): the attention products as split products on the 16-bit matrix cores; 0: the f32 MFMA kernels.  Process-wide.
extern "C" int otp_chan_attn_set_split(int on) {
    g_attn_split.store(on ? 1 : 0, std::memory_order_relaxed);
    return OTP_OK;
}

// number of T-splits / score slabs the kernels use for (BH, T)
extern "C" int otp_chan_attn_splits(int BH, int T) { return (BH > 0 && T > 0) ? attn_splits(BH, T) : 0; }

// slabs[bh][s] (HSP x HSP, zero padded) = partial a . b^T over the s-th slice of T, no scale: sum the slabs for a . b^T
extern "C" int otp_chan_attn_scores(const void* a, const void* b, void* slabs, int BH, int hs, int T, void* stream) {
    return scores_entry<otp_half_pieces>(a, b, slabs, BH, hs, T, stream);
}
extern "C" int otp_chan_attn_scores_bf16p(const void* a, const void* b, void* slabs, int BH, int hs, int T, void* stream) {
    return scores_entry<otp_bf16_pieces>(a, b, slabs, BH, hs, T, stream);
}

// out[bh][t][i] = sum_j M[bh][i][j] * v[bh][j][t]   (M: HSP x HSP zero padded; the transposed-contiguous output image)
extern "C" int otp_chan_attn_apply(const void* v, const void* M, void* out, int BH, int hs, int T, void* stream) {
    return apply_entry<otp_half_pieces>(v, M, out, BH, hs, T, stream);
}
extern "C" int otp_chan_attn_apply_bf16p(const void* v, const void* M, void* out, int BH, int hs, int T, void* stream) {
    return apply_entry<otp_bf16_pieces>(v, M, out, BH, hs, T, stream);
}

extern "C" int otp_transpose_scale(const void* in, void* out, int batches, int R, int Cc, float scale, void* stream) {
    if (!in || !out || batches <= 0 || R <= 0 || Cc <= 0) return OTP_ERR_BAD_ARG;
    hipLaunchKernelGGL(transpose_scale_kernel, dim3(otp_ceil_div(Cc, 32), otp_ceil_div(R, 32), batches), dim3(32, 8), 0,
                       static_cast<hipStream_t>(stream), static_cast<const float*>(in), static_cast<float*>(out), R, Cc, scale);
    return otp_launch_status();
}

extern "C" int otp_softmax_backward(const void* slabs, const void* P, void* dS, void* dST, void* PT, int BH, int hs, int NS,
                                    void* stream) {
    if (!slabs || !P || !dS || !dST || !PT || BH <= 0 || hs <= 0 || NS <= 0) return OTP_ERR_BAD_ARG;
    const int HSP = (hs + 15) & ~15;
    if (HSP > 128) return OTP_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(softmax_bwd_kernel, dim3(BH, HSP), dim3(64), 0, static_cast<hipStream_t>(stream),
                       static_cast<const float*>(slabs), static_cast<const float*>(P), static_cast<float*>(dS),
                       static_cast<float*>(dST), static_cast<float*>(PT), hs, HSP, NS);
    return otp_launch_status();
}

extern "C" int otp_softmax_backward_dropout(const void* slabs, const void* P, void* dS, void* dST, void* PT, int BH, int hs, int NS,
                                            float p, unsigned long long seed, void* stream) {
    if (!slabs || !P || !dS || !dST || !PT || BH <= 0 || hs <= 0 || NS <= 0 || !otp_attn_drop_rate_ok(p)) return OTP_ERR_BAD_ARG;
    const otp_attn_drop drop = otp_attn_drop_make(p, seed);
    if (!drop.thr) return otp_softmax_backward(slabs, P, dS, dST, PT, BH, hs, NS, stream);
    const int HSP = (hs + 15) & ~15;
    if (HSP > 128) return OTP_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(softmax_bwd_drop_kernel, dim3(BH, HSP), dim3(64), 0, static_cast<hipStream_t>(stream),
                       static_cast<const float*>(slabs), static_cast<const float*>(P), static_cast<float*>(dS),
                       static_cast<float*>(dST), static_cast<float*>(PT), hs, HSP, NS, drop);
    return otp_launch_status();
}
