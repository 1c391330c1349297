// Temporal segment NMS (the reference's thirdparty/utils: nms_1d_cpu and the Python layer of nms.py) on a segmented batch:
// G groups, one per (video, class) pair, given by offsets (G+1) over flat segs (N, 2) and scores (N).  One workgroup per
// group, every group in one launch, no host round trip.
//   otp_seg_nms       hard NMS (nms_cpu.cpp:19-58) with NMSop's score pre-filter and max_num cut
//   otp_seg_softnms   soft NMS (nms_cpu.cpp:67-160): hard / linear / gaussian decay, arg-max selection per round
//   otp_seg_voting    seg_voting (nms.py:67-101): score-weighted mean of the group's segments around each kept segment
// A group of up to OTP_SEG_NMS_LDS_CAP segments works in LDS, a larger one in its rows of a global workspace (the code is
// the same, instantiated for both).  The arithmetic is the contract written out in include/otpose_hip.h.  Plain C++: no
// inline assembly, no float atomics, every sum in a fixed order - the same input gives the same bytes.  DESIGN.md section 3.13.
#include "common.h"

// every product, quotient and sum rounded on its own, as the reference's scalar float32 loops are (tests/segnms_ref.py)
#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kCap = OTP_SEG_NMS_LDS_CAP;
constexpr int kWsWords = OTP_SEG_NMS_WS_WORDS;       // workspace words per segment (both kernels)

// a NaN score orders as -inf: the order stays total
__device__ __forceinline__ float order_key(float s) { return s == s ? s : -INFINITY; }

// [o0, o0 + n) of group g, or n = -1 for offsets that do not describe a range inside [0, N] (nothing of segs is then touched)
__device__ __forceinline__ int group_range(const int* __restrict__ offsets, int g, int N, int& o0) {
    o0 = offsets[g];
    const int o1 = offsets[g + 1];
    return (o0 < 0 || o1 < o0 || o1 > N) ? -1 : o1 - o0;
}

// ---- hard NMS --------------------------------------------------------------------------------------------------------------
// key (n): the order key of a segment that passes the pre-filter, NaN for one that does not.  sx1 / sx2 / sarea / sidx / alive
// (n): the candidates in descending-score order.
__device__ __forceinline__ void seg_nms_group(const float* __restrict__ segs, const float* __restrict__ scores, int n,
                                              float iou_threshold, float min_score, int max_num, float* key, float* sx1,
                                              float* sx2, float* sarea, int* sidx, int* alive, int* s_cnt, int* keep,
                                              int* count) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const bool filter = min_score > 0.f;              // NMSop: is_filtering_by_score
    int M = 0;
    for (int base = 0; base < n; base += kThreads) {
        const int e = base + t;
        bool valid = false;
        if (e < n) {
            const float s = scores[e];
            valid = !filter || s > min_score;
            key[e] = valid ? order_key(s) : NAN;
        }
        M += __syncthreads_count(valid);
    }
    __syncthreads();

    // rank by counting: descending score, equal scores by ascending index (the reference's sort leaves ties open)
    for (int e = t; e < n; e += kThreads) {
        const float s = key[e];
        if (s != s) continue;
        int rank = 0;
        for (int o = 0; o < n; ++o) {
            const float so = key[o];
            rank += (so > s || (so == s && o < e)) ? 1 : 0;
        }
        const float x1 = segs[2 * (size_t)e], x2 = segs[2 * (size_t)e + 1];
        sx1[rank] = x1;
        sx2[rank] = x2;
        sarea[rank] = (x2 - x1) + 1e-6f;
        sidx[rank] = e;
        alive[rank] = 1;
    }
    __syncthreads();

    // the reference's loop: the first live candidate is kept and suppresses every later live one with ovr >= iou_threshold
    int head = 0;
    for (;;) {
        while (head < M && !alive[head]) ++head;
        if (head >= M) break;
        __syncthreads();                              // every thread has found the head before anyone clears a flag
        const float ix1 = sx1[head], ix2 = sx2[head], iarea = sarea[head];
        for (int p = head + 1 + t; p < M; p += kThreads) {
            if (!alive[p]) continue;
            const float xx1 = fmaxf(ix1, sx1[p]), xx2 = fminf(ix2, sx2[p]);
            const float inter = fmaxf(0.f, xx2 - xx1);
            const float ovr = inter / (iarea + sarea[p] - inter);
            if (ovr >= iou_threshold) alive[p] = 0;
        }
        ++head;
        __syncthreads();                              // orders the alive[] stores before the next scan
    }

    // the kept candidates in order, cut at max_num; -1 behind them
    int kept = 0;
    for (int base = 0; base < M; base += kThreads) {
        const int p = base + t;
        const bool flag = p < M && alive[p];
        const unsigned long long mask = __ballot(flag);
        if (lane == 0) s_cnt[wave] = __popcll(mask);
        __syncthreads();
        int off = kept, total = 0;
        for (int w = 0; w < kWaves; ++w) {
            if (w < wave) off += s_cnt[w];
            total += s_cnt[w];
        }
        if (flag) keep[off + __popcll(mask & ((1ull << lane) - 1ull))] = sidx[p];
        kept += total;
        __syncthreads();
    }
    if (max_num > 0 && kept > max_num) kept = max_num;
    for (int e = kept + t; e < n; e += kThreads) keep[e] = -1;
    if (t == 0) *count = kept;
}

__global__ __launch_bounds__(kThreads) void seg_nms_kernel(const float* __restrict__ segs, const float* __restrict__ scores,
                                                           const int* __restrict__ offsets, int N, float iou_threshold,
                                                           float min_score, int max_num, int* __restrict__ ws,
                                                           int* __restrict__ counts, int* __restrict__ keep) {
    __shared__ int s_mem[kWsWords * kCap];
    __shared__ int s_cnt[kWaves];
    const int g = blockIdx.x;
    int o0;
    const int n = group_range(offsets, g, N, o0);
    if (n <= 0) {
        if (threadIdx.x == 0) counts[g] = 0;
        return;
    }
    const float* S = segs + 2 * (size_t)o0;
    if (n <= kCap) {
        seg_nms_group(S, scores + o0, n, iou_threshold, min_score, max_num, reinterpret_cast<float*>(s_mem),
                      reinterpret_cast<float*>(s_mem + kCap), reinterpret_cast<float*>(s_mem + 2 * kCap),
                      reinterpret_cast<float*>(s_mem + 3 * kCap), s_mem + 4 * kCap, s_mem + 5 * kCap, s_cnt, keep + o0,
                      counts + g);
    } else {                                          // plane j of the workspace holds N words; the group owns [o0, o0 + n) of each
        int* w = ws + o0;
        seg_nms_group(S, scores + o0, n, iou_threshold, min_score, max_num, reinterpret_cast<float*>(w),
                      reinterpret_cast<float*>(w + (size_t)N), reinterpret_cast<float*>(w + 2 * (size_t)N),
                      reinterpret_cast<float*>(w + 3 * (size_t)N), w + 4 * (size_t)N, w + 5 * (size_t)N, s_cnt, keep + o0,
                      counts + g);
    }
}

// ---- soft NMS --------------------------------------------------------------------------------------------------------------
// Segment e belongs to thread e % kThreads for the whole run: only its owner writes sc[e] and live[e].  One barrier per round;
// the cross-wave slots alternate between two sets, so a wave that is a round ahead does not overwrite what another still reads.
__device__ __forceinline__ void seg_softnms_group(const float* __restrict__ segs, const float* __restrict__ scores, int n,
                                                  float iou_threshold, float sigma, float min_score, int method, int max_num,
                                                  float* sc, float* x1, float* x2, float* area, int* live,
                                                  float (*s_key)[kWaves], int (*s_idx)[kWaves], float* dets, int* inds,
                                                  int* count) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    for (int e = t; e < n; e += kThreads) {
        const float a = segs[2 * (size_t)e], b = segs[2 * (size_t)e + 1];
        x1[e] = a;
        x2[e] = b;
        area[e] = (b - a) + 1e-6f;
        sc[e] = scores[e];
        live[e] = 1;
    }
    __syncthreads();
    const int rounds = (max_num > 0 && max_num < n) ? max_num : n;
    int r = 0;
    for (; r < rounds; ++r) {
        // the live arg-max: the highest score, of equal scores the lowest index (a thread walks its segments upwards)
        float bk = 0.f;
        int bi = -1;
        for (int e = t; e < n; e += kThreads) {
            if (!live[e]) continue;
            const float k = order_key(sc[e]);
            if (bi < 0 || k > bk) { bk = k; bi = e; }
        }
        for (int o = 32; o > 0; o >>= 1) {
            const float ok = __shfl_xor(bk, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (oi >= 0 && (bi < 0 || ok > bk || (ok == bk && oi < bi))) { bk = ok; bi = oi; }
        }
        if (lane == 0) { s_key[r & 1][wave] = bk; s_idx[r & 1][wave] = bi; }
        __syncthreads();
        bk = s_key[r & 1][0];
        bi = s_idx[r & 1][0];
        for (int w = 1; w < kWaves; ++w) {
            const float ok = s_key[r & 1][w];
            const int oi = s_idx[r & 1][w];
            if (oi >= 0 && (bi < 0 || ok > bk || (ok == bk && oi < bi))) { bk = ok; bi = oi; }
        }
        if (bi < 0) break;                            // nobody is left (uniform: every thread reads the same slots)
        const float ix1 = x1[bi], ix2 = x2[bi], iarea = area[bi];
        if (t == 0) {
            dets[3 * (size_t)r] = ix1;
            dets[3 * (size_t)r + 1] = ix2;
            dets[3 * (size_t)r + 2] = sc[bi];
            inds[r] = bi;
        }
        for (int e = t; e < n; e += kThreads) {
            if (!live[e]) continue;
            if (e == bi) { live[e] = 0; continue; }
            const float xx1 = fmaxf(ix1, x1[e]), xx2 = fminf(ix2, x2[e]);
            const float inter = fmaxf(0.f, xx2 - xx1);
            const float ovr = inter / (iarea + area[e] - inter);
            float weight = 1.f;
            if (method == 0) {
                if (ovr >= iou_threshold) weight = 0.f;
            } else if (method == 1) {
                if (ovr >= iou_threshold) weight = 1.f - ovr;
            } else {
                weight = expf(-(ovr * ovr) / sigma);
            }
            const float s = sc[e] * weight;
            sc[e] = s;
            if (s < min_score) live[e] = 0;
        }
    }
    __syncthreads();                                  // t == 0 has read the last taken score before the rows behind are cleared
    for (int e = r + t; e < n; e += kThreads) {
        dets[3 * (size_t)e] = 0.f;
        dets[3 * (size_t)e + 1] = 0.f;
        dets[3 * (size_t)e + 2] = 0.f;
        inds[e] = -1;
    }
    if (t == 0) *count = r;
}

__global__ __launch_bounds__(kThreads) void seg_softnms_kernel(const float* __restrict__ segs, const float* __restrict__ scores,
                                                               const int* __restrict__ offsets, int N, float iou_threshold,
                                                               float sigma, float min_score, int method, int max_num,
                                                               int* __restrict__ ws, int* __restrict__ counts,
                                                               float* __restrict__ dets, int* __restrict__ inds) {
    __shared__ int s_mem[5 * kCap];
    __shared__ float s_key[2][kWaves];
    __shared__ int s_idx[2][kWaves];
    const int g = blockIdx.x;
    int o0;
    const int n = group_range(offsets, g, N, o0);
    if (n <= 0) {
        if (threadIdx.x == 0) counts[g] = 0;
        return;
    }
    const float* S = segs + 2 * (size_t)o0;
    float* D = dets + 3 * (size_t)o0;
    if (n <= kCap) {
        seg_softnms_group(S, scores + o0, n, iou_threshold, sigma, min_score, method, max_num,
                          reinterpret_cast<float*>(s_mem), reinterpret_cast<float*>(s_mem + kCap),
                          reinterpret_cast<float*>(s_mem + 2 * kCap), reinterpret_cast<float*>(s_mem + 3 * kCap),
                          s_mem + 4 * kCap, s_key, s_idx, D, inds + o0, counts + g);
    } else {
        int* w = ws + o0;
        seg_softnms_group(S, scores + o0, n, iou_threshold, sigma, min_score, method, max_num, reinterpret_cast<float*>(w),
                          reinterpret_cast<float*>(w + (size_t)N), reinterpret_cast<float*>(w + 2 * (size_t)N),
                          reinterpret_cast<float*>(w + 3 * (size_t)N), w + 4 * (size_t)N, s_key, s_idx, D, inds + o0,
                          counts + g);
    }
}

// ---- voting ----------------------------------------------------------------------------------------------------------------
// One wave per kept segment: lane l adds the terms j = l, l + 64, ... in ascending order, a butterfly adds the 64 lanes.  Two
// passes, as the reference normalises the weights before the product: the sum of the weights, then sum((w / total) x).
__global__ __launch_bounds__(kThreads) void seg_voting_kernel(const float* __restrict__ nms_segs,
                                                              const int* __restrict__ nms_offsets,
                                                              const float* __restrict__ segs, const float* __restrict__ scores,
                                                              const int* __restrict__ offsets, int K, int N,
                                                              float voting_thresh, float* __restrict__ out) {
    const int g = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int o0, k0;
    const int n = group_range(offsets, g, N, o0);
    const int kn = group_range(nms_offsets, g, K, k0);
    if (n < 0 || kn <= 0) return;
    const float* S = segs + 2 * (size_t)o0;
    const float* W = scores + o0;
    for (int k = wave; k < kn; k += kWaves) {
        const float a1 = nms_segs[2 * (size_t)(k0 + k)], a2 = nms_segs[2 * (size_t)(k0 + k) + 1];
        const float alen = a2 - a1;
        auto weight = [&](int j, float& b1, float& b2) {
            b1 = S[2 * (size_t)j];
            b2 = S[2 * (size_t)j + 1];
            const float d = fminf(a2, b2) - fmaxf(a1, b1);
            const float inter = d < 0.f ? 0.f : d;
            const float iou = inter / (alen + (b2 - b1) - inter);
            return (iou >= voting_thresh ? 1.f : 0.f) * W[j];
        };
        float total = 0.f, b1, b2;
        for (int j = lane; j < n; j += 64) total = total + weight(j, b1, b2);
        for (int o = 32; o > 0; o >>= 1) total = total + __shfl_xor(total, o, 64);
        float r1 = 0.f, r2 = 0.f;
        for (int j = lane; j < n; j += 64) {
            const float w = weight(j, b1, b2) / total;
            r1 = r1 + w * b1;
            r2 = r2 + w * b2;
        }
        for (int o = 32; o > 0; o >>= 1) {
            r1 = r1 + __shfl_xor(r1, o, 64);
            r2 = r2 + __shfl_xor(r2, o, 64);
        }
        if (lane == 0) {
            out[2 * (size_t)(k0 + k)] = r1;
            out[2 * (size_t)(k0 + k) + 1] = r2;
        }
    }
}

}  // namespace

extern "C" size_t otp_seg_nms_workspace(int G, int N) {
    if (G <= 0 || N <= 0) return 0;
    return (size_t)kWsWords * (size_t)N * sizeof(int);             // the groups share N rows, whatever G is
}

extern "C" int otp_seg_nms(const void* segs, const void* scores, const void* offsets, int G, int N, float iou_threshold,
                           float min_score, int max_num, void* workspace, size_t workspace_bytes, void* counts, void* keep,
                           void* stream) {
    if (!segs || !scores || !offsets || !workspace || !counts || !keep || G <= 0 || N <= 0) return OTP_ERR_BAD_ARG;
    if (iou_threshold != iou_threshold || min_score != min_score) return OTP_ERR_BAD_ARG;
    if (N >= (1 << 28)) return OTP_ERR_UNSUPPORTED;
    if (workspace_bytes < otp_seg_nms_workspace(G, N)) return OTP_ERR_WORKSPACE;
    hipLaunchKernelGGL(seg_nms_kernel, dim3(G), dim3(kThreads), 0, static_cast<hipStream_t>(stream),
                       static_cast<const float*>(segs), static_cast<const float*>(scores), static_cast<const int*>(offsets), N,
                       iou_threshold, min_score, max_num, static_cast<int*>(workspace), static_cast<int*>(counts),
                       static_cast<int*>(keep));
    return otp_launch_status();
}

extern "C" int otp_seg_softnms(const void* segs, const void* scores, const void* offsets, int G, int N, float iou_threshold,
                               float sigma, float min_score, int method, int max_num, void* workspace, size_t workspace_bytes,
                               void* counts, void* dets, void* inds, void* stream) {
    if (!segs || !scores || !offsets || !workspace || !counts || !dets || !inds || G <= 0 || N <= 0) return OTP_ERR_BAD_ARG;
    if (method < 0 || method > 2 || iou_threshold != iou_threshold || min_score != min_score) return OTP_ERR_BAD_ARG;
    if (method == 2 && !(sigma > 0.f && sigma * 0.f == 0.f)) return OTP_ERR_BAD_ARG;
    if (N >= (1 << 28)) return OTP_ERR_UNSUPPORTED;
    if (workspace_bytes < otp_seg_nms_workspace(G, N)) return OTP_ERR_WORKSPACE;
    hipLaunchKernelGGL(seg_softnms_kernel, dim3(G), dim3(kThreads), 0, static_cast<hipStream_t>(stream),
                       static_cast<const float*>(segs), static_cast<const float*>(scores), static_cast<const int*>(offsets), N,
                       iou_threshold, sigma, min_score, method, max_num, static_cast<int*>(workspace),
                       static_cast<int*>(counts), static_cast<float*>(dets), static_cast<int*>(inds));
    return otp_launch_status();
}

extern "C" int otp_seg_voting(const void* nms_segs, const void* nms_offsets, const void* segs, const void* scores,
                              const void* offsets, int G, int K, int N, float voting_thresh, void* out, void* stream) {
    if (!nms_segs || !nms_offsets || !segs || !scores || !offsets || !out || G <= 0 || K <= 0 || N <= 0) return OTP_ERR_BAD_ARG;
    if (voting_thresh != voting_thresh) return OTP_ERR_BAD_ARG;
    if (N >= (1 << 28) || K >= (1 << 28)) return OTP_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(seg_voting_kernel, dim3(G), dim3(kThreads), 0, static_cast<hipStream_t>(stream),
                       static_cast<const float*>(nms_segs), static_cast<const int*>(nms_offsets),
                       static_cast<const float*>(segs), static_cast<const float*>(scores), static_cast<const int*>(offsets), K,
                       N, voting_thresh, static_cast<float*>(out));
    return otp_launch_status();
}
