// Temporal detection AP (the reference's thirdparty/utils/metrics.py: compute_average_precision_detection, segment_iou,
// interpolated_prec_rec) on a segmented batch, behind otpose_amd/segmetrics.py:
//   otp_seg_ap_match   the greedy assignment of predictions to ground-truth segments: G groups, one per (video, class) pair, given
//                      by two offset tables over flat float64 segments; one workgroup per group, every threshold in one launch
//   otp_seg_ap         interpolated AP per (class, threshold) from the matches: one workgroup each
// A prediction only touches the locks of its own group, so the reference's loop over all predictions of a class is sequential
// only inside a group; and "the first unlocked ground truth in descending tIoU that reaches the threshold" is an arg-max, not a
// sort.  The arithmetic is the contract written out in include/otpose_hip.h.  Plain C++: no inline assembly, no atomics, every
// sum in a fixed order - the same input gives the same bytes.  DESIGN.md section 3.15.
#include "common.h"

// every difference, sum and quotient rounded on its own, as numpy rounds them (tests/segap_ref.py)
#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kCap = OTP_SEG_AP_LDS_GT;
constexpr int kMaxT = OTP_SEG_AP_MAX_THRESHOLDS;
static_assert(kCap % 64 == 0 && kCap / 64 <= 32, "a lane's locks of an LDS group are the bits of one register");

struct Thresholds {
    double v[kMaxT];
};

// [o0, o0 + n) of group g, or n = -1 for offsets that do not describe a range inside [0, N]
__device__ __forceinline__ int group_range(const int* __restrict__ offsets, int g, int N, int& o0) {
    o0 = offsets[g];
    const int o1 = offsets[g + 1];
    return (o0 < 0 || o1 < o0 || o1 > N) ? -1 : o1 - o0;
}

// numpy's maximum / minimum: a NaN operand is the result
__device__ __forceinline__ double np_maximum(double a, double b) { return a != a ? a : (b != b ? b : (a > b ? a : b)); }
__device__ __forceinline__ double np_minimum(double a, double b) { return a != a ? a : (b != b ? b : (a < b ? a : b)); }

// segment_iou (metrics.py:285-309) of prediction (t0, t1) and ground truth (c0, c1)
__device__ __forceinline__ double tiou(double t0, double t1, double c0, double c1) {
    const double d = np_minimum(t1, c1) - np_maximum(t0, c0);
    const double inter = d < 0.0 ? 0.0 : d;           // clip(0): a NaN stays
    const double uni = (c1 - c0) + (t1 - t0) - inter;
    return inter / uni;
}

// the order of the reference's argsort()[::-1]: a NaN above every number, then descending; equal values by ascending row
__device__ __forceinline__ bool before(double va, int ra, double vb, int rb) {
    const bool na = va != va, nb = vb != vb;
    if (na != nb) return na;
    if (!na && va != vb) return va > vb;
    return ra < rb;
}

// ---- the greedy assignment -------------------------------------------------------------------------------------------------
// Wave w owns thresholds w, w + kWaves, ... and walks the group's predictions in order.  Lane l owns the ground truths l, l + 64,
// ...: it alone reads and sets their locks, so a threshold's locks are lane-private bits - one register for a group in LDS
// (kWs = false: at most kCap / 64 <= 32 ground truths per lane), 32-bit words [word][lane] in the workspace otherwise.  The
// predictions come in blocks of 64, one per lane, and are handed round with a lane read; so do the results go out.
template <bool kWs>
__device__ __forceinline__ void match_group(const double* __restrict__ gt, const double* s_c0, const double* s_c1, int m,
                                            const double* __restrict__ pred, int n, const Thresholds& thr, int T,
                                            unsigned* __restrict__ ws, size_t plane, int* __restrict__ match, int N) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wpl = ((m + 63) / 64 + 31) / 32;        // lock words per lane
    for (int t = wave; t < T; t += kWaves) {
        const double th = thr.v[t];
        unsigned* L = kWs ? ws + (size_t)t * plane : nullptr;
        if (kWs)
            for (int w = 0; w < wpl; ++w) L[w * 64 + lane] = 0u;
        unsigned locks = 0u;
        int* out = match + (size_t)t * N;
        for (int base = 0; base < n; base += 64) {
            const int cnt = n - base < 64 ? n - base : 64;
            double my0 = 0.0, my1 = 0.0;
            if (lane < cnt) {
                my0 = pred[2 * (size_t)(base + lane)];
                my1 = pred[2 * (size_t)(base + lane) + 1];
            }
            int mine = -1;
            for (int k = 0; k < cnt; ++k) {
                const double t0 = __shfl(my0, k, 64), t1 = __shfl(my1, k, 64);
                double bv = 0.0;
                int br = -1;
                unsigned word = locks;
                for (int j = lane, i = 0; j < m; j += 64, ++i) {
                    if (kWs && (i & 31) == 0) word = L[(i >> 5) * 64 + lane];
                    if ((word >> (i & 31)) & 1u) continue;
                    const double v = kWs ? tiou(t0, t1, gt[2 * (size_t)j], gt[2 * (size_t)j + 1]) : tiou(t0, t1, s_c0[j], s_c1[j]);
                    if (v < th) continue;             // the reference's test: a NaN tIoU passes it
                    if (br < 0 || before(v, j, bv, br)) { bv = v; br = j; }
                }
                for (int o = 32; o > 0; o >>= 1) {
                    const double ov = __shfl_xor(bv, o, 64);
                    const int orow = __shfl_xor(br, o, 64);
                    if (orow >= 0 && (br < 0 || before(ov, orow, bv, br))) { bv = ov; br = orow; }
                }
                if (br >= 0 && (br & 63) == lane) {   // the owner locks it
                    const int i = br >> 6;
                    if (kWs) L[(i >> 5) * 64 + lane] |= 1u << (i & 31);
                    else locks |= 1u << i;
                }
                if (lane == k) mine = br;
            }
            if (lane < cnt) out[base + lane] = mine;
        }
    }
}

__global__ __launch_bounds__(kThreads) void seg_ap_match_kernel(const double* __restrict__ pred_seg,
                                                                const int* __restrict__ pred_offsets,
                                                                const double* __restrict__ gt_seg,
                                                                const int* __restrict__ gt_offsets, int N, int M, Thresholds thr,
                                                                int T, unsigned* __restrict__ ws, size_t plane,
                                                                int* __restrict__ match) {
    __shared__ double s_c0[kCap], s_c1[kCap];
    const int g = blockIdx.x;
    int p0, q0;
    const int n = group_range(pred_offsets, g, N, p0);
    if (n <= 0) return;                               // nothing to answer, or rows that cannot be named: match holds -1 already
    const int m = group_range(gt_offsets, g, M, q0);
    if (m <= 0) return;                               // no ground truth: every prediction is a false positive
    const double* P = pred_seg + 2 * (size_t)p0;
    const double* Q = gt_seg + 2 * (size_t)q0;
    if (m <= kCap) {
        for (int j = threadIdx.x; j < m; j += kThreads) {
            s_c0[j] = Q[2 * (size_t)j];
            s_c1[j] = Q[2 * (size_t)j + 1];
        }
        __syncthreads();
        match_group<false>(Q, s_c0, s_c1, m, P, n, thr, T, nullptr, 0, match + p0, N);
    } else {                                          // the group's own words of every threshold's plane (otp_seg_ap_match_workspace)
        unsigned* w = ws + (size_t)(q0 >> 5) + 64 * (size_t)(q0 / kCap);
        match_group<true>(Q, s_c0, s_c1, m, P, n, thr, T, w, plane, match + p0, N);
    }
}

// words of one threshold's plane.  A group with m > kCap ground truths at offset q0 owns 64 * ceil(ceil(m / 64) / 32) <=
// m / 32 + 64 words from word q0 / 32 + 64 * (q0 / kCap) on: the next such group starts at q0' >= q0 + m, which moves the first
// term by at least m / 32 and the second by at least 64; the last word of any range inside [0, M] lies below the plane's end.
inline size_t plane_words(int M) { return (size_t)(M >> 5) + 64 * (size_t)(M / kCap) + 64; }

// ---- AP from the matches ---------------------------------------------------------------------------------------------------
// Position i of a class (its rows in descending score) is a true positive when its match is >= 0; k_i true positives up to and
// including it.  precision_i = k_i / (i + 1), recall_i = k_i / npos.  AP = sum over the true positives of
// (k_i / npos - (k_i - 1) / npos) * max_{j >= i} precision_j: the positions where recall changes are the true positives, and the
// reference's closing term has the precision 0.  The chunks are walked from the end with the suffix maximum carried along.
__global__ __launch_bounds__(kThreads) void seg_ap_kernel(const int* __restrict__ match, const int* __restrict__ order,
                                                          const int* __restrict__ class_offsets, const int* __restrict__ npos,
                                                          int C, int N, double* __restrict__ ap) {
    __shared__ int s_cnt[kWaves];
    __shared__ double s_max[kWaves], s_sum[kWaves];
    const int c = blockIdx.x, t = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int o0;
    const int n = group_range(class_offsets, c, N, o0);
    const int np = npos[c];
    double* out = ap + (size_t)t * C + c;
    if (n <= 0 || np <= 0) {
        if (tid == 0) *out = 0.0;
        return;
    }
    const int* mt = match + (size_t)t * N;
    const int* ord = order + o0;
    auto is_tp = [&](int i) {
        if (i >= n) return false;
        const int r = ord[i];
        return r >= 0 && r < N && mt[r] >= 0;
    };

    int total = 0;
    for (int base = 0; base < n; base += kThreads) total += __syncthreads_count(is_tp(base + tid));

    const double dn = (double)np;
    int behind = 0;                                   // true positives in the chunks already walked (the later positions)
    double carry = 0.0, acc = 0.0;                    // max precision over the later chunks; this thread's terms
    for (int base = (n - 1) / kThreads * kThreads; base >= 0; base -= kThreads) {
        const int i = base + tid;
        const bool flag = is_tp(i);
        const unsigned long long mask = __ballot(flag);
        if (lane == 0) s_cnt[wave] = __popcll(mask);
        __syncthreads();
        int before_wave = 0, chunk = 0;
        for (int w = 0; w < kWaves; ++w) {
            if (w < wave) before_wave += s_cnt[w];
            chunk += s_cnt[w];
        }
        const int k = total - behind - chunk + before_wave + __popcll(mask & ((2ull << lane) - 1ull));
        double sm = i < n ? (double)k / (double)(i + 1) : 0.0;
        for (int o = 1; o < 64; o <<= 1) {            // suffix maximum over the wave
            const double other = __shfl_down(sm, o, 64);
            if (lane + o < 64) sm = fmax(sm, other);
        }
        if (lane == 0) s_max[wave] = sm;
        __syncthreads();
        double all = carry;
        for (int w = 0; w < kWaves; ++w) {
            const double v = s_max[w];
            if (w > wave) sm = fmax(sm, v);
            all = fmax(all, v);
        }
        sm = fmax(sm, carry);
        if (flag) acc = acc + ((double)k / dn - (double)(k - 1) / dn) * sm;
        carry = all;
        behind += chunk;
        __syncthreads();                              // s_cnt and s_max are written again in the next chunk
    }
    for (int o = 32; o > 0; o >>= 1) acc = acc + __shfl_xor(acc, o, 64);
    if (lane == 0) s_sum[wave] = acc;
    __syncthreads();
    if (tid == 0) *out = (s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3]);
}
static_assert(kWaves == 4, "the last line of seg_ap_kernel adds four wave sums");

}  // namespace

extern "C" size_t otp_seg_ap_match_workspace(int G, int M, int T) {
    if (G <= 0 || M <= 0 || T <= 0) return 0;
    return (size_t)T * plane_words(M) * sizeof(unsigned);          // whatever G is: only groups above OTP_SEG_AP_LDS_GT take rows
}

extern "C" int otp_seg_ap_match(const void* pred_seg, const void* pred_offsets, const void* gt_seg, const void* gt_offsets,
                                const double* thresholds, int G, int N, int M, int T, void* workspace, size_t workspace_bytes,
                                void* match, void* stream) {
    if (!pred_seg || !pred_offsets || !gt_seg || !gt_offsets || !thresholds || !workspace || !match) return OTP_ERR_BAD_ARG;
    if (G <= 0 || N <= 0 || M <= 0 || T <= 0) return OTP_ERR_BAD_ARG;
    if (T > kMaxT || N >= (1 << 28) || M >= (1 << 28)) return OTP_ERR_UNSUPPORTED;
    Thresholds thr = {};
    for (int t = 0; t < T; ++t) {
        if (thresholds[t] != thresholds[t]) return OTP_ERR_BAD_ARG;
        thr.v[t] = thresholds[t];
    }
    if (workspace_bytes < otp_seg_ap_match_workspace(G, M, T)) return OTP_ERR_WORKSPACE;
    hipStream_t s = static_cast<hipStream_t>(stream);
    // -1 everywhere first: the rows of a group that cannot be named, of one without ground truth, and of no group at all
    if (hipMemsetAsync(match, 0xff, (size_t)T * (size_t)N * sizeof(int), s) != hipSuccess) return OTP_ERR_LAUNCH;
    hipLaunchKernelGGL(seg_ap_match_kernel, dim3(G), dim3(kThreads), 0, s, static_cast<const double*>(pred_seg),
                       static_cast<const int*>(pred_offsets), static_cast<const double*>(gt_seg),
                       static_cast<const int*>(gt_offsets), N, M, thr, T, static_cast<unsigned*>(workspace), plane_words(M),
                       static_cast<int*>(match));
    return otp_launch_status();
}

extern "C" int otp_seg_ap(const void* match, const void* order, const void* class_offsets, const void* npos, int C, int T, int N,
                          void* ap, void* stream) {
    if (!match || !order || !class_offsets || !npos || !ap || C <= 0 || T <= 0 || N <= 0) return OTP_ERR_BAD_ARG;
    if (T > kMaxT || N >= (1 << 28)) return OTP_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(seg_ap_kernel, dim3(C, T), dim3(kThreads), 0, static_cast<hipStream_t>(stream),
                       static_cast<const int*>(match), static_cast<const int*>(order), static_cast<const int*>(class_offsets),
                       static_cast<const int*>(npos), C, N, static_cast<double*>(ap));
    return otp_launch_status();
}
