// PoseTrack / poseval pose evaluation (reference utils/evaluate.py): the per-frame assignment of predicted persons to
// ground-truth persons and the per-joint VOC average precision, in float64.  Plain C++: no inline assembly, no float
// atomics, every sum in a fixed order - the same input gives the same bytes.  DESIGN.md section 3.9.
#include "common.h"

// every product and sum rounded on its own, as numpy's element-wise float64 operations are (tests/posetrack_ap_ref.py)
#pragma clang fp contract(off)

namespace {

constexpr int kJ = OTP_POSEVAL_JOINTS;            // PoseTrack_Official_Keypoint_Ordering (configs/constants.py:2-18)
constexpr int kMaxPr = OTP_POSEVAL_MAX_PR;
constexpr int kMaxGt = OTP_POSEVAL_MAX_GT;
constexpr int kThreads = 256;

// coco2posetrack_ord (utils/keypoints.py:7-28): official joint k is read from this index of the model's 17-joint ordering
// (PoseTrack_COCO_Keypoint_Ordering, configs/constants.py:38-56).  All 15 official names occur among the 17, so the
// 'neck' / 'head_top' synthesis branches of utils/keypoints.py:29-65 are dead for this configuration and are not built.
__constant__ int kCocoOfOfficial[kJ] = {16, 14, 12, 11, 13, 15, 10, 8, 6, 5, 7, 9, 1, 0, 2};

// Even-odd crossing test in float64 (the reference calls shapely's Polygon.contains, utils/evaluate.py:28-33).  An edge
// counts when exactly one of its ends lies strictly above the point's row and the point lies strictly left of the edge's
// crossing of that row; horizontal (and zero-length) edges never count.  A point on the boundary therefore falls to
// either side (left / bottom edges in, right / top edges out); tests keep points 1e-6 px away from every edge.
__device__ bool in_any_polygon(double px, double py, const int* vert_off, const double* vert_xy, int p0, int p1) {
    for (int p = p0; p < p1; ++p) {
        const int v0 = vert_off[p], v1 = vert_off[p + 1];
        bool in = false;
        for (int i = v0, j = v1 - 1; i < v1; j = i++) {
            const double xi = vert_xy[2 * i], yi = vert_xy[2 * i + 1], xj = vert_xy[2 * j], yj = vert_xy[2 * j + 1];
            if ((yi > py) != (yj > py)) {
                const double xc = (xj - xi) * (py - yi) / (yj - yi) + xi;
                if (px < xc) in = !in;
            }
        }
        if (in) return true;                       // utils/evaluate.py:30-34: the first containing polygon decides
    }
    return false;
}

// One workgroup per ground-truth frame: removeIgnoredPoints (utils/evaluate.py:22-67) + one iteration of assignGTmulti's
// frame loop (utils/evaluate.py:498-680).  Removed persons keep their slot (alive = 0), so "first on ties" over the alive
// slots is the reference's first argmax over the compacted lists.
__global__ __launch_bounds__(kThreads) void pose_assign_kernel(
    const int* __restrict__ pr_off, const int* __restrict__ pr_sample, const float* __restrict__ preds,
    const float* __restrict__ maxvals, const double* __restrict__ box_score, const int* __restrict__ gt_off,
    const double* __restrict__ gt_xy, const int* __restrict__ gt_has, const double* __restrict__ gt_head,
    const int* __restrict__ poly_off, const int* __restrict__ vert_off, const double* __restrict__ vert_xy,
    double dist_thresh, signed char* __restrict__ labels, double* __restrict__ scores, int* __restrict__ ngt) {
    __shared__ double s_px[kMaxPr * kJ], s_py[kMaxPr * kJ], s_gx[kMaxGt * kJ], s_gy[kMaxGt * kJ], s_head[kMaxGt];
    __shared__ double s_bestval[kMaxPr];
    __shared__ unsigned char s_phas[kMaxPr * kJ], s_ghas[kMaxGt * kJ], s_cnt[kMaxPr * kMaxGt];
    __shared__ unsigned short s_match[kMaxPr * kMaxGt], s_pmask[kMaxPr], s_gmask[kMaxGt];
    __shared__ int s_ngtp[kMaxGt], s_bestgt[kMaxPr], s_assign[kMaxPr], s_alive[2];

    const int f = blockIdx.x, t = threadIdx.x;
    const int p0 = pr_off[f], g0 = gt_off[f], q0 = poly_off[f], q1 = poly_off[f + 1];
    const int np = pr_off[f + 1] - p0, ng = gt_off[f + 1] - g0;
    if (np > kMaxPr || ng > kMaxGt || np < 0 || ng < 0) {       // the host refuses such input; never index past the tiles
        for (int e = t; e < (np > 0 ? np : 0) * kJ; e += kThreads) { labels[(size_t)p0 * kJ + e] = -1; scores[(size_t)p0 * kJ + e] = 0.0; }
        if (t < kJ) ngt[f * kJ + t] = 0;
        return;
    }

    // ---- load, joint permutation, ignore regions ----------------------------------------------------------------
    for (int e = t; e < np * kJ; e += kThreads) {
        const int p = e / kJ, k = e - p * kJ, s = pr_sample[p0 + p];
        double x = 0.0, y = 0.0;
        bool has;
        if (s < 0) {
            has = k == 0;                          // the placeholder person of a frame without detections: one point,
        } else {                                   // id 0 at (0, 0) (utils/evaluate.py:787-796)
            const float* q = preds + ((size_t)s * 17 + kCocoOfOfficial[k]) * 2;
            x = (double)q[0];
            y = (double)q[1];
            has = true;
        }
        if (has && q1 > q0 && in_any_polygon(x, y, vert_off, vert_xy, q0, q1)) has = false;
        s_px[e] = x;
        s_py[e] = y;
        s_phas[e] = has;
    }
    for (int e = t; e < ng * kJ; e += kThreads) {
        const int g = e / kJ, k = e - g * kJ;
        const double x = gt_xy[((size_t)(g0 + g) * kJ + k) * 2], y = gt_xy[((size_t)(g0 + g) * kJ + k) * 2 + 1];
        bool has = (gt_has[g0 + g] >> k) & 1;
        if (has && q1 > q0 && in_any_polygon(x, y, vert_off, vert_xy, q0, q1)) has = false;
        s_gx[e] = x;
        s_gy[e] = y;
        s_ghas[e] = has;
    }
    if (t < ng) {
        // get_head_size (utils/evaluate.py:462-464): 0.6 * ||(x2 - x1, y2 - y1)||
        const double* h = gt_head + (size_t)(g0 + t) * 4;
        const double dx = h[2] - h[0], dy = h[3] - h[1];
        s_head[t] = 0.6 * sqrt(dx * dx + dy * dy);
    }
    __syncthreads();

    // ---- per-person joint masks; a person of a frame WITH ignore regions that has no point left is removed
    // (utils/evaluate.py:37-42; frames without regions are not filtered, :49-50, so a GT person annotated with an empty
    // point list stays there with nGTp = 0) -------------------------------------------------------------------------
    if (t < np) {
        unsigned m = 0;
        for (int k = 0; k < kJ; ++k) m |= (unsigned)s_phas[t * kJ + k] << k;
        s_pmask[t] = (unsigned short)m;
        s_assign[t] = -1;
    } else if (t >= 64 && t < 64 + ng) {
        const int g = t - 64;
        unsigned m = 0;
        for (int k = 0; k < kJ; ++k) m |= (unsigned)s_ghas[g * kJ + k] << k;
        s_gmask[g] = (unsigned short)m;
        s_ngtp[g] = __popc(m);
    }
    __syncthreads();
    const bool filtered = q1 > q0;
    if (t == 0) {
        int a = 0;
        for (int p = 0; p < np; ++p) a += !filtered || s_pmask[p];
        s_alive[0] = a;
    } else if (t == 64) {
        int a = 0;
        for (int g = 0; g < ng; ++g) a += !filtered || s_gmask[g];
        s_alive[1] = a;
    }
    if (t >= 128 && t < 128 + kJ) {               // nGTall (utils/evaluate.py:675-678)
        const int k = t - 128;
        int n = 0;
        for (int g = 0; g < ng; ++g) n += s_ghas[g * kJ + k];
        ngt[f * kJ + k] = n;
    }

    // ---- match[pr, gt, joint] = dist <= thresh and its joint sum (utils/evaluate.py:574-591) -----------------------
    for (int e = t; e < np * ng; e += kThreads) {
        const int p = e / ng, g = e - p * ng;
        const unsigned both = s_pmask[p] & s_gmask[g];
        const double head = s_head[g];
        unsigned m = 0;
        for (int k = 0; k < kJ; ++k) {
            if (!((both >> k) & 1)) continue;      // dist stays inf: no match
            const double dx = s_gx[g * kJ + k] - s_px[p * kJ + k], dy = s_gy[g * kJ + k] - s_py[p * kJ + k];
            const double d = sqrt(dx * dx + dy * dy) / head;
            if (d <= dist_thresh) m |= 1u << k;
        }
        s_match[p * kMaxGt + g] = (unsigned short)m;
        s_cnt[p * kMaxGt + g] = (unsigned char)__popc(m);
    }
    __syncthreads();
    const int alive_pr = s_alive[0], alive_gt = s_alive[1];

    // ---- pck[i, j] = sum / nGTp[j] (undivided for nGTp = 0); each predicted person keeps its best GT only, first on
    // ties (utils/evaluate.py:592-603) --------------------------------------------------------------------------------
    if (t < np) {
        int best = -1;
        double bv = 0.0;
        if (!filtered || s_pmask[t]) {
            for (int g = 0; g < ng; ++g) {
                if (filtered && !s_gmask[g]) continue;
                const int n = s_ngtp[g];
                const double v = n > 0 ? (double)s_cnt[t * kMaxGt + g] / (double)n : (double)s_cnt[t * kMaxGt + g];
                if (best < 0 || v > bv) { best = g; bv = v; }
            }
        }
        s_bestgt[t] = best;
        s_bestval[t] = bv;
    }
    __syncthreads();
    // ---- each GT takes the best remaining predicted person, first on ties; a best value of 0 takes nobody
    // (utils/evaluate.py:604-606).  A predicted person is the best of at most one GT, so the writes do not collide. -----
    if (t < ng && (!filtered || s_gmask[t])) {
        int best = -1;
        double bv = 0.0;
        for (int p = 0; p < np; ++p)
            if (s_bestgt[p] == t && s_bestval[p] > bv) { best = p; bv = s_bestval[p]; }
        if (best >= 0) s_assign[best] = t;
    }
    __syncthreads();

    // ---- labels and scores (utils/evaluate.py:629-661): only joints with hasPr produce an entry ---------------------
    for (int e = t; e < np * kJ; e += kThreads) {
        const int p = e / kJ, k = e - p * kJ;
        signed char lab = -1;
        double sc = 0.0;
        if (s_phas[e] && alive_pr > 0) {
            const int s = pr_sample[p0 + p], g = s_assign[p];
            // coco2posetrack_ord: local_score = (p + p) / 2.0 (exact), conf = local_score * global_score
            sc = s < 0 ? -100.0 : (double)maxvals[(size_t)s * 17 + kCocoOfOfficial[k]] * box_score[s];
            lab = (alive_gt > 0 && g >= 0) ? (signed char)((s_match[p * kMaxGt + g] >> k) & 1) : (signed char)0;
        }
        labels[(size_t)p0 * kJ + e] = lab;
        scores[(size_t)p0 * kJ + e] = sc;
    }
}

// One workgroup per joint over that joint's entries sorted by descending score: compute_rpc (utils/evaluate.py:686-702)
// and vocap (:735-751).  Thread t owns the contiguous slice [t * per, (t + 1) * per) of the entries; the three passes
// (count, precision maximum, area) meet in two scans over the 256 slice totals, and the partial areas are added by one
// thread in slice order.
__global__ __launch_bounds__(kThreads) void ap_curve_kernel(const signed char* __restrict__ labels,
                                                            const long long* __restrict__ joint_off,
                                                            const long long* __restrict__ n_gt, double* __restrict__ out,
                                                            double* __restrict__ precision, double* __restrict__ recall) {
    __shared__ long long s_pos[kThreads];
    __shared__ double s_max[kThreads], s_sum[kThreads];
    __shared__ long long s_total;
    const int j = blockIdx.x, t = threadIdx.x;
    const long long e0 = joint_off[j], n = joint_off[j + 1] - e0;
    if (n <= 0) {                                  // compute_metrics leaves the zeros of np.zeros (utils/evaluate.py:720)
        if (t < 3) out[j * 3 + t] = 0.0;
        return;
    }
    const signed char* lab = labels + e0;
    const double total = (double)n_gt[j];          // nGT = sum(nGTall[j, :]), a float64 (utils/evaluate.py:718)
    const long long per = (n + kThreads - 1) / kThreads;
    const long long b = per * t < n ? per * t : n, e = b + per < n ? b + per : n;

    long long c = 0;
    for (long long i = b; i < e; ++i) c += lab[i] == 1;
    s_pos[t] = c;
    __syncthreads();
    if (t == 0) {                                  // exclusive scan of the slice counts
        long long run = 0;
        for (int k = 0; k < kThreads; ++k) { const long long v = s_pos[k]; s_pos[k] = run; run += v; }
        s_total = run;
    }
    __syncthreads();
    const long long start = s_pos[t];

    // precision[i] = npos / (i + 1), recall[i] = npos / nGT (utils/evaluate.py:698-700)
    long long npos = start;
    double m = 0.0;
    for (long long i = b; i < e; ++i) {
        npos += lab[i] == 1;
        const double pr = (double)npos / (double)(i + 1);
        if (pr > m) m = pr;
        if (precision) precision[e0 + i] = pr;
        if (recall) recall[e0 + i] = (double)npos / total;
    }
    s_max[t] = m;
    __syncthreads();
    if (t == 0) {                                  // mpre of the slices to the right; the closing sentinel is 0
        double run = 0.0;
        for (int k = kThreads - 1; k >= 0; --k) { const double v = s_max[k]; s_max[k] = run; if (v > run) run = v; }
    }
    __syncthreads();

    // right to left: mpre[i] = max(precision[i], mpre[i + 1]); area where recall changes (utils/evaluate.py:742-749)
    double mpre = s_max[t], sum = 0.0;
    npos = start + c;
    for (long long i = e - 1; i >= b; --i) {
        const double pr = (double)npos / (double)(i + 1), rc = (double)npos / total;
        if (pr > mpre) mpre = pr;
        npos -= lab[i] == 1;
        const double prev = i == 0 ? 0.0 : (double)npos / total;
        if (!(rc == prev)) sum = sum + (rc - prev) * mpre;
    }
    s_sum[t] = sum;
    __syncthreads();
    if (t == 0) {
        double ap = 0.0;
        for (int k = 0; k < kThreads; ++k) ap = ap + s_sum[k];
        const long long last = s_total;
        const double pl = (double)last / (double)n, rl = (double)last / total;
        // the closing sentinel: mrec = 1.0 meets mpre = 0 (utils/evaluate.py:736-740); kept for its NaN when nGT = 0
        if (!(1.0 == rl)) ap = ap + (1.0 - rl) * 0.0;
        out[j * 3] = ap * 100.0;                   // compute_metrics (utils/evaluate.py:721-723)
        out[j * 3 + 1] = pl * 100.0;
        out[j * 3 + 2] = rl * 100.0;
    }
}

}  // namespace

extern "C" int otp_pose_assign(const void* pr_off, const void* pr_sample, const void* preds, const void* maxvals,
                               const void* box_score, const void* gt_off, const void* gt_xy, const void* gt_has,
                               const void* gt_head, const void* poly_off, const void* vert_off, const void* vert_xy,
                               double dist_thresh, void* labels, void* scores, void* ngt, int F, int NP, int N, int NG,
                               void* stream) {
    if (!pr_off || !pr_sample || !gt_off || !poly_off || !vert_off || !labels || !scores || !ngt) return OTP_ERR_BAD_ARG;
    if (F <= 0 || NP <= 0 || N < 0 || NG < 0) return OTP_ERR_BAD_ARG;
    if (N > 0 && (!preds || !maxvals || !box_score)) return OTP_ERR_BAD_ARG;
    if (NG > 0 && (!gt_xy || !gt_has || !gt_head)) return OTP_ERR_BAD_ARG;
    hipLaunchKernelGGL(pose_assign_kernel, dim3(F), dim3(kThreads), 0, static_cast<hipStream_t>(stream),
                       static_cast<const int*>(pr_off), static_cast<const int*>(pr_sample), static_cast<const float*>(preds),
                       static_cast<const float*>(maxvals), static_cast<const double*>(box_score),
                       static_cast<const int*>(gt_off), static_cast<const double*>(gt_xy), static_cast<const int*>(gt_has),
                       static_cast<const double*>(gt_head), static_cast<const int*>(poly_off),
                       static_cast<const int*>(vert_off), static_cast<const double*>(vert_xy), dist_thresh,
                       static_cast<signed char*>(labels), static_cast<double*>(scores), static_cast<int*>(ngt));
    return otp_launch_status();
}

extern "C" int otp_ap_curve(const void* labels_sorted, const void* joint_off, const void* n_gt, void* out, void* precision,
                            void* recall, int J, void* stream) {
    if (!labels_sorted || !joint_off || !n_gt || !out || J <= 0) return OTP_ERR_BAD_ARG;
    hipLaunchKernelGGL(ap_curve_kernel, dim3(J), dim3(kThreads), 0, static_cast<hipStream_t>(stream),
                       static_cast<const signed char*>(labels_sorted), static_cast<const long long*>(joint_off),
                       static_cast<const long long*>(n_gt), static_cast<double*>(out), static_cast<double*>(precision),
                       static_cast<double*>(recall));
    return otp_launch_status();
}
