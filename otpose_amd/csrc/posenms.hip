// Pose NMS of top-down predictions, per frame: keypoint rescoring and OKS suppression (hard, soft gaussian, soft linear) in
// float64.  The arithmetic is the contract written out in include/otpose_hip.h (it follows HRNet's lib/nms/nms.py and the
// rescoring loop of its COCO evaluate; the reference declares the switches and carries no code behind them).  Plain C++: no
// inline assembly, no float atomics, every sum in a fixed order - the same input gives the same bytes.  DESIGN.md section 3.10.
#include "common.h"

// every product, quotient and sum rounded on its own, as numpy's element-wise float64 operations are (tests/pose_nms_ref.py)
#pragma clang fp contract(off)

namespace {

constexpr int kJ = OTP_POSENMS_JOINTS;            // the model's joint set
constexpr int kMaxPr = OTP_POSEVAL_MAX_PR;
constexpr int kPitch = kMaxPr + 1;                 // OKS tile: the rows of a small frame do not all start on one LDS bank
constexpr int kThreads = 256;

struct Sigmas { double v[kJ]; };                   // by value in the kernel arguments

// Order rule: descending score; of two equal scores the later person first (a stable ascending sort, reversed); a NaN
// before every number, several NaNs by the same tie rule.  A strict total order over (score, index).
__device__ __forceinline__ bool comes_before(double sb, int b, double sa, int a) {
    const bool nb = sb != sb, na = sa != sa;
    if (nb || na) return nb && (!na || b > a);
    return sb > sa || (sb == sa && b > a);
}

// One workgroup per frame of the CSR pack_predictions builds.  keep (NP) int8, person_score (NP) f64, rank (NP) int32,
// oks (NP, 64) f64 or null: row = the kept person g, column = the candidate d of the same frame, zeros past the frame.
__global__ __launch_bounds__(kThreads) void pose_nms_kernel(
    const int* __restrict__ pr_off, const int* __restrict__ pr_sample, const float* __restrict__ preds,
    const float* __restrict__ maxvals, const double* __restrict__ box_score, const double* __restrict__ area, Sigmas sig,
    double in_vis_thre, double oks_thresh, double oks_in_vis_thre, int mode, int max_dets, signed char* __restrict__ keep,
    double* __restrict__ person_score, int* __restrict__ rank, double* __restrict__ oks_out) {
    __shared__ double s_x[kMaxPr * kJ], s_y[kMaxPr * kJ], s_v[kMaxPr * kJ], s_oks[kMaxPr * kPitch];
    __shared__ double s_score[kMaxPr], s_area[kMaxPr];
    __shared__ int s_ord[kMaxPr], s_sample[kMaxPr];

    const int f = blockIdx.x, t = threadIdx.x;
    const int p0 = pr_off[f], np = pr_off[f + 1] - p0;
    if (np > kMaxPr || np <= 0) return;             // the host refuses such input; never index past the tiles

    // ---- load: thread per (person, joint); the placeholder person (-1) is a pose of zeros ---------------------------
    for (int e = t; e < np * kJ; e += kThreads) {
        const int p = e / kJ, s = pr_sample[p0 + p];
        double x = 0.0, y = 0.0, v = 0.0;
        if (s >= 0) {
            const int j = e - p * kJ;
            x = (double)preds[((size_t)s * kJ + j) * 2];
            y = (double)preds[((size_t)s * kJ + j) * 2 + 1];
            v = (double)maxvals[(size_t)s * kJ + j];
        }
        s_x[e] = x;
        s_y[e] = y;
        s_v[e] = v;
    }
    __syncthreads();

    // ---- person score: box score x mean confidence of the joints above in_vis_thre, 0 for the placeholder ----------
    if (t < np) {
        const int s = pr_sample[p0 + t];
        double kpt = 0.0, a = 0.0, score = 0.0;
        if (s >= 0) {
            int n = 0;
            for (int j = 0; j < kJ; ++j) {
                const double v = s_v[t * kJ + j];
                if (v > in_vis_thre) { kpt = kpt + v; ++n; }
            }
            if (n > 0) kpt = kpt / (double)n;
            score = kpt * box_score[s];
            a = area[s];
        }
        s_score[t] = score;
        s_area[t] = a;
        s_sample[t] = s;
    }
    __syncthreads();

    // ---- rank by counting: the number of persons that come before this one ------------------------------------------
    int my_rank = 0;
    if (t < np) {
        const double sa = s_score[t];
        for (int b = 0; b < np; ++b) my_rank += b != t && comes_before(s_score[b], b, sa, t);
        s_ord[my_rank] = t;
    }

    // ---- OKS tile: thread per ordered (kept g, candidate d) pair.  A pair with the placeholder is 0: it suppresses
    // nobody and nobody suppresses it. ---------------------------------------------------------------------------------
    const bool vis = oks_in_vis_thre == oks_in_vis_thre;                // NaN = no joint selection (HRNet's call)
    for (int e = t; e < np * np; e += kThreads) {
        const int g = e / np, d = e - g * np;
        double o = 0.0;
        if (s_sample[g] >= 0 && s_sample[d] >= 0) {
            const double half_area = (s_area[g] + s_area[d]) / 2 + 0x1p-52;
            double sum = 0.0;
            int n = 0;
            for (int j = 0; j < kJ; ++j) {
                if (vis && !(s_v[d * kJ + j] > oks_in_vis_thre)) continue;
                const double dx = s_x[d * kJ + j] - s_x[g * kJ + j], dy = s_y[d * kJ + j] - s_y[g * kJ + j];
                const double two_sigma = sig.v[j] * 2, var = two_sigma * two_sigma;
                const double ej = (dx * dx + dy * dy) / var / half_area / 2;
                sum = sum + exp(-ej);
                ++n;
            }
            o = n > 0 ? sum / (double)n : 0.0;
        }
        s_oks[g * kPitch + d] = o;
    }
    __syncthreads();
    if (oks_out)
        for (int e = t; e < np * kMaxPr; e += kThreads) {
            const int g = e / kMaxPr, d = e - g * kMaxPr;
            oks_out[(size_t)(p0 + g) * kMaxPr + d] = d < np ? s_oks[g * kPitch + d] : 0.0;
        }
    if (t >= 64) return;                            // one wave walks

    if (mode == 0) {
        // ---- hard NMS: lane = position in the order.  The first person alive is kept and kills every later one whose
        // OKS against it is NOT <= thresh (a NaN kills). -------------------------------------------------------------
        const int p = t < np ? s_ord[t] : 0;
        bool alive = t < np;
        for (int i = 0; i < np; ++i) {
            const unsigned long long mask = __ballot(alive);
            if (!((mask >> i) & 1)) continue;
            const int g = s_ord[i];
            if (alive && t > i && !(s_oks[g * kPitch + p] <= oks_thresh)) alive = false;
        }
        if (t < np) {
            keep[p0 + p] = (signed char)(alive || s_sample[p] < 0);
            person_score[p0 + t] = s_score[t];
            rank[p0 + t] = my_rank;
        }
        return;
    }

    // ---- soft NMS: lane = person.  max_dets times: the head of the order is taken with the score it has now, every
    // remaining score decays by its OKS against the head, and the wave arg-max under the order rule stands in for the
    // re-sort. ---------------------------------------------------------------------------------------------------------
    double sc = t < np ? s_score[t] : 0.0;
    bool remaining = t < np, taken = false;
    int step_taken = -1;
    for (int step = 0; step < max_dets; ++step) {
        if (!__ballot(remaining)) break;
        double bs = sc;
        int bi = remaining ? t : -1;
        for (int o = 32; o > 0; o >>= 1) {
            const double os = __shfl_xor(bs, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (oi >= 0 && (bi < 0 || comes_before(os, oi, bs, bi))) { bs = os; bi = oi; }
        }
        if (t == bi) {
            remaining = false;
            taken = true;
            step_taken = step;
        } else if (remaining) {
            const double o = s_oks[bi * kPitch + t];
            if (mode == 1) sc = sc * exp(-(o * o) / oks_thresh);
            else if (o >= oks_thresh) sc = sc * (1 - o);
        }
    }
    if (t < np) {
        keep[p0 + t] = (signed char)(taken || s_sample[t] < 0);
        person_score[p0 + t] = sc;
        rank[p0 + t] = step_taken;
    }
}

}  // namespace

extern "C" int otp_pose_nms(const void* pr_off, const void* pr_sample, const void* preds, const void* maxvals,
                            const void* box_score, const void* area, const double* sigmas, double in_vis_thre,
                            double oks_thresh, double oks_in_vis_thre, int mode, int max_dets, void* keep,
                            void* person_score, void* rank, void* oks, int F, int NP, int N, void* stream) {
    if (!pr_off || !pr_sample || !sigmas || !keep || !person_score || !rank) return OTP_ERR_BAD_ARG;
    if (F <= 0 || NP <= 0 || N < 0 || mode < 0 || mode > 2 || max_dets < 1) return OTP_ERR_BAD_ARG;
    if (N > 0 && (!preds || !maxvals || !box_score || !area)) return OTP_ERR_BAD_ARG;
    if (!(oks_thresh > 0.0) || oks_thresh * 0.0 != 0.0) return OTP_ERR_BAD_ARG;
    Sigmas sig;
    for (int j = 0; j < kJ; ++j) {
        if (!(sigmas[j] > 0.0) || sigmas[j] * 0.0 != 0.0) return OTP_ERR_BAD_ARG;
        sig.v[j] = sigmas[j];
    }
    hipLaunchKernelGGL(pose_nms_kernel, dim3(F), dim3(kThreads), 0, static_cast<hipStream_t>(stream),
                       static_cast<const int*>(pr_off), static_cast<const int*>(pr_sample), static_cast<const float*>(preds),
                       static_cast<const float*>(maxvals), static_cast<const double*>(box_score),
                       static_cast<const double*>(area), sig, in_vis_thre, oks_thresh, oks_in_vis_thre, mode, max_dets,
                       static_cast<signed char*>(keep), static_cast<double*>(person_score), static_cast<int*>(rank),
                       static_cast<double*>(oks));
    return otp_launch_status();
}
