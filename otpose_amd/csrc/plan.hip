// otp_pose_plan: the crop plan of the video path on the device - what otpose_amd/crop.py computes on the host per person
// (box -> center / scale, the rotation-0 crop matrix, the 5-frame window) plus the compaction of the detector's (frame, box)
// grid into dense rows.  The contract is in include/otpose_hip.h; the host functions are the specification.
//
// One launch of ONE workgroup: the plan of a chunk is a few thousand (frame, box) pairs of some fifty operations each, so the
// launch latency is the cost and a second workgroup would only buy an inter-workgroup hand-off of the scan.  The workgroup
// (a) scans the kept counts of the frames in passes of PLAN_THREADS frames (wave scans joined through LDS, a running carry),
// (b) strides over the (frame, box) pairs and writes the row of every kept one, (c) fills the padding rows.
//
// Every step that the host code rounds is rounded here: this file is compiled without FMA contraction (the pragma below and
// -ffp-contract=off in the Makefile), because a fused x + w * 0.5 would change center / scale in the last bit.
#include "common.h"

#pragma clang fp contract(off)

#define PLAN_THREADS 1024
#define PLAN_WAVES (PLAN_THREADS / 64)

namespace {

__device__ __forceinline__ int plan_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// kept: inside the frame's count and not below min_score (the comparison is made in double)
__device__ __forceinline__ bool plan_kept(const float* __restrict__ scores, int s, int k, int K, double min_score) {
    return !((double)scores[(size_t)s * K + k] < min_score);
}

// The pool slot that holds frame number `target` of the sequence of slot s, looking at most two slots away in direction dir
// (+1 / -1); -1 if there is none.  A sequence is a run of slots with one num_frames and strictly increasing frame numbers.
__device__ __forceinline__ int plan_find(const int* __restrict__ fn, const int* __restrict__ nf, int S, int s, int target, int dir) {
    int last = fn[s];
    if (target == last) return s;
    const int n = nf[s];
    int t = s;
    for (int step = 0; step < 2; ++step) {
        t += dir;
        if (t < 0 || t >= S || nf[t] != n) return -1;
        const int f = fn[t];
        if (dir > 0 ? f <= last : f >= last) return -1;
        if (f == target) return t;
        last = f;
    }
    return -1;
}

__global__ __launch_bounds__(PLAN_THREADS) void pose_plan_kernel(
    const double* __restrict__ boxes, const float* __restrict__ scores, const int* __restrict__ counts,
    const int* __restrict__ frame_number, const int* __restrict__ num_frames, int S, int K, int lo, int hi, double min_score,
    double ar, float enlarge, float out_w, float out_h, int pt18, int P, float* __restrict__ center, float* __restrict__ scale,
    double* __restrict__ M, int* __restrict__ frame_idx, float* __restrict__ margin, double* __restrict__ box_score,
    int* __restrict__ person_slot, int* __restrict__ pr_off, int* __restrict__ total) {
    __shared__ int wave_tot[PLAN_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    // ---- (a) exclusive scan of the kept counts: pr_off[s] = min(persons before frame s, P) -------------------------------
    int carry = 0;
    for (int base = 0; base < S; base += PLAN_THREADS) {
        const int s = base + tid;
        int v = 0;
        if (s < S && s >= lo && s < hi) {
            const int c = plan_clampi(counts[s], 0, K);
            for (int k = 0; k < c; ++k) v += plan_kept(scores, s, k, K, min_score) ? 1 : 0;
        }
        int incl = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int up = __shfl_up(incl, o, 64);
            if (lane >= o) incl += up;
        }
        if (lane == 63) wave_tot[wave] = incl;
        __syncthreads();
        int before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < PLAN_WAVES; ++w) {
            const int t = wave_tot[w];
            before += w < wave ? t : 0;
            all += t;
        }
        if (s < S) {
            const int excl = carry + before + incl - v;
            pr_off[s] = excl < P ? excl : P;
        }
        carry += all;
        __syncthreads();                                   // wave_tot is rewritten by the next pass
    }
    if (tid == 0) {
        pr_off[S] = carry < P ? carry : P;
        *total = carry;
    }
    __syncthreads();                                       // pr_off (global, written by this workgroup) is read below

    // ---- (b) one row per kept (frame, box) pair -----------------------------------------------------------------------------
    const int pairs = (hi - lo) * K;
    for (int i = tid; i < pairs; i += PLAN_THREADS) {
        const int s = lo + i / K, k = i - (i / K) * K;
        if (k >= plan_clampi(counts[s], 0, K) || !plan_kept(scores, s, k, K, min_score)) continue;
        int row = pr_off[s];
        for (int j = 0; j < k; ++j) row += plan_kept(scores, s, j, K, min_score) ? 1 : 0;
        if (row >= P) continue;

        // box -> center / scale (crop.box_to_center_scale on float64 boxes)
        const double* b = boxes + ((size_t)s * K + k) * 4;
        const double x = b[0], y = b[1], w = b[2], h = b[3];
        const float cx = (float)(x + w * 0.5), cy = (float)(y + h * 0.5);
        const double arh = ar * h;
        const double h2 = w > arh ? w / ar : h;
        const double w2 = w < arh ? h * ar : w;
        float sx = (float)(w2 / 200.0), sy = (float)(h2 / 200.0);
        if (cx != -1.0f) {                                 // the reference's quirk: center x == -1 is not enlarged
            sx = sx * enlarge;
            sy = sy * enlarge;
        }
        center[2 * row] = cx;
        center[2 * row + 1] = cy;
        scale[2 * row] = sx;
        scale[2 * row + 1] = sy;

        // crop matrix at rotation 0 (crop.crop_matrix): the three point pairs in float32, their affine map in float64.
        // src = (cx, cy), (cx, y1), (x2, y1) and dst = (u0, v0), (u0, v1), (u2, v1): an axis-parallel right angle each, so the
        // 6 x 6 system splits into  a = (u2 - u0) / (x2 - cx),  d = (v0 - v1) / (cy - y1),  b = c = 0  and the translation.
        const double p1 = (double)(sx * 200.0f) * -0.5;
        const float y1 = (float)((double)cy + p1);
        const float x2 = cx + -(cy - y1);
        const float u0 = out_w * 0.5f, v0 = out_h * 0.5f;
        const float v1 = v0 + out_w * -0.5f;
        const float u2 = u0 + -(v0 - v1);
        const double a = ((double)u2 - (double)u0) / ((double)x2 - (double)cx);
        const double d = ((double)v0 - (double)v1) / ((double)cy - (double)y1);
        double* m = M + (size_t)row * 6;
        m[0] = a;
        m[1] = 0.0;
        m[2] = (double)u0 - a * (double)cx;
        m[3] = 0.0;
        m[4] = d;
        m[5] = (double)v0 - d * (double)cy;

        // window (crop.window, distance 2): how many earlier / later frames the sequence has, capped at 2
        const int cur = frame_number[s], n = num_frames[s];
        const int lp = plan_clampi(pt18 ? cur : cur - 1, 0, 2);
        const int ln = plan_clampi(pt18 ? n - cur - 1 : n - cur, 0, 2);
        int left = lp >= 1 ? 1 : 0, right = ln >= 1 ? 1 : 0;
        const int lleft = lp >= 2 ? 2 : 0, rright = ln >= 2 ? 1 : 0;              // nnext is the SAME frame as next
        int sprev = plan_find(frame_number, num_frames, S, s, cur - left, -1);
        int snext = plan_find(frame_number, num_frames, S, s, cur + right, 1);
        if (sprev < 0) { sprev = s; left = 0; }                                   // not in the pool: the current frame
        if (snext < 0) { snext = s; right = 0; }
        int* fi = frame_idx + (size_t)row * 5;
        fi[0] = s;
        fi[1] = sprev;
        fi[2] = snext;
        fi[3] = plan_find(frame_number, num_frames, S, s, cur - lleft, -1);       // unchecked by the reference: -1 if absent
        fi[4] = plan_find(frame_number, num_frames, S, s, cur + rright, 1);
        float* mg = margin + (size_t)row * 4;
        mg[0] = (float)left;
        mg[1] = (float)right;
        mg[2] = (float)lleft;
        mg[3] = (float)rright;
        box_score[row] = (double)scores[(size_t)s * K + k];
        person_slot[row] = s;
    }

    // ---- (c) padding rows -----------------------------------------------------------------------------------------------------
    for (int row = (carry < P ? carry : P) + tid; row < P; row += PLAN_THREADS) {
        center[2 * row] = center[2 * row + 1] = 0.f;
        scale[2 * row] = scale[2 * row + 1] = 0.f;
        double* m = M + (size_t)row * 6;
        m[0] = 1.0; m[1] = 0.0; m[2] = 0.0;
        m[3] = 0.0; m[4] = 1.0; m[5] = 0.0;
        for (int f = 0; f < 5; ++f) frame_idx[(size_t)row * 5 + f] = -1;
        for (int f = 0; f < 4; ++f) margin[(size_t)row * 4 + f] = 0.f;
        box_score[row] = 0.0;
        person_slot[row] = -1;
    }
}

}  // namespace

extern "C" int otp_pose_plan(const void* boxes, const void* scores, const void* counts, const void* frame_number,
                             const void* num_frames, int S, int K, int detect_lo, int detect_hi, double min_score,
                             double aspect_ratio, double enlarge, int out_w, int out_h, int posetrack18, int max_persons,
                             void* center, void* scale, void* M, void* frame_idx, void* margin, void* box_score,
                             void* person_slot, void* pr_off, void* total, void* stream) {
    if (!counts || !frame_number || !num_frames || !pr_off || !total) return OTP_ERR_BAD_ARG;
    if (S <= 0 || K < 0 || max_persons < 0 || out_w <= 0 || out_h <= 0) return OTP_ERR_BAD_ARG;
    if (K > 0 && (!boxes || !scores)) return OTP_ERR_BAD_ARG;
    if (max_persons > 0 && (!center || !scale || !M || !frame_idx || !margin || !box_score || !person_slot)) return OTP_ERR_BAD_ARG;
    if (detect_lo < 0 || detect_hi > S || detect_lo > detect_hi) return OTP_ERR_BAD_ARG;
    if (!(aspect_ratio > 0) || !(enlarge > 0) || min_score != min_score) return OTP_ERR_BAD_ARG;
    if ((long long)S * (K > 0 ? K : 1) > 0x7fffffffLL || out_w > (1 << 23) || out_h > (1 << 23)) return OTP_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(pose_plan_kernel, dim3(1), dim3(PLAN_THREADS), 0, static_cast<hipStream_t>(stream),
                       static_cast<const double*>(boxes), static_cast<const float*>(scores), static_cast<const int*>(counts),
                       static_cast<const int*>(frame_number), static_cast<const int*>(num_frames), S, K, detect_lo, detect_hi,
                       min_score, aspect_ratio, (float)enlarge, (float)out_w, (float)out_h, posetrack18 ? 1 : 0, max_persons,
                       static_cast<float*>(center), static_cast<float*>(scale), static_cast<double*>(M),
                       static_cast<int*>(frame_idx), static_cast<float*>(margin), static_cast<double*>(box_score),
                       static_cast<int*>(person_slot), static_cast<int*>(pr_off), static_cast<int*>(total));
    return otp_launch_status();
}
