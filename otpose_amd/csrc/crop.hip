// Person crops straight from video frames (the step before the input assembly of glue.hip):
//   otp_crop_clips_u8 - the five cv2.warpAffine(frame, M, (W, H), INTER_LINEAR) of dataset/PoseTrackDataset.py:389-399
//                       per person, with ToTensor + Normalize + the channel concat of frames_u8_kernel fused behind them;
//   otp_pose_targets  - the joint transform, the visibility cut and generate_heatmaps of PoseTrackDataset.py:407-420 /
//                       utils/heatmap.py:48-105.
//   otp_crop_clips_blur_u8 - the same crops of frames first blurred per (sample, slot) as torchvision 0.8's
//                       T.GaussianBlur((5, 9)) blurs an (H, W, 3) uint8 tensor (PoseTrackDataset.py:374-388).
//   otp_crop_clips_pair_u8 - the plain crops and their exact column mirrors (the flip-test twin batch) in one pass.
// They restate integer / double arithmetic exactly (the contract is in include/otpose_hip.h), so their outputs are
// bit-identical to the host restatements in tests/crop_ref.py and tests/augment_ref.py.
#include "common.h"

namespace {

constexpr int kAB = 1024;           // AB_SCALE: 1 << AB_BITS (10)
constexpr int kRoundDelta = 16;     // AB_SCALE / INTER_TAB_SIZE / 2

// saturate_cast<int>(double): round half to even, clamp to int32 (NaN -> INT_MIN, as cvRound on x86)
__device__ __forceinline__ int sat_rint_i32(double v) {
    const double r = __builtin_rint(v);
    if (!(r == r)) return INT32_MIN;
    if (r >= 2147483647.0) return INT32_MAX;
    if (r <= -2147483648.0) return INT32_MIN;
    return (int)r;
}

__device__ __forceinline__ int sat_i16(int v) { return v < -32768 ? -32768 : (v > 32767 ? 32767 : v); }

// The two neighbouring RGB pixels at byte offset `off` (may be -3: column -1) of the pool as 6 bytes in the low 48 bits,
// a pixel outside its row zeroed.  One dword-aligned 12-byte load covers the 6 bytes at any offset; near the two ends
// of the pool, where those 12 bytes would leave it, the valid pixels are read byte by byte instead.
__device__ __forceinline__ uint64_t load_pair(const uint8_t* pool, size_t pool_bytes, long long off, bool inL, bool inR) {
    if (!inL && !inR) return 0;
    const uintptr_t base = reinterpret_cast<uintptr_t>(pool);
    const uintptr_t addr = base + (uintptr_t)off;
    const uintptr_t a4 = addr & ~(uintptr_t)3;
    uint64_t v = 0;
    if (off >= 0 && a4 >= base && a4 + 12 <= base + pool_bytes) {
        const uint32_t* q = reinterpret_cast<const uint32_t*>(pool + (a4 - base));   // (keeps the global address space)
        const uint32_t d0 = q[0], d1 = q[1], d2 = q[2];
        const int sh = (int)(addr - a4) * 8;
        v = ((uint64_t)d1 << 32 | d0) >> sh;
        if (sh) v |= (uint64_t)d2 << (64 - sh);
    } else {
        const uint8_t* p = pool + off;
        if (inL) v = (uint64_t)p[0] | (uint64_t)p[1] << 8 | (uint64_t)p[2] << 16;
        if (inR) v |= (uint64_t)p[3] << 24 | (uint64_t)p[4] << 32 | (uint64_t)p[5] << 40;
    }
    if (!inL) v &= ~(uint64_t)0xFFFFFF;
    if (!inR) v &= ~((uint64_t)0xFFFFFF << 24);
    return v;
}

// The blurred bytes of the two pool columns cl, cl + 1 (memory order, as load_pair packs them) of one row that starts at
// byte offset `row`, for a table `tab` (9 x 5 float32, row i = image column offset i - 4, column j = RGB offset j - 2).
// torchvision 0.8 reads the (H, W, 3) frame as (C=H, H'=W, W'=3): every image row is blurred on its own, along the
// width with reflection at the frame's left / right edges and across the RGB axis reflected as [b,g,r,g,b,g,r].  Under
// `fl` the mirrored frame is blurred: the window is read right to left.  The 10 pixels (30 bytes) around the two
// columns come from one dword-aligned 36-byte load where the window lies inside the row and the pool, else pixel by
// pixel with the reflection (clamped for a corner outside the frame, whose value is dropped anyway).
// Arithmetic (fixed, restated by tests/augment_ref.py): per output byte acc = 0; for i in 0..8, for j in 0..4:
// acc = acc + tab[i][j] * px (float32, every product and sum rounded: no FMA); then rint (half to even), clamp [0, 255].
__device__ __forceinline__ uint64_t blur_pair(const uint8_t* pool, size_t pool_bytes, long long row, int Wp, int cl,
                                              bool fl, bool inL, bool inR, const float* __restrict__ tab) {
#pragma clang fp contract(off)
    if (!inL && !inR) return 0;
    float px[10][3];
    const uintptr_t base = reinterpret_cast<uintptr_t>(pool);
    const long long off = row + (long long)(cl - 4) * 3;
    const uintptr_t addr = base + (uintptr_t)off;
    const uintptr_t a4 = addr & ~(uintptr_t)3;
    if (cl - 4 >= 0 && cl + 5 <= Wp - 1 && a4 >= base && a4 + 36 <= base + pool_bytes) {
        const uint32_t* q = reinterpret_cast<const uint32_t*>(pool + (a4 - base));
        uint32_t d[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) d[k] = q[k];
        const uint32_t sh = (uint32_t)(addr - a4);
        uint32_t e[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) e[k] = __builtin_amdgcn_alignbyte(d[k + 1], d[k], sh);
#pragma unroll
        for (int t = 0; t < 10; ++t)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int n = 3 * t + c;
                px[t][c] = (float)((e[n >> 2] >> (8 * (n & 3))) & 255u);
            }
    } else {
#pragma unroll
        for (int t = 0; t < 10; ++t) {
            int col = cl - 4 + t;
            col = col < 0 ? -col : col;
            col = col > Wp - 1 ? 2 * (Wp - 1) - col : col;
            col = col < 0 ? 0 : (col > Wp - 1 ? Wp - 1 : col);
            const uint8_t* p = pool + row + (long long)col * 3;
            px[t][0] = (float)p[0];
            px[t][1] = (float)p[1];
            px[t][2] = (float)p[2];
        }
    }
    if (fl) {
#pragma unroll
        for (int t = 0; t < 5; ++t)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float v = px[t][c];
                px[t][c] = px[9 - t][c];
                px[9 - t][c] = v;
            }
    }
    // a[c]: the column whose taps are px[i] (cl, or cl + 1 under flip); b[c]: px[i + 1]
    float a[3] = {0.f, 0.f, 0.f}, bb[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < 9; ++i)
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            const float w = tab[i * 5 + j];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int k = c + j - 2;
                const int ch = k < 0 ? -k : (k > 2 ? 4 - k : k);
                a[c] = a[c] + w * px[i][ch];
                bb[c] = bb[c] + w * px[i + 1][ch];
            }
        }
    uint64_t lo = 0, hi = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const uint64_t va = (uint32_t)fminf(fmaxf(__builtin_rintf(a[c]), 0.f), 255.f);
        const uint64_t vb = (uint32_t)fminf(fmaxf(__builtin_rintf(bb[c]), 0.f), 255.f);
        lo |= (fl ? vb : va) << (8 * c);
        hi |= (fl ? va : vb) << (8 * c);
    }
    return (inL ? lo : 0) | (inR ? hi << 24 : 0);
}

// One thread per output pixel (b, y, x) of one sample: the fixed-point source position is the same for all F frames of
// the sample, so it is computed once and the F gathers reuse it.  Writes: 3F coalesced float rows along x.
// BLUR: slot (b, f) with blur_on[b, f] != 0 (or blur_on NULL) reads its corner bytes through blur_pair with the table
// blur[b, f]; the other slots read the pool as the plain kernel does.
// PAIR: no flip; every value of sample b (of gridDim.y) is also stored at column W - 1 - x of sample gridDim.y + b, so the
// position work and the gathers of the mirrored twin are shared (the second store stream runs right to left per wave).
template <bool BLUR, bool PAIR>
__global__ __launch_bounds__(256) void crop_clips_kernel(const uint8_t* __restrict__ pool, int S, int Hp, int Wp,
                                                         const int* __restrict__ frame_idx, const double* __restrict__ Ms,
                                                         const uint8_t* __restrict__ flip, float* __restrict__ out, int F,
                                                         int H, int W, float m0, float m1, float m2, float s0, float s1,
                                                         float s2, const float* __restrict__ blur,
                                                         const uint8_t* __restrict__ blur_on) {
#pragma clang fp contract(off)
    const int b = blockIdx.y;
    const int HW = H * W;
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= HW) return;
    const int y = p / W, x = p - y * W;

    // inverse of the forward matrix, as warpAffine does without WARP_INVERSE_MAP (every product / sum rounded once)
    const double* M = Ms + (size_t)b * 6;
    double D = M[0] * M[4] - M[1] * M[3];
    D = D != 0.0 ? 1.0 / D : 0.0;
    const double A0 = M[4] * D, A1 = M[1] * -D, A3 = M[3] * -D, A4 = M[0] * D;
    const double A2 = -A0 * M[2] - A1 * M[5], A5 = -A3 * M[2] - A4 * M[5];

    // WarpAffineInvoker: row origin + column delta in 1/1024 px, then >> 5 to 1/32 px (int32, wrapping like the C code)
    const int X0 = (int)((unsigned)sat_rint_i32((A1 * y + A2) * kAB) + kRoundDelta);
    const int Y0 = (int)((unsigned)sat_rint_i32((A4 * y + A5) * kAB) + kRoundDelta);
    const int X = (int)((unsigned)X0 + (unsigned)sat_rint_i32(A0 * x * kAB)) >> 5;
    const int Y = (int)((unsigned)Y0 + (unsigned)sat_rint_i32(A3 * x * kAB)) >> 5;
    const int sx = sat_i16(X >> 5), sy = sat_i16(Y >> 5);
    const int ax = X & 31, ay = Y & 31;
    const int w00 = (32 - ax) * (32 - ay) * 32, w01 = ax * (32 - ay) * 32;
    const int w10 = (32 - ax) * ay * 32, w11 = ax * ay * 32;

    // remapBilinear, BORDER_CONSTANT 0: a corner outside the frame contributes nothing.  In memory the two columns
    // of a corner row are cl, cl + 1; flip reads column Wp - 1 - c, which swaps them.
    const bool fl = !PAIR && flip != nullptr && flip[b] != 0;
    const int cl = fl ? Wp - 2 - sx : sx;
    const bool inL = cl >= 0 && cl < Wp, inR = cl + 1 >= 0 && cl + 1 < Wp;
    const bool in_r0 = sy >= 0 && sy < Hp, in_r1 = sy + 1 >= 0 && sy + 1 < Hp;
    const int sh0 = fl ? 24 : 0, sh1 = fl ? 0 : 24;          // bit offset of corner column c0 / c1 in a loaded pair
    const size_t pool_bytes = (size_t)S * Hp * Wp * 3;

    float* o = out + (size_t)b * 3 * F * HW + p;
    float* om = PAIR ? out + (size_t)(gridDim.y + b) * 3 * F * HW + (size_t)y * W + (W - 1 - x) : nullptr;
    for (int f = 0; f < F; ++f) {
        const int fi = frame_idx[(size_t)b * F + f];
        const bool fr = fi >= 0 && fi < S;
        const long long off0 = (((long long)fi * Hp + sy) * Wp + cl) * 3;
        uint64_t q0, q1;
        if (BLUR && (blur_on == nullptr || blur_on[(size_t)b * F + f] != 0)) {
            const float* tab = blur + ((size_t)b * F + f) * 45;
            const long long row0 = ((long long)fi * Hp + sy) * Wp * 3;
            q0 = fr && in_r0 ? blur_pair(pool, pool_bytes, row0, Wp, cl, fl, inL, inR, tab) : 0;
            q1 = fr && in_r1 ? blur_pair(pool, pool_bytes, row0 + (long long)Wp * 3, Wp, cl, fl, inL, inR, tab) : 0;
        } else {
            q0 = fr && in_r0 ? load_pair(pool, pool_bytes, off0, inL, inR) : 0;
            q1 = fr && in_r1 ? load_pair(pool, pool_bytes, off0 + (long long)Wp * 3, inL, inR) : 0;
        }
        float v[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int p00 = (int)(q0 >> (sh0 + 8 * c)) & 255, p01 = (int)(q0 >> (sh1 + 8 * c)) & 255;
            const int p10 = (int)(q1 >> (sh0 + 8 * c)) & 255, p11 = (int)(q1 >> (sh1 + 8 * c)) & 255;
            v[c] = (float)((p00 * w00 + p01 * w01 + p10 * w10 + p11 * w11 + (1 << 14)) >> 15);
        }
        // ToTensor + Normalize: the float32 operation order of frames_u8_kernel (glue.hip)
        o[0] = (v[0] / 255.f - m0) / s0;
        o[(size_t)HW] = (v[1] / 255.f - m1) / s1;
        o[(size_t)2 * HW] = (v[2] / 255.f - m2) / s2;
        o += (size_t)3 * HW;
        if (PAIR) {                                           // (the same expressions: computed once)
            om[0] = (v[0] / 255.f - m0) / s0;
            om[(size_t)HW] = (v[1] / 255.f - m1) / s1;
            om[(size_t)2 * HW] = (v[2] / 255.f - m2) / s2;
            om += (size_t)3 * HW;
        }
    }
}

// generate_heatmaps per (sample, joint) plane: one block per plane, every thread derives the joint's patch (a few double
// operations) and writes its share of the plane; thread 0 writes the weight.
__global__ __launch_bounds__(256) void pose_targets_kernel(const double* __restrict__ joints, const float* __restrict__ vis,
                                                           const double* __restrict__ Ms, const float* __restrict__ gauss,
                                                           float* __restrict__ target, float* __restrict__ weight, int J,
                                                           int W, int H, int w, int h, int t3) {
#pragma clang fp contract(off)
    const int bj = blockIdx.x, b = bj / J;
    const double* M = Ms + (size_t)b * 6;
    const double jx = joints[(size_t)bj * 2], jy = joints[(size_t)bj * 2 + 1];
    float v = vis[bj];
    // exec_affine_transform, applied to joints with vis > 0 only (PoseTrackDataset.py:403-405); products and sums in the
    // plain left-to-right order (numpy's dot may sum through BLAS in another order: last-bit differences)
    const bool moved = v > 0.f;
    const double x = moved ? M[0] * jx + M[1] * jy + M[2] : jx;
    const double y = moved ? M[3] * jx + M[4] * jy + M[5] : jy;
    if (x < 0.0 || y < 0.0 || x > (double)W || y > (double)H) v = 0.f;       // PoseTrackDataset.py:408-414
    // mu = int(p / feat_stride + 0.5): truncation towards zero (clamped: int() of a huge double has no int32 value)
    const double fx = x / ((double)W / (double)w) + 0.5, fy = y / ((double)H / (double)h) + 0.5;
    const double lim = 1 << 28;
    const int mux = (int)(fx > lim ? lim : (fx < -lim ? -lim : (fx == fx ? fx : 0.0)));
    const int muy = (int)(fy > lim ? lim : (fy < -lim ? -lim : (fy == fy ? fy : 0.0)));
    const int ulx = mux - t3, uly = muy - t3, brx = mux + t3 + 1, bry = muy + t3 + 1;
    if (ulx >= w || uly >= h || brx < 0 || bry < 0) v = 0.f;
    const bool draw = v > 0.5f;
    const int size = 2 * t3 + 1;
    float* t = target + (size_t)bj * h * w;
    for (int i = threadIdx.x; i < h * w; i += blockDim.x) {
        const int yy = i / w, xx = i - yy * w;
        const int gx = xx - ulx, gy = yy - uly;
        const bool in = draw && gx >= 0 && gx < size && gy >= 0 && gy < size;
        t[i] = in ? gauss[gy * size + gx] : 0.f;
    }
    if (threadIdx.x == 0) weight[bj] = v;
}

}  // namespace

extern "C" int otp_crop_clips_u8(const void* pool_u8, int S, int Hp, int Wp, const void* frame_idx, const void* M,
                                 const void* flip, void* out, int B, int F, int H, int W, float mean_r, float mean_g,
                                 float mean_b, float std_r, float std_g, float std_b, void* stream) {
    if (!pool_u8 || !frame_idx || !M || !out) return OTP_ERR_BAD_ARG;
    if (S <= 0 || Hp <= 0 || Wp <= 0 || B <= 0 || F <= 0 || H <= 0 || W <= 0) return OTP_ERR_BAD_ARG;
    if (Hp > 32767 || Wp > 32767 || std_r == 0.f || std_g == 0.f || std_b == 0.f) return OTP_ERR_UNSUPPORTED;
    if ((long long)H * W > INT32_MAX / 4 || B > 65535) return OTP_ERR_UNSUPPORTED;
    const unsigned blocks = (unsigned)otp_ceil_div(H * W, 256);
    hipLaunchKernelGGL((crop_clips_kernel<false, false>), dim3(blocks, B), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const uint8_t*>(pool_u8), S, Hp, Wp, static_cast<const int*>(frame_idx),
                       static_cast<const double*>(M), static_cast<const uint8_t*>(flip), static_cast<float*>(out), F, H, W,
                       mean_r, mean_g, mean_b, std_r, std_g, std_b, nullptr, nullptr);
    return otp_launch_status();
}

extern "C" int otp_crop_clips_blur_u8(const void* pool_u8, int S, int Hp, int Wp, const void* frame_idx, const void* M,
                                      const void* flip, void* out, int B, int F, int H, int W, float mean_r, float mean_g,
                                      float mean_b, float std_r, float std_g, float std_b, const void* blur,
                                      const void* blur_on, void* stream) {
    if (!pool_u8 || !frame_idx || !M || !out || !blur) return OTP_ERR_BAD_ARG;
    if (S <= 0 || Hp <= 0 || Wp <= 0 || B <= 0 || F <= 0 || H <= 0 || W <= 0) return OTP_ERR_BAD_ARG;
    if (Hp > 32767 || Wp > 32767 || std_r == 0.f || std_g == 0.f || std_b == 0.f) return OTP_ERR_UNSUPPORTED;
    if ((long long)H * W > INT32_MAX / 4 || B > 65535) return OTP_ERR_UNSUPPORTED;
    if (Wp < 5) return OTP_ERR_UNSUPPORTED;          // the width reflection by 4 needs 5 columns (as torch's reflect pad)
    const unsigned blocks = (unsigned)otp_ceil_div(H * W, 256);
    hipLaunchKernelGGL((crop_clips_kernel<true, false>), dim3(blocks, B), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const uint8_t*>(pool_u8), S, Hp, Wp, static_cast<const int*>(frame_idx),
                       static_cast<const double*>(M), static_cast<const uint8_t*>(flip), static_cast<float*>(out), F, H, W,
                       mean_r, mean_g, mean_b, std_r, std_g, std_b, static_cast<const float*>(blur),
                       static_cast<const uint8_t*>(blur_on));
    return otp_launch_status();
}

extern "C" int otp_crop_clips_pair_u8(const void* pool_u8, int S, int Hp, int Wp, const void* frame_idx, const void* M,
                                      void* out, int B, int F, int H, int W, float mean_r, float mean_g, float mean_b,
                                      float std_r, float std_g, float std_b, void* stream) {
    if (!pool_u8 || !frame_idx || !M || !out) return OTP_ERR_BAD_ARG;
    if (S <= 0 || Hp <= 0 || Wp <= 0 || B <= 0 || F <= 0 || H <= 0 || W <= 0) return OTP_ERR_BAD_ARG;
    if (Hp > 32767 || Wp > 32767 || std_r == 0.f || std_g == 0.f || std_b == 0.f) return OTP_ERR_UNSUPPORTED;
    if ((long long)H * W > INT32_MAX / 4 || B > 65535) return OTP_ERR_UNSUPPORTED;
    const unsigned blocks = (unsigned)otp_ceil_div(H * W, 256);
    hipLaunchKernelGGL((crop_clips_kernel<false, true>), dim3(blocks, B), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const uint8_t*>(pool_u8), S, Hp, Wp, static_cast<const int*>(frame_idx),
                       static_cast<const double*>(M), nullptr, static_cast<float*>(out), F, H, W, mean_r, mean_g, mean_b,
                       std_r, std_g, std_b, nullptr, nullptr);
    return otp_launch_status();
}

extern "C" int otp_pose_targets(const void* joints, const void* vis, const void* M, const void* gauss, void* target,
                                void* target_weight, int B, int J, int W, int H, int w, int h, int sigma3, void* stream) {
    if (!joints || !vis || !M || !gauss || !target || !target_weight) return OTP_ERR_BAD_ARG;
    if (B <= 0 || J <= 0 || W <= 0 || H <= 0 || w <= 0 || h <= 0 || sigma3 < 0) return OTP_ERR_BAD_ARG;
    if ((long long)B * J > INT32_MAX || (long long)w * h > INT32_MAX || sigma3 > 4096) return OTP_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(pose_targets_kernel, dim3(B * J), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const double*>(joints), static_cast<const float*>(vis), static_cast<const double*>(M),
                       static_cast<const float*>(gauss), static_cast<float*>(target), static_cast<float*>(target_weight),
                       J, W, H, w, h, sigma3);
    return otp_launch_status();
}
