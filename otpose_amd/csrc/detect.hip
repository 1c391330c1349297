// Person detector (the reference's object_detector/YOLOv3): the four kernels around the Darknet convolutions, which themselves
// run on otp_conv2d with no activation and BatchNorm folded into scale / shift.
//   otp_letterbox_u8    uint8 frames -> the square network input: pad to a square with 127, area-average to S x S, round to a
//                       uint8 level, / 255 (detector_utils.py:12-38); one pass, the padded square is never materialised
//   otp_leaky_pass      LeakyReLU(0.1) of a conv's raw output, optional + shortcut, optional nearest 2x upsample, on channel
//                       slices (a [route] concat is a write offset)
//   otp_yolo_decode     one [yolo] layer's eval output (models.py:123-165) written into its rows of the prediction tensor
//   otp_box_nms_merge   confidence filter + the merging NMS (detector_utils.py:253-291) + the rescale to frame pixels
//                       (detector_yolov3.py:79-98), one workgroup per image on a global workspace sized by N
// Plain C++: no inline assembly, no float atomics, every sum in a fixed order - the same input gives the same bytes.
// DESIGN.md section 3.12.
#include "common.h"

// every product, quotient and sum rounded on its own, as torch's element-wise float32 operations are (tests/detector_ref.py)
#pragma clang fp contract(off)

namespace {

// ---- letterbox -------------------------------------------------------------------------------------------------------------
// Exact integer arithmetic.  With D = max(H, W) the padded square has D x D pixels and output pixel (oy, ox) is the mean of the
// source rectangle [ox D / S, (ox + 1) D / S) x [oy D / S, (oy + 1) D / S).  In units of 1 / S a source pixel is S wide and an
// output pixel D wide, so every coverage weight is an integer, the weights of a row sum to D, and
// level = round(sum(wy wx v) / D^2) is one 64-bit division (a tie rounds up).
constexpr int kPadLevel = 127;                       // np.pad(uint8 image, 127.5) stores 127

__global__ __launch_bounds__(256) void letterbox_kernel(const unsigned char* __restrict__ frames, float* __restrict__ out,
                                                        int B, int H, int W, int S, int D, int pad_y, int pad_x) {
    const int ox = blockIdx.x * 64 + (threadIdx.x & 63), oy = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (ox >= S || oy >= S) return;
    const int ya = oy * D, yb = ya + D, xa = ox * D, xb = xa + D;
    const int y0 = ya / S, y1 = (yb + S - 1) / S, x0 = xa / S, x1 = (xb + S - 1) / S;      // source rows / columns [y0, y1) x [x0, x1)
    for (int b = blockIdx.z; b < B; b += gridDim.z) {
        const unsigned char* img = frames + (size_t)b * H * W * 3;
        unsigned long long acc[3] = {0ull, 0ull, 0ull};
        for (int y = y0; y < y1; ++y) {
            const int lo = y * S > ya ? y * S : ya, hi = (y + 1) * S < yb ? (y + 1) * S : yb;
            const unsigned wy = (unsigned)(hi - lo);
            const int fy = y - pad_y;
            unsigned row[3] = {0u, 0u, 0u};
            if (fy < 0 || fy >= H) {
                row[0] = row[1] = row[2] = (unsigned)D * kPadLevel;
            } else {
                const unsigned char* line = img + (size_t)fy * W * 3;
                for (int x = x0; x < x1; ++x) {
                    const int l = x * S > xa ? x * S : xa, h = (x + 1) * S < xb ? (x + 1) * S : xb;
                    const unsigned wx = (unsigned)(h - l);
                    const int fx = x - pad_x;
                    if (fx < 0 || fx >= W) {
                        row[0] += wx * kPadLevel; row[1] += wx * kPadLevel; row[2] += wx * kPadLevel;
                    } else {
                        const unsigned char* px = line + (size_t)fx * 3;
                        row[0] += wx * px[0]; row[1] += wx * px[1]; row[2] += wx * px[2];
                    }
                }
            }
            acc[0] += (unsigned long long)wy * row[0];
            acc[1] += (unsigned long long)wy * row[1];
            acc[2] += (unsigned long long)wy * row[2];
        }
        const unsigned long long d2 = (unsigned long long)D * D;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const unsigned level = (unsigned)((2ull * acc[c] + d2) / (2ull * d2));
            out[(((size_t)b * 3 + c) * S + oy) * S + ox] = (float)level / 255.0f;        // torch: uint8 -> float, / 255.0
        }
    }
}

// ---- activation pass ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float leaky(float x, int on) { return (on && !(x > 0.f)) ? 0.1f * x : x; }

struct PassArgs {
    int NC, C, H, W, leaky, up;
    int in_ctot, in_coff, sc_ctot, sc_coff, out_ctot, out_coff;
};

// VEC = 4: W % 4 == 0 and 16-byte aligned bases, an item is four pixels of a row; VEC = 1: an item is a pixel.
// grid.x walks the items of a plane, grid.y the (n, c) planes.
template <int VEC>
__global__ __launch_bounds__(256) void leaky_pass_kernel(const float* __restrict__ in, const float* __restrict__ sc,
                                                         float* __restrict__ out, PassArgs a) {
    const int HW = a.H * a.W, items = HW / VEC, f = a.up, Wo = a.W * f;
    for (int p = blockIdx.y; p < a.NC; p += gridDim.y) {
        const int n = p / a.C, c = p - n * a.C;
        const float* ip = in + ((size_t)n * a.in_ctot + a.in_coff + c) * HW;
        const float* sp = sc ? sc + ((size_t)n * a.sc_ctot + a.sc_coff + c) * HW : nullptr;
        float* op = out + ((size_t)n * a.out_ctot + a.out_coff + c) * HW * f * f;
        for (int i = blockIdx.x * 256 + threadIdx.x; i < items; i += gridDim.x * 256) {
            float v[VEC];
            if constexpr (VEC == 4) {
                const otp_f32x4 x = *reinterpret_cast<const otp_f32x4*>(ip + (size_t)i * 4);
                v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
            } else {
                v[0] = ip[i];
            }
#pragma unroll
            for (int k = 0; k < VEC; ++k) v[k] = leaky(v[k], a.leaky);
            if (sp) {
                if constexpr (VEC == 4) {
                    const otp_f32x4 s = *reinterpret_cast<const otp_f32x4*>(sp + (size_t)i * 4);
                    v[0] = v[0] + s.x; v[1] = v[1] + s.y; v[2] = v[2] + s.z; v[3] = v[3] + s.w;
                } else {
                    v[0] = v[0] + sp[i];
                }
            }
            if (f == 1) {
                if constexpr (VEC == 4) *reinterpret_cast<otp_f32x4*>(op + (size_t)i * 4) = otp_f32x4{v[0], v[1], v[2], v[3]};
                else op[i] = v[0];
            } else {                                              // f == 2 (the host refuses anything else)
                const int pix = i * VEC, y = pix / a.W, x = pix - y * a.W;
                float* o0 = op + (size_t)(2 * y) * Wo + 2 * x;
                if constexpr (VEC == 4) {
                    const otp_f32x4 lo{v[0], v[0], v[1], v[1]}, hi{v[2], v[2], v[3], v[3]};
                    *reinterpret_cast<otp_f32x4*>(o0) = lo;
                    *reinterpret_cast<otp_f32x4*>(o0 + 4) = hi;
                    *reinterpret_cast<otp_f32x4*>(o0 + Wo) = lo;
                    *reinterpret_cast<otp_f32x4*>(o0 + Wo + 4) = hi;
                } else {
                    o0[0] = v[0]; o0[1] = v[0]; o0[Wo] = v[0]; o0[Wo + 1] = v[0];
                }
            }
        }
    }
}

// ---- head decode -----------------------------------------------------------------------------------------------------------------
constexpr int kMaxAnchors = OTP_YOLO_MAX_ANCHORS;
struct Anchors { float w[kMaxAnchors], h[kMaxAnchors]; };           // a / stride, rounded to fp32 as FloatTensor(...) does

__device__ __forceinline__ float sigmoidf(float x) { return 1.f / (1.f + expf(-x)); }

// One workgroup per 64 cells of one (image, anchor): lanes read a channel plane along the cells (coalesced), the values turn
// in LDS, and the 64 rows leave as one contiguous run of 64 * K floats.  tile pitch K | 1: odd, so a column read is conflict free.
__global__ __launch_bounds__(256) void yolo_decode_kernel(const float* __restrict__ in, float* __restrict__ pred, Anchors an,
                                                          int A, int K, int G, float stride, int N, int row_off) {
    extern __shared__ float tile[];
    const int GG = G * G, pitch = K | 1;
    const int cell0 = blockIdx.x * 64, a = blockIdx.y, b = blockIdx.z, t = threadIdx.x;
    const int ncell = GG - cell0 < 64 ? GG - cell0 : 64;
    const float* src = in + ((size_t)b * A + a) * K * GG;
    const int lane = t & 63;
    if (lane < ncell) {
        const int cell = cell0 + lane, gy = cell / G, gx = cell - gy * G;
        for (int k = t >> 6; k < K; k += 4) {
            const float x = src[(size_t)k * GG + cell];
            float v;
            if (k == 0) v = (sigmoidf(x) + (float)gx) * stride;
            else if (k == 1) v = (sigmoidf(x) + (float)gy) * stride;
            else if (k == 2) v = (expf(x) * an.w[a]) * stride;
            else if (k == 3) v = (expf(x) * an.h[a]) * stride;
            else v = sigmoidf(x);
            tile[lane * pitch + k] = v;
        }
    }
    __syncthreads();
    float* dst = pred + ((size_t)b * N + row_off + (size_t)a * GG + cell0) * K;
    for (int e = t; e < ncell * K; e += 256) {
        const int r = e / K, k = e - r * K;
        dst[e] = tile[r * pitch + k];
    }
}

// ---- filter + merging NMS ----------------------------------------------------------------------------------------------------
constexpr int kNmsThreads = 1024, kNmsWaves = kNmsThreads / 64;
constexpr int kWsWords = OTP_BOX_NMS_WS_WORDS;       // workspace words per prediction row (below)

struct Frame { double pad_x2, pad_y2, unpad_w, unpad_h, w, h; };    // detector_yolov3.py:79-93, evaluated by the caller in float64

// Workspace of image b, N words each: cand | score | cls | x1 y1 x2 y2 conf (candidate order) | x1 y1 x2 y2 conf cls alive
// (score order).
__global__ __launch_bounds__(kNmsThreads) void box_nms_merge_kernel(
    const float* __restrict__ pred, int N, int K, float conf_thres, float nms_thres, int person_class, Frame fr, int max_out,
    int* __restrict__ ws_all, int* __restrict__ counts, float* __restrict__ dets, int* __restrict__ person_counts,
    double* __restrict__ person_boxes, float* __restrict__ person_scores) {
    __shared__ int s_cnt[kNmsWaves];
    __shared__ float s_red[kNmsWaves][5];
    const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const float* P = pred + (size_t)b * N * K;
    int* ws = ws_all + (size_t)b * kWsWords * N;
    int* cand = ws;
    float* score = reinterpret_cast<float*>(ws + (size_t)N);
    int* cls = ws + (size_t)2 * N;
    float* ubox = reinterpret_cast<float*>(ws + (size_t)3 * N);       // 5 planes: x1 y1 x2 y2 conf
    float* sbox = reinterpret_cast<float*>(ws + (size_t)8 * N);       // 5 planes, score order
    int* scls = ws + (size_t)13 * N;
    int* alive = ws + (size_t)14 * N;
    float* D = dets + (size_t)b * max_out * 6;
    double* PB = person_boxes + (size_t)b * max_out * 4;
    float* PS = person_scores + (size_t)b * max_out;

    // ---- 1. rows with conf >= conf_thres, in row order --------------------------------------------------------------------
    int M = 0;
    for (int base = 0; base < N; base += kNmsThreads) {
        const int r = base + t;
        const bool flag = r < N && P[(size_t)r * K + 4] >= conf_thres;
        const unsigned long long mask = __ballot(flag);
        if (lane == 0) s_cnt[wave] = __popcll(mask);
        __syncthreads();
        int off = M, total = 0;
        for (int w = 0; w < kNmsWaves; ++w) {
            if (w < wave) off += s_cnt[w];
            total += s_cnt[w];
        }
        if (flag) cand[off + __popcll(mask & ((1ull << lane) - 1ull))] = r;
        M += total;
        __syncthreads();
    }

    // ---- 2. score = conf * max(cls), class = first arg-max, corners -------------------------------------------------------
    for (int m = t; m < M; m += kNmsThreads) {
        const float* row = P + (size_t)cand[m] * K;
        float best = row[5];
        int bi = 0;
        for (int k = 1; k < K - 5; ++k) {
            const float v = row[5 + k];
            if (v > best) { best = v; bi = k; }
        }
        const float conf = row[4], s = conf * best;
        score[m] = s == s ? s : -INFINITY;                          // a NaN sorts last: the order stays total
        cls[m] = bi;
        const float cx = row[0], cy = row[1], hw = row[2] / 2, hh = row[3] / 2;
        ubox[m] = cx - hw;
        ubox[(size_t)N + m] = cy - hh;
        ubox[(size_t)2 * N + m] = cx + hw;
        ubox[(size_t)3 * N + m] = cy + hh;
        ubox[(size_t)4 * N + m] = conf;
    }
    __syncthreads();

    // ---- 3. rank by counting: descending score, a tie to the lower row ----------------------------------------------------
    for (int m = t; m < M; m += kNmsThreads) {
        const float s = score[m];
        int rank = 0;
        for (int o = 0; o < M; ++o) {
            const float so = score[o];
            rank += (so > s || (so == s && o < m)) ? 1 : 0;
        }
#pragma unroll
        for (int j = 0; j < 5; ++j) sbox[(size_t)j * N + rank] = ubox[(size_t)j * N + m];
        scls[rank] = cls[m];
        alive[rank] = 1;
    }
    __syncthreads();

    // ---- 4. the reference's loop: the first live row takes every live row of its class with IoU > nms_thres (itself too)
    // and becomes their conf-weighted mean box ---------------------------------------------------------------------------------
    int head = 0, kept = 0, persons = 0;
    for (;;) {
        while (head < M && !alive[head]) ++head;
        if (head >= M) break;
        __syncthreads();                                            // every thread has found the head before anyone clears it
        const float hx1 = sbox[head], hy1 = sbox[(size_t)N + head], hx2 = sbox[(size_t)2 * N + head],
                    hy2 = sbox[(size_t)3 * N + head], hconf = sbox[(size_t)4 * N + head];
        const int hcls = scls[head];
        const float harea = (hx2 - hx1 + 1.f) * (hy2 - hy1 + 1.f);
        float acc[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
        for (int p = head + t; p < M; p += kNmsThreads) {
            if (!alive[p]) continue;
            const float x1 = sbox[p], y1 = sbox[(size_t)N + p], x2 = sbox[(size_t)2 * N + p], y2 = sbox[(size_t)3 * N + p];
            const float iw = fmaxf(fminf(hx2, x2) - fmaxf(hx1, x1) + 1.f, 0.f);
            const float ih = fmaxf(fminf(hy2, y2) - fmaxf(hy1, y1) + 1.f, 0.f);
            const float inter = iw * ih, area = (x2 - x1 + 1.f) * (y2 - y1 + 1.f);
            const float iou = inter / (harea + area - inter + 1e-16f);
            // the head always leaves (its IoU with itself is 1); forced, so that a non-finite box cannot stall the loop
            if (p == head || (iou > nms_thres && scls[p] == hcls)) {
                alive[p] = 0;
                const float w = sbox[(size_t)4 * N + p];
                acc[0] = acc[0] + w * x1;
                acc[1] = acc[1] + w * y1;
                acc[2] = acc[2] + w * x2;
                acc[3] = acc[3] + w * y2;
                acc[4] = acc[4] + w;
            }
        }
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            float v = acc[j];
            for (int o = 32; o > 0; o >>= 1) v = v + __shfl_xor(v, o, 64);
            acc[j] = v;
        }
        if (lane == 0)
            for (int j = 0; j < 5; ++j) s_red[wave][j] = acc[j];
        __syncthreads();                                            // also orders the alive[] stores before the next scan
        if (t == 0) {
            float tot[5];
            for (int j = 0; j < 5; ++j) {
                float v = s_red[0][j];
                for (int w = 1; w < kNmsWaves; ++w) v = v + s_red[w][j];
                tot[j] = v;
            }
            const float mx1 = tot[0] / tot[4], my1 = tot[1] / tot[4], mx2 = tot[2] / tot[4], my2 = tot[3] / tot[4];
            if (kept < max_out) {
                float* d = D + (size_t)kept * 6;
                d[0] = mx1; d[1] = my1; d[2] = mx2; d[3] = my2; d[4] = hconf; d[5] = (float)hcls;
                if (hcls == person_class) {
                    const double x1 = mx1, y1 = my1, x2 = mx2, y2 = my2;
                    double* q = PB + (size_t)persons * 4;
                    q[0] = ((x1 - fr.pad_x2) / fr.unpad_w) * fr.w;
                    q[1] = ((y1 - fr.pad_y2) / fr.unpad_h) * fr.h;
                    q[2] = ((x2 - x1) / fr.unpad_w) * fr.w;
                    q[3] = ((y2 - y1) / fr.unpad_h) * fr.h;
                    PS[persons] = hconf;
                }
            }
        }
        if (kept < max_out && hcls == person_class) ++persons;
        ++kept;
        ++head;
        __syncthreads();                                            // s_red is free again
    }
    if (kept > max_out) kept = max_out;
    if (t == 0) {
        counts[b] = kept;
        person_counts[b] = persons;
    }
    // rows past the counts hold zeros, whatever an earlier call left there
    for (int e = kept * 6 + t; e < max_out * 6; e += kNmsThreads) D[e] = 0.f;
    for (int e = persons * 4 + t; e < max_out * 4; e += kNmsThreads) PB[e] = 0.0;
    for (int e = persons + t; e < max_out; e += kNmsThreads) PS[e] = 0.f;
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" int otp_letterbox_u8(const void* frames_u8, void* out, int B, int H, int W, int S, void* stream) {
    if (!frames_u8 || !out || B <= 0 || H <= 0 || W <= 0 || S <= 0) return OTP_ERR_BAD_ARG;
    const int D = H > W ? H : W;
    if (D < S || D > 16384 || S > 4096) return OTP_ERR_UNSUPPORTED;  // D < S: no longer an area average; the rest: 32-bit weights
    const int diff = H > W ? H - W : W - H, pad1 = diff / 2;
    const int pad_y = H <= W ? pad1 : 0, pad_x = H <= W ? 0 : pad1;
    dim3 grid(otp_ceil_div(S, 64), otp_ceil_div(S, 4), B < 1024 ? B : 1024);
    hipLaunchKernelGGL(letterbox_kernel, grid, dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const unsigned char*>(frames_u8), static_cast<float*>(out), B, H, W, S, D, pad_y, pad_x);
    return otp_launch_status();
}

extern "C" int otp_leaky_pass(const void* in, const void* shortcut, void* out, int N, int C, int H, int W, int leaky, int up,
                              int in_ctot, int in_coff, int sc_ctot, int sc_coff, int out_ctot, int out_coff, void* stream) {
    if (!in || !out || N <= 0 || C <= 0 || H <= 0 || W <= 0) return OTP_ERR_BAD_ARG;
    if (in_coff < 0 || in_coff + C > in_ctot || out_coff < 0 || out_coff + C > out_ctot) return OTP_ERR_BAD_ARG;
    if (shortcut && (sc_coff < 0 || sc_coff + C > sc_ctot)) return OTP_ERR_BAD_ARG;
    if (up != 1 && up != 2) return OTP_ERR_UNSUPPORTED;
    if ((long)H * W * up * up >= (1l << 30) || (long)N * C >= (1l << 30)) return OTP_ERR_UNSUPPORTED;
    PassArgs a{N * C, C, H, W, leaky ? 1 : 0, up, in_ctot, in_coff, sc_ctot, sc_coff, out_ctot, out_coff};
    const bool vec = (W & 3) == 0 && aligned16(in) && aligned16(out) && (!shortcut || aligned16(shortcut));
    const int items = H * W / (vec ? 4 : 1);
    int gx = otp_ceil_div(items, 256);
    if (gx > 64) gx = 64;
    dim3 grid(gx, a.NC < 32768 ? a.NC : 32768);
    auto st = static_cast<hipStream_t>(stream);
    if (vec)
        hipLaunchKernelGGL(leaky_pass_kernel<4>, grid, dim3(256), 0, st, static_cast<const float*>(in),
                           static_cast<const float*>(shortcut), static_cast<float*>(out), a);
    else
        hipLaunchKernelGGL(leaky_pass_kernel<1>, grid, dim3(256), 0, st, static_cast<const float*>(in),
                           static_cast<const float*>(shortcut), static_cast<float*>(out), a);
    return otp_launch_status();
}

extern "C" int otp_yolo_decode(const void* in, void* pred, const double* anchors, int B, int A, int C, int G, int img_size,
                               int N, int row_off, void* stream) {
    if (!in || !pred || !anchors || B <= 0 || A <= 0 || C <= 0 || G <= 0 || img_size <= 0 || N <= 0 || row_off < 0)
        return OTP_ERR_BAD_ARG;
    if ((long)row_off + (long)A * G * G > N) return OTP_ERR_BAD_ARG;
    const int K = 5 + C;
    const size_t lds = (size_t)64 * (K | 1) * sizeof(float);
    if (A > kMaxAnchors || lds > 64 * 1024 || B > 65535 || G > 4096) return OTP_ERR_UNSUPPORTED;
    const double stride = (double)img_size / (double)G;              // models.py:127, a float
    Anchors an{};
    for (int a = 0; a < A; ++a) {
        an.w[a] = (float)(anchors[2 * a] / stride);
        an.h[a] = (float)(anchors[2 * a + 1] / stride);
    }
    dim3 grid(otp_ceil_div(G * G, 64), A, B);
    hipLaunchKernelGGL(yolo_decode_kernel, grid, dim3(256), lds, static_cast<hipStream_t>(stream),
                       static_cast<const float*>(in), static_cast<float*>(pred), an, A, K, G, (float)stride, N, row_off);
    return otp_launch_status();
}

extern "C" size_t otp_box_nms_merge_workspace(int B, int N) {
    if (B <= 0 || N <= 0) return 0;
    return (size_t)B * kWsWords * (size_t)N * sizeof(int);
}

extern "C" int otp_box_nms_merge(const void* pred, int B, int N, int C, float conf_thres, float nms_thres, int person_class,
                                 double pad_x2, double pad_y2, double unpad_w, double unpad_h, double frame_w, double frame_h,
                                 int max_out, void* workspace, size_t workspace_bytes, void* counts, void* dets,
                                 void* person_counts, void* person_boxes, void* person_scores, void* stream) {
    if (!pred || !workspace || !counts || !dets || !person_counts || !person_boxes || !person_scores) return OTP_ERR_BAD_ARG;
    if (B <= 0 || N <= 0 || C <= 0 || max_out <= 0) return OTP_ERR_BAD_ARG;
    if (!(unpad_w != 0.0) || !(unpad_h != 0.0)) return OTP_ERR_BAD_ARG;
    if ((long)N * (5 + C) >= (1l << 31)) return OTP_ERR_UNSUPPORTED;
    if (workspace_bytes < otp_box_nms_merge_workspace(B, N)) return OTP_ERR_WORKSPACE;
    const Frame fr{pad_x2, pad_y2, unpad_w, unpad_h, frame_w, frame_h};
    hipLaunchKernelGGL(box_nms_merge_kernel, dim3(B), dim3(kNmsThreads), 0, static_cast<hipStream_t>(stream),
                       static_cast<const float*>(pred), N, 5 + C, conf_thres, nms_thres, person_class, fr, max_out,
                       static_cast<int*>(workspace), static_cast<int*>(counts), static_cast<float*>(dets),
                       static_cast<int*>(person_counts), static_cast<double*>(person_boxes),
                       static_cast<float*>(person_scores));
    return otp_launch_status();
}
