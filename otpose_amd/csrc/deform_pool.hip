// Deformable position-sensitive RoI pooling (include/otpose_hip.h: otp_deform_psroi_pool_*), the second native operator of the
// reference's thirdparty/deform_conv package (semantics: src/deform_pool_cuda_kernel.cu:20-253).  DESIGN.md section 3.11.
//
// Forward: one lane per output element (n, ctop, ph, pw), pw fastest, one workgroup row per RoI - neighbouring lanes take
//   neighbouring bins of one (n, ctop), so a wave's samples fall into a few rows of few channel planes, and the RoI header is
//   addressed by blockIdx alone (scalar loads, once per wave).  The offset pair of a bin is read once per element, not per sample.
// Backward: one wave per offset cell (n, class, part_h, part_w).  Its lanes walk the statically known set of (ctop, ph, pw, sample)
//   that feeds the cell in a fixed order:
//   * grad_offset: per-lane sums in that order, then a fixed xor tree over the wave, one plain read-modify-write per cell
//     (every cell has exactly one wave) - no atomics.
//   * grad_input: every contribution is rounded ONCE to a multiple of 2^(e-P) and added with 64-bit INTEGER atomics into a
//     workspace plane (integer addition is associative: the plane holds the same bits whatever the arrival order), where 2^e
//     bounds max|grad_out| (a max-reduction pre-pass; max is order-independent as well) and P = 62 - ceil(log2(most contributions a
//     cell can receive)).  A last pass converts the plane and adds it to the caller's grad_input once.
// Coordinates and bilinear weights are computed in the storage type, step by step as the reference writes them (no contraction:
// a fused multiply-add would move a sample by an ulp against the step-by-step result).  Sums are kept in double.
#include "common.h"

#include <math.h>

#pragma clang fp contract(off)

namespace {

struct Geo {
    int N, C, H, W, num_rois, no_trans, out_channels, G, pooled, part, spp, num_classes, cec;   // cec: channels of each class
};

// C round(): halves away from zero (not rint)
__device__ __forceinline__ float round_away(float v) { return roundf(v); }
__device__ __forceinline__ double round_away(double v) { return round(v); }

template <typename T>
struct Roi {
    int batch;          // -1: batch index outside [0, N) - the RoI pools nothing and receives no gradient
    T start_w, start_h, width, height, bin_w, bin_h, sub_w, sub_h;
};

template <typename T>
__device__ __forceinline__ Roi<T> load_roi(const T* __restrict__ rois, int n, T spatial_scale, const Geo& g) {
    const T* r = rois + (size_t)n * 5;
    Roi<T> o;
    const T b = r[0];
    o.batch = (b >= (T)0 && b < (T)g.N) ? (int)b : -1;
    o.start_w = round_away(r[1]) * spatial_scale - (T)0.5;
    o.start_h = round_away(r[2]) * spatial_scale - (T)0.5;
    const T end_w = (round_away(r[3]) + (T)1) * spatial_scale - (T)0.5;
    const T end_h = (round_away(r[4]) + (T)1) * spatial_scale - (T)0.5;
    o.width = fmax(end_w - o.start_w, (T)0.1);
    o.height = fmax(end_h - o.start_h, (T)0.1);
    o.bin_w = o.width / (T)g.pooled;
    o.bin_h = o.height / (T)g.pooled;
    o.sub_w = o.bin_w / (T)g.spp;
    o.sub_h = o.bin_h / (T)g.spp;
    return o;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// part index of a bin row / column: floor(p / pooled * part) in floating point (clamped for the sake of the address only)
template <typename T>
__device__ __forceinline__ int part_of(int p, const Geo& g) {
    return clampi((int)floor((T)p / (T)g.pooled * (T)g.part), 0, g.part - 1);
}
template <typename T>
__device__ __forceinline__ int group_of(int p, const Geo& g) {
    return clampi((int)floor((T)p * (T)g.G / (T)g.pooled), 0, g.G - 1);
}

// one sample: false when it is skipped; else the clamped neighbours and the two distances
template <typename T>
struct Tap {
    int x0, x1, y0, y1;
    T dx, dy;
};
template <typename T>
__device__ __forceinline__ bool make_tap(T w, T h, const Geo& g, Tap<T>& t) {
    if (w < (T)-0.5 || w > (T)g.W - (T)0.5 || h < (T)-0.5 || h > (T)g.H - (T)0.5) return false;
    w = fmin(fmax(w, (T)0), (T)(g.W - 1));
    h = fmin(fmax(h, (T)0), (T)(g.H - 1));
    const T fx = floor(w), fy = floor(h);
    t.x0 = clampi((int)fx, 0, g.W - 1);
    t.x1 = clampi((int)ceil(w), 0, g.W - 1);
    t.y0 = clampi((int)fy, 0, g.H - 1);
    t.y1 = clampi((int)ceil(h), 0, g.H - 1);
    t.dx = w - fx;
    t.dy = h - fy;
    return true;
}

template <typename T>
__global__ __launch_bounds__(256) void psroi_fwd_kernel(const T* __restrict__ data, const T* __restrict__ rois,
                                                        const T* __restrict__ trans, T* __restrict__ out, T* __restrict__ out_count,
                                                        Geo g, T spatial_scale, T trans_std) {
    const int per_roi = g.out_channels * g.pooled * g.pooled;
    const int chunks = (int)(((unsigned)per_roi + 255u) / 256u);
    const int n = blockIdx.x / chunks;                               // uniform over the workgroup: the RoI header is scalar loads
    const int e = (blockIdx.x % chunks) * 256 + threadIdx.x;
    if (e >= per_roi) return;
    const Roi<T> r = load_roi(rois, n, spatial_scale, g);
    const int pw = e % g.pooled, ph = (e / g.pooled) % g.pooled, ctop = e / (g.pooled * g.pooled);
    const size_t oi = (size_t)n * per_roi + e;
    if (r.batch < 0) {
        out[oi] = (T)0;
        out_count[oi] = (T)0;
        return;
    }
    T tx = (T)0, ty = (T)0;
    if (!g.no_trans) {
        const int cls = ctop / g.cec;
        const size_t ti = ((((size_t)n * g.num_classes + cls) * 2) * g.part + part_of<T>(ph, g)) * g.part + part_of<T>(pw, g);
        tx = trans[ti] * trans_std;
        ty = trans[ti + (size_t)g.part * g.part] * trans_std;
    }
    T wstart = (T)pw * r.bin_w + r.start_w;
    wstart += tx * r.width;
    T hstart = (T)ph * r.bin_h + r.start_h;
    hstart += ty * r.height;
    const int c = (ctop * g.G + group_of<T>(ph, g)) * g.G + group_of<T>(pw, g);
    const T* plane = data + ((size_t)r.batch * g.C + c) * g.H * g.W;
    double sum = 0.0;
    int count = 0;
    for (int ih = 0; ih < g.spp; ih++) {
        const T h = hstart + (T)ih * r.sub_h;
        for (int iw = 0; iw < g.spp; iw++) {
            const T w = wstart + (T)iw * r.sub_w;
            Tap<T> t;
            if (!make_tap(w, h, g, t)) continue;
            const T v11 = plane[t.y0 * g.W + t.x0], v12 = plane[t.y1 * g.W + t.x0];
            const T v21 = plane[t.y0 * g.W + t.x1], v22 = plane[t.y1 * g.W + t.x1];
            const T ox = (T)1 - t.dx, oy = (T)1 - t.dy;
            const T v = ox * oy * v11 + ox * t.dy * v12 + t.dx * oy * v21 + t.dx * t.dy * v22;
            sum += (double)v;
            count++;
        }
    }
    out[oi] = count == 0 ? (T)0 : (T)(sum / (double)count);
    out_count[oi] = (T)count;
}

// ---- backward ----------------------------------------------------------------------------------------------------------------
// workspace: [0] bits of max|grad_out| as a double (unsigned compare = value compare for non-negative doubles; a NaN is stored as
//            the quiet-NaN pattern, above inf: both take the poison path of the two kernels below),
//            [1 ..] the N*C*H*W fixed-point plane
template <typename T>
__global__ __launch_bounds__(256) void psroi_absmax_kernel(const T* __restrict__ grad_out, size_t count,
                                                           unsigned long long* __restrict__ ws) {
    double m = 0.0;
    bool nan = false;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (size_t)gridDim.x * 256) {
        const double v = fabs((double)grad_out[i]);
        nan |= v != v;
        m = fmax(m, v);
    }
    unsigned long long bits = nan ? 0x7ff8000000000000ull : (unsigned long long)__double_as_longlong(m);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_xor(bits, o, 64);
        bits = other > bits ? other : bits;
    }
    if ((threadIdx.x & 63) == 0 && bits != 0ull) atomicMax(ws, bits);
}

// nearest integer of a fixed-point contribution; out-of-range / NaN values (a count the forward did not write) add nothing
__device__ __forceinline__ unsigned long long fx_round(double v) {
    return (unsigned long long)(fabs(v) < 9.0e18 ? __double2ll_rn(v) : 0ll);
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// exponent e with 2^e > bound (bound finite, > 0)
__device__ __forceinline__ int bound_exponent(double bound) {
    int e;
    (void)frexp(bound, &e);
    return e;
}

template <typename T>
__global__ __launch_bounds__(64) void psroi_bwd_kernel(const T* __restrict__ grad_out, const T* __restrict__ data,
                                                       const T* __restrict__ rois, const T* __restrict__ trans,
                                                       const T* __restrict__ out_count, T* __restrict__ grad_trans,
                                                       unsigned long long* __restrict__ ws, Geo g, T spatial_scale, T trans_std,
                                                       int prec_bits) {
    // this wave's cell
    int cell = blockIdx.x;
    const int part_w = cell % g.part;
    cell /= g.part;
    const int part_h = cell % g.part;
    cell /= g.part;
    const int cls = cell % g.num_classes;
    const int n = cell / g.num_classes;
    const Roi<T> r = load_roi(rois, n, spatial_scale, g);
    if (r.batch < 0) return;
    const double bound = __longlong_as_double((long long)ws[0]);
    if (bound == 0.0) return;                                        // every grad_out is zero: nothing to add (NaN goes on)
    const bool finite = bound < INFINITY;                            // else: the last pass poisons grad_input, NaN flows into grad_offset
    const int shift = prec_bits - (finite ? bound_exponent(bound) : 0);
    unsigned long long* plane_fx = ws + 1;

    // the bins of this part: part_of is monotone, so they are one range per axis
    int ph_lo = g.pooled, ph_hi = -1, pw_lo = g.pooled, pw_hi = -1;
    for (int p = 0; p < g.pooled; p++) {
        const int q = part_of<T>(p, g);
        if (q == part_h) { ph_lo = p < ph_lo ? p : ph_lo; ph_hi = p; }
        if (q == part_w) { pw_lo = p < pw_lo ? p : pw_lo; pw_hi = p; }
    }
    const int nh = ph_hi - ph_lo + 1, nw = pw_hi - pw_lo + 1;
    if (nh <= 0 || nw <= 0) return;
    T tx = (T)0, ty = (T)0;
    size_t ti = 0;
    if (!g.no_trans) {
        ti = ((((size_t)n * g.num_classes + cls) * 2) * g.part + part_h) * g.part + part_w;
        tx = trans[ti] * trans_std;
        ty = trans[ti + (size_t)g.part * g.part] * trans_std;
    }
    const int spp2 = g.spp * g.spp;
    const int items = g.cec * nh * nw * spp2;                        // < 2^31: out_channels * pooled^2 * spp^2 is checked on the host
    const int per_roi = g.out_channels * g.pooled * g.pooled;
    double acc_x = 0.0, acc_y = 0.0;
    for (int it = threadIdx.x; it < items; it += 64) {
        const int s = it % spp2;
        int b = it / spp2;
        const int pw = pw_lo + b % nw;
        b /= nw;
        const int ph = ph_lo + b % nh;
        const int ctop = cls * g.cec + b / nh;
        const size_t oi = (size_t)n * per_roi + (ctop * g.pooled + ph) * g.pooled + pw;
        const T cnt = out_count[oi];
        if (!(cnt >= (T)1)) continue;                                // the forward writes whole numbers: a count below 1 (or NaN) is none
        const T diff = grad_out[oi] / cnt;
        T wstart = (T)pw * r.bin_w + r.start_w;
        wstart += tx * r.width;
        T hstart = (T)ph * r.bin_h + r.start_h;
        hstart += ty * r.height;
        const T w = wstart + (T)(s % g.spp) * r.sub_w;
        const T h = hstart + (T)(s / g.spp) * r.sub_h;
        Tap<T> t;
        if (!make_tap(w, h, g, t)) continue;
        const int c = (ctop * g.G + group_of<T>(ph, g)) * g.G + group_of<T>(pw, g);
        const size_t base = ((size_t)r.batch * g.C + c) * g.H * g.W;
        const T ox = (T)1 - t.dx, oy = (T)1 - t.dy;
        if (finite) {
            const T q00 = ox * oy * diff, q01 = ox * t.dy * diff, q10 = t.dx * oy * diff, q11 = t.dx * t.dy * diff;
            // count >= 1, so |q| <= |diff| <= bound < 2^e and |q| 2^shift < 2^prec_bits: the plane's sum cannot wrap
            atomicAdd(&plane_fx[base + t.y0 * g.W + t.x0], fx_round(ldexp((double)q00, shift)));
            atomicAdd(&plane_fx[base + t.y1 * g.W + t.x0], fx_round(ldexp((double)q01, shift)));
            atomicAdd(&plane_fx[base + t.y0 * g.W + t.x1], fx_round(ldexp((double)q10, shift)));
            atomicAdd(&plane_fx[base + t.y1 * g.W + t.x1], fx_round(ldexp((double)q11, shift)));
        }
        if (g.no_trans) continue;
        const T* plane = data + base;
        const T u00 = plane[t.y0 * g.W + t.x0], u01 = plane[t.y1 * g.W + t.x0];
        const T u10 = plane[t.y0 * g.W + t.x1], u11 = plane[t.y1 * g.W + t.x1];
        T gx = (u11 * t.dy + u10 * oy - u01 * t.dy - u00 * oy) * trans_std * diff;
        gx *= r.width;
        T gy = (u11 * t.dx + u01 * ox - u10 * t.dx - u00 * ox) * trans_std * diff;
        gy *= r.height;
        acc_x += (double)gx;
        acc_y += (double)gy;
    }
    if (g.no_trans) return;
    acc_x = wave_sum_f64(acc_x);
    acc_y = wave_sum_f64(acc_y);
    if (threadIdx.x == 0) {
        const size_t tj = ti + (size_t)g.part * g.part;
        grad_trans[ti] = (T)((double)grad_trans[ti] + acc_x);
        grad_trans[tj] = (T)((double)grad_trans[tj] + acc_y);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void psroi_bwd_finish_kernel(T* __restrict__ grad_input, const unsigned long long* __restrict__ ws,
                                                               int total, int prec_bits) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const double bound = __longlong_as_double((long long)ws[0]);
    if (bound == 0.0) return;
    if (!(bound < INFINITY)) {                                       // inf / NaN in grad_out: the plane cannot carry it - NaN, loudly
        grad_input[i] = (T)NAN;
        return;
    }
    const long long s = (long long)ws[1 + (size_t)i];
    if (s == 0) return;
    const double v = ldexp((double)s, bound_exponent(bound) - prec_bits);
    grad_input[i] = (T)((double)grad_input[i] + v);
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
struct Plan {
    Geo g;
    int prec_bits;
};

int make_plan(Plan& p, int N, int C, int H, int W, int num_rois, int offset_channels, int no_trans, int out_channels,
              int group_size, int pooled_size, int part_size, int sample_per_part, int dtype) {
    if (N <= 0 || C <= 0 || H <= 0 || W <= 0 || num_rois <= 0 || out_channels <= 0 || group_size <= 0 || pooled_size <= 0 ||
        part_size <= 0 || sample_per_part <= 0)
        return OTP_ERR_BAD_ARG;
    if ((long long)out_channels * group_size * group_size != (long long)C) return OTP_ERR_BAD_ARG;
    int num_classes = 1;
    if (!no_trans) {
        if (offset_channels <= 0 || (offset_channels & 1)) return OTP_ERR_BAD_ARG;
        num_classes = offset_channels / 2;
        if (out_channels % num_classes) return OTP_ERR_BAD_ARG;
    }
    if (dtype != OTP_DTYPE_F32 && dtype != OTP_DTYPE_F64) return OTP_ERR_UNSUPPORTED;
    const long long lim = 1ll << 31;
    if ((long long)N * C * H * W >= lim) return OTP_ERR_UNSUPPORTED;
    const long long per_roi = (long long)out_channels * pooled_size * pooled_size;
    if (per_roi >= lim || per_roi * num_rois >= lim) return OTP_ERR_UNSUPPORTED;
    if (per_roi * sample_per_part >= lim || per_roi * sample_per_part * sample_per_part >= lim) return OTP_ERR_UNSUPPORTED;
    if ((long long)num_rois * num_classes * part_size * part_size >= lim) return OTP_ERR_UNSUPPORTED;
    if (((per_roi + 255) / 256) * num_rois >= lim) return OTP_ERR_UNSUPPORTED;
    p.g = Geo{N, C, H, W, num_rois, no_trans ? 1 : 0, out_channels, group_size, pooled_size, part_size, sample_per_part,
              num_classes, out_channels / num_classes};
    // most contributions one grad_input cell can receive: every RoI, the bins of one group cell, every sample, and all four
    // neighbours of a sample where they coincide
    const long long per_group = (pooled_size + group_size - 1) / group_size + 1;
    const long long most = (long long)num_rois * per_group * per_group * sample_per_part * sample_per_part * 4;
    int bits = 0;
    while ((1ll << bits) < most) bits++;
    p.prec_bits = 62 - bits;
    if (p.prec_bits > 52) p.prec_bits = 52;
    if (p.prec_bits < 40) return OTP_ERR_UNSUPPORTED;
    return OTP_OK;
}

template <typename T>
int forward_t(const void* data, const void* rois, const void* offset, void* out, void* out_count, const Geo& g,
              float spatial_scale, float trans_std, hipStream_t s) {
    const int per_roi = g.out_channels * g.pooled * g.pooled;
    psroi_fwd_kernel<T><<<(unsigned)((((long long)per_roi + 255) / 256) * g.num_rois), 256, 0, s>>>(
        (const T*)data, (const T*)rois, (const T*)offset, (T*)out, (T*)out_count, g, (T)spatial_scale, (T)trans_std);
    return otp_launch_status();
}

template <typename T>
int backward_t(const void* grad_out, const void* data, const void* rois, const void* offset, const void* out_count,
               void* grad_input, void* grad_offset, const Plan& p, float spatial_scale, float trans_std, void* workspace,
               size_t ws_bytes, hipStream_t s) {
    const Geo& g = p.g;
    unsigned long long* ws = (unsigned long long*)workspace;
    if (hipMemsetAsync(ws, 0, ws_bytes, s) != hipSuccess) return OTP_ERR_LAUNCH;
    const size_t count = (size_t)g.num_rois * g.out_channels * g.pooled * g.pooled;
    const int nb = (int)((count + 255) / 256 < 1024 ? (count + 255) / 256 : 1024);
    psroi_absmax_kernel<T><<<nb, 256, 0, s>>>((const T*)grad_out, count, ws);
    psroi_bwd_kernel<T><<<g.num_rois * g.num_classes * g.part * g.part, 64, 0, s>>>(
        (const T*)grad_out, (const T*)data, (const T*)rois, (const T*)offset, (const T*)out_count, (T*)grad_offset, ws, g,
        (T)spatial_scale, (T)trans_std, p.prec_bits);
    const int total = g.N * g.C * g.H * g.W;
    psroi_bwd_finish_kernel<T><<<(unsigned)(((long long)total + 255) / 256), 256, 0, s>>>((T*)grad_input, ws, total, p.prec_bits);
    return otp_launch_status();
}

}  // namespace

int otp_deform_psroi_pool_forward(const void* data, const void* rois, const void* offset, void* out, void* out_count, int N, int C,
                                  int H, int W, int num_rois, int offset_channels, int no_trans, float spatial_scale,
                                  int out_channels, int group_size, int pooled_size, int part_size, int sample_per_part,
                                  float trans_std, int dtype, void* stream) {
    if (!data || !rois || !out || !out_count || (!no_trans && !offset)) return OTP_ERR_BAD_ARG;
    Plan p;
    const int st = make_plan(p, N, C, H, W, num_rois, offset_channels, no_trans, out_channels, group_size, pooled_size, part_size,
                             sample_per_part, dtype);
    if (st != OTP_OK) return st;
    hipStream_t s = (hipStream_t)stream;
    return dtype == OTP_DTYPE_F64 ? forward_t<double>(data, rois, offset, out, out_count, p.g, spatial_scale, trans_std, s)
                                  : forward_t<float>(data, rois, offset, out, out_count, p.g, spatial_scale, trans_std, s);
}

size_t otp_deform_psroi_pool_backward_workspace(int N, int C, int H, int W, int num_rois, int offset_channels, int no_trans,
                                                int out_channels, int group_size, int pooled_size, int part_size,
                                                int sample_per_part, int dtype) {
    Plan p;
    if (make_plan(p, N, C, H, W, num_rois, offset_channels, no_trans, out_channels, group_size, pooled_size, part_size,
                  sample_per_part, dtype) != OTP_OK)
        return 0;
    return 8 * ((size_t)N * C * H * W + 1);
}

int otp_deform_psroi_pool_backward(const void* grad_out, const void* data, const void* rois, const void* offset,
                                   const void* out_count, void* grad_input, void* grad_offset, int N, int C, int H, int W,
                                   int num_rois, int offset_channels, int no_trans, float spatial_scale, int out_channels,
                                   int group_size, int pooled_size, int part_size, int sample_per_part, float trans_std,
                                   void* workspace, size_t workspace_bytes, int dtype, void* stream) {
    if (!grad_out || !data || !rois || !out_count || !grad_input || !workspace || (!no_trans && (!offset || !grad_offset)))
        return OTP_ERR_BAD_ARG;
    Plan p;
    const int st = make_plan(p, N, C, H, W, num_rois, offset_channels, no_trans, out_channels, group_size, pooled_size, part_size,
                             sample_per_part, dtype);
    if (st != OTP_OK) return st;
    const size_t need = 8 * ((size_t)N * C * H * W + 1);
    if (workspace_bytes < need) return OTP_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    return dtype == OTP_DTYPE_F64 ? backward_t<double>(grad_out, data, rois, offset, out_count, grad_input, grad_offset, p,
                                                       spatial_scale, trans_std, workspace, need, s)
                                  : backward_t<float>(grad_out, data, rois, offset, out_count, grad_input, grad_offset, p,
                                                      spatial_scale, trans_std, workspace, need, s);
}
