// Optimizer step of the reference training loop (script/Common.py:136-143): global-norm gradient clipping
// (torch.nn.utils.clip_grad_norm_, max_norm = TRAIN.CLIP_GRAD_L2NORM) followed by AdamW
// (thirdparty/utils/train_utils.py:129-133, torch.optim.AdamW semantics) over FLAT parameter / gradient / moment buffers.
// Two HBM-bound passes: sum of squares (fp64 partials per workgroup, added in a fixed order: no atomics, the same bits on
// every run) and the fused clip + update, which reads the
// clip coefficient from device memory - no host synchronisation between backward and the next forward.
// TRAIN.OPTIMIZER = SGD (train_utils.py:123-128, torch.optim.SGD semantics) is a second update kernel behind the same clip.
#include "common.h"

#include <string.h>

namespace {

constexpr int SUMSQ_PARTS = 1024;       // most workgroups of one sum-of-squares launch = scratch doubles behind the accumulator

// part[block] = this workgroup's share of sum(g^2) (fp64, fixed order: strided per-thread sums, shuffle tree, waves in order)
__global__ __launch_bounds__(256) void sumsq_kernel(const float* __restrict__ g, size_t n4, size_t n,
                                                     double* __restrict__ part) {
    __shared__ double red[4];
    double s = 0.0;
    const otp_f32x4* g4 = reinterpret_cast<const otp_f32x4*>(g);
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
        const otp_f32x4 v = g4[i];
        s += (double)(v[0] * v[0] + v[1] * v[1]) + (double)(v[2] * v[2] + v[3] * v[3]);
    }
    if (blockIdx.x == 0)
        for (size_t i = n4 * 4 + threadIdx.x; i < n; i += 256) s += (double)g[i] * (double)g[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// *acc += sum of the `parts` partials in a fixed order (one workgroup; no atomics: the same bits on every run)
__global__ __launch_bounds__(256) void sumsq_finish_kernel(const double* __restrict__ part, int parts, double* __restrict__ acc) {
    __shared__ double red[4];
    double s = 0.0;
    for (int i = threadIdx.x; i < parts; i += 256) s += part[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) *acc += (red[0] + red[1]) + (red[2] + red[3]);
}

__device__ __forceinline__ void adamw_one(float& p, float g, float& m, float& v, float clip, float lr_wd, float b1, float b2,
                                          float step_size, float inv_sqrt_bc2, float eps) {
    g *= clip;
    p *= lr_wd;                                       // p * (1 - lr * weight_decay)
    m = b1 * m + (1.f - b1) * g;
    v = b2 * v + (1.f - b2) * g * g;
    const float denom = sqrtf(v) * inv_sqrt_bc2 + eps;
    p -= step_size * (m / denom);
}

__global__ __launch_bounds__(256) void adamw_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                     float* __restrict__ v, size_t n4, size_t n, float lr, float b1, float b2,
                                                     float eps, float wd, float bc1, float bc2,
                                                     const double* __restrict__ gradnorm_sq, float max_norm) {
    float clip = 1.f;
    if (gradnorm_sq && max_norm > 0.f) {
        const float c = max_norm / ((float)sqrt(*gradnorm_sq) + 1e-6f);      // clip_grad_norm_: clamped to 1
        clip = c < 1.f ? c : 1.f;
    }
    const float lr_wd = 1.f - lr * wd, step_size = lr / bc1, inv_sqrt_bc2 = 1.f / sqrtf(bc2);
    otp_f32x4* p4 = reinterpret_cast<otp_f32x4*>(p);
    otp_f32x4* m4 = reinterpret_cast<otp_f32x4*>(m);
    otp_f32x4* v4 = reinterpret_cast<otp_f32x4*>(v);
    const otp_f32x4* g4 = reinterpret_cast<const otp_f32x4*>(g);
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
        otp_f32x4 pp = p4[i], mm = m4[i], vv = v4[i];
        const otp_f32x4 gg = g4[i];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float pe = pp[e], me = mm[e], ve = vv[e];
            adamw_one(pe, gg[e], me, ve, clip, lr_wd, b1, b2, step_size, inv_sqrt_bc2, eps);
            pp[e] = pe; mm[e] = me; vv[e] = ve;
        }
        p4[i] = pp; m4[i] = mm; v4[i] = vv;
    }
    if (blockIdx.x == 0)
        for (size_t i = n4 * 4 + threadIdx.x; i < n; i += 256)
            adamw_one(p[i], g[i], m[i], v[i], clip, lr_wd, b1, b2, step_size, inv_sqrt_bc2, eps);
}

// torch.optim.SGD on one element: d = clip * g (+ wd * p); with momentum the buffer recurrence, then p -= lr * d
__device__ __forceinline__ void sgd_one(float& p, float g, float& buf, float clip, float lr, float mom, float one_m_damp,
                                        float wd, bool use_wd, bool use_mom, bool nesterov, bool first) {
    float d = clip * g;
    if (use_wd) d += wd * p;
    if (use_mom) {
        buf = first ? d : mom * buf + one_m_damp * d;
        d = nesterov ? d + mom * buf : buf;
    }
    p -= lr * d;
}

// buf == nullptr <=> momentum == 0: the buffer is neither read nor written
__global__ __launch_bounds__(256) void sgd_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf,
                                                   size_t n4, size_t n, float lr, float mom, float damp, float wd, int nesterov,
                                                   int first, const double* __restrict__ gradnorm_sq, float max_norm) {
    float clip = 1.f;
    if (gradnorm_sq && max_norm > 0.f) {
        const float c = max_norm / ((float)sqrt(*gradnorm_sq) + 1e-6f);      // clip_grad_norm_: clamped to 1
        clip = c < 1.f ? c : 1.f;
    }
    const bool use_wd = wd != 0.f, use_mom = buf != nullptr, nest = nesterov != 0, fst = first != 0;
    const float one_m_damp = 1.f - damp;
    otp_f32x4* p4 = reinterpret_cast<otp_f32x4*>(p);
    otp_f32x4* b4 = reinterpret_cast<otp_f32x4*>(buf);
    const otp_f32x4* g4 = reinterpret_cast<const otp_f32x4*>(g);
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
        otp_f32x4 pp = p4[i], bb = {0.f, 0.f, 0.f, 0.f};
        const otp_f32x4 gg = g4[i];
        if (use_mom && !fst) bb = b4[i];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float pe = pp[e], be = bb[e];
            sgd_one(pe, gg[e], be, clip, lr, mom, one_m_damp, wd, use_wd, use_mom, nest, fst);
            pp[e] = pe; bb[e] = be;
        }
        p4[i] = pp;
        if (use_mom) b4[i] = bb;
    }
    if (blockIdx.x == 0)
        for (size_t i = n4 * 4 + threadIdx.x; i < n; i += 256) {
            float be = (use_mom && !fst) ? buf[i] : 0.f;
            sgd_one(p[i], g[i], be, clip, lr, mom, one_m_damp, wd, use_wd, use_mom, nest, fst);
            if (use_mom) buf[i] = be;
        }
}

// ---- weight EMA (thirdparty/utils/train_utils.py:240-262 ModelEma) ------------------------------------------------------------
// ema = decay * ema + one_minus_decay * src, the two products and the sum each rounded to fp32: the bits of the reference's
// three PyTorch operations (mul by a Python scalar, mul, add).  Never an FMA.
__device__ __forceinline__ float ema_one(float e, float m, float d, float omd) {
#pragma clang fp contract(off)
    const float a = d * e;
    const float b = omd * m;
    return a + b;
}

// int64 entries (BatchNorm's num_batches_tracked): to fp32, the same arithmetic, back by truncation toward zero - what
// `long_tensor.copy_(decay * long_tensor + (1 - decay) * long_tensor)` does
__device__ __forceinline__ long long ema_one_i64(long long e, long long m, float d, float omd) {
    return (long long)ema_one((float)e, (float)m, d, omd);
}

typedef float ema_f32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));       // a 16-byte load from a 4-byte-aligned address

// Elements live at positions q = shift + index, shift = the floats between the preceding 16-byte boundary and `ema`, so that
// q % 4 == 0 is a 16-byte-aligned address of ema: ema_al = ema - shift, src_al = src - shift, valid positions [lo, hi).  One
// quad of positions: a 16-byte load / store where it lies inside [lo, hi) (src may sit at another offset from its own boundary:
// its load asks for 4-byte alignment only), element by element at the two ends (the scalar head and tail).
__device__ __forceinline__ void ema_quad(float* __restrict__ ema_al, const float* __restrict__ src_al, size_t q, size_t lo,
                                         size_t hi, float d, float omd) {
    if (q >= lo && q + 4 <= hi) {
        otp_f32x4 e = *reinterpret_cast<const otp_f32x4*>(ema_al + q);
        const otp_f32x4 m = *reinterpret_cast<const ema_f32x4_a4*>(src_al + q);
#pragma unroll
        for (int k = 0; k < 4; ++k) e[k] = ema_one(e[k], m[k], d, omd);
        *reinterpret_cast<otp_f32x4*>(ema_al + q) = e;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (q + k >= lo && q + k < hi) ema_al[q + k] = ema_one(ema_al[q + k], src_al[q + k], d, omd);
    }
}

__global__ __launch_bounds__(256) void ema_flat_kernel(float* __restrict__ ema_al, const float* __restrict__ src_al, size_t lo,
                                                        size_t hi, float d, float omd) {
    const size_t quads = (hi + 3) / 4;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < quads; i += (size_t)gridDim.x * 256)
        ema_quad(ema_al, src_al, i * 4, lo, hi, d, omd);
}

// One entry of otp_ema_update_table's device table, written by otp_ema_job.  The work of a table is cut into units of
// EMA_UNIT positions (one 16-byte access per thread of a workgroup); unit0 / unit_end are the running sum of the units of the
// jobs before / up to this one, so the last job's unit_end is the table's total and a unit number finds its job by bisection.
struct EmaJob {
    void* ema;
    const void* src;
    unsigned long long count;
    unsigned long long unit0, unit_end;
    int dtype;
    int shift;                            // fp32: floats between the preceding 16-byte boundary and ema (0 .. 3); int64: 0
};
constexpr unsigned long long EMA_UNIT = 1024;
constexpr unsigned EMA_TABLE_GRID = 2048;

// Workgroup b takes the units [b * total / grid, (b + 1) * total / grid): one bisection for its first unit, then it walks the
// table forward - a tensor of a million elements is spread over many workgroups, a hundred 64-element ones share one.
__global__ __launch_bounds__(256) void ema_table_kernel(const EmaJob* __restrict__ jobs, int n_jobs, float d, float omd) {
    const unsigned long long total = jobs[n_jobs - 1].unit_end;
    const unsigned long long per = total / gridDim.x, rem = total % gridDim.x, b = blockIdx.x;
    unsigned long long u = b * per + (b < rem ? b : rem);
    const unsigned long long u_end = u + per + (b < rem ? 1 : 0);
    if (u >= u_end) return;
    int lo = 0, hi = n_jobs - 1;          // the first job with unit_end > u
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (jobs[mid].unit_end > u) hi = mid; else lo = mid + 1;
    }
    int j = lo;
    EmaJob job = jobs[j];
    for (; u < u_end; ++u) {
        while (u >= job.unit_end) job = jobs[++j];             // (jobs without elements own no unit and are stepped over)
        const unsigned long long first = (u - job.unit0) * EMA_UNIT;
        if (job.dtype == OTP_DTYPE_F32) {
            const size_t vlo = (size_t)job.shift, vhi = vlo + (size_t)job.count;
            float* ema_al = reinterpret_cast<float*>(reinterpret_cast<uintptr_t>(job.ema) - 4 * vlo);
            const float* src_al = reinterpret_cast<const float*>(reinterpret_cast<uintptr_t>(job.src) - 4 * vlo);
            ema_quad(ema_al, src_al, (size_t)first + 4 * threadIdx.x, vlo, vhi, d, omd);
        } else {
            long long* e = static_cast<long long*>(job.ema);
            const long long* m = static_cast<const long long*>(job.src);
            for (unsigned long long i = first + threadIdx.x; i < first + EMA_UNIT && i < job.count; i += 256)
                e[i] = ema_one_i64(e[i], m[i], d, omd);
        }
    }
}

unsigned grid_for(size_t n4) {
    const size_t b = (n4 + 255) / 256;
    return (unsigned)(b < 1 ? 1 : (b > 4096 ? 4096 : b));
}

}  // namespace

extern "C" size_t otp_grad_sumsq_scratch(void) { return SUMSQ_PARTS; }

extern "C" int otp_grad_sumsq(const void* grad, size_t n, void* acc_f64, void* stream) {
    if (!grad || !acc_f64 || n == 0) return OTP_ERR_BAD_ARG;
    if (reinterpret_cast<uintptr_t>(grad) & 15) return OTP_ERR_UNSUPPORTED;
    unsigned grid = grid_for(n / 4);
    if (grid > SUMSQ_PARTS) grid = SUMSQ_PARTS;
    double* acc = static_cast<double*>(acc_f64);
    auto st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(sumsq_kernel, dim3(grid), dim3(256), 0, st, static_cast<const float*>(grad), n / 4, n, acc + 1);
    hipLaunchKernelGGL(sumsq_finish_kernel, dim3(1), dim3(256), 0, st, acc + 1, (int)grid, acc);
    return otp_launch_status();
}

extern "C" int otp_adamw_step(void* param, const void* grad, void* exp_avg, void* exp_avg_sq, size_t n, float lr, float beta1,
                              float beta2, float eps, float weight_decay, int step, const void* gradnorm_sq_f64,
                              float max_norm, void* stream) {
    if (!param || !grad || !exp_avg || !exp_avg_sq || n == 0 || step < 1) return OTP_ERR_BAD_ARG;
    if ((reinterpret_cast<uintptr_t>(param) | reinterpret_cast<uintptr_t>(grad) | reinterpret_cast<uintptr_t>(exp_avg) |
         reinterpret_cast<uintptr_t>(exp_avg_sq)) & 15)
        return OTP_ERR_UNSUPPORTED;
    const float bc1 = 1.f - powf(beta1, (float)step), bc2 = 1.f - powf(beta2, (float)step);
    hipLaunchKernelGGL(adamw_kernel, dim3(grid_for(n / 4)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<float*>(param), static_cast<const float*>(grad), static_cast<float*>(exp_avg),
                       static_cast<float*>(exp_avg_sq), n / 4, n, lr, beta1, beta2, eps, weight_decay, bc1, bc2,
                       static_cast<const double*>(gradnorm_sq_f64), max_norm);
    return otp_launch_status();
}

extern "C" int otp_sgd_step(void* param, const void* grad, void* momentum_buf, size_t n, float lr, float momentum,
                            float dampening, float weight_decay, int nesterov, int first_step, const void* gradnorm_sq_f64,
                            float max_norm, void* stream) {
    if (!param || !grad || n == 0) return OTP_ERR_BAD_ARG;
    if (!(lr >= 0.f) || !(momentum >= 0.f) || !(weight_decay >= 0.f)) return OTP_ERR_BAD_ARG;      // (NaN is rejected, too)
    if (momentum != 0.f && !momentum_buf) return OTP_ERR_BAD_ARG;
    if (nesterov && (momentum <= 0.f || dampening != 0.f)) return OTP_ERR_BAD_ARG;                  // torch: ValueError
    if (momentum == 0.f) momentum_buf = nullptr;                                                    // no buffer is touched
    if ((reinterpret_cast<uintptr_t>(param) | reinterpret_cast<uintptr_t>(grad) | reinterpret_cast<uintptr_t>(momentum_buf)) & 15)
        return OTP_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(sgd_kernel, dim3(grid_for(n / 4)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<float*>(param), static_cast<const float*>(grad), static_cast<float*>(momentum_buf), n / 4, n,
                       lr, momentum, dampening, weight_decay, nesterov, first_step,
                       static_cast<const double*>(gradnorm_sq_f64), max_norm);
    return otp_launch_status();
}

extern "C" size_t otp_ema_job_bytes(void) { return sizeof(EmaJob); }

extern "C" int otp_ema_job(void* ema, const void* src, size_t count, int dtype, const void* prev_job_host, void* job_host) {
    if (!job_host || !ema || !src) return OTP_ERR_BAD_ARG;
    if (dtype != OTP_DTYPE_F32 && dtype != OTP_DTYPE_I64) return OTP_ERR_UNSUPPORTED;
    const uintptr_t align = dtype == OTP_DTYPE_F32 ? 3 : 7;
    if ((reinterpret_cast<uintptr_t>(ema) | reinterpret_cast<uintptr_t>(src)) & align) return OTP_ERR_UNSUPPORTED;
    if (count > ((size_t)1 << 48)) return OTP_ERR_UNSUPPORTED;
    EmaJob job;
    memset(&job, 0, sizeof(job));
    job.ema = ema;
    job.src = src;
    job.count = count;
    job.dtype = dtype;
    job.shift = dtype == OTP_DTYPE_F32 ? (int)((reinterpret_cast<uintptr_t>(ema) & 15) / 4) : 0;
    job.unit0 = prev_job_host ? static_cast<const EmaJob*>(prev_job_host)->unit_end : 0;
    job.unit_end = job.unit0 + (count ? ((unsigned long long)job.shift + count + EMA_UNIT - 1) / EMA_UNIT : 0);
    memcpy(job_host, &job, sizeof(job));
    return OTP_OK;
}

extern "C" int otp_ema_update(void* ema, const void* src, size_t n, float decay, float one_minus_decay, void* stream) {
    if (!ema || !src) return OTP_ERR_BAD_ARG;
    if ((reinterpret_cast<uintptr_t>(ema) | reinterpret_cast<uintptr_t>(src)) & 3) return OTP_ERR_UNSUPPORTED;
    if (n == 0) return OTP_OK;
    const size_t shift = (reinterpret_cast<uintptr_t>(ema) & 15) / 4;
    float* ema_al = reinterpret_cast<float*>(reinterpret_cast<uintptr_t>(ema) - 4 * shift);
    const float* src_al = reinterpret_cast<const float*>(reinterpret_cast<uintptr_t>(src) - 4 * shift);
    hipLaunchKernelGGL(ema_flat_kernel, dim3(grid_for((shift + n + 3) / 4)), dim3(256), 0, static_cast<hipStream_t>(stream), ema_al,
                       src_al, shift, shift + n, decay, one_minus_decay);
    return otp_launch_status();
}

extern "C" int otp_ema_update_table(const void* jobs_device, int n_jobs, float decay, float one_minus_decay, void* stream) {
    if (n_jobs < 0 || (n_jobs > 0 && !jobs_device)) return OTP_ERR_BAD_ARG;
    if (n_jobs == 0) return OTP_OK;
    if (reinterpret_cast<uintptr_t>(jobs_device) & 7) return OTP_ERR_UNSUPPORTED;
    // the table is device memory: its total is not known here, so the grid is fixed and a workgroup without a unit returns
    hipLaunchKernelGGL(ema_table_kernel, dim3(EMA_TABLE_GRID), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const EmaJob*>(jobs_device), n_jobs, decay, one_minus_decay);
    return otp_launch_status();
}
