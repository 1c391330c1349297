// bf16 training path of the HRNet backbone (BASELINE configs[2]: "bf16 training step"; the reference step is
// script/Common.py:118-144 over model/HRNet.py:116-152): activations live in HBM as NHWC bfloat16 (channel stride
// rounded up to 8, padding channels zero), every contraction runs on v_mfma_f32_16x16x32_bf16 with fp32 accumulation,
// BatchNorm statistics / gradients and the weight gradients are fp32, master weights stay fp32 (cast while packing).
//
// Why NHWC here when the fp32 path is NCHW: a bf16 MFMA operand is 8 consecutive k-values per lane; with channels
// innermost both the activations (k = input channel) and the packed weights deliver a fragment as ONE 16-byte LDS
// read, taps shift whole pixels (16-byte aligned), and nothing is transposed on the way in or out.
//
// The path is four translation units - csrc/nhwc_conv.hip (plan, weight packer, nhwc_conv_kernel, route rule), csrc/nhwc_wgrad.hip
// (weight gradients), csrc/nhwc_bn.hip (BatchNorm forward / backward), csrc/nhwc_pass.hip (the other HBM-bound passes).  This
// header holds what more than one of them uses, and nothing else.
#pragma once
#include "common.h"

typedef __bf16 bf16;
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float bf2f(bf16 v) { return (float)v; }

// 16-byte range-checked buffer load: staging loops mask a unit by pointing it past the descriptor (OTP_OOB: the hardware returns
// zeros) instead of branching around the load - hipcc waits for every outstanding load at each such branch, which turns a
// batch of independent loads into a chain of L2 round trips.
__device__ __forceinline__ otp_u32x4 bload16(otp_rsrc r, int voff_bytes) {
    return __builtin_bit_cast(otp_u32x4, __builtin_amdgcn_raw_buffer_load_b128(r, voff_bytes, 0, 0));
}

#ifdef OTP_NHWC_TIMING
// development build only (tools/nhwc_timing.sh), never in libotpose_hip.so: per-workgroup phase stamps of nhwc_conv_kernel or of
// nhwc_wgrad_kernel.  The array belongs to the translation unit, so the define goes to exactly ONE of csrc/nhwc_conv.hip and
// csrc/nhwc_wgrad.hip, and that one carries otp_nhwc_read_stamps.
static __device__ unsigned long long otp_nhwc_stamps[8192 * 8];
#define OTP_STAMP(slot)                                                                              \
    do {                                                                                             \
        if (threadIdx.x == 0 && blockIdx.x < 8192) otp_nhwc_stamps[blockIdx.x * 8 + (slot)] = __builtin_readcyclecounter(); \
    } while (0)
extern "C" int otp_nhwc_read_stamps(void* host_out, size_t bytes) {
    return hipMemcpyFromSymbol(host_out, HIP_SYMBOL(otp_nhwc_stamps), bytes) == hipSuccess ? OTP_OK : OTP_ERR_LAUNCH;
}
#else
#define OTP_STAMP(slot)
#endif

static inline int round_up(int a, int b) { return (a + b - 1) / b * b; }

static inline int grid_for(size_t units) {
    size_t g = (units + 255) / 256;
    if (g > 256 * 16) g = 256 * 16;
    if (g < 1) g = 1;
    return (int)g;
}

static inline bool valid_desc(const otp_nhwc_conv_desc* d) {
    return d && d->N > 0 && d->H > 0 && d->W > 0 && d->Cin > 0 && d->Cout > 0 && d->kh > 0 && d->kw > 0 && d->stride > 0 &&
           d->dil > 0 && d->pad >= 0;
}

// partial rows of the BatchNorm backward's first pass and of the channel sum, and the pixels each row's workgroup covers
static inline int bn_bwd_rows(size_t pixels, int* pixPerWg) {
    // a workgroup strides its pixel range with 256 / (C/8) pixel lanes: 64-pixel ranges still give every lane several
    // pixels at 384 channels, and the small maps (12x9 x 80 frames = 8640 pixels) still fill the chip
    int rows = (int)((pixels + 63) / 64);
    if (rows > 1024) rows = 1024;
    if (rows < 1) rows = 1;
    *pixPerWg = (int)((pixels + rows - 1) / rows);
    return (int)((pixels + *pixPerWg - 1) / *pixPerWg);
}

// The geometry of a descriptor as nhwc_conv_kernel's plan settles it (csrc/nhwc_conv.hip: make_plan) - padded channel counts, output
// size, and the image of a pointwise conv re-read as rows of W' pixels.  The weight gradient's plan starts from it, so a descriptor the
// forward has no plan for has no weight gradient either.  Defined in csrc/nhwc_conv.hip (not exported); false: no plan.
struct NhwcGeom {
    int N, H, W, CinS, Ho, Wo, CoutS, Cin, Cout, kh, kw, stride, pad, dil;
};
__attribute__((visibility("hidden"))) bool nhwc_conv_geom(const otp_nhwc_conv_desc* d, NhwcGeom* g);
