// The keep mask of the attention-probability dropout as a tensor, for tests and debugging: the same device functions the attention
// kernels evaluate in place (csrc/common.h: otp_attn_drop; the definition is stated in include/otpose_hip.h).
#include "common.h"

namespace {

// one thread per entry of (G, R, Ccols): keep[(g R + i) Ccols + j] = 1 for a survivor, 0 for a dropped entry
__global__ __launch_bounds__(256) void attn_drop_keep_kernel(unsigned char* __restrict__ keep, size_t rows, int Ccols,
                                                             otp_attn_drop drop) {
    const size_t n = rows * (size_t)Ccols;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (size_t)gridDim.x * blockDim.x) {
        const size_t row = e / (size_t)Ccols;
        const int j = (int)(e - row * (size_t)Ccols);
        keep[e] = otp_attn_drop_at(drop, otp_attn_drop_row(row, Ccols), j) != 0.f ? 1 : 0;
    }
}

}  // namespace

extern "C" int otp_attn_dropout_keep(void* keep_u8, int G, int R, int Ccols, float p, unsigned long long seed, void* stream) {
    if (!keep_u8 || G <= 0 || R <= 0 || Ccols <= 0 || !otp_attn_drop_rate_ok(p)) return OTP_ERR_BAD_ARG;
    const size_t rows = (size_t)G * R, blocks = (rows * Ccols + 255) / 256;
    hipLaunchKernelGGL(attn_drop_keep_kernel, dim3((unsigned)(blocks > 65536 ? 65536 : blocks)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), static_cast<unsigned char*>(keep_u8), rows, Ccols,
                       otp_attn_drop_make(p, seed));
    return otp_launch_status();
}
