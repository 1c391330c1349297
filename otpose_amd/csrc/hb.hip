// The fp16 engine's window / weight-stream 3x3 kernel and its pointwise kernel (csrc/h16_kernels.h) instantiated with the Bf16
// traits on bfloat16 NHWC tensors: the training step's 3x3 forward / input-gradient convolutions and the TransformerBlock MLP's
// projections (otp_hb_* / otp_hbpw_* of csrc/hb.h, reached through csrc/nhwc_conv.hip's otp_nhwc_conv_*).
#include "h16_kernels.h"
#include <cstring>
#include <map>
#include <mutex>

namespace {
// The plan walks every pixel tile of the launch (h16_window_records) - fine once per layer when a forward is captured into a graph, not
// per launch of an eager training step (~700 convolutions, each asking three or four times): plans are kept per shape.
struct HbKey {
    int v[6];
    bool operator<(const HbKey& o) const { return memcmp(v, o.v, sizeof(v)) < 0; }
};
std::mutex g_hb_mutex;
std::map<HbKey, std::pair<bool, HPlan>> g_hb_plans;

bool hb_plan(const otp_nhwc_conv_desc* d, HPlan& P) {
    if (!d || d->kh != 3 || d->kw != 3 || d->pad != 1 || d->dil != 1 || (d->stride != 1 && d->stride != 2) || d->out_mode != 0) return false;
    const HbKey key{{d->N, d->Cin, d->H, d->W, d->Cout, d->stride}};
    std::lock_guard<std::mutex> lock(g_hb_mutex);
    auto it = g_hb_plans.find(key);
    if (it == g_hb_plans.end()) {
        otp_h16_conv_desc h{};
        h.N = d->N, h.Cin = d->Cin, h.H = d->H, h.W = d->W, h.Cout = d->Cout, h.stride = d->stride, h.act = OTP_ACT_NONE;
        h.out_scale = 1.f;
        HPlan Q{};
        const bool ok = h16_conv_plan<Bf16>(h, Q, true);
        if (g_hb_plans.size() > 4096) g_hb_plans.clear();
        it = g_hb_plans.emplace(key, std::make_pair(ok, Q)).first;
    }
    P = it->second.second;
    return it->second.first;
}
}  // namespace

// ---- 1x1 convolutions of (N, 1, T, C) sequences: the TransformerBlock MLP's projections and their input gradients ----------------
bool otp_hbpw_supported(const otp_nhwc_conv_desc* d) {
    if (!d || d->kh != 1 || d->kw != 1 || d->stride != 1 || d->pad != 0 || d->N <= 0 || d->H <= 0 || d->W <= 0) return false;
    if (d->Cin % 8 || d->Cout % 8 || d->Cout > HPW_MAXC || otp_hbpw_ks(d->Cin) == 0) return false;
    if (d->out_mode != 0 && d->out_mode != 1) return false;
    return (size_t)d->N * d->H * d->W < (1ull << 31);
}

int otp_hbpw_stats_rows(const otp_nhwc_conv_desc* d) { return otp_hbpw_supported(d) ? (d->N * d->H * d->W + 127) / 128 : 0; }

int otp_hbpw_conv(const void* x, const void* wpacked, const void* bias, const void* res, void* out, void* stats,
                  const otp_nhwc_conv_desc* d, hipStream_t stream, const otp_hbpw_epi* epi) {
    if (!otp_hbpw_supported(d)) return OTP_ERR_UNSUPPORTED;
    if (stats && d->out_mode != 0) return OTP_ERR_BAD_ARG;
    if (epi && epi->mode && (d->out_mode != 0 || stats || res || !epi->keep || (epi->mode == 1 ? !epi->out2 : !epi->aux) ||
                             ((reinterpret_cast<uintptr_t>(epi->out2) | reinterpret_cast<uintptr_t>(epi->aux)) & 15)))
        return OTP_ERR_BAD_ARG;
    if (((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(wpacked) | reinterpret_cast<uintptr_t>(res)) & 15) ||
        (reinterpret_cast<uintptr_t>(out) & (d->out_mode ? 3 : 15)) || (reinterpret_cast<uintptr_t>(bias) & 3))
        return OTP_ERR_UNSUPPORTED;
    HPw a{};
    a.x = static_cast<const unsigned char*>(x);
    a.packed = static_cast<const unsigned char*>(wpacked);
    a.res = static_cast<const unsigned char*>(res);
    a.out = static_cast<unsigned char*>(out);
    a.shift = static_cast<const float*>(bias);
    const int HW = d->H * d->W;
    a.total = d->N * HW, a.HW = HW, a.Cin = d->Cin, a.Cout = d->Cout, a.nblk = (d->Cout + 31) / 32, a.relu = 0, a.f32out = d->out_mode ? 1 : 0;
    a.x_pS = (size_t)d->Cin * 2, a.x_gS = 16, a.x_imgB = HW * a.x_pS, a.x_base = 0;
    a.r_pS = a.o_pS = (size_t)d->Cout * 2, a.r_gS = a.o_gS = 16, a.r_imgB = a.o_imgB = HW * a.o_pS, a.r_base = a.o_base = 0;
    a.o_tot = d->Cout, a.o_off = 0;
    a.post = 1.f;
    a.rflag = nullptr;
    a.stats = static_cast<float*>(stats);
    if (epi) a.epi = *epi;
    const int ks = otp_hbpw_ks(d->Cin), mode = epi ? epi->mode : 0;
    if (mode) {                                                    // the MLP epilogues: the up-projection / the down-projection's input gradient (Cin = C)
#define OTP_HBPW_EPI(KS_)                                                     \
    if (ks == KS_) return mode == 1 ? hpw_launch<Bf16, KS_, 2>(a, stream) : hpw_launch<Bf16, KS_, 3>(a, stream);
        OTP_HBPW_EPI(2) OTP_HBPW_EPI(4) OTP_HBPW_EPI(5) OTP_HBPW_EPI(8)
#undef OTP_HBPW_EPI
        return OTP_ERR_UNSUPPORTED;
    }
#define OTP_HBPW_CASE(KS_) \
    if (ks == KS_) return stats ? hpw_launch<Bf16, KS_, 1>(a, stream) : hpw_launch<Bf16, KS_, 0>(a, stream);
    OTP_HBPW_CASE(2) OTP_HBPW_CASE(4) OTP_HBPW_CASE(5) OTP_HBPW_CASE(8) OTP_HBPW_CASE(12) OTP_HBPW_CASE(17)
#undef OTP_HBPW_CASE
    return OTP_ERR_UNSUPPORTED;
}

bool otp_hb_supported(const otp_nhwc_conv_desc* d) {
    HPlan P{};
    return hb_plan(d, P);
}

// Where the window kernel pays (MI355X, 80 frames, tools/bf16_conv_bench.py with OTPOSE_NHWC_HB=2 and =0; forward / input gradient us):
// 48 -> 48 @96x72 47.8 / 46.5 against 50.3 / 49.6, 96 -> 96 @48x36 42.1 / 43.9 against 52.4 / 49.7, 192 -> 192 @24x18 41.7 / 48.4 against
// 49.8 / 52.8, 64 -> 64 @96x72 70.7 / 70.8 against 78.2 / 75.3, 48 -> 96 stride 2 38.3 / 97.3 against 64.1 / 105.0; not at 384 channels
// (54.2 / 62.9 against 53.5 / 60.5) and not on the wide maps (64 -> 64 stride 2 @192x144: 241 / 469 against 234 / 421 - rows of more
// than 96 pixels leave 128- or 64-pixel tiles).  The 16-byte pieces of an NHWC pixel make the window's LDS-DMA gather up to six cache
// lines per instruction where the H8 engine reads one: the gain is a third of what the fp16 engine's layout gives the same kernel.
bool otp_hb_pays(const otp_nhwc_conv_desc* d) { return d && d->W <= 96 && d->Cin <= 192 && d->Cout <= 192; }

int otp_hb_stats_rows(const otp_nhwc_conv_desc* d) {
    HPlan P{};
    return hb_plan(d, P) ? P.nTiles : 0;
}

int otp_hb_conv(const void* x, const void* wpacked, const void* bias, const void* res, void* out, void* stats,
                const otp_nhwc_conv_desc* d, hipStream_t stream) {
    HPlan P{};
    if (!hb_plan(d, P)) return OTP_ERR_UNSUPPORTED;
    if (((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(wpacked) | reinterpret_cast<uintptr_t>(out) |
          reinterpret_cast<uintptr_t>(res)) & 15) || (reinterpret_cast<uintptr_t>(bias) & 3))
        return OTP_ERR_UNSUPPORTED;
    P.stats = static_cast<float*>(stats);
    P.rflag = nullptr;
    return h16_conv_dispatch<Bf16>(x, wpacked, static_cast<const float*>(bias), res, out, P, d->stride, stream);
}
