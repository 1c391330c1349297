// Convolutions of the bf16 NHWC training path (csrc/nhwc.h): plan, weight packer, kernel and the rule that routes a descriptor.
//
//   nhwc_conv_kernel<MB,NB,K7,PIPE>
//                             implicit GEMM  out[px][co] = sum_{tap,ci} W[co][tap][ci] * x[px+tap][ci]   (forward and,
//                             with flipped / transposed weights, the input gradient); the epilogue also leaves the
//                             per-tile sum / sum of squares of every output channel (BatchNorm batch statistics)
#include <stdlib.h>

#include "nhwc.h"
#include "hb.h"
#include <cstring>

namespace {

// ---------------------------------------------------------------------------------------------------------------------
// plan: a pure function of the descriptor (host), shared by the packer and the launcher
// ---------------------------------------------------------------------------------------------------------------------
struct ConvPlan {
    int N, H, W, Cin, CinS, Ho, Wo, Cout, CoutS, kh, kw, stride, pad, dil, out_mode;
    int CK, CK8, CKp, nChunks, KGc, KS;      // channels per chunk, k-groups (8 channels of one tap) and k-steps per chunk
    int MB, NB, BM, nM, P, tilesPerImg;
    int RW, rowsMax;
    int ldsW, ldsX, ldsTab, lds;
    int pipe;                                 // the chunk pipeline of nhwc_conv_kernel applies (see there)
    size_t wbytes;
};

// sizes everything for a given (channels per chunk, N-blocks per wave); false when the LDS image does not fit
bool size_plan(const otp_nhwc_conv_desc* d, ConvPlan* p, int ck, int nb) {
    const int taps = d->kh * d->kw;
    p->H = d->H, p->W = d->W;
    p->Ho = (d->H + 2 * d->pad - d->dil * (d->kh - 1) - 1) / d->stride + 1;
    p->Wo = (d->W + 2 * d->pad - d->dil * (d->kw - 1) - 1) / d->stride + 1;
    p->CK = ck, p->CK8 = ck / 8;
    p->CKp = (p->CK8 & 1) ? ck : ck + 8;        // pixel stride of the LDS window: an odd multiple of 16 bytes
    p->nChunks = (p->CinS + ck - 1) / ck;
    p->KGc = taps * p->CK8;
    p->KS = (p->KGc + 3) / 4;
    const int npx = p->Ho * p->Wo;
    p->NB = nb;
    p->P = 64 * nb;
    p->tilesPerImg = (npx + p->P - 1) / p->P;
    // a pointwise conv sees the image as rows of W' pixels, W' the largest divisor of H*W that is <= the tile size (and a
    // multiple of 8): a tile's window is then (nearly) the tile itself instead of the full-width image rows it touches -
    // (B, C, T) sequences enter as H = 1, W = T
    if (taps == 1 && d->stride == 1 && d->pad == 0) {
        int w1 = 0;
        for (int cand = p->P; cand >= 32; cand -= 8)
            if (npx % cand == 0) { w1 = cand; break; }
        if (w1) {
            p->W = p->Wo = w1;
            p->H = p->Ho = npx / w1;
        }
    }
    const int need = (p->Wo - 1) * d->stride + (d->kw - 1) * d->dil + 1;
    p->RW = p->W + 2 * d->pad > need ? p->W + 2 * d->pad : need;
    int rowsOut = p->Wo % p->P == 0 ? 1 : (p->P % p->Wo == 0 ? p->P / p->Wo : (p->P - 1 + p->Wo - 1) / p->Wo + 1);
    if (rowsOut > p->Ho) rowsOut = p->Ho;
    p->rowsMax = (rowsOut - 1) * d->stride + (d->kh - 1) * d->dil + 1;
    p->ldsW = p->KS * 4 * p->BM * 16;
    p->ldsX = round_up(p->rowsMax * p->RW * p->CKp * 2, 16);
    const int outTile = p->P * (p->BM + 8) * 2;                 // the epilogue's [pixel][channel] image reuses the operand space
    if (p->ldsW + p->ldsX < outTile) p->ldsX = outTile - p->ldsW;
    p->ldsTab = round_up(p->KS * 4 * 4, 16);
    p->lds = p->ldsW + p->ldsX + p->ldsTab + 4 * 2 * p->BM * 4;
    p->wbytes = (size_t)p->nChunks * p->nM * p->ldsW;
    {
        // chunk pipeline: 256 threads hold one chunk's window (one (column, channel group) unit x 8 rows per thread, 256 / units-per-
        // row row groups) and weight slab (PIPE_WU(MB) 16-byte units per thread) in registers
        const int rowUnits = p->RW * p->CK8;
        static const int min_chunks = getenv("OTP_NHWC_PIPE_MIN_CHUNKS") ? atoi(getenv("OTP_NHWC_PIPE_MIN_CHUNKS")) : 3;
        p->pipe = p->KS == 7 && p->nChunks >= min_chunks && rowUnits <= 256 && p->rowsMax <= 8 * (256 / rowUnits) &&
                  p->ldsW / 16 <= 256 * ((448 * (p->BM / 16) + 255) / 256);
    }
    return p->lds <= OTP_LDS_LIMIT;
}

bool make_plan(const otp_nhwc_conv_desc* d, ConvPlan* p) {
    if (!valid_desc(d)) return false;
    p->N = d->N, p->Cin = d->Cin, p->Cout = d->Cout;
    p->kh = d->kh, p->kw = d->kw, p->stride = d->stride, p->pad = d->pad, p->dil = d->dil, p->out_mode = d->out_mode;
    p->CinS = round_up(d->Cin, 8), p->CoutS = round_up(d->Cout, 8);
    const int ho = (d->H + 2 * d->pad - d->dil * (d->kh - 1) - 1) / d->stride + 1;
    const int wo = (d->W + 2 * d->pad - d->dil * (d->kw - 1) - 1) / d->stride + 1;
    if (ho <= 0 || wo <= 0) return false;
    // channels per chunk: 24 keeps the per-chunk weight slab small enough for 3-4 workgroups per CU
    const int taps = d->kh * d->kw;
    int ck = p->CinS <= 24 ? p->CinS : 24;
    if (taps == 1) {
        // pointwise: one chunk when the channels fit (136 = the temporal encoders' width), else equal chunks of 136 / 72 / 40
        if (p->CinS <= 144) ck = p->CinS;
        else if (p->CinS % 136 == 0) ck = 136;
        else if (p->CinS % 72 == 0) ck = 72;
        else ck = p->CinS % 40 == 0 ? 40 : (p->CinS % 24 == 0 ? 24 : 40);
    }
    const int c16 = round_up(d->Cout, 16);
    int bm = c16 <= 96 ? c16 : 96;
    if (c16 > 96 && c16 % 96 != 0 && c16 % 64 == 0) bm = 64;
    if (taps == 1 && c16 > 96) {                                // pointwise: up to 9 M-blocks, least padding first
        int best = 1 << 30;
        for (int cand = 144; cand >= 96; cand -= 16) {
            const int padded = (c16 + cand - 1) / cand * cand;
            if (padded < best) best = padded, bm = cand;
        }
    }
    p->BM = bm, p->MB = bm / 16, p->nM = (c16 + bm - 1) / bm;
    const int npx = ho * wo;
    // 256-pixel tiles (4 N-blocks per wave: 10 LDS fragment reads per 24 MFMAs at MB = 6 instead of 8 per 12) when that
    // still leaves >= 4 workgroups per CU to balance; 128-pixel tiles otherwise
    int nb = ((long)d->N * ((npx + 255) / 256) * p->nM >= 1024) ? 4 : 2;
    if (p->MB > 6) nb = 2;                                      // 7-9 M-blocks: 72 accumulator registers at NB = 2
    static const int nb_env = getenv("OTP_NHWC_NB") ? atoi(getenv("OTP_NHWC_NB")) : 0;      // tuning override (2 or 4)
    if (nb_env && p->MB <= 6) nb = nb_env;
    // candidates in order of preference; later ones shrink the LDS image (widely dilated taps on wide maps stage many rows)
    if (size_plan(d, p, ck, nb) && (taps > 1 || nb == 2 || p->lds <= 72 * 1024)) return true;
    if (nb == 4 && size_plan(d, p, ck, 2)) return true;
    if (ck > 8 && size_plan(d, p, 8, 2)) return true;
    return false;
}

}  // namespace

bool nhwc_conv_geom(const otp_nhwc_conv_desc* d, NhwcGeom* g) {
    ConvPlan c;
    if (!make_plan(d, &c)) return false;
    g->N = c.N, g->H = c.H, g->W = c.W, g->CinS = c.CinS, g->Ho = c.Ho, g->Wo = c.Wo, g->CoutS = c.CoutS;
    g->Cin = c.Cin, g->Cout = c.Cout, g->kh = c.kh, g->kw = c.kw, g->stride = c.stride, g->pad = c.pad, g->dil = c.dil;
    return true;
}

// tool interface of nhwc_conv_kernel: its plan for the descriptor, whichever kernel the route picks
extern "C" int otp_nhwc_conv_plan(const otp_nhwc_conv_desc* d, int* out8) {
    ConvPlan p;
    if (!out8) return OTP_ERR_BAD_ARG;
    if (!make_plan(d, &p)) return OTP_ERR_UNSUPPORTED;
    out8[0] = p.MB, out8[1] = p.NB, out8[2] = p.CK, out8[3] = p.nChunks, out8[4] = p.nM, out8[5] = p.N * p.tilesPerImg * p.nM;
    out8[6] = p.lds, out8[7] = p.KS;
    return OTP_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// route: which kernel runs a descriptor
// ---------------------------------------------------------------------------------------------------------------------
namespace {
// Which kernel runs a descriptor, and the sizes that follow from it.  Every otp_nhwc_conv_* entry point below reads ONE resolve() of
// its descriptor, so the byte count, the statistics rows, the packer and the launch cannot disagree.
//
// hb 3x3: 3x3 / pad 1 / stride 1 or 2 convolutions with Cin % 16 == 0 run on csrc/hb.hip's window kernel (csrc/h16_kernels.h, the fp16 engine's conv,
// instantiated for bfloat16 NHWC tensors: whole-Cin window by LDS-DMA, weights streamed through registers, three workgroups per CU) where that is
// faster than nhwc_conv_kernel (otp_hb_pays: 96 / 192-channel branches, the stride-2 fuse convs).
//
// hb pointwise: every 1x1 convolution the pointwise kernel of csrc/hb.hip covers - the two projections of a TransformerBlock's MLP on
// (N, 1, T, C) sequences, HRNet's bottleneck / fuse 1x1s, and their input gradients (the input register-resident, the weights
// streamed through the LDS): nhwc_conv_kernel re-stages 46 KB of weights per 128-token tile and 136-channel chunk with one workgroup
// per CU (134 / 214 us per projection at cfg2).  Image-shaped 1x1 layers pay too: forward / input gradient at 80 frames
// (tools/bf16_conv_bench.py, OTPOSE_NHWC_HB=2 against =0) 256 -> 64 @96x72 80.8 / 94.2 us against 174 / 141, 64 -> 256 106.7 / 81.7
// against 156 / 176, 96 -> 48 @48x36 12.1 against 30.0, 384 -> 48 @12x9 8.9 against 31.7 - every shape measured.
//
// OTPOSE_NHWC_HB=0 keeps every layer on nhwc_conv_kernel, =2 sends every shape the window kernel covers to it, whether it pays or not
// (A/B, tests); OTPOSE_NHWC_HBPW=0 turns only the pointwise kernel off.  Both are read per call: the tests switch them inside one
// process.
enum { ROUTE_NONE = -1, ROUTE_PLAIN = 0, ROUTE_HB = 1, ROUTE_HBPW = 2 };      // (the non-negative values are PackJob::hb)
struct NhwcRoute {
    int kind;
    ConvPlan plan;                     // ROUTE_PLAIN only
    size_t wbytes;                     // packed bf16 weights
    int rows;                          // per-tile statistics rows
};

void resolve(const otp_nhwc_conv_desc* d, NhwcRoute* r) {
    r->kind = ROUTE_NONE, r->wbytes = 0, r->rows = 0;
    if (!valid_desc(d)) return;
    const char* e = getenv("OTPOSE_NHWC_HB");
    const char* e2 = getenv("OTPOSE_NHWC_HBPW");
    const int mode = e ? atoi(e) : 1;
    if (mode != 0 && (mode == 2 || otp_hb_pays(d)) && otp_hb_supported(d)) {
        const int ntw = otp_hb_ntw(d->Cout), nN = ((d->Cout + 15) / 16 + ntw - 1) / ntw;
        r->kind = ROUTE_HB, r->wbytes = (size_t)nN * (d->Cin / 16) * otp_hb_wb(ntw), r->rows = otp_hb_stats_rows(d);
    } else if (mode != 0 && !(e2 && atoi(e2) == 0) && otp_hbpw_supported(d)) {
        r->kind = ROUTE_HBPW, r->wbytes = (size_t)((d->Cout + 31) / 32) * otp_hbpw_blkb(otp_hbpw_ks(d->Cin));
        r->rows = otp_hbpw_stats_rows(d);
    } else if (make_plan(d, &r->plan)) {
        r->kind = ROUTE_PLAIN, r->wbytes = r->plan.wbytes, r->rows = r->plan.N * r->plan.tilesPerImg;
    }
}
}  // namespace

extern "C" size_t otp_nhwc_conv_weight_bytes(const otp_nhwc_conv_desc* d) {
    NhwcRoute r;
    resolve(d, &r);
    return r.wbytes;
}

extern "C" int otp_nhwc_conv_stats_rows(const otp_nhwc_conv_desc* d) {
    NhwcRoute r;
    resolve(d, &r);
    return r.rows;
}

// ---------------------------------------------------------------------------------------------------------------------
// weight packing: fp32 (O, I, kh, kw) master weights -> bf16 [chunk][m-tile][k-group (KS*4)][BM][8]
// element (o, i, dy, dx) of the EFFECTIVE conv is w[base + o*so + i*si + dy*sdy + dx*sdx] (the input-gradient conv
// reads the same tensor with o <-> i swapped and the taps flipped)
// ---------------------------------------------------------------------------------------------------------------------
namespace {
struct PackJob {                       // one weight re-layout: what pack_unit reads, by value (otp_nhwc_conv_pack) or from a device table
    const float* w;
    bf16* out;
    long so, si, sdy, sdx, base;
    size_t total;                      // packed elements = NhwcRoute::wbytes / 2
    ConvPlan p;                        // hb = 0: the plan of nhwc_conv_kernel; else only Cin / Cout are set
    int hb, hbNTW, hbChunks;           // hb = NhwcRoute::kind; 1: the operator of csrc/hb.hip's 3x3 kernel (layout: csrc/hb.h)
    int hbKS;                          // hb = 2: of its 1x1 kernel, hbKS k-steps
};

// One 16-byte unit (8 consecutive input channels of one (output channel, tap)) of a packed operator: the index arithmetic once per unit,
// the eight weight loads in flight together, one 16-byte store.  This is the ONLY statement of the three packed layouts (hb = 0:
// [chunk][m-tile][k-group (KS*4)][BM][8] of nhwc_conv_kernel; 1 / 2: csrc/hb.h); an element-wise form cost the batched pack 741 us
// at the head of every training step (a dependent scalar load per element, six integer divisions each; 160 iterations per thread
// on the 384 x 384 layers).
__device__ __forceinline__ void pack_unit(const PackJob& jb, size_t unit) {
    const float* __restrict__ w = jb.w;
    long off = -1;                       // offset of the unit's first weight; consecutive input channels are jb.si apart
    int ci0 = 0;
    if (jb.hb == 1) {
        size_t r = unit;
        const int WU = otp_hb_wb(jb.hbNTW) / 16;
        const int u = (int)(r % WU); r /= WU;
        const int chunk = (int)(r % jb.hbChunks), cb = (int)(r / jb.hbChunks);
        int s_, t, lane;
        otp_hb_unit(u, jb.hbNTW, &s_, &t, &lane);
        const int o = otp_row2ch(cb * jb.hbNTW * 16, t, lane & 15, jb.hbNTW, jb.p.Cout);
        const int q = 4 * s_ + (lane >> 4), tap = q >> 1;
        ci0 = chunk * 16 + 8 * (q & 1);
        if (tap <= 8 && o < jb.p.Cout) off = jb.base + o * jb.so + (tap / 3) * jb.sdy + (tap % 3) * jb.sdx;
    } else if (jb.hb == 2) {
        const int units = otp_hbpw_blkb(jb.hbKS) / 16;
        const int blk = (int)(unit / units), u = (int)(unit % units);
        if (u < 2 * jb.hbKS * 64) {
            const int frag = u >> 6, lane = u & 63, m = frag / jb.hbKS, ks = frag - m * jb.hbKS, r16 = lane & 15, kq = lane >> 4;
            const int o = 32 * blk + 8 * (r16 >> 2) + 4 * m + (r16 & 3);
            ci0 = 32 * ks + 8 * kq;
            if (o < jb.p.Cout) off = jb.base + o * jb.so;
        }
    } else {
        const ConvPlan& p = jb.p;
        size_t r = unit;
        const int co = r % p.BM; r /= p.BM;
        const int kg = r % (p.KS * 4); r /= (p.KS * 4);
        const int mt = r % p.nM; r /= p.nM;
        const int ch = (int)r;
        if (kg < p.KGc) {
            const int tap = kg / p.CK8, cgi = kg % p.CK8, o = mt * p.BM + co;
            ci0 = ch * p.CK + cgi * 8;
            if (o < p.Cout) off = jb.base + o * jb.so + (tap / p.kw) * jb.sdy + (tap % p.kw) * jb.sdx;
        }
    }
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (off >= 0 && ci0 + j < jb.p.Cin) ? w[off + (long)(ci0 + j) * jb.si] : 0.f;
    bf16x8 o8;
#pragma unroll
    for (int j = 0; j < 8; ++j) o8[j] = (bf16)v[j];
    *reinterpret_cast<bf16x8*>(jb.out + unit * 8) = o8;
}

// one weight (otp_nhwc_conv_pack): the job arrives by value, the grid strides over its 16-byte units
__global__ __launch_bounds__(1024) void nhwc_pack_one_kernel(PackJob jb) {
    const size_t units = jb.total >> 3;                              // (every layout is whole 16-byte units)
    for (size_t u = blockIdx.x * (size_t)blockDim.x + threadIdx.x; u < units; u += (size_t)gridDim.x * blockDim.x) pack_unit(jb, u);
}

// every weight of a training step in one launch: blockIdx.y = job (the table lives in device memory, its fields arrive
// through the scalar cache), blockIdx.x strides over the job's units
__global__ void nhwc_pack_batch_kernel(const PackJob* __restrict__ jobs) {
    const PackJob& jb = jobs[blockIdx.y];
    const size_t units = jb.total >> 3;
    for (size_t u = blockIdx.x * (size_t)blockDim.x + threadIdx.x; u < units; u += (size_t)gridDim.x * blockDim.x) pack_unit(jb, u);
}

bool make_pack_job(const void* weight, void* wpacked, const otp_nhwc_conv_desc* d, int dgrad, PackJob* jb) {
    NhwcRoute r;
    resolve(d, &r);
    if (r.kind == ROUTE_NONE) return false;
    memset(jb, 0, sizeof(*jb));        // (the caller stores a job as an opaque record: no indeterminate bytes)
    jb->hb = r.kind;
    if (r.kind == ROUTE_PLAIN) jb->p = r.plan;
    jb->p.Cin = d->Cin, jb->p.Cout = d->Cout;
    jb->hbNTW = otp_hb_ntw(d->Cout), jb->hbChunks = d->Cin / 16, jb->hbKS = otp_hbpw_ks(d->Cin);
    const long taps = (long)d->kh * d->kw;
    if (!dgrad) {
        jb->so = d->Cin * taps, jb->si = taps, jb->sdy = d->kw, jb->sdx = 1, jb->base = 0;
    } else {      // original weight is (O = d->Cin, I = d->Cout, kh, kw); this conv maps O -> I with flipped taps
        jb->so = taps, jb->si = (long)d->Cout * taps, jb->sdy = -d->kw, jb->sdx = -1, jb->base = taps - 1;
    }
    jb->total = r.wbytes / 2;
    jb->w = static_cast<const float*>(weight);
    jb->out = static_cast<bf16*>(wpacked);
    return true;
}
}  // namespace

extern "C" int otp_nhwc_conv_pack(const void* weight, void* wpacked, const otp_nhwc_conv_desc* d, int dgrad, void* stream) {
    PackJob jb;
    if (!weight || !wpacked) return OTP_ERR_BAD_ARG;
    if (!make_pack_job(weight, wpacked, d, dgrad, &jb)) return OTP_ERR_UNSUPPORTED;
    // one unit per thread in 1024-thread workgroups: a launch of this size is bound by workgroup dispatch (384 x 384 x 9: 10.1 us
    // from event to event against 12.7 with 256-thread workgroups, profiles/r10_nhwc_route_refactor.txt)
    nhwc_pack_one_kernel<<<(unsigned)(((jb.total >> 3) + 1023) / 1024), 1024, 0, static_cast<hipStream_t>(stream)>>>(jb);
    return otp_launch_status();
}

extern "C" size_t otp_nhwc_conv_pack_job_bytes(void) { return sizeof(PackJob); }

extern "C" int otp_nhwc_conv_pack_job(const void* weight, void* wpacked, const otp_nhwc_conv_desc* d, int dgrad, void* job_host) {
    if (!weight || !wpacked || !job_host) return OTP_ERR_BAD_ARG;
    PackJob jb;
    if (!make_pack_job(weight, wpacked, d, dgrad, &jb)) return OTP_ERR_UNSUPPORTED;
    memcpy(job_host, &jb, sizeof(jb));
    return OTP_OK;
}

extern "C" int otp_nhwc_conv_pack_batch(const void* jobs_device, int n_jobs, void* stream) {
    if (!jobs_device || n_jobs < 0) return OTP_ERR_BAD_ARG;
    if (n_jobs == 0) return OTP_OK;
    // 32 workgroups per job: the largest weight of the path (384 x 384 x 9 -> 1.5 M packed elements) takes ~23 units
    // per thread, a 48 x 48 x 9 one finishes in the first
    nhwc_pack_batch_kernel<<<dim3(32, (unsigned)n_jobs), 256, 0, static_cast<hipStream_t>(stream)>>>(
        static_cast<const PackJob*>(jobs_device));
    return otp_launch_status();
}

// ---------------------------------------------------------------------------------------------------------------------
// implicit-GEMM convolution
// ---------------------------------------------------------------------------------------------------------------------
namespace {
// bias, rounding, store; per-tile channel sums of the ROUNDED values (what BatchNorm will normalise).
// NHWC output: the tile is transposed through LDS (smem is free once every wave has left the MFMA loop) so that it leaves as
// 16-byte stores of whole pixel rows - the accumulator layout (4 channels x 1 pixel per lane) would otherwise issue MB*NB
// 8-byte stores per lane in 32-byte runs, which is store-issue bound (10-16k cycles per workgroup, measured with
// tools/nhwc_timing.py).  Contains workgroup barriers; every thread of the workgroup must call it.
template <int MB, int NB>
__device__ __forceinline__ void conv_epilogue(otp_f32x4 (&acc)[MB][NB], const bool (&valid)[NB], const ConvPlan& p,
                                              const float* __restrict__ bias, const bf16* __restrict__ res,
                                              bf16* __restrict__ out, float* __restrict__ out_f32, float* __restrict__ stats,
                                              unsigned char* smem, float* sRed, int n, int tile, int mt, int p0, int npx) {
    constexpr int BM = MB * 16, P = 64 * NB, BMS = BM + 8;      // LDS row stride: 16-byte aligned, odd multiple of 16 bytes
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, lg = lane >> 4;
    if (p.out_mode == 1) {                                       // fp32 NCHW (hand-over to the fp32 NCHW kernels)
#pragma unroll
        for (int m = 0; m < MB; ++m) {
            const int co = mt * BM + m * 16 + lg * 4;
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) {
                const int pix = p0 + (wave * NB + nb) * 16 + l15;
                if (valid[nb]) {
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (co + r < p.Cout)
                            out_f32[((size_t)n * p.Cout + co + r) * npx + pix] = acc[m][nb][r] + (bias ? bias[co + r] : 0.f);
                }
            }
        }
        return;
    }
    bf16* sOut = reinterpret_cast<bf16*>(smem);
    __syncthreads();                                             // every wave is done with the operand images
#pragma unroll
    for (int m = 0; m < MB; ++m) {
        const int co = mt * BM + m * 16 + lg * 4;
        float bv[4] = {0.f, 0.f, 0.f, 0.f};
        if (bias) {
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (co + r < p.Cout) bv[r] = bias[co + r];
        }
        float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            bf16x4 o;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                o[r] = (bf16)(acc[m][nb][r] + bv[r]);
                const float f = valid[nb] ? bf2f(o[r]) : 0.f;
                s1[r] += f;
                s2[r] += f * f;
            }
            *reinterpret_cast<bf16x4*>(sOut + ((wave * NB + nb) * 16 + l15) * BMS + m * 16 + lg * 4) = o;
        }
        if (stats) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float a = otp_row16_sum(s1[r]), b = otp_row16_sum(s2[r]);
                if (l15 == 0) {
                    sRed[(wave * 2 + 0) * BM + m * 16 + lg * 4 + r] = a;
                    sRed[(wave * 2 + 1) * BM + m * 16 + lg * 4 + r] = b;
                }
            }
        }
    }
    __syncthreads();
    // rows of the tile -> global: (pixel, 8-channel group) units, consecutive threads = consecutive bytes of a pixel row
    int cvalid = p.CoutS - mt * BM;
    if (cvalid > BM) cvalid = BM;
    const int cu8 = cvalid / 8, units = P * cu8;
    const int pmax = min(P, npx - p0);
    for (int u = tid; u < units; u += 256) {
        const int px = u / cu8, cg = u - px * cu8;
        if (px < pmax) {
            const size_t o = ((size_t)n * npx + p0 + px) * p.CoutS + mt * BM + cg * 8;
            bf16x8 v = *reinterpret_cast<const bf16x8*>(sOut + px * BMS + cg * 8);
            if (res) {                                           // out = bf16(conv) + res, rounded once more: what a separate
                const bf16x8 r = *reinterpret_cast<const bf16x8*>(res + o);       // bf16 add kernel would produce
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = (bf16)(bf2f(v[e]) + bf2f(r[e]));
            }
            *reinterpret_cast<bf16x8*>(out + o) = v;
        }
    }
    if (stats) {
        for (int i = tid; i < 2 * BM; i += 256) {
            const int which = i / BM, c = i - which * BM, co = mt * BM + c;
            if (co < p.CoutS) {
                float v = 0.f;
#pragma unroll
                for (int w = 0; w < 4; ++w) v += sRed[(w * 2 + which) * BM + c];
                stats[((size_t)(n * p.tilesPerImg + tile) * 2 + which) * p.CoutS + co] = v;
            }
        }
    }
}

template <int MB, int NB, bool K7, bool PIPE>
__global__ __launch_bounds__(256) void nhwc_conv_kernel(const bf16* __restrict__ x, const bf16* __restrict__ wpk,
                                                         const float* __restrict__ bias, const bf16* __restrict__ res,
                                                         bf16* __restrict__ out, float* __restrict__ out_f32,
                                                         float* __restrict__ stats, ConvPlan p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    bf16* sW = reinterpret_cast<bf16*>(smem);
    bf16* sX = reinterpret_cast<bf16*>(smem + p.ldsW);
    int* sTab = reinterpret_cast<int*>(smem + p.ldsW + p.ldsX);
    float* sRed = reinterpret_cast<float*>(smem + p.ldsW + p.ldsX + p.ldsTab);      // [4 waves][2][BM]
    constexpr int P = 64 * NB, BM = MB * 16;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, lg = lane >> 4;
    int bid = blockIdx.x;
    const int mt = bid % p.nM;
    bid /= p.nM;
    const int tile = bid % p.tilesPerImg, n = bid / p.tilesPerImg;
    const int npx = p.Ho * p.Wo;
    const int p0 = tile * P, p1 = min(p0 + P, npx);
    const int oy0 = p0 / p.Wo, oy1 = (p1 - 1) / p.Wo;
    const int rowLo = oy0 * p.stride - p.pad;
    const int nrows = (oy1 - oy0) * p.stride + (p.kh - 1) * p.dil + 1;

    OTP_STAMP(0);
    // k-group -> element offset inside the window (tap shift + channel group); identical for every chunk
    for (int kg = tid; kg < p.KS * 4; kg += 256) {
        int v = 0;
        if (kg < p.KGc) {
            const int tap = kg / p.CK8, cgi = kg - tap * p.CK8;
            const int dy = tap / p.kw, dx = tap - dy * p.kw;
            v = ((dy * p.dil) * p.RW + dx * p.dil) * p.CKp + cgi * 8;
        }
        sTab[kg] = v;
    }
    int boff[NB];
    bool valid[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
        const int pix = p0 + (wave * NB + nb) * 16 + l15;
        valid[nb] = pix < p1;
        const int pc = valid[nb] ? pix : p1 - 1;
        const int oy = pc / p.Wo, ox = pc - oy * p.Wo;
        boff[nb] = (((oy - oy0) * p.stride) * p.RW + ox * p.stride) * p.CKp;
    }
    otp_f32x4 acc[MB][NB];
#pragma unroll
    for (int m = 0; m < MB; ++m)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) acc[m][nb] = otp_f32x4{0.f, 0.f, 0.f, 0.f};

    const int wunits = p.ldsW / 16;
    const int rowUnits = p.RW * p.CK8;
    const otp_rsrc xres = make_rsrc(x, (size_t)p.N * p.H * p.W * p.CinS * 2);
    OTP_STAMP(1);
    if constexpr (K7 && PIPE) {
        {
            // ---- chunk pipeline (3x3 taps x 24-channel chunks, more than one chunk): the window and the weight slab of chunk c + 1
            // are loaded into REGISTERS while chunk c is multiplied, and go to the LDS between two barriers.  Without it a
            // workgroup's life at 48 -> 48 @96x72 is 29 k cycles for 6 k of MFMA work - load -> LDS store -> barrier -> multiply
            // with nothing in flight, hidden only by the other workgroups of the CU.  No branch around
            // the loads (hipcc would wait for every outstanding load at the join): a load that is not wanted points past its
            // descriptor and returns zeros.
            constexpr int WU = (448 * MB + 255) / 256;                 // 16-byte weight units per thread: 7 k-steps x 4 x BM x 16 B
            const int G = 256 / rowUnits, grp = tid / rowUnits, cu = tid - grp * rowUnits;
            const int col = cu / p.CK8, cgi = cu - col * p.CK8, ix = col - p.pad;
            const bool colIn = grp < G && ix >= 0 && ix < p.W;
            const int ldst = col * p.CKp + cgi * 8;
            const otp_rsrc wres = make_rsrc(wpk, p.wbytes);
            otp_u32x4 xv[8], wv[WU];
            auto issue = [&](int ch) __attribute__((always_inline)) {
                const int c = ch * p.CK + cgi * 8;
                const bool colOK = colIn && ch < p.nChunks && c < p.CinS;
                const int gcol = (ix * p.CinS + c) * 2;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int r = grp * 8 + j, iy = rowLo + r;
                    const bool ok = colOK && r < nrows && iy >= 0 && iy < p.H;
                    xv[j] = bload16(xres, ok ? (n * p.H + iy) * (p.W * p.CinS * 2) + gcol : OTP_OOB);
                }
                const int wbase = (ch * p.nM + mt) * wunits * 16;
#pragma unroll
                for (int i = 0; i < WU; ++i) {
                    const int u = tid + 256 * i;
                    wv[i] = bload16(wres, (u < wunits && ch < p.nChunks) ? wbase + u * 16 : OTP_OOB);
                }
            };
            issue(0);
            for (int ch = 0; ch < p.nChunks; ++ch) {
                if (ch) __syncthreads();                                  // every wave has left the previous chunk's images
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    if (grp < G && grp * 8 + j < nrows) *reinterpret_cast<otp_u32x4*>(sX + (grp * 8 + j) * (p.RW * p.CKp) + ldst) = xv[j];
#pragma unroll
                for (int i = 0; i < WU; ++i)
                    if (tid + 256 * i < wunits) *reinterpret_cast<otp_u32x4*>(reinterpret_cast<unsigned char*>(sW) + (tid + 256 * i) * 16) = wv[i];
                __syncthreads();
                if (ch == 0) OTP_STAMP(2);
                issue(ch + 1);                                            // in flight under this chunk's MFMAs
#pragma unroll
                for (int ks = 0; ks < 7; ++ks) {
                    const int koff = sTab[ks * 4 + lg];
                    bf16x8 a[MB];
#pragma unroll
                    for (int m = 0; m < MB; ++m) a[m] = *reinterpret_cast<const bf16x8*>(sW + ((ks * 4 + lg) * BM + m * 16 + l15) * 8);
#pragma unroll
                    for (int nb = 0; nb < NB; ++nb) {
                        const bf16x8 b = *reinterpret_cast<const bf16x8*>(sX + boff[nb] + koff);
#pragma unroll
                        for (int m = 0; m < MB; ++m) acc[m][nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[m], b, acc[m][nb], 0, 0, 0);
                    }
                }
                if (ch == 0) OTP_STAMP(3);
            }
            OTP_STAMP(4);
            conv_epilogue<MB, NB>(acc, valid, p, bias, res, out, out_f32, stats, smem, sRed, n, tile, mt, p0, npx);
            OTP_STAMP(5);
            return;
        }
    }
    for (int ch = 0; ch < p.nChunks; ++ch) {
        if (ch) __syncthreads();
        // One L2 round trip per chunk: the first 8 weight units AND the first 8 window rows of this thread are all in
        // flight before the first LDS store (weights: one contiguous slab per (chunk, m-tile); window: rows
        // [rowLo, rowLo + nrows) x columns [-pad, RW - pad) x CK channels, zeros outside the image; a thread owns one
        // (column, channel group) and walks the rows, so the column arithmetic is done once per chunk).
        const int wbase = (ch * p.nM + mt) * wunits * 16;
        const int c0 = ch * p.CK;
        otp_u32x4 xv[8];
        // weight slab of this (chunk, m-tile): global -> LDS by the LDS-DMA (the packed slab IS the LDS image: unit i lands at
        // sW + 16 i), no staging registers, no ds_write pass
        for (int u0 = wave * 64; u0 < wunits; u0 += 256)
            if (u0 + lane < wunits)
                __builtin_amdgcn_global_load_lds(
                    (const __attribute__((address_space(1))) void*)(reinterpret_cast<const unsigned char*>(wpk) + wbase + (size_t)(u0 + lane) * 16),
                    (__attribute__((address_space(3))) void*)(reinterpret_cast<unsigned char*>(sW) + u0 * 16), 16, 0, 0);
        const int col0 = tid / p.CK8, cg0 = tid - col0 * p.CK8;
        const int ix0 = col0 - p.pad;
        const bool colOK0 = tid < rowUnits && ix0 >= 0 && ix0 < p.W && c0 + cg0 * 8 < p.CinS;
        const int gcol0 = (ix0 * p.CinS + c0 + cg0 * 8) * 2, ldst0 = col0 * p.CKp + cg0 * 8;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int iy = rowLo + j;
            const bool ok = colOK0 && j < nrows && iy >= 0 && iy < p.H;
            xv[j] = bload16(xres, ok ? (n * p.H + iy) * (p.W * p.CinS * 2) + gcol0 : OTP_OOB);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (tid < rowUnits && j < nrows) *reinterpret_cast<otp_u32x4*>(sX + j * (p.RW * p.CKp) + ldst0) = xv[j];
        // the rest (rows past 8, rows wider than 256 units)
        for (int sub = 0; sub * 256 < rowUnits; ++sub) {
            const int cu = sub * 256 + tid;
            const int col = cu / p.CK8, cgi = cu - col * p.CK8;
            const int ix = col - p.pad, c = c0 + cgi * 8;
            const bool colOK = cu < rowUnits && ix >= 0 && ix < p.W && c < p.CinS;
            const int gcol = (ix * p.CinS + c) * 2, ldst = col * p.CKp + cgi * 8;
            for (int r0 = sub ? 0 : 8; r0 < nrows; r0 += 8) {
                otp_u32x4 v[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int iy = rowLo + r0 + j;
                    const bool ok = colOK && r0 + j < nrows && iy >= 0 && iy < p.H;
                    v[j] = bload16(xres, ok ? (n * p.H + iy) * (p.W * p.CinS * 2) + gcol : OTP_OOB);
                }
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    if (cu < rowUnits && r0 + j < nrows)
                        *reinterpret_cast<otp_u32x4*>(sX + (r0 + j) * (p.RW * p.CKp) + ldst) = v[j];
            }
        }
        __syncthreads();
        if (ch == 0) OTP_STAMP(2);
        auto kstep = [&](int ks) {
            const int koff = sTab[ks * 4 + lg];
            bf16x8 a[MB];
#pragma unroll
            for (int m = 0; m < MB; ++m) a[m] = *reinterpret_cast<const bf16x8*>(sW + ((ks * 4 + lg) * BM + m * 16 + l15) * 8);
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) {
                const bf16x8 b = *reinterpret_cast<const bf16x8*>(sX + boff[nb] + koff);
#pragma unroll
                for (int m = 0; m < MB; ++m) acc[m][nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[m], b, acc[m][nb], 0, 0, 0);
            }
        };
        if constexpr (K7) {               // 3x3 taps x 24 channels: fully unrolled so the LDS reads of step k+1 issue under step k
#pragma unroll
            for (int ks = 0; ks < 7; ++ks) kstep(ks);
        } else {
            for (int ks = 0; ks < p.KS; ++ks) kstep(ks);
        }
        if (ch == 0) OTP_STAMP(3);
    }

    OTP_STAMP(4);
    conv_epilogue<MB, NB>(acc, valid, p, bias, res, out, out_f32, stats, smem, sRed, n, tile, mt, p0, npx);
    OTP_STAMP(5);
}

template <int MB, int NB, bool K7, bool PIPE>
int launch_conv_k(const ConvPlan& p, const void* x, const void* wpk, const void* bias, const void* res, void* out, void* stats,
                  hipStream_t st) {
    auto kern = nhwc_conv_kernel<MB, NB, K7, PIPE>;
    OTP_ALLOW_BIG_LDS(kern, p.lds);
    const int grid = p.N * p.tilesPerImg * p.nM;
    kern<<<grid, 256, p.lds, st>>>(static_cast<const bf16*>(x), static_cast<const bf16*>(wpk), static_cast<const float*>(bias),
                                   static_cast<const bf16*>(res), static_cast<bf16*>(out), static_cast<float*>(out),
                                   static_cast<float*>(stats), p);
    return otp_launch_status();
}

template <int MB, int NB>
int launch_conv(const ConvPlan& p, const void* x, const void* wpk, const void* bias, const void* res, void* out, void* stats,
                hipStream_t st) {
    if (p.KS == 7)
        return p.pipe ? launch_conv_k<MB, NB, true, true>(p, x, wpk, bias, res, out, stats, st)
                      : launch_conv_k<MB, NB, true, false>(p, x, wpk, bias, res, out, stats, st);
    return launch_conv_k<MB, NB, false, false>(p, x, wpk, bias, res, out, stats, st);
}

int launch_route(const NhwcRoute& r, const void* x, const void* wpacked, const void* bias, const void* res, void* out, void* stats,
                 const otp_nhwc_conv_desc* d, hipStream_t st) {
    if (r.kind == ROUTE_NONE) return OTP_ERR_UNSUPPORTED;
    if (res && (d->out_mode != 0 || stats)) return OTP_ERR_BAD_ARG;   // the sum is an NHWC bf16 tensor; statistics are of conv(x)
    if (r.kind == ROUTE_HB) return otp_hb_conv(x, wpacked, bias, res, out, stats, d, st);
    if (r.kind == ROUTE_HBPW) return otp_hbpw_conv(x, wpacked, bias, res, out, stats, d, st);
    const ConvPlan& p = r.plan;
#define OTP_NHWC_CASE(mb, nb) \
    if (p.MB == mb && p.NB == nb) return launch_conv<mb, nb>(p, x, wpacked, bias, res, out, stats, st)
    OTP_NHWC_CASE(1, 2); OTP_NHWC_CASE(2, 2); OTP_NHWC_CASE(3, 2); OTP_NHWC_CASE(4, 2); OTP_NHWC_CASE(5, 2); OTP_NHWC_CASE(6, 2);
    OTP_NHWC_CASE(7, 2); OTP_NHWC_CASE(8, 2); OTP_NHWC_CASE(9, 2);
    OTP_NHWC_CASE(1, 4); OTP_NHWC_CASE(2, 4); OTP_NHWC_CASE(3, 4); OTP_NHWC_CASE(4, 4); OTP_NHWC_CASE(5, 4); OTP_NHWC_CASE(6, 4);
#undef OTP_NHWC_CASE
    return OTP_ERR_UNSUPPORTED;
}
}  // namespace

extern "C" int otp_nhwc_conv_bf16_res(const void* x, const void* wpacked, const void* bias, const void* res, void* out,
                                      void* stats, const otp_nhwc_conv_desc* d, void* stream) {
    if (!x || !wpacked || !out) return OTP_ERR_BAD_ARG;
    NhwcRoute r;
    resolve(d, &r);
    return launch_route(r, x, wpacked, bias, res, out, stats, d, static_cast<hipStream_t>(stream));
}

extern "C" int otp_nhwc_conv_bf16(const void* x, const void* wpacked, const void* bias, void* out, void* stats,
                                  const otp_nhwc_conv_desc* d, void* stream) {
    return otp_nhwc_conv_bf16_res(x, wpacked, bias, nullptr, out, stats, d, stream);
}

// conv + BatchNorm (batch statistics) + residual + ReLU as ONE call (three launches: otp_nhwc_conv_bf16 with statistics,
// otp_nhwc_bn_finalize, otp_nhwc_bn_apply): the training forward issues ~290 of these per step and is bound by the host once a loop
// synchronises every iteration (a ctypes call costs ~4 us of host time).  vec: 4 x CoutS floats (mean, rstd, scale, shift).
extern "C" int otp_nhwc_conv_bn_bf16(const void* x, const void* wpacked, const void* res, void* conv_out, void* stats, void* vec,
                                     const void* gamma, const void* beta, void* running_mean, void* running_var, float eps,
                                     float momentum, void* y, void* relu_mask, int relu, const otp_nhwc_conv_desc* d, void* stream) {
    if (!x || !wpacked || !conv_out || !stats || !vec || !gamma || !beta || !y || !d) return OTP_ERR_BAD_ARG;
    NhwcRoute r;
    resolve(d, &r);
    const int rows = r.rows;
    if (rows <= 0) return OTP_ERR_UNSUPPORTED;
    int rc = launch_route(r, x, wpacked, nullptr, nullptr, conv_out, stats, d, static_cast<hipStream_t>(stream));
    if (rc != OTP_OK) return rc;
    const int CS = (d->Cout + 7) / 8 * 8;
    const int Ho = (d->H + 2 * d->pad - d->dil * (d->kh - 1) - 1) / d->stride + 1, Wo = (d->W + 2 * d->pad - d->dil * (d->kw - 1) - 1) / d->stride + 1;
    const size_t pixels = (size_t)d->N * Ho * Wo;
    float* v = static_cast<float*>(vec);
    rc = otp_nhwc_bn_finalize(stats, rows, d->Cout, CS, (float)pixels, gamma, beta, v, v + CS, v + 2 * CS, v + 3 * CS, running_mean,
                              running_var, eps, momentum, stream);
    if (rc != OTP_OK) return rc;
    return otp_nhwc_bn_apply(conv_out, v + 2 * CS, v + 3 * CS, res, y, relu_mask, pixels, CS, relu, stream);
}

// The TransformerBlock MLP interior with its element-wise passes folded into the projections' epilogues (csrc/hb.hip's pointwise kernel):
// up: pre = bf16(W1 x + b1) AND act = dropout(gelu(pre), p) (+ keep bits) in one launch; the down-projection's input gradient times
// gelu'(pre) and the dropout factor in one launch.  desc: the (N, 1, T, C) convolution of that launch (for the gradient: the input-gradient
// convolution, channels swapped).  OTP_ERR_UNSUPPORTED when the shape is not on the pointwise kernel - the caller keeps the separate launches.
extern "C" int otp_nhwc_mlp_fused_supported(const otp_nhwc_conv_desc* d) {
    NhwcRoute r;
    resolve(d, &r);
    return (r.kind == ROUTE_HBPW && d->out_mode == 0) ? 1 : 0;
}

extern "C" int otp_nhwc_mlp_up_bf16(const void* x, const void* wpacked, const void* bias, void* pre, void* act, void* keep_bits, float p,
                                    unsigned long long seed, const otp_nhwc_conv_desc* d, void* stream) {
    if (!x || !wpacked || !pre || !act || !keep_bits || !(p >= 0.f) || !(p < 1.f)) return OTP_ERR_BAD_ARG;
    if (!otp_nhwc_mlp_fused_supported(d)) return OTP_ERR_UNSUPPORTED;
    otp_hbpw_epi e{};
    e.mode = 1, e.out2 = act, e.keep = static_cast<unsigned char*>(keep_bits);
    e.s0 = (uint32_t)seed, e.s1 = (uint32_t)(seed >> 32), e.thr = (uint32_t)(p * 65536.f + 0.5f);
    e.scale = 65536.f / (float)(65536u - e.thr);
    return otp_hbpw_conv(x, wpacked, bias, nullptr, pre, nullptr, d, static_cast<hipStream_t>(stream), &e);
}

extern "C" int otp_nhwc_mlp_down_dgrad_bf16(const void* gy, const void* wpacked, const void* pre, const void* keep_bits, void* grad_pre,
                                            float p, const otp_nhwc_conv_desc* d, void* stream) {
    if (!gy || !wpacked || !pre || !keep_bits || !grad_pre || !(p >= 0.f) || !(p < 1.f)) return OTP_ERR_BAD_ARG;
    if (!otp_nhwc_mlp_fused_supported(d)) return OTP_ERR_UNSUPPORTED;
    otp_hbpw_epi e{};
    e.mode = 2, e.aux = pre, e.keep = const_cast<unsigned char*>(static_cast<const unsigned char*>(keep_bits));
    e.thr = (uint32_t)(p * 65536.f + 0.5f);
    e.scale = 65536.f / (float)(65536u - e.thr);
    return otp_hbpw_conv(gy, wpacked, nullptr, nullptr, grad_pre, nullptr, d, static_cast<hipStream_t>(stream), &e);
}
