// Weight gradients of the bf16 NHWC training path (csrc/nhwc.h), fp32 results.
//
//   nhwc_wgrad_kernel         dW[co][tap][ci] = sum_px gy[px][co] * x[px+tap][ci]: both operands are read from their
//                             [pixel][channel] LDS images with ds_read_b64_tr_b16 (the hardware transpose read), so the
//                             contraction index (pixels) lands in the fragment's k slots without a transposed copy
//   nhwc_wgrad1x1_kernel      the same for 1x1 / stride 1 layers, the idle (tap, ci) slots carrying more output channels
//   nhwc_wgrad_reduce_kernel  folds the per-split partial sums and scatters them to (Cout, Cin, kh, kw)
#include <stdlib.h>

#include "nhwc.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------------
// weight gradient
// ---------------------------------------------------------------------------------------------------------------------
// A workgroup owns (co block of up to 48) x (ci block of 16*cbw channels: 48 for 3x3 kernels, up to 192 for 1x1) x all taps
// and a contiguous range of pixel tiles of
// TPX output pixels (TPX / 32 k-steps per staged tile); wave w owns N-blocks {w, w+4, ...} of the (tap, ci16) list for all
// 3 co blocks.  The gy tile [TPX px][48 co] and the x window live in LDS as [pixel][channel]; a fragment is two
// ds_read_b64_tr_b16 (4 pixels x 16 channels each).
struct WgradPlan {
    int N, H, W, CinS, Ho, Wo, CoutS, Cin, Cout, kh, kw, stride, pad, dil;
    int nCo, nCi, splits, tilesPerImg, tilesTotal, tilesPerSplit, TPX;
    int RW, rowsMax, XC, ldsG, ldsX, lds;
    int tapmode;           // 1: the LDS image of x is [tap][tile pixel][XC] (each tap's shifted copy of the tile) instead of a window of rows
    int nbTot, cbw;        // N-blocks per workgroup = taps * cbw; cbw = 16-channel blocks of ci per workgroup (3 for 3x3 taps)
    int cg, spg;           // 1x1 kernels (nhwc_wgrad1x1_kernel): 48-channel co groups per workgroup, ci-block slots per wave and group; 0: not used
};

__device__ __forceinline__ bf16x4 tr_read(const bf16* p) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
        (__attribute__((address_space(3))) bf16x4*)(const_cast<bf16*>(p)));
}

constexpr int WG_NBW = 7;      // N-blocks per wave (27 = 9 taps x 3 ci blocks over 4 waves)

constexpr int WG_GU = 3;       // gy units of 16 B per thread per tile (TPX * 6 / 256 at TPX = 128)
constexpr int WG_XU = 10;      // x window units per thread per tile that the prefetch path holds in registers

// PF = true: the loads of tile t+1 (gy tile + x window, at most WG_GU + WG_XU 16-byte units per thread) are issued right
// after tile t has been written to LDS and complete under its MFMAs; the unit -> (row, column, channel group)
// decomposition is computed once per thread.  PF = false: the general form (windows too large for the registers).
template <bool PF>
__global__ __launch_bounds__(256) void nhwc_wgrad_kernel(const bf16* __restrict__ x, const bf16* __restrict__ gy,
                                                          float* __restrict__ part, WgradPlan p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    bf16* sG = reinterpret_cast<bf16*>(smem);                 // [TPX px][56] (48 channels + 8 pad: row stride 112 B)
    bf16* sX = reinterpret_cast<bf16*>(smem + p.ldsG);        // [rows][RW][XC]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, lg = lane >> 4;
    int bid = blockIdx.x;
    const int split = bid % p.splits;
    bid /= p.splits;
    const int blk = bid;
    const int cib = bid % p.nCi, cob = bid / p.nCi;
    const int co0 = cob * 48, ci0 = cib * 16 * p.cbw;
    const int npx = p.Ho * p.Wo;
    const int TPX = p.TPX;

    // this wave's N-blocks: nb = wave + 4*i  ->  (tap, ci16 block)
    int xoff[WG_NBW];          // element offset inside the x window of (tap shift, ci block)
#pragma unroll
    for (int i = 0; i < WG_NBW; ++i) {
        const int nb = wave + 4 * i;
        const int nbc = nb < p.nbTot ? nb : 0;
        const int tap = nbc / p.cbw, cb = nbc - tap * p.cbw;
        const int dy = tap / p.kw, dx = tap - dy * p.kw;
        xoff[i] = (p.tapmode ? tap * p.TPX : (dy * p.dil) * p.RW + dx * p.dil) * p.XC + cb * 16;
    }
    otp_f32x4 acc[3][WG_NBW];
#pragma unroll
    for (int m = 0; m < 3; ++m)
#pragma unroll
        for (int i = 0; i < WG_NBW; ++i) acc[m][i] = otp_f32x4{0.f, 0.f, 0.f, 0.f};

    // transpose-read addressing: within a 16-lane group, lane 4q+pp supplies row q (pixel), columns 4pp..4pp+3 (channels)
    const int q = l15 >> 2, pp = l15 & 3;
    const int xcu = p.XC / 8 - 1;                             // channel groups that carry data (the last 8 are zero padding)
    const int gunits = TPX * 6;
    const int rowUnits = p.RW * xcu;
    const otp_rsrc xres = make_rsrc(x, (size_t)p.N * p.H * p.W * p.CinS * 2);
    const otp_rsrc gres = make_rsrc(gy, (size_t)p.N * npx * p.CoutS * 2);

    // the padding channel group of every window pixel is zero for the whole kernel
    for (int i = tid; i < (p.tapmode ? p.kh * p.kw * p.TPX : p.rowsMax * p.RW); i += 256)
        *reinterpret_cast<otp_u32x4*>(sX + (size_t)i * p.XC + xcu * 8) = otp_u32x4{0u, 0u, 0u, 0u};

    struct Geom {
        int n, p0, p1, oy0, rowLo, nrows;
    };
    auto geom = [&](int t) {
        Geom g;
        g.n = t / p.tilesPerImg;
        const int tile = t - g.n * p.tilesPerImg;
        g.p0 = tile * TPX;
        g.p1 = min(g.p0 + TPX, npx);
        g.oy0 = g.p0 / p.Wo;
        const int oy1 = (g.p1 - 1) / p.Wo;
        g.rowLo = g.oy0 * p.stride - p.pad;
        g.nrows = (oy1 - g.oy0) * p.stride + (p.kh - 1) * p.dil + 1;
        return g;
    };

    // per-thread unit decomposition (tile independent)
    int gpx[WG_GU], gcg[WG_GU];
#pragma unroll
    for (int j = 0; j < WG_GU; ++j) {
        const int u = j * 256 + tid;
        gpx[j] = u / 6;
        gcg[j] = u - gpx[j] * 6;
    }
    int xu[PF ? WG_XU : 1];                                   // packed (row << 24 | column << 8 | channel group)
    if constexpr (PF) {
#pragma unroll
        for (int j = 0; j < WG_XU; ++j) {
            const int u = j * 256 + tid;
            const int r = u / rowUnits, ur = u - r * rowUnits;
            const int col = ur / xcu, cg = ur - col * xcu;
            xu[j] = (r << 24) | (col << 8) | cg;
        }
    }
    otp_u32x4 gv[WG_GU], xv[PF ? WG_XU : 1];
    auto load_g = [&](const Geom& g) {
#pragma unroll
        for (int j = 0; j < WG_GU; ++j) {
            const bool ok = j * 256 + tid < gunits && g.p0 + gpx[j] < g.p1 && co0 + gcg[j] * 8 < p.CoutS;
            gv[j] = bload16(gres, ok ? ((g.n * npx + g.p0 + gpx[j]) * p.CoutS + co0 + gcg[j] * 8) * 2 : OTP_OOB);
        }
    };
    auto load_x = [&](const Geom& g) {
        if constexpr (PF) {
#pragma unroll
            for (int j = 0; j < WG_XU; ++j) {
                const int r = xu[j] >> 24, col = (xu[j] >> 8) & 0xffff, cg = xu[j] & 255;
                const int iy = g.rowLo + r, ix = col - p.pad, c = ci0 + cg * 8;
                const bool ok = r < g.nrows && iy >= 0 && iy < p.H && ix >= 0 && ix < p.W && c < p.CinS;
                xv[j] = bload16(xres, ok ? (((g.n * p.H + iy) * p.W + ix) * p.CinS + c) * 2 : OTP_OOB);
            }
        }
    };

    OTP_STAMP(0);
    const int t0 = split * p.tilesPerSplit, t1 = min(t0 + p.tilesPerSplit, p.tilesTotal);
    Geom g = geom(t0);
    load_g(g);
    load_x(g);
    for (int t = t0; t < t1; ++t) {
        __syncthreads();                                        // the previous tile's fragments have been read
        if (t == t0) OTP_STAMP(1);
#pragma unroll
        for (int j = 0; j < WG_GU; ++j)
            if (j * 256 + tid < gunits) *reinterpret_cast<otp_u32x4*>(sG + gpx[j] * 56 + gcg[j] * 8) = gv[j];
        if constexpr (PF) {
#pragma unroll
            for (int j = 0; j < WG_XU; ++j) {
                const int r = xu[j] >> 24, col = (xu[j] >> 8) & 0xffff, cg = xu[j] & 255;
                if (r < g.nrows) *reinterpret_cast<otp_u32x4*>(sX + (r * p.RW + col) * p.XC + cg * 8) = xv[j];
            }
        } else {
            // general form: flat (row, column, channel group) units - or, in tap mode, (tap, tile pixel, channel group) units:
            // each tap's shifted copy of the tile (widely dilated or strided taps would otherwise drag many full-width rows
            // through LDS) - 8 loads in flight per thread
            if (p.tapmode) {
                const int tunits = p.kh * p.kw * TPX * xcu;
                for (int base = 0; base < tunits; base += 256 * 8) {
                    otp_u32x4 v[8];
                    int dst[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const int u = base + j * 256 + tid;
                        const int tp = u / xcu, cg = u - tp * xcu;
                        const int tap = tp / TPX, px = tp - tap * TPX;
                        const int dy = tap / p.kw, dx = tap - dy * p.kw;
                        const int pc = min(g.p0 + px, g.p1 - 1);
                        const int oy = pc / p.Wo, ox = pc - oy * p.Wo;
                        const int iy = oy * p.stride - p.pad + dy * p.dil, ix = ox * p.stride - p.pad + dx * p.dil, c = ci0 + cg * 8;
                        dst[j] = u < tunits ? tp * p.XC + cg * 8 : -1;
                        const bool ok = u < tunits && iy >= 0 && iy < p.H && ix >= 0 && ix < p.W && c < p.CinS;
                        v[j] = bload16(xres, ok ? (((g.n * p.H + iy) * p.W + ix) * p.CinS + c) * 2 : OTP_OOB);
                    }
#pragma unroll
                    for (int j = 0; j < 8; ++j)
                        if (dst[j] >= 0) *reinterpret_cast<otp_u32x4*>(sX + dst[j]) = v[j];
                }
            }
            const int xunits = p.tapmode ? 0 : g.nrows * rowUnits;
            for (int base = 0; base < xunits; base += 256 * 8) {
                otp_u32x4 v[8];
                int dst[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int u = base + j * 256 + tid;
                    const int r = u / rowUnits, ur = u - r * rowUnits;
                    const int col = ur / xcu, cg = ur - col * xcu;
                    const int iy = g.rowLo + r, ix = col - p.pad, c = ci0 + cg * 8;
                    dst[j] = u < xunits ? (r * p.RW + col) * p.XC + cg * 8 : -1;
                    const bool ok = u < xunits && iy >= 0 && iy < p.H && ix >= 0 && ix < p.W && c < p.CinS;
                    v[j] = bload16(xres, ok ? (((g.n * p.H + iy) * p.W + ix) * p.CinS + c) * 2 : OTP_OOB);
                }
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    if (dst[j] >= 0) *reinterpret_cast<otp_u32x4*>(sX + dst[j]) = v[j];
            }
        }
        __syncthreads();
        if (t == t0) OTP_STAMP(2);
        const Geom gc = g;
        if (t + 1 < t1) {                                       // next tile's loads fly under this tile's MFMAs
            g = geom(t + 1);
            load_g(g);
            load_x(g);
        }
        // k-steps of 32 pixels: lane group lg covers pixels 8*lg .. 8*lg+7 of the step (two transposed reads of 4 pixels)
        for (int k0 = 0; k0 < TPX; k0 += 32) {
            if (gc.p0 + k0 >= gc.p1) break;                      // uniform: the rest of the tile is past the image
            bf16x8 a[3];
            int xrow[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int px = k0 + 8 * lg + 4 * h + q;
                const int pc = min(gc.p0 + px, gc.p1 - 1);       // rows past the tile pair with zero gy rows
                const int oy = pc / p.Wo, ox = pc - oy * p.Wo;
                xrow[h] = (p.tapmode ? pc - gc.p0 : ((oy - gc.oy0) * p.stride) * p.RW + ox * p.stride) * p.XC + 4 * pp;
            }
#pragma unroll
            for (int m = 0; m < 3; ++m) {
                const bf16x4 lo = tr_read(sG + (k0 + 8 * lg + q) * 56 + m * 16 + 4 * pp);
                const bf16x4 hi = tr_read(sG + (k0 + 8 * lg + 4 + q) * 56 + m * 16 + 4 * pp);
                a[m] = bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
            }
#pragma unroll
            for (int i = 0; i < WG_NBW; ++i) {
                const bf16x4 lo = tr_read(sX + xrow[0] + xoff[i]);
                const bf16x4 hi = tr_read(sX + xrow[1] + xoff[i]);
                const bf16x8 b = bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
#pragma unroll
                for (int m = 0; m < 3; ++m) acc[m][i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[m], b, acc[m][i], 0, 0, 0);
            }
        }
        if (t == t0) OTP_STAMP(3);
    }
    OTP_STAMP(4);
    // partial sums in FRAGMENT order, one 16-byte store per lane and accumulator tile (1 KB per wave instruction):
    // part[split][block][wave][i][m][lane][4]; nhwc_wgrad_reduce_kernel maps them to (Cout, Cin, kh, kw)
    otp_f32x4* dst = reinterpret_cast<otp_f32x4*>(part) + ((size_t)(split * p.nCo * p.nCi + blk) * 4 + wave) * (WG_NBW * 3 * 64);
#pragma unroll
    for (int i = 0; i < WG_NBW; ++i)
#pragma unroll
        for (int m = 0; m < 3; ++m) dst[(i * 3 + m) * 64 + lane] = acc[m][i];
    OTP_STAMP(5);
}

// 1x1 / stride 1 kernels (the TransformerBlock MLP's projections on (N, 1, T, C) sequences, HRNet's bottleneck / fuse 1x1s).  The kernel
// above gives a 1x1 layer taps x cbw = 4 .. 12 of its 28 N-block slots and multiplies garbage in the rest (136 -> 544: 21 MFMAs per
// k-step and wave, 7 of them wanted), and re-stages the x tile once per 48 output channels.  Here the idle slots carry more OUTPUT
// channels: a workgroup owns CG groups of 48 co x all cbw ci blocks, slot i of a wave = (group i / SPG, ci block wave + 4 (i % SPG)) -
// (2, 3) for 9 - 12 ci blocks, (3, 2) for 5 - 8, (4, 1) up to 4 - one B fragment serves CG groups.  Tiles are TPX consecutive pixels of an
// image; both operands are [pixel][channel] LDS images read with the transposing ds_read_b64_tr_b16 as above (rows past the image
// hold zeros: their loads fall off the descriptor).  Partials leave in the same fragment order.
template <int CG, int SPG>
__global__ __launch_bounds__(256) void nhwc_wgrad1x1_kernel(const bf16* __restrict__ x, const bf16* __restrict__ gy,
                                                             float* __restrict__ part, WgradPlan p) {
    constexpr int GC = 48 * CG + 8, NS = CG * SPG;
    static_assert(NS <= WG_NBW, "slots per wave");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    bf16* sG = reinterpret_cast<bf16*>(smem);                 // [TPX px][GC]
    bf16* sX = reinterpret_cast<bf16*>(smem + p.ldsG);        // [TPX px][XC]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, lg = lane >> 4;
    int bid = blockIdx.x;
    const int split = bid % p.splits;
    bid /= p.splits;
    const int blk = bid;
    const int cib = bid % p.nCi, cob = bid / p.nCi;
    const int co0 = cob * 48 * CG, ci0 = cib * 16 * p.cbw;
    const int npx = p.Ho * p.Wo, TPX = p.TPX;
    otp_f32x4 acc[3][NS];
#pragma unroll
    for (int m = 0; m < 3; ++m)
#pragma unroll
        for (int i = 0; i < NS; ++i) acc[m][i] = otp_f32x4{0.f, 0.f, 0.f, 0.f};
    const int q = l15 >> 2, pp = l15 & 3;
    const int xcu = p.XC / 8 - 1, gcu = 6 * CG;
    const int gunits = TPX * gcu, xunits = TPX * xcu;
    const otp_rsrc xres = make_rsrc(x, (size_t)p.N * npx * p.CinS * 2);
    const otp_rsrc gres = make_rsrc(gy, (size_t)p.N * npx * p.CoutS * 2);
    for (int i = tid; i < TPX; i += 256) {                     // padding channel groups: zero for the whole kernel
        *reinterpret_cast<otp_u32x4*>(sX + (size_t)i * p.XC + xcu * 8) = otp_u32x4{0u, 0u, 0u, 0u};
        *reinterpret_cast<otp_u32x4*>(sG + (size_t)i * GC + 48 * CG) = otp_u32x4{0u, 0u, 0u, 0u};
    }
    const int t0 = split * p.tilesPerSplit, t1 = min(t0 + p.tilesPerSplit, p.tilesTotal);
    for (int t = t0; t < t1; ++t) {
        const int n = t / p.tilesPerImg, p0 = (t - n * p.tilesPerImg) * TPX, p1 = min(p0 + TPX, npx);
        __syncthreads();                                        // the previous tile's fragments have been read
        for (int base = 0; base < gunits; base += 256 * 8) {
            otp_u32x4 v[8];
            int dst[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int u = base + j * 256 + tid;
                const int px = u / gcu, cgi = u - px * gcu;
                dst[j] = u < gunits ? px * GC + cgi * 8 : -1;
                const bool ok = u < gunits && p0 + px < p1 && co0 + cgi * 8 < p.CoutS;
                v[j] = bload16(gres, ok ? ((n * npx + p0 + px) * p.CoutS + co0 + cgi * 8) * 2 : OTP_OOB);
            }
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (dst[j] >= 0) *reinterpret_cast<otp_u32x4*>(sG + dst[j]) = v[j];
        }
        for (int base = 0; base < xunits; base += 256 * 8) {
            otp_u32x4 v[8];
            int dst[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int u = base + j * 256 + tid;
                const int px = u / xcu, cgi = u - px * xcu;
                dst[j] = u < xunits ? px * p.XC + cgi * 8 : -1;
                const bool ok = u < xunits && p0 + px < p1 && ci0 + cgi * 8 < p.CinS;
                v[j] = bload16(xres, ok ? ((n * npx + p0 + px) * p.CinS + ci0 + cgi * 8) * 2 : OTP_OOB);
            }
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (dst[j] >= 0) *reinterpret_cast<otp_u32x4*>(sX + dst[j]) = v[j];
        }
        __syncthreads();
        for (int k0 = 0; k0 < TPX; k0 += 32) {
            if (p0 + k0 >= p1) break;                           // uniform: the rest of the tile is past the image
            const int r0 = k0 + 8 * lg + q;                     // the lane's pixel row of the two transposed reads (r0, r0 + 4)
            bf16x8 a[CG][3];
#pragma unroll
            for (int g = 0; g < CG; ++g)
#pragma unroll
                for (int m = 0; m < 3; ++m) {
                    const bf16x4 lo = tr_read(sG + r0 * GC + g * 48 + m * 16 + 4 * pp);
                    const bf16x4 hi = tr_read(sG + (r0 + 4) * GC + g * 48 + m * 16 + 4 * pp);
                    a[g][m] = bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                }
#pragma unroll
            for (int j = 0; j < SPG; ++j) {
                const int xo = (wave + 4 * j) * 16 + 4 * pp;    // (a block past the layer's channels: finite neighbours, discarded)
                const bf16x4 lo = tr_read(sX + r0 * p.XC + xo);
                const bf16x4 hi = tr_read(sX + (r0 + 4) * p.XC + xo);
                const bf16x8 b = bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
#pragma unroll
                for (int g = 0; g < CG; ++g)
#pragma unroll
                    for (int m = 0; m < 3; ++m)
                        acc[m][g * SPG + j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[g][m], b, acc[m][g * SPG + j], 0, 0, 0);
            }
        }
    }
    otp_f32x4* dst = reinterpret_cast<otp_f32x4*>(part) + ((size_t)(split * p.nCo * p.nCi + blk) * 4 + wave) * (WG_NBW * 3 * 64);
#pragma unroll
    for (int i = 0; i < NS; ++i)
#pragma unroll
        for (int m = 0; m < 3; ++m) dst[(i * 3 + m) * 64 + lane] = acc[m][i];
}

// gw[co][ci][tap] = sum over splits of the fragment-ordered partials.  Threads walk the FRAGMENT order (coalesced reads of
// the splits x fragments slab, 4 split lanes per fragment element, 8 loads in flight) and scatter the few results.
__global__ __launch_bounds__(256) void nhwc_wgrad_reduce_kernel(const float* __restrict__ part, float* __restrict__ gw, WgradPlan p,
                                                                 size_t frag_total) {
    __shared__ float red[4][64];
    const int e = threadIdx.x & 63, sl = threadIdx.x >> 6;
    const size_t f = blockIdx.x * (size_t)64 + e;
    float s = 0.f;
    if (f < frag_total) {
        int k = sl;
        for (; k + 28 < p.splits; k += 32) {
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = part[(size_t)(k + 4 * j) * frag_total + f];
#pragma unroll
            for (int j = 0; j < 8; ++j) s += v[j];
        }
        for (; k < p.splits; k += 4) s += part[(size_t)k * frag_total + f];
    }
    red[sl][e] = s;
    __syncthreads();
    if (sl == 0 && f < frag_total) {
        // f = (((blk*4 + wave)*WG_NBW + i)*3 + m)*256 + lane*4 + r
        const int r = (int)(f & 3), lane = (int)((f >> 2) & 63);
        size_t q = f >> 8;
        const int m = (int)(q % 3); q /= 3;
        const int i = (int)(q % WG_NBW); q /= WG_NBW;
        const int wave = (int)(q & 3);
        const int blk = (int)(q >> 2);
        const int cib = blk % p.nCi, cob = blk / p.nCi;
        const int nb = wave + 4 * i;
        if (p.cg > 0) {                                          // nhwc_wgrad1x1_kernel: slot i = (co group i / spg, ci block wave + 4 (i % spg))
            const int g = i / p.spg, cb = wave + 4 * (i - g * p.spg);
            const int co = (cob * p.cg + g) * 48 + m * 16 + (lane >> 4) * 4 + r, ci = cib * 16 * p.cbw + cb * 16 + (lane & 15);
            if (i < p.cg * p.spg && cb < p.cbw && co < p.Cout && ci < p.Cin)
                gw[(size_t)co * p.Cin + ci] = red[0][e] + red[1][e] + red[2][e] + red[3][e];
        } else if (nb < p.nbTot) {
            const int tap = nb / p.cbw, cb = nb - tap * p.cbw;
            const int co = cob * 48 + m * 16 + (lane >> 4) * 4 + r, ci = cib * 16 * p.cbw + cb * 16 + (lane & 15);
            if (co < p.Cout && ci < p.Cin)
                gw[((size_t)co * p.Cin + ci) * (p.kh * p.kw) + tap] = red[0][e] + red[1][e] + red[2][e] + red[3][e];
        }
    }
}

bool make_wgrad_plan(const otp_nhwc_conv_desc* d, WgradPlan* p) {
    NhwcGeom c;
    if (!nhwc_conv_geom(d, &c)) return false;
    p->N = c.N, p->H = c.H, p->W = c.W, p->CinS = c.CinS, p->Ho = c.Ho, p->Wo = c.Wo, p->CoutS = c.CoutS;
    p->Cin = c.Cin, p->Cout = c.Cout, p->kh = c.kh, p->kw = c.kw, p->stride = c.stride, p->pad = c.pad, p->dil = c.dil;
    const int taps = c.kh * c.kw;
    if (taps * 1 > 4 * WG_NBW) return false;                   // up to 28 (tap, 16-channel) blocks per workgroup
    // ci blocks of 16 channels per workgroup: fill the 28 N-block slots (3 for 3x3 kernels, up to 12 = 192 channels for 1x1)
    int cbw = (4 * WG_NBW) / taps;
    if (cbw > 12) cbw = 12;
    if (cbw > (c.CinS + 15) / 16) cbw = (c.CinS + 15) / 16;
    p->cbw = cbw;
    p->nCo = (c.Cout + 47) / 48, p->nCi = (c.Cin + 16 * cbw - 1) / (16 * cbw);
    p->nbTot = taps * cbw;
    p->cg = p->spg = 0;
    {
        const char* e = getenv("OTPOSE_WGRAD1X1");                 // (=0: 1x1 layers on the general kernel; A/B, tests)
        if (taps == 1 && c.stride == 1 && c.pad == 0 && !(e && atoi(e) == 0)) {
            p->spg = (cbw + 3) / 4;                                  // 1 .. 3
            const int cgmax = p->spg == 1 ? 4 : (p->spg == 2 ? 3 : 2);
            p->cg = p->nCo < cgmax ? p->nCo : cgmax;
            if (p->cg < 2) p->cg = p->spg = 0;                       // <= 48 output channels: nothing to add to the general kernel
            else p->nCo = (c.Cout + 48 * p->cg - 1) / (48 * p->cg);
        }
    }
    // a pointwise conv sees the image as rows of 128 / 64 / 32 pixels (when that divides it): a tile's window is then the
    // tile itself instead of the full-width image rows it touches
    if (taps == 1 && c.stride == 1 && c.pad == 0) {
        const int npx1 = c.H * c.W;
        for (int w1 = 128; w1 >= 32; w1 >>= 1)
            if (npx1 % w1 == 0) {
                p->W = p->Wo = c.W = c.Wo = w1;
                p->H = p->Ho = c.H = c.Ho = npx1 / w1;
                break;
            }
    }
    const int npx = c.Ho * c.Wo;
    const int need = (c.Wo - 1) * c.stride + (c.kw - 1) * c.dil + 1;
    p->RW = c.W + 2 * c.pad > need ? c.W + 2 * c.pad : need;
    // window pixel stride: the ci block's channels + 8 zero channels (odd multiple of 16 bytes).  N-blocks past the real
    // channels read neighbouring pixels (finite, discarded): 128 bytes of slack.
    p->XC = 8 * (c.CinS / 8 < 2 * cbw ? c.CinS / 8 : 2 * cbw) + 8;
    // pixels per staged tile: the largest of 128 / 64 / 32 whose LDS image leaves room for two workgroups per CU, else
    // the largest that fits at all (full-width input rows make the window of wide strided layers large)
    bool found = false;
    p->tapmode = 0;
    for (int pass = 0; pass < 2 && !found; ++pass)
        for (int tpx = 128; tpx >= 32 && !found; tpx >>= 1) {
            // output rows a tile can touch (tiles start at multiples of tpx: aligned tiles never straddle a row)
            int rowsOut = c.Wo % tpx == 0 ? 1 : (tpx % c.Wo == 0 ? tpx / c.Wo : (tpx - 1 + c.Wo - 1) / c.Wo + 1);
            if (rowsOut > c.Ho) rowsOut = c.Ho;
            const int rows = (rowsOut - 1) * c.stride + (c.kh - 1) * c.dil + 1;
            const int ldsG = tpx * (p->cg > 0 ? 48 * p->cg + 8 : 56) * 2;
            const int winX = round_up(rows * p->RW * p->XC * 2, 16) + 128, tapX = taps * tpx * p->XC * 2 + 128;
            const int limit = pass == 0 ? 80 * 1024 : OTP_LDS_LIMIT;
            // the window of rows unless each tap's copy of the tile is smaller (wide dilations, strided wide maps)
            const bool tapm = taps > 1 && tapX < winX;
            const int ldsX = p->cg > 0 ? tpx * p->XC * 2 + 128 : (tapm ? tapX : winX);      // (1x1 kernel: the tile itself)
            if (ldsG + ldsX <= limit) {
                p->TPX = tpx, p->rowsMax = rows, p->ldsG = ldsG, p->ldsX = ldsX, p->lds = ldsG + ldsX, p->tapmode = tapm;
                found = true;
            }
        }
    if (!found) return false;
    p->tilesPerImg = (npx + p->TPX - 1) / p->TPX;
    p->tilesTotal = c.N * p->tilesPerImg;
    // workgroups aimed at = the 512 that are resident at once (two per CU: ~55 KB of LDS, ~200 registers): one full round instead of
    // 1.5 (768 until round 5) and a third fewer partial sums to write and fold - 96 -> 96 @48x36: 71.8 -> 61.3 us, 192 -> 192 @24x18:
    // 72.8 -> 57.3, 64 -> 64 @96x72: 182 -> 155, 64 -> 256 1x1: 129 -> 102 (OTPOSE_WGRAD_SPLITS: tuning override)
    static const int budget = getenv("OTPOSE_WGRAD_SPLITS") ? atoi(getenv("OTPOSE_WGRAD_SPLITS")) : 512;
    int splits = budget / (p->nCo * p->nCi);
    if (splits < 1) splits = 1;
    if (splits > p->tilesTotal) splits = p->tilesTotal;
    if (splits > 512) splits = 512;
    p->tilesPerSplit = (p->tilesTotal + splits - 1) / splits;
    p->splits = (p->tilesTotal + p->tilesPerSplit - 1) / p->tilesPerSplit;
    return true;
}

}  // namespace

extern "C" size_t otp_nhwc_wgrad_workspace(const otp_nhwc_conv_desc* d) {
    WgradPlan p;
    if (!make_wgrad_plan(d, &p)) return 0;
    return (size_t)p.splits * p.nCo * p.nCi * 4 * WG_NBW * 3 * 256 * sizeof(float);
}

extern "C" int otp_nhwc_wgrad_bf16(const void* x, const void* gy, void* grad_weight, void* workspace, size_t workspace_bytes,
                                   const otp_nhwc_conv_desc* d, void* stream) {
    WgradPlan p;
    if (!x || !gy || !grad_weight || !workspace) return OTP_ERR_BAD_ARG;
    if (!make_wgrad_plan(d, &p)) return OTP_ERR_UNSUPPORTED;
    if (workspace_bytes < otp_nhwc_wgrad_workspace(d)) return OTP_ERR_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    // register prefetch of the next tile when the window fits WG_XU units per thread
    const int xunits = p.rowsMax * p.RW * (p.XC / 8 - 1);
    const bool pf = !p.tapmode && xunits <= WG_XU * 256 && p.TPX * 6 <= WG_GU * 256;
    const int grid = p.nCo * p.nCi * p.splits;
    if (p.cg > 0) {
#define OTP_W1_CASE(CG_, SPG_)                                                                                                  \
    if (p.cg == CG_ && p.spg == SPG_) {                                                                                         \
        OTP_ALLOW_BIG_LDS((nhwc_wgrad1x1_kernel<CG_, SPG_>), p.lds);                                                            \
        nhwc_wgrad1x1_kernel<CG_, SPG_><<<grid, 256, p.lds, st>>>(static_cast<const bf16*>(x), static_cast<const bf16*>(gy),   \
                                                                  static_cast<float*>(workspace), p);                          \
    }
        OTP_W1_CASE(2, 1) OTP_W1_CASE(3, 1) OTP_W1_CASE(4, 1) OTP_W1_CASE(2, 2) OTP_W1_CASE(3, 2) OTP_W1_CASE(2, 3)
#undef OTP_W1_CASE
    } else if (pf) {
        OTP_ALLOW_BIG_LDS(nhwc_wgrad_kernel<true>, p.lds);
        nhwc_wgrad_kernel<true><<<grid, 256, p.lds, st>>>(static_cast<const bf16*>(x), static_cast<const bf16*>(gy),
                                                           static_cast<float*>(workspace), p);
    } else {
        OTP_ALLOW_BIG_LDS(nhwc_wgrad_kernel<false>, p.lds);
        nhwc_wgrad_kernel<false><<<grid, 256, p.lds, st>>>(static_cast<const bf16*>(x), static_cast<const bf16*>(gy),
                                                            static_cast<float*>(workspace), p);
    }
    if (otp_launch_status() != OTP_OK) return OTP_ERR_LAUNCH;
    const size_t frag_total = (size_t)p.nCo * p.nCi * 4 * WG_NBW * 3 * 256;
    nhwc_wgrad_reduce_kernel<<<(int)((frag_total + 63) / 64), 256, 0, st>>>(static_cast<const float*>(workspace),
                                                                             static_cast<float*>(grad_weight), p, frag_total);
    return otp_launch_status();
}
