// k_grouped_gw<8 | 24> -- grouped 3x3 convolution + BN (+ReLU) over packed pixel rows on the matrix cores for the group widths of
// RegNetY-400MF (8) and RegNetY-1.6GF / 3.2GF (24); gfx950, bf16x3 arithmetic, the contract of k_grouped16_mfma (ldn_grouped.hip):
//     out[r, gw g + n] = act(scale * sum_{t < 9} sum_{i < gw} a[nbr[r, t], gw g + i] * w[gw g + n, t, i] + shift)
// Per group a GEMM with M = gw output channels, N = rows, K = 9 taps x gw channels, cut into CHUNKS of 8 consecutive channels of one
// tap: a lane's eight k-values of a step are 32 bytes of one neighbour row (two 16-byte loads through the neighbour table).
//   width 24: v_mfma_f32_32x32x16_bf16.  M = 32 (24 real: accumulator quad 3 is dropped), N = 32 rows, 27 chunks in 14 steps; lane l of
//             step s holds chunk q = 2 s + (l >> 5) = tap q / 3, channels 8 (q % 3) .. + 7 (q = 27: zero weights, no load).
//   width 8:  v_mfma_f32_16x16x32_bf16.  One group per tile: M = 16 (8 real: lanes 32-63 hold no output), N = 16 rows, 9 chunks in 3
//             steps; lane l of step s holds chunk q = 4 s + (l >> 4) = tap q (q >= 9: zero weights, no load).  No pairing of groups, so
//             an odd group count (13, 55) needs no tail rule and no column at or past C is ever addressed.
// One 1024-thread workgroup = a chunk of groups (their pre-split weight fragments sit in LDS for the workgroup's lifetime: 28 KB per
// width-24 group, 6 KB per width-8 group, <= 140 / 144 KB) x a strided set of row tiles, one tile per wave at a time.  A lane's loads run
// GgCfg::PF steps ahead of the MFMAs that consume them, across the group boundary.
#include "ldn_common.h"

namespace ldn {

template <int GW> struct GgCfg;
template <> struct GgCfg<8> {
    static constexpr int STEPS = 3, TILE = 16, MAXG = 24, PF = 3;
    typedef f32x4 acc_t;
};
template <> struct GgCfg<24> {
    static constexpr int STEPS = 14, TILE = 32, MAXG = 5, PF = 2;
    typedef f32x16 acc_t;
};
constexpr int GG_THREADS = 1024;

struct GgArgs {
    const float* a; int lda;
    const int32_t* nbr; const int32_t* m_count; int m_cap;
    const unsigned char* wf;                // [C / gw][STEPS][64 lanes][8 hi | 8 lo] bf16
    int C;
    const float* scale; const float* shift; int relu;
    float* out; int ldo;
    int gchunk;                             // groups per workgroup
};

__device__ __attribute__((aligned(16))) float g_gg_zero[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};

template <int GW>
__global__ __launch_bounds__(GG_THREADS, 1) void k_grouped_gw(const GgArgs p) {
    typedef GgCfg<GW> cfg;
    constexpr int STEPS = cfg::STEPS, TILE = cfg::TILE, PF = cfg::PF, FRAG = STEPS * 64 * 32;
    static_assert(STEPS % PF == 0, "the prefetch ring must close at the group boundary");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int G = p.C / GW;
    const int g0 = blockIdx.y * p.gchunk;
    const int ng = min(p.gchunk, G - g0);
    const int M = p.m_count ? min(p.m_count[0], p.m_cap) : p.m_cap;
    for (int i = tid; i < ng * (FRAG / 16); i += GG_THREADS)
        reinterpret_cast<f32x4*>(smem)[i] = reinterpret_cast<const f32x4*>(p.wf + (size_t)g0 * FRAG)[i];
    __syncthreads();
    const int n = lane & (TILE - 1), kg = lane / TILE;   // B operand / output column = row n of the tile; k-group kg of a step
    const int ntiles = (M + TILE - 1) / TILE;
    for (int tile = blockIdx.x * (GG_THREADS / 64) + wave; tile < ntiles; tile += gridDim.x * (GG_THREADS / 64)) {
        const int r = tile * TILE + n;
        // this lane's neighbour row and channel offset per K step (-1: a zero row, a row past the count or a padding chunk)
        long aoff[STEPS];
#pragma unroll
        for (int s = 0; s < STEPS; ++s) {
            const int q = (GW == 24 ? 2 : 4) * s + kg;
            const int t = GW == 24 ? q / 3 : q;
            const int ch = GW == 24 ? 8 * (q % 3) : 0;
            const int ar = (t < 9 && r < M) ? p.nbr[(size_t)r * 9 + t] : -1;
            aoff[s] = ar >= 0 ? (long)ar * p.lda + ch : -1;
        }
        f32x4 x0[PF], x1[PF];
        auto request = [&](int gl, int s, int slot) {
            const float* src = aoff[s] >= 0 ? p.a + aoff[s] + (g0 + gl) * GW : g_gg_zero;
            x0[slot] = *reinterpret_cast<const f32x4*>(src);
            x1[slot] = *reinterpret_cast<const f32x4*>(src + 4);
        };
#pragma unroll
        for (int s = 0; s < PF; ++s) request(0, s, s);
#pragma unroll 1
        for (int gl = 0; gl < ng; ++gl) {
            typename cfg::acc_t acc;
#pragma unroll
            for (int e = 0; e < (GW == 24 ? 16 : 4); ++e) acc[e] = 0.f;
            const unsigned char* wfr = smem + (size_t)gl * FRAG + lane * 32;
#pragma unroll
            for (int s = 0; s < STEPS; ++s) {
                bf16x8 bh, bl;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float v = e < 4 ? x0[s % PF][e] : x1[s % PF][e - 4];
                    const __bf16 hb = (__bf16)v;
                    bh[e] = hb;
                    bl[e] = (__bf16)(v - (float)hb);
                }
                // the slot is free: step s + PF of this group, or step s + PF - STEPS of the next one
                if (s + PF < STEPS) request(gl, s + PF, s % PF);
                else if (gl + 1 < ng) request(gl + 1, s + PF - STEPS, s % PF);
                const bf16x8 ah = *reinterpret_cast<const bf16x8*>(wfr + s * 64 * 32);
                const bf16x8 al = *reinterpret_cast<const bf16x8*>(wfr + s * 64 * 32 + 16);
                if constexpr (GW == 24) {
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc, 0, 0, 0);
                } else {
                    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, bh, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bl, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bh, acc, 0, 0, 0);
                }
            }
            // C layout.  32x32: register 4 Q + e of lane (n, kg) is output channel 8 Q + 4 kg + e (Q = 3: channels 24-31, dropped).
            //            16x16: register e of lane (n, kg) is output channel 4 kg + e (kg >= 2: channels 8-15, dropped).
            float* const orow = p.out + (size_t)r * p.ldo;
#pragma unroll
            for (int Q = 0; Q < (GW == 24 ? 3 : 1); ++Q) {
                const int c = (g0 + gl) * GW + 8 * Q + 4 * kg;
                if (r < M && (GW == 24 || kg < 2)) {
                    const f32x4 sc = *reinterpret_cast<const f32x4*>(p.scale + c), sh = *reinterpret_cast<const f32x4*>(p.shift + c);
                    f32x4 v;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        v[e] = acc[4 * Q + e] * sc[e] + sh[e];
                        if (p.relu) v[e] = fmaxf(v[e], 0.f);
                    }
                    *reinterpret_cast<f32x4*>(orow + c) = v;
                }
            }
        }
    }
}

template <int GW>
static int launch_grouped_gw(GgArgs g, hipStream_t stream) {
    typedef GgCfg<GW> cfg;
    constexpr int FRAG = cfg::STEPS * 64 * 32;
    const int G = g.C / GW;
    const int tiles = ceil_div(g.m_cap, cfg::TILE);
    int bx = ceil_div(tiles, GG_THREADS / 64);
    int cus = 256;
    (void)ldn_device_cus(&cus);
    // Groups per workgroup.  A wave walks the groups of its chunk one after the other, each behind the loads of the one before: with few row
    // tiles (the 14 x 14 and 7 x 7 maps) that chain, not the arithmetic, is the launch's time, and the device is filled from the groups
    // instead -- chunks as small as it takes to give every CU a workgroup (two at width 8, whose registers allow it).  With many tiles the
    // chunks are as large as the LDS holds, so that a tile's neighbour rows are looked up once per MAXG groups.
    int nchunks = max(ceil_div(G, cfg::MAXG), min(G, ceil_div(cus * (GW == 8 ? 2 : 1), bx)));
    g.gchunk = ceil_div(G, nchunks);
    nchunks = ceil_div(G, g.gchunk);
    const size_t lds = (size_t)g.gchunk * FRAG;
    LDN_REQUIRE(allow_dynamic_lds(reinterpret_cast<const void*>(&k_grouped_gw<GW>), lds), "k_grouped_gw<%d>: cannot reserve %zu B of LDS", GW, lds);
    const int cap = max(1, (cus * 4) / nchunks);      // a few waves of workgroups: the fragments are staged per workgroup
    if (bx > cap) bx = cap;
    hipLaunchKernelGGL(k_grouped_gw<GW>, dim3((unsigned)bx, (unsigned)nchunks), dim3(GG_THREADS), lds, stream, g);
    LDN_CHECK_LAUNCH("k_grouped_gw");
    return LDN_OK;
}

// ------------------------------------------------------------------------------------------------------------------------
// k_grouped_gw_img<8 | 24> -- the same convolution when the packed rows are WHOLE IMAGES in order (layer skip, the dense index): kept image k
// owns the input rows [k Hi Wi, (k + 1) Hi Wi) and the output rows [k Ho Wo, (k + 1) Ho Wo); the contract and the structure of
// k_grouped16_img (ldn_grouped.hip) with k_grouped_gw's fragments, lane maps and arithmetic -- the result is bit-identical to k_grouped_gw's
// over the same images' neighbour table.  Workgroup = (kept image, band of output rows) x chunk of groups: the chunk's fragments and the
// band's channels of the chunk ([pixel][GW ng + 4] floats, + one zero pixel for the taps outside the image, the padding chunks and the
// pixels past the band) are staged in LDS once; the im2col is a per-lane LDS address from the geometry.  Work items = (pixel tile, group),
// dealt to the 8 waves.  Optional by-product: the channel sums of the final output over the band (the SE squeeze), a fixed tree over every
// 16 pixels of a tile, the 16-pixel partials added in ascending order by one thread per channel.
struct GwiArgs {
    const float* a; int lda;
    const int32_t* m_count;                 // device-side number of OUTPUT rows (kept images x Ho Wo)
    const unsigned char* wf; int C;
    const float* scale; const float* shift; int relu;
    float* out; int ldo;
    int Hi, Wi, Ho, Wo, stride;
    int gchunk, in_ld;                      // groups per workgroup; floats per staged pixel (GW gchunk + 4)
    int R, nbands;                          // output rows per workgroup (Ho: the whole image), bands per image
    int images_cap;
    float* gap;                             // optional [image][band][C]
};
constexpr int GWI_THREADS = 512;

template <int GW>
__global__ __launch_bounds__(GWI_THREADS, 2) void k_grouped_gw_img(const GwiArgs p) {
    typedef GgCfg<GW> cfg;
    constexpr int STEPS = cfg::STEPS, TILE = cfg::TILE, FRAG = STEPS * 64 * 32, NW = GWI_THREADS / 64;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int G = p.C / GW;
    // workgroup order of k_grouped16_img: the group chunks of ONE (image, band) pair take linear ids L, L + 8, L + 16, ... -- one XCD
    const int nch = (G + p.gchunk - 1) / p.gchunk;
    const int per = 8 * nch, jid = (int)(blockIdx.x % (unsigned)per);
    const long pair = (long)(blockIdx.x / (unsigned)per) * 8 + (jid & 7);
    const int k = (int)(pair / p.nbands), band = (int)(pair - (long)k * p.nbands);
    const int g0 = (jid >> 3) * p.gchunk;
    const int ng = min(p.gchunk, G - g0);
    const int HWo = p.Ho * p.Wo;
    if (k >= p.images_cap || (long)k * HWo >= (long)p.m_count[0]) return;   // beyond the launch's pairs / beyond the kept images
    const int y0 = band * p.R, rows_out = min(p.R, p.Ho - y0);
    const int iy0 = max(y0 * p.stride - 1, 0), iy1 = min((y0 + rows_out - 1) * p.stride + 1, p.Hi - 1);
    const int HWi = (iy1 - iy0 + 1) * p.Wi;                                // staged pixels
    const size_t in_row0 = (size_t)k * p.Hi * p.Wi + (size_t)iy0 * p.Wi;   // first staged input row (flat)
    float* const s_in = reinterpret_cast<float*>(smem + (size_t)p.gchunk * FRAG);
    for (int i = tid; i < ng * (FRAG / 16); i += GWI_THREADS)
        reinterpret_cast<f32x4*>(smem)[i] = reinterpret_cast<const f32x4*>(p.wf + (size_t)g0 * FRAG)[i];
    const int qpp = ng * (GW / 4);                                         // 16-byte pieces per pixel
    const int npiece = HWi * qpp;                                          // (< 2^22: the staged floats fit the LDS)
    const float inv_qpp = 1.f / (float)qpp;
    for (int i0 = tid; i0 < npiece; i0 += 8 * GWI_THREADS) {               // eight pieces per thread in flight
        f32x4 v[8];
        int dst[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i = min(i0 + u * GWI_THREADS, npiece - 1);
            int px = (int)(((float)i + 0.5f) * inv_qpp);                   // i / qpp through the reciprocal, corrected
            int q = i - px * qpp;
            if (q < 0) { --px; q += qpp; } else if (q >= qpp) { ++px; q -= qpp; }
            dst[u] = px * p.in_ld + q * 4;
            v[u] = *reinterpret_cast<const f32x4*>(p.a + (in_row0 + px) * p.lda + g0 * GW + q * 4);
        }
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (i0 + u * GWI_THREADS < npiece) *reinterpret_cast<f32x4*>(s_in + dst[u]) = v[u];
    }
    for (int i = tid; i < p.in_ld; i += GWI_THREADS) s_in[(size_t)HWi * p.in_ld + i] = 0.f;   // the zero pixel
    __syncthreads();
    const int n = lane & (TILE - 1), kg = lane / TILE;
    const bool has_out = GW == 24 || kg < 2;                               // (width 8: lanes 32-63 hold output channels 8-15, which do not exist)
    const int npix = rows_out * p.Wo;                                      // output pixels of the band
    const int ntile = (npix + TILE - 1) / TILE;
    const int nsub = ntile * (TILE / 16);                                  // (gap) 16-pixel partial sums per group
    float* const s_gap = s_in + ((size_t)HWi + 1) * p.in_ld;               // (gap) [group][16-pixel piece][GW channels]
    for (int w = wave; w < ntile * ng; w += NW) {
        const int gl = w / ntile, tile = w - gl * ntile;
        const int q = tile * TILE + n;
        const bool valid = q < npix;
        const int ly = (valid ? q : 0) / p.Wo, ox = (valid ? q : 0) - ly * p.Wo;
        const int oy = y0 + ly;
        typename cfg::acc_t acc;
#pragma unroll
        for (int e = 0; e < (GW == 24 ? 16 : 4); ++e) acc[e] = 0.f;
        const unsigned char* wfr = smem + (size_t)gl * FRAG + lane * 32;
#pragma unroll
        for (int s = 0; s < STEPS; ++s) {
            const int qc = (GW == 24 ? 2 : 4) * s + kg;
            const int t = GW == 24 ? qc / 3 : qc;
            const int ch = GW == 24 ? 8 * (qc - 3 * t) : 0;
            const int ty = t / 3;
            const int iy = oy * p.stride - 1 + ty, ix = ox * p.stride - 1 + (t - 3 * ty);
            const bool inb = valid && t < 9 && iy >= 0 && iy < p.Hi && ix >= 0 && ix < p.Wi;
            const float* src = s_in + (size_t)(inb ? (iy - iy0) * p.Wi + ix : HWi) * p.in_ld + (inb ? gl * GW + ch : 0);
            const f32x4 x0 = *reinterpret_cast<const f32x4*>(src), x1 = *reinterpret_cast<const f32x4*>(src + 4);
            bf16x8 bh, bl;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float v = e < 4 ? x0[e] : x1[e - 4];
                const __bf16 hb = (__bf16)v;
                bh[e] = hb;
                bl[e] = (__bf16)(v - (float)hb);
            }
            const bf16x8 ah = *reinterpret_cast<const bf16x8*>(wfr + s * 64 * 32);
            const bf16x8 al = *reinterpret_cast<const bf16x8*>(wfr + s * 64 * 32 + 16);
            if constexpr (GW == 24) {
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc, 0, 0, 0);
            } else {
                acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, bh, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bl, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bh, acc, 0, 0, 0);
            }
        }
        // C layout of k_grouped_gw.  Lanes without output (width 8, kg >= 2) run the epilogue on the channels of kg & 1 -- every lane takes part
        // in the DPP sums below -- and neither store nor add anything.
        float* const orow = p.out + ((size_t)k * HWo + (size_t)y0 * p.Wo + q) * p.ldo;
#pragma unroll
        for (int Q = 0; Q < (GW == 24 ? 3 : 1); ++Q) {
            const int c = (g0 + gl) * GW + 8 * Q + 4 * (GW == 24 ? kg : (kg & 1));
            const f32x4 sc = *reinterpret_cast<const f32x4*>(p.scale + c), sh = *reinterpret_cast<const f32x4*>(p.shift + c);
            f32x4 v;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                v[e] = __builtin_fmaf(acc[4 * Q + e], sc[e], sh[e]);      // k_grouped_gw's epilogue compiles to fused multiply-adds: the same bits
                if (p.relu) v[e] = fmaxf(v[e], 0.f);
            }
            if (valid && has_out) *reinterpret_cast<f32x4*>(orow + c) = v;
            if (p.gap) {      // (uniform) channel sums over the 16 pixels of this lane's DPP row
                f32x4 t4;
#pragma unroll
                for (int e = 0; e < 4; ++e) t4[e] = row16_sum(valid && has_out ? v[e] : 0.f);
                const int sub = GW == 24 ? 2 * tile + ((lane >> 4) & 1) : tile;
                if ((lane & 15) == 0 && has_out)
                    *reinterpret_cast<f32x4*>(s_gap + ((size_t)gl * nsub + sub) * GW + 8 * Q + 4 * kg) = t4;
            }
        }
    }
    if (p.gap) {
        __syncthreads();
        for (int i = tid; i < ng * GW; i += GWI_THREADS) {
            const int gl = i / GW, ch = i - gl * GW;
            float s = 0.f;
            for (int t = 0; t < nsub; ++t) s += s_gap[((size_t)gl * nsub + t) * GW + ch];
            p.gap[((size_t)k * p.nbands + band) * p.C + (g0 + gl) * GW + ch] = s;
        }
    }
}

// LDS bytes of one k_grouped_gw_img workgroup: ng groups' fragments, in_rows input rows (+ the zero pixel) and, with gap, the 16-pixel partial sums
static size_t gwi_bytes(int gw, int ng, int in_rows, int out_rows, int Wi, int Wo, bool gap) {
    const size_t frag = (size_t)(gw == 24 ? GgCfg<24>::STEPS : GgCfg<8>::STEPS) * 64 * 32;
    const int tile = gw == 24 ? GgCfg<24>::TILE : GgCfg<8>::TILE;
    const size_t ntile = ((size_t)out_rows * Wo + tile - 1) / tile;
    return (size_t)ng * frag + ((size_t)in_rows * Wi + 1) * (size_t)(gw * ng + 4) * 4 + (gap ? (size_t)ng * ntile * (tile / 16) * gw * 4 : 0);
}

// The plan (pure host arithmetic; gi_plan's for these widths): groups per workgroup and output rows per workgroup for an Hi x Wi input map; false:
// not even three input rows of one group fit.  Whole images where one group's share of the image fits a workgroup alone on its CU (150 KB), with as
// many groups per workgroup as leave room for two workgroups per CU (80 KB); bands of output rows of one group otherwise -- as many rows as
// two workgroups per CU allow, or, where that band has less than one pixel tile per wave, as one workgroup per CU allows.  gap: the partial
// sums count against the same budgets.
static bool gwi_plan(int gw, int Hi, int Wi, int Ho, int stride, int G, int* ng_out, int* R_out, bool gap) {
    constexpr size_t ONE = 150 * 1024, TWO = 80 * 1024;
    if (Hi <= 0 || Wi <= 0 || Ho <= 0 || G <= 0 || Wi > (1 << 16)) return false;      // (three rows of a 2^16-wide map are far past the LDS)
    const int Wo = (Wi - 1) / stride + 1;
    const int maxg = gw == 24 ? GgCfg<24>::MAXG : GgCfg<8>::MAXG, tile = gw == 24 ? GgCfg<24>::TILE : GgCfg<8>::TILE;
    if ((size_t)Hi * Wi < (1u << 20) && gwi_bytes(gw, 1, Hi, Ho, Wi, Wo, gap) <= ONE) {
        int ng = 1;
        while (ng < G && ng < maxg && gwi_bytes(gw, ng + 1, Hi, Ho, Wi, Wo, gap) <= TWO) ++ng;
        *ng_out = ceil_div(G, ceil_div(G, ng));
        *R_out = Ho;
        return true;
    }
    auto rows = [&](size_t budget) {
        int R = 0;                             // (R + 1 - 1) stride + 3 input rows for R + 1 output rows
        while (R < Ho && gwi_bytes(gw, 1, R * stride + 3, R + 1, Wi, Wo, gap) <= budget) ++R;
        return R;
    };
    int R = rows(TWO);
    if (R < Ho && (long)R * Wo < (long)(GWI_THREADS / 64) * tile) R = rows(ONE);
    if (R < 1) return false;
    *ng_out = 1;
    *R_out = ceil_div(Ho, ceil_div(Ho, R));
    return true;
}

static bool gwi_geometry(int Hi, int Wi, int Ho, int Wo, int stride) {
    return (stride == 1 || stride == 2) && Hi > 0 && Wi > 0 && Ho == (Hi - 1) / stride + 1 && Wo == (Wi - 1) / stride + 1;
}

template <int GW>
static int launch_grouped_gw_img(GwiArgs g, hipStream_t stream) {
    constexpr int FRAG = GgCfg<GW>::STEPS * 64 * 32;
    const int G = g.C / GW;
    g.nbands = ceil_div(g.Ho, g.R);
    g.in_ld = GW * g.gchunk + 4;
    const int in_rows = g.R == g.Ho ? g.Hi : min(g.Hi, (g.R - 1) * g.stride + 3);
    const size_t lds = gwi_bytes(GW, g.gchunk, in_rows, g.R, g.Wi, g.Wo, g.gap != nullptr);
    static_assert(FRAG % 16 == 0, "the staged rows behind the fragments stay 16-byte aligned");
    LDN_REQUIRE(allow_dynamic_lds(reinterpret_cast<const void*>(&k_grouped_gw_img<GW>), lds), "k_grouped_gw_img<%d>: cannot reserve %zu B of LDS", GW, lds);
    const long pairs = (long)g.images_cap * g.nbands;
    const long nwg = (pairs + 7) / 8 * 8 * ceil_div(G, g.gchunk);
    LDN_REQUIRE(nwg < (1l << 31), "ldn_grouped_mfma_conv3x3_images: too many workgroups (%ld)", nwg);
    hipLaunchKernelGGL(k_grouped_gw_img<GW>, dim3((unsigned)nwg), dim3(GWI_THREADS), lds, stream, g);
    LDN_CHECK_LAUNCH("k_grouped_gw_img");
    return LDN_OK;
}

}  // namespace ldn

using namespace ldn;

extern "C" int ldn_grouped_mfma_ok(int C, int group_width) {
    return (group_width == 8 || group_width == 24) && C > 0 && C % group_width == 0 ? 1 : 0;
}

extern "C" size_t ldn_grouped_mfma_weight_bytes(int C, int group_width) {
    if (!ldn_grouped_mfma_ok(C, group_width)) return 0;
    return (size_t)(C / group_width) * (group_width == 24 ? GgCfg<24>::STEPS : GgCfg<8>::STEPS) * 64 * 32;
}

extern "C" int ldn_grouped_mfma_conv3x3_rows(const float* a, int lda, const int32_t* nbr, const int32_t* m_count, int m_cap,
                                             const void* w_frag, int C, int group_width, const float* scale, const float* shift,
                                             int relu, float* out, int ldo, void* stream) {
    LDN_REQUIRE(a && nbr && w_frag && scale && shift && out, "ldn_grouped_mfma_conv3x3_rows: null pointer");
    LDN_REQUIRE(ldn_grouped_mfma_ok(C, group_width),
                "ldn_grouped_mfma_conv3x3_rows: group width %d with %d channels is not built (widths 8 and 24, channels a multiple of the width)",
                group_width, C);
    LDN_REQUIRE(lda % 4 == 0 && ldo % 4 == 0 && lda >= C && ldo >= C, "ldn_grouped_mfma_conv3x3_rows: strides must be multiples of 4");
    LDN_REQUIRE((uintptr_t)a % 16 == 0 && (uintptr_t)out % 16 == 0 && (uintptr_t)w_frag % 16 == 0 && (uintptr_t)scale % 16 == 0 &&
                (uintptr_t)shift % 16 == 0, "ldn_grouped_mfma_conv3x3_rows: pointers must be 16-byte aligned");
    if (m_cap <= 0) return LDN_OK;
    GgArgs g{};
    g.a = a; g.lda = lda; g.nbr = nbr; g.m_count = m_count; g.m_cap = m_cap; g.wf = static_cast<const unsigned char*>(w_frag); g.C = C;
    g.scale = scale; g.shift = shift; g.relu = relu; g.out = out; g.ldo = ldo;
    return group_width == 24 ? launch_grouped_gw<24>(g, static_cast<hipStream_t>(stream)) : launch_grouped_gw<8>(g, static_cast<hipStream_t>(stream));
}

extern "C" int ldn_grouped_mfma_images_fit(int Hi, int Wi, int C, int group_width) {
    int ng = 0, R = 0;   // both strides and the channel-sum scratch of the gap form: the module gates its paths on this answer
    if (!ldn_grouped_mfma_ok(C, group_width) || Hi <= 0 || Wi <= 0) return 0;
    const int G = C / group_width;
    return (gwi_plan(group_width, Hi, Wi, (Hi - 1) / 2 + 1, 2, G, &ng, &R, true) && gwi_plan(group_width, Hi, Wi, Hi, 1, G, &ng, &R, true)) ? ng : 0;
}

extern "C" int ldn_grouped_mfma_images_bands(int Hi, int Wi, int Ho, int stride, int C, int group_width) {
    int ng = 0, R = 0;   // (the gap form's bands: it sizes that form's buffer, and the plain form runs the same plan)
    if (!ldn_grouped_mfma_ok(C, group_width) || !gwi_geometry(Hi, Wi, Ho, Wi > 0 && stride > 0 ? (Wi - 1) / stride + 1 : 0, stride)) return 0;
    if (!gwi_plan(group_width, Hi, Wi, Ho, stride, C / group_width, &ng, &R, true)) return 0;
    return ceil_div(Ho, R);
}

static int grouped_mfma_images(const float* a, int lda, const int32_t* m_count, int images_cap, int Hi, int Wi, int Ho, int Wo, int stride,
                               const void* w_frag, int C, int group_width, const float* scale, const float* shift, int relu, float* out,
                               int ldo, float* gap, void* stream) {
    LDN_REQUIRE(a && m_count && w_frag && scale && shift && out, "ldn_grouped_mfma_conv3x3_images: null pointer");
    LDN_REQUIRE(ldn_grouped_mfma_ok(C, group_width),
                "ldn_grouped_mfma_conv3x3_images: group width %d with %d channels is not built (widths 8 and 24, channels a multiple of the width)",
                group_width, C);
    LDN_REQUIRE(lda % 4 == 0 && ldo % 4 == 0 && lda >= C && ldo >= C, "ldn_grouped_mfma_conv3x3_images: strides must be multiples of 4");
    LDN_REQUIRE((uintptr_t)a % 16 == 0 && (uintptr_t)out % 16 == 0 && (uintptr_t)w_frag % 16 == 0 && (uintptr_t)scale % 16 == 0 &&
                (uintptr_t)shift % 16 == 0 && (uintptr_t)gap % 16 == 0, "ldn_grouped_mfma_conv3x3_images: pointers must be 16-byte aligned");
    LDN_REQUIRE(gwi_geometry(Hi, Wi, Ho, Wo, stride), "ldn_grouped_mfma_conv3x3_images: %dx%d -> %dx%d is not a 3x3 / pad 1 / stride %d (1 or 2) geometry",
                Hi, Wi, Ho, Wo, stride);
    GwiArgs g{};
    // one plan for the plain and the gap form (the scratch of the sums is counted in both): ldn_grouped_mfma_images_bands answers for either
    LDN_REQUIRE(gwi_plan(group_width, Hi, Wi, Ho, stride, C / group_width, &g.gchunk, &g.R, true),
                "ldn_grouped_mfma_conv3x3_images: three rows of a %d-wide map do not fit the LDS (ldn_grouped_mfma_images_fit)", Wi);
    if (images_cap <= 0) return LDN_OK;
    g.a = a; g.lda = lda; g.m_count = m_count; g.wf = static_cast<const unsigned char*>(w_frag); g.C = C;
    g.scale = scale; g.shift = shift; g.relu = relu; g.out = out; g.ldo = ldo;
    g.Hi = Hi; g.Wi = Wi; g.Ho = Ho; g.Wo = Wo; g.stride = stride; g.gap = gap; g.images_cap = images_cap;
    return group_width == 24 ? launch_grouped_gw_img<24>(g, static_cast<hipStream_t>(stream)) : launch_grouped_gw_img<8>(g, static_cast<hipStream_t>(stream));
}

extern "C" int ldn_grouped_mfma_conv3x3_images(const float* a, int lda, const int32_t* m_count, int images_cap, int Hi, int Wi, int Ho, int Wo,
                                               int stride, const void* w_frag, int C, int group_width, const float* scale, const float* shift,
                                               int relu, float* out, int ldo, void* stream) {
    return grouped_mfma_images(a, lda, m_count, images_cap, Hi, Wi, Ho, Wo, stride, w_frag, C, group_width, scale, shift, relu, out, ldo, nullptr, stream);
}

extern "C" int ldn_grouped_mfma_conv3x3_images_gap(const float* a, int lda, const int32_t* m_count, int images_cap, int Hi, int Wi, int Ho, int Wo,
                                                   int stride, const void* w_frag, int C, int group_width, const float* scale, const float* shift,
                                                   int relu, float* out, int ldo, float* gap_partial, void* stream) {
    LDN_REQUIRE(gap_partial, "ldn_grouped_mfma_conv3x3_images_gap: null pointer");
    return grouped_mfma_images(a, lda, m_count, images_cap, Hi, Wi, Ho, Wo, stride, w_frag, C, group_width, scale, shift, relu, out, ldo, gap_partial, stream);
}
