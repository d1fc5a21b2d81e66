// k_grouped_wide<56 | 112 | 232> -- LAD-RegNet conv b in CHANNEL mode (and the 'both' branch) on the matrix cores at the group widths of RegNetY-8GF,
// RegNetY-16GF and RegNetY-32GF: the contract of k_grouped_chan (ldn_grouped_chan.hip) and its DENSE-SLOT form -- the packed columns of an image are EXPANDED
// into their group slots with zeros in the inactive slots, the dense gw x gw x 9 product of the group runs in bf16x3, the active output slots
// are COMPRESSED back to their packed columns in the epilogue; exact because the mask multiplies after conv + BN + ReLU.
// What is different: a group's pre-split fragments are 128 KB (width 56) / 504 KB (width 112) / 2096 KB (width 232) and do not fit a CU's LDS, so
//   * the WEIGHTS STREAM THROUGH REGISTERS.  v_mfma_f32_32x32x16_bf16; the out channels are padded to MT = 2 / 4 / 8 row tiles of 32.  Wave w of
//     the 8 owns row tile w % MT and pixel-tile set w / MT: per K step it loads ITS 32 B per lane of ITS row tile straight from global memory
//     (one coalesced 2 KB line per wave; the fragment order makes a lane's [8 hi | 8 lo] contiguous), one step ahead, and uses them for the
//     up to PT = 4 pixel tiles whose accumulators it keeps resident across the whole K loop (width 232: MT = 8, every wave its own row tile,
//     one tile set).  No LDS ring, no barrier inside the K loop; the
//     LDS holds the input only, and the waves that share a row tile read the same lines within a few hundred cycles of each other (L1 / L2);
//   * one workgroup = (group, RUN OF IMAGES, rectangle of output pixels): on small maps up to 8 whole images share a workgroup, so one pass
//     over a group's fragments serves 4 (width 232) / 8 (width 112) / 16 (width 56) pixel tiles.  A pixel tile never mixes images.  An (image, group) pair
//     without an active channel is not staged and gets no tile;
//   * the input is staged PRE-SPLIT ([8 hi | 8 lo] bf16 per octet, the 4 B per element of fp32) WITH ITS ZERO HALO: a rectangle of R x Wc
//     output pixels stages ((R - 1) stride + 3) x ((Wc - 1) stride + 3) pixels, those outside the image as zeros, so the im2col address of a
//     lane is base(pixel) + offset(tap, octet) with no bounds test in the K loop, and the split is done once per staged element, not per tap.
//     Maps that do not fit are cut into bands of output rows and, where a band of full rows does not fit either (width 112 keeps 480 B per
//     staged pixel: three rows of a 112-wide map are 161 KB), into column strips as well.
// K = 9 gw in octets q = tap * (gw / 8) + octet of 8 consecutive channels; K step s covers octets 2 s and 2 s + 1 (lane half h = lane >> 5).
// Width 56: 63 octets in 32 steps (octet 63 is a zero pad of the fragments); width 112: 126 octets in 63 steps; width 232: 261 octets in 131
// steps (octet 261 is the zero pad).
// Input columns >= ch_cnt[b] and the pad columns of lda are never read; output columns >= C are never written.  No atomics: deterministic.
// k_grouped_wide<GW, true> (ldn_grouped_wide_conv3x3_image_gap) is the same kernel that also leaves the channel sums of its output: see GAP below.
#include <algorithm>

#include "ldn_common.h"
#include "ldn_grouped_wide_frag.h"

namespace ldn {

// bytes of a staged pixel.  Width 56: 224, 8 consecutive pixels cover the 64 banks; width 112: 448 + 32, the same bank walk (448 B would repeat after 4);
// width 232: 928 = 32 x 29 with no pad -- an odd count of 32-byte pieces, so 8 consecutive pixels again start in the 8 different 32-byte
// pieces of the 256 bytes the banks span (chosen on paper by that rule; not measured with counters)
constexpr int gwd_pixb(int gw) { return gw == 56 ? 224 : gw == 112 ? 480 : 928; }
constexpr int GWD_THREADS = 512;
constexpr int GWD_PT = 4;                    // pixel tiles (of 32) a wave keeps accumulators for
constexpr int GWD_MAXIMG = 8;                // images per workgroup
constexpr int GWD_MAXCUT = 32;               // bands / strips per dimension the plan tries
constexpr size_t GWD_LDS_TWO = 80 * 1024;    // two workgroups per CU
constexpr size_t GWD_LDS_ONE = 150 * 1024;   // one

struct GwArgs {
    const float* a; int lda;
    int B, Hi, Wi, Ho, Wo, stride;
    const unsigned char* wf; int C;         // [C / gw][NSTEP][MT][64 lanes][8 hi | 8 lo] bf16
    const int32_t* ch_idx; const int32_t* ch_cnt;
    const float* scale; const float* shift; int relu;
    float* out; int ldo;
    int nimg;                               // images per workgroup (> 1 only when the rectangle is the whole image)
    int R, Wc, nrb, ncb;                    // output rows / columns per rectangle, row bands / column strips per image
    int tab_bytes;                          // the tables in front of the staged input
    float* gap; int gap_off;                // (GAP) [image][rectangle][C] channel sums of the rectangle's output, packed-column order; the tile sums' scratch in LDS
};

__host__ __device__ inline int gwd_tab_bytes(int gw, int nimg) { return round_up((nimg * gw + 2 * GWD_MAXIMG + 4) * 4, 32); }   // map, active list, counts, n

// The K loop of one wave over NPT resident pixel tiles: this lane's fragments of step s + 1 are in flight under the MFMAs of step s.
template <int GW, int NPT>
__device__ __forceinline__ void gw_kloop(const unsigned char* wbase, const unsigned char* s_in, const int (&pbase)[GWD_PT], int sw, int h,
                                         f32x16 (&acc)[GWD_PT]) {
    constexpr int MT = GwCfg<GW>::MT, NSTEP = GwCfg<GW>::NSTEP, PIXB = gwd_pixb(GW), OCT = GW / 8;
    bf16x8 ah = *reinterpret_cast<const bf16x8*>(wbase), al = *reinterpret_cast<const bf16x8*>(wbase + 16);
#pragma unroll 1
    for (int s = 0; s < NSTEP; ++s) {
        const int sn = min(s + 1, NSTEP - 1);
        const bf16x8 nh = *reinterpret_cast<const bf16x8*>(wbase + (size_t)sn * (MT * 2048));
        const bf16x8 nl = *reinterpret_cast<const bf16x8*>(wbase + (size_t)sn * (MT * 2048) + 16);
        const int q8 = 2 * s + h;
        int t = q8 / OCT;
        const int oct = q8 - t * OCT;
        if (gw_frag_pad_octet<GW>()) t = min(t, 8);                                // octet 63 / 261: zero weights; any staged (finite) input serves
        const int dy = t / 3, dx = t - 3 * dy;
        const int koff = (dy * sw + dx) * PIXB + oct * 32;
        bf16x8 bh[NPT], bl[NPT];
#pragma unroll
        for (int pt = 0; pt < NPT; ++pt) {
            const unsigned char* src = s_in + pbase[pt] + koff;
            bh[pt] = *reinterpret_cast<const bf16x8*>(src);
            bl[pt] = *reinterpret_cast<const bf16x8*>(src + 16);
        }
#pragma unroll
        for (int pt = 0; pt < NPT; ++pt) {
            acc[pt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh[pt], acc[pt], 0, 0, 0);
            acc[pt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl[pt], acc[pt], 0, 0, 0);
            acc[pt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh[pt], acc[pt], 0, 0, 0);
        }
        ah = nh;
        al = nl;
    }
}

// sum over the 32 lanes of a half-wave, in each of them: the DPP tree of the 16-lane row, then row 0 + row 1 (row 2 + row 3) through the
// gfx950 row exchange (a + b in both rows); fixed order.  EVERY lane of the wave must be active.
__device__ __forceinline__ float half32_sum(float v) {
    const float t = row16_sum(v);
    const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(t), __float_as_uint(t), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

// GAP: the epilogue also leaves the sums of the rectangle's output pixels per packed column (the SE squeeze of the block, ldn_se_gate_image),
// as k_grouped_chan's gap form does: a tree over the 32 pixels of a tile (half32_sum), one row of LDS per pixel tile [tile][MT x 32 slots],
// then, behind the last pass, one thread per (active image, active slot) adds its image's tiles in ascending order -- no atomics, the same
// bits in every launch.  The scratch lies behind the staged input (gwd_gap_bytes: the plain form's plan does not count it;
// ldn_grouped_wide_gap_ok answers whether it still fits).  The zeros of the columns behind the count are written with the output's zeros
// (step 2), so every element of gap has exactly one writer.
template <int GW, bool GAP = false>
__global__ __launch_bounds__(GWD_THREADS, 4) void k_grouped_wide(const GwArgs p) {
    typedef GwCfg<GW> cfg;
    constexpr int MT = cfg::MT, NSTEP = cfg::NSTEP, PIXB = gwd_pixb(GW), OCT = GW / 8, NSET = 8 / MT, PT = GWD_PT, CAP = NSET * PT;
    extern __shared__ __attribute__((aligned(32))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int G = p.C / GW;
    // workgroup order: the group is the slowest index, so the workgroups in flight at one time stream the fragments of one or two groups
    const int nrect = p.nrb * p.ncb, nruns = (p.B + p.nimg - 1) / p.nimg;
    const unsigned per = (unsigned)nruns * (unsigned)nrect;
    const int g = (int)(blockIdx.x / per);
    const int rem = (int)(blockIdx.x - (unsigned)g * per);
    const int run = rem / nrect, rect = rem - run * nrect;
    const int rb = rect / p.ncb, cb = rect - rb * p.ncb;
    const int b0 = run * p.nimg, ni = min(p.nimg, p.B - b0);
    const int y0 = rb * p.R, rows = min(p.R, p.Ho - y0), x0 = cb * p.Wc, cols = min(p.Wc, p.Wo - x0);
    const int npix = rows * cols;
    int* const s_map = reinterpret_cast<int*>(smem);            // [nimg][GW] packed column of the slot, -1: inactive
    int* const s_act = s_map + p.nimg * GW;                     // [MAXIMG] the run's images with an active channel in this group, in order
    int* const s_cb = s_act + GWD_MAXIMG;                       // [MAXIMG] clamped counts
    int* const s_nact = s_cb + GWD_MAXIMG;
    unsigned char* const s_in = smem + p.tab_bytes;             // [active image][staged pixel][PIXB]: octet o at 32 o = [8 hi | 8 lo]
    // ---- 1. slot maps and active images
    for (int i = tid; i < ni * GW; i += GWD_THREADS) s_map[i] = -1;
    if (tid < ni) {
        const int cnt = p.ch_cnt[b0 + tid];
        LDN_DCHECK(cnt >= 0 && cnt <= p.C, 423);
        s_cb[tid] = min(max(cnt, 0), p.C);
    }
    __syncthreads();
    const int c_lo = g * GW, c_hi = c_lo + GW;
    for (int il = 0; il < ni; ++il) {
        const int32_t* const chb = p.ch_idx + (size_t)(b0 + il) * p.C;
        const int Cb = s_cb[il];
        for (int j = tid; j < Cb; j += GWD_THREADS) {
            const int c = chb[j];
            LDN_DCHECK(c >= 0 && c < p.C, 421);                                     // channel list entries
            LDN_DCHECK(j == 0 || c > chb[j - 1], 422);                              // ascending
            if (c >= c_lo && c < c_hi) s_map[il * GW + c - c_lo] = j;               // entries outside the workgroup's group are dropped
        }
    }
    __syncthreads();
    if (wave == 0) {
        bool act = false;
        if (lane < ni)
            for (int s = 0; s < GW; ++s) act |= s_map[lane * GW + s] >= 0;
        const unsigned long long m = __ballot(act);
        if (act) s_act[__popcll(m & ((1ull << lane) - 1ull))] = lane;
        if (lane == 0) *s_nact = __popcll(m);
    }
    __syncthreads();
    const int nact = *s_nact;
    // ---- 2. zeros behind the counts: the groups share the columns [Cb, C) of every pixel of the rectangle
    for (int il = 0; il < ni; ++il) {
        const int Cb = s_cb[il], zc = p.C - Cb;
        const int z0 = Cb + (int)((long)zc * g / G), nz = Cb + (int)((long)zc * (g + 1) / G) - z0;
        float* const ob = p.out + ((size_t)(b0 + il) * p.Ho * p.Wo) * p.ldo;
        for (int i = tid; i < npix * nz; i += GWD_THREADS) {
            const int px = i / nz, ly = px / cols, lx = px - ly * cols;
            ob[((size_t)(y0 + ly) * p.Wo + x0 + lx) * p.ldo + z0 + (i - px * nz)] = 0.f;
        }
        if constexpr (GAP)
            for (int i = tid; i < nz; i += GWD_THREADS) p.gap[((size_t)(b0 + il) * nrect + rect) * p.C + z0 + i] = 0.f;
    }
    if (nact == 0) return;                                      // (uniform) no active channel of this group in the run: nothing staged, no MFMA
    // ---- 3. the rectangle's input pixels with their halo, expanded into the group's slots and pre-split
    const int sh = (rows - 1) * p.stride + 3, sw = (cols - 1) * p.stride + 3, sp = sh * sw;
    const int iy0 = y0 * p.stride - 1, ix0 = x0 * p.stride - 1;
    {
        const int ppi = sp * OCT, npiece = nact * ppi;         // 32-byte pieces
        for (int i0 = tid; i0 < npiece; i0 += 2 * GWD_THREADS) {
            f32x4 v[2][2];
            int dst[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int i = min(i0 + u * GWD_THREADS, npiece - 1);
                const int ia = i / ppi, r = i - ia * ppi;
                const int px = r / OCT, o = r - px * OCT;
                const int sy = px / sw, sx = px - sy * sw;
                const int iy = iy0 + sy, ix = ix0 + sx;
                const bool in = iy >= 0 && iy < p.Hi && ix >= 0 && ix < p.Wi;
                const int il = s_act[ia];
                const i32x4 m0 = *reinterpret_cast<const i32x4*>(s_map + il * GW + 8 * o);
                const i32x4 m1 = *reinterpret_cast<const i32x4*>(s_map + il * GW + 8 * o + 4);
                const float* src = p.a + (((size_t)(b0 + il) * p.Hi + (in ? iy : 0)) * p.Wi + (in ? ix : 0)) * p.lda;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    v[u][0][e] = in && m0[e] >= 0 ? src[m0[e]] : 0.f;
                    v[u][1][e] = in && m1[e] >= 0 ? src[m1[e]] : 0.f;
                }
                dst[u] = (ia * sp + px) * PIXB + o * 32;
            }
#pragma unroll
            for (int u = 0; u < 2; ++u)
                if (i0 + u * GWD_THREADS < npiece) {
                    bf16x8 hi, lo;
                    split8<f32x4>(v[u][0], v[u][1], hi, lo);
                    *reinterpret_cast<bf16x8*>(s_in + dst[u]) = hi;
                    *reinterpret_cast<bf16x8*>(s_in + dst[u] + 16) = lo;
                }
        }
    }
    __syncthreads();
    // ---- 4. passes of up to CAP pixel tiles: wave = (row tile mt, tile set); tile T of a pass belongs to set T % NSET, slot T / NSET
    const int mt = wave % MT, set = wave / MT;
    const int n = lane & 31, h = lane >> 5;
    const int tpr = (npix + 31) / 32, ntile = nact * tpr;
    const unsigned char* const wbase = p.wf + (size_t)g * (NSTEP * MT * 2048) + mt * 2048 + lane * 32;
    float* const s_gap = reinterpret_cast<float*>(smem + p.gap_off);               // (GAP) [pixel tile of the workgroup][MT x 32 slots]
    for (int t0 = 0; t0 < ntile; t0 += CAP) {
        const int left = ntile - t0 - set;
        const int npt = left <= 0 ? 0 : min(PT, (left + NSET - 1) / NSET);      // (wave-uniform) this wave's tiles of the pass
        if (npt == 0) continue;
        int pbase[PT];
        f32x16 acc[PT];
#pragma unroll
        for (int pt = 0; pt < PT; ++pt) {
            const int T = min(t0 + pt * NSET + set, ntile - 1);
            const int ia = T / tpr, q = (T - ia * tpr) * 32 + n;
            const int qq = q < npix ? q : 0;                                       // lanes past the rectangle compute pixel 0 and store nothing
            const int ly = qq / cols, lx = qq - ly * cols;
            pbase[pt] = (ia * sp + ly * p.stride * sw + lx * p.stride) * PIXB;
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[pt][e] = 0.f;
        }
        switch (npt) {                                                              // the tile count as a constant: straight-line K steps
            case 1: gw_kloop<GW, 1>(wbase, s_in, pbase, sw, h, acc); break;
            case 2: gw_kloop<GW, 2>(wbase, s_in, pbase, sw, h, acc); break;
            case 3: gw_kloop<GW, 3>(wbase, s_in, pbase, sw, h, acc); break;
            default: gw_kloop<GW, 4>(wbase, s_in, pbase, sw, h, acc); break;
        }
        // ---- 5. C layout of 32x32: register 4 Q + e of lane (n, h) is output slot 32 mt + 8 Q + 4 h + e of pixel n; slots >= GW are pads
#pragma unroll
        for (int pt = 0; pt < PT; ++pt)
            if (pt < npt) {
                const int T = t0 + pt * NSET + set;
                const int ia = T / tpr, q = (T - ia * tpr) * 32 + n;
                if constexpr (GAP) {
                    // every lane takes part in the sums; lanes past the rectangle computed pixel 0, add zeros and store nothing.  The values
                    // are those of the plain branch below (the same expression on the same operands), inactive slots included: their sums
                    // go to LDS and are dropped by the final pass.  Pad slots (32 mt + 8 Q >= GW: wave-uniform) are skipped.
                    const bool live = q < npix;
                    const int qq = live ? q : 0;
                    const int il = s_act[ia];
                    const int ly = qq / cols, lx = qq - ly * cols;
                    float* const orow = p.out + (((size_t)(b0 + il) * p.Ho + y0 + ly) * p.Wo + x0 + lx) * p.ldo;
#pragma unroll
                    for (int Q = 0; Q < 4; ++Q) {
                        if (32 * mt + 8 * Q < GW) {
                            const int sb = 32 * mt + 8 * Q + 4 * h;
                            const int c = g * GW + sb;
                            const f32x4 sc = *reinterpret_cast<const f32x4*>(p.scale + c), sf = *reinterpret_cast<const f32x4*>(p.shift + c);
                            f32x4 v, t4;
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                v[e] = acc[pt][4 * Q + e] * sc[e] + sf[e];
                                if (p.relu) v[e] = fmaxf(v[e], 0.f);
                                t4[e] = half32_sum(live ? v[e] : 0.f);
                            }
                            if (live) {
                                const i32x4 m = *reinterpret_cast<const i32x4*>(s_map + il * GW + sb);
                                if (m[0] >= 0 && (m[0] & 3) == 0 && m[1] == m[0] + 1 && m[2] == m[0] + 2 && m[3] == m[0] + 3) {
                                    *reinterpret_cast<f32x4*>(orow + m[0]) = v;
                                } else {
#pragma unroll
                                    for (int e = 0; e < 4; ++e)
                                        if (m[e] >= 0) orow[m[e]] = v[e];
                                }
                            }
                            if (n == 0) *reinterpret_cast<f32x4*>(s_gap + (size_t)T * (MT * 32) + sb) = t4;
                        }
                    }
                } else if (q < npix) {
                    const int il = s_act[ia];
                    const int ly = q / cols, lx = q - ly * cols;
                    float* const orow = p.out + (((size_t)(b0 + il) * p.Ho + y0 + ly) * p.Wo + x0 + lx) * p.ldo;
#pragma unroll
                    for (int Q = 0; Q < 4; ++Q) {
                        const int sb = 32 * mt + 8 * Q + 4 * h;
                        if (sb < GW) {
                            const int c = g * GW + sb;
                            const f32x4 sc = *reinterpret_cast<const f32x4*>(p.scale + c), sf = *reinterpret_cast<const f32x4*>(p.shift + c);
                            const i32x4 m = *reinterpret_cast<const i32x4*>(s_map + il * GW + sb);
                            f32x4 v;
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                v[e] = acc[pt][4 * Q + e] * sc[e] + sf[e];
                                if (p.relu) v[e] = fmaxf(v[e], 0.f);
                            }
                            if (m[0] >= 0 && (m[0] & 3) == 0 && m[1] == m[0] + 1 && m[2] == m[0] + 2 && m[3] == m[0] + 3) {
                                *reinterpret_cast<f32x4*>(orow + m[0]) = v;
                            } else {
#pragma unroll
                                for (int e = 0; e < 4; ++e)
                                    if (m[e] >= 0) orow[m[e]] = v[e];
                            }
                        }
                    }
                }
            }
    }
    if constexpr (GAP) {
        __syncthreads();
        for (int i = tid; i < nact * GW; i += GWD_THREADS) {
            const int ia = i / GW, sl = i - ia * GW;
            const int il = s_act[ia];
            const int m = s_map[il * GW + sl];
            if (m < 0) continue;
            float s = 0.f;
            for (int t = 0; t < tpr; ++t) s += s_gap[(size_t)(ia * tpr + t) * (MT * 32) + sl];
            p.gap[((size_t)(b0 + il) * nrect + rect) * p.C + m] = s;
        }
    }
}

// The plan: images per workgroup and the rectangle of output pixels of one workgroup.  Everything counts against one budget: the tables and
// (images x staged pixels) x PIXB, staged pixels = ((R - 1) stride + 3) x ((Wc - 1) stride + 3) -- the halo is staged as zeros, so a whole
// 7 x 7 image is 81 staged pixels.  In staged pixels of one image: width 56: 364 (80 KB, two workgroups per CU) / 684 (150 KB); width 112:
// 169 / 318; width 232: 87 / 164 (each further image of the workgroup takes one or two pixels' worth of tables).  A candidate's cost is its matrix-core time per output pixel (a pass over the group's fragments costs one tile slot
// for the stream plus the most tiles one wave has; 32 NSET pixels per slot) plus a tenth of its staged pixels per output pixel, times 1.1
// when only one workgroup fits a CU.  Candidates: 1-8 whole images; one image cut into 1-32 row bands x 1-32 column strips.  A map that no
// candidate holds is answered "does not fit", never by a failed launch.
struct GwPlan { int nimg, R, Wc, nrb, ncb; size_t lds; };

static size_t gwd_bytes(int gw, int nimg, long sp) { return (size_t)gwd_tab_bytes(gw, nimg) + (size_t)nimg * (size_t)sp * gwd_pixb(gw); }

// (GAP) the scratch of the tile sums behind the staged input: a row of MT x 32 slots per pixel tile of the workgroup's images.  Within the
// plain plan's 150 KB a rectangle has at most 22 / 10 / 6 pixel tiles (width 56 / 112 / 232): at most 6 KB, inside the 160 KB of a CU
constexpr size_t GWD_LDS_CU = 160 * 1024;
static size_t gwd_gap_bytes(int gw, int nimg, int R, int Wc) { return (size_t)nimg * ceil_div(R * Wc, 32) * gw_frag_mt(gw) * 32 * 4; }

static double gwd_cost(int gw, int nimg, int R, int Wc, long sp, size_t lds) {
    const int nset = 8 / gw_frag_mt(gw), cap = nset * GWD_PT;
    const long outpx = (long)R * Wc;
    const long tiles = (long)nimg * ((outpx + 31) / 32);
    const long full = tiles / cap, last = tiles - full * cap;
    const long slots = full * (GWD_PT + 1) + (last ? (last + nset - 1) / nset + 1 : 0);
    const double mfma = (double)slots * nset * 32 / ((double)nimg * outpx);
    return (mfma + 0.1 * (double)sp / outpx) * (lds > GWD_LDS_TWO ? 1.1 : 1.0);
}

static bool gwd_plan(int gw, int Hi, int Wi, int Ho, int Wo, int stride, GwPlan* out) {
    double best = 0.;
    bool found = false;
    auto consider = [&](int nimg, int nrb, int ncb) {
        const int R = ceil_div(Ho, nrb), Wc = ceil_div(Wo, ncb);
        const long sp = ((long)(R - 1) * stride + 3) * ((long)(Wc - 1) * stride + 3);
        if (sp > (long)(GWD_LDS_ONE / 32)) return false;
        const size_t lds = gwd_bytes(gw, nimg, sp);
        if (lds > GWD_LDS_ONE) return false;
        const double c = gwd_cost(gw, nimg, R, Wc, sp, lds);
        if (!found || c < best) {
            best = c;
            found = true;
            *out = GwPlan{nimg, R, Wc, ceil_div(Ho, R), ceil_div(Wo, Wc), lds};
        }
        return true;
    };
    for (int nimg = 1; nimg <= GWD_MAXIMG; ++nimg)
        if (!consider(nimg, 1, 1)) break;
    int last_R = 0;
    for (int nrb = 1; nrb <= std::min(Ho, GWD_MAXCUT); ++nrb) {
        if (ceil_div(Ho, nrb) == last_R) continue;
        last_R = ceil_div(Ho, nrb);
        int last_W = 0;
        for (int ncb = 1; ncb <= std::min(Wo, GWD_MAXCUT); ++ncb) {
            if (ceil_div(Wo, ncb) == last_W || (nrb == 1 && ncb == 1)) continue;
            last_W = ceil_div(Wo, ncb);
            consider(1, nrb, ncb);
        }
    }
    return found;
}

template <int GW, bool GAP>
static int launch_grouped_wide(const GwArgs& g, size_t lds, unsigned nwg, hipStream_t stream) {
    LDN_REQUIRE(allow_dynamic_lds(reinterpret_cast<const void*>(&k_grouped_wide<GW, GAP>), lds), "k_grouped_wide<%d>: cannot reserve %zu B of LDS", GW, lds);
    hipLaunchKernelGGL((k_grouped_wide<GW, GAP>), dim3(nwg), dim3(GWD_THREADS), lds, stream, g);
    LDN_CHECK_LAUNCH("k_grouped_wide");
    return LDN_OK;
}

LDN_DEFINE_TU_VIOLATIONS(tu_violations_grouped_wide)

}  // namespace ldn

using namespace ldn;

// the shape check and the plan behind the five queries: false outside ldn_grouped_wide_ok
static bool gwd_query(int C, int gw, int Hi, int Wi, int stride, GwPlan* pl) {
    return gw_frag_width(gw) && C > 0 && C % gw == 0 && (stride == 1 || stride == 2) && Hi > 0 && Wi > 0 &&
           gwd_plan(gw, Hi, Wi, (Hi - 1) / stride + 1, (Wi - 1) / stride + 1, stride, pl);
}

extern "C" int ldn_grouped_wide_ok(int C, int group_width, int Hi, int Wi, int stride) {
    GwPlan pl;
    return gwd_query(C, group_width, Hi, Wi, stride, &pl) ? 1 : 0;
}

extern "C" int ldn_grouped_wide_bands(int C, int group_width, int Hi, int Wi, int Ho, int stride) {
    GwPlan pl;
    return stride > 0 && Ho == (Hi - 1) / stride + 1 && gwd_query(C, group_width, Hi, Wi, stride, &pl) ? pl.nrb : 0;
}

extern "C" int ldn_grouped_wide_images(int C, int group_width, int Hi, int Wi, int stride) {
    GwPlan pl;
    return gwd_query(C, group_width, Hi, Wi, stride, &pl) ? pl.nimg : 0;
}

extern "C" int ldn_grouped_wide_strips(int C, int group_width, int Hi, int Wi, int stride) {
    GwPlan pl;
    return gwd_query(C, group_width, Hi, Wi, stride, &pl) ? pl.ncb : 0;
}

extern "C" size_t ldn_grouped_wide_weight_bytes(int C, int group_width) {
    if (!gw_frag_width(group_width) || C <= 0 || C % group_width) return 0;
    return (size_t)(C / group_width) * gw_frag_bytes(group_width);
}

// LDS of a launch of the plan on nimg images a workgroup, with the tile sums' scratch when gap
static size_t gwd_launch_bytes(int gw, int nimg, const GwPlan& pl, int stride, bool gap) {
    const long sp = ((long)(pl.R - 1) * stride + 3) * ((long)(pl.Wc - 1) * stride + 3);
    return gwd_bytes(gw, nimg, sp) + (gap ? gwd_gap_bytes(gw, nimg, pl.R, pl.Wc) : 0);
}

extern "C" int ldn_grouped_wide_gap_ok(int C, int group_width, int Hi, int Wi, int stride) {
    GwPlan pl;
    return gwd_query(C, group_width, Hi, Wi, stride, &pl) && gwd_launch_bytes(group_width, pl.nimg, pl, stride, true) <= GWD_LDS_CU ? 1 : 0;
}

static int grouped_wide_image(const char* name, const float* a, int lda, int B, int Hi, int Wi, int stride, int Ho, int Wo, const void* w_frag, int C,
                              int group_width, const int32_t* ch_idx, const int32_t* ch_cnt, const float* scale, const float* shift, int relu,
                              float* out, int ldo, float* gap, void* stream) {
    LDN_REQUIRE(a && w_frag && ch_idx && ch_cnt && scale && shift && out, "%s: null pointer", name);
    LDN_REQUIRE(B > 0 && Hi > 0 && Wi > 0 && stride >= 1 && Ho == (Hi - 1) / stride + 1 && Wo == (Wi - 1) / stride + 1,
                "%s: %dx%d -> %dx%d is not a 3x3 / pad 1 / stride %d geometry", name, Hi, Wi, Ho, Wo, stride);
    LDN_REQUIRE(ldn_grouped_wide_ok(C, group_width, Hi, Wi, stride),
                "%s: group width %d with %d channels on a %dx%d map at stride %d is not built (widths 56, 112 and 232, "
                "channels a multiple of the width, stride 1 or 2, a rectangle of the map in the LDS: ldn_grouped_wide_ok)", name, group_width, C, Hi, Wi, stride);
    LDN_REQUIRE(lda % 4 == 0 && ldo % 4 == 0 && lda >= C && ldo >= C, "%s: strides must be multiples of 4 and at least C", name);
    LDN_REQUIRE((uintptr_t)a % 16 == 0 && (uintptr_t)out % 16 == 0 && (uintptr_t)w_frag % 16 == 0 && (uintptr_t)scale % 16 == 0 &&
                (uintptr_t)shift % 16 == 0 && (uintptr_t)gap % 16 == 0, "%s: pointers must be 16-byte aligned", name);
    GwPlan pl;
    LDN_REQUIRE(gwd_plan(group_width, Hi, Wi, Ho, Wo, stride, &pl), "%s: the map does not fit the LDS", name);
    GwArgs g{};
    g.a = a; g.lda = lda; g.B = B; g.Hi = Hi; g.Wi = Wi; g.Ho = Ho; g.Wo = Wo; g.stride = stride;
    g.wf = static_cast<const unsigned char*>(w_frag); g.C = C; g.ch_idx = ch_idx; g.ch_cnt = ch_cnt;
    g.scale = scale; g.shift = shift; g.relu = relu; g.out = out; g.ldo = ldo; g.gap = gap;
    g.nimg = std::min(pl.nimg, B); g.R = pl.R; g.Wc = pl.Wc; g.nrb = pl.nrb; g.ncb = pl.ncb;
    g.tab_bytes = gwd_tab_bytes(group_width, g.nimg);
    const size_t plain = gwd_launch_bytes(group_width, g.nimg, pl, stride, false);
    LDN_REQUIRE(plain <= GWD_LDS_ONE, "%s: %zu B of LDS planned", name, plain);
    g.gap_off = (int)plain;                 // (a multiple of 32: the tables and every staged pixel are)
    const size_t lds = gwd_launch_bytes(group_width, g.nimg, pl, stride, gap != nullptr);
    LDN_REQUIRE(lds <= GWD_LDS_CU, "%s: %zu B of LDS planned (ldn_grouped_wide_gap_ok)", name, lds);
    const long nwg = (long)(C / group_width) * ceil_div(B, g.nimg) * g.nrb * g.ncb;
    LDN_REQUIRE(nwg < (1l << 31), "%s: too many workgroups (%ld)", name, nwg);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (gap)
        return group_width == 56 ? launch_grouped_wide<56, true>(g, lds, (unsigned)nwg, st)
             : group_width == 112 ? launch_grouped_wide<112, true>(g, lds, (unsigned)nwg, st) : launch_grouped_wide<232, true>(g, lds, (unsigned)nwg, st);
    return group_width == 56 ? launch_grouped_wide<56, false>(g, lds, (unsigned)nwg, st)
         : group_width == 112 ? launch_grouped_wide<112, false>(g, lds, (unsigned)nwg, st) : launch_grouped_wide<232, false>(g, lds, (unsigned)nwg, st);
}

extern "C" int ldn_grouped_wide_conv3x3_image(const float* a, int lda, int B, int Hi, int Wi, int stride, int Ho, int Wo,
                                              const void* w_frag, int C, int group_width, const int32_t* ch_idx, const int32_t* ch_cnt,
                                              const float* scale, const float* shift, int relu, float* out, int ldo, void* stream) {
    return grouped_wide_image("ldn_grouped_wide_conv3x3_image", a, lda, B, Hi, Wi, stride, Ho, Wo, w_frag, C, group_width, ch_idx, ch_cnt, scale, shift,
                              relu, out, ldo, nullptr, stream);
}

extern "C" int ldn_grouped_wide_conv3x3_image_gap(const float* a, int lda, int B, int Hi, int Wi, int stride, int Ho, int Wo,
                                                  const void* w_frag, int C, int group_width, const int32_t* ch_idx, const int32_t* ch_cnt,
                                                  const float* scale, const float* shift, int relu, float* out, int ldo, float* gap_partial,
                                                  void* stream) {
    LDN_REQUIRE(gap_partial, "ldn_grouped_wide_conv3x3_image_gap: null pointer");
    return grouped_wide_image("ldn_grouped_wide_conv3x3_image_gap", a, lda, B, Hi, Wi, stride, Ho, Wo, w_frag, C, group_width, ch_idx, ch_cnt, scale,
                              shift, relu, out, ldo, gap_partial, stream);
}
