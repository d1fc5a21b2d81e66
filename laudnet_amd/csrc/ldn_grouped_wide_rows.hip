// k_grouped_wide_rows<56 | 112 | 232> -- grouped 3x3 convolution + BN (+ReLU) over PACKED PIXEL ROWS on the matrix cores at the group widths of
// RegNetY-8GF (56), RegNetY-16GF (112) and RegNetY-32GF (232); gfx950, bf16x3 arithmetic, v_mfma_f32_32x32x16_bf16.  The contract of k_grouped_gw
// (ldn_grouped_gw.hip), the fragments of k_grouped_wide (ldn_grouped_wide.hip), unchanged:
//     out[r, gw g + n] = act(scale * sum_{t < 9} sum_{i < gw} a[nbr[r, t], gw g + i] * w[gw g + n, t, i] + shift),   r < M
// Per group a GEMM with M = gw output channels padded to MT = 2 / 4 / 8 row tiles of 32, N = rows in pixel tiles of 32, K = 9 gw in octets
// q = tap * (gw / 8) + octet of 8 consecutive channels; K step s covers octets 2 s and 2 s + 1 (lane half h = lane >> 5): 32 steps at width
// 56 (octet 63 is a zero pad of the fragments: no load), 63 at width 112, 131 at width 232 (octet 261 is the zero pad).
//   * A group's fragments (128 KB / 504 KB / 2096 KB) do not fit the LDS: they STREAM THROUGH REGISTERS as in k_grouped_wide, one coalesced 2 KB line per
//     (step, row tile), one step ahead of the MFMAs.  The four waves of a workgroup read the same lines of the same group within a few steps
//     of each other (L1, then the XCD's L2).
//   * WAVE = RT row tiles x up to NPT pixel tiles, accumulators resident over the whole K loop.  The form that is launched is RT = MT (one
//     wave holds EVERY row tile of its pixel tiles): an input octet is fetched through the neighbour table and split to hi / lo exactly once,
//     straight from global memory into registers as in k_grouped_gw<24>, two steps ahead.  No LDS, no barrier, no atomics.
//     RT = 1 (a wave = one row tile, the MT waves that share a pixel tile gather it again) is compiled for the A/B of DESIGN.md 4zc only.
//   * one workgroup = (group, row-tile set) x 4 NPT consecutive pixel tiles; NPT = 2, or 1 where two would leave a SIMD fewer than 3 waves at the cap
//     (gwr_tiles_per_wave); the grid and NPT depend on m_cap and the shapes only.  Width 232: RT = MT = 8 keeps 128 accumulator registers
//     per pixel tile, so NPT = 1 is the only form with every row tile in one wave (two tiles would be 256 accumulators: the whole file).
// Rows >= M are neither looked up nor written; a table entry of -1 is a zero row; columns >= C of a / out are never touched; the padded out
// channels (56-63, 112-127, 232-255) are dropped in the epilogue.
#include <stdlib.h>
#include <string.h>

#include "ldn_common.h"
#include "ldn_grouped_wide_frag.h"

namespace ldn {

constexpr int GWR_THREADS = 256;             // 4 waves: one per SIMD
constexpr int GWR_WAVES = GWR_THREADS / 64;

struct GwrArgs {
    const float* a; int lda;
    const int32_t* nbr; const int32_t* m_count; int m_cap;
    const unsigned char* wf; int C;         // [C / gw][NSTEP][MT][64 lanes][8 hi | 8 lo] bf16 (ops.pack_grouped_wide_weights)
    const float* scale; const float* shift; int relu;
    float* out; int ldo;
};

__device__ __attribute__((aligned(16))) float g_gwr_zero[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};

// The K loop of one wave over RT row tiles x NPT live pixel tiles.  row[pt][t] = this lane's neighbour row of tap t (-1: a zero row or a row
// past the count).  Fragments of step s + 1 and input octets of step s + 2 are in flight under the MFMAs of step s.
template <int GW, int RT, int CAP, int NPT>
__device__ __forceinline__ void gwr_kloop(const unsigned char* wbase, const float* abase, int lda, const int (&row)[CAP][9], int h,
                                          f32x16 (&acc)[RT][CAP]) {
    constexpr int MT = GwCfg<GW>::MT, NSTEP = GwCfg<GW>::NSTEP, OCT = GW / 8;
    auto request = [&](int s, f32x4 (&x0)[NPT], f32x4 (&x1)[NPT]) {
        const int q = 2 * s + h;
        const int t = q / OCT, oct = q - t * OCT;                                    // t = 9: octet 63 of width 56 / 261 of width 232, zero weights
#pragma unroll
        for (int pt = 0; pt < NPT; ++pt) {
            int ar = -1;
#pragma unroll
            for (int u = 0; u < 9; ++u) ar = t == u ? row[pt][u] : ar;
            const float* src = ar >= 0 ? abase + (size_t)ar * lda + 8 * oct : g_gwr_zero;
            x0[pt] = *reinterpret_cast<const f32x4*>(src);
            x1[pt] = *reinterpret_cast<const f32x4*>(src + 4);
        }
    };
    bf16x8 ah[RT], al[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        ah[rt] = *reinterpret_cast<const bf16x8*>(wbase + rt * 2048);
        al[rt] = *reinterpret_cast<const bf16x8*>(wbase + rt * 2048 + 16);
    }
    f32x4 c0[NPT], c1[NPT], n0[NPT], n1[NPT];
    request(0, c0, c1);
    request(1, n0, n1);
#pragma unroll 1
    for (int s = 0; s < NSTEP; ++s) {
        bf16x8 bh[NPT], bl[NPT];
#pragma unroll
        for (int pt = 0; pt < NPT; ++pt) {
            split8<f32x4>(c0[pt], c1[pt], bh[pt], bl[pt]);
            c0[pt] = n0[pt];
            c1[pt] = n1[pt];
        }
        request(min(s + 2, NSTEP - 1), n0, n1);
        const size_t wn = (size_t)min(s + 1, NSTEP - 1) * (MT * 2048);
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            const bf16x8 nh = *reinterpret_cast<const bf16x8*>(wbase + wn + rt * 2048);
            const bf16x8 nl = *reinterpret_cast<const bf16x8*>(wbase + wn + rt * 2048 + 16);
#pragma unroll
            for (int pt = 0; pt < NPT; ++pt) {
                acc[rt][pt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[rt], bh[pt], acc[rt][pt], 0, 0, 0);
                acc[rt][pt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[rt], bl[pt], acc[rt][pt], 0, 0, 0);
                acc[rt][pt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[rt], bh[pt], acc[rt][pt], 0, 0, 0);
            }
            ah[rt] = nh;
            al[rt] = nl;
        }
    }
}

// RT = 8 (width 232, 128 accumulator registers): held to two waves per SIMD -- 234 registers, no scratch; unbounded the compiler takes 374 and one wave
template <int GW, int RT, int NPT>
__global__ __launch_bounds__(GWR_THREADS, RT == 8 ? 2 : 1) void k_grouped_wide_rows(const GwrArgs p) {
    typedef GwCfg<GW> cfg;
    constexpr int MT = cfg::MT, NSTEP = cfg::NSTEP, NRS = MT / RT;
    static_assert(MT % RT == 0, "wave roles");
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int M = p.m_count ? min(p.m_count[0], p.m_cap) : p.m_cap;
    const int ntiles = (M + 31) / 32;
    const int t0 = (blockIdx.x * GWR_WAVES + wave) * NPT;                            // this wave's pixel tiles: t0 .. t0 + npt - 1
    if (t0 >= ntiles) return;                                                        // (wave-uniform; the kernel has no barrier)
    const int npt = min(NPT, ntiles - t0);
    const int g = blockIdx.y / NRS, mt0 = (blockIdx.y - g * NRS) * RT;
    const int n = lane & 31, h = lane >> 5;
    int row[NPT][9];
    f32x16 acc[RT][NPT];
#pragma unroll
    for (int pt = 0; pt < NPT; ++pt) {
        const int r = (t0 + pt) * 32 + n;
#pragma unroll
        for (int t = 0; t < 9; ++t) row[pt][t] = (pt < npt && r < M) ? p.nbr[(size_t)r * 9 + t] : -1;
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[rt][pt][e] = 0.f;
    }
    const unsigned char* const wbase = p.wf + (size_t)g * (NSTEP * MT * 2048) + mt0 * 2048 + lane * 32;
    const float* const abase = p.a + g * GW;
    if constexpr (NPT == 1) {
        gwr_kloop<GW, RT, NPT, 1>(wbase, abase, p.lda, row, h, acc);
    } else if constexpr (NPT == 2) {
        if (npt == 1) gwr_kloop<GW, RT, NPT, 1>(wbase, abase, p.lda, row, h, acc);        // the tile count as a constant: straight-line K steps
        else gwr_kloop<GW, RT, NPT, 2>(wbase, abase, p.lda, row, h, acc);
    } else {
        static_assert(NPT == 4, "pixel tiles per wave: 1, 2 or 4");
        switch (npt) {
            case 1: gwr_kloop<GW, RT, NPT, 1>(wbase, abase, p.lda, row, h, acc); break;
            case 2: gwr_kloop<GW, RT, NPT, 2>(wbase, abase, p.lda, row, h, acc); break;
            case 3: gwr_kloop<GW, RT, NPT, 3>(wbase, abase, p.lda, row, h, acc); break;
            default: gwr_kloop<GW, RT, NPT, 4>(wbase, abase, p.lda, row, h, acc); break;
        }
    }
    // C layout of 32x32: register 4 Q + e of lane (n, h) is out channel 32 mt + 8 Q + 4 h + e of the group, row n of the tile; >= GW: pads
#pragma unroll
    for (int pt = 0; pt < NPT; ++pt) {
        const int r = (t0 + pt) * 32 + n;
        if (pt < npt && r < M) {
            float* const orow = p.out + (size_t)r * p.ldo + g * GW;
#pragma unroll
            for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                for (int Q = 0; Q < 4; ++Q) {
                    const int sb = 32 * (mt0 + rt) + 8 * Q + 4 * h;
                    if (sb < GW) {
                        const int c = g * GW + sb;
                        const f32x4 sc = *reinterpret_cast<const f32x4*>(p.scale + c), sf = *reinterpret_cast<const f32x4*>(p.shift + c);
                        f32x4 v;
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            v[e] = acc[rt][pt][4 * Q + e] * sc[e] + sf[e];
                            if (p.relu) v[e] = fmaxf(v[e], 0.f);
                        }
                        *reinterpret_cast<f32x4*>(orow + sb) = v;
                    }
                }
        }
    }
}

template <int GW, int RT, int NPT>
static int launch_grouped_wide_rows(const GwrArgs& g, hipStream_t stream) {
    constexpr int NRS = GwCfg<GW>::MT / RT;
    const int bx = (int)(((long)g.m_cap + 32 * GWR_WAVES * NPT - 1) / (32 * GWR_WAVES * NPT));
    const long by = (long)(g.C / GW) * NRS;
    LDN_REQUIRE(by <= 65535, "k_grouped_wide_rows<%d>: too many groups (%d channels)", GW, g.C);
    hipLaunchKernelGGL((k_grouped_wide_rows<GW, RT, NPT>), dim3((unsigned)bx, (unsigned)by), dim3(GWR_THREADS), 0, stream, g);
    LDN_CHECK_LAUNCH("k_grouped_wide_rows");
    return LDN_OK;
}

// Pixel tiles per wave.  Two halve the fragment bytes a wave streams per MFMA, but a wave then walks its two tiles' K steps behind one another
// and (width 112: 282 registers) is alone on its SIMD: where the launch has few waves per SIMD the K loop's load latency, not the matrix
// pipe, is its time, and one tile per wave -- twice the waves, two to four on a SIMD -- is up to 1.7x faster (14 x 14 at width
// 112, 7 x 7 at width 56, half of 64 images kept).  The plan sees m_cap, never the device-side count: one tile per wave below 3 waves per
// SIMD (256 CUs x 4) AT THE CAP, the threshold that separates the shapes measured with half the cap kept.
constexpr long GWR_FILL = 3 * 1024;
static int gwr_tiles_per_wave(int C, int gw, int m_cap) {
    if (gw_frag_mt(gw) * 2 * 16 > 128) return 1;                                     // width 232: one tile's accumulators are 128 registers
    return (long)(C / gw) * (((long)m_cap + 63) / 64) < GWR_FILL ? 1 : 2;
}

// The wave roles.  Launched: every row tile of the group in one wave, one or two pixel tiles (gwr_tiles_per_wave).
// LDN_GROUPED_WIDE_ROWS_FORM (read per call; tuning, tests and the measurements of DESIGN.md 4zc only) overrides the plan: "b1" / "b2" / "b4" =
// that form with one / two / four pixel tiles, "a" = one row tile x four pixel tiles per wave (k_grouped_wide's split, the input gathered once
// per row tile).  At width 232 only "a" and "b1" are compiled: "b2" and "b4" launch the plan's choice.
template <int GW>
static int dispatch_grouped_wide_rows(const GwrArgs& g, hipStream_t stream) {
    constexpr int MT = GwCfg<GW>::MT;
    const char* form = getenv("LDN_GROUPED_WIDE_ROWS_FORM");
    if (form && !strcmp(form, "a")) return launch_grouped_wide_rows<GW, 1, 4>(g, stream);
    if constexpr (MT * 2 * 16 > 128) {       // width 232: two pixel tiles of every row tile do not fit the accumulators; "b2" / "b4" are not
        return launch_grouped_wide_rows<GW, MT, 1>(g, stream);      // compiled and fall back to the plan's choice, which is always "b1"
    } else {
        if (form && !strcmp(form, "b4")) return launch_grouped_wide_rows<GW, MT, 4>(g, stream);
        const int npt = form && !strcmp(form, "b1") ? 1 : form && !strcmp(form, "b2") ? 2 : gwr_tiles_per_wave(g.C, GW, g.m_cap);
        return npt == 1 ? launch_grouped_wide_rows<GW, MT, 1>(g, stream) : launch_grouped_wide_rows<GW, MT, 2>(g, stream);
    }
}

}  // namespace ldn

using namespace ldn;

extern "C" int ldn_grouped_wide_rows_ok(int C, int group_width) {
    return gw_frag_width(group_width) && C > 0 && C % group_width == 0 ? 1 : 0;
}

extern "C" int ldn_grouped_wide_rows_tiles(int C, int group_width, int m_cap) {
    return ldn_grouped_wide_rows_ok(C, group_width) && m_cap > 0 ? gwr_tiles_per_wave(C, group_width, m_cap) : 0;
}

extern "C" int ldn_grouped_wide_conv3x3_rows(const float* a, int lda, const int32_t* nbr, const int32_t* m_count, int m_cap,
                                             const void* w_frag, int C, int group_width, const float* scale, const float* shift,
                                             int relu, float* out, int ldo, void* stream) {
    LDN_REQUIRE(a && nbr && w_frag && scale && shift && out, "ldn_grouped_wide_conv3x3_rows: null pointer");
    LDN_REQUIRE(ldn_grouped_wide_rows_ok(C, group_width),
                "ldn_grouped_wide_conv3x3_rows: group width %d with %d channels is not built (widths 56, 112 and 232, channels a multiple of the width)",
                group_width, C);
    LDN_REQUIRE(lda % 4 == 0 && ldo % 4 == 0 && lda >= C && ldo >= C,
                "ldn_grouped_wide_conv3x3_rows: strides must be multiples of 4 and at least C");
    LDN_REQUIRE((uintptr_t)a % 16 == 0 && (uintptr_t)out % 16 == 0 && (uintptr_t)w_frag % 16 == 0 && (uintptr_t)scale % 16 == 0 &&
                (uintptr_t)shift % 16 == 0, "ldn_grouped_wide_conv3x3_rows: pointers must be 16-byte aligned");
    LDN_REQUIRE(m_cap <= INT32_MAX - 256, "ldn_grouped_wide_conv3x3_rows: too many rows (%d)", m_cap);      // row indices of a last tile stay ints
    if (m_cap <= 0) return LDN_OK;
    GwrArgs g{};
    g.a = a; g.lda = lda; g.nbr = nbr; g.m_count = m_count; g.m_cap = m_cap; g.wf = static_cast<const unsigned char*>(w_frag); g.C = C;
    g.scale = scale; g.shift = shift; g.relu = relu; g.out = out; g.ldo = ldo;
    hipStream_t st = static_cast<hipStream_t>(stream);
    return group_width == 56 ? dispatch_grouped_wide_rows<56>(g, st)
                             : group_width == 112 ? dispatch_grouped_wide_rows<112>(g, st) : dispatch_grouped_wide_rows<232>(g, st);
}
