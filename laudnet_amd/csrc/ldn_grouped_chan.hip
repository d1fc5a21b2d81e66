// k_grouped_chan<8 | 16 | 24> -- LAD-RegNet conv b in CHANNEL mode (and the 'both' branch) on the matrix cores: grouped 3x3 convolution + BN
// (+ReLU) over a dense image whose columns are LEFT-PACKED per image (laud_regnet.py:160-189; gfx950, bf16x3 arithmetic), the contract of
// k_grouped3x3_chan (ldn_regnet.hip): column j of image b is channel ch_idx[b, j], ascending, j < ch_cnt[b];
//     out[b, p, j] = act(scale[c] * sum_{t < 9} sum_{q active in group(c)} a[b, pix(p, t), q] * w[c, t, ch(q) - gw g] + shift[c]),  c = ch_idx[b, j]
// and columns ch_cnt[b] <= j < C are written as zeros.  The mask multiplies AFTER conv + BN + ReLU, so a masked channel is an exact zero:
// the DENSE gw x gw x 9 product of a group with zeros in the inactive input slots is exact (a zero splits into hi = 0, lo = 0), the weight
// fragments of the packed-row kernels (ops.pack_grouped16_weights, ops.pack_grouped_mfma_weights) serve unchanged with no per-image gather,
// and so do their K steps, lane maps and C layouts (k_grouped16_mfma, k_grouped_gw<8 | 24>).  What is new here is the EXPANSION of the packed
// input columns into their group slots, the COMPRESSION of the active output slots back into packed columns, and the skipping of groups with
// no active channel.  The cost of the form: an active group does the full gw x gw work however few of its channels are active.
// One 512-thread workgroup = (image, chunk of groups, band of output rows), as k_grouped16_img:
//   1. from ch_idx / ch_cnt: the slot -> packed-column map of the chunk's groups (-1: inactive) and the list of its ACTIVE groups;
//   2. the zeros of this workgroup's share of the columns [ch_cnt[b], C); a chunk without an active group ends here;
//   3. the fragments of the active groups and the band's input rows (+ one halo row on each side) go to LDS, the rows EXPANDED: channel c sits
//      in slot c - gw g of its group, inactive slots are zeros, one zero pixel serves the taps outside the image; empty groups are not staged;
//   4. work items = (pixel tile, active group) dealt to the 8 waves; the im2col is a per-lane LDS address computed from the geometry;
//   5. epilogue: scale, shift, ReLU; a lane stores those of its output slots that are active to their packed column (one 16-byte store when
//      its four slots are four consecutive, aligned columns -- whole active quads, the case of granularities that are multiples of 4).
// Input columns >= ch_cnt[b] and the pad columns of lda are never read; output columns >= C are never written.  No atomics: deterministic.
#include <algorithm>
#include <initializer_list>
#include <type_traits>

#include "ldn_common.h"

namespace ldn {

template <int GW> struct GcCfg;
template <> struct GcCfg<8> { static constexpr int STEPS = 3, TILE = 16; };       // v_mfma_f32_16x16x32_bf16, tap 4 s + kg
template <> struct GcCfg<16> { static constexpr int STEPS = 5, TILE = 16; };      // v_mfma_f32_16x16x32_bf16, tap 2 s + (kg >> 1), channels 8 (kg & 1)
template <> struct GcCfg<24> { static constexpr int STEPS = 14, TILE = 32; };     // v_mfma_f32_32x32x16_bf16, chunk q = 2 s + h = 3 tap + octet
constexpr int GC_THREADS = 512;
constexpr int GC_MAXG = 16;                 // groups per workgroup (the active-group list is one ballot of wave 0)
constexpr size_t GC_LDS_TWO = 80 * 1024;    // two workgroups per CU
constexpr size_t GC_LDS_ONE = 150 * 1024;   // one

struct GcArgs {
    const float* a; int lda;
    int B, Hi, Wi, Ho, Wo, stride;
    const unsigned char* wf; int C;         // [C / gw][STEPS][64 lanes][8 hi | 8 lo] bf16
    const int32_t* ch_idx; const int32_t* ch_cnt;
    const float* scale; const float* shift; int relu;
    float* out; int ldo;
    int gchunk, in_ld;                      // groups per workgroup; floats per staged pixel (gw gchunk + 4)
    int R, nbands;                          // output rows per workgroup (Ho: the whole image), bands per image
    int tab_bytes;                          // the tables in front of the fragments
    float* gap;                             // (GAP) [image][band][C] channel sums of the band's output, packed-column order
};

__host__ __device__ inline int gc_frag_bytes(int gw) { return (gw == 24 ? 14 : gw == 16 ? 5 : 3) * 64 * 32; }
__host__ __device__ inline int gc_tab_bytes(int gw, int ng) { return round_up((ng * gw + ng + 4) * 4, 16); }     // map [ng gw], active list [ng], count

// GAP: the epilogue also leaves the sums of the band's output pixels per packed column (the SE squeeze of the block, ldn_se_gate_image),
// as k_grouped_gw_img's gap form does: a DPP tree over the 16 pixels of a lane row, one slot of LDS per (active group, 16-pixel piece),
// then the pieces in ascending order -- no atomics, the same bits in every launch.  The scratch lies behind the staged rows
// (gc_gap_bytes: the plain form's plan does not count it; ldn_grouped_chan_mfma_gap_ok answers whether it still fits).  The zeros of the
// columns behind the count are written with the output's zeros (step 2), so every element of gap has exactly one writer.
template <int GW, bool GAP = false>
__global__ __launch_bounds__(GC_THREADS, 2) void k_grouped_chan(const GcArgs p) {
    typedef GcCfg<GW> cfg;
    constexpr int STEPS = cfg::STEPS, TILE = cfg::TILE, FRAG = STEPS * 64 * 32, QG = GW / 4;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int G = p.C / GW;
    // workgroup order as k_grouped16_img: the group chunks of one (image, band) pair are consecutive workgroups of one XCD
    const int nch = (G + p.gchunk - 1) / p.gchunk;
    const int per = 8 * nch, jid = (int)(blockIdx.x % (unsigned)per);
    const long pair = (long)(blockIdx.x / (unsigned)per) * 8 + (jid & 7);
    if (pair >= (long)p.B * p.nbands) return;
    const int b = (int)(pair / p.nbands), band = (int)(pair - (long)b * p.nbands);
    const int kch = jid >> 3, g0 = kch * p.gchunk;
    const int ng = min(p.gchunk, G - g0);
    int* const s_map = reinterpret_cast<int*>(smem);            // [ng][GW] packed column of the slot, -1: inactive
    int* const s_act = s_map + p.gchunk * GW;                   // [ng] the active groups of the chunk, in order
    int* const s_nact = s_act + p.gchunk;
    unsigned char* const s_w = smem + p.tab_bytes;              // [active group][FRAG]
    float* const s_in = reinterpret_cast<float*>(s_w + (size_t)p.gchunk * FRAG);
    const int cnt = p.ch_cnt[b];
    LDN_DCHECK(cnt >= 0 && cnt <= p.C, 413);
    const int Cb = min(max(cnt, 0), p.C);
    // ---- 1. slot map and active groups
    for (int i = tid; i < ng * GW; i += GC_THREADS) s_map[i] = -1;
    __syncthreads();
    const int32_t* const chb = p.ch_idx + (size_t)b * p.C;
    const int c_lo = g0 * GW, c_hi = (g0 + ng) * GW;
    for (int j = tid; j < Cb; j += GC_THREADS) {
        const int c = chb[j];
        LDN_DCHECK(c >= 0 && c < p.C, 411);                                     // channel list entries
        LDN_DCHECK(j == 0 || c > chb[j - 1], 412);                              // ascending
        if (c >= c_lo && c < c_hi) s_map[c - c_lo] = j;
    }
    __syncthreads();
    if (wave == 0) {
        bool act = false;
        if (lane < ng)
            for (int s = 0; s < GW; ++s) act |= s_map[lane * GW + s] >= 0;
        const unsigned long long m = __ballot(act);
        if (act) s_act[__popcll(m & ((1ull << lane) - 1ull))] = lane;
        if (lane == 0) *s_nact = __popcll(m);
    }
    __syncthreads();
    const int nact = *s_nact;
    // this workgroup's band of output rows and the input rows it reads (pad 1: one halo row on each side, inside the image)
    const int y0 = band * p.R, rows_out = min(p.R, p.Ho - y0);
    const int npix = rows_out * p.Wo;
    float* const obase = p.out + ((size_t)b * p.Ho * p.Wo + (size_t)y0 * p.Wo) * p.ldo;
    // ---- 2. zeros behind the count: the chunks of a pair share the columns [Cb, C)
    {
        const int zc = p.C - Cb;
        const int z0 = Cb + (int)((long)zc * kch / nch), nz = Cb + (int)((long)zc * (kch + 1) / nch) - z0;
        for (int i = tid; i < npix * nz; i += GC_THREADS) {
            const int px = i / nz;
            obase[(size_t)px * p.ldo + z0 + (i - px * nz)] = 0.f;
        }
        if constexpr (GAP)
            for (int i = tid; i < nz; i += GC_THREADS) p.gap[((size_t)b * p.nbands + band) * p.C + z0 + i] = 0.f;
    }
    if (nact == 0) return;                                      // (uniform) no active channel in the chunk: nothing staged, no MFMA
    // ---- 3. fragments of the active groups; the band's input rows, expanded
    for (int i = tid; i < nact * (FRAG / 16); i += GC_THREADS) {
        const int ga = i / (FRAG / 16), r = i - ga * (FRAG / 16);
        reinterpret_cast<f32x4*>(s_w)[i] = reinterpret_cast<const f32x4*>(p.wf + (size_t)(g0 + s_act[ga]) * FRAG)[r];
    }
    const int iy0 = max(y0 * p.stride - 1, 0), iy1 = min((y0 + rows_out - 1) * p.stride + 1, p.Hi - 1);
    const int HWi = (iy1 - iy0 + 1) * p.Wi;                                // staged pixels
    const float* const abase = p.a + ((size_t)b * p.Hi * p.Wi + (size_t)iy0 * p.Wi) * p.lda;
    const int qpp = nact * QG;                                              // 16-byte pieces per staged pixel
    const int npiece = HWi * qpp;
    for (int i0 = tid; i0 < npiece; i0 += 4 * GC_THREADS) {                 // four pieces per thread in flight
        f32x4 v[4];
        int dst[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = min(i0 + u * GC_THREADS, npiece - 1);
            const int px = i / qpp, q = i - px * qpp;
            const int ga = q / QG, sl = (q - ga * QG) * 4;
            const i32x4 m = *reinterpret_cast<const i32x4*>(s_map + s_act[ga] * GW + sl);
            const float* src = abase + (size_t)px * p.lda;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[u][e] = m[e] >= 0 ? src[m[e]] : 0.f;
            dst[u] = px * p.in_ld + ga * GW + sl;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (i0 + u * GC_THREADS < npiece) *reinterpret_cast<f32x4*>(s_in + dst[u]) = v[u];
    }
    for (int i = tid; i < p.in_ld; i += GC_THREADS) s_in[(size_t)HWi * p.in_ld + i] = 0.f;     // the zero pixel
    __syncthreads();
    // ---- 4. (pixel tile, active group) items
    const int n = lane & (TILE - 1), kg = lane / TILE;          // B operand / output column = pixel n of the tile; k-group kg of a step
    const int ntile = (npix + TILE - 1) / TILE;
    const int nsub = ntile * (TILE / 16);                       // (GAP) 16-pixel pieces per group
    float* const s_gap = s_in + ((size_t)HWi + 1) * p.in_ld;    // (GAP) [active group][piece][GW slots]
    for (int w = wave; w < ntile * nact; w += GC_THREADS / 64) {
        const int ga = w / ntile, tile = w - ga * ntile;
        const int gl = __builtin_amdgcn_readfirstlane(s_act[ga]);
        const int q = tile * TILE + n;
        const bool valid = q < npix;
        const int ly = (valid ? q : 0) / p.Wo, ox = (valid ? q : 0) - ly * p.Wo;
        const int oy = y0 + ly;
        typename std::conditional<GW == 24, f32x16, f32x4>::type acc;
#pragma unroll
        for (int e = 0; e < (GW == 24 ? 16 : 4); ++e) acc[e] = 0.f;
        const unsigned char* wfr = s_w + (size_t)ga * FRAG + lane * 32;
#pragma unroll
        for (int s = 0; s < STEPS; ++s) {
            // this lane's tap and first channel slot of the step (the maps of k_grouped_gw<8 | 24> and k_grouped16_mfma)
            const int ck = GW == 24 ? 2 * s + kg : 0;
            const int t = GW == 24 ? ck / 3 : GW == 16 ? 2 * s + (kg >> 1) : 4 * s + kg;
            const int ch = GW == 24 ? 8 * (ck % 3) : GW == 16 ? 8 * (kg & 1) : 0;
            const int iy = oy * p.stride - 1 + t / 3, ix = ox * p.stride - 1 + t % 3;
            const bool inb = valid && t < 9 && iy >= 0 && iy < p.Hi && ix >= 0 && ix < p.Wi;
            const float* src = s_in + (size_t)(inb ? (iy - iy0) * p.Wi + ix : HWi) * p.in_ld + ga * GW + ch;
            const f32x4 x0 = *reinterpret_cast<const f32x4*>(src), x1 = *reinterpret_cast<const f32x4*>(src + 4);
            bf16x8 bh, bl;
            split8<f32x4>(x0, x1, bh, bl);
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
        // ---- 5. C layout.  32x32: register 4 Q + e of lane (n, kg) is output slot 8 Q + 4 kg + e (Q = 3: slots 24-31, dropped).
        //                    16x16: register e of lane (n, kg) is output slot 4 kg + e (width 8, kg >= 2: slots 8-15, dropped).
        float* const orow = obase + (size_t)q * p.ldo;
#pragma unroll
        for (int Q = 0; Q < (GW == 24 ? 3 : 1); ++Q) {
            const int sb = GW == 24 ? 8 * Q + 4 * kg : 4 * kg;
            if constexpr (GAP) {
                // every lane takes part in the DPP sums; lanes without output (tile tail; width 8, kg >= 2) add zeros and store nothing.
                // The values are those of the plain branch below (the same expression on the same operands), inactive slots included:
                // their sums go to LDS and are dropped by the final pass.
                const bool has_out = GW != 8 || kg < 2;
                const int c = (g0 + gl) * GW + (has_out ? sb : sb - 8);
                const f32x4 sc = *reinterpret_cast<const f32x4*>(p.scale + c), sh = *reinterpret_cast<const f32x4*>(p.shift + c);
                f32x4 v, t4;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    v[e] = acc[4 * Q + e] * sc[e] + sh[e];
                    if (p.relu) v[e] = fmaxf(v[e], 0.f);
                    t4[e] = row16_sum(valid && has_out ? v[e] : 0.f);
                }
                if (valid && has_out) {
                    const i32x4 m = *reinterpret_cast<const i32x4*>(s_map + gl * GW + sb);
                    if (m[0] >= 0 && (m[0] & 3) == 0 && m[1] == m[0] + 1 && m[2] == m[0] + 2 && m[3] == m[0] + 3) {
                        *reinterpret_cast<f32x4*>(orow + m[0]) = v;
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (m[e] >= 0) orow[m[e]] = v[e];
                    }
                }
                const int sub = GW == 24 ? 2 * tile + ((lane >> 4) & 1) : tile;
                if ((lane & 15) == 0 && has_out) *reinterpret_cast<f32x4*>(s_gap + ((size_t)ga * nsub + sub) * GW + sb) = t4;
            } else if (valid && (GW != 8 || kg < 2)) {
                const int c = (g0 + gl) * GW + sb;
                const f32x4 sc = *reinterpret_cast<const f32x4*>(p.scale + c), sh = *reinterpret_cast<const f32x4*>(p.shift + c);
                const i32x4 m = *reinterpret_cast<const i32x4*>(s_map + gl * GW + sb);
                f32x4 v;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    v[e] = acc[4 * Q + e] * sc[e] + sh[e];
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
    if constexpr (GAP) {
        __syncthreads();
        for (int i = tid; i < nact * GW; i += GC_THREADS) {
            const int ga = i / GW, sl = i - ga * GW;
            const int m = s_map[s_act[ga] * GW + sl];
            if (m < 0) continue;
            float s = 0.f;
            for (int t = 0; t < nsub; ++t) s += s_gap[((size_t)ga * nsub + t) * GW + sl];
            p.gap[((size_t)b * p.nbands + band) * p.C + m] = s;
        }
    }
}

// Groups per workgroup and output rows per workgroup (false: not even the three input rows of one output row of one group fit).
// Whole images when one group's does with room for a second workgroup on the CU, then as many groups as keep that room; else bands of output
// rows with one group per workgroup -- at two workgroups per CU unless that leaves fewer than four rows a band (RegNetY-1.6GF's first block,
// 112 x 112 at stride 2: three input rows per output row), then one.  The tables count against the same budget as the rows and the fragments,
// so a map near a limit is answered "does not fit", never by a failed launch (the lesson recorded at gi_plan, ldn_grouped.hip).
static size_t gc_bytes(int gw, int ng, long in_rows, int Wi) {
    return (size_t)gc_tab_bytes(gw, ng) + (size_t)ng * gc_frag_bytes(gw) + ((size_t)in_rows * Wi + 1) * (gw * ng + 4) * 4;
}

// (GAP) the scratch of the channel sums behind the staged rows: one slot per (group, 16 output pixels), out_rows output rows a workgroup
static size_t gc_gap_bytes(int gw, int ng, long out_rows, int Wo) {
    const int tile = gw == 24 ? 32 : 16;
    return (size_t)ng * ceil_div((int)(out_rows * Wo), tile) * (tile / 16) * gw * 4;
}

static bool gc_plan(int C, int gw, int Hi, int Wi, int Ho, int stride, int* ng_out, int* R_out) {
    const int G = C / gw;
    if (gc_bytes(gw, 1, Hi, Wi) <= GC_LDS_TWO) {
        int ng = 1;
        while (ng < G && ng < GC_MAXG && gc_bytes(gw, ng + 1, Hi, Wi) <= GC_LDS_TWO) ++ng;
        *ng_out = ceil_div(G, ceil_div(G, ng));
        *R_out = Ho;
        return true;
    }
    for (const size_t budget : {GC_LDS_TWO, GC_LDS_ONE}) {
        int R = 0;                                 // (R + 1 - 1) stride + 3 input rows for R + 1 output rows
        while (R < Ho && gc_bytes(gw, 1, std::min<long>(Hi, (long)R * stride + 3), Wi) <= budget) ++R;
        if (R >= std::min(4, Ho) || (budget == GC_LDS_ONE && R >= 1)) {
            *ng_out = 1;
            *R_out = ceil_div(Ho, ceil_div(Ho, R));
            return true;
        }
    }
    return false;
}

template <int GW, bool GAP>
static int launch_grouped_chan(const GcArgs& g, size_t lds, unsigned nwg, hipStream_t stream) {
    LDN_REQUIRE(allow_dynamic_lds(reinterpret_cast<const void*>(&k_grouped_chan<GW, GAP>), lds), "k_grouped_chan<%d>: cannot reserve %zu B of LDS", GW, lds);
    hipLaunchKernelGGL((k_grouped_chan<GW, GAP>), dim3(nwg), dim3(GC_THREADS), lds, stream, g);
    LDN_CHECK_LAUNCH("k_grouped_chan");
    return LDN_OK;
}

LDN_DEFINE_TU_VIOLATIONS(tu_violations_grouped_chan)

}  // namespace ldn

using namespace ldn;

extern "C" int ldn_grouped_chan_mfma_ok(int C, int group_width, int Hi, int Wi, int stride) {
    int ng = 0, R = 0;
    return ((group_width == 8 || group_width == 16 || group_width == 24) && C > 0 && C % group_width == 0 && (stride == 1 || stride == 2) &&
            Hi > 0 && Wi > 0 && gc_plan(C, group_width, Hi, Wi, (Hi - 1) / stride + 1, stride, &ng, &R)) ? 1 : 0;
}

extern "C" int ldn_grouped_chan_mfma_bands(int C, int group_width, int Hi, int Wi, int Ho, int stride) {
    int ng = 0, R = 0;
    if (!ldn_grouped_chan_mfma_ok(C, group_width, Hi, Wi, stride) || Ho != (Hi - 1) / stride + 1) return 0;
    if (!gc_plan(C, group_width, Hi, Wi, Ho, stride, &ng, &R)) return 0;
    return ceil_div(Ho, R);
}

// LDS of a launch of the plan (ng groups, R output rows a workgroup), with the channel sums' scratch when gap
static size_t gc_launch_bytes(int gw, int ng, int R, int Hi, int Wi, int Ho, int Wo, int stride, bool gap) {
    const long in_rows = R == Ho ? (long)Hi : std::min<long>(Hi, (long)(R - 1) * stride + 3);
    return gc_bytes(gw, ng, in_rows, Wi) + (gap ? gc_gap_bytes(gw, ng, R, Wo) : 0);
}

constexpr size_t GC_LDS_CU = 160 * 1024;    // the LDS of a CU: the gap form may use what the plain plan's budget leaves of it

extern "C" int ldn_grouped_chan_mfma_gap_ok(int C, int group_width, int Hi, int Wi, int stride) {
    int ng = 0, R = 0;
    if (!ldn_grouped_chan_mfma_ok(C, group_width, Hi, Wi, stride)) return 0;
    const int Ho = (Hi - 1) / stride + 1, Wo = (Wi - 1) / stride + 1;
    if (!gc_plan(C, group_width, Hi, Wi, Ho, stride, &ng, &R)) return 0;
    return gc_launch_bytes(group_width, ng, R, Hi, Wi, Ho, Wo, stride, true) <= GC_LDS_CU ? 1 : 0;
}

static int grouped_chan_image(const char* name, const float* a, int lda, int B, int Hi, int Wi, int stride, int Ho, int Wo, const void* w_frag, int C,
                              int group_width, const int32_t* ch_idx, const int32_t* ch_cnt, const float* scale, const float* shift, int relu,
                              float* out, int ldo, float* gap, void* stream) {
    LDN_REQUIRE(a && w_frag && ch_idx && ch_cnt && scale && shift && out, "%s: null pointer", name);
    LDN_REQUIRE(B > 0 && Hi > 0 && Wi > 0 && stride >= 1 && Ho == (Hi - 1) / stride + 1 && Wo == (Wi - 1) / stride + 1,
                "%s: %dx%d -> %dx%d is not a 3x3 / pad 1 / stride %d geometry", name, Hi, Wi, Ho, Wo, stride);
    LDN_REQUIRE(ldn_grouped_chan_mfma_ok(C, group_width, Hi, Wi, stride),
                "%s: group width %d with %d channels on a %dx%d map at stride %d is not built (widths 8, 16 and 24, "
                "channels a multiple of the width, stride 1 or 2, three rows of one group in the LDS: ldn_grouped_chan_mfma_ok)", name, group_width, C, Hi, Wi, stride);
    LDN_REQUIRE(lda % 4 == 0 && ldo % 4 == 0 && lda >= C && ldo >= C, "%s: strides must be multiples of 4 and at least C", name);
    LDN_REQUIRE((uintptr_t)a % 16 == 0 && (uintptr_t)out % 16 == 0 && (uintptr_t)w_frag % 16 == 0 && (uintptr_t)scale % 16 == 0 &&
                (uintptr_t)shift % 16 == 0 && (uintptr_t)gap % 16 == 0, "%s: pointers must be 16-byte aligned", name);
    GcArgs g{};
    g.a = a; g.lda = lda; g.B = B; g.Hi = Hi; g.Wi = Wi; g.Ho = Ho; g.Wo = Wo; g.stride = stride;
    g.wf = static_cast<const unsigned char*>(w_frag); g.C = C; g.ch_idx = ch_idx; g.ch_cnt = ch_cnt;
    g.scale = scale; g.shift = shift; g.relu = relu; g.out = out; g.ldo = ldo; g.gap = gap;
    LDN_REQUIRE(gc_plan(C, group_width, Hi, Wi, Ho, stride, &g.gchunk, &g.R), "%s: the map does not fit the LDS", name);
    g.nbands = ceil_div(Ho, g.R);
    g.in_ld = group_width * g.gchunk + 4;
    g.tab_bytes = gc_tab_bytes(group_width, g.gchunk);
    const size_t lds = gc_launch_bytes(group_width, g.gchunk, g.R, Hi, Wi, Ho, Wo, stride, gap != nullptr);
    LDN_REQUIRE(lds <= (gap ? GC_LDS_CU : GC_LDS_ONE), "%s: %zu B of LDS planned%s", name, lds, gap ? " (ldn_grouped_chan_mfma_gap_ok)" : "");
    const long pairs = (long)B * g.nbands;
    const long nwg = (pairs + 7) / 8 * 8 * ceil_div(C / group_width, g.gchunk);
    LDN_REQUIRE(nwg < (1l << 31), "%s: too many workgroups (%ld)", name, nwg);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (gap)
        return group_width == 24 ? launch_grouped_chan<24, true>(g, lds, (unsigned)nwg, st)
             : group_width == 16 ? launch_grouped_chan<16, true>(g, lds, (unsigned)nwg, st) : launch_grouped_chan<8, true>(g, lds, (unsigned)nwg, st);
    return group_width == 24 ? launch_grouped_chan<24, false>(g, lds, (unsigned)nwg, st)
         : group_width == 16 ? launch_grouped_chan<16, false>(g, lds, (unsigned)nwg, st) : launch_grouped_chan<8, false>(g, lds, (unsigned)nwg, st);
}

extern "C" int ldn_grouped_chan_mfma_conv3x3_image(const float* a, int lda, int B, int Hi, int Wi, int stride, int Ho, int Wo,
                                                   const void* w_frag, int C, int group_width, const int32_t* ch_idx, const int32_t* ch_cnt,
                                                   const float* scale, const float* shift, int relu, float* out, int ldo, void* stream) {
    return grouped_chan_image("ldn_grouped_chan_mfma_conv3x3_image", a, lda, B, Hi, Wi, stride, Ho, Wo, w_frag, C, group_width, ch_idx, ch_cnt, scale, shift,
                              relu, out, ldo, nullptr, stream);
}

extern "C" int ldn_grouped_chan_mfma_conv3x3_image_gap(const float* a, int lda, int B, int Hi, int Wi, int stride, int Ho, int Wo,
                                                       const void* w_frag, int C, int group_width, const int32_t* ch_idx, const int32_t* ch_cnt,
                                                       const float* scale, const float* shift, int relu, float* out, int ldo, float* gap_partial,
                                                       void* stream) {
    LDN_REQUIRE(gap_partial, "ldn_grouped_chan_mfma_conv3x3_image_gap: null pointer");
    return grouped_chan_image("ldn_grouped_chan_mfma_conv3x3_image_gap", a, lda, B, Hi, Wi, stride, Ho, Wo, w_frag, C, group_width, ch_idx, ch_cnt, scale,
                              shift, relu, out, ldo, gap_partial, stream);
}
