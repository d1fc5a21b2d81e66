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
// GwCfg::PF steps ahead of the MFMAs that consume them, across the group boundary.
#include "ldn_common.h"

namespace ldn {

template <int GW> struct GwCfg;
template <> struct GwCfg<8> {
    static constexpr int STEPS = 3, TILE = 16, MAXG = 24, PF = 3;
    typedef f32x4 acc_t;
};
template <> struct GwCfg<24> {
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
    typedef GwCfg<GW> cfg;
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
    typedef GwCfg<GW> cfg;
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

}  // namespace ldn

using namespace ldn;

extern "C" int ldn_grouped_mfma_ok(int C, int group_width) {
    return (group_width == 8 || group_width == 24) && C > 0 && C % group_width == 0 ? 1 : 0;
}

extern "C" size_t ldn_grouped_mfma_weight_bytes(int C, int group_width) {
    if (!ldn_grouped_mfma_ok(C, group_width)) return 0;
    return (size_t)(C / group_width) * (group_width == 24 ? GwCfg<24>::STEPS : GwCfg<8>::STEPS) * 64 * 32;
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
