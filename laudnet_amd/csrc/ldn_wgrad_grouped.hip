// ldn_wgrad_grouped.hip -- the weight gradient of the grouped 3x3 over packed rows (ldn_wgrad_grouped_rows; include/ldn_hip.h):
//
//     dW[c, t, j] = sum_{r < count} dY[r, c] * A[nbr[r * 9 + t], (c / gw) * gw + j]         c < C, t < 9, j < gw
//
// Per group a gw x 9 gw tile reduced over the rows, in the weight layout of ldn_grouped_conv3x3_rows ([C][9][gw]).  Plain fp32 on the
// VALU in BOTH arithmetic modes (v_fma_f32, fp32 accumulation; there is no three-product form): per group the tile is at most 24 x 216 and
// every output element needs ten gathered floats per row, so on paper the gathers and not the arithmetic bound it (not measured).
//
// One workgroup = one group x one row split.  A chunk of 32 rows is staged in the LDS -- the group's gw columns of the dY row and of the nine
// neighbour rows, each as 16-byte loads; a table entry < 0 or >= a_valid stores a zero row -- the next chunk's loads are in flight behind the
// current chunk's arithmetic.  A thread owns 4 x 4 blocks of the tile (4 output channels x 4 input channels of one tap: two 16-byte LDS reads
// per 16 FMAs); where the tile has fewer blocks than the workgroup has threads (gw = 8: 36) the chunk's rows are dealt to S thread slices
// whose partial blocks are added in ascending slice order at the end.
//
// Rows r >= count are never read (neither dY nor nbr).  Determinism: the rows are split over `splits` workgroups per group (a function of
// m_cap and the shapes only -- never of the device-side count, so the launch is graph-capturable); each writes its partial [C][9][gw] to the
// workspace and k_wgrad_grouped_reduce adds the partials of the splits that hold rows in ascending order.  No floating-point atomics.
#include "ldn_common.h"

namespace ldn {

constexpr int WGG_CHUNK = 32;            // rows per staged chunk
constexpr int WGG_THREADS = 256;
constexpr int WGG_MIN_SPLIT_ROWS = 256;
constexpr int WGG_TARGET_WGS = 512;
constexpr int WGG_MAX_SPLITS = 128;

struct WgradGroupedArgs {
    const float* dy; const float* a; const int32_t* nbr; const int32_t* m_count;
    float* out; float* work;
    int lddy, lda, a_valid, m_cap, C, splits, rps;
};

__device__ __forceinline__ int wgg_count(const WgradGroupedArgs& p) {
    int c = p.m_count ? *p.m_count : p.m_cap;
    return c < 0 ? 0 : (c > p.m_cap ? p.m_cap : c);
}

// grid = (C / GW, splits); 256 threads
template <int GW>
__global__ __launch_bounds__(WGG_THREADS) void k_wgrad_grouped(const WgradGroupedArgs p) {
    constexpr int Q = GW / 4;                                        // channel quads of a group
    constexpr int NB = 9 * Q * Q;                                    // 4 x 4 blocks of the tile: (tap, out quad, in quad)
    constexpr int BPT = (NB + WGG_THREADS - 1) / WGG_THREADS;        // blocks per thread (gw 24: 2)
    constexpr int S = NB < WGG_THREADS ? WGG_THREADS / NB : 1;       // row slices (gw 8: 7)
    constexpr int ROWQ = 10 * Q;                                     // quads of a staged row: [dY | tap 0 .. tap 8]
    constexpr int NLD = (WGG_CHUNK * ROWQ + WGG_THREADS - 1) / WGG_THREADS;
    __shared__ __attribute__((aligned(16))) float s_row[WGG_CHUNK * ROWQ * 4];
    __shared__ __attribute__((aligned(16))) float s_red[S > 1 ? S * NB * 16 : 4];
    const int tid = threadIdx.x;
    const int grp = blockIdx.x, split = blockIdx.y;
    const int count = wgg_count(p);
    const int r_begin = split * p.rps;
    if (p.splits > 1 && r_begin >= count) return;       // (uniform) this split holds no rows: the reduce launch does not read its partial
    const int r_end = min(count, r_begin + p.rps);
    const int nchunks = r_begin < r_end ? (r_end - r_begin + WGG_CHUNK - 1) / WGG_CHUNK : 0;
    const int c0 = grp * GW;

    f32x4 v[NLD];
    auto load_chunk = [&](int c) {
        const int rb = r_begin + c * WGG_CHUNK;
#pragma unroll
        for (int k = 0; k < NLD; ++k) {
            const int i = tid + k * WGG_THREADS;                     // (row of the chunk, slot 0 = dY / 1 + tap, quad)
            const int q = i % Q, slot = (i / Q) % 10, r = rb + i / ROWQ;
            f32x4 x = {0.f, 0.f, 0.f, 0.f};
            if (i < WGG_CHUNK * ROWQ && r < r_end) {
                if (slot == 0) {
                    x = *reinterpret_cast<const f32x4*>(p.dy + (size_t)r * p.lddy + c0 + 4 * q);
                } else {
                    const int idx = p.nbr[(size_t)r * 9 + (slot - 1)];
                    LDN_DCHECK(idx >= -1, 611);
                    if (idx >= 0 && idx < p.a_valid) x = *reinterpret_cast<const f32x4*>(p.a + (size_t)idx * p.lda + c0 + 4 * q);
                }
            }
            v[k] = x;
        }
    };
    auto store_chunk = [&]() {
#pragma unroll
        for (int k = 0; k < NLD; ++k) {
            const int i = tid + k * WGG_THREADS;
            if (i < WGG_CHUNK * ROWQ) *reinterpret_cast<f32x4*>(s_row + 4 * i) = v[k];
        }
    };

    // ---- compute role: block b = (tap, out quad cq, in quad jq); slice = which rows of a chunk
    const int slice = BPT == 1 ? tid / NB : 0;
    const bool worker = BPT > 1 || slice < S;
    int cq[BPT], fq[BPT];                                           // fq = quad offset of (tap, jq) inside the staged row
    bool live[BPT];
#pragma unroll
    for (int u = 0; u < BPT; ++u) {
        const int b = BPT == 1 ? tid % NB : tid + u * WGG_THREADS;
        live[u] = worker && b < NB;
        const int bb = b < NB ? b : 0;
        cq[u] = (bb / Q) % Q;
        fq[u] = Q + (bb / (Q * Q)) * Q + bb % Q;
    }
    f32x4 acc[BPT][4];
#pragma unroll
    for (int u = 0; u < BPT; ++u)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[u][i] = f32x4{0.f, 0.f, 0.f, 0.f};

    if (nchunks > 0) load_chunk(0);
    for (int c = 0; c < nchunks; ++c) {
        store_chunk();
        __syncthreads();
        if (c + 1 < nchunks) load_chunk(c + 1);           // in flight behind this chunk's arithmetic
        const int nr = min(WGG_CHUNK, r_end - (r_begin + c * WGG_CHUNK));
#pragma unroll
        for (int u = 0; u < BPT; ++u) {
            if (!live[u]) continue;
            for (int r = slice; r < nr; r += S) {
                const f32x4 d = *reinterpret_cast<const f32x4*>(s_row + 4 * (r * ROWQ + cq[u]));
                const f32x4 x = *reinterpret_cast<const f32x4*>(s_row + 4 * (r * ROWQ + fq[u]));
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[u][i] += d[i] * x;
            }
        }
        __syncthreads();
    }

    // ---- the slices' partial blocks, added in ascending slice order by slice 0
    if constexpr (S > 1) {
        if (live[0]) {
#pragma unroll
            for (int i = 0; i < 4; ++i) *reinterpret_cast<f32x4*>(s_red + ((slice * NB + tid % NB) * 4 + i) * 4) = acc[0][i];
        }
        __syncthreads();
        if (live[0] && slice == 0) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                f32x4 s = acc[0][i];
                for (int k = 1; k < S; ++k) s += *reinterpret_cast<const f32x4*>(s_red + ((k * NB + tid) * 4 + i) * 4);
                acc[0][i] = s;
            }
        }
    }

    // ---- epilogue: dW[c0 + 4 cq + i][tap][4 jq .. + 3]
    float* dst = p.splits > 1 ? p.work + (size_t)split * p.C * 9 * GW : p.out;
#pragma unroll
    for (int u = 0; u < BPT; ++u) {
        if (!live[u] || slice != 0) continue;
        const int f = fq[u] - Q;                                     // tap * Q + jq
#pragma unroll
        for (int i = 0; i < 4; ++i)
            *reinterpret_cast<f32x4*>(dst + ((size_t)(c0 + 4 * cq[u] + i) * 9 * GW + 4 * f)) = acc[u][i];
    }
}

// out = the partials of the splits that hold rows, added in ascending order (count == 0: zeros)
__global__ __launch_bounds__(256) void k_wgrad_grouped_reduce(const WgradGroupedArgs p, int gw, int quads) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= quads) return;
    const int count = wgg_count(p);
    const int live = min(p.splits, (count + p.rps - 1) / p.rps);
    const size_t stride = (size_t)p.C * 9 * gw;
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < live; ++k) s += *reinterpret_cast<const f32x4*>(p.work + k * stride + (size_t)i * 4);
    *reinterpret_cast<f32x4*>(p.out + (size_t)i * 4) = s;
}

LDN_DEFINE_TU_VIOLATIONS(tu_violations_wgrad_grouped)

static bool wgg_ok(int C, int gw) {
    return (gw == 8 || gw == 16 || gw == 24) && C > 0 && C % gw == 0 && C <= 2048;
}

// the launch plan: a function of m_cap and the shapes ONLY
static void wgg_plan(int m_cap, int C, int gw, int* splits, int* rps) {
    int s = ceil_div(WGG_TARGET_WGS, C / gw);
    const int most = m_cap / WGG_MIN_SPLIT_ROWS;
    if (s > most) s = most;
    if (s > WGG_MAX_SPLITS) s = WGG_MAX_SPLITS;
    if (s < 1) s = 1;
    *rps = round_up(ceil_div(m_cap > 0 ? m_cap : 1, s), WGG_CHUNK);
    *splits = ceil_div(m_cap > 0 ? m_cap : 1, *rps);      // (no split without rows)
}

}  // namespace ldn

using namespace ldn;

extern "C" int ldn_wgrad_grouped_rows_ok(int C, int gw) { return wgg_ok(C, gw) ? 1 : 0; }

extern "C" size_t ldn_wgrad_grouped_rows_workspace_bytes(int m_cap, int C, int gw) {
    if (!wgg_ok(C, gw) || m_cap < 0) return 0;
    int splits, rps;
    wgg_plan(m_cap, C, gw, &splits, &rps);
    return splits > 1 ? (size_t)splits * C * 9 * gw * sizeof(float) : 0;
}

extern "C" int ldn_wgrad_grouped_rows(const float* dy, int lddy, const float* a, int lda, int a_valid, const int32_t* nbr,
                                      const int32_t* m_count, int m_cap, int C, int gw, float* dw, float* work, int math_mode,
                                      void* stream) {
    LDN_REQUIRE(dy && a && nbr && dw, "ldn_wgrad_grouped_rows: null pointer");
    LDN_REQUIRE(math_mode >= -1 && math_mode <= 1, "ldn_wgrad_grouped_rows: math_mode must be LDN_MATH_DEFAULT (-1), LDN_MATH_FP32 (0) or LDN_MATH_BF16X3 (1), got %d", math_mode);
    LDN_REQUIRE(wgg_ok(C, gw), "ldn_wgrad_grouped_rows: unsupported shape C %d group width %d (group width 8 | 16 | 24, C %% group width == 0, C <= 2048)", C, gw);
    LDN_REQUIRE(m_cap >= 0 && a_valid >= 0, "ldn_wgrad_grouped_rows: negative row count");
    LDN_REQUIRE(lddy >= C && lda >= C && lddy % 4 == 0 && lda % 4 == 0, "ldn_wgrad_grouped_rows: lddy >= C, lda >= C, both multiples of 4 (got %d, %d)", lddy, lda);
    LDN_REQUIRE((uintptr_t)dy % 16 == 0 && (uintptr_t)a % 16 == 0 && (uintptr_t)dw % 16 == 0 && (uintptr_t)work % 16 == 0,
                "ldn_wgrad_grouped_rows: dy / a / dw / work must be 16-byte aligned");
    WgradGroupedArgs p;
    p.dy = dy; p.a = a; p.nbr = nbr; p.m_count = m_count; p.out = dw; p.work = work;
    p.lddy = lddy; p.lda = lda; p.a_valid = a_valid; p.m_cap = m_cap; p.C = C;
    wgg_plan(m_cap, C, gw, &p.splits, &p.rps);
    LDN_REQUIRE(p.splits == 1 || work, "ldn_wgrad_grouped_rows: this shape splits its rows %d ways and needs the workspace (ldn_wgrad_grouped_rows_workspace_bytes)", p.splits);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)(C / gw), (unsigned)p.splits);
    switch (gw) {      // (both arithmetic modes: the fp32 form)
        case 8: k_wgrad_grouped<8><<<grid, WGG_THREADS, 0, st>>>(p); break;
        case 16: k_wgrad_grouped<16><<<grid, WGG_THREADS, 0, st>>>(p); break;
        default: k_wgrad_grouped<24><<<grid, WGG_THREADS, 0, st>>>(p); break;
    }
    LDN_CHECK_LAUNCH("k_wgrad_grouped");
    if (p.splits > 1) {
        const int quads = C * 9 * gw / 4;
        k_wgrad_grouped_reduce<<<ceil_div(quads, 256), 256, 0, st>>>(p, gw, quads);
        LDN_CHECK_LAUNCH("k_wgrad_grouped_reduce");
    }
    return LDN_OK;
}
