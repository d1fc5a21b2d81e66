// ldn_wgrad_grouped_wide.hip -- the weight gradient of the grouped 3x3 over packed rows at group widths 56, 112 and 232, on the matrix cores
// (ldn_wgrad_grouped_wide_rows; include/ldn_hip.h):
//
//     dW[c, t, j] = sum_{r < count} dY[r, c] * A[nbr[r * 9 + t], (c / gw) * gw + j]         c < C, t < 9, j < gw,  gw = 56 | 112 | 232
//
// Per group a gw x 9 gw GEMM (56 x 504, 112 x 1008 or 232 x 2088) whose REDUCTION runs over the packed rows: the GEMM of ldn_wgrad.hip (k_wgrad) with
// cin = cout = gw, a column offset g * gw into dY and into A and a row offset g * gw into dW.  The groups ride in the grid: one launch covers
// every group (plus the reduce launch when the rows are split).  The staging scheme is k_wgrad's, restated here so that that translation
// unit's kernels stay what they are: a thread reads 8 consecutive rows of one column quad (8 x 16 B), transposes them in registers and writes
// each column's 8 values as ONE 16-byte unit of a column-major LDS image; bf16x3 splits there (a column record is [32 rows hi | 32 rows lo]
// bf16, the fp32 mode's 32 floats: 128 bytes, padded to 144 -- the pitch is k_wgrad's, chosen on paper; bank conflicts of this layout have NOT
// been measured with counters).  The nine taps' rows are gathered through nbr: column f = t * gw + j of the group's tile reads row
// nbr[r * 9 + t], channels g * gw + j; gw % 4 == 0, so a column quad never straddles a tap.  No [rows, 9 gw] matrix exists.
//
// Tiles: the dY tile is 64 (gw 56: 56 live) or 128 (gw 112: 112 live) columns, the A tile 128 columns of the flattened (tap, channel) axis --
// 4 column tiles over F = 504, 8 over F = 1008.  Width 232 has TWO dY tiles of 128 (n-tiles; the second with 104 live columns) and 17 column
// tiles over F = 2088 (the last with 40 live): the n-tile is one more index of the grid over the gw 112 kernel, a column offset into dY and a
// row offset into dW.  The group's dY tile is re-staged once per column tile (the form that was launched; a
// workgroup that stages dY once and walks several column tiles was NOT built or timed).
//
// Rows r >= count are never read (neither dY nor nbr); a table entry < 0 or >= a_valid is a zero row.  Determinism: the rows are split over
// `splits` workgroups per tile (a function of m_cap and the shapes only -- never of the device-side count, so the launch is graph-capturable);
// each writes its partial tile to the workspace and k_wgrad_gwide_reduce adds the partials of the splits that hold rows in ascending order.
// No floating-point atomics.
#include "ldn_common.h"

namespace ldn {

constexpr int WGW_KT = 128;        // tile columns over the flattened (tap, channel) axis of one group
constexpr int WGW_CHUNK = 32;      // rows per staged chunk = two K16 steps
constexpr int WGW_PITCH = 144;     // bytes per column record of the LDS image (128 + 16 pad)
// The row splits: k_wgrad's plan with four times its workgroup target and half its rows per split.  A workgroup keeps ONE chunk of loads in
// flight, so the loop is latency-bound and wants every workgroup slot of the machine filled (by the compiler's register counts in bf16x3 mode
// 4 workgroups per CU at gw 56 and 2 at gw 112: 1024 / 512 slots on 256 CUs), and the splits past the device-side count retire at once (layer
// skip keeps about half the rows).  Timed on the eight stride-1 conv b shapes of RegNetY-8GF / 16GF against k_wgrad's own 512 / 256 / 128
// (2.8x .. 1.7x shorter at gw 56, 1.7x shorter .. 1.07x longer at gw 112).
constexpr int WGW_MIN_SPLIT_ROWS = 128;
constexpr int WGW_TARGET_WGS = 2048;
constexpr int WGW_MAX_SPLITS = 256;

struct WgradGroupedWideArgs {
    const float* dy; const float* a; const int32_t* nbr; const int32_t* m_count;
    float* out; float* work;
    int lddy, lda, a_valid, m_cap, C, gw, splits, rps, ftn, ntn;
};

__device__ __forceinline__ int wgw_count(const WgradGroupedWideArgs& p) {
    int c = p.m_count ? *p.m_count : p.m_cap;
    return c < 0 ? 0 : (c > p.m_cap ? p.m_cap : c);
}

// grid = ((C / gw) * ntn * ftn, splits); 256 threads = 4 waves as 2 (n) x 2 (columns); wave tile = (NS x 32) x 64; NS = 1: gw 56, NS = 2: gw 112
// and (ntn = 2 n-tiles) gw 232
template <int NS, bool F32>
__global__ __launch_bounds__(256) void k_wgrad_gwide(const WgradGroupedWideArgs p) {
    constexpr int NT = 64 * NS;
    __shared__ __attribute__((aligned(16))) unsigned char s_img[(NT + WGW_KT) * WGW_PITCH];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l31 = lane & 31, h = lane >> 5;
    const int split = blockIdx.y;
    const int count = wgw_count(p);
    const int r_begin = split * p.rps;
    if (p.splits > 1 && r_begin >= count) return;       // (uniform) this split holds no rows: the reduce launch does not read its tile
    const int r_end = min(count, r_begin + p.rps);
    const int nchunks = r_begin < r_end ? (r_end - r_begin + WGW_CHUNK - 1) / WGW_CHUNK : 0;
    const int ft = blockIdx.x % p.ftn, gn = blockIdx.x / p.ftn;       // a group's column tiles are neighbours in the grid
    const int grp = gn / p.ntn, n0 = (gn - grp * p.ntn) * NT;         // the n-tile: dY columns / dW rows n0 .. n0 + NT - 1 of the group
    const int c0 = grp * p.gw, f0 = ft * WGW_KT;
    const int F = 9 * p.gw;

    // ---- staging role: wave `wave` owns 64 columns of the combined (dY | A) column space, lane = (row group g of 8 rows, column quad q)
    const int g = lane & 3, q = lane >> 2;
    const int cc = wave * 64 + 4 * q;                    // combined column
    const bool is_dy = cc < NT;
    const bool stager = cc < NT + WGW_KT;
    const int lcol = is_dy ? cc : cc - NT;               // column inside the operand's image
    unsigned char* s_dst = s_img + (is_dy ? 0 : NT * WGW_PITCH) + lcol * WGW_PITCH;
    const int gcol = is_dy ? n0 + lcol : f0 + lcol;      // column inside the group: n, or f = t * gw + j
    const bool col_ok = stager && (is_dy ? gcol < p.gw : gcol < F);
    const int tap = is_dy ? 0 : gcol / p.gw;
    const int kch = c0 + (is_dy ? gcol : gcol - tap * p.gw);     // channel of dY / of A: < C wherever col_ok

    f32x4 v[8];
    auto load_chunk = [&](int c) {
        const int rb = r_begin + c * WGW_CHUNK + 8 * g;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int r = rb + j;
            f32x4 x = {0.f, 0.f, 0.f, 0.f};
            if (col_ok && r < r_end) {
                if (is_dy) {
                    x = *reinterpret_cast<const f32x4*>(p.dy + (size_t)r * p.lddy + kch);
                } else {
                    const int idx = p.nbr[(size_t)r * 9 + tap];
                    LDN_DCHECK(idx >= -1, 621);
                    if (idx >= 0 && idx < p.a_valid) x = *reinterpret_cast<const f32x4*>(p.a + (size_t)idx * p.lda + kch);
                }
            }
            v[j] = x;
        }
    };
    auto store_chunk = [&]() {
        if (!stager) return;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            unsigned char* d = s_dst + i * WGW_PITCH;
            if constexpr (F32) {
                *reinterpret_cast<f32x4*>(d + g * 32) = f32x4{v[0][i], v[1][i], v[2][i], v[3][i]};
                *reinterpret_cast<f32x4*>(d + g * 32 + 16) = f32x4{v[4][i], v[5][i], v[6][i], v[7][i]};
            } else {
                bf16x8 hi, lo;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float x = v[j][i];
                    const __bf16 hb = (__bf16)x;
                    hi[j] = hb;
                    lo[j] = (__bf16)(x - (float)hb);
                }
                *reinterpret_cast<bf16x8*>(d + g * 16) = hi;
                *reinterpret_cast<bf16x8*>(d + 64 + g * 16) = lo;
            }
        }
    };

    // ---- compute role
    const int wn = wave & 1, wk = wave >> 1;
    const unsigned char* s_n = s_img + ((wn * NS) * 32 + l31) * WGW_PITCH;
    const unsigned char* s_k = s_img + NT * WGW_PITCH + ((wk * 2) * 32 + l31) * WGW_PITCH;
    f32x16 acc[NS][2];
#pragma unroll
    for (int a = 0; a < NS; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

    if (nchunks > 0) load_chunk(0);
    for (int c = 0; c < nchunks; ++c) {
        store_chunk();
        __syncthreads();
        if (c + 1 < nchunks) load_chunk(c + 1);           // in flight behind this chunk's MFMAs
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            // the lane's 8 rows of the K16 step: rows 16 s + 8 h .. + 7 of its column (both operands use the same row -> slot map)
            const int off = F32 ? 64 * s + 32 * h : 32 * s + 16 * h;
            bf16x8 n_h[NS], n_l[NS], k_h[2], k_l[2];       // F32: the raw floats of slots 0-3 / 4-7
            const int second = F32 ? 16 : 64;
#pragma unroll
            for (int a = 0; a < NS; ++a) {
                n_h[a] = *reinterpret_cast<const bf16x8*>(s_n + a * 32 * WGW_PITCH + off);
                n_l[a] = *reinterpret_cast<const bf16x8*>(s_n + a * 32 * WGW_PITCH + off + second);
            }
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                k_h[b] = *reinterpret_cast<const bf16x8*>(s_k + b * 32 * WGW_PITCH + off);
                k_l[b] = *reinterpret_cast<const bf16x8*>(s_k + b * 32 * WGW_PITCH + off + second);
            }
#pragma unroll
            for (int a = 0; a < NS; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b) {
                    if constexpr (F32) {
                        const f32x4 a0 = __builtin_bit_cast(f32x4, n_h[a]), a1 = __builtin_bit_cast(f32x4, n_l[a]);
                        const f32x4 b0 = __builtin_bit_cast(f32x4, k_h[b]), b1 = __builtin_bit_cast(f32x4, k_l[b]);
#pragma unroll
                        for (int i = 0; i < 4; ++i) acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[i], b0[i], acc[a][b], 0, 0, 0);
#pragma unroll
                        for (int i = 0; i < 4; ++i) acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[i], b1[i], acc[a][b], 0, 0, 0);
                    } else {      // the order of k_wgrad (lo.hi, hi.lo, hi.hi)
                        acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(n_l[a], k_h[b], acc[a][b], 0, 0, 0);
                        acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(n_h[a], k_l[b], acc[a][b], 0, 0, 0);
                        acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(n_h[a], k_h[b], acc[a][b], 0, 0, 0);
                    }
                }
        }
        __syncthreads();
    }

    // ---- epilogue: accumulator register r = row (r & 3) + 8 (r >> 2) + 4 h of the subtile, lane & 31 = its column; dW[c0 + n][f]
    float* dst = (p.splits > 1 ? p.work + (size_t)split * p.C * F : p.out) + (size_t)c0 * F;
#pragma unroll
    for (int a = 0; a < NS; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int f = f0 + (wk * 2 + b) * 32 + l31;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int n = n0 + (wn * NS + a) * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                if (n < p.gw && f < F) dst[(size_t)n * F + f] = acc[a][b][r];
            }
        }
}

// out = the partial tiles of the splits that hold rows, added in ascending order (count == 0: zeros)
__global__ __launch_bounds__(256) void k_wgrad_gwide_reduce(const WgradGroupedWideArgs p, int quads) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= quads) return;
    const int count = wgw_count(p);
    const int live = min(p.splits, (count + p.rps - 1) / p.rps);
    const size_t stride = (size_t)p.C * 9 * p.gw;
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < live; ++k) s += *reinterpret_cast<const f32x4*>(p.work + k * stride + (size_t)i * 4);
    *reinterpret_cast<f32x4*>(p.out + (size_t)i * 4) = s;
}

LDN_DEFINE_TU_VIOLATIONS(tu_violations_wgrad_grouped_wide)

static bool wgw_ok(int C, int gw) {
    return (gw == 56 || gw == 112 || gw == 232) && C > 0 && C % gw == 0 && C <= 4096;
}

// the launch plan: a function of m_cap and the shapes ONLY
static void wgw_plan(int m_cap, int C, int gw, int* ftn, int* ntn, int* splits, int* rps) {
    *ftn = ceil_div(9 * gw, WGW_KT);
    *ntn = ceil_div(gw, 128);                             // dY tiles of the group: 1 at gw 56 / 112, 2 at gw 232
    int s = ceil_div(WGW_TARGET_WGS, (C / gw) * *ntn * *ftn);
    const int most = m_cap / WGW_MIN_SPLIT_ROWS;
    if (s > most) s = most;
    if (s > WGW_MAX_SPLITS) s = WGW_MAX_SPLITS;
    if (s < 1) s = 1;
    *rps = round_up(ceil_div(m_cap > 0 ? m_cap : 1, s), WGW_CHUNK);
    *splits = ceil_div(m_cap > 0 ? m_cap : 1, *rps);      // (no split without rows)
}

}  // namespace ldn

using namespace ldn;

extern "C" int ldn_wgrad_grouped_wide_rows_ok(int C, int gw) { return wgw_ok(C, gw) ? 1 : 0; }

extern "C" size_t ldn_wgrad_grouped_wide_rows_workspace_bytes(int m_cap, int C, int gw) {
    if (!wgw_ok(C, gw) || m_cap < 0) return 0;
    int ftn, ntn, splits, rps;
    wgw_plan(m_cap, C, gw, &ftn, &ntn, &splits, &rps);
    return splits > 1 ? (size_t)splits * C * 9 * gw * sizeof(float) : 0;
}

extern "C" int ldn_wgrad_grouped_wide_rows(const float* dy, int lddy, const float* a, int lda, int a_valid, const int32_t* nbr,
                                           const int32_t* m_count, int m_cap, int C, int gw, float* dw, float* work, int math_mode,
                                           void* stream) {
    LDN_REQUIRE(dy && a && nbr && dw, "ldn_wgrad_grouped_wide_rows: null pointer");
    LDN_REQUIRE(math_mode >= -1 && math_mode <= 1, "ldn_wgrad_grouped_wide_rows: math_mode must be LDN_MATH_DEFAULT (-1), LDN_MATH_FP32 (0) or LDN_MATH_BF16X3 (1), got %d", math_mode);
    const int math = math_mode < 0 ? ldn_default_math_mode() : math_mode;
    LDN_REQUIRE(wgw_ok(C, gw), "ldn_wgrad_grouped_wide_rows: unsupported shape C %d group width %d (group width 56 | 112 | 232, C %% group width == 0, C <= 4096)", C, gw);
    LDN_REQUIRE(m_cap >= 0 && a_valid >= 0, "ldn_wgrad_grouped_wide_rows: negative row count");
    LDN_REQUIRE(lddy >= C && lda >= C && lddy % 4 == 0 && lda % 4 == 0, "ldn_wgrad_grouped_wide_rows: lddy >= C, lda >= C, both multiples of 4 (got %d, %d)", lddy, lda);
    LDN_REQUIRE((uintptr_t)dy % 16 == 0 && (uintptr_t)a % 16 == 0 && (uintptr_t)dw % 16 == 0 && (uintptr_t)work % 16 == 0,
                "ldn_wgrad_grouped_wide_rows: dy / a / dw / work must be 16-byte aligned");
    WgradGroupedWideArgs p;
    p.dy = dy; p.a = a; p.nbr = nbr; p.m_count = m_count; p.out = dw; p.work = work;
    p.lddy = lddy; p.lda = lda; p.a_valid = a_valid; p.m_cap = m_cap; p.C = C; p.gw = gw;
    wgw_plan(m_cap, C, gw, &p.ftn, &p.ntn, &p.splits, &p.rps);
    LDN_REQUIRE(p.splits == 1 || work, "ldn_wgrad_grouped_wide_rows: this shape splits its rows %d ways and needs the workspace (ldn_wgrad_grouped_wide_rows_workspace_bytes)", p.splits);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)((C / gw) * p.ntn * p.ftn), (unsigned)p.splits);
    if (math == LDN_MATH_FP32) {
        if (gw == 56) k_wgrad_gwide<1, true><<<grid, 256, 0, st>>>(p); else k_wgrad_gwide<2, true><<<grid, 256, 0, st>>>(p);
    } else {
        if (gw == 56) k_wgrad_gwide<1, false><<<grid, 256, 0, st>>>(p); else k_wgrad_gwide<2, false><<<grid, 256, 0, st>>>(p);
    }
    LDN_CHECK_LAUNCH("k_wgrad_gwide");
    if (p.splits > 1) {
        const int quads = C * 9 * gw / 4;
        k_wgrad_gwide_reduce<<<ceil_div(quads, 256), 256, 0, st>>>(p, quads);
        LDN_CHECK_LAUNCH("k_wgrad_gwide_reduce");
    }
    return LDN_OK;
}
