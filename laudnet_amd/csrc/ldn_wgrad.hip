// ldn_wgrad.hip -- the weight gradient of a packed-row convolution (ldn_wgrad_rows; include/ldn_hip.h):
//
//     dW[n, t, k] = sum_{r < count} dY[r, n] * A[src(r, t), k]         src(r, t) = a_rows ? a_rows[r * taps + t] : r
//
// a GEMM whose REDUCTION runs over the packed rows: M = cout (n), N = taps * cin (the flattened (t, k) axis = the weight row of
// ldn_conv_rows), K = rows.  Both operands are row-major along the reduction axis, so a tile is transposed on its way into MFMA operand
// order: a thread reads 8 consecutive rows of one column quad from memory (8 x 16 B, coalesced along the row), and writes each of its four
// columns' 8 values as ONE 16-byte unit of a column-major LDS image -- the transposition happens in registers.  bf16x3 splits there too
// (once per element and workgroup, not once per fragment): a column record of the image is [32 rows hi | 32 rows lo] bf16, the fp32 mode's
// is 32 floats -- 128 bytes either way, padded to 144 (36 banks, chosen on paper so that consecutive columns' 16-byte units start 4 banks
// apart modulo 64; bank conflicts of this layout have NOT been measured with counters).  A fragment is then one ds_read_b128 per operand half.
//
// The nine taps' rows are gathered straight from A through a_rows: column f = t * cin + k of the tile reads row a_rows[r * 9 + t].  No
// [rows, 9 K] matrix exists.  Rows r >= count are never read (neither dY nor a_rows); an index < 0 or >= a_valid is a zero row.
//
// Determinism: the rows are split over `splits` workgroups per tile (a function of m_cap and the shapes only -- never of the device-side
// count, so the launch is graph-capturable); each writes its partial tile to the workspace and k_wgrad_reduce adds the partials of the
// splits that hold rows in ascending order.  No floating-point atomics.
#include "ldn_common.h"

namespace ldn {

constexpr int WG_KT = 128;        // tile columns over the flattened (tap, channel) axis
constexpr int WG_CHUNK = 32;      // rows per staged chunk = two K16 steps
constexpr int WG_PITCH = 144;     // bytes per column record of the LDS image (128 + 16 pad)
constexpr int WG_MIN_SPLIT_ROWS = 256;
constexpr int WG_TARGET_WGS = 512;
constexpr int WG_MAX_SPLITS = 128;

struct WgradArgs {
    const float* dy; const float* a; const int32_t* a_rows; const int32_t* m_count;
    float* out; float* work;
    int lddy, lda, a_valid, taps, m_cap, cin, cout, splits, rps, ntn;
};

__device__ __forceinline__ int wgrad_count(const WgradArgs& p) {
    int c = p.m_count ? *p.m_count : p.m_cap;
    return c < 0 ? 0 : (c > p.m_cap ? p.m_cap : c);
}

// grid = (ntn * ftn, splits); 256 threads = 4 waves as 2 (n) x 2 (columns); wave tile = (NS x 32) x 64
template <int NS, bool F32>
__global__ __launch_bounds__(256) void k_wgrad(const WgradArgs p) {
    constexpr int NT = 64 * NS;
    __shared__ __attribute__((aligned(16))) unsigned char s_img[(NT + WG_KT) * WG_PITCH];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l31 = lane & 31, h = lane >> 5;
    const int split = blockIdx.y;
    const int count = wgrad_count(p);
    const int r_begin = split * p.rps;
    if (p.splits > 1 && r_begin >= count) return;       // (uniform) this split holds no rows: k_wgrad_reduce does not read its tile
    const int r_end = min(count, r_begin + p.rps);
    const int nchunks = r_begin < r_end ? (r_end - r_begin + WG_CHUNK - 1) / WG_CHUNK : 0;
    const int nt = blockIdx.x % p.ntn, ft = blockIdx.x / p.ntn;
    const int n0 = nt * NT, f0 = ft * WG_KT;
    const int F = p.taps * p.cin;

    // ---- staging role: wave `wave` owns 64 columns of the combined (dY | A) column space, lane = (row group g of 8 rows, column quad q)
    const int g = lane & 3, q = lane >> 2;
    const int cc = wave * 64 + 4 * q;                    // combined column
    const bool is_dy = cc < NT;
    const bool stager = cc < NT + WG_KT;
    const int lcol = is_dy ? cc : cc - NT;               // column inside the operand's image
    unsigned char* s_dst = s_img + (is_dy ? 0 : NT * WG_PITCH) + lcol * WG_PITCH;
    const int gcol = is_dy ? n0 + lcol : f0 + lcol;      // global column: n, or f = t * cin + k
    const bool col_ok = stager && (is_dy ? gcol < p.cout : gcol < F);
    const int tap = is_dy ? 0 : gcol / p.cin;
    const int kch = is_dy ? gcol : gcol - tap * p.cin;

    f32x4 v[8];
    auto load_chunk = [&](int c) {
        const int rb = r_begin + c * WG_CHUNK + 8 * g;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int r = rb + j;
            f32x4 x = {0.f, 0.f, 0.f, 0.f};
            if (col_ok && r < r_end) {
                if (is_dy) {
                    x = *reinterpret_cast<const f32x4*>(p.dy + (size_t)r * p.lddy + kch);
                } else {
                    const int idx = p.a_rows ? p.a_rows[(size_t)r * p.taps + tap] : r;
                    LDN_DCHECK(idx >= -1, 601);
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
            unsigned char* d = s_dst + i * WG_PITCH;
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
    const unsigned char* s_n = s_img + ((wn * NS) * 32 + l31) * WG_PITCH;
    const unsigned char* s_k = s_img + NT * WG_PITCH + ((wk * 2) * 32 + l31) * WG_PITCH;
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
                n_h[a] = *reinterpret_cast<const bf16x8*>(s_n + a * 32 * WG_PITCH + off);
                n_l[a] = *reinterpret_cast<const bf16x8*>(s_n + a * 32 * WG_PITCH + off + second);
            }
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                k_h[b] = *reinterpret_cast<const bf16x8*>(s_k + b * 32 * WG_PITCH + off);
                k_l[b] = *reinterpret_cast<const bf16x8*>(s_k + b * 32 * WG_PITCH + off + second);
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
                    } else {      // the order of k_dense (lo.hi, hi.lo, hi.hi)
                        acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(n_l[a], k_h[b], acc[a][b], 0, 0, 0);
                        acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(n_h[a], k_l[b], acc[a][b], 0, 0, 0);
                        acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(n_h[a], k_h[b], acc[a][b], 0, 0, 0);
                    }
                }
        }
        __syncthreads();
    }

    // ---- epilogue: accumulator register r = row (r & 3) + 8 (r >> 2) + 4 h of the subtile, lane & 31 = its column
    float* dst = p.splits > 1 ? p.work + (size_t)split * p.cout * F : p.out;
#pragma unroll
    for (int a = 0; a < NS; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int f = f0 + (wk * 2 + b) * 32 + l31;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int n = n0 + (wn * NS + a) * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                if (n < p.cout && f < F) dst[(size_t)n * F + f] = acc[a][b][r];
            }
        }
}

// out = the partial tiles of the splits that hold rows, added in ascending order (count == 0: zeros)
__global__ __launch_bounds__(256) void k_wgrad_reduce(const WgradArgs p, int quads) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= quads) return;
    const int count = wgrad_count(p);
    const int live = min(p.splits, (count + p.rps - 1) / p.rps);
    const size_t stride = (size_t)p.cout * p.taps * p.cin;
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < live; ++k) s += *reinterpret_cast<const f32x4*>(p.work + k * stride + (size_t)i * 4);
    *reinterpret_cast<f32x4*>(p.out + (size_t)i * 4) = s;
}

LDN_DEFINE_TU_VIOLATIONS(tu_violations_wgrad)

static bool wgrad_ok(int cin, int cout, int taps) {
    if (taps != 1 && taps != 9) return false;
    const int lim = taps == 1 ? 2048 : 512;
    return cin > 0 && cout > 0 && cin % 8 == 0 && cout % 4 == 0 && cin <= lim && cout <= lim;
}

// the launch plan: a function of m_cap and the shapes ONLY
static void wgrad_plan(int m_cap, int cin, int cout, int taps, int* ns, int* ntn, int* ftn, int* splits, int* rps) {
    *ns = cout <= 64 ? 1 : 2;
    *ntn = ceil_div(cout, 64 * *ns);
    *ftn = ceil_div(taps * cin, WG_KT);
    int s = ceil_div(WG_TARGET_WGS, *ntn * *ftn);
    const int most = m_cap / WG_MIN_SPLIT_ROWS;
    if (s > most) s = most;
    if (s > WG_MAX_SPLITS) s = WG_MAX_SPLITS;
    if (s < 1) s = 1;
    *rps = round_up(ceil_div(m_cap > 0 ? m_cap : 1, s), WG_CHUNK);
    *splits = ceil_div(m_cap > 0 ? m_cap : 1, *rps);      // (no split without rows)
}

}  // namespace ldn

using namespace ldn;

extern "C" int ldn_wgrad_rows_ok(int cin, int cout, int taps) { return wgrad_ok(cin, cout, taps) ? 1 : 0; }

extern "C" size_t ldn_wgrad_rows_workspace_bytes(int m_cap, int cin, int cout, int taps) {
    if (!wgrad_ok(cin, cout, taps) || m_cap < 0) return 0;
    int ns, ntn, ftn, splits, rps;
    wgrad_plan(m_cap, cin, cout, taps, &ns, &ntn, &ftn, &splits, &rps);
    return splits > 1 ? (size_t)splits * cout * taps * cin * sizeof(float) : 0;
}

extern "C" int ldn_wgrad_rows(const float* dy, int lddy, const float* a, int lda, int a_valid, const int32_t* a_rows, int taps,
                              const int32_t* m_count, int m_cap, int cin, int cout, float* dw, float* work, int math_mode,
                              void* stream) {
    LDN_REQUIRE(dy && a && dw, "ldn_wgrad_rows: null pointer");
    LDN_REQUIRE(math_mode >= -1 && math_mode <= 1, "ldn_wgrad_rows: math_mode must be LDN_MATH_DEFAULT (-1), LDN_MATH_FP32 (0) or LDN_MATH_BF16X3 (1), got %d", math_mode);
    const int math = math_mode < 0 ? ldn_default_math_mode() : math_mode;
    LDN_REQUIRE(wgrad_ok(cin, cout, taps), "ldn_wgrad_rows: unsupported shape cin %d cout %d taps %d (taps 1 | 9, cin %% 8 == 0, cout %% 4 == 0, "
                "both <= 2048 for taps 1 / <= 512 for taps 9)", cin, cout, taps);
    LDN_REQUIRE(m_cap >= 0 && a_valid >= 0, "ldn_wgrad_rows: negative row count");
    LDN_REQUIRE(a_rows || m_cap <= a_valid, "ldn_wgrad_rows: without a_rows, row r of dY pairs with row r of A: m_cap %d exceeds a_valid %d", m_cap, a_valid);
    LDN_REQUIRE(lddy >= cout && lda >= cin && lddy % 4 == 0 && lda % 4 == 0, "ldn_wgrad_rows: lddy >= cout, lda >= cin, both multiples of 4 (got %d, %d)", lddy, lda);
    LDN_REQUIRE((uintptr_t)dy % 16 == 0 && (uintptr_t)a % 16 == 0 && (uintptr_t)dw % 16 == 0 && (uintptr_t)work % 16 == 0,
                "ldn_wgrad_rows: dy / a / dw / work must be 16-byte aligned");
    WgradArgs p;
    p.dy = dy; p.a = a; p.a_rows = a_rows; p.m_count = m_count; p.out = dw; p.work = work;
    p.lddy = lddy; p.lda = lda; p.a_valid = a_valid; p.taps = taps; p.m_cap = m_cap; p.cin = cin; p.cout = cout;
    int ns, ftn;
    wgrad_plan(m_cap, cin, cout, taps, &ns, &p.ntn, &ftn, &p.splits, &p.rps);
    LDN_REQUIRE(p.splits == 1 || work, "ldn_wgrad_rows: this shape splits its rows %d ways and needs the workspace (ldn_wgrad_rows_workspace_bytes)", p.splits);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)(p.ntn * ftn), (unsigned)p.splits);
    if (math == LDN_MATH_FP32) {
        if (ns == 1) k_wgrad<1, true><<<grid, 256, 0, st>>>(p); else k_wgrad<2, true><<<grid, 256, 0, st>>>(p);
    } else {
        if (ns == 1) k_wgrad<1, false><<<grid, 256, 0, st>>>(p); else k_wgrad<2, false><<<grid, 256, 0, st>>>(p);
    }
    LDN_CHECK_LAUNCH("k_wgrad");
    if (p.splits > 1) {
        const int quads = cout * taps * cin / 4;
        k_wgrad_reduce<<<ceil_div(quads, 256), 256, 0, st>>>(p, quads);
        LDN_CHECK_LAUNCH("k_wgrad_reduce");
    }
    return LDN_OK;
}
