// ldn_train_rows.hip -- the elementwise backward chain of training on packed rows (ldn_rows_chanmask, ldn_rows_act_bwd, ldn_rows_postmask_bwd,
// ldn_rows_img_dot; include/ldn_hip.h), the reducer launch they share with ldn_train_bn.hip, and the LayerNorm backward on listed rows
// (ldn_rows_ln_bwd, further down with its own notes).
//
// The first four are bandwidth-bound row kernels over [m_cap, C] fp32 matrices; all but ldn_rows_chanmask (one thread per row and quad, a binary
// search for the row's image) are the walk of ldn_rows_plan.h.  The image of a packed row comes from the per-image row prefix ([B + 1]: image b
// owns the rows from prefix[b] up to the next image's) inside the kernel: there is no [m_cap] image-id tensor and no host read.
//
// ldn_rows_act_bwd, per element of a row r < count of image b:
//     h  = u + c                      (the forward value: u = m * (relu(z) - c) is what the forward stored)
//     a  = h > 0 ? dh : 0             (through the ReLU)
//     dz = a * m[b, k]                (d L / d z on the active channels)
//     du = dz * s[k]
//     g_shift[k]     += a             (every channel: a masked channel's z = t still feeds the ReLU)
//     g_scale_num[k] += dz * (h - t[k])
//     g_mask[b, k]   += a * (zy - t[k])        zy = s * y + t, the unmasked convolution in the affine form a relu = 0 launch stores
// h and h - t are formed in double from the three fp32 inputs, so h - t carries ONE rounding: with h = fl(u + c) first, a channel whose
// h is close to t would lose the leading digits of s * y to the rounding of u + c.
// g_shift / g_scale_num are column partials 0 / 1 of the work layout, g_mask its image slots.
//
// ldn_rows_postmask_bwd is the same for a mask applied AFTER the ReLU (LAD-RegNet: h = m * relu(zy), the UNMASKED r = relu(zy) stored), with
// an optional squeeze-excitation prologue on the incoming gradient; per element of a row r < count of image b:
//     dh = gate ? fma(dz, gate[b, k], dsq[b, k]) : dz          (one rounding)
//     a  = r > 0 ? dh * m[b, k] : 0
//     du = a * s[k]
//     g_shift[k]     += a
//     g_scale_num[k] += a * (r - t[k])
//     g_mask[b, k]   += dh * r              (every channel: non-zero exactly where the activation is on, masked channels included)
// ldn_rows_img_dot is its per-image reduction alone: out[b, k] = sum over the rows of image b of a[r, k] * b[r, k], image slots without columns.
#include "ldn_rows_plan.h"

namespace ldn {

// u[r, k] *= chan_mask[img(r), k] for r < count; rows [count, m_cap) = 0.  One thread per (row, quad).
__global__ __launch_bounds__(256) void k_rows_chanmask(float* u, int ldu, const int32_t* prefix, int B, const float* chan_mask,
                                                       const int32_t* m_count, int m_cap, int C) {
    const int Q = C >> 2;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t r64 = i / Q;
    if (r64 >= (size_t)m_cap) return;
    const int r = (int)r64, q = (int)(i - r64 * Q);
    float* dst = u + (size_t)r * ldu + 4 * q;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (r < rows_count(m_count, m_cap)) {
        const int b = image_of_row(prefix, B, r);
        v = *reinterpret_cast<const f32x4*>(dst) * *reinterpret_cast<const f32x4*>(chan_mask + (size_t)b * C + 4 * q);
    }
    store16(dst, v);
}

// B = 0 without a per-image argument (chan_mask / zy; chan_mask / gate / g_mask; chan_mask / g_mask): the walk is then one segment
struct ActArgs {
    const float* dh; const float* u; const float* post_sub; const float* scale; const float* shift; const float* chan_mask;
    const int32_t* prefix; const float* zy; const int32_t* m_count;
    float* du; float* work;
    int lddh, ldu, ldzy, lddu, B, m_cap, C, splits, rps;
};

__global__ __launch_bounds__(ACT_THREADS) void k_rows_act_bwd(const ActArgs p) {
    __shared__ f32x4 s_red[ACT_THREADS];
    const RowWalk w = row_walk(p.C, p.m_count, p.m_cap, p.rps);
    zero_past_count(w, p.du, p.lddu);
    if (w.empty()) return;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 sc = zero, sh = zero, c = zero;
    if (w.active) {
        sc = ld4(p.scale + w.k);
        sh = ld4(p.shift + w.k);
        if (p.post_sub) c = ld4(p.post_sub + w.k);
    }
    f32x4 g_sh = zero, g_sc = zero;
    for_each_image_segment(w, p.prefix, p.B, [&](int b, int r0, int seg_end) {
        f32x4 m = {1.f, 1.f, 1.f, 1.f}, g_m = zero;
        if (w.active && p.chan_mask) m = ld4(p.chan_mask + (size_t)b * p.C + w.k);
        if (w.active)
            for (int r = r0 + w.rl; r < seg_end; r += w.RL) {
                const f32x4 dh = ld4(p.dh + (size_t)r * p.lddh + w.k);
                const f32x4 u = ld4(p.u + (size_t)r * p.ldu + w.k);
                f32x4 zy = zero;
                if (p.zy) zy = ld4(p.zy + (size_t)r * p.ldzy + w.k);
                f32x4 du;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const double h = (double)u[i] + (double)c[i];
                    const float a = h > 0.0 ? dh[i] : 0.f;
                    const float dz = a * m[i];
                    du[i] = dz * sc[i];
                    g_sh[i] += a;
                    g_sc[i] += dz * (float)(h - (double)sh[i]);
                    g_m[i] += a * (zy[i] - sh[i]);
                }
                store16(p.du + (size_t)r * p.lddu + w.k, du);
            }
        if (p.zy) lane_sum_to(s_red, w, g_m, work_slot(p.work, p.splits, p.C, 2, w.split + b));
    });
    lane_sum_to(s_red, w, g_sh, work_col(p.work, p.splits, p.C, 0, w.split));
    lane_sum_to(s_red, w, g_sc, work_col(p.work, p.splits, p.C, 1, w.split));
}

struct PmArgs {
    const float* dz; const float* r; const float* scale; const float* shift; const float* chan_mask; const int32_t* prefix;
    const float* gate; const float* dsq; const int32_t* m_count;
    float* du; float* g_mask; float* work;
    int lddz, ldr, lddu, B, m_cap, C, splits, rps;
};

__global__ __launch_bounds__(ACT_THREADS) void k_rows_postmask_bwd(const PmArgs p) {
    __shared__ f32x4 s_red[ACT_THREADS];
    const RowWalk w = row_walk(p.C, p.m_count, p.m_cap, p.rps);
    zero_past_count(w, p.du, p.lddu);
    if (w.empty()) return;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 sc = zero, sh = zero;
    if (w.active) {
        sc = ld4(p.scale + w.k);
        sh = ld4(p.shift + w.k);
    }
    f32x4 g_sh = zero, g_sc = zero;
    for_each_image_segment(w, p.prefix, p.B, [&](int b, int r0, int seg_end) {
        f32x4 m = {1.f, 1.f, 1.f, 1.f}, ga = zero, dq = zero, g_m = zero;
        if (w.active && p.chan_mask) m = ld4(p.chan_mask + (size_t)b * p.C + w.k);
        if (w.active && p.gate) {
            ga = ld4(p.gate + (size_t)b * p.C + w.k);
            dq = ld4(p.dsq + (size_t)b * p.C + w.k);
        }
        if (w.active)
            for (int r = r0 + w.rl; r < seg_end; r += w.RL) {
                const f32x4 dz = ld4(p.dz + (size_t)r * p.lddz + w.k);
                const f32x4 rv = ld4(p.r + (size_t)r * p.ldr + w.k);
                f32x4 du;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float dh = p.gate ? fmaf(dz[i], ga[i], dq[i]) : dz[i];
                    const float a = rv[i] > 0.f ? dh * m[i] : 0.f;
                    du[i] = a * sc[i];
                    g_sh[i] += a;
                    g_sc[i] += a * (rv[i] - sh[i]);
                    g_m[i] += dh * rv[i];
                }
                store16(p.du + (size_t)r * p.lddu + w.k, du);
            }
        if (p.g_mask) lane_sum_to(s_red, w, g_m, work_slot(p.work, p.splits, p.C, 2, w.split + b));
    });
    lane_sum_to(s_red, w, g_sh, work_col(p.work, p.splits, p.C, 0, w.split));
    lane_sum_to(s_red, w, g_sc, work_col(p.work, p.splits, p.C, 1, w.split));
}

struct DotArgs {
    const float* a; const float* b; const int32_t* prefix; const int32_t* m_count; float* work;
    int lda, ldb, B, m_cap, C, splits, rps;
};

__global__ __launch_bounds__(ACT_THREADS) void k_rows_img_dot(const DotArgs p) {
    __shared__ f32x4 s_red[ACT_THREADS];
    const RowWalk w = row_walk(p.C, p.m_count, p.m_cap, p.rps);
    if (w.empty()) return;
    for_each_image_segment(w, p.prefix, p.B, [&](int b, int r0, int seg_end) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        if (w.active)
            for (int r = r0 + w.rl; r < seg_end; r += w.RL) acc += ld4(p.a + (size_t)r * p.lda + w.k) * ld4(p.b + (size_t)r * p.ldb + w.k);
        lane_sum_to(s_red, w, acc, work_slot(p.work, p.splits, p.C, 0, w.split + b));
    });
}

// the reducer of ldn_rows_plan.h: thread i owns quad i % Q of column vector j = i / Q < ncols, or of image j - ncols
__global__ __launch_bounds__(256) void k_rows_reduce(const RowsReduceArgs p) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int Q = p.C >> 2;
    if (i >= (p.ncols + p.nimg) * Q) return;
    const int j = i / Q, k = 4 * (i - j * Q);
    const int count = rows_count(p.m_count, p.m_cap);
    if (j < p.ncols) {
        f32x4 s = {0.f, 0.f, 0.f, 0.f};
        const int live = min(p.splits, ceil_div(count, p.rps));
        for (int t = 0; t < live; ++t) s += ld4(p.cols + ((size_t)j * p.splits + t) * p.C + k);
        st4(p.col_out[j] + k, s);
        return;
    }
    const int b = j - p.ncols;
    st4(p.img_out + (size_t)b * p.C + k, image_slots_sum(p.slots, p.prefix, p.B, b, count, p.splits, p.rps, p.C, k));
}

int rows_reduce(const RowsReduceArgs& p, hipStream_t stream) {
    k_rows_reduce<<<ceil_div((p.ncols + p.nimg) * (p.C / 4), 256), 256, 0, stream>>>(p);
    LDN_CHECK_LAUNCH("k_rows_reduce");
    return LDN_OK;
}

// ---- ldn_rows_ln_bwd: the LayerNorm backward on listed rows.  One WAVE per row (the row sums are wave reductions: lane l owns the quads l, l + 64, ...
// of the row, at most LN_MAXQ of them); a workgroup of four waves owns the list entries [split * rps, + rps), wave w every fourth of them.  The lanes'
// column sums (d_gamma, d_beta) over the wave's rows stay in registers, the four waves' are added in wave order through the LDS, and the
// workgroup writes them as the column partials 0 / 1 of its split (the work layout and the reducer of ldn_rows_plan.h).
constexpr int LN_THREADS = 256;
constexpr int LN_WAVES = LN_THREADS / 64;
constexpr int LN_MAXQ = 8;             // quads per lane: C <= 2048 (= ldn_row_stats)
constexpr int LN_MIN_SPLIT_ROWS = 32;
constexpr int LN_MAX_SPLITS = 512;

struct LnArgs {
    const float* x; const float* stats; const float* gamma; const int32_t* list; const int32_t* count; const float* dy;
    float* dx; float* xhat; float* work;
    int ldx, lddy, lddx, ldxh, rows, m_cap, C, splits, rps;
};

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(LN_THREADS) void k_rows_ln_bwd(const LnArgs p) {
    __shared__ f32x4 s_red[LN_WAVES][2][64];
    const int Q = p.C >> 2;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int split = blockIdx.x;
    const int count = rows_count(p.count, p.m_cap);
    const int r_begin = split * p.rps;
    const int r_end = min(count, min(p.m_cap, r_begin + p.rps));
    if (r_begin >= r_end) return;          // (uniform) no rows: the reducer does not read this split's partials
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    const float inv_c = 1.f / (float)p.C;
    f32x4 gam[LN_MAXQ], g_ga[LN_MAXQ], g_be[LN_MAXQ];
#pragma unroll
    for (int i = 0; i < LN_MAXQ; ++i) {
        const int q = lane + 64 * i;
        gam[i] = q < Q ? *reinterpret_cast<const f32x4*>(p.gamma + 4 * q) : zero;
        g_ga[i] = g_be[i] = zero;
    }
    for (int r = r_begin + wave; r < r_end; r += LN_WAVES) {
        const int src = p.list ? p.list[r] : r;
        if (src < 0 || src >= p.rows) continue;                           // (wave-uniform) a list entry outside the matrix is skipped, never followed
        const float mean = p.stats[2 * (size_t)src], rstd = p.stats[2 * (size_t)src + 1];
        f32x4 xh[LN_MAXQ], g[LN_MAXQ];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int i = 0; i < LN_MAXQ; ++i) {
            const int q = lane + 64 * i;
            xh[i] = g[i] = zero;
            if (q < Q) {
                const f32x4 xv = *reinterpret_cast<const f32x4*>(p.x + (size_t)src * p.ldx + 4 * q);
                const f32x4 dy = *reinterpret_cast<const f32x4*>(p.dy + (size_t)r * p.lddy + 4 * q);
                xh[i] = (xv - mean) * rstd;                               // x^ from the difference: a row with |mean| >> std keeps its digits
                g[i] = dy * gam[i];
                g_be[i] += dy;
                g_ga[i] += dy * xh[i];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    s1 += g[i][e];
                    s2 += g[i][e] * xh[i][e];
                }
            }
        }
        const float c1 = wave_sum(s1) * inv_c, c2 = wave_sum(s2) * inv_c;
#pragma unroll
        for (int i = 0; i < LN_MAXQ; ++i) {
            const int q = lane + 64 * i;
            if (q < Q) {
                float* dst = p.dx + (size_t)src * p.lddx + 4 * q;
                const f32x4 v = *reinterpret_cast<const f32x4*>(dst) + (g[i] - c1 - xh[i] * c2) * rstd;
                store16(dst, v);
                if (p.xhat) store16(p.xhat + (size_t)r * p.ldxh + 4 * q, xh[i]);
            }
        }
    }
    // the four waves' column sums in wave order (the trip count depends on C only: uniform barriers)
    const int npass = ceil_div(Q, 64);
#pragma unroll
    for (int i = 0; i < LN_MAXQ; ++i) {
        if (i >= npass) break;
        s_red[wave][0][lane] = g_ga[i];
        s_red[wave][1][lane] = g_be[i];
        __syncthreads();
        const int q = lane + 64 * i;
        if (wave < 2 && q < Q) {
            f32x4 s = zero;
            for (int w = 0; w < LN_WAVES; ++w) s += s_red[w][wave][lane];
            st4(work_col(p.work, p.splits, p.C, wave, split) + 4 * q, s);
        }
        __syncthreads();
    }
}

// the launch plan: a function of m_cap ONLY
static void ln_plan(int m_cap, int* splits, int* rps) {
    int s = m_cap / LN_MIN_SPLIT_ROWS;
    if (s > LN_MAX_SPLITS) s = LN_MAX_SPLITS;
    if (s < 1) s = 1;
    *rps = ceil_div(m_cap > 0 ? m_cap : 1, s);
    *splits = ceil_div(m_cap > 0 ? m_cap : 1, *rps);
}

}  // namespace ldn

using namespace ldn;

extern "C" int ldn_rows_chanmask(float* u, int ldu, const int32_t* row_prefix, int B, const float* chan_mask, const int32_t* m_count,
                                 int m_cap, int C, void* stream) {
    LDN_REQUIRE(u && row_prefix && chan_mask, "ldn_rows_chanmask: null pointer");
    LDN_REQUIRE(B >= 1 && m_cap >= 0, "ldn_rows_chanmask: B >= 1, m_cap >= 0 (got %d, %d)", B, m_cap);
    LDN_REQUIRE(C > 0 && C % 4 == 0 && ldu >= C && ldu % 4 == 0, "ldn_rows_chanmask: C %% 4 == 0, ldu >= C, ldu %% 4 == 0 (got C %d, ldu %d)", C, ldu);
    LDN_REQUIRE(aligned16(u) && aligned16(chan_mask), "ldn_rows_chanmask: u / chan_mask must be 16-byte aligned");
    if (m_cap == 0) return LDN_OK;
    const size_t n = (size_t)m_cap * (C / 4);
    LDN_REQUIRE((n + 255) / 256 <= 0x7fffffffull, "ldn_rows_chanmask: m_cap * C too large");
    k_rows_chanmask<<<(unsigned)((n + 255) / 256), 256, 0, static_cast<hipStream_t>(stream)>>>(u, ldu, row_prefix, B, chan_mask, m_count, m_cap, C);
    LDN_CHECK_LAUNCH("k_rows_chanmask");
    return LDN_OK;
}

extern "C" size_t ldn_rows_act_bwd_workspace_bytes(int m_cap, int C, int B) { return rows_bwd_work_bytes(m_cap, C, B); }

extern "C" int ldn_rows_act_bwd(const float* dh, int lddh, const float* u, int ldu, const float* post_sub, const float* scale,
                                const float* shift, const float* chan_mask, const int32_t* row_prefix, int B, const float* zy, int ldzy,
                                const int32_t* m_count, int m_cap, int C, float* du, int lddu, float* g_shift, float* g_scale_num,
                                float* g_mask, float* work, void* stream) {
    LDN_REQUIRE(dh && u && scale && shift && du && g_shift && g_scale_num && work, "ldn_rows_act_bwd: null pointer");
    LDN_REQUIRE(m_cap >= 0 && C > 0 && C % 4 == 0, "ldn_rows_act_bwd: m_cap >= 0, C %% 4 == 0 (got %d, %d)", m_cap, C);
    LDN_REQUIRE(lddh >= C && ldu >= C && lddu >= C && lddh % 4 == 0 && ldu % 4 == 0 && lddu % 4 == 0,
                "ldn_rows_act_bwd: leading dimensions >= C and multiples of 4 (got %d, %d, %d)", lddh, ldu, lddu);
    LDN_REQUIRE(!zy || (ldzy >= C && ldzy % 4 == 0), "ldn_rows_act_bwd: ldzy >= C and a multiple of 4 (got %d)", ldzy);
    LDN_REQUIRE(!(chan_mask || zy) || (row_prefix && B >= 1), "ldn_rows_act_bwd: chan_mask / zy need row_prefix [B + 1] and B >= 1");
    LDN_REQUIRE((zy != nullptr) == (g_mask != nullptr), "ldn_rows_act_bwd: g_mask [B][C] is the output that goes with zy: give both or neither");
    LDN_REQUIRE(aligned16(dh) && aligned16(u) && aligned16(post_sub) && aligned16(scale) && aligned16(shift) && aligned16(chan_mask) &&
                aligned16(zy) && aligned16(du) && aligned16(g_shift) && aligned16(g_scale_num) && aligned16(g_mask) && aligned16(work),
                "ldn_rows_act_bwd: every float pointer must be 16-byte aligned");
    ActArgs p;
    p.dh = dh; p.u = u; p.post_sub = post_sub; p.scale = scale; p.shift = shift; p.chan_mask = chan_mask; p.prefix = row_prefix; p.zy = zy;
    p.m_count = m_count; p.du = du; p.work = work;
    p.lddh = lddh; p.ldu = ldu; p.ldzy = ldzy; p.lddu = lddu; p.B = (chan_mask || zy) ? B : 0; p.m_cap = m_cap; p.C = C;
    const dim3 grid = rows_grid(m_cap, C, &p.splits, &p.rps);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (m_cap > 0) {
        k_rows_act_bwd<<<grid, ACT_THREADS, 0, st>>>(p);
        LDN_CHECK_LAUNCH("k_rows_act_bwd");
    }
    return rows_reduce({work, work_slot(work, p.splits, C, 2, 0), row_prefix, m_count, {g_shift, g_scale_num}, g_mask, 2, g_mask ? B : 0, B, m_cap, C,
                        p.splits, p.rps}, st);
}

extern "C" size_t ldn_rows_postmask_bwd_workspace_bytes(int m_cap, int C, int B) { return rows_bwd_work_bytes(m_cap, C, B); }

extern "C" int ldn_rows_postmask_bwd(const float* dz, int lddz, const float* r, int ldr, const float* scale, const float* shift,
                                     const float* chan_mask, const int32_t* row_prefix, int B, const float* gate, const float* dsq,
                                     const int32_t* m_count, int m_cap, int C, float* du, int lddu, float* g_shift, float* g_scale_num,
                                     float* g_mask, float* work, void* stream) {
    LDN_REQUIRE(dz && r && scale && shift && du && g_shift && g_scale_num && work, "ldn_rows_postmask_bwd: null pointer");
    LDN_REQUIRE(m_cap >= 0 && C > 0 && C % 4 == 0, "ldn_rows_postmask_bwd: m_cap >= 0, C %% 4 == 0 (got %d, %d)", m_cap, C);
    LDN_REQUIRE(lddz >= C && ldr >= C && lddu >= C && lddz % 4 == 0 && ldr % 4 == 0 && lddu % 4 == 0,
                "ldn_rows_postmask_bwd: leading dimensions >= C and multiples of 4 (got %d, %d, %d)", lddz, ldr, lddu);
    LDN_REQUIRE((gate != nullptr) == (dsq != nullptr), "ldn_rows_postmask_bwd: gate and dsq [B][C] are the SE prologue: give both or neither");
    const bool per_image = chan_mask || gate || g_mask;
    LDN_REQUIRE(!per_image || (row_prefix && B >= 1), "ldn_rows_postmask_bwd: chan_mask / gate / g_mask need row_prefix [B + 1] and B >= 1");
    LDN_REQUIRE(aligned16(dz) && aligned16(r) && aligned16(scale) && aligned16(shift) && aligned16(chan_mask) && aligned16(gate) && aligned16(dsq) &&
                aligned16(du) && aligned16(g_shift) && aligned16(g_scale_num) && aligned16(g_mask) && aligned16(work),
                "ldn_rows_postmask_bwd: every float pointer must be 16-byte aligned");
    PmArgs p;
    p.dz = dz; p.r = r; p.scale = scale; p.shift = shift; p.chan_mask = chan_mask; p.prefix = row_prefix; p.gate = gate; p.dsq = dsq;
    p.m_count = m_count; p.du = du; p.g_mask = g_mask; p.work = work;
    p.lddz = lddz; p.ldr = ldr; p.lddu = lddu; p.B = per_image ? B : 0; p.m_cap = m_cap; p.C = C;
    const dim3 grid = rows_grid(m_cap, C, &p.splits, &p.rps);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (m_cap > 0) {
        k_rows_postmask_bwd<<<grid, ACT_THREADS, 0, st>>>(p);
        LDN_CHECK_LAUNCH("k_rows_postmask_bwd");
    }
    return rows_reduce({work, work_slot(work, p.splits, C, 2, 0), row_prefix, m_count, {g_shift, g_scale_num}, g_mask, 2, g_mask ? B : 0, B, m_cap, C,
                        p.splits, p.rps}, st);
}

extern "C" size_t ldn_rows_img_dot_workspace_bytes(int m_cap, int C, int B) {
    if (m_cap < 0 || C <= 0 || C % 4 || B < 1) return 0;
    return rows_work_bytes(m_cap, C, 0, B);
}

extern "C" int ldn_rows_img_dot(const float* a, int lda, const float* b, int ldb, const int32_t* row_prefix, int B, const int32_t* m_count,
                                int m_cap, int C, float* out, float* work, void* stream) {
    LDN_REQUIRE(a && b && row_prefix && out && work, "ldn_rows_img_dot: null pointer");
    LDN_REQUIRE(B >= 1 && m_cap >= 0 && C > 0 && C % 4 == 0, "ldn_rows_img_dot: B >= 1, m_cap >= 0, C %% 4 == 0 (got %d, %d, %d)", B, m_cap, C);
    LDN_REQUIRE(lda >= C && ldb >= C && lda % 4 == 0 && ldb % 4 == 0, "ldn_rows_img_dot: leading dimensions >= C and multiples of 4 (got %d, %d)", lda, ldb);
    LDN_REQUIRE(aligned16(a) && aligned16(b) && aligned16(out) && aligned16(work), "ldn_rows_img_dot: every float pointer must be 16-byte aligned");
    DotArgs p;
    p.a = a; p.b = b; p.prefix = row_prefix; p.m_count = m_count; p.work = work;
    p.lda = lda; p.ldb = ldb; p.B = B; p.m_cap = m_cap; p.C = C;
    const dim3 grid = rows_grid(m_cap, C, &p.splits, &p.rps);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (m_cap > 0) {
        k_rows_img_dot<<<grid, ACT_THREADS, 0, st>>>(p);
        LDN_CHECK_LAUNCH("k_rows_img_dot");
    }
    return rows_reduce({nullptr, work, row_prefix, m_count, {nullptr, nullptr}, out, 0, B, B, m_cap, C, p.splits, p.rps}, st);
}

extern "C" size_t ldn_rows_ln_bwd_workspace_bytes(int m_cap, int C) {
    if (m_cap < 0 || C <= 0 || C % 4) return 0;
    int splits, rps;
    ln_plan(m_cap, &splits, &rps);
    return (size_t)2 * splits * C * sizeof(float);
}

extern "C" int ldn_rows_ln_bwd(const float* x, int ldx, int rows, const float* stats, const float* gamma, const int32_t* list,
                               const int32_t* count, int m_cap, int C, const float* dy, int lddy, float* dx, int lddx, float* d_gamma,
                               float* d_beta, float* xhat, int ldxh, float* work, void* stream) {
    LDN_REQUIRE(x && stats && gamma && dy && dx && d_gamma && d_beta && work, "ldn_rows_ln_bwd: null pointer");
    LDN_REQUIRE(rows >= 0 && m_cap >= 0 && C > 0 && C % 4 == 0 && C <= 256 * LN_MAXQ,
                "ldn_rows_ln_bwd: rows >= 0, m_cap >= 0, C %% 4 == 0, C <= %d (got %d, %d, %d)", 256 * LN_MAXQ, rows, m_cap, C);
    LDN_REQUIRE(list || m_cap <= rows, "ldn_rows_ln_bwd: without a list the rows are 0 .. m_cap - 1: m_cap %d exceeds %d rows", m_cap, rows);
    LDN_REQUIRE(ldx >= C && lddy >= C && lddx >= C && ldx % 4 == 0 && lddy % 4 == 0 && lddx % 4 == 0,
                "ldn_rows_ln_bwd: leading dimensions >= C and multiples of 4 (got %d, %d, %d)", ldx, lddy, lddx);
    LDN_REQUIRE(!xhat || (ldxh >= C && ldxh % 4 == 0), "ldn_rows_ln_bwd: ldxh >= C and a multiple of 4 (got %d)", ldxh);
    LDN_REQUIRE(aligned16(x) && aligned16(gamma) && aligned16(dy) && aligned16(dx) && aligned16(d_gamma) && aligned16(d_beta) && aligned16(xhat) &&
                aligned16(work), "ldn_rows_ln_bwd: every float pointer except stats must be 16-byte aligned");
    LnArgs p;
    p.x = x; p.stats = stats; p.gamma = gamma; p.list = list; p.count = count; p.dy = dy; p.dx = dx;
    p.xhat = xhat; p.work = work; p.ldx = ldx; p.lddy = lddy; p.lddx = lddx; p.ldxh = ldxh; p.rows = rows; p.m_cap = m_cap; p.C = C;
    ln_plan(m_cap, &p.splits, &p.rps);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (m_cap > 0) {
        k_rows_ln_bwd<<<(unsigned)p.splits, LN_THREADS, 0, st>>>(p);
        LDN_CHECK_LAUNCH("k_rows_ln_bwd");
    }
    return rows_reduce({work, nullptr, nullptr, count, {d_gamma, d_beta}, nullptr, 2, 0, 0, m_cap, C, p.splits, p.rps}, st);
}
