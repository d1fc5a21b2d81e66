// ldn_train_bn.hip -- BatchNorm on BATCH statistics over packed rows, forward and backward (ldn_rows_bn_stats, ldn_rows_bn_fwd, ldn_rows_bn_bwd,
// ldn_rows_bn_postmask_fwd, ldn_rows_bn_postmask_bwd; include/ldn_hip.h): what training needs of the reference's own recipe, where bn1 / bn2 / bn3 normalise with the statistics of the batch.
//
// Bandwidth-bound fp32 row kernels, whatever the math mode of the convolutions around them; all but ldn_rows_bn_fwd (one thread per row and
// quad) are the walk of ldn_rows_plan.h, with its zeros past the count, its partials, its reducer and its bit-identical sums.
//
// The optional channel mask c [B][C] multiplies u BEFORE the statistics and the normalisation (the reference's apply_channel_mask in front of
// bn1 / bn2): x = c[img(r)][k] * u[r][k], a channel dropped in one image contributes zeros to the batch statistics.  u itself is the UNMASKED
// convolution output -- the backward needs it for the mask's straight-through term.  The image of a row comes from the per-image row prefix,
// by the walk's image segments (statistics, backward) or a binary search per thread (forward).
//
// ldn_rows_bn_stats: mean and BIASED variance over the rows below the count, never as E[x^2] - E[x]^2.  A thread runs Welford's update over its
// rows; (n, mean, M2) triples are merged pairwise with Chan's formula -- the row lanes in ascending lane order, then the splits in ascending
// split order (n of a split follows from the count: it is not stored).  invstd = 1 / sqrt(var + eps).
//
// ldn_rows_bn_fwd: h = row_scale[r] * relu?(gamma * (x - mean) * invstd + beta), one pass, one thread per (row, quad).
//
// ldn_rows_bn_bwd, per element of a row r < count:  xhat = (x - mean) * invstd,  dz = row_scale[r] * (gate ? dh : 0).
// The ReLU gate is READ FROM THE STORED h (h > 0 <=> gamma * xhat + beta > 0: the forward's own decision, whatever the compiler contracts), not
// recomputed; h == NULL: no ReLU.  Launches 1 + 2: d_beta[k] = sum dz, d_gamma[k] = sum dz * xhat.  Launch 3:
//     g  = gamma * invstd * (dz - d_beta / n - xhat * d_gamma / n)        n = the device-side count        (= d L / d x)
//     du = c[img(r)][k] * g                                                                                (= d L / d u)
// and, where the mask's straight-through gradient is wanted, g_mask[b][k] = sum over the rows of image b of g * u -- FUSED into launch 3 through
// the image slots and one more reducer launch that adds them: four launches, against six for the same through
// ldn_rows_img_dot (two) and ldn_rows_chanmask (one) behind a three-launch backward.
//
// ldn_rows_bn_postmask_fwd / ldn_rows_bn_postmask_bwd (further down) are the same for a mask applied AFTER BatchNorm + ReLU (LAD-RegNet channel
// mode: h = m * relu(gamma * xhat + beta), statistics without a mask), with ldn_rows_postmask_bwd's optional squeeze-excitation prologue:
//     dh = gate ? fma(dz, gate[b, k], dsq[b, k]) : dz        a = h > 0 ? dh * m[b, k] : 0        (the gate read from the stored MASKED h)
//     d_beta[k] = sum a        d_gamma[k] = sum a * xhat        g_mask[b, k] = sum over image b of dh * relu(gamma * xhat + beta)
//     du = gamma * invstd * (a - d_beta / n - xhat * d_gamma / n)
// g_mask needs the UNMASKED ReLU output, which h does not hold at a masked channel: it is recomputed.  It needs none of the reduced sums, so it
// rides in launch 1 and ONE reducer launch adds d_beta, d_gamma and g_mask: three launches.
#include "ldn_rows_plan.h"

namespace ldn {

// Chan's merge of (nb, mb, m2b) into (na, ma, m2a); nb > 0
__device__ __forceinline__ void chan_merge(int& na, f32x4& ma, f32x4& m2a, int nb, const f32x4 mb, const f32x4 m2b) {
    const int n = na + nb;
    const float fb = (float)nb / (float)n;
    const f32x4 d = mb - ma;
    ma += d * fb;
    m2a += m2b + d * d * ((float)na * fb);
    na = n;
}

struct BnStatArgs {
    const float* u; const float* chan_mask; const int32_t* prefix; const int32_t* m_count;
    float* mean; float* var; float* invstd; float* work;
    float eps;
    int ldu, B, m_cap, C, splits, rps;
};

// column partials 0 / 1 of the work layout: the split's mean and M2
__global__ __launch_bounds__(ACT_THREADS) void k_bn_stats_partial(const BnStatArgs p) {
    __shared__ f32x4 s_mean[ACT_THREADS], s_m2[ACT_THREADS];
    __shared__ int s_n[ACT_THREADS];
    const RowWalk w = row_walk(p.C, p.m_count, p.m_cap, p.rps);
    if (w.empty()) return;                 // k_bn_stats_reduce does not read this split's partials either
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 mean = zero, m2 = zero;
    int n = 0;
    for_each_image_segment(w, p.prefix, p.B, [&](int b, int r0, int seg_end) {
        if (!w.active) return;
        f32x4 m = {1.f, 1.f, 1.f, 1.f};
        if (p.chan_mask) m = ld4(p.chan_mask + (size_t)b * p.C + w.k);
        for (int r = r0 + w.rl; r < seg_end; r += w.RL) {
            const f32x4 x = ld4(p.u + (size_t)r * p.ldu + w.k) * m;
            ++n;
            const f32x4 d = x - mean;
            mean += d * (1.f / (float)n);
            m2 += d * (x - mean);
        }
    });
    s_mean[threadIdx.x] = mean;
    s_m2[threadIdx.x] = m2;
    s_n[threadIdx.x] = n;
    __syncthreads();
    if (w.active && w.rl == 0) {           // lane_sum's order, Chan's merge for its addition
        f32x4 ma = zero, m2a = zero;
        int na = 0;
        for (int j = 0; j < w.RL; ++j) {
            const int i = w.lane_slot(j);
            if (s_n[i] > 0) chan_merge(na, ma, m2a, s_n[i], s_mean[i], s_m2[i]);
        }
        st4(work_col(p.work, p.splits, p.C, 0, w.split) + w.k, ma);
        st4(work_col(p.work, p.splits, p.C, 1, w.split) + w.k, m2a);
    }
}

// rows_reduce with Chan's merge for its addition: one thread per quad, the splits that hold rows in ascending order; a split's n follows from the count
__global__ __launch_bounds__(256) void k_bn_stats_reduce(const BnStatArgs p) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= (p.C >> 2)) return;
    const int k = 4 * i;
    const int count = rows_count(p.m_count, p.m_cap);
    const int live = min(p.splits, ceil_div(count, p.rps));
    f32x4 ma = {0.f, 0.f, 0.f, 0.f}, m2a = ma;
    int na = 0;
    for (int t = 0; t < live; ++t) {
        const int nb = min(count - t * p.rps, p.rps);
        chan_merge(na, ma, m2a, nb, ld4(work_col(p.work, p.splits, p.C, 0, t) + k), ld4(work_col(p.work, p.splits, p.C, 1, t) + k));
    }
    const f32x4 var = na > 0 ? m2a * (1.f / (float)na) : m2a;
    f32x4 inv;
#pragma unroll
    for (int e = 0; e < 4; ++e) inv[e] = 1.f / sqrtf(var[e] + p.eps);
    st4(p.mean + k, ma);
    st4(p.var + k, var);
    st4(p.invstd + k, inv);
}

struct BnFwdArgs {
    const float* u; const float* mean; const float* invstd; const float* gamma; const float* beta; const float* chan_mask;
    const int32_t* prefix; const float* row_scale; const int32_t* m_count;
    float* h;
    int ldu, ldh, B, m_cap, C, relu;
};

// one thread per (row, quad); h may be u itself
__global__ __launch_bounds__(256) void k_rows_bn_fwd(const BnFwdArgs p) {
    const int Q = p.C >> 2;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t r64 = i / Q;
    if (r64 >= (size_t)p.m_cap) return;
    const int r = (int)r64, k = 4 * (int)(i - r64 * Q);
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (r < rows_count(p.m_count, p.m_cap)) {
        f32x4 x = ld4(p.u + (size_t)r * p.ldu + k);
        if (p.chan_mask) x *= ld4(p.chan_mask + (size_t)image_of_row(p.prefix, p.B, r) * p.C + k);
        v = ld4(p.gamma + k) * ((x - ld4(p.mean + k)) * ld4(p.invstd + k)) + ld4(p.beta + k);
        if (p.relu) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = v[e] > 0.f ? v[e] : 0.f;
        }
        if (p.row_scale) v *= p.row_scale[r];
    }
    store16(p.h + (size_t)r * p.ldh + k, v);
}

struct BnBwdArgs {
    const float* dh; const float* u; const float* h; const float* mean; const float* invstd; const float* gamma; const float* chan_mask;
    const int32_t* prefix; const float* row_scale; const int32_t* m_count;
    float* du; float* d_gamma; float* d_beta; float* g_mask; float* work;
    int lddh, ldu, ldh, lddu, B, m_cap, C, splits, rps;
};

// (xhat, dz) of one quad of row r; m = the channel mask of the row's image (ones without one)
__device__ __forceinline__ void bn_bwd_quad(const BnBwdArgs& p, int r, int k, const f32x4 m, const f32x4 mean, const f32x4 inv, f32x4& u, f32x4& xhat,
                                            f32x4& dz) {
    u = ld4(p.u + (size_t)r * p.ldu + k);
    xhat = (u * m - mean) * inv;
    dz = ld4(p.dh + (size_t)r * p.lddh + k);
    if (p.h) {
        const f32x4 h = ld4(p.h + (size_t)r * p.ldh + k);
#pragma unroll
        for (int e = 0; e < 4; ++e) dz[e] = h[e] > 0.f ? dz[e] : 0.f;
    }
    if (p.row_scale) dz *= p.row_scale[r];
}

// launch 1: the split's partial d_beta / d_gamma, column partials 0 / 1 of the work layout
__global__ __launch_bounds__(ACT_THREADS) void k_bn_bwd_partial(const BnBwdArgs p) {
    __shared__ f32x4 s_red[ACT_THREADS];
    const RowWalk w = row_walk(p.C, p.m_count, p.m_cap, p.rps);
    if (w.empty()) return;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 mean = zero, inv = zero, g_b = zero, g_g = zero;
    if (w.active) {
        mean = ld4(p.mean + w.k);
        inv = ld4(p.invstd + w.k);
    }
    // (g_mask alone does not cut this launch's rows into images: a thread's rows, and so the order of its sum, depend on the segments)
    for_each_image_segment(w, p.prefix, p.chan_mask ? p.B : 0, [&](int b, int r0, int seg_end) {
        if (!w.active) return;
        f32x4 m = {1.f, 1.f, 1.f, 1.f};
        if (p.chan_mask) m = ld4(p.chan_mask + (size_t)b * p.C + w.k);
        for (int r = r0 + w.rl; r < seg_end; r += w.RL) {
            f32x4 u, xhat, dz;
            bn_bwd_quad(p, r, w.k, m, mean, inv, u, xhat, dz);
            g_b += dz;
            g_g += dz * xhat;
        }
    });
    lane_sum_to(s_red, w, g_b, work_col(p.work, p.splits, p.C, 0, w.split));
    lane_sum_to(s_red, w, g_g, work_col(p.work, p.splits, p.C, 1, w.split));
}

// launch 3 (launch 2 has reduced d_beta / d_gamma): du, and the partial g_mask of every image that owns rows of the split, in the image slots
__global__ __launch_bounds__(ACT_THREADS) void k_bn_bwd_final(const BnBwdArgs p) {
    __shared__ f32x4 s_red[ACT_THREADS];
    const RowWalk w = row_walk(p.C, p.m_count, p.m_cap, p.rps);
    zero_past_count(w, p.du, p.lddu);
    if (w.empty()) return;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 mean = zero, inv = zero, gi = zero, cb = zero, cg = zero;
    if (w.active) {
        const float inv_n = 1.f / (float)w.count;          // (count >= r_end > 0)
        mean = ld4(p.mean + w.k);
        inv = ld4(p.invstd + w.k);
        gi = ld4(p.gamma + w.k) * inv;
        cb = ld4(p.d_beta + w.k) * inv_n;
        cg = ld4(p.d_gamma + w.k) * inv_n;
    }
    for_each_image_segment(w, p.prefix, p.B, [&](int b, int r0, int seg_end) {
        f32x4 m = {1.f, 1.f, 1.f, 1.f}, g_m = zero;
        if (w.active) {
            if (p.chan_mask) m = ld4(p.chan_mask + (size_t)b * p.C + w.k);
            for (int r = r0 + w.rl; r < seg_end; r += w.RL) {
                f32x4 u, xhat, dz;
                bn_bwd_quad(p, r, w.k, m, mean, inv, u, xhat, dz);
                const f32x4 g = gi * (dz - cb - xhat * cg);
                g_m += g * u;
                store16(p.du + (size_t)r * p.lddu + w.k, g * m);
            }
        }
        if (p.g_mask) lane_sum_to(s_red, w, g_m, work_slot(p.work, p.splits, p.C, 2, w.split + b));
    });
}

// ---- the POST-ACTIVATION form (LAD-RegNet channel mode): the mask multiplies after BatchNorm + ReLU, so every channel of every image feeds the
// statistics (ldn_rows_bn_stats without a mask) and the stored h = m * relu(..) holds no unmasked ReLU output: the backward recomputes it.
struct BnPmFwdArgs {
    const float* u; const float* mean; const float* invstd; const float* gamma; const float* beta; const float* chan_mask;
    const int32_t* prefix; const int32_t* m_count;
    float* h;
    int ldu, ldh, B, m_cap, C;
};

// one thread per (row, quad); h may be u itself
__global__ __launch_bounds__(256) void k_rows_bn_postmask_fwd(const BnPmFwdArgs p) {
    const int Q = p.C >> 2;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t r64 = i / Q;
    if (r64 >= (size_t)p.m_cap) return;
    const int r = (int)r64, k = 4 * (int)(i - r64 * Q);
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (r < rows_count(p.m_count, p.m_cap)) {
        v = ld4(p.gamma + k) * ((ld4(p.u + (size_t)r * p.ldu + k) - ld4(p.mean + k)) * ld4(p.invstd + k)) + ld4(p.beta + k);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = v[e] > 0.f ? v[e] : 0.f;
        if (p.chan_mask) v *= ld4(p.chan_mask + (size_t)image_of_row(p.prefix, p.B, r) * p.C + k);
    }
    store16(p.h + (size_t)r * p.ldh + k, v);
}

struct BnPmBwdArgs {
    const float* dz; const float* u; const float* h; const float* mean; const float* invstd; const float* gamma; const float* beta;
    const float* chan_mask; const int32_t* prefix; const float* gate; const float* dsq; const int32_t* m_count;
    float* du; float* d_gamma; float* d_beta; float* g_mask; float* work;
    int lddz, ldu, ldh, lddu, B, m_cap, C, splits, rps;
};

// what a thread keeps of its image for the length of a segment: the mask and the SE prologue of its quad (ones / unused without them)
struct BnPmImage { f32x4 m, ga, dq; };

__device__ __forceinline__ BnPmImage bn_pm_image(const BnPmBwdArgs& p, int b, int k) {
    BnPmImage im;
    im.m = f32x4{1.f, 1.f, 1.f, 1.f};
    im.ga = im.dq = f32x4{0.f, 0.f, 0.f, 0.f};
    if (p.chan_mask) im.m = ld4(p.chan_mask + (size_t)b * p.C + k);
    if (p.gate) {
        im.ga = ld4(p.gate + (size_t)b * p.C + k);
        im.dq = ld4(p.dsq + (size_t)b * p.C + k);
    }
    return im;
}

// (dh, xhat, a) of one quad of row r: the prologue as ldn_rows_postmask_bwd's (one rounding), the ReLU gate READ FROM THE STORED h
__device__ __forceinline__ void bn_pm_quad(const BnPmBwdArgs& p, int r, int k, const BnPmImage& im, const f32x4 mean, const f32x4 inv, f32x4& dh,
                                           f32x4& xhat, f32x4& a) {
    xhat = (ld4(p.u + (size_t)r * p.ldu + k) - mean) * inv;
    const f32x4 dz = ld4(p.dz + (size_t)r * p.lddz + k);
    const f32x4 h = ld4(p.h + (size_t)r * p.ldh + k);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        dh[e] = p.gate ? fmaf(dz[e], im.ga[e], im.dq[e]) : dz[e];
        a[e] = h[e] > 0.f ? dh[e] * im.m[e] : 0.f;
    }
}

// launch 1: the split's partial d_beta / d_gamma (column partials 0 / 1) and -- it needs none of the reduced sums -- the partial g_mask of every
// image that owns rows of the split (image slots); launch 2, ONE rows_reduce, adds all three
__global__ __launch_bounds__(ACT_THREADS) void k_bn_pm_bwd_partial(const BnPmBwdArgs p) {
    __shared__ f32x4 s_red[ACT_THREADS];
    const RowWalk w = row_walk(p.C, p.m_count, p.m_cap, p.rps);
    if (w.empty()) return;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 mean = zero, inv = zero, gam = zero, bet = zero, g_b = zero, g_g = zero;
    if (w.active) {
        mean = ld4(p.mean + w.k);
        inv = ld4(p.invstd + w.k);
        gam = ld4(p.gamma + w.k);
        bet = ld4(p.beta + w.k);
    }
    for_each_image_segment(w, p.prefix, p.B, [&](int b, int r0, int seg_end) {
        f32x4 g_m = zero;
        if (w.active) {
            const BnPmImage im = bn_pm_image(p, b, w.k);
            for (int r = r0 + w.rl; r < seg_end; r += w.RL) {
                f32x4 dh, xhat, a;
                bn_pm_quad(p, r, w.k, im, mean, inv, dh, xhat, a);
                g_b += a;
                g_g += a * xhat;
                f32x4 rv = gam * xhat + bet;               // the UNMASKED ReLU output: a masked channel's is not in h
#pragma unroll
                for (int e = 0; e < 4; ++e) rv[e] = rv[e] > 0.f ? rv[e] : 0.f;
                g_m += dh * rv;
            }
        }
        if (p.g_mask) lane_sum_to(s_red, w, g_m, work_slot(p.work, p.splits, p.C, 2, w.split + b));
    });
    lane_sum_to(s_red, w, g_b, work_col(p.work, p.splits, p.C, 0, w.split));
    lane_sum_to(s_red, w, g_g, work_col(p.work, p.splits, p.C, 1, w.split));
}

// launch 3: du
__global__ __launch_bounds__(ACT_THREADS) void k_bn_pm_bwd_final(const BnPmBwdArgs p) {
    const RowWalk w = row_walk(p.C, p.m_count, p.m_cap, p.rps);
    zero_past_count(w, p.du, p.lddu);
    if (w.empty() || !w.active) return;                    // (no barrier below)
    const float inv_n = 1.f / (float)w.count;              // (count >= r_end > 0)
    const f32x4 mean = ld4(p.mean + w.k), inv = ld4(p.invstd + w.k);
    const f32x4 gi = ld4(p.gamma + w.k) * inv, cb = ld4(p.d_beta + w.k) * inv_n, cg = ld4(p.d_gamma + w.k) * inv_n;
    for_each_image_segment(w, p.prefix, p.B, [&](int b, int r0, int seg_end) {
        const BnPmImage im = bn_pm_image(p, b, w.k);
        for (int r = r0 + w.rl; r < seg_end; r += w.RL) {
            f32x4 dh, xhat, a;
            bn_pm_quad(p, r, w.k, im, mean, inv, dh, xhat, a);
            store16(p.du + (size_t)r * p.lddu + w.k, gi * (a - cb - xhat * cg));
        }
    });
}

}  // namespace ldn

using namespace ldn;

extern "C" size_t ldn_rows_bn_stats_workspace_bytes(int m_cap, int C) {
    if (m_cap < 0 || C <= 0 || C % 4) return 0;
    return rows_work_bytes(m_cap, C, 2, 0);
}

extern "C" int ldn_rows_bn_stats(const float* u, int ldu, const float* chan_mask, const int32_t* row_prefix, int B, const int32_t* m_count,
                                 int m_cap, int C, float eps, float* mean, float* var, float* invstd, float* work, void* stream) {
    LDN_REQUIRE(u && mean && var && invstd && work, "ldn_rows_bn_stats: null pointer");
    LDN_REQUIRE(m_cap >= 0 && C > 0 && C % 4 == 0 && ldu >= C && ldu % 4 == 0,
                "ldn_rows_bn_stats: m_cap >= 0, C %% 4 == 0, ldu >= C, ldu %% 4 == 0 (got %d, %d, %d)", m_cap, C, ldu);
    LDN_REQUIRE(eps >= 0.f, "ldn_rows_bn_stats: eps >= 0 (got %g)", (double)eps);
    LDN_REQUIRE(!chan_mask || (row_prefix && B >= 1), "ldn_rows_bn_stats: chan_mask needs row_prefix [B + 1] and B >= 1");
    LDN_REQUIRE(aligned16(u) && aligned16(chan_mask) && aligned16(mean) && aligned16(var) && aligned16(invstd) && aligned16(work),
                "ldn_rows_bn_stats: every float pointer must be 16-byte aligned");
    BnStatArgs p;
    p.u = u; p.chan_mask = chan_mask; p.prefix = row_prefix; p.m_count = m_count; p.mean = mean; p.var = var; p.invstd = invstd; p.work = work;
    p.eps = eps; p.ldu = ldu; p.B = chan_mask ? B : 0; p.m_cap = m_cap; p.C = C;
    const dim3 grid = rows_grid(m_cap, C, &p.splits, &p.rps);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (m_cap > 0) {
        k_bn_stats_partial<<<grid, ACT_THREADS, 0, st>>>(p);
        LDN_CHECK_LAUNCH("k_bn_stats_partial");
    }
    k_bn_stats_reduce<<<ceil_div(C / 4, 256), 256, 0, st>>>(p);
    LDN_CHECK_LAUNCH("k_bn_stats_reduce");
    return LDN_OK;
}

extern "C" int ldn_rows_bn_fwd(const float* u, int ldu, const float* mean, const float* invstd, const float* gamma, const float* beta,
                               const float* chan_mask, const int32_t* row_prefix, int B, const float* row_scale, int relu,
                               const int32_t* m_count, int m_cap, int C, float* h, int ldh, void* stream) {
    LDN_REQUIRE(u && mean && invstd && gamma && beta && h, "ldn_rows_bn_fwd: null pointer");
    LDN_REQUIRE(m_cap >= 0 && C > 0 && C % 4 == 0, "ldn_rows_bn_fwd: m_cap >= 0, C %% 4 == 0 (got %d, %d)", m_cap, C);
    LDN_REQUIRE(ldu >= C && ldh >= C && ldu % 4 == 0 && ldh % 4 == 0, "ldn_rows_bn_fwd: leading dimensions >= C and multiples of 4 (got %d, %d)", ldu, ldh);
    LDN_REQUIRE(!chan_mask || (row_prefix && B >= 1), "ldn_rows_bn_fwd: chan_mask needs row_prefix [B + 1] and B >= 1");
    LDN_REQUIRE(aligned16(u) && aligned16(mean) && aligned16(invstd) && aligned16(gamma) && aligned16(beta) && aligned16(chan_mask) && aligned16(h),
                "ldn_rows_bn_fwd: every float pointer except row_scale must be 16-byte aligned");
    if (m_cap == 0) return LDN_OK;
    const size_t n = (size_t)m_cap * (C / 4);
    LDN_REQUIRE((n + 255) / 256 <= 0x7fffffffull, "ldn_rows_bn_fwd: m_cap * C too large");
    BnFwdArgs p;
    p.u = u; p.mean = mean; p.invstd = invstd; p.gamma = gamma; p.beta = beta; p.chan_mask = chan_mask; p.prefix = row_prefix;
    p.row_scale = row_scale; p.m_count = m_count; p.h = h; p.ldu = ldu; p.ldh = ldh; p.B = chan_mask ? B : 0; p.m_cap = m_cap; p.C = C;
    p.relu = relu != 0;
    k_rows_bn_fwd<<<(unsigned)((n + 255) / 256), 256, 0, static_cast<hipStream_t>(stream)>>>(p);
    LDN_CHECK_LAUNCH("k_rows_bn_fwd");
    return LDN_OK;
}

extern "C" size_t ldn_rows_bn_bwd_workspace_bytes(int m_cap, int C, int B) { return rows_bwd_work_bytes(m_cap, C, B); }

extern "C" int ldn_rows_bn_bwd(const float* dh, int lddh, const float* u, int ldu, const float* h, int ldh, const float* mean,
                               const float* invstd, const float* gamma, const float* chan_mask, const int32_t* row_prefix, int B,
                               const float* row_scale, const int32_t* m_count, int m_cap, int C, float* du, int lddu, float* d_gamma,
                               float* d_beta, float* g_mask, float* work, void* stream) {
    LDN_REQUIRE(dh && u && mean && invstd && gamma && du && d_gamma && d_beta && work, "ldn_rows_bn_bwd: null pointer");
    LDN_REQUIRE(m_cap >= 0 && C > 0 && C % 4 == 0, "ldn_rows_bn_bwd: m_cap >= 0, C %% 4 == 0 (got %d, %d)", m_cap, C);
    LDN_REQUIRE(lddh >= C && ldu >= C && lddu >= C && lddh % 4 == 0 && ldu % 4 == 0 && lddu % 4 == 0,
                "ldn_rows_bn_bwd: leading dimensions >= C and multiples of 4 (got %d, %d, %d)", lddh, ldu, lddu);
    LDN_REQUIRE(!h || (ldh >= C && ldh % 4 == 0), "ldn_rows_bn_bwd: ldh >= C and a multiple of 4 (got %d)", ldh);
    LDN_REQUIRE(!(chan_mask || g_mask) || (row_prefix && B >= 1), "ldn_rows_bn_bwd: chan_mask / g_mask need row_prefix [B + 1] and B >= 1");
    LDN_REQUIRE(aligned16(dh) && aligned16(u) && aligned16(h) && aligned16(mean) && aligned16(invstd) && aligned16(gamma) && aligned16(chan_mask) &&
                aligned16(du) && aligned16(d_gamma) && aligned16(d_beta) && aligned16(g_mask) && aligned16(work),
                "ldn_rows_bn_bwd: every float pointer except row_scale must be 16-byte aligned");
    BnBwdArgs p;
    p.dh = dh; p.u = u; p.h = h; p.mean = mean; p.invstd = invstd; p.gamma = gamma; p.chan_mask = chan_mask; p.prefix = row_prefix;
    p.row_scale = row_scale; p.m_count = m_count; p.du = du; p.d_gamma = d_gamma; p.d_beta = d_beta; p.g_mask = g_mask; p.work = work;
    p.lddh = lddh; p.ldu = ldu; p.ldh = ldh; p.lddu = lddu; p.B = (chan_mask || g_mask) ? B : 0; p.m_cap = m_cap; p.C = C;
    const dim3 grid = rows_grid(m_cap, C, &p.splits, &p.rps);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (m_cap > 0) {
        k_bn_bwd_partial<<<grid, ACT_THREADS, 0, st>>>(p);
        LDN_CHECK_LAUNCH("k_bn_bwd_partial");
    }
    const int rc = rows_reduce({work, nullptr, nullptr, m_count, {d_beta, d_gamma}, nullptr, 2, 0, 0, m_cap, C, p.splits, p.rps}, st);
    if (rc != LDN_OK) return rc;
    if (m_cap > 0) {
        k_bn_bwd_final<<<grid, ACT_THREADS, 0, st>>>(p);
        LDN_CHECK_LAUNCH("k_bn_bwd_final");
    }
    if (g_mask) return rows_reduce({nullptr, work_slot(work, p.splits, C, 2, 0), row_prefix, m_count, {nullptr, nullptr}, g_mask, 0, B, B, m_cap, C, p.splits, p.rps}, st);
    return LDN_OK;
}

extern "C" int ldn_rows_bn_postmask_fwd(const float* u, int ldu, const float* mean, const float* invstd, const float* gamma, const float* beta,
                                        const float* chan_mask, const int32_t* row_prefix, int B, const int32_t* m_count, int m_cap, int C,
                                        float* h, int ldh, void* stream) {
    LDN_REQUIRE(u && mean && invstd && gamma && beta && h, "ldn_rows_bn_postmask_fwd: null pointer");
    LDN_REQUIRE(m_cap >= 0 && C > 0 && C % 4 == 0, "ldn_rows_bn_postmask_fwd: m_cap >= 0, C %% 4 == 0 (got %d, %d)", m_cap, C);
    LDN_REQUIRE(ldu >= C && ldh >= C && ldu % 4 == 0 && ldh % 4 == 0,
                "ldn_rows_bn_postmask_fwd: leading dimensions >= C and multiples of 4 (got %d, %d)", ldu, ldh);
    LDN_REQUIRE(!chan_mask || (row_prefix && B >= 1), "ldn_rows_bn_postmask_fwd: chan_mask needs row_prefix [B + 1] and B >= 1");
    LDN_REQUIRE(aligned16(u) && aligned16(mean) && aligned16(invstd) && aligned16(gamma) && aligned16(beta) && aligned16(chan_mask) && aligned16(h),
                "ldn_rows_bn_postmask_fwd: every float pointer must be 16-byte aligned");
    if (m_cap == 0) return LDN_OK;
    const size_t n = (size_t)m_cap * (C / 4);
    LDN_REQUIRE((n + 255) / 256 <= 0x7fffffffull, "ldn_rows_bn_postmask_fwd: m_cap * C too large");
    BnPmFwdArgs p;
    p.u = u; p.mean = mean; p.invstd = invstd; p.gamma = gamma; p.beta = beta; p.chan_mask = chan_mask; p.prefix = row_prefix;
    p.m_count = m_count; p.h = h; p.ldu = ldu; p.ldh = ldh; p.B = chan_mask ? B : 0; p.m_cap = m_cap; p.C = C;
    k_rows_bn_postmask_fwd<<<(unsigned)((n + 255) / 256), 256, 0, static_cast<hipStream_t>(stream)>>>(p);
    LDN_CHECK_LAUNCH("k_rows_bn_postmask_fwd");
    return LDN_OK;
}

extern "C" size_t ldn_rows_bn_postmask_bwd_workspace_bytes(int m_cap, int C, int B) { return rows_bwd_work_bytes(m_cap, C, B); }

extern "C" int ldn_rows_bn_postmask_bwd(const float* dz, int lddz, const float* u, int ldu, const float* h, int ldh, const float* mean,
                                        const float* invstd, const float* gamma, const float* beta, const float* chan_mask,
                                        const int32_t* row_prefix, int B, const float* gate, const float* dsq, const int32_t* m_count, int m_cap,
                                        int C, float* du, int lddu, float* d_gamma, float* d_beta, float* g_mask, float* work, void* stream) {
    LDN_REQUIRE(dz && u && h && mean && invstd && gamma && beta && du && d_gamma && d_beta && work, "ldn_rows_bn_postmask_bwd: null pointer");
    LDN_REQUIRE(m_cap >= 0 && C > 0 && C % 4 == 0, "ldn_rows_bn_postmask_bwd: m_cap >= 0, C %% 4 == 0 (got %d, %d)", m_cap, C);
    LDN_REQUIRE(lddz >= C && ldu >= C && ldh >= C && lddu >= C && lddz % 4 == 0 && ldu % 4 == 0 && ldh % 4 == 0 && lddu % 4 == 0,
                "ldn_rows_bn_postmask_bwd: leading dimensions >= C and multiples of 4 (got %d, %d, %d, %d)", lddz, ldu, ldh, lddu);
    LDN_REQUIRE((gate != nullptr) == (dsq != nullptr), "ldn_rows_bn_postmask_bwd: gate and dsq [B][C] are the SE prologue: give both or neither");
    const bool per_image = chan_mask || gate || g_mask;
    LDN_REQUIRE(!per_image || (row_prefix && B >= 1), "ldn_rows_bn_postmask_bwd: chan_mask / gate / g_mask need row_prefix [B + 1] and B >= 1");
    LDN_REQUIRE(aligned16(dz) && aligned16(u) && aligned16(h) && aligned16(mean) && aligned16(invstd) && aligned16(gamma) && aligned16(beta) &&
                aligned16(chan_mask) && aligned16(gate) && aligned16(dsq) && aligned16(du) && aligned16(d_gamma) && aligned16(d_beta) &&
                aligned16(g_mask) && aligned16(work), "ldn_rows_bn_postmask_bwd: every float pointer must be 16-byte aligned");
    BnPmBwdArgs p;
    p.dz = dz; p.u = u; p.h = h; p.mean = mean; p.invstd = invstd; p.gamma = gamma; p.beta = beta; p.chan_mask = chan_mask;
    p.prefix = row_prefix; p.gate = gate; p.dsq = dsq; p.m_count = m_count; p.du = du; p.d_gamma = d_gamma; p.d_beta = d_beta; p.g_mask = g_mask;
    p.work = work; p.lddz = lddz; p.ldu = ldu; p.ldh = ldh; p.lddu = lddu; p.B = per_image ? B : 0; p.m_cap = m_cap; p.C = C;
    const dim3 grid = rows_grid(m_cap, C, &p.splits, &p.rps);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (m_cap > 0) {
        k_bn_pm_bwd_partial<<<grid, ACT_THREADS, 0, st>>>(p);
        LDN_CHECK_LAUNCH("k_bn_pm_bwd_partial");
    }
    const int rc = rows_reduce({work, work_slot(work, p.splits, C, 2, 0), row_prefix, m_count, {d_beta, d_gamma}, g_mask, 2, g_mask ? B : 0, B, m_cap, C,
                                p.splits, p.rps}, st);
    if (rc != LDN_OK) return rc;
    if (m_cap > 0) {
        k_bn_pm_bwd_final<<<grid, ACT_THREADS, 0, st>>>(p);
        LDN_CHECK_LAUNCH("k_bn_pm_bwd_final");
    }
    return LDN_OK;
}
