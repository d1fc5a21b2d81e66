// ldn_train_bn.hip -- BatchNorm on BATCH statistics over packed rows, forward and backward (ldn_rows_bn_stats, ldn_rows_bn_fwd, ldn_rows_bn_bwd;
// include/ldn_hip.h): what training needs of the reference's own recipe, where bn1 / bn2 / bn3 normalise with the statistics of the batch.
//
// Bandwidth-bound row kernels with the conventions of ldn_train_rows.hip (ldn_rows_plan.h): [m_cap, C] fp32 matrices with a leading dimension,
// C % 4 == 0, every access 16 bytes wide; the count is read on the device, rows r >= count are never read and are written as exact zeros; the
// rows are split over `splits` workgroups per 256-channel column tile by act_plan -- a function of (m_cap, C) only, so every launch is
// graph-capturable; inside a workgroup a thread owns one channel quad and every RL-th row, the row lanes are combined in ascending lane order
// through the LDS, the workgroups' partials in ascending split order by a second small launch.  No floating-point atomics: two runs are
// bit-identical.  fp32 arithmetic whatever the math mode of the convolutions around them.
//
// The optional channel mask c [B][C] multiplies u BEFORE the statistics and the normalisation (the reference's apply_channel_mask in front of
// bn1 / bn2): x = c[img(r)][k] * u[r][k], a channel dropped in one image contributes zeros to the batch statistics.  u itself is the UNMASKED
// convolution output -- the backward needs it for the mask's straight-through term.  The image of a row comes from the per-image row prefix,
// by a walk over the images of a workgroup's rows (statistics, backward) or a binary search per thread (forward).
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
// and, where the mask's straight-through gradient is wanted, g_mask[b][k] = sum over the rows of image b of g * u -- FUSED into launch 3 with the
// (split + b) slots of ldn_rows_act_bwd and one more small launch that adds them: four launches, against six for the same through
// ldn_rows_img_dot (two) and ldn_rows_chanmask (one) behind a three-launch backward.
#include "ldn_rows_plan.h"

namespace ldn {

// thread = (row lane rl, quad ql) of a QT-quad column tile, QT = min(C / 4, 64), RL = 256 / QT row lanes; grid = (column tiles, splits)
struct RowWalk {
    int QT, RL, rl, ql, k, split, count, r_begin, r_cap_end, r_end;
    bool active;
};

__device__ __forceinline__ RowWalk row_walk(int C, const int32_t* m_count, int m_cap, int rps) {
    RowWalk w;
    const int Q = C >> 2;
    w.QT = Q < ACT_QT ? Q : ACT_QT;
    w.RL = ACT_THREADS / w.QT;
    w.rl = threadIdx.x / w.QT;
    w.ql = threadIdx.x - w.rl * w.QT;
    const int q = blockIdx.x * ACT_QT + w.ql;
    w.active = w.rl < w.RL && q < Q;
    w.k = 4 * q;
    w.split = blockIdx.y;
    w.count = rows_count(m_count, m_cap);
    w.r_begin = w.split * rps;
    w.r_cap_end = min(m_cap, w.r_begin + rps);
    w.r_end = min(w.count, w.r_cap_end);
    return w;
}

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }

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

// work layout of ldn_rows_bn_stats: [splits][C] mean partials | [splits][C] M2 partials
__global__ __launch_bounds__(ACT_THREADS) void k_bn_stats_partial(const BnStatArgs p) {
    __shared__ f32x4 s_mean[ACT_THREADS], s_m2[ACT_THREADS];
    __shared__ int s_n[ACT_THREADS];
    const RowWalk w = row_walk(p.C, p.m_count, p.m_cap, p.rps);
    if (w.r_begin >= w.r_end) return;      // (uniform) no rows: k_bn_stats_reduce does not read this split's partials
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 mean = zero, m2 = zero;
    int n = 0;
    int b = p.chan_mask ? image_of_row(p.prefix, p.B, w.r_begin) : 0;
    int r0 = w.r_begin;
    while (r0 < w.r_end) {                 // (uniform) one segment per image that owns rows of this split
        int seg_end = w.r_end;
        if (p.chan_mask && b < p.B - 1) seg_end = min(w.r_end, max(p.prefix[b + 1], r0));
        if (seg_end > r0 && w.active) {
            f32x4 m = {1.f, 1.f, 1.f, 1.f};
            if (p.chan_mask) m = ld4(p.chan_mask + (size_t)b * p.C + w.k);
            for (int r = r0 + w.rl; r < seg_end; r += w.RL) {
                const f32x4 x = ld4(p.u + (size_t)r * p.ldu + w.k) * m;
                ++n;
                const f32x4 d = x - mean;
                mean += d * (1.f / (float)n);
                m2 += d * (x - mean);
            }
        }
        r0 = seg_end;
        ++b;
    }
    s_mean[threadIdx.x] = mean;
    s_m2[threadIdx.x] = m2;
    s_n[threadIdx.x] = n;
    __syncthreads();
    if (w.active && w.rl == 0) {           // the row lanes in ascending lane order
        f32x4 ma = zero, m2a = zero;
        int na = 0;
        for (int j = 0; j < w.RL; ++j) {
            const int i = j * w.QT + w.ql;
            if (s_n[i] > 0) chan_merge(na, ma, m2a, s_n[i], s_mean[i], s_m2[i]);
        }
        *reinterpret_cast<f32x4*>(p.work + (size_t)w.split * p.C + w.k) = ma;
        *reinterpret_cast<f32x4*>(p.work + (size_t)(p.splits + w.split) * p.C + w.k) = m2a;
    }
}

// one thread per quad: the splits that hold rows in ascending order; a split's n follows from the count
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
        chan_merge(na, ma, m2a, nb, ld4(p.work + (size_t)t * p.C + k), ld4(p.work + (size_t)(p.splits + t) * p.C + k));
    }
    const f32x4 var = na > 0 ? m2a * (1.f / (float)na) : m2a;
    f32x4 inv;
#pragma unroll
    for (int e = 0; e < 4; ++e) inv[e] = 1.f / sqrtf(var[e] + p.eps);
    *reinterpret_cast<f32x4*>(p.mean + k) = ma;
    *reinterpret_cast<f32x4*>(p.var + k) = var;
    *reinterpret_cast<f32x4*>(p.invstd + k) = inv;
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

// work layout of ldn_rows_bn_bwd: [splits][C] d_beta partials | [splits][C] d_gamma partials | [splits + B][C] g_mask slots
__device__ __forceinline__ float* bn_work_mask(const BnBwdArgs& p) { return p.work + (size_t)2 * p.splits * p.C; }

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

// launch 1: the partial d_beta / d_gamma of the split
__global__ __launch_bounds__(ACT_THREADS) void k_bn_bwd_partial(const BnBwdArgs p) {
    __shared__ f32x4 s_red[2][ACT_THREADS];
    const RowWalk w = row_walk(p.C, p.m_count, p.m_cap, p.rps);
    if (w.r_begin >= w.r_end) return;      // (uniform) no rows: k_bn_bwd_reduce does not read this split's partials
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 mean = zero, inv = zero, g_b = zero, g_g = zero;
    if (w.active) {
        mean = ld4(p.mean + w.k);
        inv = ld4(p.invstd + w.k);
    }
    int b = p.chan_mask ? image_of_row(p.prefix, p.B, w.r_begin) : 0;
    int r0 = w.r_begin;
    while (r0 < w.r_end) {                 // (uniform) one segment per image that owns rows of this split
        int seg_end = w.r_end;
        if (p.chan_mask && b < p.B - 1) seg_end = min(w.r_end, max(p.prefix[b + 1], r0));
        if (seg_end > r0 && w.active) {
            f32x4 m = {1.f, 1.f, 1.f, 1.f};
            if (p.chan_mask) m = ld4(p.chan_mask + (size_t)b * p.C + w.k);
            for (int r = r0 + w.rl; r < seg_end; r += w.RL) {
                f32x4 u, xhat, dz;
                bn_bwd_quad(p, r, w.k, m, mean, inv, u, xhat, dz);
                g_b += dz;
                g_g += dz * xhat;
            }
        }
        r0 = seg_end;
        ++b;
    }
    s_red[0][threadIdx.x] = g_b;
    s_red[1][threadIdx.x] = g_g;
    __syncthreads();
    if (w.active && w.rl == 0) {           // the row lanes in ascending lane order
        f32x4 sb = zero, sg = zero;
        for (int j = 0; j < w.RL; ++j) {
            sb += s_red[0][j * w.QT + w.ql];
            sg += s_red[1][j * w.QT + w.ql];
        }
        *reinterpret_cast<f32x4*>(p.work + (size_t)w.split * p.C + w.k) = sb;
        *reinterpret_cast<f32x4*>(p.work + (size_t)(p.splits + w.split) * p.C + w.k) = sg;
    }
}

// launch 2: one thread per quad of d_beta (j == 0) and d_gamma (j == 1), the partials in ascending split order
__global__ __launch_bounds__(256) void k_bn_bwd_reduce(const BnBwdArgs p) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int Q = p.C >> 2;
    if (i >= 2 * Q) return;
    const int j = i / Q, k = 4 * (i - j * Q);
    const int live = min(p.splits, ceil_div(rows_count(p.m_count, p.m_cap), p.rps));
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    for (int t = 0; t < live; ++t) s += ld4(p.work + (size_t)(j * p.splits + t) * p.C + k);
    *reinterpret_cast<f32x4*>((j == 0 ? p.d_beta : p.d_gamma) + k) = s;
}

// launch 3: du, and the partial g_mask of every image that owns rows of the split
__global__ __launch_bounds__(ACT_THREADS) void k_bn_bwd_final(const BnBwdArgs p) {
    __shared__ f32x4 s_red[ACT_THREADS];
    const RowWalk w = row_walk(p.C, p.m_count, p.m_cap, p.rps);
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    // rows past the count: exact zeros, nothing read
    if (w.active)
        for (int r = max(w.r_end, w.r_begin) + w.rl; r < w.r_cap_end; r += w.RL) store16(p.du + (size_t)r * p.lddu + w.k, zero);
    if (w.r_begin >= w.r_end) return;      // (uniform) no rows: k_bn_mask_reduce does not read this split's slots
    f32x4 mean = zero, inv = zero, gi = zero, cb = zero, cg = zero;
    if (w.active) {
        const float inv_n = 1.f / (float)w.count;          // (count >= r_end > 0)
        mean = ld4(p.mean + w.k);
        inv = ld4(p.invstd + w.k);
        gi = ld4(p.gamma + w.k) * inv;
        cb = ld4(p.d_beta + w.k) * inv_n;
        cg = ld4(p.d_gamma + w.k) * inv_n;
    }
    const bool per_image = p.chan_mask || p.g_mask;
    int b = per_image ? image_of_row(p.prefix, p.B, w.r_begin) : 0;
    int r0 = w.r_begin;
    while (r0 < w.r_end) {                 // (uniform) one segment per image that owns rows of this split
        int seg_end = w.r_end;
        if (per_image && b < p.B - 1) seg_end = min(w.r_end, max(p.prefix[b + 1], r0));
        if (seg_end > r0) {
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
            if (p.g_mask) {                // the row lanes in ascending lane order
                s_red[threadIdx.x] = g_m;
                __syncthreads();
                if (w.active && w.rl == 0) {
                    f32x4 s = zero;
                    for (int j = 0; j < w.RL; ++j) s += s_red[j * w.QT + w.ql];
                    *reinterpret_cast<f32x4*>(bn_work_mask(p) + (size_t)(w.split + b) * p.C + w.k) = s;
                }
                __syncthreads();
            }
        }
        r0 = seg_end;
        ++b;
    }
}

// launch 4 (with g_mask only): one thread per quad of g_mask[b]
__global__ __launch_bounds__(256) void k_bn_mask_reduce(const BnBwdArgs p) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int Q = p.C >> 2;
    if (i >= p.B * Q) return;
    const int b = i / Q, k = 4 * (i - b * Q);
    *reinterpret_cast<f32x4*>(p.g_mask + (size_t)b * p.C + k) =
        image_slots_sum(bn_work_mask(p), p.prefix, p.B, b, rows_count(p.m_count, p.m_cap), p.splits, p.rps, p.C, k);
}

}  // namespace ldn

using namespace ldn;

extern "C" size_t ldn_rows_bn_stats_workspace_bytes(int m_cap, int C) {
    if (m_cap < 0 || C <= 0 || C % 4) return 0;
    int tiles, splits, rps;
    act_plan(m_cap, C, &tiles, &splits, &rps);
    return (size_t)2 * splits * C * sizeof(float);
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
    int tiles;
    act_plan(m_cap, C, &tiles, &p.splits, &p.rps);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (m_cap > 0) {
        k_bn_stats_partial<<<dim3((unsigned)tiles, (unsigned)p.splits), ACT_THREADS, 0, st>>>(p);
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

extern "C" size_t ldn_rows_bn_bwd_workspace_bytes(int m_cap, int C, int B) {
    if (m_cap < 0 || C <= 0 || C % 4 || B < 0) return 0;
    int tiles, splits, rps;
    act_plan(m_cap, C, &tiles, &splits, &rps);
    return ((size_t)2 * splits + (B > 0 ? splits + B : 0)) * C * sizeof(float);
}

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
    int tiles;
    act_plan(m_cap, C, &tiles, &p.splits, &p.rps);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)tiles, (unsigned)p.splits);
    if (m_cap > 0) {
        k_bn_bwd_partial<<<grid, ACT_THREADS, 0, st>>>(p);
        LDN_CHECK_LAUNCH("k_bn_bwd_partial");
    }
    k_bn_bwd_reduce<<<ceil_div(2 * (C / 4), 256), 256, 0, st>>>(p);
    LDN_CHECK_LAUNCH("k_bn_bwd_reduce");
    if (m_cap > 0) {
        k_bn_bwd_final<<<grid, ACT_THREADS, 0, st>>>(p);
        LDN_CHECK_LAUNCH("k_bn_bwd_final");
    }
    if (g_mask) {
        k_bn_mask_reduce<<<ceil_div(B * (C / 4), 256), 256, 0, st>>>(p);
        LDN_CHECK_LAUNCH("k_bn_mask_reduce");
    }
    return LDN_OK;
}
