// ldn_train_rows.hip -- the elementwise backward chain of training on packed rows (ldn_rows_chanmask, ldn_rows_act_bwd, ldn_rows_postmask_bwd,
// ldn_rows_img_dot; include/ldn_hip.h), and the LayerNorm backward on listed rows (ldn_rows_ln_bwd, further down with its own notes).
//
// The first four are bandwidth-bound row kernels over [m_cap, C] fp32 matrices with a leading dimension: C % 4 == 0, every access 16 bytes wide, a wave
// reads consecutive quads of a row.  The count is read on the device; rows r >= count are never read and are written as exact zeros.
//
// The image of a packed row comes from the per-image row prefix ([B + 1]: image b owns rows [prefix[b], prefix[b + 1])) inside the kernel --
// a binary search per thread (ldn_rows_chanmask) or per workgroup, followed by a walk over the images of the workgroup's rows
// (ldn_rows_act_bwd).  There is no [m_cap] image-id tensor and no host read.
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
//
// Determinism: the rows are split over `splits` workgroups per column tile -- a function of m_cap and C only, never of the device-side count
// (the launch is graph-capturable).  Inside a workgroup a thread owns one channel quad and every RL-th row; the row lanes' sums are added in
// ascending lane order through the LDS.  A workgroup writes its partial g_shift / g_scale_num to work[split], and the partial g_mask of
// every image b that owns rows of the split to the slot split + b: an image's rows may straddle splits, and because images and splits both
// ascend along the rows, (split, b) -> split + b is one-to-one over the pairs that meet (splits + B slots instead of splits * B).
// k_act_reduce adds the partials in ascending split order.  No floating-point atomics.
//
// ldn_rows_postmask_bwd is the same walk for a mask applied AFTER the ReLU (LAD-RegNet: h = m * relu(zy), the UNMASKED r = relu(zy) stored), with
// an optional squeeze-excitation prologue on the incoming gradient; per element of a row r < count of image b:
//     dh = gate ? fma(dz, gate[b, k], dsq[b, k]) : dz          (one rounding)
//     a  = r > 0 ? dh * m[b, k] : 0
//     du = a * s[k]
//     g_shift[k]     += a
//     g_scale_num[k] += a * (r - t[k])
//     g_mask[b, k]   += dh * r              (every channel: non-zero exactly where the activation is on, masked channels included)
// ldn_rows_img_dot is its per-image reduction alone: out[b, k] = sum over the rows of image b of a[r, k] * b[r, k].  Both use act_plan and the
// (split + b) slots of ldn_rows_act_bwd.
#include "ldn_rows_plan.h"      // thread-layout constants, rows_count, image_of_row, act_plan, aligned16

namespace ldn {

struct ActArgs {
    const float* dh; const float* u; const float* post_sub; const float* scale; const float* shift; const float* chan_mask;
    const int32_t* prefix; const float* zy; const int32_t* m_count;
    float* du; float* g_shift; float* g_scale; float* g_mask; float* work;
    int lddh, ldu, ldzy, lddu, B, m_cap, C, splits, rps;
};

// work layout: [splits][C] g_shift partials | [splits][C] g_scale_num partials | [splits + B][C] g_mask partials
__device__ __forceinline__ float* act_work_shift(const ActArgs& p) { return p.work; }
__device__ __forceinline__ float* act_work_scale(const ActArgs& p) { return p.work + (size_t)p.splits * p.C; }
__device__ __forceinline__ float* act_work_mask(const ActArgs& p) { return p.work + (size_t)2 * p.splits * p.C; }

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

// grid = (column tiles, splits); thread = (row lane rl, quad ql) of a QT-quad tile, QT = min(C / 4, 64), RL = 256 / QT row lanes
__global__ __launch_bounds__(ACT_THREADS) void k_rows_act_bwd(const ActArgs p) {
    __shared__ f32x4 s_red[ACT_THREADS];
    const int Q = p.C >> 2;
    const int QT = Q < ACT_QT ? Q : ACT_QT;
    const int RL = ACT_THREADS / QT;
    const int tid = threadIdx.x, rl = tid / QT, ql = tid - rl * QT;
    const int q = blockIdx.x * ACT_QT + ql;
    const bool active = rl < RL && q < Q;
    const int split = blockIdx.y;
    const int count = rows_count(p.m_count, p.m_cap);
    const int r_begin = split * p.rps;
    const int r_cap_end = min(p.m_cap, r_begin + p.rps);
    const int r_end = min(count, r_cap_end);
    const int k = 4 * q;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};

    // rows past the count: exact zeros, nothing read
    if (active)
        for (int r = max(r_end, r_begin) + rl; r < r_cap_end; r += RL) store16(p.du + (size_t)r * p.lddu + k, zero);
    if (r_begin >= r_end) return;          // (uniform) no rows: k_act_reduce does not read this split's partials

    // lane-order sum over the row lanes; the result is valid in row lane 0
    auto lane_sum = [&](f32x4 v) {
        s_red[tid] = v;
        __syncthreads();
        f32x4 s = zero;
        if (rl == 0)
            for (int j = 0; j < RL; ++j) s += s_red[j * QT + ql];
        __syncthreads();
        return s;
    };

    f32x4 sc = zero, sh = zero, c = zero;
    if (active) {
        sc = *reinterpret_cast<const f32x4*>(p.scale + k);
        sh = *reinterpret_cast<const f32x4*>(p.shift + k);
        if (p.post_sub) c = *reinterpret_cast<const f32x4*>(p.post_sub + k);
    }
    const bool per_image = p.chan_mask || p.zy;
    int b = per_image ? image_of_row(p.prefix, p.B, r_begin) : 0;
    f32x4 g_sh = zero, g_sc = zero;
    int r0 = r_begin;
    while (r0 < r_end) {                   // (uniform) one segment per image that owns rows of this split
        int seg_end = r_end;
        if (per_image && b < p.B - 1) seg_end = min(r_end, max(p.prefix[b + 1], r0));
        if (seg_end > r0) {
            f32x4 m = {1.f, 1.f, 1.f, 1.f}, g_m = zero;
            if (active && p.chan_mask) m = *reinterpret_cast<const f32x4*>(p.chan_mask + (size_t)b * p.C + k);
            if (active)
                for (int r = r0 + rl; r < seg_end; r += RL) {
                    const f32x4 dh = *reinterpret_cast<const f32x4*>(p.dh + (size_t)r * p.lddh + k);
                    const f32x4 u = *reinterpret_cast<const f32x4*>(p.u + (size_t)r * p.ldu + k);
                    f32x4 zy = zero;
                    if (p.zy) zy = *reinterpret_cast<const f32x4*>(p.zy + (size_t)r * p.ldzy + k);
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
                    store16(p.du + (size_t)r * p.lddu + k, du);
                }
            if (p.zy) {
                const f32x4 s = lane_sum(g_m);
                if (active && rl == 0) *reinterpret_cast<f32x4*>(act_work_mask(p) + (size_t)(split + b) * p.C + k) = s;
            }
        }
        r0 = seg_end;
        ++b;
    }
    const f32x4 s1 = lane_sum(g_sh), s2 = lane_sum(g_sc);
    if (active && rl == 0) {
        *reinterpret_cast<f32x4*>(act_work_shift(p) + (size_t)split * p.C + k) = s1;
        *reinterpret_cast<f32x4*>(act_work_scale(p) + (size_t)split * p.C + k) = s2;
    }
}

// one thread per quad of g_shift (j == 0), g_scale_num (j == 1) and g_mask[b] (j == 2 + b): the partials in ascending split order
__global__ __launch_bounds__(256) void k_act_reduce(const ActArgs p, int nvec) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int Q = p.C >> 2;
    if (i >= nvec * Q) return;
    const int j = i / Q, k = 4 * (i - j * Q);
    const int count = rows_count(p.m_count, p.m_cap);
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    if (j < 2) {
        const int live = min(p.splits, ceil_div(count, p.rps));
        const float* w = j == 0 ? act_work_shift(p) : act_work_scale(p);
        for (int t = 0; t < live; ++t) s += *reinterpret_cast<const f32x4*>(w + (size_t)t * p.C + k);
        *reinterpret_cast<f32x4*>((j == 0 ? p.g_shift : p.g_scale) + k) = s;
        return;
    }
    const int b = j - 2;
    *reinterpret_cast<f32x4*>(p.g_mask + (size_t)b * p.C + k) = image_slots_sum(act_work_mask(p), p.prefix, p.B, b, count, p.splits, p.rps, p.C, k);
}

struct PmArgs {
    const float* dz; const float* r; const float* scale; const float* shift; const float* chan_mask; const int32_t* prefix;
    const float* gate; const float* dsq; const int32_t* m_count;
    float* du; float* g_shift; float* g_scale; float* g_mask; float* work;
    int lddz, ldr, lddu, B, m_cap, C, splits, rps;
};

// work layout of ldn_rows_postmask_bwd: that of ldn_rows_act_bwd
__device__ __forceinline__ float* pm_work_shift(const PmArgs& p) { return p.work; }
__device__ __forceinline__ float* pm_work_scale(const PmArgs& p) { return p.work + (size_t)p.splits * p.C; }
__device__ __forceinline__ float* pm_work_mask(const PmArgs& p) { return p.work + (size_t)2 * p.splits * p.C; }

// grid, threads and row walk of k_rows_act_bwd
__global__ __launch_bounds__(ACT_THREADS) void k_rows_postmask_bwd(const PmArgs p) {
    __shared__ f32x4 s_red[ACT_THREADS];
    const int Q = p.C >> 2;
    const int QT = Q < ACT_QT ? Q : ACT_QT;
    const int RL = ACT_THREADS / QT;
    const int tid = threadIdx.x, rl = tid / QT, ql = tid - rl * QT;
    const int q = blockIdx.x * ACT_QT + ql;
    const bool active = rl < RL && q < Q;
    const int split = blockIdx.y;
    const int count = rows_count(p.m_count, p.m_cap);
    const int r_begin = split * p.rps;
    const int r_cap_end = min(p.m_cap, r_begin + p.rps);
    const int r_end = min(count, r_cap_end);
    const int k = 4 * q;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};

    // rows past the count: exact zeros, nothing read
    if (active)
        for (int r = max(r_end, r_begin) + rl; r < r_cap_end; r += RL) store16(p.du + (size_t)r * p.lddu + k, zero);
    if (r_begin >= r_end) return;          // (uniform) no rows: k_postmask_reduce does not read this split's partials

    auto lane_sum = [&](f32x4 v) {         // lane-order sum over the row lanes; the result is valid in row lane 0
        s_red[tid] = v;
        __syncthreads();
        f32x4 s = zero;
        if (rl == 0)
            for (int j = 0; j < RL; ++j) s += s_red[j * QT + ql];
        __syncthreads();
        return s;
    };

    f32x4 sc = zero, sh = zero;
    if (active) {
        sc = *reinterpret_cast<const f32x4*>(p.scale + k);
        sh = *reinterpret_cast<const f32x4*>(p.shift + k);
    }
    const bool per_image = p.B > 0;        // chan_mask, the SE prologue or g_mask
    int b = per_image ? image_of_row(p.prefix, p.B, r_begin) : 0;
    f32x4 g_sh = zero, g_sc = zero;
    int r0 = r_begin;
    while (r0 < r_end) {                   // (uniform) one segment per image that owns rows of this split
        int seg_end = r_end;
        if (per_image && b < p.B - 1) seg_end = min(r_end, max(p.prefix[b + 1], r0));
        if (seg_end > r0) {
            f32x4 m = {1.f, 1.f, 1.f, 1.f}, ga = zero, dq = zero, g_m = zero;
            if (active && p.chan_mask) m = *reinterpret_cast<const f32x4*>(p.chan_mask + (size_t)b * p.C + k);
            if (active && p.gate) {
                ga = *reinterpret_cast<const f32x4*>(p.gate + (size_t)b * p.C + k);
                dq = *reinterpret_cast<const f32x4*>(p.dsq + (size_t)b * p.C + k);
            }
            if (active)
                for (int r = r0 + rl; r < seg_end; r += RL) {
                    const f32x4 dz = *reinterpret_cast<const f32x4*>(p.dz + (size_t)r * p.lddz + k);
                    const f32x4 rv = *reinterpret_cast<const f32x4*>(p.r + (size_t)r * p.ldr + k);
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
                    store16(p.du + (size_t)r * p.lddu + k, du);
                }
            if (p.g_mask) {
                const f32x4 s = lane_sum(g_m);
                if (active && rl == 0) *reinterpret_cast<f32x4*>(pm_work_mask(p) + (size_t)(split + b) * p.C + k) = s;
            }
        }
        r0 = seg_end;
        ++b;
    }
    const f32x4 s1 = lane_sum(g_sh), s2 = lane_sum(g_sc);
    if (active && rl == 0) {
        *reinterpret_cast<f32x4*>(pm_work_shift(p) + (size_t)split * p.C + k) = s1;
        *reinterpret_cast<f32x4*>(pm_work_scale(p) + (size_t)split * p.C + k) = s2;
    }
}

// k_act_reduce for PmArgs
__global__ __launch_bounds__(256) void k_postmask_reduce(const PmArgs p, int nvec) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int Q = p.C >> 2;
    if (i >= nvec * Q) return;
    const int j = i / Q, k = 4 * (i - j * Q);
    const int count = rows_count(p.m_count, p.m_cap);
    if (j < 2) {
        f32x4 s = {0.f, 0.f, 0.f, 0.f};
        const int live = min(p.splits, ceil_div(count, p.rps));
        const float* w = j == 0 ? pm_work_shift(p) : pm_work_scale(p);
        for (int t = 0; t < live; ++t) s += *reinterpret_cast<const f32x4*>(w + (size_t)t * p.C + k);
        *reinterpret_cast<f32x4*>((j == 0 ? p.g_shift : p.g_scale) + k) = s;
        return;
    }
    const int b = j - 2;
    *reinterpret_cast<f32x4*>(p.g_mask + (size_t)b * p.C + k) = image_slots_sum(pm_work_mask(p), p.prefix, p.B, b, count, p.splits, p.rps, p.C, k);
}

struct DotArgs {
    const float* a; const float* b; const int32_t* prefix; const int32_t* m_count; float* out; float* work;
    int lda, ldb, B, m_cap, C, splits, rps;
};

// out[b, k] partials = sum over the rows of image b in this split of a * b: the walk of k_rows_act_bwd with its g_mask alone; work = [splits + B][C]
__global__ __launch_bounds__(ACT_THREADS) void k_rows_img_dot(const DotArgs p) {
    __shared__ f32x4 s_red[ACT_THREADS];
    const int Q = p.C >> 2;
    const int QT = Q < ACT_QT ? Q : ACT_QT;
    const int RL = ACT_THREADS / QT;
    const int tid = threadIdx.x, rl = tid / QT, ql = tid - rl * QT;
    const int q = blockIdx.x * ACT_QT + ql;
    const bool active = rl < RL && q < Q;
    const int split = blockIdx.y;
    const int count = rows_count(p.m_count, p.m_cap);
    const int r_begin = split * p.rps;
    const int r_end = min(count, min(p.m_cap, r_begin + p.rps));
    const int k = 4 * q;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    if (r_begin >= r_end) return;          // (uniform) no rows: k_img_dot_reduce does not read this split's slots
    int b = image_of_row(p.prefix, p.B, r_begin);
    int r0 = r_begin;
    while (r0 < r_end) {                   // (uniform) one segment per image that owns rows of this split
        int seg_end = r_end;
        if (b < p.B - 1) seg_end = min(r_end, max(p.prefix[b + 1], r0));
        if (seg_end > r0) {
            f32x4 acc = zero;
            if (active)
                for (int r = r0 + rl; r < seg_end; r += RL)
                    acc += *reinterpret_cast<const f32x4*>(p.a + (size_t)r * p.lda + k) * *reinterpret_cast<const f32x4*>(p.b + (size_t)r * p.ldb + k);
            s_red[tid] = acc;              // lane-order sum over the row lanes
            __syncthreads();
            if (active && rl == 0) {
                f32x4 s = zero;
                for (int j = 0; j < RL; ++j) s += s_red[j * QT + ql];
                *reinterpret_cast<f32x4*>(p.work + (size_t)(split + b) * p.C + k) = s;
            }
            __syncthreads();
        }
        r0 = seg_end;
        ++b;
    }
}

// one thread per quad of out[b]
__global__ __launch_bounds__(256) void k_img_dot_reduce(const DotArgs p) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int Q = p.C >> 2;
    if (i >= p.B * Q) return;
    const int b = i / Q, k = 4 * (i - b * Q);
    *reinterpret_cast<f32x4*>(p.out + (size_t)b * p.C + k) =
        image_slots_sum(p.work, p.prefix, p.B, b, rows_count(p.m_count, p.m_cap), p.splits, p.rps, p.C, k);
}

// ---- ldn_rows_ln_bwd: the LayerNorm backward on listed rows.  One WAVE per row (the row sums are wave reductions: lane l owns the quads l, l + 64, ...
// of the row, at most LN_MAXQ of them); a workgroup of four waves owns the list entries [split * rps, + rps), wave w every fourth of them.  The lanes'
// column sums (d_gamma, d_beta) over the wave's rows stay in registers, the four waves' are added in wave order through the LDS, and the
// workgroup writes them to work[split]; k_ln_reduce adds the splits in ascending order.
constexpr int LN_THREADS = 256;
constexpr int LN_WAVES = LN_THREADS / 64;
constexpr int LN_MAXQ = 8;             // quads per lane: C <= 2048 (= ldn_row_stats)
constexpr int LN_MIN_SPLIT_ROWS = 32;
constexpr int LN_MAX_SPLITS = 512;

struct LnArgs {
    const float* x; const float* stats; const float* gamma; const int32_t* list; const int32_t* count; const float* dy;
    float* dx; float* d_gamma; float* d_beta; float* xhat; float* work;
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
    if (r_begin >= r_end) return;          // (uniform) no rows: k_ln_reduce does not read this split's partials
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
            *reinterpret_cast<f32x4*>(p.work + ((size_t)(2 * split + wave)) * p.C + 4 * q) = s;
        }
        __syncthreads();
    }
}

// one thread per quad of d_gamma (j == 0) and d_beta (j == 1): the partials of the splits that hold rows, in ascending order
__global__ __launch_bounds__(256) void k_ln_reduce(const LnArgs p) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int Q = p.C >> 2;
    if (i >= 2 * Q) return;
    const int j = i / Q, k = 4 * (i - j * Q);
    const int count = rows_count(p.count, p.m_cap);
    const int live = min(p.splits, ceil_div(count, p.rps));
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    for (int t = 0; t < live; ++t) s += *reinterpret_cast<const f32x4*>(p.work + ((size_t)(2 * t + j)) * p.C + k);
    *reinterpret_cast<f32x4*>((j == 0 ? p.d_gamma : p.d_beta) + k) = s;
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

extern "C" size_t ldn_rows_act_bwd_workspace_bytes(int m_cap, int C, int B) {
    if (m_cap < 0 || C <= 0 || C % 4 || B < 0) return 0;
    int tiles, splits, rps;
    act_plan(m_cap, C, &tiles, &splits, &rps);
    return ((size_t)2 * splits + (B > 0 ? splits + B : 0)) * C * sizeof(float);
}

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
    p.m_count = m_count; p.du = du; p.g_shift = g_shift; p.g_scale = g_scale_num; p.g_mask = g_mask; p.work = work;
    p.lddh = lddh; p.ldu = ldu; p.ldzy = ldzy; p.lddu = lddu; p.B = (chan_mask || zy) ? B : 0; p.m_cap = m_cap; p.C = C;
    int tiles;
    act_plan(m_cap, C, &tiles, &p.splits, &p.rps);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (m_cap > 0) {
        k_rows_act_bwd<<<dim3((unsigned)tiles, (unsigned)p.splits), ACT_THREADS, 0, st>>>(p);
        LDN_CHECK_LAUNCH("k_rows_act_bwd");
    }
    const int nvec = 2 + (zy ? B : 0);
    k_act_reduce<<<ceil_div(nvec * (C / 4), 256), 256, 0, st>>>(p, nvec);
    LDN_CHECK_LAUNCH("k_act_reduce");
    return LDN_OK;
}

extern "C" size_t ldn_rows_postmask_bwd_workspace_bytes(int m_cap, int C, int B) { return ldn_rows_act_bwd_workspace_bytes(m_cap, C, B); }

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
    p.m_count = m_count; p.du = du; p.g_shift = g_shift; p.g_scale = g_scale_num; p.g_mask = g_mask; p.work = work;
    p.lddz = lddz; p.ldr = ldr; p.lddu = lddu; p.B = per_image ? B : 0; p.m_cap = m_cap; p.C = C;
    int tiles;
    act_plan(m_cap, C, &tiles, &p.splits, &p.rps);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (m_cap > 0) {
        k_rows_postmask_bwd<<<dim3((unsigned)tiles, (unsigned)p.splits), ACT_THREADS, 0, st>>>(p);
        LDN_CHECK_LAUNCH("k_rows_postmask_bwd");
    }
    const int nvec = 2 + (g_mask ? B : 0);
    k_postmask_reduce<<<ceil_div(nvec * (C / 4), 256), 256, 0, st>>>(p, nvec);
    LDN_CHECK_LAUNCH("k_postmask_reduce");
    return LDN_OK;
}

extern "C" size_t ldn_rows_img_dot_workspace_bytes(int m_cap, int C, int B) {
    if (m_cap < 0 || C <= 0 || C % 4 || B < 1) return 0;
    int tiles, splits, rps;
    act_plan(m_cap, C, &tiles, &splits, &rps);
    return ((size_t)splits + B) * C * sizeof(float);
}

extern "C" int ldn_rows_img_dot(const float* a, int lda, const float* b, int ldb, const int32_t* row_prefix, int B, const int32_t* m_count,
                                int m_cap, int C, float* out, float* work, void* stream) {
    LDN_REQUIRE(a && b && row_prefix && out && work, "ldn_rows_img_dot: null pointer");
    LDN_REQUIRE(B >= 1 && m_cap >= 0 && C > 0 && C % 4 == 0, "ldn_rows_img_dot: B >= 1, m_cap >= 0, C %% 4 == 0 (got %d, %d, %d)", B, m_cap, C);
    LDN_REQUIRE(lda >= C && ldb >= C && lda % 4 == 0 && ldb % 4 == 0, "ldn_rows_img_dot: leading dimensions >= C and multiples of 4 (got %d, %d)", lda, ldb);
    LDN_REQUIRE(aligned16(a) && aligned16(b) && aligned16(out) && aligned16(work), "ldn_rows_img_dot: every float pointer must be 16-byte aligned");
    DotArgs p;
    p.a = a; p.b = b; p.prefix = row_prefix; p.m_count = m_count; p.out = out; p.work = work;
    p.lda = lda; p.ldb = ldb; p.B = B; p.m_cap = m_cap; p.C = C;
    int tiles;
    act_plan(m_cap, C, &tiles, &p.splits, &p.rps);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (m_cap > 0) {
        k_rows_img_dot<<<dim3((unsigned)tiles, (unsigned)p.splits), ACT_THREADS, 0, st>>>(p);
        LDN_CHECK_LAUNCH("k_rows_img_dot");
    }
    k_img_dot_reduce<<<ceil_div(B * (C / 4), 256), 256, 0, st>>>(p);
    LDN_CHECK_LAUNCH("k_img_dot_reduce");
    return LDN_OK;
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
    p.x = x; p.stats = stats; p.gamma = gamma; p.list = list; p.count = count; p.dy = dy; p.dx = dx; p.d_gamma = d_gamma; p.d_beta = d_beta;
    p.xhat = xhat; p.work = work; p.ldx = ldx; p.lddy = lddy; p.lddx = lddx; p.ldxh = ldxh; p.rows = rows; p.m_cap = m_cap; p.C = C;
    ln_plan(m_cap, &p.splits, &p.rps);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (m_cap > 0) {
        k_rows_ln_bwd<<<(unsigned)p.splits, LN_THREADS, 0, st>>>(p);
        LDN_CHECK_LAUNCH("k_rows_ln_bwd");
    }
    k_ln_reduce<<<ceil_div(2 * (C / 4), 256), 256, 0, st>>>(p);
    LDN_CHECK_LAUNCH("k_ln_reduce");
    return LDN_OK;
}
