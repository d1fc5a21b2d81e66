// What the training row kernels share (ldn_train_rows.hip, ldn_train_bn.hip): the launch plan, the walk of a workgroup over its packed rows, the
// lane-order sum, the layout of the partials and the two reducers that add them.  A kernel body keeps its per-element arithmetic.
//
// THE WALK.  [m_cap, C] fp32 matrices with a leading dimension, C % 4 == 0, every access 16 bytes wide.  The rows are split over `splits`
// workgroups per 256-channel column tile by act_plan -- a function of (m_cap, C) ONLY, never of the device-side count, so every launch is
// graph-capturable.  The count is read on the device: rows r >= count are never read and are written as exact zeros (zero_past_count); a split
// without rows below the count leaves early, uniformly, and writes no partials.  Inside a workgroup a thread owns one channel quad and every
// RL-th row; the rows are walked one segment per image that owns rows of the split (for_each_image_segment), and the row lanes are added in
// ascending lane order through the LDS (lane_sum).  A second small launch (rows_reduce) adds the partials of the splits THAT HOLD ROWS in
// ascending split order.  No floating-point atomics: two runs are bit-identical.
#pragma once
#include "ldn_common.h"

namespace ldn {

constexpr int ACT_THREADS = 256;
constexpr int ACT_QT = 64;             // quads per column tile (256 channels)
constexpr int ACT_MIN_SPLIT_ROWS = 64;
constexpr int ACT_TARGET_WGS = 2048;
constexpr int ACT_MAX_SPLITS = 256;

__device__ __forceinline__ int rows_count(const int32_t* m_count, int m_cap) {
    int c = m_count ? *m_count : m_cap;
    return c < 0 ? 0 : (c > m_cap ? m_cap : c);
}

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ void st4(float* p, const f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }

// the image b in [0, B) with prefix[b] <= r < prefix[b + 1] (images without rows are stepped over; rows past prefix[B] fall to B - 1; B <= 0: 0, nothing read)
__device__ __forceinline__ int image_of_row(const int32_t* prefix, int B, int r) {
    int lo = 0, hi = B - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (prefix[mid + 1] > r) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// the launch plan: a function of m_cap and C ONLY
static inline void act_plan(int m_cap, int C, int* tiles, int* splits, int* rps) {
    *tiles = ceil_div(C / 4, ACT_QT);
    int s = ceil_div(ACT_TARGET_WGS, *tiles);
    const int most = m_cap / ACT_MIN_SPLIT_ROWS;
    if (s > most) s = most;
    if (s > ACT_MAX_SPLITS) s = ACT_MAX_SPLITS;
    if (s < 1) s = 1;
    *rps = ceil_div(m_cap > 0 ? m_cap : 1, s);
    *splits = ceil_div(m_cap > 0 ? m_cap : 1, *rps);
}

// fills splits / rps; the grid of a walking kernel: (column tiles, splits)
static inline dim3 rows_grid(int m_cap, int C, int* splits, int* rps) {
    int tiles;
    act_plan(m_cap, C, &tiles, splits, rps);
    return dim3((unsigned)tiles, (unsigned)*splits);
}

// ---- the partials.  work = [ncols][splits][C] column partials | [splits + B][C] image slots.  A workgroup writes its partial of column vector j to
// (j, split), and the partial per-image sum of every image b that owns rows of its split to the slot split + b: an image's rows may straddle
// splits, and because images and splits BOTH ASCEND along the rows, (split, b) -> split + b is one-to-one over the pairs that meet (splits + B
// slots instead of splits * B).
__host__ __device__ __forceinline__ float* work_col(float* work, int splits, int C, int j, int split) { return work + ((size_t)j * splits + split) * C; }
__host__ __device__ __forceinline__ float* work_slot(float* work, int splits, int C, int ncols, int slot) {
    return work + ((size_t)ncols * splits + slot) * C;
}
// the sum of image b's slots in ascending split order (zero for an image without rows below the count)
__device__ __forceinline__ f32x4 image_slots_sum(const float* slots, const int32_t* prefix, int B, int b, int count, int splits, int rps, int C, int k) {
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    const int lo = min(prefix[b], count), hi = b == B - 1 ? count : min(prefix[b + 1], count);     // (the segments of for_each_image_segment)
    if (lo < hi) {
        // image b meets the splits lo / rps .. (hi - 1) / rps -- unless an earlier image reaches past prefix[b] (never with a monotone prefix)
        const int t_hi = min(splits - 1, (hi - 1) / rps);
        for (int t = lo / rps; t <= t_hi; ++t) s += ld4(slots + (size_t)(t + b) * C + k);
    }
    return s;
}

static inline size_t rows_work_bytes(int m_cap, int C, int ncols, int B) {
    int splits, rps;
    rows_grid(m_cap, C, &splits, &rps);
    return ((size_t)ncols * splits + (B > 0 ? splits + B : 0)) * C * sizeof(float);
}
// ldn_rows_{act,postmask,bn}_bwd_workspace_bytes: two column vectors, and image slots where there are images
static inline size_t rows_bwd_work_bytes(int m_cap, int C, int B) { return m_cap < 0 || C <= 0 || C % 4 || B < 0 ? 0 : rows_work_bytes(m_cap, C, 2, B); }

// thread = (row lane rl, quad ql) of a QT-quad column tile, QT = min(C / 4, 64), RL = 256 / QT row lanes; grid = rows_grid.  The split owns the rows
// [r_begin, r_cap_end), of which [r_begin, r_end) lie below the count; k = the thread's first channel
struct RowWalk {
    int QT, RL, rl, ql, k, split, count, r_begin, r_cap_end, r_end;
    bool active;                       // false for the threads past RL * QT and the quads past C / 4 of a ragged last tile: they only keep the barriers
    __device__ __forceinline__ bool empty() const { return r_begin >= r_end; }      // uniform over the workgroup
    __device__ __forceinline__ int lane_slot(int j) const { return j * QT + ql; }   // where row lane j of this thread's quad sits in the LDS
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

// the split's rows past the count: exact zeros, nothing read
__device__ __forceinline__ void zero_past_count(const RowWalk& w, float* du, int lddu) {
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    if (w.active)
        for (int r = max(w.r_end, w.r_begin) + w.rl; r < w.r_cap_end; r += w.RL) store16(du + (size_t)r * lddu + w.k, zero);
}

// body(b, r0, seg_end) once per image b that owns the rows [r0, seg_end) != {} of a non-empty split, images ascending; image b owns the rows
// [prefix[b], prefix[b + 1]) (prefix [B + 1]).  B == 0 (no per-image argument): one segment, b = 0, prefix is not read.  The trip count is uniform
// over the workgroup, so the body may hold barriers.  b < B - 1: the last image takes whatever is left (image_of_row sends rows past prefix[B]
// there too) and prefix[B] is never needed; max(.., r0): a prefix that does not ascend cannot move the walk backwards, so no row is visited
// twice, b never passes B - 1 and the loop ends after at most B trips.
template <class Body>
__device__ __forceinline__ void for_each_image_segment(const RowWalk& w, const int32_t* prefix, int B, Body body) {
    int b = image_of_row(prefix, B, w.r_begin);
    int r0 = w.r_begin;
    while (r0 < w.r_end) {
        int seg_end = w.r_end;
        if (b < B - 1) seg_end = min(w.r_end, max(prefix[b + 1], r0));
        if (seg_end > r0) body(b, r0, seg_end);
        r0 = seg_end;
        ++b;
    }
}

// the sum of v over the row lanes of the thread's quad in ascending lane order (uniform barriers); valid in row lane 0
__device__ __forceinline__ f32x4 lane_sum(f32x4* s_red, const RowWalk& w, const f32x4 v) {
    s_red[threadIdx.x] = v;
    __syncthreads();
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    if (w.rl == 0)
        for (int j = 0; j < w.RL; ++j) s += s_red[w.lane_slot(j)];
    __syncthreads();
    return s;
}

// ... written to dst[k .. k + 3], dst = a row of work_col / work_slot
__device__ __forceinline__ void lane_sum_to(f32x4* s_red, const RowWalk& w, const f32x4 v, float* dst) {
    const f32x4 s = lane_sum(s_red, w, v);
    if (w.active && w.rl == 0) st4(dst + w.k, s);
}

// ---- the reducer launch, one thread per quad of an output vector (k_rows_reduce, ldn_train_rows.hip):
//   col_out[j][k]    = sum of cols[j][t][k] over the splits t that hold rows, ascending                             j < ncols <= 2
//   img_out[b][k]    = sum of image b's slots in ascending split order (zero for an image without rows below the count)   b < nimg, 0 or B
// An empty split wrote nothing, so neither sum touches it: live = ceil(count / rps) bounds the first, [prefix[b], prefix[b + 1]) the second.
struct RowsReduceArgs {
    const float* cols; const float* slots; const int32_t* prefix; const int32_t* m_count;
    float* col_out[2]; float* img_out;
    int ncols, nimg, B, m_cap, C, splits, rps;
};
int rows_reduce(const RowsReduceArgs& p, hipStream_t stream);      // LDN_OK or LDN_EHIP

static inline bool aligned16(const void* ptr) { return (uintptr_t)ptr % 16 == 0; }

}  // namespace ldn
