// What the training row kernels share (ldn_train_rows.hip, ldn_train_bn.hip): the thread layout's constants, the device-side row count, the image of a
// packed row, and the launch plan -- a function of m_cap and C ONLY, never of the device-side count, so every launch is graph-capturable.
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

// the image b in [0, B) with prefix[b] <= r < prefix[b + 1] (images without rows are stepped over; rows past prefix[B] fall to B - 1)
__device__ __forceinline__ int image_of_row(const int32_t* prefix, int B, int r) {
    int lo = 0, hi = B - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (prefix[mid + 1] > r) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// A workgroup writes the partial per-image sum of every image b that owns rows of its split to the slot split + b: images and splits both ascend
// along the rows, so (split, b) -> split + b is one-to-one over the pairs that meet.  The sum of image b's slots in ascending split order (zero for an image without rows below the count)
__device__ __forceinline__ f32x4 image_slots_sum(const float* slots, const int32_t* prefix, int B, int b, int count, int splits, int rps, int C, int k) {
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    const int lo = min(prefix[b], count), hi = b == B - 1 ? count : min(prefix[b + 1], count);     // (the walk of the row kernels)
    if (lo < hi) {
        // image b meets the splits lo / rps .. (hi - 1) / rps -- unless an earlier image reaches past prefix[b] (never with a monotone prefix)
        const int t_hi = min(splits - 1, (hi - 1) / rps);
        for (int t = lo / rps; t <= t_hi; ++t) s += *reinterpret_cast<const f32x4*>(slots + (size_t)(t + b) * C + k);
    }
    return s;
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

static inline bool aligned16(const void* ptr) { return (uintptr_t)ptr % 16 == 0; }

}  // namespace ldn
