// k_packed_mha_bwd -- the backward of k_packed_mha (csrc/ldn_attn.hip): d L / d (q | k | v) of the kept tokens of every image from d L / d (the
// packed attention rows).  gfx950, bf16x3 arithmetic for every GEMM, fp32 softmax, head dimension 64, at most 256 kept tokens per image; beyond,
// the two phases below become the two kernels k_packed_mha_bwd_q / k_packed_mha_bwd_kv further down (ldn_packed_mha_bwd_long).
//
// Per (image, head), with P = softmax(scale Q K^T) over the image's kept keys:
//     dV = P^T dO      dP = dO V^T      D_i = sum_d dO_id O_id = sum_j P_ij dP_ij      dS = P o (dP - D)      dQ = scale dS K      dK = scale dS^T Q
// (D in its second form: the forward's output rows are not an input).
//
// One 512-thread workgroup per (image, head), TWO phases over one LDS region of two [256][AB_KS] fp32 tiles (139,264 B) + 3 KiB of statistics
// -- the four tiles Q, K, V, dO together would be 256 KB, the CU has 160 KiB:
//   phase A, lane = QUERY (the forward's transposed scheme; wave w owns the queries [32 w, 32 w + 32), Q^T and dO^T fragments in registers):
//     LDS = K rows | V rows.  Pass 1 over the 32-key chunks: S^T = K_chunk . Q^T and dP^T = V_chunk . dO^T, the running max m, the sum l and
//     sum e dP -> the query's {m, 1 / l, D}, kept in LDS for phase B.  Pass 2: S^T and dP^T again, dS^T = P^T o (dP^T - D) in the C layout,
//     which is the B layout of  dQ^T[d][query] += K^T_chunk . dS^T  (the A operand reads K transposed out of the K rows: eight 4-byte reads).
//   phase B, lane = KEY (wave w owns the keys [32 w, 32 w + 32), K^T and V^T fragments in registers):
//     LDS = Q rows | dO rows.  Per 32-query chunk: S = Q_chunk . K^T, dP = dO_chunk . V^T (C layout: lane = key, registers = queries), P from
//     the statistics of phase A, then  dV^T[d][key] += dO^T_chunk . P  and  dK^T[d][key] += Q^T_chunk . dS  with P / dS as B operands.
// The probabilities never leave the registers in either phase.  S and dP are computed three times in all (9 GEMM passes where 5 is the
// minimum): the price of neither storing P nor taking the forward's statistics.
//
// DETERMINISM: dK / dV of an (image, head) are summed inside its workgroup, query chunks in ascending order; no atomics.  The grid is
// (B * heads), the LDS a function of max_tokens: nothing depends on a device-side count (graph-capturable).  Every loop is bounded by
// Lb = min(prefix[b + 1] - prefix[b], max_tokens).
// BARRIERS (four): every wave of a workgroup that passes the two uniform early exits (no tokens, dropped head) runs all of them; a wave
// without queries / keys skips the arithmetic only.
#include "ldn_common.h"

namespace ldn {

constexpr int AB_D = 64;                // head dimension
constexpr int AB_KS = 68;               // row stride of an LDS tile (floats): 16-byte aligned, 4 banks of shift per row
constexpr int AB_MAXTOK = 256;          // kept tokens of one image (k_packed_mha_bwd), of one tile (k_packed_mha_bwd_q / _kv)
constexpr int AB_MAXTILES = 65535;      // tiles of the tiled pair (gridDim.y)

struct MhaBwdArgs {
    const float* qkv; int ld;           // dense token rows [rows][ld]: q | k | v, each [heads][64]
    const int32_t* tok_rows;            // [N] flat row of every kept token
    const int32_t* prefix;              // [B + 1]
    int B, heads, dim, max_tokens;
    float scale;
    const float* d_out; int ldo;        // packed rows [N][ldo]: d L / d (row n of ldn_packed_mha's out)
    float* d_qkv; int ldg;              // dense token rows [rows][ldg]: dq | dk | dv
    const float* head_keep;             // optional [B][heads] {0,1}
};

// the 32 x 32 products S^T / dP^T (phase A) or S / dP (phase B) of one chunk: A operand = 32 rows of an LDS tile, 16 d per K16 step.  SWAP
// exchanges the two mixed products: phase A (tile = K / V) and phase B (tile = Q / dO, SWAP) then add the same three products of
// every (query, key) pair in the same order, so that both phases see the same S and dP
template <bool SWAP> __device__ __forceinline__ f32x16 chunk_gemm(const float* tile_row, const bf16x8 (&bh)[4], const bf16x8 (&bl)[4]) {
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(tile_row + 16 * s);
        const f32x4 c4 = *reinterpret_cast<const f32x4*>(tile_row + 16 * s + 4);
        bf16x8 ah, al;
        split8(a, c4, ah, al);
        if constexpr (SWAP) {
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl[s], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh[s], acc, 0, 0, 0);
        } else {
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh[s], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl[s], acc, 0, 0, 0);
        }
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh[s], acc, 0, 0, 0);
    }
    return acc;
}

// acc[j][d 32 j + ..][lane] += T^T_chunk . X: T = an LDS tile whose rows [row0, row0 + 32) are the summed index, X = a C-layout tile (registers 8 t .. 8 t + 7
// = rows 16 t + (e & 3) + 8 (e >> 2) + 4 h) as the B operand; the A operand reads column d = 32 j + l31 of T in the same row order
__device__ __forceinline__ void chunk_gemm_t(f32x16 (&acc)[2], const float* tile, int row0, int l31, int h, const f32x16& x) {
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        bf16x8 xh, xl;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float v = x[8 * t + e];
            const __bf16 hb = (__bf16)v;
            xh[e] = hb;
            xl[e] = (__bf16)(v - (float)hb);
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const float* col = tile + (size_t)(row0 + 16 * t + 4 * h) * AB_KS + 32 * j + l31;
            bf16x8 ah, al;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float v = col[((e & 3) + 8 * (e >> 2)) * AB_KS];
                const __bf16 hb = (__bf16)v;
                ah[e] = hb;
                al[e] = (__bf16)(v - (float)hb);
            }
            acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, xh, acc[j], 0, 0, 0);
            acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, xl, acc[j], 0, 0, 0);
            acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, xh, acc[j], 0, 0, 0);
        }
    }
}

// B-operand fragments of one 64-float row: K16 step s of lane (l31, h) = elements 16 s + 8 h .. + 7
__device__ __forceinline__ void row_fragments(const float* row, int h, bf16x8 (&fh)[4], bf16x8 (&fl)[4]) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(row + 16 * s + 8 * h);
        const f32x4 c = *reinterpret_cast<const f32x4*>(row + 16 * s + 8 * h + 4);
        split8(a, c, fh[s], fl[s]);
    }
}

// acc (C layout: lane = column, registers 4 q4 .. 4 q4 + 3 = d 32 j + 8 q4 + 4 h + {0..3}) * f -> 64 floats at dst
__device__ __forceinline__ void store_t(float* dst, const f32x16 (&acc)[2], int h, float f) {
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) {
            const f32x4 v = {acc[j][4 * q4] * f, acc[j][4 * q4 + 1] * f, acc[j][4 * q4 + 2] * f, acc[j][4 * q4 + 3] * f};
            *reinterpret_cast<f32x4*>(dst + 32 * j + 8 * q4 + 4 * h) = v;
        }
}

// ---- the bodies of the two phases over ONE LDS tile of `nchunk` 32-element chunks, shared by k_packed_mha_bwd (one tile holds the image) and
// the tiled pair below (the tiles of an image in ascending order): the same triplets in the same order, so an image with <= 256 kept
// tokens gets the same floats from either form.
// phase A, pass 1: the running {m, l, sum e dP} of the lane's query over the keys [k0, k0 + 32 nchunk) of the K (s_a) / V (s_b) tile.
// register r = key k0 + 32 c + (r & 3) + 8 (r >> 2) + 4 h of the lane's query
__device__ __forceinline__ void stats_tile(const float* s_a, const float* s_b, int nchunk, int k0, int Lb, float scale, int l31, int h,
                                           const bf16x8 (&qh)[4], const bf16x8 (&ql)[4], const bf16x8 (&gh)[4], const bf16x8 (&gl)[4],
                                           float& m_run, float& l_run, float& d_run) {
    for (int c = 0; c < nchunk; ++c) {
        f32x16 sacc = chunk_gemm<false>(s_a + (32 * c + l31) * AB_KS + 8 * h, qh, ql);
        const f32x16 pacc = chunk_gemm<false>(s_b + (32 * c + l31) * AB_KS + 8 * h, gh, gl);
        float mc = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int key = k0 + 32 * c + (r & 3) + 8 * (r >> 2) + 4 * h;
            const float v = key < Lb ? sacc[r] * scale : -INFINITY;
            sacc[r] = v;
            mc = fmaxf(mc, v);
        }
        mc = fmaxf(mc, __shfl_xor(mc, 32, 64));                          // the query's other 16 keys live in the partner half-wave
        const float m_new = fmaxf(m_run, mc);                            // finite: key k0 + 32 c is always a real key
        const float alpha = __expf(m_run - m_new);                       // 0 for the first chunk
        float ls = 0.f, ds = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float e = __expf(sacc[r] - m_new);                     // 0 on the padding keys (their dP is 0 too: V is zero there)
            ls += e;
            ds += e * pacc[r];
        }
        l_run = l_run * alpha + ls;
        d_run = d_run * alpha + ds;
        m_run = m_new;
    }
}

// phase A, pass 2: dQ^T += K^T_chunk . dS^T over the same keys, with the query's final {m, 1 / l, D}
__device__ __forceinline__ void dq_tile(const float* s_a, const float* s_b, int nchunk, int k0, int Lb, float scale, int l31, int h,
                                        const bf16x8 (&qh)[4], const bf16x8 (&ql)[4], const bf16x8 (&gh)[4], const bf16x8 (&gl)[4],
                                        float m_run, float inv, float dd, f32x16 (&dq)[2]) {
    for (int c = 0; c < nchunk; ++c) {
        f32x16 sacc = chunk_gemm<false>(s_a + (32 * c + l31) * AB_KS + 8 * h, qh, ql);
        const f32x16 pacc = chunk_gemm<false>(s_b + (32 * c + l31) * AB_KS + 8 * h, gh, gl);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int key = k0 + 32 * c + (r & 3) + 8 * (r >> 2) + 4 * h;
            const float pr = key < Lb ? __expf(sacc[r] * scale - m_run) * inv : 0.f;
            sacc[r] = pr * (pacc[r] - dd);
        }
        chunk_gemm_t(dq, s_a, 32 * c, l31, h, sacc);
    }
}

// phase B: dV^T += dO^T_chunk . P and dK^T += Q^T_chunk . dS of the lane's key over the 32 nchunk queries of the Q (s_a) / dO (s_b) tile, their
// statistics in s_m / s_il / s_dd.  register r = query 32 c + (r & 3) + 8 (r >> 2) + 4 h of the tile against the lane's key
__device__ __forceinline__ void dkv_tile(const float* s_a, const float* s_b, const float* s_m, const float* s_il, const float* s_dd, int nchunk,
                                         float scale, int l31, int h, const bf16x8 (&kh)[4], const bf16x8 (&kl)[4], const bf16x8 (&vh)[4],
                                         const bf16x8 (&vl)[4], f32x16 (&dk)[2], f32x16 (&dv)[2]) {
    for (int c = 0; c < nchunk; ++c) {
        f32x16 sacc = chunk_gemm<true>(s_a + (32 * c + l31) * AB_KS + 8 * h, kh, kl);
        f32x16 pacc = chunk_gemm<true>(s_b + (32 * c + l31) * AB_KS + 8 * h, vh, vl);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int qi = 32 * c + (r & 3) + 8 * (r >> 2) + 4 * h;
            const float pr = __expf(sacc[r] * scale - s_m[qi]) * s_il[qi];   // padding queries: exp(0) * 0
            sacc[r] = pr;
            pacc[r] = pr * (pacc[r] - s_dd[qi]);
        }
        chunk_gemm_t(dv, s_b, 32 * c, l31, h, sacc);
        chunk_gemm_t(dk, s_a, 32 * c, l31, h, pacc);
    }
}

__device__ __forceinline__ void zero2(f32x16 (&a)[2]) {
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) a[j][r] = 0.f;
}

__global__ __launch_bounds__(512) void k_packed_mha_bwd(const MhaBwdArgs p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int b = blockIdx.x / p.heads, hd = blockIdx.x - b * p.heads;
    const int n0 = p.prefix[b];
    const int Lb = min(min(p.prefix[b + 1] - n0, p.max_tokens), AB_MAXTOK);
    if (Lb <= 0) return;                                                  // (uniform) a skipped attention sub-block: nothing is touched
    const int tid = threadIdx.x, lane = tid & 63;
    if (p.head_keep && p.head_keep[(size_t)b * p.heads + hd] < 0.5f) {   // (uniform) dropped head: exact zeros in its 3 x 64 columns
        for (int i = tid; i < Lb * 48; i += 512) {
            const int key = i / 48, c = i - key * 48;
            float* dst = p.d_qkv + (size_t)p.tok_rows[n0 + key] * p.ldg + (c >> 4) * p.dim + hd * AB_D + (c & 15) * 4;
            *reinterpret_cast<f32x4*>(dst) = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        return;
    }
    const int Lp = round_up(Lb, 32);
    float* const s_a = reinterpret_cast<float*>(smem);                   // [Lp][AB_KS]: K rows (phase A), Q rows (phase B)
    float* const s_b = s_a + (size_t)Lp * AB_KS;                         // [Lp][AB_KS]: V rows (phase A), dO rows (phase B)
    float* const s_m = s_b + (size_t)Lp * AB_KS;                         // [Lp] running max of every query (0 on the padding queries)
    float* const s_il = s_m + Lp;                                        // [Lp] 1 / sum (0 on the padding queries: their P is 0)
    float* const s_dd = s_il + Lp;                                       // [Lp] D
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, h = lane >> 5;
    const int ti = wave * 32 + l31;                                       // this lane's query (phase A) / key (phase B)
    const bool tvalid = ti < Lb;
    const bool wlive = wave * 32 < Lb;                                    // wave-uniform
    const int trow = p.tok_rows[n0 + (tvalid ? ti : 0)];                  // a lane without a token reads the image's first one
    const float* const qkv_row = p.qkv + (size_t)trow * p.ld + hd * AB_D;
    float* const g_row = p.d_qkv + (size_t)trow * p.ldg + hd * AB_D;
    const int nchunk = Lp / 32;

    // ---- phase A: gather K rows and V rows: thread = (key, 4 d-values); padding keys are zero
    for (int i = tid; i < Lp * 16; i += 512) {
        const int key = i >> 4, q4 = i & 15;
        f32x4 kv = {0.f, 0.f, 0.f, 0.f}, vv = {0.f, 0.f, 0.f, 0.f};
        if (key < Lb) {
            const float* row = p.qkv + (size_t)p.tok_rows[n0 + key] * p.ld + hd * AB_D + q4 * 4;
            kv = *reinterpret_cast<const f32x4*>(row + p.dim);
            vv = *reinterpret_cast<const f32x4*>(row + 2 * p.dim);
        }
        *reinterpret_cast<f32x4*>(s_a + key * AB_KS + q4 * 4) = kv;
        *reinterpret_cast<f32x4*>(s_b + key * AB_KS + q4 * 4) = vv;
    }
    __syncthreads();
    if (wlive) {
        bf16x8 qh[4], ql[4], gh[4], gl[4];                                // Q^T and dO^T of this lane's query
        row_fragments(qkv_row, h, qh, ql);
        row_fragments(p.d_out + (size_t)(n0 + (tvalid ? ti : 0)) * p.ldo + hd * AB_D, h, gh, gl);
        // pass 1: the softmax statistics and D
        float m_run = -INFINITY, l_run = 0.f, d_run = 0.f;
        stats_tile(s_a, s_b, nchunk, 0, Lb, p.scale, l31, h, qh, ql, gh, gl, m_run, l_run, d_run);
        const float inv = 1.f / (l_run + __shfl_xor(l_run, 32, 64));
        const float dd = (d_run + __shfl_xor(d_run, 32, 64)) * inv;
        if (h == 0) {                                                     // ti < Lp: the wave is live
            s_m[ti] = tvalid ? m_run : 0.f;
            s_il[ti] = tvalid ? inv : 0.f;
            s_dd[ti] = tvalid ? dd : 0.f;
        }
        // pass 2: dQ^T += K^T_chunk . dS^T
        f32x16 dq[2];
        zero2(dq);
        dq_tile(s_a, s_b, nchunk, 0, Lb, p.scale, l31, h, qh, ql, gh, gl, m_run, inv, dd, dq);
        if (tvalid) store_t(g_row, dq, h, p.scale);
    }
    __syncthreads();                                                      // every wave has finished reading K / V; the statistics are in LDS

    // ---- phase B: gather Q rows and dO rows: thread = (query, 4 d-values); padding queries are zero
    for (int i = tid; i < Lp * 16; i += 512) {
        const int qi = i >> 4, q4 = i & 15;
        f32x4 qv = {0.f, 0.f, 0.f, 0.f}, gv = {0.f, 0.f, 0.f, 0.f};
        if (qi < Lb) {
            qv = *reinterpret_cast<const f32x4*>(p.qkv + (size_t)p.tok_rows[n0 + qi] * p.ld + hd * AB_D + q4 * 4);
            gv = *reinterpret_cast<const f32x4*>(p.d_out + (size_t)(n0 + qi) * p.ldo + hd * AB_D + q4 * 4);
        }
        *reinterpret_cast<f32x4*>(s_a + qi * AB_KS + q4 * 4) = qv;
        *reinterpret_cast<f32x4*>(s_b + qi * AB_KS + q4 * 4) = gv;
    }
    __syncthreads();
    if (!wlive) return;                                                   // after the last barrier
    bf16x8 kh[4], kl[4], vh[4], vl[4];                                    // K^T and V^T of this lane's key
    row_fragments(qkv_row + p.dim, h, kh, kl);
    row_fragments(qkv_row + 2 * p.dim, h, vh, vl);
    f32x16 dk[2], dv[2];
    zero2(dk);
    zero2(dv);
    dkv_tile(s_a, s_b, s_m, s_il, s_dd, nchunk, p.scale, l31, h, kh, kl, vh, vl, dk, dv);
    if (!tvalid) return;
    store_t(g_row + p.dim, dk, h, p.scale);
    store_t(g_row + 2 * p.dim, dv, h, 1.f);
}

// ---- images with MORE than 256 kept tokens: the two phases as two launches on one stream, grid (image, head) x ceil(max_tokens / 256) tiles.
// An image's queries now spread over several workgroups, so the statistics {m, 1 / l, D} cross the kernel boundary in a caller-provided
// workspace ws [heads][3][ws_rows] fp32, column = packed row n0 + query.  The LDS region is the short kernel's at 256 tokens (142,336 B);
// each kernel streams the other side's rows through the two tiles, 256 at a time in ascending order, the chunk arithmetic carried from one
// tile to the next: an image with <= 256 kept tokens gets the floats of k_packed_mha_bwd, bit for bit.
// BARRIERS: the trip count of every tile loop comes from Lb alone; every wave of a workgroup that passes the uniform early exits (tile past
// Lb, dropped head) runs every gather and every barrier, a wave without queries / keys skips the arithmetic only.
// RECYCLED MEMORY: the workspace and the rows of d_out at and past n0 + Lb hold anything; every load of either is guarded by `< Lb`, the
// padding queries' statistics are written into LDS as zeros, and k_packed_mha_bwd_kv reads exactly the entries k_packed_mha_bwd_q wrote (the
// same Lb, the same dropped heads).
struct MhaBwdLongArgs {
    MhaBwdArgs a;
    float* ws;                          // [heads][3][ws_rows]: m | 1 / l | D of every live query
    int ws_rows;
};

// Lb of image b: min(count, max_tokens), and never past the workspace (a list that breaks the caller's promise n0 + Lb <= ws_rows cannot
// reach outside it)
__device__ __forceinline__ int long_tokens(const MhaBwdLongArgs& pl, int b, int& n0) {
    n0 = pl.a.prefix[b];
    return min(min(pl.a.prefix[b + 1] - n0, pl.a.max_tokens), pl.ws_rows - n0);
}

// gather the rows [r0, r0 + Lp) of the image into the two tiles: thread = (row, 4 d-values), padding rows (>= Lb) are zero.  KV: K rows | V rows
// of qkv; otherwise Q rows of qkv | rows of d_out
template <bool KV> __device__ __forceinline__ void gather_tile(const MhaBwdArgs& p, float* s_a, float* s_b, int n0, int hd, int r0, int Lp, int Lb,
                                                               int tid) {
    for (int i = tid; i < Lp * 16; i += 512) {
        const int r = i >> 4, q4 = i & 15;
        f32x4 av = {0.f, 0.f, 0.f, 0.f}, bv = {0.f, 0.f, 0.f, 0.f};
        if (r0 + r < Lb) {
            const float* row = p.qkv + (size_t)p.tok_rows[n0 + r0 + r] * p.ld + hd * AB_D + q4 * 4;
            if constexpr (KV) {
                av = *reinterpret_cast<const f32x4*>(row + p.dim);
                bv = *reinterpret_cast<const f32x4*>(row + 2 * p.dim);
            } else {
                av = *reinterpret_cast<const f32x4*>(row);
                bv = *reinterpret_cast<const f32x4*>(p.d_out + (size_t)(n0 + r0 + r) * p.ldo + hd * AB_D + q4 * 4);
            }
        }
        *reinterpret_cast<f32x4*>(s_a + r * AB_KS + q4 * 4) = av;
        *reinterpret_cast<f32x4*>(s_b + r * AB_KS + q4 * 4) = bv;
    }
}

// phase A, lane = QUERY: the statistics of the tile's queries -> ws, their dq columns -> d_qkv
__global__ __launch_bounds__(512) void k_packed_mha_bwd_q(const MhaBwdLongArgs pl) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const MhaBwdArgs& p = pl.a;
    const int b = blockIdx.x / p.heads, hd = blockIdx.x - b * p.heads;
    int n0;
    const int Lb = long_tokens(pl, b, n0);
    const int q0 = blockIdx.y * AB_MAXTOK;                                // first query of this tile
    if (q0 >= Lb) return;                                                 // (uniform; Lb <= 0 too) before any barrier
    const int tid = threadIdx.x, lane = tid & 63;
    if (p.head_keep && p.head_keep[(size_t)b * p.heads + hd] < 0.5f) {   // (uniform) dropped head: exact zeros in the tile's 64 dq columns
        const int nq = min(Lb - q0, AB_MAXTOK);
        for (int i = tid; i < nq * 16; i += 512)
            *reinterpret_cast<f32x4*>(p.d_qkv + (size_t)p.tok_rows[n0 + q0 + (i >> 4)] * p.ldg + hd * AB_D + (i & 15) * 4) = f32x4{0.f, 0.f, 0.f, 0.f};
        return;
    }
    float* const s_a = reinterpret_cast<float*>(smem);                   // [256][AB_KS]: K rows of the current key tile
    float* const s_b = s_a + (size_t)AB_MAXTOK * AB_KS;                  // [256][AB_KS]: V rows
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, h = lane >> 5;
    const int qi = q0 + wave * 32 + l31;                                  // this lane's query
    const bool tvalid = qi < Lb;
    const bool wlive = q0 + wave * 32 < Lb;                               // wave-uniform
    const int qn = n0 + (tvalid ? qi : q0);                               // a lane without a query reads the tile's first one (q0 < Lb)
    const int trow = p.tok_rows[qn];
    bf16x8 qh[4], ql[4], gh[4], gl[4];                                    // Q^T and dO^T of this lane's query
    row_fragments(p.qkv + (size_t)trow * p.ld + hd * AB_D, h, qh, ql);
    row_fragments(p.d_out + (size_t)qn * p.ldo + hd * AB_D, h, gh, gl);
    const int ntile = ceil_div(Lb, AB_MAXTOK);                            // from Lb only: the same for every wave of the workgroup

    // pass 1 over all key tiles: the softmax statistics and D
    float m_run = -INFINITY, l_run = 0.f, d_run = 0.f;
    for (int kt = 0; kt < ntile; ++kt) {
        const int k0 = kt * AB_MAXTOK;
        const int Lp = round_up(min(Lb - k0, AB_MAXTOK), 32);             // keys of the tile, padded to whole chunks
        if (kt) __syncthreads();                                          // every wave has finished reading the previous tile
        gather_tile<true>(p, s_a, s_b, n0, hd, k0, Lp, Lb, tid);
        __syncthreads();
        if (wlive) stats_tile(s_a, s_b, Lp / 32, k0, Lb, p.scale, l31, h, qh, ql, gh, gl, m_run, l_run, d_run);
    }
    const float inv = 1.f / (l_run + __shfl_xor(l_run, 32, 64));          // (a wave without queries: 1 / 0, never used)
    const float dd = (d_run + __shfl_xor(d_run, 32, 64)) * inv;
    if (tvalid && h == 0) {
        float* w = pl.ws + (size_t)hd * 3 * pl.ws_rows + n0 + qi;
        w[0] = m_run;
        w[pl.ws_rows] = inv;
        w[2 * (size_t)pl.ws_rows] = dd;
    }
    // pass 2 over the key tiles again: dQ^T += K^T_chunk . dS^T.  One tile (<= 256 kept tokens) is still in LDS: no second gather
    f32x16 dq[2];
    zero2(dq);
    for (int kt = 0; kt < ntile; ++kt) {
        const int k0 = kt * AB_MAXTOK;
        const int Lp = round_up(min(Lb - k0, AB_MAXTOK), 32);
        if (ntile > 1) {                                                  // (uniform)
            __syncthreads();
            gather_tile<true>(p, s_a, s_b, n0, hd, k0, Lp, Lb, tid);
            __syncthreads();
        }
        if (wlive) dq_tile(s_a, s_b, Lp / 32, k0, Lb, p.scale, l31, h, qh, ql, gh, gl, m_run, inv, dd, dq);
    }
    if (tvalid) store_t(p.d_qkv + (size_t)trow * p.ldg + hd * AB_D, dq, h, p.scale);
}

// phase B, lane = KEY: the dk | dv columns of the tile's keys, summed over the image's query tiles in ascending order
__global__ __launch_bounds__(512) void k_packed_mha_bwd_kv(const MhaBwdLongArgs pl) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const MhaBwdArgs& p = pl.a;
    const int b = blockIdx.x / p.heads, hd = blockIdx.x - b * p.heads;
    int n0;
    const int Lb = long_tokens(pl, b, n0);
    const int k0 = blockIdx.y * AB_MAXTOK;                                // first key of this tile
    if (k0 >= Lb) return;                                                 // (uniform; Lb <= 0 too) before any barrier
    const int tid = threadIdx.x, lane = tid & 63;
    if (p.head_keep && p.head_keep[(size_t)b * p.heads + hd] < 0.5f) {   // (uniform) dropped head: exact zeros in the tile's 64 + 64 dk / dv columns
        const int nk = min(Lb - k0, AB_MAXTOK);
        for (int i = tid; i < nk * 32; i += 512) {
            const int key = i >> 5, c = i & 31;
            float* dst = p.d_qkv + (size_t)p.tok_rows[n0 + k0 + key] * p.ldg + (1 + (c >> 4)) * p.dim + hd * AB_D + (c & 15) * 4;
            *reinterpret_cast<f32x4*>(dst) = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        return;
    }
    float* const s_a = reinterpret_cast<float*>(smem);                   // [256][AB_KS]: Q rows of the current query tile
    float* const s_b = s_a + (size_t)AB_MAXTOK * AB_KS;                  // [256][AB_KS]: dO rows
    float* const s_m = s_b + (size_t)AB_MAXTOK * AB_KS;                  // [256] m of the tile's queries (0 on the padding queries)
    float* const s_il = s_m + AB_MAXTOK;                                 // [256] 1 / l (0 on the padding queries: their P is 0)
    float* const s_dd = s_il + AB_MAXTOK;                                // [256] D
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, h = lane >> 5;
    const int ki = k0 + wave * 32 + l31;                                  // this lane's key
    const bool tvalid = ki < Lb;
    const bool wlive = k0 + wave * 32 < Lb;                               // wave-uniform
    const int trow = p.tok_rows[n0 + (tvalid ? ki : k0)];                 // a lane without a key reads the tile's first one (k0 < Lb)
    const float* const qkv_row = p.qkv + (size_t)trow * p.ld + hd * AB_D;
    bf16x8 kh[4], kl[4], vh[4], vl[4];                                    // K^T and V^T of this lane's key
    row_fragments(qkv_row + p.dim, h, kh, kl);
    row_fragments(qkv_row + 2 * p.dim, h, vh, vl);
    f32x16 dk[2], dv[2];
    zero2(dk);
    zero2(dv);
    const int ntile = ceil_div(Lb, AB_MAXTOK);                            // from Lb only
    for (int qt = 0; qt < ntile; ++qt) {
        const int q0 = qt * AB_MAXTOK;
        const int Lp = round_up(min(Lb - q0, AB_MAXTOK), 32);             // queries of the tile, padded to whole chunks
        if (qt) __syncthreads();                                          // every wave has finished reading the previous tile
        gather_tile<false>(p, s_a, s_b, n0, hd, q0, Lp, Lb, tid);
        if (tid < Lp) {                                                   // the statistics k_packed_mha_bwd_q wrote; zeros, not loads, on the padding queries
            const bool live = q0 + tid < Lb;
            const float* w = pl.ws + (size_t)hd * 3 * pl.ws_rows + n0 + q0 + tid;
            s_m[tid] = live ? w[0] : 0.f;
            s_il[tid] = live ? w[pl.ws_rows] : 0.f;
            s_dd[tid] = live ? w[2 * (size_t)pl.ws_rows] : 0.f;
        }
        __syncthreads();
        if (wlive) dkv_tile(s_a, s_b, s_m, s_il, s_dd, Lp / 32, p.scale, l31, h, kh, kl, vh, vl, dk, dv);
    }
    if (!tvalid) return;
    float* const g_row = p.d_qkv + (size_t)trow * p.ldg + hd * AB_D;
    store_t(g_row + p.dim, dk, h, p.scale);
    store_t(g_row + 2 * p.dim, dv, h, 1.f);
}

}  // namespace ldn

using namespace ldn;

extern "C" int ldn_packed_mha_bwd(const float* qkv, int ld_qkv, const int32_t* tok_rows, const int32_t* img_prefix, int B, int heads,
                                  int head_dim, int max_tokens, float scale, const float* head_keep, const float* d_out, int ldo,
                                  float* d_qkv, int ld_dqkv, void* stream) {
    LDN_REQUIRE(qkv && tok_rows && img_prefix && d_out && d_qkv, "ldn_packed_mha_bwd: null pointer");
    LDN_REQUIRE(head_dim == AB_D, "ldn_packed_mha_bwd: head_dim must be 64 (got %d)", head_dim);
    LDN_REQUIRE(B > 0 && heads > 0 && max_tokens > 0, "ldn_packed_mha_bwd: B, heads and max_tokens must be positive");
    LDN_REQUIRE((long long)B * heads <= 0x7fffffffLL, "ldn_packed_mha_bwd: B * heads exceeds the grid");
    LDN_REQUIRE(max_tokens <= AB_MAXTOK, "ldn_packed_mha_bwd: at most %d kept tokens per image (got max_tokens %d): ldn_packed_mha_bwd_long tiles beyond",
                AB_MAXTOK, max_tokens);
    const int dim = heads * head_dim;
    LDN_REQUIRE(ld_qkv >= 3 * dim && ld_qkv % 4 == 0 && ld_dqkv >= 3 * dim && ld_dqkv % 4 == 0 && ldo >= dim && ldo % 4 == 0,
                "ldn_packed_mha_bwd: bad row strides");
    LDN_REQUIRE((uintptr_t)qkv % 16 == 0 && (uintptr_t)d_out % 16 == 0 && (uintptr_t)d_qkv % 16 == 0,
                "ldn_packed_mha_bwd: qkv / d_out / d_qkv must be 16-byte aligned");
    MhaBwdArgs a{};
    a.qkv = qkv; a.ld = ld_qkv; a.tok_rows = tok_rows; a.prefix = img_prefix; a.B = B; a.heads = heads; a.dim = dim; a.max_tokens = max_tokens;
    a.scale = scale; a.d_out = d_out; a.ldo = ldo; a.d_qkv = d_qkv; a.ldg = ld_dqkv; a.head_keep = head_keep;
    const int Lp = round_up(max_tokens, 32);
    const size_t lds = ((size_t)2 * Lp * AB_KS + (size_t)3 * Lp) * 4;
    LDN_REQUIRE(lds <= 160 * 1024, "ldn_packed_mha_bwd: %zu B of LDS exceed 160 KiB", lds);
    LDN_REQUIRE(allow_dynamic_lds(reinterpret_cast<const void*>(&k_packed_mha_bwd), lds), "k_packed_mha_bwd: cannot reserve %zu B of LDS", lds);
    hipLaunchKernelGGL(k_packed_mha_bwd, dim3((unsigned)B * heads), dim3(512), lds, static_cast<hipStream_t>(stream), a);
    LDN_CHECK_LAUNCH("k_packed_mha_bwd");
    return LDN_OK;
}

extern "C" int ldn_packed_mha_bwd_long(const float* qkv, int ld_qkv, const int32_t* tok_rows, const int32_t* img_prefix, int B, int heads,
                                       int head_dim, int max_tokens, float scale, const float* head_keep, const float* d_out, int ldo,
                                       float* d_qkv, int ld_dqkv, float* ws, int ws_rows, void* stream) {
    LDN_REQUIRE(qkv && tok_rows && img_prefix && d_out && d_qkv && ws, "ldn_packed_mha_bwd_long: null pointer");
    LDN_REQUIRE(head_dim == AB_D, "ldn_packed_mha_bwd_long: head_dim must be 64 (got %d)", head_dim);
    LDN_REQUIRE(B > 0 && heads > 0 && max_tokens > 0, "ldn_packed_mha_bwd_long: B, heads and max_tokens must be positive");
    LDN_REQUIRE((long long)B * heads <= 0x7fffffffLL, "ldn_packed_mha_bwd_long: B * heads exceeds the grid");
    LDN_REQUIRE(max_tokens <= AB_MAXTILES * AB_MAXTOK, "ldn_packed_mha_bwd_long: at most %d kept tokens per image (got %d)", AB_MAXTILES * AB_MAXTOK,
                max_tokens);
    LDN_REQUIRE(ws_rows > 0, "ldn_packed_mha_bwd_long: the statistics workspace must hold at least one packed row (got ws_rows %d)", ws_rows);
    const int dim = heads * head_dim;
    LDN_REQUIRE(ld_qkv >= 3 * dim && ld_qkv % 4 == 0 && ld_dqkv >= 3 * dim && ld_dqkv % 4 == 0 && ldo >= dim && ldo % 4 == 0,
                "ldn_packed_mha_bwd_long: bad row strides");
    LDN_REQUIRE((uintptr_t)qkv % 16 == 0 && (uintptr_t)d_out % 16 == 0 && (uintptr_t)d_qkv % 16 == 0 && (uintptr_t)ws % 4 == 0,
                "ldn_packed_mha_bwd_long: qkv / d_out / d_qkv must be 16-byte aligned, ws 4-byte");
    MhaBwdLongArgs al{};
    MhaBwdArgs& a = al.a;
    a.qkv = qkv; a.ld = ld_qkv; a.tok_rows = tok_rows; a.prefix = img_prefix; a.B = B; a.heads = heads; a.dim = dim; a.max_tokens = max_tokens;
    a.scale = scale; a.d_out = d_out; a.ldo = ldo; a.d_qkv = d_qkv; a.ldg = ld_dqkv; a.head_keep = head_keep;
    al.ws = ws; al.ws_rows = ws_rows;
    const size_t lds = ((size_t)2 * AB_MAXTOK * AB_KS + (size_t)3 * AB_MAXTOK) * 4;      // 142,336 B: one workgroup per CU, as the short kernel at 256
    LDN_REQUIRE(allow_dynamic_lds(reinterpret_cast<const void*>(&k_packed_mha_bwd_q), lds), "k_packed_mha_bwd_q: cannot reserve %zu B of LDS", lds);
    LDN_REQUIRE(allow_dynamic_lds(reinterpret_cast<const void*>(&k_packed_mha_bwd_kv), lds), "k_packed_mha_bwd_kv: cannot reserve %zu B of LDS", lds);
    const dim3 grid((unsigned)B * heads, (unsigned)ceil_div(max_tokens, AB_MAXTOK));
    hipLaunchKernelGGL(k_packed_mha_bwd_q, grid, dim3(512), lds, static_cast<hipStream_t>(stream), al);
    LDN_CHECK_LAUNCH("k_packed_mha_bwd_q");
    hipLaunchKernelGGL(k_packed_mha_bwd_kv, grid, dim3(512), lds, static_cast<hipStream_t>(stream), al);
    LDN_CHECK_LAUNCH("k_packed_mha_bwd_kv");
    return LDN_OK;
}
