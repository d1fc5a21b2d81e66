// Which instantiation of k_dense / k_dense2 (csrc/ldn_dense.hip) runs a shared-weight row convolution: a pure function of the launch's
// shape, and the one list of the instantiations that are built.  Plain C++17 -- no HIP, no environment -- so that the choice is checked
// exhaustively on a CPU (tests/test_dense_plan.py) before anything runs on a device: a FULL kernel on a ragged cout, or a k_dense2 form
// on a cin it cannot tile, writes out of bounds.  Results never depend on the choice, only the time does.
#pragma once
#include <initializer_list>
#include <stdio.h>
#include <string>

namespace ldn {

// A launch, as far as the choice depends on it.
//   taps        1, or 9 (the 3x3 over a neighbour table)
//   rows_known  m_cap without a device-side count, else the hint clamped to m_cap (ldn_hint_rows), else -1: dense_rows_known()
//   f32         true-fp32 MFMA arithmetic (ldn_conv_rows_f32); otherwise bf16x3
//   ps, of      pre-split A rows / pre-split output rows (ldn_conv_rows_ps)
//   pool        pooled patch means as a by-product (ldn_conv_rows_pool; does not steer the choice)
//   feat        a rarely used epilogue term: post_sub, chan_mask, ln_stats or the GELU of relu == 3
//   gated       per-image gate on the A rows (ldn_conv_rows_gated); gate_bytes: the LDS its gate vectors take, dense_gate_bytes()
struct DenseShape {
    int taps, cin, cout, m_cap;
    long rows_known;
    bool f32, ps, of, pool, feat, gated;
    long gate_bytes;
};

// The kernel that runs it: the family (k_dense2, or k_dense), NSUB = columns per workgroup / 32, rows per workgroup (256, or 128: k_dense's
// short-K forms), full (cout is a whole number of column tiles) and, k_dense2 only, the FEAT epilogue and the ragged form (any cin % 8 == 0,
// ragged last column tile).  t9 / f32 / ps / of / ag repeat the shape's form, so that a plan names one instantiation -- or none.
struct DensePlan {
    bool dense2;
    int nsub, rows;
    bool full, feat, rag, t9, f32, ps, of, ag;
};
inline bool operator==(const DensePlan& a, const DensePlan& b) {
    return a.dense2 == b.dense2 && a.nsub == b.nsub && a.rows == b.rows && a.full == b.full && a.feat == b.feat && a.rag == b.rag && a.t9 == b.t9 &&
           a.f32 == b.f32 && a.ps == b.ps && a.of == b.of && a.ag == b.ag;
}
inline std::string dense_plan_name(const DensePlan& p) {
    char s[64];
    if (p.dense2) snprintf(s, sizeof s, "k_dense2<%d,%d,%d,%d,%d,%d,%d>%s", p.nsub, p.t9, p.ps, p.of, p.feat, p.rag, p.ag, p.full && !p.f32 && p.rows == 256 ? "" : "?");
    else snprintf(s, sizeof s, "k_dense<%d,%d,%d,%d,%d,%d,%d>%s", p.nsub, p.t9, p.full, p.f32, p.rows, p.ps, p.of, p.feat || p.rag || p.ag ? "?" : "");
    return s;
}

// THE list of the instantiations in ldn_dense's code object; nothing else instantiates k_dense or k_dense2.  A row is live if
// dense_plan() returns it for some shape of the sweep of tests/test_dense_plan.py; the test fails on a row that no shape reaches.
//   D1(NSUB, T9, FULL, F32, R, PS, OF)      k_dense<...>     D2(NSUB, T9, PS, OF, FEAT, RAG, AG)     k_dense2<...>
// k_dense, bf16x3 1x1 on 256-row tiles (what k_dense2 cannot tile: cin % 64, cin > 2048, a ragged cout), on 128-row tiles (the short-K
// forms), bf16x3 3x3, pre-split A rows, pre-split output rows, true fp32 1x1 and 3x3; k_dense2, 1x1 with the lean epilogue, with the FEAT
// epilogue, the ragged form, 3x3, pre-split A rows, pre-split output rows, gated A rows: in this order.
#define LDN_DENSE_KERNELS(D1, D2)                                                                                                                             \
    D1(2, 0, 0, 0, 256, 0, 0) D1(2, 0, 1, 0, 256, 0, 0) D1(4, 0, 0, 0, 256, 0, 0) D1(4, 0, 1, 0, 256, 0, 0) D1(5, 0, 0, 0, 256, 0, 0)                         \
    D1(5, 0, 1, 0, 256, 0, 0) D1(6, 0, 1, 0, 256, 0, 0) D1(8, 0, 1, 0, 256, 0, 0)                                                                             \
    D1(2, 0, 0, 0, 128, 0, 0) D1(2, 0, 1, 0, 128, 0, 0) D1(4, 0, 1, 0, 128, 0, 0) D1(5, 0, 0, 0, 128, 0, 0) D1(5, 0, 1, 0, 128, 0, 0)                         \
    D1(2, 1, 0, 0, 256, 0, 0) D1(2, 1, 1, 0, 256, 0, 0) D1(4, 1, 0, 0, 256, 0, 0) D1(4, 1, 1, 0, 256, 0, 0)                                                   \
    D1(2, 0, 1, 0, 256, 1, 0) D1(4, 0, 1, 0, 256, 1, 0) D1(8, 0, 1, 0, 256, 1, 0) D1(2, 0, 1, 0, 256, 0, 1) D1(4, 0, 1, 0, 256, 0, 1) D1(8, 0, 1, 0, 256, 0, 1)\
    D1(2, 0, 0, 1, 256, 0, 0) D1(2, 0, 1, 1, 256, 0, 0) D1(4, 0, 0, 1, 256, 0, 0) D1(4, 0, 1, 1, 256, 0, 0) D1(5, 0, 0, 1, 256, 0, 0)                         \
    D1(5, 0, 1, 1, 256, 0, 0) D1(8, 0, 1, 1, 256, 0, 0) D1(2, 1, 0, 1, 256, 0, 0) D1(2, 1, 1, 1, 256, 0, 0) D1(4, 1, 0, 1, 256, 0, 0) D1(4, 1, 1, 1, 256, 0, 0)\
    D2(2, 0, 0, 0, 0, 0, 0) D2(4, 0, 0, 0, 0, 0, 0) D2(5, 0, 0, 0, 0, 0, 0) D2(6, 0, 0, 0, 0, 0, 0) D2(8, 0, 0, 0, 0, 0, 0)                                   \
    D2(2, 0, 0, 0, 1, 0, 0) D2(4, 0, 0, 0, 1, 0, 0) D2(5, 0, 0, 0, 1, 0, 0) D2(6, 0, 0, 0, 1, 0, 0) D2(8, 0, 0, 0, 1, 0, 0)                                   \
    D2(2, 0, 0, 0, 1, 1, 0) D2(5, 0, 0, 0, 1, 1, 0) D2(2, 1, 0, 0, 0, 0, 0) D2(4, 1, 0, 0, 0, 0, 0)                                                           \
    D2(2, 0, 1, 0, 0, 0, 0) D2(4, 0, 1, 0, 0, 0, 0) D2(8, 0, 1, 0, 0, 0, 0) D2(2, 0, 0, 1, 0, 0, 0) D2(4, 0, 0, 1, 0, 0, 0) D2(8, 0, 0, 1, 0, 0, 0)           \
    D2(2, 0, 0, 0, 1, 1, 1) D2(4, 0, 0, 0, 1, 1, 1) D2(5, 0, 0, 0, 1, 1, 1)
// The plan that a row of the list is.  k_dense2 has no FULL / F32 / R arguments: whole (or ragged-form) column tiles, bf16x3, 256 rows.
#define LDN_DENSE_ROW1(NSUB, T9, FULL, F32, R, PS, OF) ::ldn::DensePlan{false, NSUB, R, bool(FULL), false, false, bool(T9), bool(F32), bool(PS), bool(OF), false}
#define LDN_DENSE_ROW2(NSUB, T9, PS, OF, FEAT, RAG, AG) ::ldn::DensePlan{true, NSUB, 256, true, bool(FEAT), bool(RAG), bool(T9), false, bool(PS), bool(OF), bool(AG)}

// ---- the chooser ----------------------------------------------------------------------------------------------------------------
constexpr int kDenseTileRows = 256;
// The rows a launch will find: m_cap without a device-side count; with one, what ldn_hint_rows announced (at most m_cap), or -1.
inline long dense_rows_known(int m_cap, bool counted, long hint) { return !counted ? (long)m_cap : (hint >= 0 ? (hint < m_cap ? hint : (long)m_cap) : -1); }
// The LDS of the gated form's gate vectors: those of every image (of gate_rows rows) that a 256-row tile can touch, cin rounded up to 32 floats each.
inline long dense_gate_bytes(int gate_rows, int cin) { return (long)(255 / gate_rows + 2) * ((cin + 31) / 32 * 32) * 4; }
// The cost model: the time of a launch is rounds x tile time, rounds = ceil(live workgroups / 256) (one workgroup
// per CU: 115-159 KB of LDS), tile time = chunks x (kChunkCycles + kChunkCyclesPerSub NSUB) + kSubtileCycles NSUB cycles (the per-chunk
// law of 4r; the last constant, fitted: epilogue + pipeline fill per 32-column subtile).
constexpr long kChunkCycles = 1700, kChunkCyclesPerSub = 500, kSubtileCycles = 12000, kDenseCus = 256;
// ONE K chunk (a 32-wide input: LAD-RegNet's stage 1 behind its 32-channel stem): nothing to pipeline inside a workgroup, so the launch
// lives on workgroups overlapping EACH OTHER -- 128-row tiles with a two-slot ring (49 KB: three per CU) instead of 256-row tiles with
// the 122 KB ring of the long-K form.  The widest input that takes this form, and the same for 160-column tiles (RegNet 3.25 -> 3.22 ms).
constexpr int kShortK = 32, kShortK5 = 144;
constexpr long kWideMinWorkgroups = 384;      // 256-column tiles without the model: only where they still fill the chip 1.5 times
constexpr long kGatedWideLds = 30 * 1024;     // what the 128-column tiles of the gated form (130 KB of staging) leave for the gate vectors

// can k_dense2 run this launch with tiles of ns * 32 columns?  (whole column tiles, cin a multiple of the tile's K step, a zero row of cin floats)
inline bool dense2_ok(int ns, int taps, int cin, int cout) { return cout % (ns * 32) == 0 && cin % 64 == 0 && cin <= 2048 && (taps == 1 || ns <= 4); }
// ... and its ragged form (64- and 160-column tiles: LAD-RegNet's widths), where that fails?
inline bool dense2_rag_ok(int ns, int cin) { return cin <= 2048 && (ns == 5 || (ns == 2 && cin > 64)); }
// 160-column tiles: layers whose width is a multiple of 160 (320: two whole tiles instead of 128 + 128 + 64), and ragged widths above
// 128 (144 in one tile; 784 = 4 x 160 + 144) -- LAD-RegNet
inline bool dense_tiles5(int cout) { return cout % 160 == 0 || (cout % 32 != 0 && cout > 128); }
inline bool dense_wide_ok(const DenseShape& s) { return s.cout % 256 == 0 && (long)((s.m_cap + kDenseTileRows - 1) / kDenseTileRows) * (s.cout / 256) >= kWideMinWorkgroups; }

inline double dense_tile_cost(const DenseShape& s, int ns) {
    const long chunks = (long)s.taps * ((s.cin + 31) / 32), wgs = (s.rows_known + kDenseTileRows - 1) / kDenseTileRows * (s.cout / (ns * 32));
    return (double)((wgs + kDenseCus - 1) / kDenseCus) * (double)(chunks * (kChunkCycles + kChunkCyclesPerSub * ns) + kSubtileCycles * ns);
}
// The cheapest of the candidate widths that tile cout exactly (the first of equals), when the number of rows is known or hinted; else 0.
inline int dense_cheapest(const DenseShape& s, std::initializer_list<int> widths) {
    int best = 0;
    for (int ns : widths)
        if (s.rows_known > 0 && s.cout % (ns * 32) == 0 && (!best || dense_tile_cost(s, ns) < dense_tile_cost(s, best))) best = ns;
    return best;
}
// Without a row count: as wide as the layer allows (fewer passes over the activation rows) while the grid still fills the chip.
inline int dense_default_width(const DenseShape& s) { return dense_wide_ok(s) ? 8 : s.cout % 128 == 0 ? 4 : s.cout <= 64 ? 2 : dense_tiles5(s.cout) ? 5 : 4; }

inline DensePlan dense_plan_v1(const DenseShape& s, int ns, int rows = kDenseTileRows) { return {false, ns, rows, s.cout % (ns * 32) == 0, false, false, s.taps == 9, s.f32, s.ps, s.of, s.gated}; }
inline DensePlan dense_plan_v2(const DenseShape& s, int ns, bool feat, bool rag) { return {true, ns, kDenseTileRows, rag || s.cout % (ns * 32) == 0, feat, rag, s.taps == 9, s.f32, s.ps, s.of, s.gated}; }
// k_dense2 where it can tile the launch (T9 / PS / OF: one epilogue each; plain 1x1: FEAT on demand), else k_dense
inline DensePlan dense_plan_whole(const DenseShape& s, int ns) { return dense2_ok(ns, s.taps, s.cin, s.cout) ? dense_plan_v2(s, ns, s.feat && s.taps == 1, false) : dense_plan_v1(s, ns); }

inline DensePlan dense_plan(const DenseShape& s) {
    // gated: the gate vectors sit in LDS behind the staging buffers, so wide gates take the 160-column tiles (114 KB of staging)
    const bool gate_fits4 = (s.cout % 128 == 0 || (s.cout > 64 && s.cout <= 128)) && s.gate_bytes <= kGatedWideLds;
    if (s.gated) return dense_plan_v2(s, gate_fits4 ? 4 : s.cout <= 64 ? 2 : 5, true, true);
    if (s.taps == 9) {      // 128- or 64-column tiles; the model only chooses between whole tiles of bf16x3
        const int ns = (s.cout % 128 == 0 ? !s.f32 && dense_cheapest(s, {4, 2}) == 2 : s.cout <= 64) ? 2 : 4;
        return s.f32 ? dense_plan_v1(s, ns) : dense_plan_whole(s, ns);
    }
    if (s.f32) return dense_plan_v1(s, dense_default_width(s));      // the same tile rules (the matrix time per tile is 5.3x longer, the staging the same)
    if (s.ps || s.of) {      // pre-split rows on one side: whole column tiles of 256 / 128 / 64
        const int ns = dense_cheapest(s, {8, 4, 2});
        return dense_plan_whole(s, ns ? ns : dense_wide_ok(s) ? 8 : s.cout % 128 == 0 ? 4 : 2);
    }
    if (!s.feat && s.cin <= kShortK && (s.cout <= 64 || s.cout % 128 == 0)) return dense_plan_v1(s, s.cout <= 64 ? 2 : 4, 128);
    if (!s.feat && s.cin <= kShortK5 && dense_tiles5(s.cout)) return dense_plan_v1(s, 5, 128);
    const int best = dense_cheapest(s, {8, 6, 5, 4, 2}), ns = best ? best : dense_default_width(s);
    if (!best && ns == 5 && s.cin <= 2048) return dense_plan_v2(s, 5, true, true);      // (the ragged form even on whole tiles of 160: it carries every epilogue term)
    if (!dense2_ok(ns, 1, s.cin, s.cout) && dense2_rag_ok(ns, s.cin)) return dense_plan_v2(s, ns, true, true);
    return dense_plan_whole(s, ns);
}

}  // namespace ldn
