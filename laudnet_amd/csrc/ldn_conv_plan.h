// Which instantiation of k_conv_image / k_conv_bf3 / k_conv1x1_stream (csrc/ldn_conv_image.hip) runs a launch of ldn_conv_image or
// ldn_conv_packed, with what geometry: a pure function of the launch's shape, and the one list of the instantiations that are built.
// Plain C++17 -- no HIP, no environment, no pointers -- so that the choice, the grid and the LDS of every admitted shape are checked
// exhaustively on a CPU (tests/test_conv_plan.py) before anything runs on a device: a block of more rows or columns than its tile holds
// writes out of bounds.  Results never depend on the choice, only the time does.
#pragma once
#include <stdio.h>
#include <string>

namespace ldn {

// How the weights are laid out and staged (the kernels' BMODE; described at k_conv_image).
enum { B_NK = 0, B_KN4 = 1, B_KN2 = 2, B_KN1 = 3 };

constexpr int BK = 32;   // K chunk = one 128-byte LDS row
// k_conv1x1_stream: 128 x 128 tiles, a ring of four A slots and three raw-B slots, two converted-B slots
constexpr int ST_BM = 128, ST_BN = 128;
constexpr int ST_TILE = ST_BM * BK;                       // 4096 floats = 16 KiB: one A slot, one raw-B slot, one converted-B slot
constexpr int ST_A_SLOTS = 4, ST_B_SLOTS = 3;
constexpr int ST_OFF_BRAW = ST_A_SLOTS * ST_TILE, ST_OFF_CB = ST_OFF_BRAW + ST_B_SLOTS * ST_TILE;
constexpr int ST_LDS_FLOATS = ST_OFF_CB + 2 * ST_TILE;    // 9 slots = 144 KiB
constexpr int ST_MAXROWS = 1024;                          // rows per workgroup (8 M blocks)
constexpr long kConvLdsLimit = 160 * 1024;                // the LDS of a CU: a plan above it is refused
constexpr long kConvWeightLimit = 1L << 31;               // the weight staging computes 32-bit element offsets

// A launch, as far as the choice and the geometry depend on it.
//   rows         m_cap of a packed launch, Ho * Wo of an image launch
//   taps         1 or 9 (ksize of a packed launch, ksize * ksize of an image launch)
//   has_k/has_n  per-image input / output channel list; kgran: the granularity of the lists
//   scale        a per-column scale is given (with a residual it keeps a launch off the streaming kernel, whose weights carry the scale)
//   out_split    out_format 1 of ldn_conv_image: rows pre-split for ldn_bottleneck_tail
//   math         0 = fp32 MFMA, 1 = bf16x3
//   stream_rows  LDN_STREAM_ROWS as the library resolved it: rows per workgroup of k_conv1x1_stream, 0 disables the kernel
struct ConvShape {
    bool packed;
    int B, rows, taps, cin, cout;
    bool has_k, has_n;
    int kgran, shift_classes;
    bool residual, scale, out_split;
    int math, stream_rows;
};

// The kernel that runs it: the family, MS x NS subtiles of 32 per block, WM rows of the consumer wave grid (k_conv_bf3 only) and the weight
// staging mode.  k_conv1x1_stream has no tile arguments (ms = ns = wm = 0).
enum ConvFamily { CONV_IMAGE = 0, CONV_BF3 = 1, CONV_STREAM = 2 };
struct ConvKernel {
    int family, ms, ns, wm, bmode;
};
inline bool operator==(const ConvKernel& a, const ConvKernel& b) {
    return a.family == b.family && a.ms == b.ms && a.ns == b.ns && a.wm == b.wm && a.bmode == b.bmode;
}
// ... and the numbers of its launch: bn columns per N block (k_conv1x1_stream: N tiles of 128 per workgroup), ntn N blocks, bm rows per M
// block, mtn M blocks per image, the grid and the dynamic LDS.
struct ConvPlan : ConvKernel {
    int bn, ntn, bm, mtn;
    long grid, lds_bytes;
};

// The two template arguments that follow from the tile: KSKIP (skip the empty k groups of a partial chunk) only pays for the narrow layers,
// which use the small shapes; blocks of <= 64 KiB LDS run two per CU (memory-bound early stages need the extra waves in flight).
constexpr bool conv_kskip(int /*ms*/, int ns) { return ns <= 4; }
constexpr int conv_minw(int ms, int ns) { return ms + ns <= 8 ? 4 : 2; }

inline std::string conv_plan_name(const ConvKernel& k) {
    static const char* const bmodes[] = {"B_NK", "B_KN4", "B_KN2", "B_KN1"};
    const char* b = k.bmode >= 0 && k.bmode < 4 ? bmodes[k.bmode] : "?";
    char s[64];
    if (k.family == CONV_IMAGE) snprintf(s, sizeof s, "k_conv_image<%d,%d,%s>", k.ms, k.ns, b);
    else if (k.family == CONV_BF3) snprintf(s, sizeof s, "k_conv_bf3<%d,%d,%d,%s>", k.ms, k.ns, k.wm, b);
    else snprintf(s, sizeof s, "k_conv1x1_stream<%s>", b);
    return s;
}

// THE list of the instantiations in ldn_conv_image's code object; nothing else instantiates the three kernels.  A row is live if
// conv_plan() returns it for some shape of the sweep of tests/test_conv_plan.py; the test fails on a row that no shape reaches.
//   I(MS, NS, BMODE)  k_conv_image<MS, NS, BMODE, conv_kskip, conv_minw>      F(MS, NS, WM, BMODE)  k_conv_bf3<MS, NS, WM, BMODE, conv_kskip, conv_minw>
//   S(BMODE)          k_conv1x1_stream<BMODE>
// k_conv_bf3<4, 4, 2> (the 4 x 4 tile behind a residual) has no B_KN2 / B_KN1 row: those need both channel lists, and the entry points
// refuse a residual with an output list.
#define LDN_CONV_KERNELS(I, F, S)                                                                                              \
    I(6, 2, B_NK) I(4, 4, B_NK) I(8, 6, B_NK) I(4, 10, B_NK) I(6, 2, B_KN4) I(4, 4, B_KN4) I(8, 6, B_KN4) I(4, 10, B_KN4)      \
    I(6, 2, B_KN2) I(4, 4, B_KN2) I(8, 6, B_KN2) I(4, 10, B_KN2) I(6, 2, B_KN1) I(4, 4, B_KN1) I(8, 6, B_KN1) I(4, 10, B_KN1)  \
    F(6, 2, 2, B_NK) F(4, 4, 4, B_NK) F(4, 4, 2, B_NK) F(8, 6, 4, B_NK) F(4, 10, 2, B_NK) F(2, 10, 2, B_NK)                    \
    F(6, 2, 2, B_KN4) F(4, 4, 4, B_KN4) F(4, 4, 2, B_KN4) F(8, 6, 4, B_KN4) F(4, 10, 2, B_KN4) F(2, 10, 2, B_KN4)              \
    F(6, 2, 2, B_KN2) F(4, 4, 4, B_KN2) F(8, 6, 4, B_KN2) F(4, 10, 2, B_KN2) F(2, 10, 2, B_KN2)                                \
    F(6, 2, 2, B_KN1) F(4, 4, 4, B_KN1) F(8, 6, 4, B_KN1) F(4, 10, 2, B_KN1) F(2, 10, 2, B_KN1)                                \
    S(B_NK) S(B_KN4)
// The gated instantiations of k_conv_bf3 (ldn_conv_image_gated: conv c of a channel-mode block behind the folded SE), a list of its own:
// the B_KN4 rows that conv_plan_gated() returns for the shapes conv_gated_shape_ok() admits, each reached by the sweep of
// tests/test_conv_gated_plan.py.  A gated plan that is no row here is refused.
#define LDN_CONV_GATED_KERNELS(F) \
    F(6, 2, 2, B_KN4) F(4, 4, 4, B_KN4) F(4, 4, 2, B_KN4) F(8, 6, 4, B_KN4) F(4, 10, 2, B_KN4) F(2, 10, 2, B_KN4)
// The kernel that a row of the list is.
#define LDN_CONV_ROW_I(MS, NS, BMODE) ::ldn::ConvKernel{::ldn::CONV_IMAGE, MS, NS, 0, ::ldn::BMODE}
#define LDN_CONV_ROW_F(MS, NS, WM, BMODE) ::ldn::ConvKernel{::ldn::CONV_BF3, MS, NS, WM, ::ldn::BMODE}
#define LDN_CONV_ROW_S(BMODE) ::ldn::ConvKernel{::ldn::CONV_STREAM, 0, 0, 0, ::ldn::BMODE}

// ---- the chooser ----------------------------------------------------------------------------------------------------------------
constexpr int conv_ceil_div(int a, int b) { return (a + b - 1) / b; }
constexpr int conv_round_up(int a, int b) { return conv_ceil_div(a, b) * b; }

// What the entry points refuse by shape, before any launch: an input list on a cin that is no multiple of 8, a weight tensor beyond the
// 32-bit offsets of the weight staging, and (on the plan) more LDS than a CU has.
inline bool conv_list_ok(const ConvShape& s) { return !s.has_k || s.cin % 8 == 0; }
inline long conv_weight_elems(const ConvShape& s) { return (long)s.taps * s.cin * s.cout; }
inline bool conv_admitted(const ConvShape& s, const ConvPlan& p) {
    return conv_list_ok(s) && conv_weight_elems(s) < kConvWeightLimit && p.lds_bytes <= kConvLdsLimit;
}

// The LDS of a k_conv_image / k_conv_bf3 block: two staging buffers of (MS + NS) x 32 rows of a K chunk; the per-column scale / post_sub /
// shift tables; the pixel, class and column tables, the input-channel list and, packed, the rows' out row and A row per tap.
inline long conv_tile_lds_bytes(const ConvShape& s, int ms, int ns) {
    return (long)2 * (ms + ns) * 32 * BK * 4 + (long)((2 + s.shift_classes) * ns * 32) * 4 +
           (long)(2 * ms * 32 + ns * 32 + (s.has_k ? s.cin : 0) + (s.packed ? ms * 32 * (1 + s.taps) : 0)) * 4;
}

// wide 1x1 convolutions without an output-channel list: the persistent streaming kernel (bf16x3 arithmetic only; its epilogue stores fp32
// rows, so a pre-split output stays with k_conv_bf3)
inline bool conv_streams(const ConvShape& s) {
    return s.math == 1 && s.stream_rows >= ST_BM && s.taps == 1 && !s.has_n && s.shift_classes == 1 && !s.out_split && s.cout % ST_BN == 0 &&
           s.cout >= 2 * ST_BN && !(s.residual && s.scale) && s.cin <= 1024 &&
           s.rows >= 96;   // (7x7 images would leave most of every 128-row M block empty)
}

inline ConvPlan conv_plan_stream(const ConvShape& s) {
    ConvPlan p{};
    static_cast<ConvKernel&>(p) = {CONV_STREAM, 0, 0, 0, s.has_k ? B_KN4 : B_NK};
    p.lds_bytes = (long)ST_LDS_FLOATS * 4 + (long)(2 * ST_MAXROWS + s.cin + 32) * 4;
    int rpb = s.stream_rows;                           // rows per workgroup: fewer when that is needed to fill the chip
    while (rpb > ST_BM && s.B * conv_ceil_div(s.rows, rpb) < 512) rpb /= 2;
    int nblk = conv_ceil_div(s.rows, rpb);
    p.bm = conv_round_up(conv_ceil_div(s.rows, nblk), ST_BM);      // balanced, whole M blocks
    nblk = conv_ceil_div(s.rows, p.bm);
    p.mtn = nblk;
    // too few row blocks to fill the chip (shared-weight launches over a few thousand packed rows): split the N tiles too
    const int ntiles = s.cout / ST_BN;
    int nsplit = 1;
    while (s.B * nblk * nsplit < 512 && nsplit < ntiles) nsplit *= 2;
    p.bn = conv_ceil_div(ntiles, nsplit);
    p.ntn = conv_ceil_div(ntiles, p.bn);
    p.grid = (long)s.B * nblk * p.ntn;
    return p;
}

// The k_conv_image / k_conv_bf3 plan of a shape (conv_plan() below asks the streaming kernel first).
inline ConvPlan conv_plan_tile(const ConvShape& s) {
    // how the weights are staged: w is [cout][taps][cin] without an input list, [taps][cin][cout] with one
    const int g = s.has_n ? s.kgran : 4;
    const int bmode = !s.has_k ? B_NK : g % 4 == 0 ? B_KN4 : g % 2 == 0 ? B_KN2 : B_KN1;
    const int nsubs = conv_ceil_div(s.cout, 32), msubs = conv_ceil_div(s.rows, 32);
    // tile shape: as many output pixels as the LDS budget allows for the layer's width, so that every byte pulled
    // into the CU is reused by as many MFMAs as possible (whole 14x14 / 7x7 images at stages 3 / 4)
    int per;                                                       // n-subtiles per N block
    if (nsubs <= 4) per = nsubs;                                   // <= 128 columns: memory-bound layers, two 64 KiB blocks per CU
    else if (s.rows <= 128) per = nsubs < 10 ? nsubs : 10;         // 7x7 images: wide N blocks (weights dominate the traffic)
    else if (s.rows <= 256 && s.has_n) per = nsubs < 6 ? nsubs : 6;   // 14x14 images: whole image x <= 192 columns per block
    // (measured: the wide 1x1 convs without an output list -- conv3, downsample -- are faster as two co-resident
    //  64 KiB blocks per CU whose phases overlap than as one whole-image block: 208 vs 294 us at stage 3)
    else per = 4;
    int ms = per <= 2 ? 6 : per <= 4 ? 4 : per <= 6 ? 8 : 4;
    const int ns = per <= 2 ? 2 : per <= 4 ? 4 : per <= 6 ? 6 : 10;
    int wm = 0;
    if (s.math == 1) {
        // consumer wave grid WM x 4/WM: every wave owns whole m-subtiles (A fragments are split once and reused);
        // 4 x 1 for the tall 8 x 6 tile, 2 x 2 otherwise; 7x7 images (<= 2 m-subtiles) get a 2-subtile-high tile
        if (ms == 4 && ns == 10 && msubs <= 2) ms = 2;
        // 4x4 tiles: 4 x 1 wave grid (one A split per four tiles) unless the epilogue adds a residual, where the
        // 2 x 2 grid measured 5-8 % faster (conv3-type launches)
        wm = (ms == 4 && ns == 4 && !s.residual) || ms >= 8 ? 4 : 2;
    }
    ConvPlan p{};
    static_cast<ConvKernel&>(p) = {s.math == 1 ? CONV_BF3 : CONV_IMAGE, ms, ns, wm, bmode};
    p.bn = per * 32;
    p.ntn = conv_ceil_div(s.cout, p.bn);
    p.mtn = conv_ceil_div(msubs, ms);                              // M blocks per image, then balance their sizes
    p.bm = conv_ceil_div(msubs, p.mtn) * 32;
    p.grid = (long)conv_round_up(s.B * p.mtn, 8) * p.ntn;          // units padded to the 8 XCDs (tile_setup)
    p.lds_bytes = conv_tile_lds_bytes(s, ms, ns);
    return p;
}

inline ConvPlan conv_plan(const ConvShape& s) {
    if (conv_streams(s)) return conv_plan_stream(s);
    return conv_plan_tile(s);
}

// ---- the gated form of k_conv_bf3 ---------------------------------------------------------------------------------------------------
// What it admits by shape: conv c of a channel-mode block -- bf16x3, a 1x1 at stride 1 over a dense image, an input list and no output
// list, one shift class, fp32 rows out.  (post_sub, colsum and the alignment of the pointers are the entry point's to refuse.)
inline bool conv_gated_shape_ok(const ConvShape& s) {
    return !s.packed && s.math == 1 && s.taps == 1 && s.has_k && !s.has_n && s.shift_classes == 1 && !s.out_split && s.B > 0 && s.rows > 0 &&
           s.cin > 0 && s.cin % 8 == 0 && s.cout > 0 && s.cout % 4 == 0 && s.kgran >= 1;
}
// Its plan: the tile plan of the shape, never the streaming kernel, plus the image's gate vector behind the input-channel list.
inline long conv_gate_lds_bytes(const ConvShape& s) { return (long)conv_round_up(s.cin, BK) * 4; }
inline ConvPlan conv_plan_gated(const ConvShape& s) {
    ConvPlan p = conv_plan_tile(s);
    p.lds_bytes += conv_gate_lds_bytes(s);
    return p;
}
inline bool conv_gated_built(const ConvKernel& k) {
#define LDN_G(MS, NS, WM, BMODE) if (k == ::ldn::ConvKernel{::ldn::CONV_BF3, MS, NS, WM, ::ldn::BMODE}) return true;
    LDN_CONV_GATED_KERNELS(LDN_G)
#undef LDN_G
    return false;
}
// 1 iff ldn_conv_image_gated takes the shape: admitted, its plan a row of the gated list, within the LDS of a CU.
inline bool conv_gated_ok(const ConvShape& s) {
    if (!conv_gated_shape_ok(s)) return false;
    const ConvPlan p = conv_plan_gated(s);
    return conv_admitted(s, p) && conv_gated_built(p);
}

// ---- ... and over packed rows (ldn_conv_packed_gated: conv c of a 'both' block, per mask group, behind the folded SE) ---------------------
// What it admits by shape: the same arithmetic over the packed rows of the images' active pixels (row_prefix) -- bf16x3, one tap, an input
// list and no output list, one shift class.  (post_sub, pix_map, relu == 2 and the alignment of the pointers are the entry point's to refuse.)
inline bool conv_packed_gated_shape_ok(const ConvShape& s) {
    return s.packed && s.math == 1 && s.taps == 1 && s.has_k && !s.has_n && s.shift_classes == 1 && !s.out_split && s.B > 0 && s.rows > 0 &&
           s.cin > 0 && s.cin % 8 == 0 && s.cout > 0 && s.cout % 4 == 0 && s.kgran >= 1;
}
// Its plan: the tile plan of the packed shape, never the streaming kernel, plus the image's gate vector, which lies BEHIND the packed
// tables here (the rows' out row and A row sit where the image form keeps it).
inline ConvPlan conv_plan_packed_gated(const ConvShape& s) {
    ConvPlan p = conv_plan_tile(s);
    p.lds_bytes += conv_gate_lds_bytes(s);
    return p;
}
// 1 iff ldn_conv_packed_gated takes the shape: admitted, its plan a row of the gated list, within the LDS of a CU.
inline bool conv_packed_gated_ok(const ConvShape& s) {
    if (!conv_packed_gated_shape_ok(s)) return false;
    const ConvPlan p = conv_plan_packed_gated(s);
    return conv_admitted(s, p) && conv_gated_built(p);
}

}  // namespace ldn
