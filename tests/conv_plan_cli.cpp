// Host-only driver of csrc/ldn_conv_plan.h for tests/test_conv_plan.py and tests/conv_plan.py (and for finding the smallest shape that
// reaches a kernel).
//   conv_plan_cli sweep    the chooser over a grid of shapes: one line "<kernel> <cases>" per row of LDN_CONV_KERNELS, one line
//                          "UNBUILT <kernel> <shape>" per plan that names no row, one line "BAD <invariant> <shape> <plan>" per admitted shape
//                          whose geometry breaks an invariant, one line "maxcin <tile> <image 1x1> <packed 3x3, 16 classes>" per tile shape;
//                          exit status 1 if there is an UNBUILT or BAD line, an unreached row or a row listed twice
//   conv_plan_cli          stdin: shape lines
//                              "<packed|image> <fp32|bf16x3> <B> <rows> <taps> <cin> <cout> <has_k> <has_n> <kgran> <shift_classes> <residual>
//                               <scale> <out_split> <stream_rows>"
//                          ('#' lines and blank lines pass through); stdout: the same lines with the plan appended:
//                              "<kernel> <bn> <ntn> <bm> <mtn> <grid> <lds_bytes>", then " REFUSED" if an entry point refuses the shape and
//                              " UNBUILT" if the kernel is no row of the list.
//                          A line that begins with "grid" holds the same fields, each a comma-separated list: the answer is ONE line, the
//                          distinct kernels of the cross product (refused shapes left out), separated by blanks.
#include <stdlib.h>
#include <string.h>

#include <iostream>
#include <set>
#include <sstream>
#include <string>
#include <vector>

#include "../laudnet_amd/csrc/ldn_conv_plan.h"

using namespace ldn;

static const ConvKernel kRows[] = {
#define ROW_I(...) LDN_CONV_ROW_I(__VA_ARGS__),
#define ROW_F(...) LDN_CONV_ROW_F(__VA_ARGS__),
#define ROW_S(...) LDN_CONV_ROW_S(__VA_ARGS__),
    LDN_CONV_KERNELS(ROW_I, ROW_F, ROW_S)
#undef ROW_I
#undef ROW_F
#undef ROW_S
};
constexpr int kNumRows = sizeof kRows / sizeof kRows[0];

static int row_of(const ConvKernel& k) {      // the plan's row of the list, or -1
    for (int i = 0; i < kNumRows; ++i)
        if (k == kRows[i]) return i;
    return -1;
}

static std::string shape_text(const ConvShape& s) {
    char t[160];
    snprintf(t, sizeof t, "%s %s %d %d %d %d %d %d %d %d %d %d %d %d %d", s.packed ? "packed" : "image", s.math == 1 ? "bf16x3" : "fp32", s.B, s.rows, s.taps,
             s.cin, s.cout, s.has_k, s.has_n, s.kgran, s.shift_classes, s.residual, s.scale, s.out_split, s.stream_rows);
    return t;
}
static std::string plan_text(const ConvPlan& p) {
    char t[96];
    snprintf(t, sizeof t, " %d %d %d %d %ld %ld", p.bn, p.ntn, p.bm, p.mtn, p.grid, p.lds_bytes);
    return conv_plan_name(p) + t;
}

// The geometry invariants of an admitted shape: what the kernels assume of bn / ntn / bm / mtn, the grid and the LDS.  nullptr = all hold.
static const char* broken_invariant(const ConvShape& s, const ConvPlan& p) {
    if (p.lds_bytes > kConvLdsLimit) return "lds";
    if (p.grid <= 0 || p.grid >= (1L << 32)) return "grid32";
    if ((long)p.mtn * p.bm < s.rows || p.mtn < 1) return "rows_covered";
    if (p.family == CONV_STREAM) {
        if (p.bm % ST_BM != 0 || p.bm > ST_MAXROWS || p.bm <= 0) return "stream_bm";
        if (p.bn < 1 || (long)p.ntn * p.bn < s.cout / ST_BN || s.cout % ST_BN != 0) return "stream_n_split";
        if (p.grid != (long)s.B * p.mtn * p.ntn) return "stream_grid";
        return nullptr;
    }
    if (p.bn % 32 != 0 || p.bn <= 0 || p.bn > p.ns * 32) return "bn";
    if ((long)p.ntn * p.bn < s.cout) return "cols_covered";
    if (p.bm % 32 != 0 || p.bm <= 0 || p.bm > p.ms * 32) return "bm";
    if (p.grid != (long)conv_round_up(s.B * p.mtn, 8) * p.ntn) return "grid";
    return nullptr;
}

// the largest cin, a multiple of 8, that an input list still fits in the LDS of an ms x ns tile with
static int max_cin_with_list(int ms, int ns, bool packed, int taps, int classes) {
    ConvShape s{};
    s.packed = packed; s.taps = taps; s.shift_classes = classes; s.has_k = true;
    const long room = kConvLdsLimit - conv_tile_lds_bytes(s, ms, ns);      // (cin = 0)
    return room < 0 ? 0 : (int)(room / 4 / 8 * 8);
}

static int sweep() {
    long reached[kNumRows] = {}, cases = 0, admitted = 0, unbuilt = 0, bad = 0;
    std::set<std::string> names;
    for (const ConvKernel& k : kRows) names.insert(conv_plan_name(k));
    const int rows[] = {1, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 255, 256, 257, 512, 520, 3136, 12544};
    const int couts[] = {32, 60, 64, 68, 96, 128, 132, 160, 192, 196, 224, 256, 260, 320, 384, 512, 1024, 2048};
    const int cins[] = {32, 64, 1024, 1032, 2048, 8192, 16384, 131072};
    ConvShape s{};
    for (int packed = 0; packed < 2; ++packed) for (int math = 0; math < 2; ++math) for (int taps : {1, 9}) for (int classes : {1, 16})
    for (int lists = 0; lists < 4; ++lists) for (int gran : {1, 2, 4}) for (int res = 0; res < 3; ++res) for (int split = 0; split < 2; ++split)
    for (int sr : {0, 128, 512, 1024}) for (int B : {1, 8, 9, 256}) {
        s.packed = packed; s.math = math; s.taps = taps; s.shift_classes = classes; s.has_k = lists & 1; s.has_n = lists >> 1; s.kgran = gran;
        s.residual = res > 0; s.scale = res < 2; s.out_split = split; s.stream_rows = sr; s.B = B;      // (res: none / with scale / without)
        // what the entry points refuse whatever the sizes, and what does not steer the plan: a residual with an output list; a pre-split
        // output of a packed, fp32 or residual launch; a granularity without both lists; stream_rows in fp32
        if ((s.residual && s.has_n) || (split && (packed || !math || s.residual)) || (gran != 1 && lists != 3) || (sr != 512 && !math)) continue;
        for (int r : rows) for (int cout : couts) for (int cin : cins) {
            s.rows = r; s.cout = cout; s.cin = cin;
            const ConvPlan p = conv_plan(s);
            ++cases;
            if (!conv_admitted(s, p)) continue;
            ++admitted;
            const int row = row_of(p);
            if (row < 0) { ++unbuilt; printf("UNBUILT %s %s\n", conv_plan_name(p).c_str(), shape_text(s).c_str()); continue; }
            ++reached[row];
            if (const char* what = broken_invariant(s, p)) { ++bad; printf("BAD %s %s %s\n", what, shape_text(s).c_str(), plan_text(p).c_str()); }
        }
    }
    long unreached = 0;
    for (int i = 0; i < kNumRows; ++i) { printf("%s %ld\n", conv_plan_name(kRows[i]).c_str(), reached[i]); unreached += reached[i] == 0; }
    const int tiles[][2] = {{6, 2}, {4, 4}, {8, 6}, {4, 10}, {2, 10}};
    for (const auto& t : tiles)
        printf("maxcin %dx%d %d %d\n", t[0], t[1], max_cin_with_list(t[0], t[1], false, 1, 1), max_cin_with_list(t[0], t[1], true, 9, 16));
    printf("cases %ld admitted %ld rows %d distinct %zu unbuilt %ld unreached %ld bad %ld\n", cases, admitted, kNumRows, names.size(), unbuilt, unreached, bad);
    return (unbuilt || unreached || bad || (int)names.size() != kNumRows) ? 1 : 0;
}

// a shape from its 15 fields (shape_text's order), the two words as 0 / 1
constexpr int NF = 15;
static int field(const std::string& t) { return t == "packed" || t == "bf16x3" ? 1 : atoi(t.c_str()); }
static ConvShape shape_of(const int* f) {
    ConvShape s{};
    s.packed = f[0]; s.math = f[1]; s.B = f[2]; s.rows = f[3]; s.taps = f[4]; s.cin = f[5]; s.cout = f[6]; s.has_k = f[7];
    s.has_n = f[8]; s.kgran = f[9]; s.shift_classes = f[10]; s.residual = f[11]; s.scale = f[12]; s.out_split = f[13]; s.stream_rows = f[14];
    return s;
}

static std::vector<std::string> split(const std::string& text, char sep) {
    std::vector<std::string> out;
    std::stringstream in(text);
    for (std::string t; std::getline(in, t, sep);)
        if (!t.empty()) out.push_back(t);
    return out;
}

int main(int argc, char** argv) {
    if (argc > 1 && !strcmp(argv[1], "sweep")) return sweep();
    for (std::string line; std::getline(std::cin, line);) {
        std::vector<std::string> f = split(line, ' ');
        const bool grid = !f.empty() && f[0] == "grid";
        if (grid) f.erase(f.begin());
        if (line.empty() || line[0] == '#' || (int)f.size() != NF) { puts(line.c_str()); continue; }
        std::vector<int> lists[NF];
        size_t at[NF] = {}, total = 1;
        for (int i = 0; i < NF; ++i) {
            for (const std::string& t : split(f[i], ',')) lists[i].push_back(field(t));
            total *= lists[i].size();
        }
        int one[NF];
        if (!grid) {
            for (int i = 0; i < NF; ++i) one[i] = lists[i][0];
            const ConvShape s = shape_of(one);
            const ConvPlan p = conv_plan(s);
            printf("%s %s%s%s\n", line.c_str(), plan_text(p).c_str(), conv_admitted(s, p) ? "" : " REFUSED", row_of(p) < 0 ? " UNBUILT" : "");
            continue;
        }
        bool seen[kNumRows + 1] = {};      // (the last: a kernel that is no row)
        std::string unbuilt;
        for (size_t c = 0; c < total; ++c) {
            for (int i = 0; i < NF; ++i) one[i] = lists[i][at[i]];
            const ConvShape s = shape_of(one);
            const ConvPlan p = conv_plan(s);
            if (conv_admitted(s, p)) {
                const int row = row_of(p);
                seen[row < 0 ? kNumRows : row] = true;
                if (row < 0) unbuilt = conv_plan_name(p) + "!UNBUILT";
            }
            for (int i = NF - 1; i >= 0 && ++at[i] == lists[i].size(); --i) at[i] = 0;
        }
        std::string out = unbuilt;
        for (int i = 0; i < kNumRows; ++i)
            if (seen[i]) out += (out.empty() ? "" : " ") + conv_plan_name(kRows[i]);
        puts(out.c_str());
    }
    return 0;
}
