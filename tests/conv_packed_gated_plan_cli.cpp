// The packed-row gated form's side of laudnet_amd/csrc/ldn_conv_plan.h on the CPU (tests/test_conv_packed_gated_plan.py; host compiler, no HIP).
//   conv_packed_gated_plan_cli lists       "<rows of LDN_CONV_KERNELS> <rows of LDN_CONV_GATED_KERNELS>", then one gated row per line
//   conv_packed_gated_plan_cli < shapes    per line "B m_cap cin cout residual scale": the line, then
//                                          "<ok 0|1> <shape_ok 0|1> <kernel conv_plan_packed_gated names> <built 0|1> <bn> <ntn> <bm> <mtn> <grid>
//                                           <lds bytes> <ungated packed lds bytes> <weight elements>"
// shape_ok, built, the LDS and the weight elements are what ldn_conv_packed_gated itself checks before it launches: a line with ok 0 names the
// check that refuses it.
#include <stdio.h>
#include <string.h>

#include "../laudnet_amd/csrc/ldn_conv_plan.h"

using namespace ldn;

int main(int argc, char** argv) {
    if (argc > 1 && !strcmp(argv[1], "lists")) {
        int all = 0, gated = 0;
#define CNT(...) ++all;
        LDN_CONV_KERNELS(CNT, CNT, CNT)
#undef CNT
#define CNT(...) ++gated;
        LDN_CONV_GATED_KERNELS(CNT)
#undef CNT
        printf("%d %d\n", all, gated);
#define ROW(MS, NS, WM, BMODE) printf("%s\n", conv_plan_name(LDN_CONV_ROW_F(MS, NS, WM, BMODE)).c_str());
        LDN_CONV_GATED_KERNELS(ROW)
#undef ROW
        return 0;
    }
    char line[256];
    while (fgets(line, sizeof line, stdin)) {
        int B, rows, cin, cout, residual, scale;
        if (sscanf(line, "%d %d %d %d %d %d", &B, &rows, &cin, &cout, &residual, &scale) != 6) return 2;
        ConvShape s{};
        s.packed = true; s.B = B; s.rows = rows; s.taps = 1; s.cin = cin; s.cout = cout; s.has_k = true; s.kgran = 1; s.shift_classes = 1;
        s.residual = residual != 0; s.scale = scale != 0; s.math = 1; s.stream_rows = 512;
        const bool plannable = rows > 0 && cout > 0;         // (the chooser divides by the row and column blocks: no plan without them)
        const ConvPlan p = plannable ? conv_plan_packed_gated(s) : ConvPlan{};
        printf("%d %d %d %d %d %d %d %d %s %d %d %d %d %d %ld %ld %ld %ld\n", B, rows, cin, cout, residual, scale, conv_packed_gated_ok(s) ? 1 : 0,
               conv_packed_gated_shape_ok(s) ? 1 : 0, conv_plan_name(p).c_str(), conv_gated_built(p) ? 1 : 0, p.bn, p.ntn, p.bm, p.mtn, p.grid,
               p.lds_bytes, plannable ? conv_plan_tile(s).lds_bytes : 0L, conv_weight_elems(s));
    }
    return 0;
}
