// Host-only driver of csrc/ldn_dense_plan.h for tests/test_dense_plan.py (and for finding the smallest shape that reaches a kernel).
//   dense_plan_cli sweep    the chooser over a grid of shapes: one line "<kernel> <cases>" per row of LDN_DENSE_KERNELS, one line
//                           "UNBUILT <kernel> <shape>" per plan that names no row; exit status 1 if there is such a plan or an unreached row
//   dense_plan_cli          stdin: lines "<form> <taps> <cin> <cout> <m_cap> <counted> <hint> <gate_rows>" (form: plain, or flags of
//                           f32 / ps / of / pool / feat / gated joined by '+'; '#' lines and blank lines pass through); stdout: the
//                           same lines with the chosen kernel appended
#include <stdlib.h>
#include <string.h>

#include <map>
#include <string>

#include "../laudnet_amd/csrc/ldn_dense_plan.h"

using namespace ldn;

static DenseShape shape(const char* form, int taps, int cin, int cout, int m_cap, bool counted, long hint, int gate_rows) {
    DenseShape s{};
    s.taps = taps; s.cin = cin; s.cout = cout; s.m_cap = m_cap;
    s.rows_known = dense_rows_known(m_cap, counted, hint);
    auto has = [&](const char* flag) { return strstr(form, flag) != nullptr; };
    s.f32 = has("f32"); s.ps = has("ps"); s.of = has("of"); s.pool = has("pool"); s.feat = has("feat"); s.gated = has("gated");
    if (s.gated) { s.rows_known = -1; s.gate_bytes = dense_gate_bytes(gate_rows, cin); }      // (the gated form reads no hint)
    return s;
}

static bool built(const DensePlan& k) {      // is the plan a row of the list?
#define ROW1(...) if (k == LDN_DENSE_ROW1(__VA_ARGS__)) return true;
#define ROW2(...) if (k == LDN_DENSE_ROW2(__VA_ARGS__)) return true;
    LDN_DENSE_KERNELS(ROW1, ROW2)
#undef ROW1
#undef ROW2
    return false;
}

static int sweep() {
    std::map<std::string, long> reached;
    size_t rows = 0;      // (a row listed twice would not compile into two kernels: counted here, compared below)
#define ROW1(...) ++rows, reached[dense_plan_name(LDN_DENSE_ROW1(__VA_ARGS__))] = 0;
#define ROW2(...) ++rows, reached[dense_plan_name(LDN_DENSE_ROW2(__VA_ARGS__))] = 0;
    LDN_DENSE_KERNELS(ROW1, ROW2)
    long cases = 0, unbuilt = 0;
    auto visit = [&](const char* form, int taps, int cin, int cout, int m_cap, int counted, long hint, int gate_rows) {
        const DenseShape s = shape(form, taps, cin, cout, m_cap, counted, hint, gate_rows);
        const DensePlan k = dense_plan(s);
        ++cases;
        if (built(k)) { ++reached[dense_plan_name(k)]; return; }
        ++unbuilt;
        printf("UNBUILT %s %s %d %d %d %d %d %ld %d\n", dense_plan_name(k).c_str(), form, taps, cin, cout, m_cap, counted, hint, gate_rows);
    };
    const int cins[] = {32, 64, 72, 144, 256, 320, 512, 784, 1024, 2048, 2112};
    const int couts[] = {32, 64, 96, 128, 144, 160, 168, 216, 256, 320, 384, 512, 784, 1024, 2048};
    const int caps[] = {1, 256, 3136, 12544, 50176, 200704, 802816};
    const char* forms1[] = {"plain", "feat", "f32", "f32+feat", "pool", "f32+pool", "ps", "of"};      // what the entry points accept with taps == 1 ...
    const char* forms9[] = {"plain", "feat", "f32", "f32+feat"};                                      // ... and with the neighbour table
    for (int cin : cins) for (int cout : couts) for (int cap : caps) for (int counted = 0; counted < 2; ++counted)
        for (long hint : {-1L, 0L, 100L, (long)cap / 2, 2L * cap}) {
            for (const char* f : forms1) {      // (what the entry points refuse: pooled means of cout % 128 != 0, pre-split rows of cin % 32 != 0 or cout % 64 != 0)
                if (strstr(f, "pool") ? cout % 128 != 0 : (!strcmp(f, "ps") || !strcmp(f, "of")) && (cin % 32 != 0 || cout % 64 != 0)) continue;
                visit(f, 1, cin, cout, cap, counted, hint, 0);
            }
            for (const char* f : forms9) visit(f, 9, cin, cout, cap, counted, hint, 0);
            for (int gate_rows : {1, 49, 196, 3136}) visit("gated", 1, cin, cout, cap, counted, hint, gate_rows);
        }
    long unreached = 0;
    for (const auto& r : reached) { printf("%s %ld\n", r.first.c_str(), r.second); unreached += r.second == 0; }
    printf("cases %ld rows %zu unbuilt %ld unreached %ld\n", cases, rows, unbuilt, unreached);
    return (unbuilt || unreached || reached.size() != rows) ? 1 : 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && !strcmp(argv[1], "sweep")) return sweep();
    char line[256], form[32];
    while (fgets(line, sizeof line, stdin)) {
        int taps, cin, cout, m_cap, counted, gate_rows;
        long hint;
        line[strcspn(line, "\n")] = 0;
        if (line[0] == '#' || sscanf(line, "%31s %d %d %d %d %d %ld %d", form, &taps, &cin, &cout, &m_cap, &counted, &hint, &gate_rows) != 8) { puts(line); continue; }
        const DenseShape s = shape(form, taps, cin, cout, m_cap, counted, hint, gate_rows > 0 ? gate_rows : 1);
        const DensePlan k = dense_plan(s);
        printf("%s %d %d %d %d %d %ld %d %s%s\n", form, taps, cin, cout, m_cap, counted, hint, gate_rows, dense_plan_name(k).c_str(), built(k) ? "" : " UNBUILT");
    }
    return 0;
}
