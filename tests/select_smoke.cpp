// select_smoke.cpp -- the launch choice of the multifrontal path (csrc/mf_select.cpp) on its own (no device, no library):
// sets the environment from its arguments, reads the switches as the library does and prints the choice over the whole
// domain.  tests/test_mf_select_cpu.py compiles it together with mf_select.cpp under the address and undefined-behaviour
// sanitizers and compares every line with tests/mf_select_ref.py.
//   usage:  select_smoke <sections: letters of n f p s w> [NAME=VALUE ...]
//   output, tab separated:
//     n  "name <index> <census name>"
//     f  "front <tiles> <small> <narrow> <big_lds> <census name> <packed>"            tiles 1 .. 15
//     p  "same <tiles a> <small a> <narrow a> <tiles b> <small b> <narrow b> <0|1>"     every pair of launch descriptors
//     s  "level <wimg> <hasbig> <forward> <backward>", "top <top_n> <top_count> <name|none>", "inertia <sparse> <top_n> <0|1>"
//     w  "switch <field> <value>" and "plan <field> <value>"
#include "../sqpsolver.jl_amd/csrc/mf_select.hpp"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

using namespace sqphip;

int main(int argc, char **argv)
{
    if (argc < 2) { std::fprintf(stderr, "usage: select_smoke <sections> [NAME=VALUE ...]\n"); return 2; }
    for (int k = 2; k < argc; ++k) {
        const char *eq = std::strchr(argv[k], '=');
        if (!eq) { std::fprintf(stderr, "select_smoke: %s: not NAME=VALUE\n", argv[k]); return 2; }
        if (setenv(std::string(argv[k], (size_t)(eq - argv[k])).c_str(), eq + 1, 1) != 0) return 2;
    }
    const MfSwitches sw = mf_read_switches();
    const MfPlanSwitches ps = mf_read_plan_switches();
    auto has = [&](char c) { return std::strchr(argv[1], c) != nullptr; };
    auto name = [](MfKernel k) { return k == MFK_COUNT ? "none" : mf_kernel_names[k]; };
    if (has('n'))
        for (int k = 0; k < MFK_COUNT; ++k) std::printf("name\t%d\t%s\n", k, mf_kernel_names[k]);
    if (has('f'))
        for (int T = 1; T <= 15; ++T)
            for (int small = 0; small < 2; ++small)
                for (int narrow = 0; narrow < 2; ++narrow)
                    for (int big = 0; big < 2; ++big) {
                        const MfFrontChoice c = mf_select_front(T, small != 0, narrow != 0, big != 0, sw);
                        std::printf("front\t%d\t%d\t%d\t%d\t%s\t%d\n", T, small, narrow, big, name(c.kid), (int)c.packed);
                    }
    if (has('p')) {
        // a launch of the narrow top is one at level 1 with the narrow top starting there
        auto launch = [](int T, int small, int narrow) { MfLaunch L{0, 1, 0, 0, 0, T}; L.small = small; L.level = narrow; return L; };
        for (int a = 0; a < 60; ++a)
            for (int b = 0; b < 60; ++b) {
                const MfLaunch A = launch(1 + a / 4, (a >> 1) & 1, a & 1), B = launch(1 + b / 4, (b >> 1) & 1, b & 1);
                std::printf("same\t%d\t%d\t%d\t%d\t%d\t%d\t%d\n", A.tiles, A.small, A.level, B.tiles, B.small, B.level, (int)mf_same_selection(A, B, 1));
            }
    }
    if (has('s')) {
        for (int wimg : {-1, 0, 100})
            for (int hasbig = 0; hasbig < 2; ++hasbig) {
                const MfKernel f = mf_select_solve_level(wimg, hasbig != 0, sw);
                std::printf("level\t%d\t%d\t%s\t%s\n", wimg, hasbig, name(f), name(mf_bwd_of(f)));
            }
        for (int top_n : {0, 3})
            for (int top_count : {0, 3}) std::printf("top\t%d\t%d\t%s\n", top_n, top_count, name(mf_select_top(top_n, top_count, sw)));
        for (int sparse = 0; sparse < 2; ++sparse)
            for (int top_n : {0, 3}) std::printf("inertia\t%d\t%d\t%d\n", sparse, top_n, (int)mf_top_tests_inertia(sparse != 0, top_n, sw));
    }
    if (has('w')) {
        std::printf("switch\tvalues_serial\t%d\nswitch\tv1\t%d\nswitch\tstat\t%d\nswitch\tf2_packed\t%d\nswitch\tfront_packed\t%d\n",
                    (int)sw.values_serial, (int)sw.v1, (int)sw.stat, (int)sw.f2_packed, (int)sw.front_packed);
        std::printf("switch\tstatic_min\t%d\nswitch\tstatic_max\t%d\nswitch\tnw4\t%d\nswitch\tnw8\t%d\nswitch\tbig_ldsimg\t%d\n",
                    sw.static_min, sw.static_max, sw.nw4, (int)sw.nw8, (int)sw.big_ldsimg);
        std::printf("switch\tgeneric\t%d\nswitch\tlevel2\t%d\nswitch\tinertia_kernel\t%d\nswitch\tinertia_serial\t%d\n",
                    sw.generic, (int)sw.level2, (int)sw.inertia_kernel, (int)sw.inertia_serial);
        std::printf("plan\tbig_solve\t%d\nplan\ttop\t%d\nplan\ttop_narrow\t%d\nplan\tmerge_t\t%d\nplan\tno_level_merge\t%d\n",
                    (int)ps.big_solve, ps.top, (int)ps.top_narrow, ps.merge_t, (int)ps.no_level_merge);
        std::printf("plan\ttop2\t%d\nplan\tspine\t%d\nplan\tdefer\t%d\nplan\tsym_dump\t%d\n", (int)ps.top2, (int)ps.spine, ps.defer, (int)ps.sym_dump);
    }
    return 0;
}
