// mf_select.cpp -- host only, plain C++ (no HIP): the switches of the multifrontal path and the choice of kernel per launch
// (mf_select.hpp).  Compiled into the library, and on its own under sanitizers by tests/test_mf_select_cpu.py.
#include "mf_select.hpp"
#include <algorithm>
#include <cstdlib>

namespace sqphip {

#define MF_ROW_NAME(id, name) name,
#define MF_ROW_F2_NAME(id, NW, MAXT, IMG) "k_mf_factor2<" #NW ", " #MAXT ", " #IMG ">",
#define MF_ROW_FRONT_NAME(id, T, NW, IMG) "k_mf_front<" #T ", " #NW ", " #IMG ">",
const char *const mf_kernel_names[MFK_COUNT] = { MF_KERNEL_LIST(MF_ROW_NAME, MF_ROW_F2_NAME, MF_ROW_FRONT_NAME) };

namespace {
bool env_set(const char *name) { return getenv(name) != nullptr; }
int env_int(const char *name, int unset) { const char *e = getenv(name); return e ? atoi(e) : unset; }
bool env_not0(const char *name) { const char *e = getenv(name); return !(e && atoi(e) == 0); }      // on unless "0" (or no number)
bool env_is1(const char *name) { return env_int(name, 0) == 1; }
}  // namespace

MfSwitches mf_read_switches()
{
    MfSwitches sw;
    sw.values_serial = env_int("SQPHIP_MF_VALUES_SERIAL", 0) != 0;
    sw.v1 = env_set("SQPHIP_MF_V1");
    sw.stat = env_not0("SQPHIP_MF_STATIC");
    sw.f2_packed = env_not0("SQPHIP_MF_F2_PACKED");
    sw.front_packed = env_not0("SQPHIP_MF_FRONT_PACKED");
    if (env_set("SQPHIP_MF_STATIC_MIN")) sw.static_min = std::max(0, env_int("SQPHIP_MF_STATIC_MIN", 0));
    sw.static_max = env_int("SQPHIP_MF_STATIC_MAX", sw.static_max);
    sw.nw4 = env_int("SQPHIP_MF_NW4", sw.nw4);
    sw.nw8 = env_not0("SQPHIP_MF_NW8");
    sw.big_ldsimg = env_not0("SQPHIP_MF_BIG_LDSIMG");
    sw.generic = env_int("SQPHIP_MF_GENERIC", 0);
    sw.level2 = env_not0("SQPHIP_MF_LEVEL2");
    sw.inertia_kernel = env_set("SQPHIP_MF_INERTIA_KERNEL");
    sw.inertia_serial = env_int("SQPHIP_INERTIA_SERIAL", 0) != 0;
    return sw;
}

MfPlanSwitches mf_read_plan_switches()
{
    MfPlanSwitches sw;
    sw.big_solve = env_not0("SQPHIP_MF_BIG_SOLVE");
    sw.top = env_int("SQPHIP_MF_TOP", -1);
    sw.top_narrow = env_set("SQPHIP_MF_TOP_NARROW");
    if (env_set("SQPHIP_MF_MERGE_T")) sw.merge_t = std::max(0, env_int("SQPHIP_MF_MERGE_T", 0));
    sw.no_level_merge = env_set("SQPHIP_MF_NO_LEVEL_MERGE");
    sw.top2 = env_not0("SQPHIP_MF_TOP2");
    sw.spine = env_is1("SQPHIP_MF_SPINE");
    sw.defer = env_int("SQPHIP_MF_DEFER", sw.defer);
    sw.sym_dump = env_set("SQPHIP_SYM_DUMP");
    return sw;
}

// the census entry of an instantiation of the list; one that is not there does not compile
#define MF_FRONT(T, NW, IMG) ([] { constexpr int k = mf_front_kid(T, NW, IMG); static_assert(k >= 0, "k_mf_front<" #T ", " #NW ", " #IMG ">: no row in MF_KERNEL_LIST"); return MfKernel(k); }())
#define MF_F2(NW, MAXT, IMG) ([] { constexpr int k = mf_factor2_kid(NW, MAXT, IMG); static_assert(k >= 0, "k_mf_factor2<" #NW ", " #MAXT ", " #IMG ">: no row in MF_KERNEL_LIST"); return MfKernel(k); }())

MfFrontChoice mf_select_front(int T, bool small, bool narrow, bool big_lds, const MfSwitches &sw)
{
    if (sw.v1 || T > 13) return {MFK_FACTOR_R1, false};
    const int static_min = sw.static_min >= 0 ? sw.static_min : (small && narrow ? 1 : 4);
    if (!sw.stat || T > sw.static_max || T > 12 || T < static_min) {
        // the generic kernels, by class of front height; the image of the lower three lives in LDS
        if (T <= 2) return {MF_F2(1, 3, true), sw.f2_packed};
        if (T <= 4) return {MF_F2(2, 5, true), sw.f2_packed};
        if (T <= 5) return {MF_F2(4, 4, true), sw.f2_packed};
        if (T <= 8) return {MF_F2(4, 9, false), false};
        return {MF_F2(8, 12, false), false};
    }
    const int nw4 = small ? sw.nw4 : 0;
    const bool img = small && big_lds && sw.big_ldsimg;         // six to eight tile rows: image in LDS
    const bool p = sw.front_packed;
    switch (T) {
    case 1: return {MF_FRONT(1, 1, true), p};
    case 2: return {MF_FRONT(2, 1, true), p};
    case 3: return {MF_FRONT(3, 1, true), p};
    case 4: return {(nw4 & 1) ? MF_FRONT(4, 4, true) : MF_FRONT(4, 2, true), p};
    case 5: return {(nw4 & 2) ? MF_FRONT(5, 4, true) : MF_FRONT(5, 2, true), p};
    case 6: return img ? MfFrontChoice{sw.nw8 ? MF_FRONT(6, 8, true) : MF_FRONT(6, 4, true), p} : MfFrontChoice{MF_FRONT(6, 4, false), false};
    case 7: return img ? MfFrontChoice{sw.nw8 ? MF_FRONT(7, 8, true) : MF_FRONT(7, 4, true), p} : MfFrontChoice{MF_FRONT(7, 4, false), false};
    case 8: return img ? MfFrontChoice{sw.nw8 ? MF_FRONT(8, 8, true) : MF_FRONT(8, 4, true), p} : MfFrontChoice{MF_FRONT(8, 4, false), false};
    case 9: return {MF_FRONT(9, 8, false), false};
    case 10: return {MF_FRONT(10, 8, false), false};
    case 11: return {MF_FRONT(11, 8, false), false};
    default: return {MF_FRONT(12, 8, false), false};
    }
}
#undef MF_FRONT
#undef MF_F2

bool mf_same_selection(const MfLaunch &a, const MfLaunch &b, int narrow_level)
{
    return a.tiles == b.tiles && a.small == b.small &&
           (a.tiles >= 4 || mf_launch_narrow(a, narrow_level) == mf_launch_narrow(b, narrow_level));
}

MfKernel mf_select_solve_level(int wimg, bool hasbig, const MfSwitches &sw)
{
    return sw.level2 && !sw.generic && wimg >= 0 ? (hasbig ? MFK_FWD2_BIG : MFK_FWD2) : MFK_FWD;
}

MfKernel mf_bwd_of(MfKernel fwd) { return fwd == MFK_FWD2_BIG ? MFK_BWD2_BIG : fwd == MFK_FWD2 ? MFK_BWD2 : MFK_BWD; }

MfKernel mf_select_top(int top_n, int top_count, const MfSwitches &sw)
{
    return top_n > 0 && !sw.generic ? MFK_SOLVE_TOP2 : top_count > 0 ? MFK_SOLVE_TOP : MFK_COUNT;
}

bool mf_top_tests_inertia(bool sparse, int top_n, const MfSwitches &sw)
{
    return !sw.inertia_kernel && sparse && top_n > 0 && !sw.generic;
}

}  // namespace sqphip
