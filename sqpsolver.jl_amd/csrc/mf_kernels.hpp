// mf_kernels.hpp -- the ONE list of the kernel instantiations of the multifrontal path that the launch census counts
// (Ctx::mf_census, incremented at enqueue; read by the test hook sqphip_mf_census).  Plain C++, no HIP: the host-only choice
// (mf_select.cpp) and the launches (mfront.hip) both expand it.  The order is the census order.
//   K(id, name)                 a kernel with one launch site of its own
//   F2(id, NW, MAXT, IMG)       k_mf_factor2<NW, MAXT, IMG, *>: the generic front kernels
//   FRONT(id, T, NW, IMG)       k_mf_front<T, NW, IMG, *>: the static front kernels (T tile rows, NW waves, image in LDS)
// (the last template argument, the packed LDS image, is a launch-time choice under the same census entry)
// A new static front kernel is a row here and a line in mf_select_front (mf_select.cpp): the enum, the names, the census
// look-ups, the launch switch of mf_factor and the 160 KB attribute of mf_device_setup follow from the row.
#pragma once

#define MF_KERNEL_LIST(K, F2, FRONT) \
    K(MFK_VALUES, "k_mf_values") \
    K(MFK_FACTOR_R1, "k_mf_factor<256, true>") \
    F2(MFK_F2_1_3, 1, 3, true) \
    F2(MFK_F2_2_5, 2, 5, true) \
    F2(MFK_F2_4_4, 4, 4, true) \
    F2(MFK_F2_4_9, 4, 9, false) \
    F2(MFK_F2_8_12, 8, 12, false) \
    FRONT(MFK_FRONT_1, 1, 1, true) \
    FRONT(MFK_FRONT_2, 2, 1, true) \
    FRONT(MFK_FRONT_3, 3, 1, true) \
    FRONT(MFK_FRONT_4_2, 4, 2, true) \
    FRONT(MFK_FRONT_4_4, 4, 4, true) \
    FRONT(MFK_FRONT_5_2, 5, 2, true) \
    FRONT(MFK_FRONT_5_4, 5, 4, true) \
    FRONT(MFK_FRONT_6_4, 6, 4, false) \
    FRONT(MFK_FRONT_6_4_IMG, 6, 4, true) \
    FRONT(MFK_FRONT_6_8_IMG, 6, 8, true) \
    FRONT(MFK_FRONT_7_4, 7, 4, false) \
    FRONT(MFK_FRONT_7_4_IMG, 7, 4, true) \
    FRONT(MFK_FRONT_7_8_IMG, 7, 8, true) \
    FRONT(MFK_FRONT_8_4, 8, 4, false) \
    FRONT(MFK_FRONT_8_4_IMG, 8, 4, true) \
    FRONT(MFK_FRONT_8_8_IMG, 8, 8, true) \
    FRONT(MFK_FRONT_9, 9, 8, false) \
    FRONT(MFK_FRONT_10, 10, 8, false) \
    FRONT(MFK_FRONT_11, 11, 8, false) \
    FRONT(MFK_FRONT_12, 12, 8, false) \
    K(MFK_SPINE, "k_mf_spine") \
    K(MFK_FWD, "k_mf_fwd") \
    K(MFK_FWD2, "k_mf_fwd2<false>") \
    K(MFK_FWD2_BIG, "k_mf_fwd2<true>") \
    K(MFK_SOLVE_TOP, "k_mf_solve_top") \
    K(MFK_SOLVE_TOP2, "k_mf_solve_top2") \
    K(MFK_BWD, "k_mf_bwd") \
    K(MFK_BWD2, "k_mf_bwd2<false>") \
    K(MFK_BWD2_BIG, "k_mf_bwd2<true>") \
    K(MFK_INERTIA, "k_inertia")
#define MF_ROW_SKIP(...)

namespace sqphip {

#define MF_ROW_ID(id, ...) id,
enum MfKernel { MF_KERNEL_LIST(MF_ROW_ID, MF_ROW_ID, MF_ROW_ID) MFK_COUNT };
#undef MF_ROW_ID
extern const char *const mf_kernel_names[MFK_COUNT];        // mf_select.cpp: the row's name, or the instantiation as written

// the census entry of an instantiation; -1: not in the list (the callers static_assert on it: no counter, no launch)
constexpr int mf_front_kid(int T, int NW, bool IMG)
{
#define MF_ROW_MATCH(id, t, nw, img) if (T == t && NW == nw && IMG == img) return id;
    MF_KERNEL_LIST(MF_ROW_SKIP, MF_ROW_SKIP, MF_ROW_MATCH)
    return -1;
}
constexpr int mf_factor2_kid(int NW, int MAXT, bool IMG)
{
#define MF_ROW_MATCH2(id, nw, maxt, img) if (NW == nw && MAXT == maxt && IMG == img) return id;
    MF_KERNEL_LIST(MF_ROW_SKIP, MF_ROW_MATCH2, MF_ROW_SKIP)
    return -1;
}
#undef MF_ROW_MATCH
#undef MF_ROW_MATCH2

}  // namespace sqphip
