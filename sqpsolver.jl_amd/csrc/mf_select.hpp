// mf_select.hpp -- which kernel a launch of the multifrontal path runs: the experiment switches, read in one place, and the
// choice as pure functions of the launch and the switches.  Host only, plain C++ (no HIP): mfront.hip launches what these
// functions name, mfplan.hip builds the plan under MfPlanSwitches, and tests/select_smoke.cpp walks the whole domain without
// a device.
#pragma once
#include "mf_kernels.hpp"
#include "sparse.hpp"

namespace sqphip {

// The launch-time switches (environment; none is needed for normal use).  mf_values, mf_factor, mf_solve and
// mf_solve_tests_inertia read them once per call (mf_read_switches): a process that changes its environment between calls
// -- only tests do -- gets the new setting at the next call, for every switch alike.
//
//   switch                      field          default   meaning, and the measurement behind the default
//   SQPHIP_MF_VALUES_SERIAL=1   values_serial  off       the values by the one-thread-per-destination kernel k_mf_values_serial
//   SQPHIP_MF_V1 (set)          v1             off       cross-check: the plain rank-1 kernel for every front, no values launch, no spine
//   SQPHIP_MF_STATIC=0          stat           on        static front kernels k_mf_front<T, NW, LDSIMG>; 0: the generic ones (cross-check)
//   SQPHIP_MF_F2_PACKED=0       f2_packed      on        LDS image of the generic kernels as packed tiles; 0: the square image
//   SQPHIP_MF_FRONT_PACKED=0    front_packed   on        ... and of the static front kernels (same census entry either way)
//   SQPHIP_MF_STATIC_MIN=t      static_min     -1        static kernels from t tile rows on; unset (-1): from four -- below that the
//       generic kernels are as fast per front and lighter (registers, code size) where thousands of small fronts are in
//       flight.  Measured (QP/s, static from T = 1 / from T = 4 / never): 512 x IEEE-118 5565 / 5507 / 5259, 64 x IEEE-118
//       1372 / - / 1315, 9241 shape 20.6 / 24.3 / 23.4, IEEE-14 50.9 k / 55.4 k / 53.9 k.  Tests run it at 1 to cover every
//       instantiation.  (round 4: on a narrow level -- a handful of fronts, i.e. the levels the spine kernel takes over -- the
//       static kernels run every front, unset means 1 there: the level-launch build, SQPHIP_MF_SPINE=0, then gives the bits
//       of the spine kernel)
//   SQPHIP_MF_STATIC_MAX=t      static_max     12        (round 4: nine to twelve tile rows too -- the fronts of 129 .. 192 rows of
//       the 1354- and 9241-bus shapes --, eight waves, image in the arena: 1354 buses 549 -> 557 QP/s, 9241 buses 28.5 -> 29.2;
//       8 gives them back to the generic kernel)
//   SQPHIP_MF_NW4=bits          nw4            3         four waves instead of two for fronts of four (bit 0) / five (bit 1) tile rows
//       on the levels near the top of the tree (a handful of fronts: latency, not occupancy, is what counts there): 512 x
//       IEEE-118 7 100 -> 7 154 / 7 297 / 7 326 QP/s with bit 0 / bit 1 / both, same bits (0: two waves everywhere)
//   SQPHIP_MF_NW8=0             nw8            on        ... and eight instead of four for six to eight tile rows there: 7 323 -> 7 403
//       QP/s, same bits (0: four)
//   SQPHIP_MF_BIG_LDSIMG=0      big_ldsimg     on        six to eight tile rows: the image fits the 160 KB of LDS of gfx950 too -- 74 /
//       100 / 131 KB square, 43 / 57 / 74 KB packed -- once more than 64 KB of dynamic LDS has been asked for; only for the
//       handful of fronts of a level near the top of the tree, where one workgroup of the square image per CU was all there was
//       anyway: +0.3 % on 512 x IEEE-118; 0: image in the arena.  With the packed image two workgroups of six or seven tile rows
//       fit a CU, so the reason no longer binds there; the rule stands until the wide launches have been measured with the image
//       in LDS: DESIGN.md section 10
//   SQPHIP_MF_GENERIC=g         generic        0         the generic triangular-solve path of k_mf_fwd / k_mf_bwd / k_mf_solve_top (the
//       kernels' `generic` argument) for every level, no streamed top
//   SQPHIP_MF_LEVEL2=0          level2         on        level launches of the solves by the LDS-staged k_mf_fwd2 / k_mf_bwd2 where every
//       front of the level fits them; 0: k_mf_fwd / k_mf_bwd
//   SQPHIP_MF_INERTIA_KERNEL (set)  inertia_kernel  off  experiment: the inertia test by k_inertia instead of inside k_mf_solve_top2
//   SQPHIP_INERTIA_SERIAL=1     inertia_serial off       k_mf_solve_top2 with the former counting loop and order
struct MfSwitches {
    bool values_serial = false, v1 = false, stat = true, f2_packed = true, front_packed = true;
    int static_min = -1, static_max = 12, nw4 = 3;
    bool nw8 = true, big_ldsimg = true;
    int generic = 0;
    bool level2 = true, inertia_kernel = false, inertia_serial = false;
};
MfSwitches mf_read_switches();

// The plan-time switches: mf_build_plan reads them once, at its top (SQPHIP_MF_SMALL_FRONT / _ZERO_FRAC / _ROWS_AFTER are
// options of the symbolic analysis: sparse.hpp, mf_sym_options).
//   SQPHIP_MF_BIG_SOLVE=0       big_solve      on        experiment: 0 = wave-per-front solves for every front, no narrow top
//   SQPHIP_MF_TOP=0|1           top            -1        0: the top of the tree by level launches; 1: keep k_mf_solve_top where the
//       streamed top does not apply (1354-bus shape: 495 -> 524 QP/s for the level launches, hence unset = level launches there)
//   SQPHIP_MF_TOP_NARROW (set)  top_narrow     off       levels of three or four wave-sized fronts do not join the top
//   SQPHIP_MF_MERGE_T=t         merge_t        -1        one launch per level whose tallest front has at most t tiles; unset (-1):
//       SymOptions::merge_tiles (measured in mf_build_plan)
//   SQPHIP_MF_NO_LEVEL_MERGE (set)  no_level_merge  off  a launch per size class on every level
//   SQPHIP_MF_TOP2=0            top2           on        0: no streamed top (k_mf_solve_top2)
//   SQPHIP_MF_SPINE=1           spine          off       the narrow top of the factorisation by k_mf_spine (measured in mf_build_plan)
//   SQPHIP_MF_DEFER=0|1|2       defer          1         the deferral pass: off / the latest launch allowed / the widest (mf_build_plan)
//   SQPHIP_SYM_DUMP (set)       sym_dump       off       the top, the spine and the deferred fronts to stderr
struct MfPlanSwitches {
    bool big_solve = true;
    int top = -1;
    bool top_narrow = false;
    int merge_t = -1;
    bool no_level_merge = false, top2 = true, spine = false;
    int defer = 1;
    bool sym_dump = false;
};
MfPlanSwitches mf_read_plan_switches();

// The kernel of one factor launch: its census entry (the rank-1 kernel, a row F2 or a row FRONT of mf_kernels.hpp) and whether
// the instantiation with the packed LDS image runs.  tiles: 16-row tiles of the launch's kernel (MfLaunch::tiles); small: the
// launch held at most eight fronts when the schedule was built (MfLaunch::small); narrow: its level belongs to the narrow top
// of the tree; big_lds: the device granted 160 KB of dynamic LDS (Ctx::mf_big_lds).
struct MfFrontChoice { MfKernel kid; bool packed; };
MfFrontChoice mf_select_front(int tiles, bool small, bool narrow, bool big_lds, const MfSwitches &sw);

// What the choice takes from the launch itself: tiles, small (static_min, nw4, the LDS image of six to eight tiles) and narrow
// (static_min).  The last one decides nothing from four tiles on: static_min is then 1 or 4 when unset, and a
// SQPHIP_MF_STATIC_MIN holds for every launch alike.  The deferral pass of mf_build_plan moves a front only between launches
// mf_same_selection calls equal, so no front changes kernel: equal launches get the same MfFrontChoice under every setting of
// the switches (tests/test_mf_select_cpu.py holds the two functions to each other over the whole domain).
inline bool mf_launch_narrow(const MfLaunch &L, int narrow_level) { return L.level >= narrow_level; }
bool mf_same_selection(const MfLaunch &a, const MfLaunch &b, int narrow_level);
inline MfFrontChoice mf_select_launch(const MfLaunch &L, int narrow_level, bool big_lds, const MfSwitches &sw)
{
    return mf_select_front(L.tiles, L.small != 0, mf_launch_narrow(L, narrow_level), big_lds, sw);
}
// the spine kernel takes the factor launches from MfPlan::fac_below on when the plan has a spine
inline bool mf_spine_runs(bool plan_has_spine, bool big_lds, const MfSwitches &sw) { return !sw.v1 && plan_has_spine && big_lds; }

// a level launch of the forward solve: MFK_FWD2_BIG / MFK_FWD2 (LDS-staged, wimg >= 0: every front of the level fits) or
// MFK_FWD; the backward launch of the same level runs the mirror
MfKernel mf_select_solve_level(int wimg, bool hasbig, const MfSwitches &sw);
MfKernel mf_bwd_of(MfKernel fwd);
// the top of the tree: MFK_SOLVE_TOP2 (top_n: fronts of the streamed top), MFK_SOLVE_TOP (top_count: work items of the top
// launch), or MFK_COUNT: no top launch
MfKernel mf_select_top(int top_n, int top_count, const MfSwitches &sw);
// the streamed top kernel tests the inertia of the factorised instances itself (otherwise k_inertia does)
bool mf_top_tests_inertia(bool sparse, int top_n, const MfSwitches &sw);

}  // namespace sqphip
