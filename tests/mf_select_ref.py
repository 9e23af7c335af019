"""An independent mirror of the launch choice of the multifrontal path (csrc/mf_select.cpp), written from the rules and not
from the C++: the switches as the library parses them from the environment, the front kernel of a factor launch, the
kernels of the solve launches, and when two factor launches count as the same selection.  The CPU tests compare the
stand-alone program tests/select_smoke.cpp and the hook sqphip_mf_factor_kernels with it."""
from __future__ import annotations

import re
from types import SimpleNamespace

R1 = "k_mf_factor<256, true>"
# the census of sqphip_mf_census, in its order
KERNEL_NAMES = (
    ["k_mf_values", R1]
    + [f"k_mf_factor2<{nw}, {maxt}, {img}>" for nw, maxt, img in ((1, 3, "true"), (2, 5, "true"), (4, 4, "true"), (4, 9, "false"), (8, 12, "false"))]
    + [f"k_mf_front<{t}, 1, true>" for t in (1, 2, 3)]
    + [f"k_mf_front<{t}, {nw}, true>" for t in (4, 5) for nw in (2, 4)]
    + [f"k_mf_front<{t}, {nw}, {img}>" for t in (6, 7, 8) for nw, img in ((4, "false"), (4, "true"), (8, "true"))]
    + [f"k_mf_front<{t}, 8, false>" for t in (9, 10, 11, 12)]
    + ["k_mf_spine", "k_mf_fwd", "k_mf_fwd2<false>", "k_mf_fwd2<true>", "k_mf_solve_top", "k_mf_solve_top2", "k_mf_bwd",
       "k_mf_bwd2<false>", "k_mf_bwd2<true>", "k_inertia"])
FACTOR_SIDE = [k for k in KERNEL_NAMES if k.startswith(("k_mf_factor", "k_mf_front", "k_mf_spine"))]


def atoi(text):
    """C's atoi: leading blanks, a sign, digits; anything else ends the number, no digits give 0"""
    m = re.match(r"\s*([+-]?\d+)", text)
    return int(m.group(1)) if m else 0


def switches(env):
    """The launch-time switches from an environment {name: value}: present / not "0" / "1" / a number, as each one is read"""
    def num(name, unset):
        return atoi(env[name]) if name in env else unset

    def not0(name):
        return not (name in env and atoi(env[name]) == 0)

    return SimpleNamespace(
        values_serial=num("SQPHIP_MF_VALUES_SERIAL", 0) != 0, v1="SQPHIP_MF_V1" in env, stat=not0("SQPHIP_MF_STATIC"),
        f2_packed=not0("SQPHIP_MF_F2_PACKED"), front_packed=not0("SQPHIP_MF_FRONT_PACKED"),
        static_min=num("SQPHIP_MF_STATIC_MIN", None), static_max=num("SQPHIP_MF_STATIC_MAX", 12), nw4=num("SQPHIP_MF_NW4", 3),
        nw8=not0("SQPHIP_MF_NW8"), big_ldsimg=not0("SQPHIP_MF_BIG_LDSIMG"), generic=num("SQPHIP_MF_GENERIC", 0),
        level2=not0("SQPHIP_MF_LEVEL2"), inertia_kernel="SQPHIP_MF_INERTIA_KERNEL" in env,
        inertia_serial=num("SQPHIP_INERTIA_SERIAL", 0) != 0)


def plan_switches(env):
    def num(name, unset):
        return atoi(env[name]) if name in env else unset

    def not0(name):
        return not (name in env and atoi(env[name]) == 0)

    return SimpleNamespace(
        big_solve=not0("SQPHIP_MF_BIG_SOLVE"), top=num("SQPHIP_MF_TOP", None), top_narrow="SQPHIP_MF_TOP_NARROW" in env,
        merge_t=num("SQPHIP_MF_MERGE_T", None), no_level_merge="SQPHIP_MF_NO_LEVEL_MERGE" in env, top2=not0("SQPHIP_MF_TOP2"),
        spine=num("SQPHIP_MF_SPINE", 0) == 1, defer=num("SQPHIP_MF_DEFER", 1), sym_dump="SQPHIP_SYM_DUMP" in env)


def select_front(tiles, small, narrow, big_lds, sw):
    """(census name, packed LDS image) of a factor launch of `tiles` tile rows"""
    if sw.v1 or tiles > 13:
        return R1, False
    static_min = sw.static_min if sw.static_min is not None else (1 if small and narrow else 4)
    if not sw.stat or tiles > min(sw.static_max, 12) or tiles < static_min:
        for upto, nw, maxt, img in ((2, 1, 3, True), (4, 2, 5, True), (5, 4, 4, True), (8, 4, 9, False), (13, 8, 12, False)):
            if tiles <= upto:
                return f"k_mf_factor2<{nw}, {maxt}, {'true' if img else 'false'}>", img and sw.f2_packed
    if tiles <= 3:
        nw, img = 1, True
    elif tiles <= 5:
        nw4 = sw.nw4 if small else 0
        nw, img = (4 if nw4 & (1 << (tiles - 4)) else 2), True
    elif tiles <= 8:
        img = bool(small and big_lds and sw.big_ldsimg)
        nw = (8 if sw.nw8 else 4) if img else 4
    else:
        nw, img = 8, False
    return f"k_mf_front<{tiles}, {nw}, {'true' if img else 'false'}>", img and sw.front_packed


def same_selection(a, b):
    """two launches (tiles, small, narrow) between which the deferral pass may move a front"""
    return a[0] == b[0] and a[1] == b[1] and (a[0] >= 4 or a[2] == b[2])


def select_solve_level(wimg, hasbig, sw):
    """(forward, backward) kernel of the level launches"""
    if sw.level2 and not sw.generic and wimg >= 0:
        t = "true" if hasbig else "false"
        return f"k_mf_fwd2<{t}>", f"k_mf_bwd2<{t}>"
    return "k_mf_fwd", "k_mf_bwd"


def select_top(top_n, top_count, sw):
    if top_n > 0 and not sw.generic:
        return "k_mf_solve_top2"
    return "k_mf_solve_top" if top_count > 0 else "none"


def top_tests_inertia(sparse, top_n, sw):
    return bool(sparse and top_n > 0 and not sw.generic and not sw.inertia_kernel)
