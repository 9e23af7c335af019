"""CPU tests (no GPU) of the deferral pass of the multifrontal plan (mf_build_plan, SQPHIP_MF_DEFER): a factor launch whose
fronts can all ride in a later launch of the same kernel, below their parents, is dissolved.  On every family of
tests/mf_structures.py and on the IEEE-14 / -118 / 1354-bus shapes, at a small batch (levels merged up to four tiles) and a
large one: the schedule stays a schedule (every front once, children before parents), a moved front keeps everything that
selects its kernel, and the pass never adds a launch.  With the switch at 0 the IEEE-118 table is the one the schedule had
before the pass existed; by default it loses the two launches that held three fronts with slack."""
import numpy as np
import pytest

import sqpsolver_jl_amd as pkg
from sqpsolver_jl_amd.acopf_synth import acopf_synth, acopf_layout, CASES
import mf_structures as MS
from mf_defer_structures import defer_leaf

BATCHES = (5, 128)
SETTINGS = (None, "2")                # default (destination: the latest launch allowed) and the widest own front


def _case(name):
    nb, ng, nl, seed = CASES[name]
    lay = acopf_layout(acopf_synth(nb, ng, nl, seed))
    lay.name = name
    return lay


STRUCTURES = MS.families() + [defer_leaf()] + [_case(c) for c in ("case14", "case118", "case1354")]
_CACHE = {}


def _plan(S, batch, defer, monkeypatch):
    """(fronts (columns, rows, level), launches (level, tiles, fronts, smallest tiles), per front (launch, launch before the
    pass, parent)) under SQPHIP_MF_DEFER = defer (None: unset); computed once per structure, batch and setting"""
    key = (S.name, batch, defer)
    if key not in _CACHE:
        if defer is None:
            monkeypatch.delenv("SQPHIP_MF_DEFER", raising=False)
        else:
            monkeypatch.setenv("SQPHIP_MF_DEFER", defer)
        args = (S.n, S.m, S.jrow, S.jcol, S.hrow, S.hcol, S.gL, S.gU, 1, batch)
        fr, la, _, _ = pkg.mf_plan_info(*args)
        _CACHE[key] = (fr, la, pkg.mf_front_launches(*args))
    return _CACHE[key]


def _narrow_level(fr):
    """first level of the narrow top of the tree by the rule of mf_build_plan: from the top downwards, the levels of at most
    two fronts, or of up to four fronts of at most 64 rows each; at least two such levels, else there is no narrow top"""
    nlev = int(fr[:, 2].max()) + 1
    l = nlev
    while l > 0:
        on = fr[fr[:, 2] == l - 1]
        if not (len(on) <= 2 or (len(on) <= 4 and (on[:, 0] + on[:, 1]).max() <= 64)):
            break
        l -= 1
    return l if nlev - l >= 2 else nlev


@pytest.mark.parametrize("defer", SETTINGS, ids=["latest", "widest"])
@pytest.mark.parametrize("batch", BATCHES)
def test_the_deferred_schedule_is_a_schedule_of_the_same_kernels(batch, defer, monkeypatch):
    moved_total = 0
    for S in STRUCTURES:
        fr0, la0, fl0 = _plan(S, batch, "0", monkeypatch)
        fr, la, fl = _plan(S, batch, defer, monkeypatch)
        ns = len(fr)
        assert np.array_equal(fr, fr0) and np.array_equal(fl0[:, 0], fl0[:, 1]) and np.array_equal(fl[:, 2], fl0[:, 2]), S.name
        # the launches before the pass are the rows of the table under 0, whatever the setting
        assert np.array_equal(fl[:, 1], fl0[:, 0]), S.name
        # every front in exactly one launch, and the launches hold what the table says
        assert fl[:, 0].min() >= 0 and fl[:, 0].max() < len(la), S.name
        assert np.array_equal(np.bincount(fl[:, 0], minlength=len(la)), la[:, 2]) and la[:, 2].min() >= 1, S.name
        assert la[:, 2].sum() == ns, S.name
        # after each child's launch, hence before the parent's
        kids = np.flatnonzero(fl[:, 2] >= 0)
        assert np.all(fl[kids, 0] < fl[fl[kids, 2], 0]), S.name
        assert np.all(fr[kids, 2] < fr[fl[kids, 2], 2]), S.name
        # never more launches, and the launches that remain are rows of the old table in the old order: level, tiles
        assert len(la) <= len(la0), S.name
        key0 = {(int(r[0]), int(r[1])): j for j, r in enumerate(la0)}
        assert len(key0) == len(la0), S.name                       # (level, tiles) names a launch
        orig = [key0[(int(r[0]), int(r[1]))] for r in la]
        assert orig == sorted(orig), S.name
        # a front that stayed is where it was; a moved one went to a later level below its parent's, into a launch with the
        # tiles and the selection flags of its source: at most eight fronts before the pass, and below four tiles the same
        # side of the narrow top
        narrow = _narrow_level(fr)
        for s in range(ns):
            src, dst = la0[fl[s, 1]], la0[orig[fl[s, 0]]]
            if fl[s, 1] == orig[fl[s, 0]]:
                continue
            moved_total += 1
            assert src[0] == fr[s, 2] and dst[0] > src[0], (S.name, s)
            assert fl[s, 2] < 0 or dst[0] < fr[fl[s, 2], 2], (S.name, s)
            assert dst[1] == src[1] and (dst[2] <= 8) == (src[2] <= 8), (S.name, s)
            assert src[1] >= 4 or (src[0] >= narrow) == (dst[0] >= narrow), (S.name, s)
            # its source launch is gone altogether
            assert not np.any(np.array(orig) == fl[s, 1]), (S.name, s)
    assert moved_total > 0


def test_switch_off_gives_the_ieee118_table_entry_for_entry(monkeypatch):
    _, la0, fl0 = _plan(_case("case118"), 128, "0", monkeypatch)
    assert len(la0) == 18
    assert la0[:, 0].tolist() == [0, 0, 1, 1, 2, 2, 2, 2] + list(range(3, 13))
    assert la0[:, 1].tolist() == [2, 3, 2, 3, 2, 3, 4, 5, 3, 4, 5, 5, 6, 5, 6, 6, 7, 5]
    assert np.array_equal(fl0[:, 0], fl0[:, 1])


@pytest.mark.parametrize("defer", SETTINGS, ids=["latest", "widest"])
def test_ieee118_loses_two_launches_and_moves_three_fronts(defer, monkeypatch):
    S = _case("case118")
    _, la0, _ = _plan(S, 128, "0", monkeypatch)
    fr, la, fl = _plan(S, 128, defer, monkeypatch)
    assert len(la) == 16
    key = {(int(r[0]), int(r[1])): k for k, r in enumerate(la)}
    moved = [s for s in range(len(fr)) if key.get((int(la0[fl[s, 1], 0]), int(la0[fl[s, 1], 1]))) != fl[s, 0]]
    assert sorted((int(fr[s, 0]), int(fr[s, 1])) for s in moved) == [(20, 12), (22, 46), (32, 34)]
    # the launches that went: the T = 3 launch of level 0 (one leaf) and the T = 5 launch of level 2 (two fronts)
    assert sorted({(int(la0[fl[s, 1], 0]), int(la0[fl[s, 1], 1])) for s in moved}) == [(0, 3), (2, 5)]


@pytest.mark.parametrize("batch", BATCHES)
def test_case1354_has_fewer_launches(batch, monkeypatch):
    S = _case("case1354")
    assert len(_plan(S, batch, None, monkeypatch)[1]) < len(_plan(S, batch, "0", monkeypatch)[1])


@pytest.mark.parametrize("batch", BATCHES)
def test_the_synthetic_leaf_with_slack_rides_with_the_front_above_it(batch, monkeypatch):
    """tests/mf_defer_structures.py: five launches become four, and the front that moves is the leaf of 56 x 8 whose parent
    sits two levels up"""
    S = defer_leaf()
    fr, la0, _ = _plan(S, batch, "0", monkeypatch)
    _, la, fl = _plan(S, batch, None, monkeypatch)
    assert (len(la0), len(la)) == S.target["launches"]
    s = int(np.flatnonzero((fr[:, 0] == 56) & (fr[:, 1] == 8))[0])
    assert fr[s, 2] == 0 and fr[fl[s, 2], 2] == 2 and tuple(la0[fl[s, 1]][:3]) == (0, 5, 1) and tuple(la[fl[s, 0]][:3]) == (1, 5, 2)
