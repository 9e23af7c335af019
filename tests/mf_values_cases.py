"""Structures for the tests of the values kernel (k_mf_values) and its block plan (numpy only): the IEEE-14 and IEEE-118
ACOPF layouts, and synthetic structures in which one destination of the Newton matrix collects exactly K items.

How a destination gets many items: the COO -> CSC conversion sums duplicate Hessian and Jacobian entries into one slot, so
duplicates add no items; in the condensed form every eliminated inequality row adds one item (its clique term) to every
destination among its variables.  items(K): variable 0 has its diagonal term, one Hessian entry and K - 2 inequality rows
of one entry each -- K items on destination (0, 0); two more variables carry 132 items each (together more than a block
of 256), a pair of variables 60 rows of two entries, and most destinations have one item."""
import numpy as np

import mf_structures as MS
from sqpsolver_jl_amd.acopf_synth import acopf_synth, acopf_layout, CASES


def items(K, seed=0):
    b = MS._Builder(seed)
    v = b.vars(8)
    b.h += [(int(v[i + 1]), int(v[i])) for i in range(7)]
    for _ in range(K - 2):
        b.row(v[:1], "ineq")
    for q in (2, 3):
        for _ in range(130):
            b.row(v[q:q + 1], "ineq")
    for _ in range(60):
        b.row(v[4:6], "ineq")
    b.row(v[5:8], "eq")
    b.row(v[0:2], "eq")
    return b.done(f"items{K}", {"max_items": K})


def acopf(case):
    nb, ng, nl, seed = CASES[case]
    lay = acopf_layout(acopf_synth(nb, ng, nl, seed))
    i64 = lambda a: np.asarray(a, dtype=np.int64)
    return MS.Structure(case, lay.n, lay.m, i64(lay.jrow), i64(lay.jcol), i64(lay.hrow), i64(lay.hcol),
                        np.asarray(lay.gL, float), np.asarray(lay.gU, float), {})


def structures():
    return [acopf("case14"), acopf("case118"), items(255), items(256), items(257)]


def values(S, kind, seed):
    """MS.values with at least one free row (rtype 0) among the inequality rows"""
    v = list(MS.values(S, kind, seed))
    rt = v[5]
    if not (rt == 0).any():
        rt[np.flatnonzero(~S.eq)[seed % int((~S.eq).sum())]] = 0
    return tuple(v)
