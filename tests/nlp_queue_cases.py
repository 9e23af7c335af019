"""Case definitions of the scenario queue on a factorable-NLP context (sqphip_nlp_stream_begin / _set), shared by
tests/test_nlp_stream_cpu.py (which vouches for them with the oracle) and tests/test_gpu_nlp_stream.py (which runs them):

    queue_problem     the generated problem, its layout and the twelve scenarios of the queue
    null_part_terms   the two instances of the NULL-parts test, built from the attach values
    edge_model        one tiny model per value count at a stride edge of the loader's block copy
    edge_scenarios    ... and its three scenarios
    POLAR_SCENARIOS   the IEEE-14-shaped contingencies of the generic-queue-against-dedicated-queue test"""
from __future__ import annotations

import dataclasses

import numpy as np

from sqpsolver_jl_amd.nlp_terms import POW, make_nlp_terms, nlp_terms_layout, nlp_terms_scenario, nlp_terms_synth

M = 12                                       # scenarios of the queue
SEED, NOISE = 5, 0.4
TIGHT_XL = 0.4                               # the lower bound of the scenarios with s % 4 == 3 (0.2 elsewhere)
OPTIONS = dict(max_iter=30, literal_quirks=0, tol_infeas=1e-6, tol_residual=1e-4)
ORACLE_ITERS = (7, 6, 7, 6, 9, 7, 9, 6, 9, 14, 15, 6)      # of the CPU oracle on the twelve scenarios (kkt_mode 2 and 1)

# the loader copies a block of nv2 = ceil((1 + m + nterms) / 2) double2 in trips of 2 * 1024 (TPB threads, two accesses in
# flight): value counts at the odd / padded tail, at one against two accesses in flight, and in a second trip
TPB = 1024
EDGE_COUNTS = (2047, 2048, 2049, 2050, 4097, 4099)

# contingencies of the IEEE-14-shaped base net (0: the base net itself); tests/test_gpu_nlp.py holds 0, 2 and 5 to the
# same bound in a batch.  Contingency 4 lasts to the iteration limit (status -1 after 61 iterations, on both evaluators)
POLAR_SCENARIOS = (0, 2, 5, 1, 3, 4, 6, 7)


def tightened(p):
    return dataclasses.replace(p, xL=np.full(p.n, TIGHT_XL))


def queue_problem():
    """(base, layout of the base, the twelve scenarios): coefficient noise of 40 % spreads the iteration counts, every
    fourth scenario carries a tighter lower bound that is active at its optimum."""
    base = nlp_terms_synth(24, 14, seed=SEED)
    ps = [nlp_terms_scenario(base, s, SEED, noise=NOISE) for s in range(M)]
    ps = [tightened(p) if s % 4 == 3 else p for s, p in enumerate(ps)]
    return base, nlp_terms_layout(base), ps


def scenario_layout(lay, p):
    """the base layout with the bounds of scenario p (what the oracle is given)"""
    return dataclasses.replace(lay, xL=p.xL.copy(), xU=p.xU.copy(), gL=p.gL.copy(), gU=p.gU.copy())


def null_part_terms(base, ps):
    """(tcoef of the scenario set with tcoef and x0 only, the two instances these scenarios amount to).  Only the objective's
    coefficients differ from the attach values: g0 stays, so the rows keep their value at the start."""
    tcoef = np.where(base.trow == 0, ps[5].tcoef, base.tcoef)
    return tcoef, [dataclasses.replace(base, tcoef=tcoef), base]


def edge_model(nvals: int):
    """n = 6, m = 3 (two linear rows), 1 + m + nterms = nvals: the objective sum_t c_t (x_{t mod n} - a_t)^2 fills the count."""
    n, m = 6, 3
    rows = [(1, 1.0, [(1, POW)]), (1, 1.0, [(2, POW)]), (2, 1.0, [(3, POW)]), (2, -1.0, [(4, POW)]),
            (3, 1.0, [(5, POW), (6, POW)]), (3, 0.5, [(1, POW, 2)])]
    nobj = nvals - 1 - m - len(rows)
    rng = np.random.default_rng(nvals)
    x0 = rng.uniform(0.8, 1.2, n)
    a = x0[np.arange(nobj) % n] + 0.3 * rng.choice([-1.0, 1.0], nobj)
    c = rng.uniform(0.5, 2.0, nobj) * (n / nobj)
    terms = [(0, c[t], [(t % n + 1, POW, 2, 1.0, -a[t])]) for t in range(nobj)] + rows
    g = np.array([x0[0] + x0[1], x0[2] - x0[3], x0[4] * x0[5] + 0.5 * x0[0] ** 2])
    p = make_nlp_terms(n, m, 2, terms, g0=np.zeros(m), f0=0.5, xL=np.full(n, 0.2), xU=np.full(n, 3.0),
                       gL=[g[0], g[1] - 0.3, -np.inf], gU=[g[0], g[1] + 0.3, g[2] + 0.4], x0=x0)
    assert 1 + p.m + len(p.trow) == nvals
    return p


def edge_scenarios(p):
    """three scenarios: every coefficient rescaled by 1 + 20 % noise (g0 moves so that every row keeps its value at the
    feasible start), another f0"""
    return [nlp_terms_scenario(p, s + 1, seed=len(p.trow), noise=0.2) for s in range(3)]
