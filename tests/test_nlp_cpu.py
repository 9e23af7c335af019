"""The factorable-NLP path without a GPU: the numpy reference evaluator against finite differences, the structures of
nlp_terms_layout, HS071 / a QCQP / the polar ACOPF restated as terms against their own evaluators, and the generator
(sqpsolver.jl_amd/nlp_terms.py, tests/nlp_ref.py)."""
import dataclasses
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from oracle import oracle as O                                        # noqa: E402
from sqpsolver_jl_amd.acopf_synth import acopf_layout, acopf_synth, contingency, CASES   # noqa: E402
from sqpsolver_jl_amd.nlp_terms import (POW, from_polar_acopf, from_qcqp, nlp_terms_layout, nlp_terms_scenario,   # noqa: E402
                                        nlp_terms_synth)
from sqpsolver_jl_amd.qcqp import qcqp_layout, qcqp_synth            # noqa: E402
from nlp_ref import GPU_SCENARIOS, GPU_SEED, NlpRef, OracleNlpTerms, hs071_terms              # noqa: E402
from qcqp_ref import QcqpRef, coo_sum                                 # noqa: E402

SQP_KW = dict(tol_infeas=1e-6, tol_residual=1e-4)


def rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(1.0, np.abs(np.asarray(b)).max()))


def _net(case, s=5):
    nb, ng, nl, seed = CASES[case.split("-")[0]]
    base = acopf_synth(nb, ng, nl, seed)
    net = base if s == 0 else contingency(base, s, seed)
    rng = np.random.default_rng(seed)
    if "taps" in case:
        tr = rng.random(net.nl) < 0.33
        net = dataclasses.replace(net, tap=np.where(tr, rng.uniform(0.93, 1.07, net.nl), 1.0),
                                  shift=np.where(tr & (rng.random(net.nl) < 0.3), rng.uniform(-0.08, 0.08, net.nl), 0.0))
    if "shunts" in case:
        net = dataclasses.replace(net, gs=np.where(rng.random(net.nb) < 0.3, rng.uniform(0, 0.03, net.nb), 0.0),
                                  bs=np.where(rng.random(net.nb) < 0.4, rng.uniform(-0.05, 0.19, net.nb), 0.0))
    if "dc" in case:
        dc = dict(f_bus=np.array([2, 7], dtype=np.int32), t_bus=np.array([9, 3], dtype=np.int32),
                  pminf=np.array([0.05, -0.3]), pmaxf=np.array([0.6, 0.3]), qminf=np.full(2, -0.4), qmaxf=np.full(2, 0.4),
                  qmint=np.full(2, -0.4), qmaxt=np.full(2, 0.4), loss0=np.array([0.002, 0.0]), loss1=np.array([0.03, 0.0]))
        net = dataclasses.replace(net, dcline=dc)
    return net


def test_reference_evaluator_matches_finite_differences():
    p = nlp_terms_synth(12, 8, seed=3)
    lay = nlp_terms_layout(p)
    R = NlpRef(p)
    rng = np.random.default_rng(0)
    x = rng.uniform(0.5, 1.5, p.n); lam = rng.standard_normal(p.m); sigma = 0.7
    h = 1e-6
    E = np.eye(p.n)
    fd_grad = np.array([(R.f(x + h * E[j]) - R.f(x - h * E[j])) / (2 * h) for j in range(p.n)])
    assert rel(R.grad(x), fd_grad) < 1e-8
    J = np.zeros((p.m, p.n)); J[lay.jrow - 1, lay.jcol - 1] = R.jac(x, lay.jrow, lay.jcol)
    fd_J = np.stack([(R.g(x + h * E[j]) - R.g(x - h * E[j])) / (2 * h) for j in range(p.n)], axis=1)
    assert rel(J, fd_J) < 1e-8
    # Hessian of the Lagrangian sigma f + lam'g from the gradients
    L = lambda y: sigma * R.grad(y) + R.dense_jac(y).T @ lam
    fd_H = np.stack([(L(x + h * E[j]) - L(x - h * E[j])) / (2 * h) for j in range(p.n)], axis=1)
    H = np.zeros((p.n, p.n)); H[lay.hrow - 1, lay.hcol - 1] = R.hess(x, sigma, lam, lay.hrow, lay.hcol)
    assert np.all(lay.hrow >= lay.hcol)
    assert rel(np.tril(fd_H), H) < 1e-7
    assert set(p.fkind.tolist()) == {0, 1, 2, 3, 4}                                  # the whole menu took part


def test_layout_structures_have_exactly_the_needed_entries():
    p = nlp_terms_synth(30, 20, seed=5)
    lay = nlp_terms_layout(p)
    n = p.n
    jk = ((lay.jrow - 1) * n + lay.jcol - 1).tolist()
    hk = ((lay.hrow - 1) * n + lay.hcol - 1).tolist()
    assert len(set(jk)) == len(jk) and len(set(hk)) == len(hk)                       # no duplicates
    need_j, need_h = set(), set()
    for t in range(len(p.trow)):
        ks = range(p.tptr[t], p.tptr[t + 1])
        for k in ks:
            v = int(p.fvar[k]) - 1
            if p.trow[t] > 0:
                need_j.add((int(p.trow[t]) - 1) * n + v)
            if not (p.fkind[k] == POW and p.fexp[k] == 1):
                need_h.add(v * n + v)
            for k2 in ks:
                w = int(p.fvar[k2]) - 1
                if k2 < k:
                    assert v != w                                                    # distinct variables in a term
                    need_h.add(max(v, w) * n + min(v, w))
    assert set(jk) == need_j and set(hk) == need_h                                   # nothing missing, nothing spurious
    assert np.all(lay.hrow >= lay.hcol) and lay.num_linear == p.num_linear == 2
    # linear rows: single plain factors only
    for t in np.flatnonzero((p.trow >= 1) & (p.trow <= p.num_linear)):
        k = p.tptr[t]
        assert p.tptr[t + 1] - k == 1 and (p.fkind[k], p.fexp[k], p.fscale[k], p.fshift[k]) == (POW, 1, 1.0, 0.0)
    # a structure with a duplicated slot: the first occurrence carries the value, the copy 0
    R = NlpRef(p)
    jr2, jc2 = np.concatenate([lay.jrow, lay.jrow[:1]]), np.concatenate([lay.jcol, lay.jcol[:1]])
    x = p.x0 + 0.1
    j2 = R.jac(x, jr2, jc2)
    assert j2[-1] == 0.0 and np.array_equal(j2[:-1], R.jac(x, lay.jrow, lay.jcol))


def test_hs071_as_terms_matches_the_hand_written_callbacks():
    P = O.problem_hs071()
    p, lay = hs071_terms()
    assert len(lay.jrow) == 8 and len(lay.hrow) == 10
    R = NlpRef(p)
    rng = np.random.default_rng(71)
    for _ in range(5):
        x = rng.uniform(1, 5, 4); lam = rng.standard_normal(2); sigma = rng.uniform(0.5, 2)
        for got, want in ((R.f(x), P.eval_f(x)), (R.grad(x), P.eval_grad_f(x)), (R.g(x), P.eval_g(x)),
                          (R.jac(x, lay.jrow, lay.jcol), P.eval_jac_g(x)),
                          (R.hess(x, sigma, lam, lay.hrow, lay.hcol), P.eval_h(x, sigma, lam))):
            assert rel(got, want) <= 1e-13


def test_a_qcqp_as_terms_matches_the_qcqp_reference():
    q = qcqp_synth(24, 14, 5)
    lay = qcqp_layout(q)
    p = from_qcqp(q)
    lp = nlp_terms_layout(p)
    for k in ("jrow", "jcol", "hrow", "hcol"):
        assert np.array_equal(getattr(lp, k), getattr(lay, k)), k                   # the same structures
    R, Q = NlpRef(p), QcqpRef(q)
    rng = np.random.default_rng(4)
    x = q.x0 + 0.3 * rng.standard_normal(q.n); lam = rng.standard_normal(q.m)
    assert rel(R.f(x), Q.f(x)) <= 1e-13 and rel(R.grad(x), Q.grad(x)) <= 1e-13 and rel(R.g(x), Q.g(x)) <= 1e-13
    assert rel(R.jac(x, lay.jrow, lay.jcol), Q.jac(x, lay.jrow, lay.jcol)) <= 1e-13
    assert rel(R.hess(x, 1.3, lam, lay.hrow, lay.hcol), Q.hess(1.3, lam, lay.hrow, lay.hcol)) <= 1e-13


@pytest.mark.parametrize("case", ["case14", "case14-taps-shunts", "case14-taps-shunts-dc"])
def test_polar_acopf_as_terms_matches_the_acopf_callbacks(case):
    """The two sides use different formulas for cos(th_f - th_t) (the terms expand it into products of cos / sin of the two
    angles); each entry is a handful of operations on quantities of order 1 - 100, so 1e-12 relative leaves three digits
    over rounding."""
    net = _net(case)
    lay = acopf_layout(net)
    P = O.problem_acopf(net, lay)
    p = from_polar_acopf(net, lay)
    if "dc" in case:                                                                 # two loss rows, the lines' entries in the balance rows
        assert net.ndc == 2 and lay.m == 1 + 2 * net.nb + 8 * net.nl + 2 and int((p.trow > lay.m - 2).sum()) == 4
    R = NlpRef(p)
    rng = np.random.default_rng(11)
    J = lambda v: coo_sum(v, lay.jrow, lay.jcol, lay.n)                              # duplicated slots summed
    H = lambda v: coo_sum(v, lay.hrow, lay.hcol, lay.n, lower=True)
    for _ in range(2):
        x = lay.x0 + 0.1 * rng.standard_normal(lay.n); lam = rng.standard_normal(lay.m); sigma = rng.uniform(0.5, 2)
        assert rel(R.f(x), P.eval_f(x)) <= 1e-12
        assert rel(R.grad(x), P.eval_grad_f(x)) <= 1e-12 and rel(R.g(x), P.eval_g(x)) <= 1e-12
        assert rel(J(R.jac(x, lay.jrow, lay.jcol)), J(P.eval_jac_g(x))) <= 1e-12
        assert rel(H(R.hess(x, sigma, lam, lay.hrow, lay.hcol)), H(P.eval_h(x, sigma, lam))) <= 1e-12
    # a contingency keeps the term structure
    p2 = from_polar_acopf(_net(case, 3), acopf_layout(_net(case, 3)))
    for k in ("trow", "tptr", "fvar", "fkind", "fexp", "fscale", "fshift"):
        assert np.array_equal(getattr(p, k), getattr(p2, k)), k
    assert not np.array_equal(p.tcoef, p2.tcoef)


def test_synth_start_is_feasible_and_scenarios_keep_it():
    p = nlp_terms_synth(24, 14, seed=GPU_SEED)
    g = NlpRef(p).g(p.x0)
    assert np.all(g >= p.gL - 1e-12) and np.all(g <= p.gU + 1e-12)
    assert np.all(p.x0 >= p.xL) and np.all(p.x0 <= p.xU)
    s = nlp_terms_scenario(p, 3, GPU_SEED)
    assert np.allclose(NlpRef(s).g(p.x0), g, atol=1e-12) and not np.array_equal(s.tcoef, p.tcoef)
    b = nlp_terms_synth(24, 14, seed=GPU_SEED)
    for f in dataclasses.fields(p):
        assert np.array_equal(getattr(p, f.name), getattr(b, f.name)), f.name       # deterministic per seed


@pytest.mark.parametrize("scenario", GPU_SCENARIOS)
def test_oracle_converges_on_the_generated_instances_of_the_gpu_tests(scenario):
    base = nlp_terms_synth(24, 14, seed=GPU_SEED)
    p = nlp_terms_scenario(base, scenario, GPU_SEED)
    lay = nlp_terms_layout(base)
    r = O.sqp_solve(OracleNlpTerms(p, lay), O.default_options(kkt_mode=2, max_iter=30, literal_quirks=0, **SQP_KW))
    assert r["status"] == 0, (r["status"], r["iter"])
    assert NlpRef(p).domain_margin(r["x"]) > 0                                       # LOG / negative powers stayed inside their domain
    g = NlpRef(p).g(r["x"])
    assert np.all(g >= p.gL - 1e-6) and np.all(g <= p.gU + 1e-6)
