"""The general QCQP path without a GPU: the numpy reference evaluator, the structures of qcqp_layout, the exact extraction of
QCQP data from the quadratic ACOPF forms (ACR, ACWR) and the generator (sqpsolver.jl_amd/qcqp.py, tests/qcqp_ref.py)."""
import dataclasses
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from oracle import oracle as O                                        # noqa: E402
from sqpsolver_jl_amd.acopf_synth import acopf_synth, acr_layout, acwr_layout, contingency, CASES   # noqa: E402
from sqpsolver_jl_amd.qcqp import make_qcqp, qcqp_layout, qcqp_scenario, qcqp_synth   # noqa: E402
from qcqp_ref import OracleQcqp, QcqpRef, coo_sum, extract                    # noqa: E402


def rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(1.0, np.abs(np.asarray(b)).max()))


def _net(case, seed_shift=5):
    nb, ng, nl, seed = CASES[case.split("-")[0]]
    net = contingency(acopf_synth(nb, ng, nl, seed), seed_shift, seed)
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
    q = qcqp_synth(12, 8, seed=3)
    lay = qcqp_layout(q)
    R = QcqpRef(q)
    rng = np.random.default_rng(0)
    x = rng.uniform(-1, 1, q.n); lam = rng.standard_normal(q.m); sigma = 0.7
    h = 1e-6
    E = np.eye(q.n)
    fd_grad = np.array([(R.f(x + h * E[j]) - R.f(x - h * E[j])) / (2 * h) for j in range(q.n)])
    assert rel(R.grad(x), fd_grad) < 1e-8
    J = np.zeros((q.m, q.n)); J[lay.jrow - 1, lay.jcol - 1] = R.jac(x, lay.jrow, lay.jcol)
    fd_J = np.stack([(R.g(x + h * E[j]) - R.g(x - h * E[j])) / (2 * h) for j in range(q.n)], axis=1)
    assert rel(J, fd_J) < 1e-8
    # Hessian of the Lagrangian sigma f + lam'g from the gradients
    L = lambda y: sigma * R.grad(y) + R.dense_jac(y).T @ lam
    fd_H = np.stack([(L(x + h * E[j]) - L(x - h * E[j])) / (2 * h) for j in range(q.n)], axis=1)
    H = np.zeros((q.n, q.n)); H[lay.hrow - 1, lay.hcol - 1] = R.hess(sigma, lam, lay.hrow, lay.hcol)
    assert np.all(lay.hrow >= lay.hcol)
    assert rel(np.tril(fd_H), H) < 1e-7
    # the value convention: off-diagonal v -> v x_r x_c (either triangle), diagonal v -> v x_r^2 / 2; duplicates summed
    q2 = make_qcqp(2, 1, 0, Q0=([1, 2, 1], [2, 1, 1], [3.0, 1.0, 4.0]), A=([1], [1], [1.0]), Q=([1, 1], [2, 2], [2, 1], [5.0, 1.0]),
                   c=[1.0, -1.0], g0=[0.5], f0=2.0)
    y = np.array([0.3, -0.7])
    assert np.isclose(R.__class__(q2).f(y), 2.0 + 0.3 + 0.7 + 4.0 * y[0] * y[1] + 2.0 * y[0] ** 2)
    assert np.isclose(R.__class__(q2).g(y)[0], 0.5 + y[0] + 0.5 * 5.0 * y[1] ** 2 + y[0] * y[1])


def test_layout_structures_have_exactly_the_needed_entries():
    q = qcqp_synth(30, 20, seed=5)
    lay = qcqp_layout(q)
    n = q.n
    jk = set(((lay.jrow - 1) * n + lay.jcol - 1).tolist())
    hk = set(((lay.hrow - 1) * n + lay.hcol - 1).tolist())
    assert len(jk) == len(lay.jrow) and len(hk) == len(lay.hrow)                  # no duplicates
    need_j = set(((q.ar - 1) * n + q.ac - 1).tolist()) | set(((q.qi - 1) * n + q.qr - 1).tolist()) | \
        set(((q.qi - 1) * n + q.qc - 1).tolist())
    lo = lambda r, c: (np.maximum(r, c) - 1) * n + np.minimum(r, c) - 1
    need_h = set(lo(q.q0r, q.q0c).tolist()) | set(lo(q.qr, q.qc).tolist())
    assert jk == need_j and hk == need_h                                            # nothing missing, nothing spurious
    assert np.all(lay.hrow >= lay.hcol) and lay.num_linear == q.num_linear
    assert not np.any(np.isin(q.qi, np.arange(1, q.num_linear + 1)))                 # linear rows carry no Q term
    # duplicated Q terms (both triangles of one entry) share one Hessian slot and sum there
    R = QcqpRef(q)
    lam = np.ones(q.m)
    H = R.hess(0.0, lam, lay.hrow, lay.hcol)
    want = np.zeros(len(lay.hrow))
    key = {k: s for s, k in enumerate(((lay.hrow - 1) * n + lay.hcol - 1).tolist())}
    for r, c, v in zip(q.qr, q.qc, q.qv):
        want[key[int(lo(r, c))]] += v
    assert np.allclose(H, want, rtol=0, atol=1e-15)
    # a structure with a duplicated slot: the first occurrence carries the value, the copy 0
    jr2, jc2 = np.concatenate([lay.jrow, lay.jrow[:1]]), np.concatenate([lay.jcol, lay.jcol[:1]])
    x = q.x0 + 0.1
    j2 = R.jac(x, jr2, jc2)
    assert j2[-1] == 0.0 and np.array_equal(j2[:-1], R.jac(x, lay.jrow, lay.jcol))


def test_synth_start_is_feasible():
    q = qcqp_synth(40, 24, seed=2)
    g = QcqpRef(q).g(q.x0)
    assert np.all(g >= q.gL - 1e-12) and np.all(g <= q.gU + 1e-12)
    assert np.all(q.x0 >= q.xL) and np.all(q.x0 <= q.xU)
    s = qcqp_scenario(q, 3)
    assert np.allclose(QcqpRef(s).g(q.x0), g, atol=1e-12) and not np.array_equal(s.qv, q.qv)


@pytest.mark.parametrize("case", ["case14-acr", "case118-acr-taps-shunts-dc", "case14-acwr"])
def test_extract_reproduces_the_quadratic_acopf_forms(case):
    net = _net(case)
    lay = acwr_layout(net) if "acwr" in case else acr_layout(net)
    P = O.problem_acopf(net, lay)
    q = extract(P)
    R = QcqpRef(q)
    rng = np.random.default_rng(11)
    for _ in range(2):
        x = lay.x0 + 0.1 * rng.standard_normal(lay.n); lam = rng.standard_normal(lay.m); sigma = rng.uniform(0.5, 2)
        assert abs(R.f(x) - P.eval_f(x)) <= 1e-13 * max(1.0, abs(P.eval_f(x)))
        assert rel(R.grad(x), P.eval_grad_f(x)) < 1e-13 and rel(R.g(x), P.eval_g(x)) < 1e-13
        J = lambda v: coo_sum(v, lay.jrow, lay.jcol, lay.n)               # duplicated slots summed
        H = lambda v: coo_sum(v, lay.hrow, lay.hcol, lay.n, lower=True)
        assert rel(J(R.jac(x, lay.jrow, lay.jcol)), J(P.eval_jac_g(x))) < 1e-13
        assert rel(H(R.hess(sigma, lam, lay.hrow, lay.hcol)), H(P.eval_h(x, sigma, lam))) < 1e-13
    # and the oracle's own callbacks over the extracted data agree with its ACOPF callbacks
    OQ = OracleQcqp(q, lay)
    x = lay.x0 + 0.05
    assert rel(J(OQ.eval_jac_g(x)), J(P.eval_jac_g(x))) < 1e-13


def test_extract_of_a_batch_shares_one_structure():
    nb, ng, nl, seed = CASES["case14"]
    base = acopf_synth(nb, ng, nl, seed)
    nets = [base, contingency(base, 2, seed), contingency(base, 5, seed)]
    lays = [acr_layout(nt) for nt in nets]
    qs = extract([O.problem_acopf(nt, ly) for nt, ly in zip(nets, lays)])
    for q in qs[1:]:
        for k in ("q0r", "q0c", "ar", "ac", "qi", "qr", "qc"):
            assert np.array_equal(getattr(q, k), getattr(qs[0], k))
    assert any(not np.array_equal(q.av, qs[0].av) or not np.array_equal(q.qv, qs[0].qv) for q in qs[1:])


def test_synth_is_deterministic_per_seed():
    a, b, c = qcqp_synth(40, 24, seed=7), qcqp_synth(40, 24, seed=7), qcqp_synth(40, 24, seed=8)
    for f in dataclasses.fields(a):
        va, vb = getattr(a, f.name), getattr(b, f.name)
        assert np.array_equal(va, vb), f.name
    assert not np.array_equal(a.qv, c.qv) or not np.array_equal(a.av, c.av)
    assert qcqp_layout(a).num_linear >= 1 and len(a.qv) > 0


def test_oracle_solves_a_synthetic_qcqp():
    q = qcqp_synth(20, 12, seed=3)
    r = O.sqp_solve(OracleQcqp(q), O.default_options(max_iter=60, tol_infeas=1e-6, tol_residual=1e-4))
    assert r["status"] == 0                                                        # converged (53 outer iterations)
    g = QcqpRef(q).g(r["x"])
    assert np.all(g >= q.gL - 1e-6) and np.all(g <= q.gU + 1e-6)
