"""Factors with affine multi-variable arguments without a GPU (sqpsolver.jl_amd/nlp_terms.py, tests/nlp_affine_ref.py): the
term-by-term reference against finite differences and against NlpRef, the structures of nlp_terms_layout, the joint polar
restatement v_f v_t cos(th_f - th_t) against the ACOPF callbacks and through the oracle's SQP-TR, and the oracle's
convergence on every generated instance the GPU tests run (tests/test_gpu_nlp_affine.py)."""
import dataclasses
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from oracle import oracle as O                                        # noqa: E402
from sqpsolver_jl_amd import _lib                                     # noqa: E402
from sqpsolver_jl_amd.acopf_synth import acopf_layout, acopf_synth, contingency, CASES   # noqa: E402
from sqpsolver_jl_amd.nlp_terms import (COS, POW, SIN, NlpTerms, from_polar_acopf, make_nlp_terms, nlp_affine_synth,   # noqa: E402
                                        nlp_terms_args, nlp_terms_layout, nlp_terms_rows, nlp_terms_scenario, nlp_terms_synth)
from nlp_ref import NlpRef                                            # noqa: E402
from nlp_affine_ref import (GPU_SCENARIOS, GPU_SEED, QUEUE_NOISE, QUEUE_SCENARIOS, SQP_KW, NlpAffineRef, OracleAffineTerms,   # noqa: E402
                            affine_edge_model, gpu_model, gpu_scenarios)
from qcqp_ref import coo_sum                                          # noqa: E402


def rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(1.0, np.abs(np.asarray(b)).max()))


def _dense_jac(R, lay, x):
    J = np.zeros((lay.m, lay.n)); J[lay.jrow - 1, lay.jcol - 1] = R.jac(x, lay.jrow, lay.jcol)
    return J


def test_reference_evaluator_matches_finite_differences():
    p = nlp_affine_synth(12, 8, seed=3)
    lay = nlp_terms_layout(p)
    R = NlpAffineRef(p)
    rng = np.random.default_rng(0)
    x = rng.uniform(0.5, 1.5, p.n); lam = rng.standard_normal(p.m); sigma = 0.7
    h = 1e-6
    E = np.eye(p.n)
    fd_grad = np.array([(R.f(x + h * E[j]) - R.f(x - h * E[j])) / (2 * h) for j in range(p.n)])
    assert rel(R.grad(x), fd_grad) < 1e-8
    fd_J = np.stack([(R.g(x + h * E[j]) - R.g(x - h * E[j])) / (2 * h) for j in range(p.n)], axis=1)
    assert rel(_dense_jac(R, lay, x), fd_J) < 1e-8
    L = lambda y: sigma * R.grad(y) + _dense_jac(R, lay, y).T @ lam
    fd_H = np.stack([(L(x + h * E[j]) - L(x - h * E[j])) / (2 * h) for j in range(p.n)], axis=1)
    H = np.zeros((p.n, p.n)); H[lay.hrow - 1, lay.hcol - 1] = R.hess(x, sigma, lam, lay.hrow, lay.hcol)
    assert np.all(lay.hrow >= lay.hcol)
    assert rel(np.tril(fd_H), H) < 1e-7
    assert set(p.fkind.tolist()) == {0, 1, 2, 3, 4}                                  # the whole menu took part
    assert p.affine and np.diff(p.aptr).max() == 3                                   # ... and a three-argument factor
    assert R.domain_margin(x) > 0


def test_one_argument_models_agree_with_the_one_variable_reference():
    q = nlp_terms_synth(24, 14, seed=5)
    aptr, avar, acoef = nlp_terms_args(q)
    p = dataclasses.replace(q, aptr=aptr.copy(), avar=avar.copy(), acoef=acoef.copy())     # the same model in the affine form
    lay = nlp_terms_layout(q)
    la = nlp_terms_layout(p)
    for k in ("jrow", "jcol", "hrow", "hcol"):
        assert np.array_equal(getattr(lay, k), getattr(la, k)), k
    rng = np.random.default_rng(4)
    x = np.clip(q.x0 + 0.3 * rng.standard_normal(q.n), 0.25, 2.9); lam = rng.standard_normal(q.m)
    assert np.array_equal(nlp_terms_rows(p, x), nlp_terms_rows(q, x))
    for A in (NlpAffineRef(p), NlpAffineRef(q)):
        R = NlpRef(q)
        assert rel(A.f(x), R.f(x)) <= 1e-14 and rel(A.grad(x), R.grad(x)) <= 1e-14 and rel(A.g(x), R.g(x)) <= 1e-14
        assert rel(A.jac(x, lay.jrow, lay.jcol), R.jac(x, lay.jrow, lay.jcol)) <= 1e-14
        assert rel(A.hess(x, 1.3, lam, lay.hrow, lay.hcol), R.hess(x, 1.3, lam, lay.hrow, lay.hcol)) <= 1e-14
    # every positional construction of before still works, and says that it is not affine
    old = NlpTerms(*[getattr(q, f.name) for f in dataclasses.fields(q)][:18])
    assert not old.affine and old.aptr is None


def _needed(p):
    """the entries the header of sqphip_nlp_attach_affine lists"""
    n = p.n
    aptr, avar, _ = nlp_terms_args(p)
    need_j, need_h = set(), set()
    for t in range(len(p.trow)):
        args = [(k, int(avar[j]) - 1) for k in range(p.tptr[t], p.tptr[t + 1]) for j in range(aptr[k], aptr[k + 1])]
        assert len({v for _, v in args}) == len(args)                                # distinct variables in a term
        for i, (k, v) in enumerate(args):
            plain = p.fkind[k] == POW and p.fexp[k] == 1
            if p.trow[t] > 0:
                need_j.add((int(p.trow[t]) - 1) * n + v)
            if not plain:
                need_h.add(v * n + v)
            for k2, w in args[:i]:
                if not (k2 == k and plain):
                    need_h.add(max(v, w) * n + min(v, w))
    return need_j, need_h


def test_layout_structures_have_exactly_the_needed_entries():
    for p in (nlp_affine_synth(30, 20, seed=5), affine_edge_model()[0]):
        lay = nlp_terms_layout(p)
        n = p.n
        jk = ((lay.jrow - 1) * n + lay.jcol - 1).tolist()
        hk = ((lay.hrow - 1) * n + lay.hcol - 1).tolist()
        assert len(set(jk)) == len(jk) and len(set(hk)) == len(hk)                   # no duplicates
        need_j, need_h = _needed(p)
        assert set(jk) == need_j and set(hk) == need_h                               # nothing missing, nothing spurious
        assert np.all(lay.hrow >= lay.hcol)
    # the exception: two arguments of one plain linear factor get no entry, whatever else the term holds
    p = make_nlp_terms(5, 1, 0, [(1, 1.0, [([(1, 1.0), (2, -2.0), (3, 0.5)], POW, 1, 0.3), (4, POW, 2)]),
                                 (0, 1.0, [([(4, 1.0), (5, 1.0)], POW, 2, -1.0)])])
    lay = nlp_terms_layout(p)
    assert sorted(zip(lay.hrow.tolist(), lay.hcol.tolist())) == [(4, 1), (4, 2), (4, 3), (4, 4), (5, 4), (5, 5)]
    assert sorted(zip(lay.jrow.tolist(), lay.jcol.tolist())) == [(1, 1), (1, 2), (1, 3), (1, 4)]
    # linear rows of the generator: single plain one-argument factors only
    p = nlp_affine_synth(30, 20, seed=5)
    for t in np.flatnonzero((p.trow >= 1) & (p.trow <= p.num_linear)):
        k = p.tptr[t]
        assert p.tptr[t + 1] - k == 1 and p.aptr[k + 1] - p.aptr[k] == 1
        assert (p.fkind[k], p.fexp[k], p.acoef[p.aptr[k]], p.fshift[k]) == (POW, 1, 1.0, 0.0)
    # a duplicated slot: the first copy carries the value, the other 0
    R = NlpAffineRef(p)
    lay = nlp_terms_layout(p)
    hr2, hc2 = np.concatenate([lay.hrow, lay.hrow[:1]]), np.concatenate([lay.hcol, lay.hcol[:1]])
    lam = np.ones(p.m)
    h2 = R.hess(p.x0, 1.0, lam, hr2, hc2)
    assert h2[-1] == 0.0 and np.array_equal(h2[:-1], R.hess(p.x0, 1.0, lam, lay.hrow, lay.hcol))


def test_make_nlp_terms_reads_both_forms_of_a_factor():
    p = make_nlp_terms(3, 1, 0, [(1, 2.0, [(1, SIN, 1, 2.0, 0.1), ([(2, 1.0), (3, -1.0)], COS)]), (0, 1.0, [([(3, 0.5)], POW, 2, 0.25)])])
    assert p.affine and p.aptr.tolist() == [0, 1, 3, 4] and p.avar.tolist() == [1, 2, 3, 3] and p.acoef.tolist() == [2.0, 1.0, -1.0, 0.5]
    assert p.fshift.tolist() == [0.1, 0.0, 0.25] and p.fexp.tolist() == [1, 1, 2]
    assert p.fvar.tolist() == [1, 2, 3] and p.fscale.tolist() == [2.0, 1.0, 0.5]     # the first argument of every factor
    x = np.array([0.3, 0.9, 0.4])
    assert abs(nlp_terms_rows(p, x)[0] - 2.0 * np.sin(0.7) * np.cos(0.5)) <= 1e-15
    assert abs(NlpAffineRef(p).f(x) - (0.5 * 0.4 + 0.25) ** 2) <= 1e-15
    q = make_nlp_terms(3, 1, 0, [(1, 2.0, [(1, SIN, 1, 2.0, 0.1)])])
    assert not q.affine


def test_synth_start_is_feasible_and_scenarios_keep_it():
    p, _ = gpu_model()
    g = NlpAffineRef(p).g(p.x0)
    assert np.all(g >= p.gL - 1e-12) and np.all(g <= p.gU + 1e-12)
    assert np.all(p.x0 >= p.xL) and np.all(p.x0 <= p.xU)
    s = nlp_terms_scenario(p, 3, GPU_SEED)
    assert s.affine and np.allclose(NlpAffineRef(s).g(p.x0), g, atol=1e-12) and not np.array_equal(s.tcoef, p.tcoef)
    b, _ = gpu_model()
    for f in dataclasses.fields(p):
        assert np.array_equal(getattr(p, f.name), getattr(b, f.name)), f.name       # deterministic per seed
    # LOG and negative powers keep a positive argument on the whole box: positive coefficients, shift >= 0
    k = np.flatnonzero((p.fkind == 4) | ((p.fkind == POW) & (p.fexp < 0)))
    assert len(k) and all(np.all(p.acoef[p.aptr[i]:p.aptr[i + 1]] > 0) and p.fshift[i] >= 0 for i in k)
    assert int((np.diff(p.aptr)[p.tptr[:-1][p.trow == 0]] == 3).sum()) == 4         # the four least-squares residuals


def _polar(joint=True):
    nb, ng, nl, seed = CASES["case14"]
    base = acopf_synth(nb, ng, nl, seed)
    nets = [base, contingency(base, 2, seed), contingency(base, 5, seed)]
    lays = [acopf_layout(nt) for nt in nets]
    return nets, lays, [from_polar_acopf(nt, ly, joint=joint) for nt, ly in zip(nets, lays)]


def test_joint_polar_restatement_matches_the_acopf_callbacks_and_the_oracle_run():
    """Evaluator: one cos / sin of the angle difference on both sides, entries of a handful of operations: 1e-12 as for the
    expanded form (tests/test_nlp_cpu.py).  Oracle runs on the two evaluators: equal status, iterations and decisions, points
    within 1e-8."""
    nets, lays, ps = _polar()
    ex = from_polar_acopf(nets[0], lays[0])
    assert ps[0].affine and not ex.affine
    assert len(ps[0].trow) == len(ex.trow) - 2 * 4 * nets[0].nl and len(ps[0].fkind) == len(ex.fkind) - 10 * 4 * nets[0].nl
    for k in ("trow", "tptr", "aptr", "avar", "acoef", "fkind", "fexp", "fshift"):
        assert np.array_equal(getattr(ps[0], k), getattr(ps[1], k)), k                # a contingency keeps the structure
    rng = np.random.default_rng(11)
    kw = dict(max_iter=60, use_soc=1, literal_quirks=0, tol_infeas=1e-6, tol_residual=1e-4)
    for net, lay, p in zip(nets, lays, ps):
        P = O.problem_acopf(net, lay)
        R = NlpAffineRef(p)
        J = lambda v: coo_sum(v, lay.jrow, lay.jcol, lay.n)
        H = lambda v: coo_sum(v, lay.hrow, lay.hcol, lay.n, lower=True)
        x = lay.x0 + 0.1 * rng.standard_normal(lay.n); lam = rng.standard_normal(lay.m); sigma = rng.uniform(0.5, 2)
        assert rel(R.f(x), P.eval_f(x)) <= 1e-12
        assert rel(R.grad(x), P.eval_grad_f(x)) <= 1e-12 and rel(R.g(x), P.eval_g(x)) <= 1e-12
        assert rel(J(R.jac(x, lay.jrow, lay.jcol)), J(P.eval_jac_g(x))) <= 1e-12
        assert rel(H(R.hess(x, sigma, lam, lay.hrow, lay.hcol)), H(P.eval_h(x, sigma, lam))) <= 1e-12
        rd = O.sqp_solve(P, O.default_options(kkt_mode=2, **kw))
        rj = O.sqp_solve(OracleAffineTerms(p, lay), O.default_options(kkt_mode=2, **kw))
        print("status", rj["status"], rd["status"], "iter", rj["iter"], rd["iter"], "x", rel(rj["x"], rd["x"]))
        assert (rj["status"], rj["iter"]) == (rd["status"], rd["iter"])
        dec = lambda r: [(a["iter"], a["accepted"], a["fr"], a["sub_status"]) for a in r["trace"]]
        assert dec(rj) == dec(rd)
        assert rel(rj["x"], rd["x"]) <= 1e-8


def _oracle_run(base, lay, p):
    r = O.sqp_solve(OracleAffineTerms(p, lay), O.default_options(kkt_mode=2, **SQP_KW))
    R = NlpAffineRef(p)
    assert r["status"] == 0, (r["status"], r["iter"])
    assert R.domain_margin(r["x"]) > 0                                               # LOG / negative powers stayed inside their domain
    g = R.g(r["x"])
    assert np.all(g >= p.gL - 1e-6) and np.all(g <= p.gU + 1e-6)
    return r["iter"]


@pytest.mark.parametrize("scenario", GPU_SCENARIOS)
def test_oracle_converges_on_the_generated_instances_of_the_gpu_tests(scenario):
    base, lay = gpu_model()
    _oracle_run(base, lay, gpu_scenarios(base, (scenario,))[0])


def test_oracle_converges_on_the_scenarios_of_the_queue_test_with_differing_iteration_counts():
    base, lay = gpu_model()
    iters = [_oracle_run(base, lay, p) for p in gpu_scenarios(base, QUEUE_SCENARIOS, QUEUE_NOISE)]
    print("iterations", iters)
    assert len(set(iters)) > 1                                                       # slots of the queue refill at different times


def test_the_entry_point_is_declared_exported_and_refuses_a_null_handle():
    L = _lib.lib()
    assert "sqphip_nlp_attach_affine" in _lib.EXPORTS and hasattr(L, "sqphip_nlp_attach_affine")
    assert L.sqphip_nlp_attach_affine(None, 0, None, None, None, None, None, None, None, None, None, None, 0.0) == -1
    import sqpsolver_jl_amd as pkg
    import inspect
    assert "sqphip_nlp_attach_affine" in inspect.getsource(pkg.Context.nlp_attach)
