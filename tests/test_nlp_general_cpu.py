"""Variables shared across the factors of a term and the kinds SQRT .. POWR without a GPU (sqpsolver.jl_amd/nlp_terms.py,
tests/nlp_general_ref.py): the ordered-pair reference against finite differences, against the one-variable-per-term
reference on the old class and on (x + y)(x - y) by hand, the generator's invariants, the structures of nlp_terms_layout,
the three known-answer builders, the prototypes of the new entry point and the oracle's convergence on every generated
instance the GPU tests run (tests/test_gpu_nlp_general.py)."""
import inspect
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from oracle import oracle as O                                        # noqa: E402
from sqpsolver_jl_amd import _lib                                     # noqa: E402
from sqpsolver_jl_amd.nlp_terms import (LOG, POW, POWR, SIGMOID, SOFTPLUS, SQRT, TANH, cobb_douglas_model, entropy_model,   # noqa: E402
                                        factor_values, logistic_model, make_nlp_terms, needs_general, nlp_affine_synth,
                                        nlp_general_synth, nlp_terms_args, nlp_terms_layout, nlp_terms_rows, nlp_terms_synth)
from nlp_affine_ref import NlpAffineRef                               # noqa: E402
from nlp_general_ref import (GPU_SCENARIOS, NEW_KINDS, QUEUE_NOISE, QUEUE_SCENARIOS, SQP_KW, NlpGeneralRef,   # noqa: E402
                             OracleGeneralTerms, general_edge_model, gpu_model, gpu_scenarios, saturation_model)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(1.0, np.abs(np.asarray(b)).max()))


def _dense_jac(R, lay, x):
    J = np.zeros((lay.m, lay.n)); J[lay.jrow - 1, lay.jcol - 1] = R.jac(x, lay.jrow, lay.jcol)
    return J


def test_the_entry_point_is_declared_exported_and_refuses_a_null_handle():
    L = _lib.lib()
    assert "sqphip_nlp_attach_general" in _lib.EXPORTS and hasattr(L, "sqphip_nlp_attach_general")
    assert L.sqphip_nlp_attach_general(None, 0, None, None, None, None, None, None, None, None, None, None, None, 0.0) == -1
    import sqpsolver_jl_amd as pkg
    assert "sqphip_nlp_attach_general" in inspect.getsource(pkg.Context.nlp_attach)


def test_header_ctypes_and_julia_prototypes_agree():
    """int f(ctx*, i64, i64*, f64*, i64*, i64*, i64*, f64*, i32*, i32*, f64*, f64*, f64*, f64) in all three places"""
    import ctypes as C
    want = ["ctx", "i64", "i64*", "f64*", "i64*", "i64*", "i64*", "f64*", "i32*", "i32*", "f64*", "f64*", "f64*", "f64"]
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "sqphip.h")).read(), flags=re.S)
    args = re.search(r"\bint\s+sqphip_nlp_attach_general\s*\(([^;]*?)\)\s*;", hdr, flags=re.S).group(1).split(",")
    ckind = lambda a: ("ctx" if "sqphip_ctx" in a else
                       {"int64_t": "i64", "int32_t": "i32", "double": "f64"}[re.search(r"int64_t|int32_t|double", a).group(0)] + ("*" if "*" in a else ""))
    assert [ckind(a) for a in args] == want
    names = [re.findall(r"\w+", a)[-1] for a in args]
    assert names == ["ctx", "nterms", "trow", "tcoef", "tptr", "aptr", "avar", "acoef", "fkind", "fexp", "fpar", "fshift", "g0", "f0"]
    table = {C.c_void_p: "ctx", C.c_int64: "i64", C.c_double: "f64", C.POINTER(C.c_int64): "i64*", C.POINTER(C.c_int32): "i32*",
             C.POINTER(C.c_double): "f64*"}
    assert [table[t] for t in _lib.lib().sqphip_nlp_attach_general.argtypes] == want
    jl = re.sub(r"#[^\n]*", "", open(os.path.join(ROOT, "julia", "SqpHip.jl")).read())
    ret, argt = re.search(r"ccall\(\(:sqphip_nlp_attach_general, LIBSQPHIP\),\s*(\w+),\s*\((.*?)\)\s*,", jl, flags=re.S).groups()
    jkind = {"Ptr{Cvoid}": "ctx", "Int64": "i64", "Cdouble": "f64", "Ptr{Int64}": "i64*", "Ptr{Int32}": "i32*", "Ptr{Cdouble}": "f64*"}
    assert ret == "Cint" and [jkind[a] for a in re.findall(r"Ptr\{\w+\}|\w+", argt)] == want
    assert "hip_nlp_attach_general(" in jl


def _fd_check(p, x, lam, sigma=0.7, h=1e-6):
    lay = nlp_terms_layout(p)
    R = NlpGeneralRef(p)
    E = np.eye(p.n)
    fd_grad = np.array([(R.f(x + h * E[j]) - R.f(x - h * E[j])) / (2 * h) for j in range(p.n)])
    assert rel(R.grad(x), fd_grad) < 1e-8
    if p.m:
        fd_J = np.stack([(R.g(x + h * E[j]) - R.g(x - h * E[j])) / (2 * h) for j in range(p.n)], axis=1)
        assert rel(_dense_jac(R, lay, x), fd_J) < 1e-8
    L = lambda y: sigma * R.grad(y) + _dense_jac(R, lay, y).T @ lam
    fd_H = np.stack([(L(x + h * E[j]) - L(x - h * E[j])) / (2 * h) for j in range(p.n)], axis=1)
    H = np.zeros((p.n, p.n)); H[lay.hrow - 1, lay.hcol - 1] = R.hess(x, sigma, lam, lay.hrow, lay.hcol)
    assert np.all(lay.hrow >= lay.hcol)
    assert rel(np.tril(fd_H), H) < 1e-7
    return R


def test_reference_evaluator_matches_finite_differences():
    """gradient and Jacobian from f / g, the Hessian from the analytic gradient (central differences, h = 1e-6: truncation
    h^2 f''' and rounding eps / h both near 1e-10 for values of order 1)"""
    rng = np.random.default_rng(0)
    p = nlp_general_synth(12, 8, seed=3)
    x = rng.uniform(0.5, 1.5, p.n); lam = rng.standard_normal(p.m)
    R = _fd_check(p, x, lam)
    assert set(p.fkind.tolist()) == set(range(POWR + 1)) and needs_general(p)        # the whole menu, shared variables
    assert R.domain_margin(x) > 0
    p, _ = general_edge_model()
    _fd_check(p, rng.uniform(0.5, 1.6, p.n), rng.standard_normal(p.m))


def test_the_old_class_agrees_with_the_earlier_reference_and_factor_values_with_the_new_one():
    rng = np.random.default_rng(4)
    for q in (nlp_terms_synth(24, 14, seed=5), nlp_affine_synth(24, 14, seed=1)):
        assert not needs_general(q)
        lay = nlp_terms_layout(q)
        x = np.clip(q.x0 + 0.3 * rng.standard_normal(q.n), 0.25, 2.9); lam = rng.standard_normal(q.m)
        A, G = NlpAffineRef(q), NlpGeneralRef(q)
        assert rel(G.f(x), A.f(x)) <= 1e-14 and rel(G.grad(x), A.grad(x)) <= 1e-14 and rel(G.g(x), A.g(x)) <= 1e-14
        assert rel(G.jac(x, lay.jrow, lay.jcol), A.jac(x, lay.jrow, lay.jcol)) <= 1e-14
        assert rel(G.hess(x, 1.3, lam, lay.hrow, lay.hcol), A.hess(x, 1.3, lam, lay.hrow, lay.hcol)) <= 1e-14
    # factor_values (the package's own, used to place row bounds) against the reference's kappa on every kind
    for p in (gpu_model()[0], general_edge_model()[0], saturation_model()[0]):
        R = NlpGeneralRef(p)
        x = np.clip(p.x0 + 0.1 * rng.standard_normal(p.n), 0.25, 2.9)
        want = np.array([k[0] for t in range(len(p.trow)) for k in R._eval(x, t)])
        got = factor_values(p, x)
        assert np.all(np.isfinite(got)) and rel(got, want) <= 1e-15
        assert rel(nlp_terms_rows(p, x), R.g(x)) <= 1e-14


def test_product_of_overlapping_affine_forms_by_hand():
    """(x + y)(x - y) = x^2 - y^2: Hessian values [2, 0, -2] at (1,1), (2,1), (2,2) exactly, every value that of the
    x^2 - y^2 model"""
    prod = make_nlp_terms(2, 1, 0, [(1, 1.0, [([(1, 1.0), (2, 1.0)], POW, 1, 0.0), ([(1, 1.0), (2, -1.0)], POW, 1, 0.0)])])
    sq = make_nlp_terms(2, 1, 0, [(1, 1.0, [(1, POW, 2)]), (1, -1.0, [(2, POW, 2)])])
    assert needs_general(prod) and not needs_general(sq)
    assert prod.general and not sq.general                                # make_nlp_terms records it: Context.nlp_attach goes by the record
    lay = nlp_terms_layout(prod)
    assert list(zip(lay.hrow.tolist(), lay.hcol.tolist())) == [(1, 1), (2, 1), (2, 2)]
    assert list(zip(lay.jrow.tolist(), lay.jcol.tolist())) == [(1, 1), (1, 2)]
    P, S = NlpGeneralRef(prod), NlpGeneralRef(sq)
    lam = np.array([1.0])
    for x in (np.array([1.5, -0.25]), np.array([0.3, 2.0])):
        assert P.hess(x, 1.0, lam, lay.hrow, lay.hcol).tolist() == [2.0, 0.0, -2.0]
        assert abs(P.g(x)[0] - S.g(x)[0]) <= 1e-15 * max(1.0, abs(S.g(x)[0]))
        assert rel(P.jac(x, lay.jrow, lay.jcol), S.jac(x, lay.jrow, lay.jcol)) <= 1e-15
        assert S.hess(x, 1.0, lam, [1, 2], [1, 2]).tolist() == [2.0, -2.0]
    # x log x: d/dx = log x + 1, d2/dx2 = 1 / x, from one POW and one LOG factor on the same variable
    ent = make_nlp_terms(1, 0, 0, [(0, 1.0, [(1, POW), (1, LOG)])])
    E = NlpGeneralRef(ent)
    x = np.array([0.37])
    assert abs(E.f(x) - x[0] * np.log(x[0])) <= 1e-16 and abs(E.grad(x)[0] - (np.log(x[0]) + 1.0)) <= 1e-15
    assert abs(E.hess(x, 1.0, np.zeros(0), [1], [1])[0] - 1.0 / x[0]) <= 1e-15


def test_generator_invariants():
    p, lay = gpu_model()
    b, _ = gpu_model()
    import dataclasses
    for f in dataclasses.fields(p):
        assert np.array_equal(getattr(p, f.name), getattr(b, f.name)), f.name       # deterministic per seed
    aptr, avar, acoef = nlp_terms_args(p)
    shared = twice = 0
    for t in range(len(p.trow)):
        vs = [avar[aptr[k]:aptr[k + 1]].tolist() for k in range(p.tptr[t], p.tptr[t + 1])]
        twice += sum(len(set(v)) != len(v) for v in vs)
        shared += len({x for v in vs for x in v}) < sum(len(v) for v in vs)
    assert shared >= 8 and twice == 0                                     # variables shared between factors, never inside one
    assert set(NEW_KINDS) <= set(p.fkind.tolist()) and p.fpar is not None
    assert np.all((p.fpar != 0) == (p.fkind == POWR)) and np.all(np.isfinite(p.fpar))
    # the domains stay positive over the whole box: positive coefficients and a shift >= 0 on LOG, SQRT, POWR, negative powers
    k = np.flatnonzero(np.isin(p.fkind, (LOG, SQRT, POWR)) | ((p.fkind == POW) & (p.fexp < 0)))
    assert len(k) and all(np.all(acoef[aptr[i]:aptr[i + 1]] > 0) and p.fshift[i] >= 0 for i in k)
    lo = min(float(acoef[aptr[i]:aptr[i + 1]] @ p.xL[avar[aptr[i]:aptr[i + 1]] - 1]) + p.fshift[i] for i in k)
    assert lo >= 0.1
    R = NlpGeneralRef(p)
    g = R.g(p.x0)
    assert np.all(g >= p.gL - 1e-12) and np.all(g <= p.gU + 1e-12) and np.all(p.x0 >= p.xL) and np.all(p.x0 <= p.xU)
    for t in np.flatnonzero((p.trow >= 1) & (p.trow <= p.num_linear)):   # linear rows: single plain one-argument factors
        kf = p.tptr[t]
        assert p.tptr[t + 1] - kf == 1 and aptr[kf + 1] - aptr[kf] == 1
        assert (p.fkind[kf], p.fexp[kf], acoef[aptr[kf]], p.fshift[kf]) == (POW, 1, 1.0, 0.0)
    big = nlp_general_synth(600, 500, seed=2)
    assert len(big.trow) > 1024 and len(big.fkind) > 2048 and len(big.avar) > 4096 and needs_general(big)


def _needed(p):
    """the entries the header of sqphip_nlp_attach_general lists"""
    n = p.n
    aptr, avar, _ = nlp_terms_args(p)
    need_j, need_h = set(), set()
    for t in range(len(p.trow)):
        args = [(k, int(avar[j]) - 1) for k in range(p.tptr[t], p.tptr[t + 1]) for j in range(aptr[k], aptr[k + 1])]
        plain = lambda k: p.fkind[k] == POW and p.fexp[k] == 1
        for i, (k, v) in enumerate(args):
            if p.trow[t] > 0:
                need_j.add((int(p.trow[t]) - 1) * n + v)
            if not plain(k):
                need_h.add(v * n + v)                                     # every argument of a factor that is not plain linear
            for k2, w in args[:i]:
                if k2 != k or not plain(k):                               # different factors, or one factor that is not plain
                    need_h.add(max(v, w) * n + min(v, w))                 # (v = w: a variable that sits in two factors)
    return need_j, need_h


def test_layout_structures_have_exactly_the_needed_entries():
    for p in (gpu_model()[0], nlp_general_synth(30, 20, seed=5), general_edge_model()[0], saturation_model()[0]):
        lay = nlp_terms_layout(p)
        n = p.n
        jk = ((lay.jrow - 1) * n + lay.jcol - 1).tolist()
        hk = ((lay.hrow - 1) * n + lay.hcol - 1).tolist()
        assert len(set(jk)) == len(jk) and len(set(hk)) == len(hk)                   # no duplicates
        need_j, need_h = _needed(p)
        assert set(jk) == need_j and set(hk) == need_h                               # nothing missing, nothing spurious
        assert np.all(lay.hrow >= lay.hcol)
    # a variable in two plain linear factors gets its diagonal entry; alone in one it gets none
    p = make_nlp_terms(3, 1, 0, [(1, 1.0, [(1, POW), ([(1, 2.0), (2, 1.0)], POW, 1, 0.5), (3, POW)])])
    lay = nlp_terms_layout(p)
    assert sorted(zip(lay.hrow.tolist(), lay.hcol.tolist())) == [(1, 1), (2, 1), (3, 1), (3, 2)]
    # POWR with p = 1 is not plain
    p = make_nlp_terms(1, 1, 0, [(1, 1.0, [(1, POWR, 1.0)])])
    assert list(zip(nlp_terms_layout(p).hrow.tolist(), nlp_terms_layout(p).hcol.tolist())) == [(1, 1)] and p.fpar.tolist() == [1.0]


def test_edge_model_is_what_the_gpu_test_says_it_is():
    p, lay = general_edge_model()
    aptr, avar, _ = nlp_terms_args(p)
    assert np.diff(p.tptr)[0] == 8 and np.diff(aptr)[:8].tolist() == [8, 1, 2, 3, 2, 2, 2, 2]
    assert all(1 in avar[aptr[k]:aptr[k + 1]] for k in range(8))                     # variable 1 in every factor of term 1
    for kind in NEW_KINDS:
        na = np.diff(aptr)[p.fkind == kind]
        assert (na == 1).any() and (na > 1).any(), kind
    assert sorted(p.fpar[p.fkind == POWR].tolist()) == [-0.7, 0.5, 1.5]
    assert (1 + p.m + len(p.trow)) % 2 == 1
    R = NlpGeneralRef(p)
    x = np.linspace(0.6, 1.5, p.n)
    assert R.grad(x)[29] != 0.0 and 30 not in lay.jcol.tolist()                                              # variable 30: in the objective only
    assert R.domain_margin(np.full(p.n, 0.2)) > 0 and R.domain_margin(np.full(p.n, 3.0)) > 0


def test_builders_have_their_known_answers_on_the_oracle():
    import scipy.optimize
    kw = dict(max_iter=60, literal_quirks=0, tol_infeas=1e-8, tol_residual=1e-8)
    c = np.array([0.3, -0.5, 1.2, 0.0, 0.8, -1.0])
    alpha, prices, wealth = np.array([0.2, 0.3, 0.4]), np.array([1.0, 2.0, 0.5]), 10.0
    X, y, reg = logistic_data()
    loss = lambda w: float(np.sum(np.logaddexp(0.0, X @ w) - y * (X @ w)) + 0.5 * reg * (w @ w))
    wopt = scipy.optimize.minimize(loss, np.zeros(3), method="BFGS", options=dict(gtol=1e-10)).x
    for p, want in ((entropy_model(c), np.exp(-c) / np.exp(-c).sum()), (cobb_douglas_model(alpha, prices, wealth), alpha * wealth / (prices * alpha.sum())),
                    (logistic_model(X, y, reg), wopt)):
        assert needs_general(p)
        r = O.sqp_solve(OracleGeneralTerms(p, nlp_terms_layout(p)), O.default_options(kkt_mode=2, **kw))
        assert r["status"] == 0 and np.abs(r["x"] - want).max() <= 1e-6, (r["status"], r["x"], want)
    assert abs(NlpGeneralRef(logistic_model(X, y, reg)).f(wopt) - loss(wopt)) <= 1e-13 * max(1.0, abs(loss(wopt)))


def logistic_data():
    rng = np.random.default_rng(4)
    X = np.c_[np.ones(12), rng.standard_normal((12, 2))]
    y = (X @ np.array([0.3, 1.0, -0.7]) + 0.5 * rng.standard_normal(12) > 0).astype(float)
    return X, y, 0.5


def _oracle_run(lay, p, kkt_mode=2):
    r = O.sqp_solve(OracleGeneralTerms(p, lay), O.default_options(kkt_mode=kkt_mode, **({"kkt_tile_order": 1} if kkt_mode == 1 else {}), **SQP_KW))
    R = NlpGeneralRef(p)
    assert r["status"] == 0 and r["iter"] < SQP_KW["max_iter"], (r["status"], r["iter"])
    assert R.domain_margin(r["x"]) > 0                                               # LOG / SQRT / POWR stayed inside their domain
    g = R.g(r["x"])
    assert np.all(g >= p.gL - 1e-6) and np.all(g <= p.gU + 1e-6)
    return r["iter"]


@pytest.mark.parametrize("kkt_mode", [2, 1])
@pytest.mark.parametrize("scenario", GPU_SCENARIOS)
def test_oracle_converges_on_the_generated_instances_of_the_gpu_tests(scenario, kkt_mode):
    base, lay = gpu_model()
    try:
        _oracle_run(lay, gpu_scenarios(base, (scenario,))[0], kkt_mode)
    finally:
        O.set_kkt_order(None)


def test_oracle_converges_on_the_scenarios_of_the_queue_test():
    base, lay = gpu_model()
    iters = [_oracle_run(lay, p) for p in gpu_scenarios(base, QUEUE_SCENARIOS, QUEUE_NOISE)]
    print("iterations", iters)
    assert len(set(iters)) > 1                                                       # slots of the queue refill at different times
