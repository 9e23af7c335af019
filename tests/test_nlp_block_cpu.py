"""Dense data blocks of a factorable NLP, the parts that need no GPU: the 50-digit reference (tests/nlp_block_ref.py) against
finite differences and against numpy, the layout, the builders' closed forms, and the oracle's word for every case that
tests/test_gpu_nlp_block.py solves."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from sqpsolver_jl_amd.nlp_terms import (EXP, LOG, POW, SIGMOID, SOFTPLUS, NlpBlock, block_eval, fold_weights,   # noqa: E402
                                        least_squares_block_model, logistic_block_model, logistic_fold_indices,
                                        logistic_model, make_nlp_terms, nlp_terms_layout, poisson_block_model)
from oracle import oracle as O                                        # noqa: E402
from nlp_general_ref import NlpGeneralRef, OracleGeneralTerms                             # noqa: E402
from nlp_block_ref import (EDGE_CASES, SQP_TIGHT, NlpBlockNumpy, NlpBlockRef, OracleBlockTerms, block_reference,   # noqa: E402
                           both_paths_case, edge_model, folds_case, newton_logistic, newton_poisson, poisson_case, rows_case,
                           two_block_model)


@pytest.mark.parametrize("kind,e", [(SOFTPLUS, 1), (SIGMOID, 1), (EXP, 1), (POW, 2), (POW, -1), (LOG, 1)])
def test_reference_matches_numpy_and_finite_differences(kind, e):
    p, lay, _ = edge_model(5, 17, kind, e)
    b = p.blocks[0]
    x = np.linspace(0.6, 1.4, p.n)
    (f, g, H), (Bf, Bg, BH) = block_reference(b, x, 1.0)
    fn, gn, Hn = block_eval(p, x)
    c = b.cols - 1
    assert abs(f - fn) <= 4 * Bf and np.all(np.abs(g - gn[c]) <= 4 * Bg) and np.all(np.abs(H - Hn[np.ix_(c, c)]) <= 4 * BH)
    assert Bf > 0 and np.all(Bg > 0) and np.all(BH > 0) and np.all(BH <= 1e-12 * max(1.0, np.abs(H).max()))
    h = 1e-6
    for j in (0, 7, 16):
        dx = np.zeros(p.n); dx[c[j]] = h
        fp, gp, _ = block_eval(p, x + dx)
        fm, gm, _ = block_eval(p, x - dx)
        assert abs((fp - fm) / (2 * h) - g[j]) <= 1e-7 * max(1.0, abs(g[j]))
        assert np.all(np.abs((gp - gm)[c] / (2 * h) - H[:, j]) <= 1e-6 * max(1.0, np.abs(H).max()))


def test_layout_holds_every_pair_of_block_columns():
    p, lay, _ = edge_model(5, 17, SOFTPLUS, 1)
    pairs = set(zip(lay.hrow.tolist(), lay.hcol.tolist()))
    cols = p.blocks[0].cols.tolist()
    assert cols != sorted(cols) and max(cols) - min(cols) + 1 > len(cols)          # unsorted, not contiguous
    assert all((max(a, b), min(a, b)) in pairs for a in cols for b in cols)
    assert all(r >= c for r, c in pairs)
    q, layq = two_block_model()
    pairs = set(zip(layq.hrow.tolist(), layq.hcol.tolist()))
    for b in q.blocks:
        assert all((max(a, c), min(a, c)) in pairs for a in b.cols.tolist() for c in b.cols.tolist())
    assert (12, 1) not in pairs                                                     # variables of different blocks only
    # a problem without blocks keeps its layout
    t = make_nlp_terms(3, 0, 0, [(0, 1.0, [(1, POW, 2)]), (0, 1.0, [(2, POW), (3, POW)])])
    assert t.blocks == [] and list(zip(nlp_terms_layout(t).hrow, nlp_terms_layout(t).hcol)) == [(1, 1), (3, 2)]


def test_builders_closed_forms():
    X, y, reg, pb, pt = both_paths_case()
    rng = np.random.default_rng(1)
    for _ in range(3):
        w = rng.standard_normal(6)
        want = float(np.sum(np.logaddexp(0.0, X @ w) - y * (X @ w)) + 0.5 * reg * (w @ w))
        assert abs(NlpBlockNumpy(pb).f(w) - want) <= 1e-12 * abs(want)              # softplus(u) - y u = softplus((1 - 2 y) u)
        assert abs(NlpGeneralRef(pt).f(w) - want) <= 1e-12 * abs(want)
        assert np.abs(NlpBlockNumpy(pb).grad(w) - NlpGeneralRef(pt).grad(w)).max() <= 1e-12
    assert len(pb.trow) == 6 and pb.blocks[0].kind == SOFTPLUS                      # no linear terms: folds differ in weights only
    W = fold_weights(11, 3)
    for f, (tr, va) in enumerate(logistic_fold_indices(11, 3)):
        assert np.array_equal(np.flatnonzero(W[f]), np.sort(tr)) and not W[f, va].any() and not W[f, 9:].any()
    Xp, c, regp, Wp = poisson_case()
    pp = poisson_block_model(Xp, c, regp, Wp[1])
    b = 0.1 * rng.standard_normal(20)
    want = float(Wp[1] @ (np.exp(Xp @ b) - c * (Xp @ b)) + 0.5 * regp * (b @ b))
    assert abs(NlpBlockNumpy(pp).f(b) - want) <= 1e-12 * abs(want)
    A = rng.standard_normal((7, 3)); m = rng.standard_normal(7)
    pl = least_squares_block_model(A, m, 0.2)
    v = rng.standard_normal(3)
    assert abs(NlpBlockNumpy(pl).f(v) - (np.sum((A @ v - m) ** 2) + 0.1 * (v @ v))) <= 1e-12
    assert pl.blocks[0].exp == 2 and np.array_equal(pl.blocks[0].shift, -m)


def test_hessian_of_two_blocks_on_overlapping_columns_counts_every_entry_once():
    p, lay = two_block_model()
    x = np.linspace(-0.4, 0.6, p.n)
    val, bnd = NlpBlockRef(p).want(x, 0.7, np.zeros(0), lay)
    got = NlpBlockNumpy(p)
    hv = got.hess(x, 0.7, np.zeros(0), lay.hrow, lay.hcol)
    assert np.all(np.abs(hv - val["hval"]) <= 4 * bnd["hval"] + 1e-13 * np.abs(val["hval"]).max())
    assert np.all(np.abs(got.grad(x) - val["grad"]) <= 4 * bnd["grad"] + 1e-13 * np.abs(val["grad"]).max())


# ---- the oracle converges on every case the GPU tests solve
def _solve(p, lay=None):
    ro = O.sqp_solve(OracleBlockTerms(p, lay), O.default_options(**SQP_TIGHT))
    assert ro["status"] == 0, ro["status"]
    return ro


def test_oracle_on_both_paths_case_reaches_the_scipy_optimum():
    import scipy.optimize
    X, y, reg, pb, pt = both_paths_case()
    loss = lambda w: float(np.sum(np.logaddexp(0.0, X @ w) - y * (X @ w)) + 0.5 * reg * (w @ w))
    want = scipy.optimize.minimize(loss, np.zeros(6), method="BFGS", options=dict(gtol=1e-10)).x
    assert np.abs(_solve(pb)["x"] - want).max() <= 1e-6
    ro = O.sqp_solve(OracleGeneralTerms(pt), O.default_options(**SQP_TIGHT))
    assert ro["status"] == 0 and np.abs(ro["x"] - want).max() <= 1e-6
    assert np.abs(newton_logistic(X, y, reg, np.ones(40))[0] - want).max() <= 1e-6


def test_oracle_on_the_folds_and_newton_facts():
    X, y, reg, W = folds_case()
    sol = [newton_logistic(X, y, reg, w) for w in W]
    assert all(it <= 8 for _, it in sol) and max(np.abs(b).max() for b, _ in sol) <= 1.7
    assert min(np.abs(sol[a][0] - sol[b][0]).max() for a in range(4) for b in range(a)) > 1e-3
    for f in range(4):
        assert np.abs(_solve(logistic_block_model(X, y, reg, W[f]))["x"] - sol[f][0]).max() <= 1e-6, f


def test_oracle_on_a_poisson_bootstrap():
    X, c, reg, W = poisson_case()
    for w in list(W) + [np.ones(150)]:                                 # the six resamples and the add call's unit weights
        b, it = newton_poisson(X, c, reg, w)
        assert it <= 8 and np.abs(b).max() < 50
        assert np.abs(_solve(poisson_block_model(X, c, reg, w))["x"] - b).max() <= 1e-6


def test_oracle_on_the_rows_case_with_active_bounds():
    import dataclasses
    p, lay, shifts = rows_case()
    for s in shifts:
        q = dataclasses.replace(p, blocks=[dataclasses.replace(p.blocks[0], shift=s)])
        ro = _solve(q, lay)
        assert (np.abs(ro["x"] - p.xL) < 1e-7).any() or (np.abs(ro["x"] - p.xU) < 1e-7).any()
        assert abs(ro["x"].sum() - 1.0) <= 1e-8


def test_edge_cases_cover_the_shape_edges():
    shapes = {(N, d) for N, d, _, _ in EDGE_CASES}
    assert {N % 4 for N, _ in shapes} == {0, 1, 2, 3} and {0, 1, 15} <= {d % 16 for _, d in shapes}
    assert any(N > 1024 for N, _ in shapes) and (130, 128) in shapes
    assert {(k, e) for _, _, k, e in EDGE_CASES} == {(SOFTPLUS, 1), (SIGMOID, 1), (EXP, 1), (POW, 2), (POW, -1), (LOG, 1)}
    for N, d, kind, e in EDGE_CASES[1:5]:                      # (N = 1 has room for one weight only)
        p, lay, inst = edge_model(N, d, kind, e)
        assert len(lay.hrow) == len(set(zip(lay.hrow.tolist(), lay.hcol.tolist()))) + 2            # duplicated slots
        assert any((w == 0).any() for w, _ in inst) and all((w < 0).any() for w, _ in inst)
