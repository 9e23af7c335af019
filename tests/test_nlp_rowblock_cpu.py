"""Dense data blocks with several outputs (nlp_terms.NlpRowBlock, sqphip_nlp_add_row_block) without a device: the 50-digit
reference of tests/nlp_rowblock_ref.py against numpy and against the same model written as per-point terms, the layout, the
refusals of the Python layer, the ABI, and scipy's and the oracle's word for the cases that tests/test_gpu_nlp_rowblock.py solves."""
import dataclasses
import itertools
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from sqpsolver_jl_amd import _lib                                     # noqa: E402
from sqpsolver_jl_amd.nlp_terms import (POW, SIGMOID, SOFTPLUS, NlpBlock, NlpRowBlock, make_nlp_terms, nlp_terms_layout,   # noqa: E402
                                        row_block_eval)
from oracle import oracle as O                                        # noqa: E402
from nlp_general_ref import NlpGeneralRef                             # noqa: E402
from nlp_rowblock_ref import (EDGE_CASES, EDGE_LAM, NP_ALPHA, NP_ALPHAS, NP_OPTS, NP_REG, SQP_TIGHT, NlpRowBlockNumpy, NlpRowBlockRef,   # noqa: E402
                              OracleRowBlockTerms, check_outputs, edge_row_model, np_case, np_data, np_fold_models, np_scipy,
                              overlap_model, per_point_terms, rate_case)


def _numpy_outputs(ref, x, sigma, lam, lay):
    return dict(f=ref.f(x), grad=ref.grad(x), g=ref.g(x), jval=ref.jac(x, lay.jrow, lay.jcol), hval=ref.hess(x, sigma, lam, lay.hrow, lay.hcol))


@pytest.mark.parametrize("N,d,rows,kind,e", EDGE_CASES, ids=[f"N{N}-d{d}-R{len(r)}-k{k}e{e}" for N, d, r, k, e in EDGE_CASES])
def test_reference_agrees_with_numpy_within_the_bound(N, d, rows, kind, e):
    p, lay, inst = edge_row_model(N, d, rows, kind, e)
    x = np.random.default_rng(N + d).uniform(0.6, 1.4, p.n)
    for sigma in (0.7, 0.0):
        val, bnd = NlpRowBlockRef(p).want(x, sigma, EDGE_LAM, lay)
        got = _numpy_outputs(NlpRowBlockNumpy(p), x, sigma, EDGE_LAM, lay)
        check_outputs(got, val, bnd, f"{(N, d, rows, kind, e)} sigma {sigma}")
        assert np.all(got["hval"][-2:] == 0.0) and np.all(got["jval"][-2:] == 0.0)
    # the block moves every target and nothing else
    terms = _numpy_outputs(NlpRowBlockNumpy(dataclasses.replace(p, blocks=[])), x, 0.7, EDGE_LAM, lay)
    moved = np.flatnonzero(np.abs(val["g"] - terms["g"]) > 0) + 1
    assert set(moved.tolist()) == {i for i in rows if i >= 1}
    assert (abs(val["f"] - terms["f"]) > 0) == (0 in rows)


def test_reference_agrees_with_the_model_written_as_per_point_terms():
    p, lay, inst = edge_row_model(9, 5, (0, 3, 2), SOFTPLUS, 1)       # d <= 8: one factor per point holds a row of A
    pp = per_point_terms(p)
    layp = nlp_terms_layout(pp)
    assert set(zip(layp.jrow, layp.jcol)) == set(zip(lay.jrow, lay.jcol)) and set(zip(layp.hrow, layp.hcol)) == set(zip(lay.hrow, lay.hcol))
    x = np.random.default_rng(3).uniform(0.6, 1.4, p.n)
    val, bnd = NlpRowBlockRef(p).want(x, 0.7, EDGE_LAM, lay)
    got = _numpy_outputs(NlpGeneralRef(pp), x, 0.7, EDGE_LAM, lay)
    check_outputs(got, val, bnd, "per-point terms")


def test_overlap_model_shares_entries():
    p, lay = overlap_model()
    x = np.random.default_rng(2).uniform(-1.0, 1.0, p.n); lam = np.array([0.3, -0.6])
    val, bnd = NlpRowBlockRef(p).want(x, 1.3, lam, lay)
    check_outputs(_numpy_outputs(NlpRowBlockNumpy(p), x, 1.3, lam, lay), val, bnd, "overlap")
    shared = [2, 4, 6]
    hs = [s for s, (r, c) in enumerate(zip(lay.hrow - 1, lay.hcol - 1)) if r in shared and c in shared]
    assert len(hs) == 6
    for alone in (p.blocks[:1], p.blocks[1:]):
        only = NlpRowBlockRef(p).want(x, 1.3, lam, lay, blocks=alone)[0]
        assert np.abs(only["grad"][shared] - val["grad"][shared]).min() > 1e-3
        assert np.abs(only["hval"][hs] - val["hval"][hs]).min() > 1e-3


def test_layout_holds_exactly_the_entries_of_the_block():
    n = 7
    blk = NlpRowBlock(SIGMOID, [6, 2, 5], np.ones((4, 3)), [3, 0])
    p = make_nlp_terms(n, 3, 1, [(1, 1.0, [(1, POW)]), (2, 1.0, [(7, POW, 2)])], blocks=[blk])
    lay = nlp_terms_layout(p)
    assert sorted(zip(lay.jrow.tolist(), lay.jcol.tolist())) == [(1, 1), (2, 7), (3, 2), (3, 5), (3, 6)]
    assert sorted(zip(lay.hrow.tolist(), lay.hcol.tolist())) == [(2, 2), (5, 2), (5, 5), (6, 2), (6, 5), (6, 6), (7, 7)]
    # an output on row 0 alone adds no Jacobian entry
    q = make_nlp_terms(n, 3, 1, [(1, 1.0, [(1, POW)])], blocks=[dataclasses.replace(blk, rows=[0], weight=None)])
    assert sorted(zip(nlp_terms_layout(q).jrow.tolist(), nlp_terms_layout(q).jcol.tolist())) == [(1, 1)]


def test_python_refusals():
    A = np.ones((4, 3))
    with pytest.raises(ValueError, match="R = 0"):
        NlpRowBlock(SOFTPLUS, [1, 2, 3], A, [])
    with pytest.raises(ValueError, match="R = 9"):
        NlpRowBlock(SOFTPLUS, [1, 2, 3], A, list(range(9)))
    with pytest.raises(ValueError, match="two outputs"):
        NlpRowBlock(SOFTPLUS, [1, 2, 3], A, [2, 0, 2])
    with pytest.raises(ValueError, match="R N = 2 x 4"):
        NlpRowBlock(SOFTPLUS, [1, 2, 3], A, [0, 2], None, np.ones(4))
    mk = lambda rows, cols=(1, 2, 3): make_nlp_terms(5, 3, 1, [], blocks=[NlpRowBlock(SOFTPLUS, list(cols), A, rows)])
    with pytest.raises(ValueError, match="block 1: a row outside 0..3"):
        mk([0, 4])
    with pytest.raises(ValueError, match="block 1: a row among the num_linear = 1 linear rows"):
        mk([1])
    with pytest.raises(ValueError, match="block 1: a column outside 1..5"):
        mk([0], (1, 2, 6))
    assert mk([0, 2, 3]).blocks[0].weight.shape == (3, 4)
    with pytest.raises(ValueError, match="at most 4"):
        make_nlp_terms(5, 3, 1, [], blocks=[NlpRowBlock(SOFTPLUS, [1, 2, 3], A, [0])] * 5)


def test_row_block_eval_against_finite_differences():
    p, lay = overlap_model()
    x = np.random.default_rng(5).uniform(-1.0, 1.0, p.n); lam = np.array([0.0, 0.8])
    f, g, gv, J, H = row_block_eval(p, x, 1.3, lam)
    L = lambda z: 1.3 * row_block_eval(p, z)[0] + lam @ row_block_eval(p, z)[2]
    h = 1e-5
    for j in range(p.n):
        e = np.zeros(p.n); e[j] = h
        assert np.allclose((row_block_eval(p, x + e)[2] - row_block_eval(p, x - e)[2]) / (2 * h), J[:, j], atol=1e-8)
        assert abs((row_block_eval(p, x + e)[0] - row_block_eval(p, x - e)[0]) / (2 * h) - g[j]) <= 1e-8
        dg = (1.3 * (row_block_eval(p, x + e)[1] - row_block_eval(p, x - e)[1]) + lam @ (row_block_eval(p, x + e)[3] - row_block_eval(p, x - e)[3])) / (2 * h)
        assert np.allclose(dg, H[:, j], atol=1e-7)
    assert np.isfinite(L(x))


def test_abi_and_python_layer_know_the_call():
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sqphip.h")).read(), flags=re.S)
    m = re.search(r"int\s+sqphip_nlp_add_row_block\s*\(([^;]*)\)\s*;", code)
    assert m and len(m.group(1).split(",")) == 13
    L = _lib.lib()
    assert "sqphip_nlp_add_row_block" in _lib.EXPORTS and hasattr(L, "sqphip_nlp_add_row_block")
    assert "nlp_rowblock_dev.hpp" in _lib.HEADERS
    assert L.sqphip_nlp_add_row_block(None, 9, 1, 0.0, 1, 1, None, None, 1, None, None, None, None) == -1      # a NULL handle


# ---- the solved cases of the GPU tests
def test_neyman_pearson_case_is_vouched_for_by_scipy_and_the_oracle():
    import scipy.optimize
    X, y, p = np_case()
    x1, x2, mult = np_scipy(X, y, NP_ALPHA, NP_REG)
    assert np.abs(x1 - x2).max() <= 5e-8 and abs(abs(mult) - 34.6) < 0.1
    sp = lambda u: np.logaddexp(0.0, u)
    free = scipy.optimize.minimize(lambda b: float((y == 1) @ (sp(X @ b) - X @ b) + 0.5 * NP_REG * (b @ b)), np.zeros(6), method="BFGS",
                                   options=dict(gtol=1e-10)).x
    assert abs((y == 0) @ sp(X @ free) / (y == 0).sum() - 2.13) < 0.01           # the unconstrained fit violates the row
    lay = nlp_terms_layout(p)
    try:
        ro = O.sqp_solve(OracleRowBlockTerms(p, lay), O.default_options(kkt_mode=2, **NP_OPTS))
        stall = O.sqp_solve(OracleRowBlockTerms(p, lay), O.default_options(kkt_mode=2, **SQP_TIGHT))
    finally:
        O.set_kkt_order(None)
    assert ro["status"] == 0 and np.abs(ro["x"] - x2).max() <= 1e-6 and abs(abs(ro["mult_g"][0]) - abs(mult)) <= 1e-4
    assert abs(ro["g"][0] - NP_ALPHA) <= 1e-8
    assert stall["status"] != 0                                       # (NP_OPTS: why the penalty starts above the multiplier)


def test_fold_cases_are_vouched_for_by_scipy_and_the_oracle():
    X, y = np_data()
    ps = np_fold_models(extra=2)
    lay = nlp_terms_layout(ps[0])
    xs = []
    try:
        for s, p in enumerate(ps):
            ro = O.sqp_solve(OracleRowBlockTerms(p, nlp_terms_layout(p)), O.default_options(kkt_mode=2, **NP_OPTS))      # (its own level)
            assert ro["status"] == 0 and abs(ro["g"][0] - p.gU[0]) <= 1e-8 and abs(ro["mult_g"][0]) > 1.0, s
            xs.append(ro["x"])
    finally:
        O.set_kkt_order(None)
    assert min(np.abs(a - b).max() for a, b in itertools.combinations(xs, 2)) > 1e-3
    from sqpsolver_jl_amd.nlp_terms import fold_weights
    W = fold_weights(60, 4)
    for s in (0, 2):
        assert np.abs(np_scipy(X, y, NP_ALPHAS[s], NP_REG, W[s])[1] - xs[s]).max() <= 1e-6


def test_rate_equality_case_ends_inside_the_tight_options():
    X, y, group, p = rate_case()
    lay = nlp_terms_layout(p)
    try:
        ro = O.sqp_solve(OracleRowBlockTerms(p, lay), O.default_options(kkt_mode=2, **SQP_TIGHT))
    finally:
        O.set_kkt_order(None)
    s = 1.0 / (1.0 + np.exp(-(X @ ro["x"])))
    assert ro["status"] == 0 and ro["iter"] < SQP_TIGHT["max_iter"]
    assert abs(s[group == 1].mean() - s[group == 0].mean()) <= 1e-8 and abs(ro["mult_g"][0]) > 1.0
    assert isinstance(p.blocks[0], NlpBlock) and isinstance(p.blocks[1], NlpRowBlock)
