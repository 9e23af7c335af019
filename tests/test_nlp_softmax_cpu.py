"""Multinomial (softmax) data blocks of a factorable NLP, the parts that need no GPU: numpy's block_eval against the 50-digit
reference and its bound (tests/nlp_softmax_ref.py) at every shape edge, the bound against planted mistakes, finite
differences, the K = 2 pinned block against the softplus block, layout, builder and refusals, the oracle's and Newton's word
for the solved cases, header and binding."""
import dataclasses
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from sqpsolver_jl_amd import _lib                                       # noqa: E402
from sqpsolver_jl_amd.nlp_terms import (POW, NlpBlock, NlpSoftmaxBlock, block_eval, logistic_block_model, make_nlp_terms,   # noqa: E402
                                        multinomial_block_model, nlp_terms_layout)
from oracle import oracle as O                                        # noqa: E402
from nlp_block_ref import NlpBlockRef                                 # noqa: E402
from nlp_softmax_ref import (BIG_LOGITS, EDGE_CASES, SQP_TIGHT, NlpSoftmaxNumpy, NlpSoftmaxRef, OracleSoftmaxTerms,   # noqa: E402
                             check_outputs, edge_model, edge_reference, folds_case3, mixed_model, newton_multinomial,
                             queue_case, rows_case, softmax_reference, with_block)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_EDGES = [(c, False) for c in EDGE_CASES] + [(BIG_LOGITS, True)]
IDS = ["N%d-d%d-K%d-pinned%d" % c + ("-big" if big else "") for c, big in ALL_EDGES]
OUT = ("f", "grad", "hval")


def _accepts(got, val, bnd):
    """the acceptance rule per output: {key: bool}"""
    ok = {}
    for key in OUT:
        g_, w_, b_ = (np.atleast_1d(np.asarray(a, float)) for a in (got[key], val[key], bnd[key]))
        ok[key] = bool(np.all(np.abs(g_ - w_) <= 4.0 * b_ + 1e-13 * np.abs(w_).max()))
    return ok


# ---- (a) numpy meets the bound at every edge; (b) the bound is not vacuous there
@pytest.mark.parametrize("case,big", ALL_EDGES, ids=IDS)
def test_numpy_meets_the_bound_and_the_bound_is_tight_enough(case, big):
    q, lay, x, sigma, lam, val, bnd = edge_reference(case, 0, big)
    got = NlpSoftmaxNumpy(q).outputs(x, sigma, lam, lay)
    assert all(np.all(np.isfinite(got[k])) for k in got)
    check_outputs(got, val, bnd, f"numpy {case} big={big}")            # prints err / B (DESIGN 5.8 records the largest)
    for key in OUT:
        ratio = float(np.max(bnd[key]) / np.abs(val[key]).max())
        print("B / max|want|", key, ratio)
        assert ratio <= 1e-10, (key, ratio)


def _planted(q, lay, x, sigma, lam, mistake):
    b = q.blocks[0]
    N = b.A.shape[0]
    if mistake == "label":
        y = b.labels.copy(); y[N // 2] = (y[N // 2] + 1) % b.K
        return NlpSoftmaxNumpy(with_block(q, 0, labels=y)).outputs(x, sigma, lam, lay)
    if mistake == "point":
        i = next(i for i in range(N) if b.weight[i] > 0)
        w = b.weight.copy(); w[i] = 0.0
        return NlpSoftmaxNumpy(with_block(q, 0, weight=w)).outputs(x, sigma, lam, lay)
    # classes k, l swapped in one Hessian block: the block (1, 0) computed with p_1 p_1 in place of p_1 p_0
    got = NlpSoftmaxNumpy(q).outputs(x, sigma, lam, lay)
    Kf, d = b.cols.shape
    u = np.stack([b.A @ x[b.cols[k] - 1] + b.shift[k] for k in range(Kf)])
    if b.pinned:
        u = np.vstack([u, np.zeros(N)])
    e = np.exp(u - u.max(axis=0)); P = e / e.sum(axis=0)
    wrong = -sigma * (b.A.T @ ((b.weight * P[1] * P[1])[:, None] * b.A))
    right = -sigma * (b.A.T @ ((b.weight * P[1] * P[0])[:, None] * b.A))
    slot = {(int(r), int(c)): s for s, (r, c) in reversed(list(enumerate(zip(lay.hrow, lay.hcol))))}
    for j in range(d):
        for j2 in range(d):
            r, c = int(b.cols[1, j]), int(b.cols[0, j2])
            got["hval"][slot[(max(r, c), min(r, c))]] += wrong[j, j2] - right[j, j2]
    return got


@pytest.mark.parametrize("mistake", ["label", "point", "classes"])
def test_planted_mistakes_break_the_acceptance_rule(mistake):
    for case in [(3, 2, 3, 0), (65, 5, 7, 1), (64, 8, 16, 0)]:
        q, lay, x, sigma, lam, val, bnd = edge_reference(case, 0)
        ok = _accepts(_planted(q, lay, x, sigma, lam, mistake), val, bnd)
        assert not all(ok.values()), (mistake, case, ok)


# ---- (c) finite differences
@pytest.mark.parametrize("pinned", [0, 1])
def test_gradient_and_hessian_agree_with_central_differences(pinned):
    p, lay, _ = edge_model(5, 4, 4, pinned)
    b = p.blocks[0]
    x = np.linspace(0.6, 1.4, p.n)
    (f, g, H), _ = softmax_reference(b, x, 1.0)
    c = b.cols.ravel() - 1
    h = 1e-6
    for j in range(len(c)):
        dx = np.zeros(p.n); dx[c[j]] = h
        fp, gp, _ = block_eval(p, x + dx)
        fm, gm, _ = block_eval(p, x - dx)
        assert abs((fp - fm) / (2 * h) - g[j]) <= 1e-7 * max(1.0, abs(g[j]))
        assert np.all(np.abs((gp - gm)[c] / (2 * h) - H[:, j]) <= 1e-6 * max(1.0, np.abs(H).max()))


# ---- (d) K = 2 pinned is the softplus block
def test_two_classes_pinned_equal_the_softplus_block_within_both_bounds():
    rng = np.random.default_rng(40)
    X = np.column_stack([np.ones(40), rng.standard_normal((40, 5))])
    y = (X @ rng.standard_normal(6) + 0.8 * rng.standard_normal(40) > 0).astype(np.int32)
    w = rng.uniform(0.0, 2.0, 40)
    ps = multinomial_block_model(X, y, 2, 0.5, True, w)                # class 0 carries the variables: its "positive" label is y = 0
    pl = logistic_block_model(X, (y == 0).astype(float), 0.5, w)
    ls, ll = nlp_terms_layout(ps), nlp_terms_layout(pl)
    assert np.array_equal(ls.hrow, ll.hrow) and np.array_equal(ls.hcol, ll.hcol)
    x = rng.uniform(-1.0, 1.0, 6)
    vs, bs = NlpSoftmaxRef(ps).want(x, 0.9, np.zeros(0), ls)
    vl, bl = NlpBlockRef(pl).want(x, 0.9, np.zeros(0), ll)
    gs, gl = NlpSoftmaxNumpy(ps).outputs(x, 0.9, np.zeros(0), ls), NlpSoftmaxNumpy(pl).outputs(x, 0.9, np.zeros(0), ll)
    for k in OUT:
        lim = 4.0 * (np.asarray(bs[k]) + np.asarray(bl[k])) + 2e-13 * np.abs(vl[k]).max()
        assert np.all(np.abs(np.asarray(vs[k]) - np.asarray(vl[k])) <= lim), k       # the two references
        assert np.all(np.abs(np.asarray(gs[k]) - np.asarray(gl[k])) <= lim), k       # the two numpy evaluations


# ---- (e) layout, builder, refusals
def test_layout_builder_and_refusals():
    p, lay, _ = edge_model(5, 17, 2, 0)
    pairs = set(zip(lay.hrow.tolist(), lay.hcol.tolist()))
    cols = p.blocks[0].cols.ravel().tolist()
    assert cols != sorted(cols) and max(cols) - min(cols) + 1 > len(cols)          # unsorted, not contiguous
    assert all((max(a, b), min(a, b)) in pairs for a in cols for b in cols) and all(r >= c for r, c in pairs)
    assert len(lay.hrow) == len(pairs) + 2                                         # duplicated slots
    for order in (False, True):
        q, layq = mixed_model(order)
        pairs = set(zip(layq.hrow.tolist(), layq.hcol.tolist()))
        for b in q.blocks:
            c = np.ravel(b.cols).tolist()
            assert all((max(a, e), min(a, e)) in pairs for a in c for e in c)
        assert (13, 1) not in pairs                                                # variables of different blocks only
    X, y, reg, W = folds_case3()
    for pinned, n in ((True, 12), (False, 18)):
        m = multinomial_block_model(X, y, 3, reg, pinned, W[1])
        b = m.blocks[0]
        assert m.n == n and len(m.trow) == n and b.cols.shape == (n // 6, 6) and np.array_equal(b.cols.ravel(), np.arange(1, n + 1))
        assert np.array_equal(b.weight, W[1]) and not b.shift.any() and np.all(m.xL == -50.0) and np.all(m.xU == 50.0)
        v = np.random.default_rng(2).standard_normal(n)
        u = X @ v.reshape(-1, 6).T
        u = np.column_stack([u, np.zeros(150)]) if pinned else u
        want = float(W[1] @ (np.log(np.exp(u).sum(axis=1)) - u[np.arange(150), y])) + 0.25 * (v @ v)
        assert abs(NlpSoftmaxNumpy(m).f(v) - want) <= 1e-12 * abs(want)
    A = np.ones((3, 2))
    for bad in (dict(K=1), dict(K=65), dict(cols=[[1, 2], [3, 1]]), dict(cols=[1, 2, 3]), dict(labels=[0, 1, 3]), dict(labels=[0, -1, 1]),
                dict(labels=[0, 1]), dict(A=np.ones((3, 43)), cols=np.arange(1, 130), K=4)):
        kw = {**dict(cols=[[1, 2], [3, 4]], A=A, labels=[0, 1, 2], K=3, pinned=True), **bad}
        with pytest.raises(ValueError):
            NlpSoftmaxBlock(**kw)
    ok = NlpSoftmaxBlock([[1, 2], [3, 4]], A, [0, 1, 2], 3)
    terms = [(0, 1.0, [(1, POW, 2)])]
    with pytest.raises(ValueError):
        make_nlp_terms(3, 0, 0, terms, blocks=[ok])                                # column 4 of 3 variables
    with pytest.raises(ValueError):
        make_nlp_terms(4, 0, 0, terms, blocks=[ok] * 5)                            # a fifth block
    assert make_nlp_terms(4, 0, 0, terms, blocks=[ok]).blocks == [ok]


def test_edge_cases_cover_the_shape_edges():
    D = {(K - p) * d for _, d, K, p in EDGE_CASES}
    assert {1, 117, 128} <= D and any(N > 1024 for N, _, _, _ in EDGE_CASES) and {N % 4 for N, _, _, _ in EDGE_CASES} == {0, 1, 2, 3}
    assert (4, 16, 2, 0) in EDGE_CASES and (5, 17, 2, 0) in EDGE_CASES             # class = tile; a boundary mid-tile
    p, lay, inst = edge_model(*BIG_LOGITS, big=True)
    assert all((np.abs(s) == 800.0).sum() >= 4 and (s == 800.0).any() and (s == -800.0).any() for _, s in inst)
    assert any((w == 0).any() for w, _ in inst) and all((w < 0).any() for w, _ in inst)


# ---- (f) the oracle and Newton on the cases the GPU tests solve
def _solve(p, lay=None):
    ro = O.sqp_solve(OracleSoftmaxTerms(p, lay), O.default_options(**SQP_TIGHT))
    assert ro["status"] == 0, ro["status"]
    return ro


@pytest.mark.parametrize("pinned", [True, False])
def test_oracle_solves_the_folds_to_the_newton_reference(pinned):
    X, y, reg, W = folds_case3()
    sol = [newton_multinomial(X, y, 3, reg, w, pinned) for w in W]
    print("Newton steps", [it for _, it, _ in sol], "max |b|", max(np.abs(b).max() for b, _, _ in sol), "min eig", min(e for _, _, e in sol))
    # (unpinned, a common shift of the classes leaves the block unchanged: the smallest eigenvalue is reg = 0.5 itself, up to the
    # rounding of eigvalsh)
    assert all(it <= 9 for _, it, _ in sol) and max(np.abs(b).max() for b, _, _ in sol) < 3 and min(e for _, _, e in sol) >= 0.5 - 1e-12
    assert min(np.abs(sol[a][0] - sol[b][0]).max() for a in range(4) for b in range(a)) > 1e-3
    for f in range(4):
        assert np.abs(_solve(multinomial_block_model(X, y, 3, reg, pinned, W[f]))["x"] - sol[f][0]).max() <= 1e-6, f


def test_oracle_on_two_classes_the_rows_case_and_the_queue_case():
    X, y, reg, W = folds_case3(2)
    b = newton_multinomial(X, y, 2, reg, W[0], True)[0]
    assert np.abs(_solve(multinomial_block_model(X, y, 2, reg, True, W[0]))["x"] - b).max() <= 1e-6
    assert np.abs(_solve(logistic_block_model(X, (y == 0).astype(float), reg, W[0]))["x"] - b).max() <= 1e-6
    p, lay, shifts = rows_case()
    for s in shifts:
        ro = _solve(with_block(p, 0, shift=s), lay)
        assert (np.abs(ro["x"] - p.xL) < 1e-7).any() or (np.abs(ro["x"] - p.xU) < 1e-7).any()
        assert abs(ro["x"].sum() - 0.6) <= 1e-8
    p, lay, scen = queue_case()
    xs = [_solve(with_block(p, 0, weight=w, shift=s), lay)["x"] for w, s in scen]
    assert min(np.abs(xs[a] - xs[b]).max() for a in range(5) for b in range(a)) > 1e-3


# ---- (g) header and binding
def test_header_carries_the_prototype_and_the_loader_binds_it():
    hdr = open(os.path.join(ROOT, "include", "sqphip.h")).read()
    code = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    m = re.search(r"int\s+sqphip_nlp_add_softmax_block\s*\(([^;]*)\)\s*;", code)
    assert m, "prototype"
    kinds = [re.sub(r"\s*(\*?)\s*\w+$", r"\1", re.sub(r"\s+", " ", a.strip())) for a in m.group(1).split(",")]      # the type of an argument
    assert kinds == ["sqphip_ctx*", "int64_t", "int32_t", "int32_t", "int32_t", "const int64_t*", "const double*", "const int32_t*",
                     "const double*", "const double*", "int32_t*"], kinds
    assert "sqphip_nlp_add_softmax_block" in _lib.EXPORTS
    src = open(os.path.join(ROOT, "sqpsolver.jl_amd", "_lib.py")).read()
    assert "L.sqphip_nlp_add_softmax_block.argtypes = [vp, C.c_int64, C.c_int32, C.c_int32, C.c_int32, lp, dp, ip, dp, dp, ip]" in src
    assert "nlp_softmax_dev.hpp" in _lib.HEADERS
