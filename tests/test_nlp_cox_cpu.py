"""Cox partial-likelihood data blocks of a factorable NLP, the parts that need no GPU: numpy's block_eval against the 50-digit
reference and its bound (tests/nlp_cox_ref.py) on every case of the GPU tests, the bound against a planted perturbation, finite
differences, the risk sets of cox_block_model, a zero-weight fold against the block built on the subset, the cases' own edges,
the oracle on a ridge-penalised fit, the refusals of the Python layer, header and binding."""
import dataclasses
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from sqpsolver_jl_amd import _lib                                       # noqa: E402
from sqpsolver_jl_amd.nlp_terms import (POW, NlpCoxBlock, block_eval, cox_block_model, cox_risk, fold_weights,   # noqa: E402
                                        make_nlp_terms, nlp_terms_layout)
from oracle import oracle as O                                        # noqa: E402
from nlp_cox_ref import (EDGE_CASES, GROUPS, IDS, NO_EVENT, SQP_TIGHT, NlpCoxNumpy, NlpCoxRef, OracleCoxTerms, check_outputs,   # noqa: E402
                         cox_reference, edge_model, edge_reference, folds_case, mixed_model, queue_case, risk_pattern,
                         rows_case, survival_data, with_block)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = ("f", "grad", "hval")


def _accepts(got, val, bnd):
    """the acceptance rule per output: {key: bool}"""
    ok = {}
    for key in OUT:
        g_, w_, b_ = (np.atleast_1d(np.asarray(a, float)) for a in (got[key], val[key], bnd[key]))
        ok[key] = bool(np.all(np.abs(g_ - w_) <= 4.0 * b_ + 1e-13 * np.abs(w_).max()))
    return ok


# ---- (a) numpy meets the bound on every case; the covariance part of the reference is there in every tile
@pytest.mark.parametrize("case", EDGE_CASES, ids=IDS)
def test_numpy_meets_the_bound_and_every_tile_has_a_covariance_part(case):
    for b in range(3):
        q, lay, x, sigma, lam, val, bnd, (H1, H2) = edge_reference(case, b)
        got = NlpCoxNumpy(q).outputs(x, sigma, lam, lay)
        assert all(np.all(np.isfinite(got[k])) for k in got)
        check_outputs(got, val, bnd, f"numpy {case} instance {b}")
        d = case[1]
        for R in range((d + 15) // 16):
            for C in range(R + 1):
                t1, t2 = (np.abs(H[16 * R:16 * R + 16, 16 * C:16 * C + 16]).max() for H in (H1, H2))
                assert t2 > 1e-6 * t1 > 0.0 or case[0] == 1, (case, b, R, C, t1, t2)
        if case[0] == 1:
            assert np.array_equal(H1, H2)                             # one point: no variance at all
    for key in OUT:
        ratio = float(np.max(bnd[key]) / np.abs(val[key]).max())
        print("B / max|want|", key, ratio)
        assert ratio <= 1e-10, (key, ratio)


def test_no_event_is_exactly_zero():
    p, lay, inst = edge_model(*NO_EVENT)
    x = np.linspace(0.6, 1.4, p.n)
    f, g, H = block_eval(p, x)
    assert f == 0.0 and not g.any() and not H.any()
    (f, g, H), (Bf, Bg, BH), _ = cox_reference(p.blocks[0], x, 0.7)
    assert f == 0.0 and not g.any() and not H.any() and Bf == 0.0 and not Bg.any() and not BH.any()


# ---- (b) the bound is not vacuous: one entry of A moved by 1e-9 relative fails it
@pytest.mark.parametrize("case", [(5, 17, "groups", "mixed", 0), (65, 5, "groups", "mixed", 0), (1025, 3, "groups", "mixed", 0)])
def test_a_perturbed_entry_of_A_breaks_the_acceptance_rule(case):
    q, lay, x, sigma, lam, val, bnd, _ = edge_reference(case, 0)
    b = q.blocks[0]
    i = int(np.argmax(b.weight * b.event * np.abs(b.A[:, 0])))
    A = b.A.copy(); A[i, 0] *= 1.0 + 1e-9
    ok = _accepts(NlpCoxNumpy(with_block(q, 0, A=A)).outputs(x, sigma, lam, lay), val, bnd)
    assert not all(ok.values()), (case, ok)


# ---- (c) finite differences
@pytest.mark.parametrize("risk_kind", ["untied", "tied", "groups"])
def test_gradient_and_hessian_agree_with_central_differences(risk_kind):
    p, lay, _ = edge_model(23, 4, risk_kind, "mixed", 0)
    b = p.blocks[0]
    x = np.linspace(0.6, 1.4, p.n)
    (f, g, H), _, _ = cox_reference(b, x, 1.0)
    c = b.cols - 1
    h = 1e-6
    for j in range(len(c)):
        dx = np.zeros(p.n); dx[c[j]] = h
        fp, gp, _ = block_eval(p, x + dx)
        fm, gm, _ = block_eval(p, x - dx)
        assert abs((fp - fm) / (2 * h) - g[j]) <= 1e-7 * max(1.0, abs(g[j]))
        assert np.all(np.abs((gp - gm)[c] / (2 * h) - H[:, j]) <= 1e-6 * max(1.0, np.abs(H).max()))


def test_the_value_is_the_partial_likelihood_written_out():
    p, lay, inst = edge_model(65, 5, "groups", "mixed", 0)
    b = p.blocks[0]
    x = np.linspace(0.6, 1.4, p.n)
    u = b.A @ x[b.cols - 1] + b.shift
    want = sum(b.weight[i] * b.event[i] * (np.log(np.sum(b.weight[:b.risk[i]] * np.exp(u[:b.risk[i]]))) - u[i])
               for i in range(65) if b.weight[i] * b.event[i] != 0)
    assert abs(block_eval(p, x)[0] - want) <= 1e-12 * abs(want)


# ---- (d) the builder: risk sets for tied, untied and all-tied times; folds
def test_cox_block_model_builds_the_risk_sets():
    assert cox_risk([5, 4, 4, 3, 3, 3, 1]).tolist() == [1, 3, 3, 6, 6, 6, 7]
    assert cox_risk([3, 2, 1]).tolist() == [1, 2, 3] and cox_risk([2, 2, 2]).tolist() == [3, 3, 3] and cox_risk([7]).tolist() == [1]
    with pytest.raises(ValueError):
        cox_risk([1, 2])
    rng = np.random.default_rng(3)
    A = rng.standard_normal((7, 2))
    for t, want in (([3, 1, 4, 1, 5, 9, 2], [1, 2, 3, 4, 5, 7, 7]), ([2, 2, 2, 2, 2, 2, 2], [7] * 7), ([1, 2, 1, 2, 3, 3, 1], [2, 2, 4, 4, 7, 7, 7])):
        ev = np.array([1, 0, 1, 1, 0, 1, 1.0]); w = np.arange(1.0, 8.0); s = 0.1 * np.arange(7.0)
        p = cox_block_model(A, t, ev, 0.3, weight=w, shift=s)
        b, o = p.blocks[0], p.cox_order
        assert b.risk.tolist() == want and np.all(np.diff(np.asarray(t, float)[o]) <= 0)
        assert np.array_equal(b.A, A[o]) and np.array_equal(b.event, ev[o]) and np.array_equal(b.weight, w[o]) and np.array_equal(b.shift, s[o])
        assert all(b.risk[i] == np.sum(np.asarray(t)[o] >= np.asarray(t)[o][i]) for i in range(7))
        assert p.n == 2 and len(p.trow) == 2 and np.all(p.xL == -50.0) and np.all(p.xU == 50.0) and not p.x0.any()
        x = np.array([0.3, -0.2])
        u = A @ x + s
        want_f = sum(w[i] * ev[i] * (np.log(np.sum((w * np.exp(u))[np.asarray(t) >= t[i]])) - u[i]) for i in range(7)) + 0.15 * (x @ x)
        assert abs(NlpCoxNumpy(p).f(x) - want_f) <= 1e-12 * abs(want_f)
    p, W = folds_case()
    assert W.shape == (4, 48) and len(nlp_terms_layout(p).hrow) == 6 and len(set(p.blocks[0].risk.tolist())) < 48      # ties in the data


def test_a_zero_weight_fold_equals_the_block_built_on_the_subset():
    A, t, ev = survival_data()
    p, W = folds_case()
    b = p.blocks[0]
    x, lam = np.array([0.4, -0.3, 0.2]), np.zeros(0)
    lay = nlp_terms_layout(p)
    for w in W:
        keep = w > 0
        sub = cox_block_model(b.A[keep], np.asarray(t)[p.cox_order][keep], b.event[keep], 0.5)
        assert np.array_equal(sub.blocks[0].A, b.A[keep])             # (sorted already: the stable sort keeps the order)
        vf, bf = NlpCoxRef(with_block(p, 0, weight=w)).want(x, 0.9, lam, lay)
        vs, bs = NlpCoxRef(sub).want(x, 0.9, lam, lay)
        gf, gs = NlpCoxNumpy(with_block(p, 0, weight=w)).outputs(x, 0.9, lam, lay), NlpCoxNumpy(sub).outputs(x, 0.9, lam, lay)
        for k in OUT:
            lim = 4.0 * (np.asarray(bf[k]) + np.asarray(bs[k])) + 2e-13 * np.abs(vs[k]).max()
            assert np.all(np.abs(np.asarray(vf[k]) - np.asarray(vs[k])) <= lim), k       # the two references
            assert np.all(np.abs(np.asarray(gf[k]) - np.asarray(gs[k])) <= lim), k       # the two numpy evaluations
        assert abs(vf["f"] - NlpCoxRef(p).want(x, 0.9, lam, lay)[0]["f"]) > 1e-3          # the weights count


# ---- (e) the cases cover what they claim
def test_edge_cases_cover_the_shape_edges():
    assert {c[0] for c in EDGE_CASES} >= {1, 3, 4, 5, 63, 64, 65, 1023, 1024, 1025, 2049}
    assert {c[1] for c in EDGE_CASES} >= {1, 15, 16, 17, 33, 128} and all(c[0] <= 64 for c in EDGE_CASES if c[1] > 17)
    assert {c[2] for c in EDGE_CASES} == {"untied", "tied", "groups"} and {c[3] for c in EDGE_CASES} == {"mixed", "first"}
    r = risk_pattern(2049, "groups")
    assert np.all(r >= np.arange(1, 2050)) and np.all(np.diff(r) >= 0) and r[-1] == 2049
    inside = lambda k: r[k - 1] == r[k]                               # points k - 1 and k sit in one tie group
    assert inside(8) and inside(64) and inside(1024) and sum(GROUPS) == 18
    assert risk_pattern(5, "untied").tolist() == [1, 2, 3, 4, 5] and risk_pattern(4, "tied").tolist() == [4] * 4
    for case in EDGE_CASES:
        p, lay, inst = edge_model(*case)
        b = p.blocks[0]
        assert all(np.all(w >= 0) and w[0] * b.event[0] > 0 for w, _ in inst)
        if case[3] == "first":
            assert b.event[0] == 1.0 and not b.event[1:].any()
        if case[4]:
            u = [b.A @ edge_reference(case, k)[2][b.cols - 1] + s for k, (_, s) in enumerate(inst)]
            assert all(v.max() > 250 and v.min() < -250 for v in u)
        if case[0] >= 63 and case[2] == "groups":
            w = inst[0][0]
            lead = [i for i in range(1, case[0] - 1) if b.risk[i] != b.risk[i - 1] and b.risk[i] == b.risk[i + 1] and w[i] == 0]
            assert lead and (w == 0).sum() > 5                       # zero weights scattered in, one of them leading a tie group
    p, lay, inst = edge_model(*NO_EVENT)
    assert not p.blocks[0].event.any()


# ---- (f) the oracle reaches stationarity on a ridge-penalised fit, and solves the cases of the GPU tests
def _solve(p, lay=None):
    ro = O.sqp_solve(OracleCoxTerms(p, lay), O.default_options(**SQP_TIGHT))
    assert ro["status"] == 0, ro["status"]
    return ro


def test_oracle_reaches_stationarity_on_the_folds_the_rows_case_and_the_queue_case():
    p, W = folds_case()
    xs = []
    for w in W:
        q = with_block(p, 0, weight=w)
        x = _solve(q)["x"]
        R = NlpCoxNumpy(q)
        assert np.abs(R.grad(x)).max() <= 1e-7 and np.abs(x).max() < 5          # interior: the gradient itself vanishes
        assert np.linalg.eigvalsh(block_eval(q, x)[2] + 0.5 * np.eye(3)).min() >= 0.5 - 1e-9
        xs.append(x)
    assert min(np.abs(xs[a] - xs[b]).max() for a in range(4) for b in range(a)) > 1e-3
    p, lay, shifts = rows_case()
    for s in shifts:
        ro = _solve(with_block(p, 0, shift=s), lay)
        assert abs(ro["x"].sum() - 0.3) <= 1e-8
    p, lay, scen = queue_case()
    xs = [_solve(with_block(p, 0, weight=w, shift=s), lay)["x"] for w, s in scen]
    assert min(np.abs(xs[a] - xs[b]).max() for a in range(5) for b in range(a)) > 1e-3


# ---- (g) layout and the refusals of the Python layer
def test_layout_and_refusals_of_the_python_layer():
    p, lay, _ = edge_model(5, 17, "groups", "mixed", 0)
    pairs = set(zip(lay.hrow.tolist(), lay.hcol.tolist()))
    cols = p.blocks[0].cols.tolist()
    assert cols != sorted(cols) and max(cols) - min(cols) + 1 > len(cols)          # unsorted, not contiguous
    assert all((max(a, b), min(a, b)) in pairs for a in cols for b in cols) and len(lay.hrow) == len(pairs) + 2
    for order in (False, True):
        q, layq = mixed_model(order)
        pairs = set(zip(layq.hrow.tolist(), layq.hcol.tolist()))
        for b in q.blocks:
            c = np.ravel(b.cols).tolist()
            assert all((max(a, e), min(a, e)) in pairs for a in c for e in c)
    A = np.ones((3, 2))
    ok = dict(cols=[1, 2], A=A, risk=[1, 3, 3], event=[1, 0, 1])
    for bad, words in ((dict(risk=[1, 1, 3]), "point 2: risk 1 outside 2..3"), (dict(risk=[1, 3, 4]), "point 3: risk 4 outside 3..3"),
                       (dict(risk=[3, 2, 3]), "point 2: risk 2 decreases from 3"), (dict(risk=[1, 3]), "3 values each"),
                       (dict(event=[1, -1, 0]), "point 2: event -1.0"), (dict(event=[1, 0, np.nan]), "point 3: event nan"),
                       (dict(cols=[1, 1]), "2 distinct variables"), (dict(cols=[1, 2, 3]), "2 distinct variables"),
                       (dict(A=np.ones((3, 129)), cols=np.arange(1, 130)), "d = 129 columns (1..128)"),
                       (dict(weight=[1, 1]), "3 values each"), (dict(shift=[0.0] * 4), "3 values each")):
        with pytest.raises(ValueError, match=re.escape(words)):
            NlpCoxBlock(**{**ok, **bad})
    blk = NlpCoxBlock(**ok)
    assert blk.risk.dtype == np.int32 and np.array_equal(blk.weight, np.ones(3)) and not blk.shift.any()
    terms = [(0, 1.0, [(1, POW, 2)])]
    with pytest.raises(ValueError, match="block 1: a column outside 1..1"):
        make_nlp_terms(1, 0, 0, terms, blocks=[blk])
    with pytest.raises(ValueError):
        make_nlp_terms(2, 0, 0, terms, blocks=[blk] * 5)
    with pytest.raises(ValueError, match="3 values each"):
        cox_block_model(A, [1, 2], [1, 0, 1], 0.1)
    assert make_nlp_terms(2, 0, 0, terms, blocks=[blk]).blocks == [blk]


# ---- (h) header and binding
def test_header_carries_the_prototype_and_the_loader_binds_it():
    hdr = open(os.path.join(ROOT, "include", "sqphip.h")).read()
    code = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    m = re.search(r"int\s+sqphip_nlp_add_cox_block\s*\(([^;]*)\)\s*;", code)
    assert m, "prototype"
    kinds = [re.sub(r"\s*(\*?)\s*\w+$", r"\1", re.sub(r"\s+", " ", a.strip())) for a in m.group(1).split(",")]      # the type of an argument
    assert kinds == ["sqphip_ctx*", "int64_t", "int32_t", "const int64_t*", "const double*", "const int32_t*", "const double*",
                     "const double*", "const double*", "int32_t*"], kinds
    assert "sqphip_nlp_add_cox_block" in _lib.EXPORTS
    src = open(os.path.join(ROOT, "sqpsolver.jl_amd", "_lib.py")).read()
    assert "L.sqphip_nlp_add_cox_block.argtypes = [vp, C.c_int64, C.c_int32, lp, dp, ip, dp, dp, dp, ip]" in src
    assert "nlp_cox_dev.hpp" in _lib.HEADERS
