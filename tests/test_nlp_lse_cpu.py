"""Log-sum-exp row blocks of a factorable NLP, the parts that need no GPU: numpy's lse_block_eval against the 50-digit reference
and its bound (tests/nlp_lse_ref.py) on every case of the GPU tests, the bound against a planted perturbation, finite
differences, the reference against the softmax block's on one model written both ways, the cases' own edges, scipy's and the
oracle's word on the solved cases, layout and the refusals of the Python layer, header and binding."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from sqpsolver_jl_amd import _lib                                       # noqa: E402
from sqpsolver_jl_amd.nlp_terms import (POW, NlpLseBlock, NlpSoftmaxBlock, geometric_program_model, gp_scenario, gp_synth,   # noqa: E402
                                        lse_block_eval, make_nlp_terms, nlp_terms_layout)
from oracle import oracle as O                                        # noqa: E402
from nlp_lse_ref import (EDGE_CASES, EDGE_LAM, GP_LENS, GP_N, GP_SEEDS, IDS, M_EDGE, SQP_TIGHT, NlpLseNumpy, NlpLseRef, OracleLseTerms,   # noqa: E402
                         box_gp, check_outputs, edge_lse_model, edge_reference, gp_cases, gp_queue_case, gp_scipy, lse_reference,
                         overlap_model, softmax_reference, stable_case, with_block)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = ("f", "grad", "g", "jval", "hval")


def _accepts(got, val, bnd):
    """the acceptance rule per output: {key: bool}"""
    ok = {}
    for key in OUT:
        g_, w_, b_ = (np.atleast_1d(np.asarray(a, float)) for a in (got[key], val[key], bnd[key]))
        ok[key] = bool(np.all(np.abs(g_ - w_) <= 4.0 * b_ + 1e-13 * np.abs(w_).max()))
    return ok


# ---- (a) numpy meets the bound on every case
@pytest.mark.parametrize("case", EDGE_CASES, ids=IDS)
def test_numpy_meets_the_bound_on_every_edge_case(case):
    worst = {}
    for b in range(3):
        q, lay, x, sigma, lam, val, bnd = edge_reference(case, b)
        got = NlpLseNumpy(q).outputs(x, sigma, lam, lay)
        assert all(np.all(np.isfinite(got[k])) for k in got)
        for k, v in check_outputs(got, val, bnd, f"numpy {case} instance {b}").items():
            worst[k] = max(worst.get(k, 0.0), v)
    print("largest err / B", worst)
    q, lay, x, sigma, lam, val, bnd = edge_reference(case, 0)       # (instance 2 has sigma = 0: its Hessian can vanish)
    for key in OUT:
        ratio = float(np.max(bnd[key]) / np.abs(val[key]).max())
        print("B / max|want|", key, ratio)
        assert ratio <= 1e-10, (key, ratio)


def test_numpy_meets_the_bound_on_the_stability_case_and_a_removed_monomial_leaves_no_trace():
    p, lay, inst, gone, p0 = stable_case()
    x = np.linspace(0.6, 1.4, p.n)
    for b, (w, s) in enumerate(inst):
        q = with_block(p, 0, weight=w, shift=s)
        u = q.blocks[0].A @ x[q.blocks[0].cols - 1] + s
        got = NlpLseNumpy(q).outputs(x, 0.7, EDGE_LAM, lay)
        assert all(np.all(np.isfinite(got[k])) for k in got)
        val, bnd = NlpLseRef(q).want(x, 0.7, EDGE_LAM, lay)
        check_outputs(got, val, bnd, f"stability, instance {b}")
        if b == 0:
            assert all(u[a:e].max() - u[a:e].min() > 590 for a, e in ((0, 5), (5, 70)))       # 300 either side
        else:
            for i, (a, e) in zip(gone, ((0, 5), (5, 70))):
                assert int(np.argmax(u[a:e])) + a == i and u[i] - np.delete(u[a:e], i - a).max() > 790 and w[i] == 0.0
            zero = NlpLseNumpy(with_block(p0, 0, weight=w, shift=s)).outputs(x, 0.7, EDGE_LAM, lay)
            for k in OUT:
                assert np.array_equal(np.asarray(got[k]), np.asarray(zero[k])), k


# ---- (b) the bound is not vacuous: one entry of A moved by 1e-9 relative fails it
@pytest.mark.parametrize("case", [EDGE_CASES[1], EDGE_CASES[3]], ids=[IDS[1], IDS[3]])
def test_a_perturbed_entry_of_A_breaks_the_acceptance_rule(case):
    import dataclasses
    q, lay, x, sigma, lam, val, bnd = edge_reference(case, 0)
    b = q.blocks[0]
    i = int(np.argmax(b.weight * np.abs(b.A[:, 0])))
    A = b.A.copy(); A[i, 0] *= 1.0 + 1e-9
    moved = dataclasses.replace(q, blocks=[dataclasses.replace(b, A=A)])
    ok = _accepts(NlpLseNumpy(moved).outputs(x, sigma, lam, lay), val, bnd)
    assert not all(ok.values()), (case, ok)


# ---- (c) finite differences of the reference
def test_jacobian_and_hessian_agree_with_central_differences():
    p, lay, inst = edge_lse_model(23, 4, (1, 9, 13), (0, 3, 6))
    b = p.blocks[0]
    x = np.linspace(0.6, 1.4, p.n)
    lam = EDGE_LAM
    (F, G, H), _, (H1, H2) = lse_reference(b, x, 0.7, lam)
    assert np.allclose(H, H1 - H2, rtol=0, atol=1e-15 * np.abs(H1).max())
    c = b.cols - 1
    h = 1e-6
    mu = np.array([0.7, lam[2], lam[5]])
    for j in range(len(c)):
        dx = np.zeros(p.n); dx[c[j]] = h
        Fp, Gp = lse_reference(b, x + dx, 0.7, lam)[0][:2]
        Fm, Gm = lse_reference(b, x - dx, 0.7, lam)[0][:2]
        assert np.all(np.abs((Fp - Fm) / (2 * h) - G[:, j]) <= 1e-7)
        assert np.all(np.abs(mu @ (Gp - Gm) / (2 * h) - H[:, j]) <= 1e-6 * max(1.0, np.abs(H).max()))
    # the value written out
    u = b.A @ x[c] + b.shift
    for r in range(3):
        s = slice(int(b.seg[r]), int(b.seg[r + 1]))
        assert abs(F[r] - np.log(np.sum(b.weight[s] * np.exp(u[s])))) <= 1e-13


# ---- (d) the same model as a softmax block: one point, K classes, unpinned, label 0
def test_the_reference_equals_the_softmax_reference_on_one_model_written_both_ways():
    K, d = 5, 3
    rng = np.random.default_rng(71)
    a0 = rng.standard_normal(d)
    cols = rng.permutation(K * d + 3)[:K * d].reshape(K, d) + 1
    shift = 0.4 * rng.standard_normal((K, 1))
    soft = NlpSoftmaxBlock(cols, a0[None, :], [0], K, pinned=False, shift=shift)
    A = np.zeros((K, K * d))
    for k in range(K):
        A[k, k * d:(k + 1) * d] = a0
    lse = NlpLseBlock(cols.ravel(), A, [0], [0, K], shift.ravel())
    x = rng.uniform(-1.0, 1.0, K * d + 3)
    (fs, gs, Hs), (Bfs, Bgs, BHs) = softmax_reference(soft, x, 1.3)
    (F, G, H), (BF, BG, BH), _ = lse_reference(lse, x, 1.3, np.zeros(0))
    u0 = float(a0 @ x[cols[0] - 1] + shift[0, 0])
    lin = np.zeros(K * d); lin[:d] = a0                               # the linear term -u_0 of the softmax loss
    tiny = 8 * 2.0 ** -53
    assert abs(fs - (F[0] - u0)) <= 4 * (Bfs + BF[0]) + tiny * (1 + abs(u0))
    assert np.all(np.abs(gs - (G[0] - lin)) <= 4 * (Bgs + BG[0]) + tiny * np.abs(lin))
    assert np.all(np.abs(Hs - H) <= 4 * (BHs + BH) + 1e-13 * np.abs(H).max())
    assert np.abs(H).max() > 1e-2 and abs(F[0]) > 1e-2


# ---- (e) the cases cover what they claim
def test_edge_cases_cover_the_shape_edges():
    assert [(c[0], c[1]) for c in EDGE_CASES] == [(1, 1), (5, 17), (193, 15), (133, 16), (68, 33), (1030, 20), (130, 128)]
    lens = [c[2] for c in EDGE_CASES]
    assert lens[2] == (1, 63, 64, 65) and lens[3] == (1,) * 5 + (128,) and lens[4] == (4,) * 17 and lens[5] == (1027, 3) and lens[6] == (129, 1)
    assert 0 not in EDGE_CASES[2][3] and 0 in EDGE_CASES[3][3] and len(EDGE_CASES[3][3]) % 4 != 0 and len(EDGE_CASES[4][3]) == 17
    assert (EDGE_LAM == 0).sum() == 1 and (EDGE_LAM < 0).sum() == 2 and len(EDGE_LAM) == M_EDGE
    for case in EDGE_CASES:
        p, lay, inst = edge_lse_model(*case)
        b = p.blocks[0]
        assert sum(case[2]) == case[0] and len(set(case[3])) == len(case[3]) and all(i == 0 or 2 <= i <= M_EDGE for i in case[3])
        cols = b.cols.tolist()
        assert case[1] == 1 or (cols != sorted(cols) and max(cols) - min(cols) + 1 > len(cols))
        for w, s in inst:
            assert np.all(w >= 0) and all(w[a:e].any() for a, e in zip(b.seg[:-1], b.seg[1:]))
        assert case[0] < 5 or sum((w == 0).sum() for w, _ in inst) >= 3
        assert len({tuple(w) for w, _ in inst}) == 3 and len({tuple(s) for _, s in inst}) == 3
        assert len(lay.hrow) == len(set(zip(lay.hrow.tolist(), lay.hcol.tolist()))) + 2
        assert len(lay.jrow) == len(set(zip(lay.jrow.tolist(), lay.jcol.tolist()))) + 2


# ---- (f) scipy's and the oracle's word on the solved cases of the GPU tests
def _solve(p, **kw):
    try:
        ro = O.sqp_solve(OracleLseTerms(p), O.default_options(**{**SQP_TIGHT, **kw}))
    finally:
        O.set_kkt_order(None)
    assert ro["status"] == 0, ro["status"]
    return ro


@pytest.mark.parametrize("kkt_mode", [1, 2])
def test_oracle_solves_the_box_gp_and_scipy_agrees(kkt_mode):
    p = box_gp()
    ro = _solve(p, **(dict(kkt_mode=2) if kkt_mode == 2 else dict(kkt_mode=1, kkt_tile_order=1)))
    want = gp_scipy(p)
    print("iter", ro["iter"], "x", ro["x"], "scipy", np.abs(ro["x"] - want).max(), "g", ro["g"], "mult", ro["mult_g"])
    assert np.abs(ro["x"] - want).max() <= 1e-6
    assert np.all(np.abs(ro["g"]) <= 1e-8) and np.all(np.abs(ro["mult_g"]) > 1e-3)          # both rows active
    h, w, d = np.exp(ro["x"])
    assert abs(0.02 * h * w + 0.02 * h * d - 1.0) <= 1e-7 and abs(0.1 * w * d - 1.0) <= 1e-7


@pytest.mark.parametrize("seed", GP_SEEDS)
def test_oracle_solves_the_synthetic_gps_and_scipy_agrees(seed):
    for k, p in enumerate(gp_cases(seed)):
        ro = _solve(p, kkt_mode=2)
        r1 = _solve(p, kkt_mode=1, kkt_tile_order=1)
        assert r1["iter"] == ro["iter"] and np.abs(r1["x"] - ro["x"]).max() <= 1e-8          # both linear solvers
        want = gp_scipy(p)
        active = int((np.abs(ro["g"]) <= 1e-8).sum())
        print("seed", seed, "scenario", k, "iter", ro["iter"], "scipy", np.abs(ro["x"] - want).max(), "active rows", active,
              "at a bound", int((np.abs(np.abs(ro["x"]) - 3.0) < 1e-6).sum()))
        assert np.abs(ro["x"] - want).max() <= 1e-6
        assert active >= 1


def test_oracle_solves_the_queue_scenarios_and_they_differ():
    p, scen = gp_queue_case()
    assert scen[0] is p
    xs = [_solve(q, kkt_mode=2)["x"] for q in scen]
    assert min(np.abs(xs[a] - xs[b]).max() for a in range(6) for b in range(a)) > 1e-3


def test_the_generator_is_what_it_says():
    p = gp_synth(GP_N, GP_LENS, 1)
    b = p.blocks[0]
    assert b.A.shape[0] == sum(GP_LENS) and b.seg.tolist() == np.concatenate([[0], np.cumsum(GP_LENS)]).tolist() and b.rows.tolist() == [0, 1, 2, 3, 4, 5]
    assert np.array_equal(2 * b.A, np.round(2 * b.A)) and np.abs(b.A).max() <= 2.0 and np.all(np.any(b.A != 0, axis=1))
    assert 0.3 < (b.A != 0).mean() < 0.5
    f, _, g, _, _ = lse_block_eval(p, np.zeros(p.n))
    assert abs(f) <= 1e-14 and np.all(np.abs(g - np.log(0.5)) <= 1e-14)
    assert np.all(p.xL == -3.0) and np.all(p.xU == 3.0) and not p.x0.any() and np.all(p.gU == 0.0) and np.all(np.isinf(p.gL))
    assert len(p.trow) == GP_N and np.all(p.tcoef == 1e-3) and np.all(p.fexp == 2)          # the ridge stays in the terms
    q = gp_scenario(p, 2, 1, 0.1)
    assert np.array_equal(q.blocks[0].A, b.A) and 0.01 < np.abs(q.blocks[0].shift - b.shift).max() < 1.0
    assert gp_scenario(p, 0, 1, 0.1) is p and gp_scenario(p, 3, 1, 0.0) is p
    assert np.array_equal(gp_scenario(p, 2, 1, 0.1).blocks[0].shift, q.blocks[0].shift)
    # monomial equalities become linear rows
    m = geometric_program_model(3, [([1.0, 2.0], [[1, 0, 0], [0, 1, 0]]), ([0.5], [[0, 0, 1]])], monomial_rows=[(2.0, [1, -1, 0])])
    assert (m.m, m.num_linear) == (2, 1) and m.blocks[0].rows.tolist() == [0, 2] and m.gL[0] == m.gU[0] == 0.0
    assert abs(NlpLseNumpy(m).g(np.array([0.3, 0.1, 0.2]))[0] - (np.log(2.0) + 0.3 - 0.1)) <= 1e-15


# ---- (g) layout and the refusals of the Python layer
def test_layout_and_refusals_of_the_python_layer():
    p, lay, _ = edge_lse_model(5, 17, (2, 3), (0, 3))
    pairs = set(zip(lay.hrow.tolist(), lay.hcol.tolist()))
    jp = set(zip(lay.jrow.tolist(), lay.jcol.tolist()))
    cols = p.blocks[0].cols.tolist()
    assert all((max(a, b), min(a, b)) in pairs for a in cols for b in cols)
    assert all((3, c) in jp for c in cols) and not any(r == 0 for r, _ in jp)
    for order in (False, True):
        q, layq = overlap_model(order)
        pairs, jp = set(zip(layq.hrow.tolist(), layq.hcol.tolist())), set(zip(layq.jrow.tolist(), layq.jcol.tolist()))
        for b in q.blocks:
            c = np.ravel(b.cols).tolist()
            assert all((max(a, e), min(a, e)) in pairs for a in c for e in c) and all((2, a) in jp for a in c)
    A = np.ones((3, 2))
    ok = dict(cols=[1, 2], A=A, rows=[0, 2], seg=[0, 1, 3])
    for bad, words in ((dict(seg=[1, 2, 3]), "output 1: seg[0] = 1"), (dict(seg=[0, 1, 2]), "output 2: seg[R] = 2"),
                       (dict(seg=[0, 0, 3]), "output 1: the segment 0..0 is empty"), (dict(seg=[0, 3, 2]), "output 2: the segment 3..2 is decreasing"),
                       (dict(seg=[0, 3]), "seg: R + 1 = 3 values"), (dict(rows=[2, 2]), "two outputs"),
                       (dict(rows=[0, 1, 2, 3], seg=[0, 1, 2, 3, 4]), "R = 4 outputs (1..3)"), (dict(rows=[], seg=[0]), "R = 0 outputs (1..3)"),
                       (dict(cols=[1, 1]), "2 distinct variables"), (dict(cols=[1, 2, 3]), "2 distinct variables"),
                       (dict(A=np.ones((3, 129)), cols=np.arange(1, 130)), "d = 129 columns (1..128)"),
                       (dict(weight=[1, 1]), "3 values each"), (dict(shift=[0.0] * 4), "3 values each")):
        with pytest.raises(ValueError, match=re.escape(words)):
            NlpLseBlock(**{**ok, **bad})
    blk = NlpLseBlock(**ok)
    assert blk.seg.dtype == np.int64 and np.array_equal(blk.weight, np.ones(3)) and not blk.shift.any()
    terms = [(0, 1.0, [(1, POW, 2)])]
    with pytest.raises(ValueError, match="block 1: a column outside 1..1"):
        make_nlp_terms(1, 2, 0, terms, blocks=[blk])
    with pytest.raises(ValueError, match="block 1: a row outside 0..1"):
        make_nlp_terms(2, 1, 0, terms, blocks=[blk])
    with pytest.raises(ValueError, match="block 1: a row among the num_linear = 2 linear rows"):
        make_nlp_terms(2, 2, 2, terms, blocks=[blk])
    with pytest.raises(ValueError):
        make_nlp_terms(2, 2, 0, terms, blocks=[blk] * 5)
    assert make_nlp_terms(2, 2, 0, terms, blocks=[blk]).blocks == [blk]
    # a zero-weight point contributes exactly 0, whatever its logit
    q = make_nlp_terms(2, 2, 0, terms, blocks=[NlpLseBlock([1, 2], A, [0, 2], [0, 1, 3], [0.0, 0.0, 5000.0], [1.0, 1.0, 0.0])])
    out = lse_block_eval(q, np.array([0.5, 0.25]), 1.0, np.array([0.0, 1.0]))
    assert all(np.all(np.isfinite(v)) for v in out) and out[2][1] == 0.75 and not out[4].any()


# ---- (h) header and binding
def test_header_carries_the_prototype_and_the_loader_binds_it():
    hdr = open(os.path.join(ROOT, "include", "sqphip.h")).read()
    code = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    m = re.search(r"int\s+sqphip_nlp_add_lse_block\s*\(([^;]*)\)\s*;", code)
    assert m, "prototype"
    kinds = [re.sub(r"\s*(\*?)\s*\w+$", r"\1", re.sub(r"\s+", " ", a.strip())) for a in m.group(1).split(",")]      # the type of an argument
    assert kinds == ["sqphip_ctx*", "int64_t", "int32_t", "const int64_t*", "const double*", "int32_t", "const int64_t*",
                     "const int64_t*", "const double*", "const double*", "int32_t*"], kinds
    assert "sqphip_nlp_add_lse_block" in _lib.EXPORTS
    src = open(os.path.join(ROOT, "sqpsolver.jl_amd", "_lib.py")).read()
    assert "L.sqphip_nlp_add_lse_block.argtypes = [vp, C.c_int64, C.c_int32, lp, dp, C.c_int32, lp, lp, dp, dp, ip]" in src
    assert "nlp_lse_dev.hpp" in _lib.HEADERS
