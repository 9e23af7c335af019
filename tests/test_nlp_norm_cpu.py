"""Euclidean-norm row blocks of a factorable NLP, the parts that need no GPU: numpy's norm_block_eval against the 50-digit
reference and its bound (tests/nlp_norm_ref.py) on every case of the GPU tests, the bound against a planted perturbation, finite
differences, one model written two ways, the cases' own edges, scipy's and the oracle's word on the solved cases, layout and the
refusals of the Python layer, header and binding.  (The plan builder of the add call: tests/test_norm_targets_cpu.py.)"""
import dataclasses
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from sqpsolver_jl_amd import _lib                                       # noqa: E402
from sqpsolver_jl_amd.nlp_terms import (POW, NlpNormBlock, make_nlp_terms, nlp_terms_layout, norm_block_eval, norm_scenario,   # noqa: E402
                                        robust_lp_model, socp_synth, sum_of_norms_model)
from oracle import oracle as O                                        # noqa: E402
from nlp_norm_ref import (APEX, EDGE_CASES, EDGE_LAM, IDS, M_EDGE, SOCP_LENS, SOCP_N, SOCP_SEEDS, SQP_TIGHT, STABLE_GRID, NlpNormNumpy,   # noqa: E402
                          NlpNormRef, OracleNormTerms, apex_case, apex_point, check_outputs, edge_norm_model, edge_reference,
                          fermat_weber, norm_reference, norm_scipy, overlap_model, robust_lp, socp_cases, socp_queue_case,
                          stable_case, with_block)

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
        got = NlpNormNumpy(q).outputs(x, sigma, lam, lay)
        assert all(np.all(np.isfinite(got[k])) for k in got)
        for k, v in check_outputs(got, val, bnd, f"numpy {case[:2]} instance {b}").items():
            worst[k] = max(worst.get(k, 0.0), v)
    print("largest err / B", worst)
    for b in range(3):
        q, lay, x, sigma, lam, val, bnd = edge_reference(case, b)
        for key in OUT:
            if sigma == 0.0 and key == "hval":
                continue                                                # (instance 2 has sigma = 0: its Hessian can vanish)
            ratio = float(np.max(bnd[key]) / np.abs(val[key]).max())
            print("B / max|want|", b, key, ratio)
            assert ratio <= 1e-10, (b, key, ratio)


def test_numpy_meets_the_bound_on_the_stability_case_and_a_removed_point_leaves_no_trace():
    p, lay, inst, gone, p0 = stable_case()
    x = np.linspace(0.6, 1.4, p.n)
    for b, (w, s) in enumerate(inst):
        q = with_block(p, 0, weight=w, shift=s)
        blk = q.blocks[0]
        with np.errstate(all="ignore"):
            v = blk.A @ x[blk.cols - 1] + s
        assert all(np.isinf(v[i]) and w[i] == 0.0 for i in gone)         # the residual of a zero-weight point overflows
        got = NlpNormNumpy(q).outputs(x, 0.7, EDGE_LAM, lay)
        assert all(np.all(np.isfinite(got[k])) for k in got)
        val, bnd = NlpNormRef(q, STABLE_GRID).want(x, 0.7, EDGE_LAM, lay)
        check_outputs(got, val, bnd, f"stability, instance {b}")
        if b == 0:
            for a, e in ((0, 5), (5, 70)):
                on = [i for i in range(a, e) if w[i] != 0.0]
                assert np.abs(v[on]).max() >= 0.99e200 and np.abs(v[on]).min() <= 1.01e-200       # 1e-200 .. 1e200 in one segment
        zero = NlpNormNumpy(with_block(p0, 0, weight=w, shift=s)).outputs(x, 0.7, EDGE_LAM, lay)
        for k in OUT:
            assert np.array_equal(np.asarray(got[k]), np.asarray(zero[k])), k


def test_an_output_at_the_apex_files_zero_and_contributes_nothing():
    p, lay, cut = apex_case()
    x = apex_point(p)
    b = p.blocks[0]
    v = b.A @ x[b.cols - 1] + b.shift
    assert np.all(v[36:39] == 0.0) and np.all(b.weight[36:39] > 0) and np.any(b.A[36] != 0) and b.weight[39] == 0.0 and v[39] != 0.0
    got, less = (NlpNormNumpy(q).outputs(x, 0.7, EDGE_LAM, lay) for q in (p, cut))
    for k in OUT:
        assert np.all(np.isfinite(got[k])) and np.array_equal(np.asarray(got[k]), np.asarray(less[k])), k
    (F, G, H), (BF, BG, BH), _, _ = norm_reference(b, x, 0.7, EDGE_LAM)
    assert np.all(F[3:] == 0.0) and not G[3:].any() and np.all(F[:3] > 0.1)
    val, bnd = NlpNormRef(p).want(x, 0.7, EDGE_LAM, lay)
    check_outputs(got, val, bnd, "apex")


# ---- (b) the bound is not vacuous: one entry of A moved by 1e-9 relative fails it
@pytest.mark.parametrize("case", [EDGE_CASES[1], EDGE_CASES[3]], ids=[IDS[1], IDS[3]])
def test_a_perturbed_entry_of_A_breaks_the_acceptance_rule(case):
    q, lay, x, sigma, lam, val, bnd = edge_reference(case, 0)
    b = q.blocks[0]
    i = int(np.argmax(b.weight * np.abs(b.A[:, 0])))
    A = b.A.copy(); A[i, 0] *= 1.0 + 1e-9
    moved = dataclasses.replace(q, blocks=[dataclasses.replace(b, A=A)])
    ok = _accepts(NlpNormNumpy(moved).outputs(x, sigma, lam, lay), val, bnd)
    assert not all(ok.values()), (case, ok)


# ---- (c) finite differences of the reference
def test_jacobian_and_hessian_agree_with_central_differences():
    p, lay, inst = edge_norm_model(23, 4, (1, 9, 13), (0, 3, 0))
    b = p.blocks[0]
    x = np.linspace(0.6, 1.4, p.n)
    lam = EDGE_LAM
    (F, G, H), _, (H1, H2), _ = norm_reference(b, x, 0.7, lam)
    assert np.allclose(H, H1 - H2, rtol=0, atol=1e-15 * np.abs(H1).max())
    c = b.cols - 1
    h = 1e-6
    mu = np.array([0.7, lam[2], 0.7])
    for j in range(len(c)):
        dx = np.zeros(p.n); dx[c[j]] = h
        Fp, Gp = norm_reference(b, x + dx, 0.7, lam)[0][:2]
        Fm, Gm = norm_reference(b, x - dx, 0.7, lam)[0][:2]
        assert np.all(np.abs((Fp - Fm) / (2 * h) - G[:, j]) <= 1e-7)
        assert np.all(np.abs(mu @ (Gp - Gm) / (2 * h) - H[:, j]) <= 1e-6 * max(1.0, np.abs(H).max()))
    # the value written out
    v = b.A @ x[c] + b.shift
    for r in range(3):
        s = slice(int(b.seg[r]), int(b.seg[r + 1]))
        assert abs(F[r] - np.sqrt(np.sum(b.weight[s] * v[s] ** 2))) <= 1e-13


# ---- (d) one model written two ways
def test_one_model_written_two_ways_agrees_within_the_added_bounds():
    rng = np.random.default_rng(72)
    N, d = 11, 4
    A, S, W = rng.standard_normal((N, d)), 1.0 + 0.3 * rng.standard_normal(N), rng.uniform(0.5, 1.5, N)
    cols = np.array([3, 1, 6, 4])
    x = rng.uniform(0.6, 1.4, 6)
    lam = np.array([0.0, 0.8])
    # a coefficient c on the norm is c^2 on its weights; the points in another order; split over the same row as two outputs of
    # which one has weight 0 throughout
    one = NlpNormBlock(cols, 3.0 * A, [2], [0, N], 3.0 * S, W)
    perm = rng.permutation(N)
    two = NlpNormBlock(cols, np.vstack([A[perm], A[:2]]), [2, 2], [0, N, N + 2], np.concatenate([S[perm], S[:2]]),
                       np.concatenate([9.0 * W[perm], np.zeros(2)]))
    (F1, G1, H1), (BF1, BG1, BH1), _, _ = norm_reference(one, x, 1.0, lam)
    (F2, G2, H2), (BF2, BG2, BH2), _, _ = norm_reference(two, x, 1.0, lam)
    assert F2[1] == 0.0 and not G2[1].any()
    assert abs(F1[0] - F2[0]) <= 4 * (BF1[0] + BF2[0]) and np.all(np.abs(G1[0] - G2[0]) <= 4 * (BG1[0] + BG2[0]))
    assert np.all(np.abs(H1 - H2) <= 4 * (BH1 + BH2)) and np.abs(H1).max() > 1e-2
    # a single-point output sqrt(W v^2) = sqrt(W) |v| with v > 0 is the linear function sqrt(W) (a'x + s)
    a, s, w = np.array([0.5, 0.25, 1.5, 0.75]), 0.5, 2.25
    (F, G, H), (BF, BG, BH), _, _ = norm_reference(NlpNormBlock(cols, a[None, :], [0], [0, 1], [s], [w]), x, 1.0, lam)
    lin = 1.5 * (a @ x[cols - 1] + s)
    tiny = 8 * 2.0 ** -53
    assert lin > 1.0 and abs(F[0] - lin) <= 4 * BF[0] + tiny * lin and np.all(np.abs(G[0] - 1.5 * a) <= 4 * BG[0] + tiny * 1.5 * a)
    assert np.all(np.abs(H) <= 4 * BH) and BH.max() < 1e-13


# ---- (e) the cases cover what they claim
def test_edge_cases_cover_the_shape_edges():
    short = 64                                                        # NLP_NORM_SHORT of csrc/nlp_norm_dev.hpp
    src = open(os.path.join(ROOT, "sqpsolver.jl_amd", "csrc", "nlp_norm_dev.hpp")).read()
    assert re.search(r"#define NLP_NORM_SHORT 64\b", src)
    assert [(c[0], c[1]) for c in EDGE_CASES] == [(1, 1), (5, 17), (193, 15), (133, 16), (68, 33), (1030, 20), (130, 128), (1100, 2)]
    lens, rows = [c[2] for c in EDGE_CASES], [c[3] for c in EDGE_CASES]
    assert lens[0] == (1,) and rows[0] == (5,) and lens[1] == (2, 3) and rows[1] == (0, 0)
    assert lens[2] == (1, short - 1, short, short + 1) and rows[2] == (4, 2, 4, 7)      # a short and a long output share row 4
    assert lens[3] == (1,) * 5 + (128,) and rows[3] == (0, 0, 9, 0, 3, 0)
    assert lens[4] == (4,) * 17 and rows[4] == (0,) * 17 and len(rows[4]) > 16 and len(rows[4]) % 4 != 0
    assert lens[5] == (1027, 3) and rows[5] == (2, 0) and lens[5][0] > 1024 and lens[5][0] > 16 * 64
    assert lens[6] == (129, 1) and rows[6] == (0, 9) and EDGE_CASES[6][1] == 128
    assert lens[7] == (1,) * 1100 and rows[7] == tuple((0, 2, 3)[r % 3] for r in range(1100)) and len(lens[7]) > 1024
    assert len(lens[7]) * EDGE_CASES[7][1] > 1024 and 3 * EDGE_CASES[7][1] < 1024
    assert (EDGE_LAM == 0).sum() == 1 and (EDGE_LAM < 0).sum() == 2 and len(EDGE_LAM) == M_EDGE
    for case in EDGE_CASES:
        p, lay, inst = edge_norm_model(*case)
        b = p.blocks[0]
        assert sum(case[2]) == case[0] and all(i == 0 or 2 <= i <= M_EDGE for i in case[3])
        cols = b.cols.tolist()
        assert case[1] == 1 or (cols != sorted(cols) and max(cols) - min(cols) + 1 > len(cols))
        for w, s in inst:
            assert np.all(w >= 0) and all(w[a:e].any() for a, e in zip(b.seg[:-1], b.seg[1:]))
        assert case[0] < 5 or sum((w == 0).sum() for w, _ in inst) >= 3 or max(case[2]) == 1
        assert len({tuple(w) for w, _ in inst}) == 3 and len({tuple(s) for _, s in inst}) == 3
        assert len(lay.hrow) == len(set(zip(lay.hrow.tolist(), lay.hcol.tolist()))) + 2
        assert len(lay.jrow) == len(set(zip(lay.jrow.tolist(), lay.jcol.tolist()))) + 2
    assert APEX[3][3] in APEX[3][:3] and APEX[3][4] in APEX[3][:3]     # the apex outputs sit on rows that other outputs use


# ---- (f) scipy's and the oracle's word on the solved cases of the GPU tests
def _solve(p, **kw):
    try:
        ro = O.sqp_solve(OracleNormTerms(p), O.default_options(**{**SQP_TIGHT, **kw}))
    finally:
        O.set_kkt_order(None)
    assert ro["status"] == 0, ro["status"]
    return ro


def _lin(kkt_mode):
    return dict(kkt_mode=2) if kkt_mode == 2 else dict(kkt_mode=1, kkt_tile_order=1)


@pytest.mark.parametrize("kkt_mode", [1, 2])
def test_oracle_solves_fermat_weber_and_scipy_agrees(kkt_mode):
    p = fermat_weber()
    b = p.blocks[0]
    assert p.m == 0 and b.rows.tolist() == [0] * 5 and b.A.shape == (15, 2) and np.all(b.shift[2::3] == 1e-3)
    ro = _solve(p, **_lin(kkt_mode))
    want = norm_scipy(p)
    print("iter", ro["iter"], "x", ro["x"], "scipy", np.abs(ro["x"] - want).max())
    assert np.abs(ro["x"] - want).max() <= 1e-6
    g = NlpNormNumpy(p).grad(ro["x"])
    assert np.abs(g).max() <= 1e-7                                      # stationary, strictly inside the box


@pytest.mark.parametrize("kkt_mode", [1, 2])
def test_oracle_solves_the_robust_lp_and_scipy_agrees(kkt_mode):
    p = robust_lp()
    ro = _solve(p, **_lin(kkt_mode))
    want = norm_scipy(p)
    print("iter", ro["iter"], "x", ro["x"], "scipy", np.abs(ro["x"] - want).max(), "g - b", ro["g"] - p.gU, "mult", ro["mult_g"])
    assert np.abs(ro["x"] - want).max() <= 1e-6
    active = (np.abs(ro["g"] - p.gU) <= 1e-8) & (np.abs(ro["mult_g"]) > 1e-3)
    assert active.sum() >= 2                                            # at least two active cone rows
    # the rows are what they say: a'x + kappa sqrt(|P x|^2 + delta^2)
    f, _, g, _, _ = norm_block_eval(p, ro["x"])
    assert f == 0.0 and np.all(g > 0)


@pytest.mark.parametrize("seed", SOCP_SEEDS)
def test_oracle_solves_the_synthetic_cone_programmes_and_scipy_agrees(seed):
    for k, p in enumerate(socp_cases(seed)):
        ro = _solve(p, kkt_mode=2)
        r1 = _solve(p, kkt_mode=1, kkt_tile_order=1)
        assert r1["iter"] == ro["iter"] and np.abs(r1["x"] - ro["x"]).max() <= 1e-8          # both linear solvers
        want = norm_scipy(p)
        active = int((np.abs(ro["g"] - p.gU) <= 1e-8).sum())
        print("seed", seed, "scenario", k, "iter", ro["iter"], "scipy", np.abs(ro["x"] - want).max(), "active rows", active)
        assert np.abs(ro["x"] - want).max() <= 1e-6
        assert active >= 1


def test_oracle_solves_the_queue_scenarios_and_they_differ():
    p, scen = socp_queue_case()
    assert scen[0] is p
    xs = [_solve(q, kkt_mode=2)["x"] for q in scen]
    assert min(np.abs(xs[a] - xs[b]).max() for a in range(6) for b in range(a)) > 1e-3


def test_the_generators_are_what_they_say():
    p = socp_synth(SOCP_N, SOCP_LENS, 1)
    b = p.blocks[0]
    lens = [3] * SOCP_LENS[0] + [k + 1 for k in SOCP_LENS[1:]]
    assert b.seg.tolist() == np.concatenate([[0], np.cumsum(lens)]).tolist()
    assert b.rows.tolist() == [0] * SOCP_LENS[0] + list(range(1, len(SOCP_LENS)))
    smooth = b.seg[1:] - 1
    assert not b.A[smooth].any() and np.all(b.shift[smooth] == 1e-2) and np.all(b.weight == 1.0)
    f, _, g, _, _ = norm_block_eval(p, np.zeros(p.n))
    assert np.all(g < p.gU - 0.49) and f > 0                            # x = 0 is strictly feasible
    assert np.all(p.xL == -3.0) and np.all(p.xU == 3.0) and not p.x0.any() and np.all(np.isinf(p.gL)) and p.num_linear == 0
    q = norm_scenario(p, 2, 1, 0.1)
    moved = q.blocks[0].shift != b.shift
    assert np.array_equal(q.blocks[0].A, b.A) and not moved[smooth].any() and moved.sum() == len(moved) - len(smooth)
    assert norm_scenario(p, 0, 1, 0.1) is p and norm_scenario(p, 3, 1, 0.0) is p
    assert np.array_equal(norm_scenario(p, 2, 1, 0.1).blocks[0].shift, q.blocks[0].shift)
    # Fermat-Weber: the value written out, weights as squares
    a = np.array([[0.0, 0.0], [3.0, 4.0]])
    m = sum_of_norms_model(a, weights=[2.0, 0.5], smooth=0.0)
    assert m.blocks[0].weight.tolist() == [4.0, 4.0, 0.25, 0.25] and m.blocks[0].rows.tolist() == [0, 0]
    assert abs(norm_block_eval(m, np.array([3.0, 0.0]))[0] - (2.0 * 3.0 + 0.5 * 4.0)) <= 1e-15
    # at an anchor the unsmoothed norm is at its apex: value exact, no derivative from that output
    f, g, _, _, H = norm_block_eval(m, np.array([0.0, 0.0]))
    assert f == 0.5 * 5.0 and np.allclose(g, 0.5 * np.array([-0.6, -0.8]), atol=1e-16) and np.all(np.isfinite(H))
    # the robust LP: the linear part is plain terms on the cone's row
    r = robust_lp_model([1.0, 0.0], [[2.0, 3.0]], [np.array([[1.0, 0.0], [0.0, 2.0]])], [0.5], [4.0])
    assert (r.m, r.num_linear) == (1, 0) and r.blocks[0].rows.tolist() == [1] and r.blocks[0].weight.tolist() == [0.25, 0.25]
    xx = np.array([1.0, -1.0])
    assert abs(NlpNormNumpy(r).g(xx)[0] - (2.0 - 3.0 + 0.5 * np.sqrt(1.0 + 4.0))) <= 1e-15 and r.gU[0] == 4.0


# ---- (g) layout and the refusals of the Python layer
def test_layout_and_refusals_of_the_python_layer():
    p, lay, _ = edge_norm_model(193, 15, (1, 63, 64, 65), (4, 2, 4, 7))
    pairs = set(zip(lay.hrow.tolist(), lay.hcol.tolist()))
    jp = set(zip(lay.jrow.tolist(), lay.jcol.tolist()))
    cols = p.blocks[0].cols.tolist()
    assert all((max(a, b), min(a, b)) in pairs for a in cols for b in cols)
    assert all((i, c) in jp for c in cols for i in (2, 4, 7)) and not any(r == 0 for r, _ in jp)
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
                       (dict(seg=[0, 3]), "seg: R + 1 = 3 values"),
                       (dict(rows=[0, 1, 2, 3], seg=[0, 1, 2, 3, 4]), "R = 4 outputs (1..3)"), (dict(rows=[], seg=[0]), "R = 0 outputs (1..3)"),
                       (dict(cols=[1, 1]), "2 distinct variables"), (dict(cols=[1, 2, 3]), "2 distinct variables"),
                       (dict(A=np.ones((3, 129)), cols=np.arange(1, 130)), "d = 129 columns (1..128)"),
                       (dict(weight=[1, 1]), "3 values each"), (dict(shift=[0.0] * 4), "3 values each")):
        with pytest.raises(ValueError, match=re.escape(words)):
            NlpNormBlock(**{**ok, **bad})
    blk = NlpNormBlock(**ok)
    assert blk.seg.dtype == np.int64 and np.array_equal(blk.weight, np.ones(3)) and not blk.shift.any()
    assert NlpNormBlock(**{**ok, **dict(rows=[2, 2])}).rows.tolist() == [2, 2]          # a repeated row is allowed
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
    # a zero-weight point is masked, whatever its residual
    q = make_nlp_terms(2, 2, 0, terms, blocks=[NlpNormBlock([1, 2], A, [0, 2], [0, 1, 3], [0.0, 0.25, np.inf], [1.0, 4.0, 0.0])])
    out = norm_block_eval(q, np.array([0.5, 0.25]), 1.0, np.array([0.0, 1.0]))
    assert all(np.all(np.isfinite(v)) for v in out) and out[0] == 0.75 and out[2][1] == 2.0


# ---- (h) header and binding
def test_header_carries_the_prototype_and_the_loader_binds_it():
    hdr = open(os.path.join(ROOT, "include", "sqphip.h")).read()
    code = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    m = re.search(r"int\s+sqphip_nlp_add_norm_block\s*\(([^;]*)\)\s*;", code)
    assert m, "prototype"
    kinds = [re.sub(r"\s*(\*?)\s*\w+$", r"\1", re.sub(r"\s+", " ", a.strip())) for a in m.group(1).split(",")]      # the type of an argument
    assert kinds == ["sqphip_ctx*", "int64_t", "int32_t", "const int64_t*", "const double*", "int32_t", "const int64_t*",
                     "const int64_t*", "const double*", "const double*", "int32_t*"], kinds
    assert "sqphip_nlp_add_norm_block" in _lib.EXPORTS
    src = open(os.path.join(ROOT, "sqpsolver.jl_amd", "_lib.py")).read()
    assert "L.sqphip_nlp_add_norm_block.argtypes = [vp, C.c_int64, C.c_int32, lp, dp, C.c_int32, lp, lp, dp, dp, ip]" in src
    assert "nlp_norm_dev.hpp" in _lib.HEADERS
    assert "apex" in hdr and "apex" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
