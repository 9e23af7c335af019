"""The planted-optimum QPs of tests/planted_qps.py on the CPU: the generator is self-consistent, and the oracle
(oracle/qp_ipm.c) meets every tolerance of tests/test_gpu_planted_qps.py divided by 10 on every committed case -- the
condition under which those tolerances (10 x the oracle's worst error) mean anything.  No GPU."""
import numpy as np
import pytest

import planted_qps as PQ
from oracle import oracle as O

SETTINGS = {"default": dict(), "full": dict(kkt_condense=0), "dense": dict(kkt_mode=1), "corrector": dict(ipm_corrector=1)}
MODES = {"QP": (O.MODE_QP, 1.0), "SOC": (O.MODE_SOC, 1.0), "L1QP": (O.MODE_L1QP, PQ.MU_L1QP)}
SMALL = PQ.SIZE_NAMES + list(PQ.STRUCTURES)


def _within(errs, tol, frac=0.1):
    for k, e in errs.items():
        assert e <= frac * tol[k], (k, e, tol[k])


def _planted_errors(q, r):
    return {k: PQ.rel(r[k], v) for k, v in q.planted().items()}


# ------------------------------------------------------------------ 1. the generator
@pytest.mark.parametrize("name", PQ.ALL_NAMES)
def test_planted_point_satisfies_the_kkt_conditions_to_rounding(name):
    q = PQ.case(name)
    k = PQ.kkt_residuals(q, q.planted())
    # c is formed in extended precision and rounded once: the residual is that rounding (eps/2 * |c|, |c| <= 10) plus the
    # rounding of the active rows' bounds
    assert k["stationarity"] <= 2e-15 and k["feasibility"] <= 2e-15 and k["complementarity"] <= 4e-15, k
    assert k["sign"] == 0.0 and k["infinite_side"] == 0.0
    assert q.sigma > PQ.SIGMA_MIN and q.redraws < 200
    assert np.abs(q.c).max() < 100.0                      # below the objective scaling of both implementations
    H, J = q.dense()
    assert np.allclose(H, H.T) and np.all(2 * np.diag(H) > np.abs(H).sum(axis=1))      # strictly diagonally dominant
    lb, ub = q.box()
    assert np.all(lb < ub) and np.all(q.p >= lb) and np.all(q.p <= ub)
    inside = q.vkind == PQ.V_BOX
    assert np.all((q.xL < q.x_k)[inside] & (q.x_k < q.xU)[inside])
    assert np.all(np.abs(q.lam[q.lam != 0]) >= 0.1) and np.all(np.abs(q.lam) <= 2.0) and PQ.MU_L1QP > 2.0
    assert np.sum(q.vkind >= PQ.V_AT_XL) <= q.n // 3 and np.sum(q.rkind <= PQ.R_AT_GL) <= max(q.n // 3, 0)


def test_independence_measure_is_the_smallest_singular_value_of_the_active_block():
    q = PQ.case("65x33")
    _, J = q.dense()
    A = J[np.ix_(q.rkind <= PQ.R_AT_GL, q.vkind <= PQ.V_BOX)]
    assert A.shape[0] > 0 and abs(np.linalg.svd(A, compute_uv=False).min() - q.sigma) < 1e-12
    # the multipliers follow from p* through that block alone: solve the stationarity rows of the free variables
    H, _ = q.dense()
    free = q.vkind <= PQ.V_BOX
    lam_act, *_ = np.linalg.lstsq(A.T, (H @ q.p + q.c)[free], rcond=None)
    assert np.abs(lam_act - q.lam[q.rkind <= PQ.R_AT_GL]).max() < 1e-12


def test_every_variable_kind_and_row_kind_occurs():
    vk = np.concatenate([PQ.case(nm).vkind for nm in PQ.ALL_NAMES]); rk = np.concatenate([PQ.case(nm).rkind for nm in PQ.ALL_NAMES])
    assert set(vk) == set(range(6)) and set(rk) == set(range(6))
    for nm in ("65x33", "257x300", "300x600"):            # the shapes of the vector-stage and batch tests carry every kind themselves
        assert set(PQ.case(nm).vkind) == set(range(6)) and set(PQ.case(nm).rkind) == set(range(6)), nm
    # active sides have their two variants: the other side infinite, and finite
    q = PQ.case("257x300")
    for kind, other in ((PQ.V_AT_XL, q.xU), (PQ.V_AT_XU, q.xL)):
        fin = np.isfinite(other[q.vkind == kind]); assert fin.any() and (~fin).any()
    for kind, other in ((PQ.R_AT_GU, q.gL), (PQ.R_AT_GL, q.gU)):
        fin = np.isfinite(other[q.rkind == kind]); assert fin.any() and (~fin).any()


def test_structure_options_are_what_they_say():
    q = PQ.case("hfull-65")
    assert len(q.hrow) == 65 * 66 // 2 and np.count_nonzero(q.dense()[0]) == 65 * 65
    q = PQ.case("long-rows")
    cnt = np.bincount(q.jrow - 1, minlength=q.m)
    assert cnt[0] == 33 and cnt[1] == 40 and cnt[2:].max() <= 5 and q.gL[0] != q.gU[0] and q.gL[1] != q.gU[1]
    assert q.rkind[0] == PQ.R_AT_GU and q.lam[0] < 0
    q = PQ.case("empty-row")
    i = q.m - 1
    assert not np.any(q.jrow - 1 == i) and q.gL[i] < q.b[i] < q.gU[i] and q.lam[i] == 0
    assert PQ.case("no-rows-257").m == 0 and len(PQ.case("no-rows-257").jrow) == 0
    for nm, tot in (("lds-7000", 7000), ("lds-7001", 7001)):
        q = PQ.case(nm); assert 2 * q.n + q.m == tot and np.all(q.gL == q.gU)


def test_duplicate_entries_sum_to_the_plain_matrices():
    """The same seeds with and without repeated COO entries: a repeated entry takes a share of its original's value, so
    both give the same dense matrices (to the rounding of v - s + s) and the same planted point."""
    qd = PQ.case("dups"); qp = PQ.generate(63, 40, pseed=0, vseed=0)
    for r, c in ((qd.jrow, qd.jcol), (qd.hrow, qd.hcol)):
        assert len(set(zip(r.tolist(), c.tolist()))) < len(r)
    assert len(qd.jrow) > len(qp.jrow) and len(qd.hrow) > len(qp.hrow)
    Hd, Jd = qd.dense(); Hp, Jp = qp.dense()
    assert np.array_equal(Hd != 0, Hp != 0) and np.array_equal(Jd != 0, Jp != 0)
    assert np.abs(Hd - Hp).max() <= 4e-16 * np.abs(Hp).max() and np.abs(Jd - Jp).max() <= 4e-16 * np.abs(Jp).max()
    assert np.array_equal(qd.p, qp.p) and np.array_equal(qd.lam, qp.lam) and np.abs(qd.c - qp.c).max() <= 1e-14
    # and a duplicate really carries part of the value: dropping the repeats changes the matrices
    first = PQ.dataclasses.replace(qd, hval=np.where(PQ.pattern(63, 40, 0, dups=True).hdup < 0, qd.hval, 0.0))
    assert not np.allclose(first.dense()[0], Hd)
    jcp, jrv, jslot, _ = O.coo_to_csc(qd.n, qd.jrow, qd.jcol)
    jv = np.zeros(len(jrv)); np.add.at(jv, jslot, qd.jval)
    assert len(jrv) == (Jd != 0).sum() and np.allclose(np.sort(np.abs(jv)), np.sort(np.abs(Jd[Jd != 0])), rtol=1e-14)


def test_variants_keep_what_they_promise():
    q = PQ.case("65x33")
    b = PQ.on_bound(q)
    moved = (b.xL != q.xL) | (b.xU != q.xU)
    assert 1 <= moved.sum() <= max(1, q.n // 6) and np.all((b.xL == b.x_k)[moved] | (b.xU == b.x_k)[moved])
    lb, ub = b.box()
    assert np.all((lb == 0)[moved] | (ub == 0)[moved]) and np.all(np.abs(b.p[moved]) > 0.05)
    k = PQ.kkt_residuals(b, b.planted())
    assert max(k.values()) <= 4e-15
    v = PQ.nonconvex(q)
    Hq, Hv = q.dense()[0], v.dense()[0]
    flipped = np.diag(Hv) < 0
    assert flipped.sum() == q.n // 3 and np.array_equal(np.diag(Hv)[flipped], -np.diag(Hq)[flipped])
    assert np.array_equal(Hv - np.diag(np.diag(Hv)), Hq - np.diag(np.diag(Hq))) and np.linalg.eigvalsh(Hv).min() < 0
    # a wrong answer does not pass the residual check: one multiplier with the other sign, one step entry moved
    bad = {k2: a.copy() for k2, a in q.planted().items()}; bad["lam"][np.argmax(np.abs(q.lam))] *= -1
    assert PQ.kkt_residuals(q, bad)["stationarity"] > 1e-2
    bad = {k2: a.copy() for k2, a in q.planted().items()}; j = int(np.argmax(q.vkind == PQ.V_AT_XL)); bad["p"][j] -= 1e-3
    assert PQ.kkt_residuals(q, bad)["feasibility"] > 9e-4
    bad = {k2: a.copy() for k2, a in q.planted().items()}; j = int(np.argmax(q.vkind == PQ.V_AT_XL))
    bad["mult_x_U"][j], bad["mult_x_L"][j] = -q.mult_x_L[j], 0.0
    assert PQ.kkt_residuals(q, bad)["complementarity"] > 1e-3


# ------------------------------------------------------------------ 2. the oracle meets a tenth of every tolerance
@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("name", SMALL)
def test_oracle_reaches_the_planted_optimum(name, setting):
    q = PQ.case(name)
    solve = PQ.oracle_solver(q, O.default_options(**SETTINGS[setting]))
    for mname, (mode, mu) in MODES.items():
        r = solve(q, mode, mu)
        assert r["status"] == O.MOI_LOCALLY_SOLVED and r["term_rule"] == 0, (mname, r["status"], r["ipm_iters"])
        _within(_planted_errors(q, r), PQ.PLANTED_TOL)
        _within(PQ.kkt_residuals(q, r), PQ.KKT_TOL)
        assert np.abs(r["slack"]).max(initial=0.0) <= PQ.SLACK_TOL, mname


@pytest.mark.parametrize("name", list(PQ.LDS_EDGE))
def test_oracle_reaches_the_planted_optimum_at_the_lds_edge(name):
    """n = 3400: the sparse factorisation under the default options (order >= 3000), plain and with x_k on bounds."""
    q = PQ.case(name)
    for qq in (q, PQ.on_bound(q)):
        r = PQ.oracle_solver(qq, O.default_options())(qq)
        assert r["status"] == O.MOI_LOCALLY_SOLVED and r["term_rule"] == 0
        _within(_planted_errors(qq, r), PQ.PLANTED_TOL)
        _within(PQ.kkt_residuals(qq, r), PQ.KKT_TOL)


# ------------------------------------------------------------------ 3. variants
@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("name", SMALL)
def test_oracle_on_the_variants(name, setting):
    q = PQ.case(name)
    opts = O.default_options(**SETTINGS[setting])
    b = PQ.on_bound(q)
    r = PQ.oracle_solver(b, opts)(b)
    assert r["status"] == O.MOI_LOCALLY_SOLVED
    _within(_planted_errors(b, r), PQ.PLANTED_TOL)
    _within(PQ.kkt_residuals(b, r), PQ.KKT_TOL)
    v = PQ.nonconvex(q)
    r = PQ.oracle_solver(v, opts)(v)
    assert r["status"] == O.MOI_LOCALLY_SOLVED
    _within(PQ.kkt_residuals(v, r), PQ.KKT_TOL)


ONE_VAR = dict(h=1.17659791, c=0.76824136, x_k=0.62845148, xL=-1.56303591, delta=1.0, p=-0.6529344931)
ONE_VAR_XU = (0.59494881, 0.62, 0.6284, 0.63)


def one_var_oracle(xU, corrector):
    s = O.QpSolver(1, 0, 0, np.array([0, 0]), np.zeros(0, dtype=np.int64), np.array([0, 1]), np.array([0]),
                   [ONE_VAR["xL"]], [xU], [], [], O.default_options(ipm_corrector=corrector))
    return s.solve(O.MODE_QP, [ONE_VAR["x_k"]], ONE_VAR["delta"], 1.0, [ONE_VAR["c"]], np.zeros(0), np.zeros(0), [ONE_VAR["h"]])


@pytest.mark.parametrize("corrector", [0, 1])
@pytest.mark.parametrize("xU", ONE_VAR_XU)
def test_oracle_one_variable_programme(xU, corrector):
    """min 0.5 h p^2 + c p with the start point on, just inside or just outside its upper bound; optimum -c / h far inside.
    The predictor-corrector rule used to repeat four iterates for ever on it (ITERATION_LIMIT after 200 iterations); its
    stall guard (qp_ipm.c, ipm_run) hands over to the monotone rule after eight iterations without progress."""
    assert abs(-ONE_VAR["c"] / ONE_VAR["h"] - ONE_VAR["p"]) < 1e-10
    r = one_var_oracle(xU, corrector)
    assert r["status"] == O.MOI_LOCALLY_SOLVED and r["term_rule"] == 0 and r["ipm_iters"] <= 20
    assert abs(r["p"][0] - ONE_VAR["p"]) <= 0.1 * PQ.PLANTED_TOL["p"]
    assert r["mult_x_L"][0] <= 0.1 * PQ.PLANTED_TOL["mult_x_L"] and abs(r["mult_x_U"][0]) <= 0.1 * PQ.PLANTED_TOL["mult_x_U"]


def test_stall_guard_leaves_converging_predictor_corrector_runs_alone():
    """With an upper bound a little further away (xU = 0.7: the start is not pushed against the bound) the predictor-corrector rule
    needs 5 iterations, fewer than the guard's eight: the guard cannot have acted."""
    r = one_var_oracle(0.7, 1)
    assert r["status"] == O.MOI_LOCALLY_SOLVED and r["ipm_iters"] == 5 and abs(r["p"][0] - ONE_VAR["p"]) <= 0.1 * PQ.PLANTED_TOL["p"]
