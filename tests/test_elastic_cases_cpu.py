"""The elastic, certificate and restart cases of tests/elastic_cases.py on the CPU: the generators keep their promises
(certificate margin in extended precision, reachability of the pair rows, stationarity of the planted point, the
max|c| conditions, the index ranges of the certificate rows), and the oracle (oracle/qp_ipm.c) meets a tenth of every
tolerance of tests/test_gpu_elastic_cases.py, returns LOCALLY_INFEASIBLE with zeros on every certificate case in every
listed mode under both ipm_phase1 values, and needs a second run on every restart case.  No GPU."""
import numpy as np
import pytest

import planted_qps as PQ
import elastic_cases as EC
from oracle import oracle as O

SETTINGS = {"default": dict(), "full": dict(kkt_condense=0), "dense": dict(kkt_mode=1), "corrector": dict(ipm_corrector=1)}
MODE = dict(QP=O.MODE_QP, SOC=O.MODE_SOC, L1QP=O.MODE_L1QP, INFEAS=O.MODE_INFEAS)
ids = lambda v: "-".join(str(a) for a in v) if isinstance(v, tuple) else str(v)


def _solve(q, mode, mu, **kw):
    O.set_kkt_order(None)
    return PQ.oracle_solver(q, O.default_options(**kw))(q, mode, mu)


def _within(errs, tol, frac=0.1):
    for k, e in errs.items():
        assert e <= frac * tol[k], (k, e, tol[k])


# ------------------------------------------------------------------ 1. the generators
@pytest.mark.parametrize("case", EC.elastic_list(), ids=ids)
def test_planted_elastic_point_is_stationary_and_violates_what_it_says(case):
    name, mu = case
    q = EC.case("elastic", name, mu); q0 = PQ.case(name); m = q.m
    assert q.num_linear == m - m // 2 and len(q.rows) >= 1 and min(q.rows) >= q.num_linear
    elig = (np.arange(m) >= q.num_linear) & (q0.rkind >= PQ.R_IN_BELOW)
    assert all(elig[i] for i in q.rows) and (m - 1 in q.rows) == bool(elig[m - 1])
    assert abs(len(q.rows) - elig.sum() / 2) <= 1                              # about half of the eligible rows
    # stationarity to the rounding of c (formed in extended precision, rounded once: eps / 2 x |c|)
    H = q.hess_mul(q.p) + q.c.astype(PQ.LD) - q.jact_mul(q.lam) - q.mult_x_L - q.mult_x_U
    assert float(np.abs(H).max()) <= 2.3e-16 * max(1.0, np.abs(q.c).max())
    # the violated rows: exactly t* outside their bound on the stated side, multiplier +-mu; every other row as planted
    row = (q.b.astype(PQ.LD) + q.jac_mul(q.p))
    viol = np.concatenate([np.maximum(q.gL.astype(PQ.LD) - row, 0), np.maximum(row - q.gU.astype(PQ.LD), 0)]).astype(np.float64)
    assert np.abs(viol - q.slack).max() <= 1e-15              # (an active row sits at its rounded value: eps / 2 x |r_i|, |r_i| < 8)
    assert np.count_nonzero(q.slack) == len(q.rows)
    t = q.slack[list(q.rows)] + q.slack[m + np.array(q.rows)]
    assert np.all((t >= 0.1 - 1e-15) & (t <= 1.0 + 1e-15))
    rows = np.array(q.rows)
    assert np.array_equal(q.lam[rows], np.where(q.slack[rows] > 0, mu, -mu))
    rest = np.setdiff1d(np.arange(m), rows)
    assert np.array_equal(q.lam[rest], q0.lam[rest]) and np.array_equal(q.gL[rest], q0.gL[rest]) and np.array_equal(q.gU[rest], q0.gU[rest])
    assert np.all(q.gL < q.gU) or np.array_equal(q.gL >= q.gU, q0.gL == q0.gU)         # no row changed its type
    assert np.all(np.abs(q0.lam) <= 2.0) and mu > 2.0                            # the penalty is exact on every other soft row
    # the cases keep meaning what they claim: the objective scale sf = 100 / max|c| acts at mu = 1000 only
    assert (np.abs(q.c).max() > 100.0) == (mu == 1000.0)
    if len(q.rows) >= 4:
        assert np.any(q.slack[:m] > 0) and np.any(q.slack[m:] > 0)               # both sides occur
        fin = np.isfinite(np.where(q.slack[rows] > 0, q.gU[rows], q.gL[rows])); assert fin.any() and (~fin).any()


def test_elastic_cases_of_one_name_differ_in_the_multipliers_alone():
    a, b = EC.case("elastic", "257x300", 3.0), EC.case("elastic", "257x300", 1000.0)
    assert a.rows == b.rows and np.array_equal(a.slack, b.slack) and np.array_equal(a.gL, b.gL) and np.array_equal(a.gU, b.gU)
    assert not np.array_equal(a.c, b.c) and np.array_equal(np.abs(a.lam[list(a.rows)]), np.full(len(a.rows), 3.0))
    q = EC.case("elastic", "long-rows", 10.0)
    assert np.bincount(q.jrow - 1)[list(q.rows)].max() <= 5          # (the long rows 0, 1 are linear; see the certificate cases)
    assert len(set(zip(q.jrow.tolist(), q.jcol.tolist()))) == len(q.jrow)
    q = EC.case("elastic", "dups", 10.0)
    assert len(set(zip(q.jrow.tolist(), q.jcol.tolist()))) < len(q.jrow)


@pytest.mark.parametrize("case", EC.farkas_list(), ids=ids)
def test_certificate_holds_in_extended_precision(case):
    name, kind, place = case
    q = EC.case("farkas", name, kind, place); q0 = PQ.case(name); m = q.m
    assert EC.certificate_margin(q) >= EC.MARGIN_MIN
    lo, hi = EC.place_range(m, q.num_linear, place)
    assert all(lo <= i < hi for i in q.rows) and set(np.nonzero(q.y)[0]) == set(q.rows)
    if place == "low": assert max(q.rows) < 64 and max(q.rows) < q.num_linear
    else:
        assert m - 1 in q.rows and min(q.rows) >= q.num_linear
        assert min(q.rows) >= EC.far_index(m) and EC.far_index(m) == (256 if m > 256 else 0)
    assert len(q.rows) == {"unreachable-1": 1, "pair": 2, "combo-5": min(5, hi - lo), "zero-row-1": 1}[kind]
    assert np.array_equal(q.gL == q.gU, q0.gL == q0.gU) and not np.any(np.isinf(q.gL) & np.isinf(q.gU))
    rest = np.setdiff1d(np.arange(m), q.rows)
    assert np.array_equal(q.gL[rest], q0.gL[rest]) and np.array_equal(q.gU[rest], q0.gU[rest])
    lb, ub = q.box(); assert np.all(np.isfinite(lb)) and np.all(np.isfinite(ub))
    assert np.abs(q.y).max() <= 2.0
    if kind in ("unreachable-1", "zero-row-1"):
        assert not EC.row_reachable(q, q.rows[0])
    if kind == "zero-row-1":
        assert not np.any(q.dense()[1][q.rows[0]]) and np.array_equal(q.jrow, q0.jrow) and m > 256
        assert np.array_equal(np.delete(q.dense()[1], q.rows[0], axis=0), np.delete(q0.dense()[1], q.rows[0], axis=0))
    if kind == "pair":
        assert EC.row_reachable(q, q.rows[0]) and EC.row_reachable(q, q.rows[1])
        _, J = q.dense(); i1, i2 = q.rows
        kappa = -J[i2][J[i1] != 0] / J[i1][J[i1] != 0]
        assert np.ptp(kappa) <= 1e-15 and 0.5 <= kappa[0] <= 2.0 and np.array_equal(J[i2] != 0, J[i1] != 0)
        assert len(q.jrow) > len(q0.jrow)
    if kind == "combo-5" and len(q.rows) >= 2:
        assert np.any(q.y > 0) and np.any(q.y < 0)
    # the planted programme the case was made from is feasible: the certificate rows alone make it infeasible
    r0 = q0.b.astype(PQ.LD) + q0.jac_mul(q0.p)
    assert np.all(r0[rest] >= q.gL[rest] - 1e-15) and np.all(r0[rest] <= q.gU[rest] + 1e-15)


def test_certificate_check_refuses_a_feasible_programme():
    q = EC.case("farkas", "65x33", "combo-5", "low")
    i = q.rows[0]; gL, gU = q.gL.copy(), q.gU.copy()
    if q.y[i] > 0: gL[i] -= 10.0
    else: gU[i] += 10.0
    assert EC.certificate_margin(PQ.dataclasses.replace(q, gL=gL, gU=gU)) < 0


def test_structure_cases_keep_a_certificate_row_in_the_condensed_matrix():
    q = EC.case("farkas", "long-rows", "combo-5", "low")
    cnt = np.bincount(q.jrow - 1, minlength=q.m)
    assert any(cnt[i] > 32 and q.gL[i] != q.gU[i] for i in q.rows)
    q = EC.case("farkas", "dups", "combo-5", "low")
    assert len(set(zip(q.jrow.tolist(), q.jcol.tolist()))) < len(q.jrow)


@pytest.mark.parametrize("case", EC.restart_list(), ids=ids)
def test_restart_rows_are_scaled_copies_with_large_multipliers(case):
    name, k = case
    q = EC.case("restart", name, k); q0 = PQ.case(name)
    assert len(q.rows) == k and all(q0.rkind[i] <= PQ.R_AT_GL for i in q.rows)
    if k == 2 and q.m > 256: assert q.rows[0] < 256 <= q.rows[1]
    _, J = q.dense(); _, J0 = q0.dense()
    for i in q.rows:
        assert np.abs(J[i] - EC.ROW_SCALE * J0[i]).max() <= 1e-19 and q.b[i] == q0.b[i] * EC.ROW_SCALE
        assert 1.2 * EC.RHO_BIG0 <= abs(q.lam[i]) <= 2.0 * EC.RHO_BIG0 and np.sign(q.lam[i]) == np.sign(q0.lam[i])
        assert (q.gL[i] == q.gU[i]) == (q0.gL[i] == q0.gU[i])
        assert np.array_equal(np.isfinite([q.gL[i], q.gU[i]]), np.isfinite([q0.gL[i], q0.gU[i]]))
    rest = np.setdiff1d(np.arange(q.m), q.rows)
    assert np.array_equal(J[rest], J0[rest]) and np.array_equal(q.lam[rest], q0.lam[rest]) and np.array_equal(q.p, q0.p)
    kk = PQ.kkt_residuals(q, q.planted())
    assert kk["stationarity"] <= 2e-15 and kk["feasibility"] <= 2e-15 and kk["complementarity"] <= 4e-11      # (|lam| = 2e4 x the rounding of a bound)
    assert kk["sign"] == 0.0 and kk["infinite_side"] == 0.0 and np.abs(q.c).max() < 100.0


def test_case_lists_are_deterministic():
    """The same bits on two generations."""
    for gen, args in [("elastic", a) for a in EC.elastic_list()] + [("farkas", a) for a in EC.farkas_list()] + \
                     [("restart", a) for a in EC.restart_list()] + [(g, tuple(a)) for g, *a in EC.stride_list()]:
        a, b = EC.case(gen, *args), getattr(EC, gen)(*args)
        assert a is not b and a.rows == b.rows and a.num_linear == b.num_linear
        for k in ("jrow", "jcol", "jval", "hval", "b", "c", "gL", "gU", "xL", "xU", "lam", "p", "slack", "y"):
            u, v = getattr(a, k), getattr(b, k)
            assert (u is None and v is None) or u.tobytes() == v.tobytes(), (gen, args, k)


def test_tolerances_are_ten_times_the_oracle_figures():
    def up(v):                           # rounded up to one digit
        e = np.floor(np.log10(v)); return float(np.ceil(v / 10 ** e - 1e-9) * 10 ** e)
    for worst, tol in ((EC.ORACLE_WORST_ELASTIC, EC.ELASTIC_TOL), (EC.ORACLE_WORST_ELASTIC_SF, EC.ELASTIC_SF_TOL),
                       (EC.ORACLE_WORST_ELASTIC_STRIDE, EC.ELASTIC_STRIDE_TOL),
                       (EC.ORACLE_WORST_RESTART, EC.RESTART_TOL), (EC.ORACLE_WORST_SOFT, EC.SOFT_TOL)):
        for k, v in worst.items():
            assert v > 0 and np.isclose(tol[k], up(10 * v), rtol=1e-12), (k, v, tol[k])


# ------------------------------------------------------------------ 1b. past the threads of a vector stage
SPARSE = {"sparse": dict(kkt_mode=2), "sparse-full": dict(kkt_mode=2, kkt_condense=0), "sparse-corrector": dict(kkt_mode=2, ipm_corrector=1)}


def test_stride_cases_lie_past_the_threads_of_a_vector_stage():
    q0 = EC.base(EC.STRIDE_NAME)
    assert q0.n > EC.VEC_THREADS and q0.m > EC.VEC_THREADS and 2 * q0.n + q0.m <= 7000       # (vectors still staged in LDS)
    k = PQ.kkt_residuals(q0, q0.planted())
    assert k["stationarity"] <= 2e-15 and k["feasibility"] <= 2e-15 and k["complementarity"] <= 4e-15
    for gen, *args in EC.stride_list():
        q = EC.case(gen, *args)
        assert max(q.rows) >= EC.VEC_THREADS, (gen, args)
        if gen == "farkas":
            assert min(q.rows) >= EC.VEC_THREADS and q.m - 1 in q.rows and EC.certificate_margin(q) >= EC.MARGIN_MIN
            assert np.array_equal(q.gL == q.gU, q0.gL == q0.gU) and np.abs(q.y).max() <= 2.0
        if gen == "elastic":
            assert np.abs(q.c).max() <= 100.0 and sum(i >= EC.VEC_THREADS for i in q.rows) >= 10
            H = q.hess_mul(q.p) + q.c.astype(PQ.LD) - q.jact_mul(q.lam) - q.mult_x_L - q.mult_x_U
            assert float(np.abs(H).max()) <= 2.3e-16 * np.abs(q.c).max()
        if gen == "restart":
            assert q.rows[0] < 256 and PQ.kkt_residuals(q, q.planted())["stationarity"] <= 2e-15


@pytest.mark.parametrize("setting", list(SPARSE))
def test_oracle_on_the_stride_cases(setting):
    kw = SPARSE[setting]
    for gen, name, *args in EC.stride_list():
        q = EC.case(gen, name, *args)
        if gen == "elastic":
            r = _solve(q, O.MODE_L1QP, args[0], **kw)
            assert r["status"] == O.MOI_LOCALLY_SOLVED and r["term_rule"] == 0
            _within(EC.errors(q, r), EC.elastic_tol(name, args[0]))
        elif gen == "restart":
            r0 = _solve(EC.base(name), O.MODE_QP, 1.0, **kw)
            for ph in (0, 1):
                r = _solve(q, O.MODE_QP, 1.0, ipm_phase1=ph, **kw)
                assert r["status"] == O.MOI_LOCALLY_SOLVED and r["ipm_iters"] > r0["ipm_iters"]
                _within(EC.errors(q, r), EC.RESTART_TOL)
        else:
            for ph in (0, 1):
                for md in EC.FARKAS_MODES["high"]:
                    r = _solve(q, MODE[md], PQ.MU_L1QP, ipm_phase1=ph, **kw)
                    ok = (O.MOI_LOCALLY_INFEASIBLE, O.MOI_ITERATION_LIMIT) if (args[0], ph) == ("zero-row-1", 0) else (O.MOI_LOCALLY_INFEASIBLE,)
                    assert r["status"] in ok and EC.all_zero(r), (args, md, ph, r["status"])
                r = _solve(q, O.MODE_L1QP, PQ.MU_L1QP, ipm_phase1=ph, **kw)
                assert r["status"] == O.MOI_LOCALLY_SOLVED
                _within(EC.hard_rows_of(q, r), EC.SOFT_TOL)


# ------------------------------------------------------------------ 2. the oracle on the elastic cases
@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("case", EC.elastic_list(), ids=ids)
def test_oracle_returns_the_planted_elastic_optimum(case, setting):
    name, mu = case
    q = EC.case("elastic", name, mu)
    r = _solve(q, O.MODE_L1QP, mu, **SETTINGS[setting])
    assert r["status"] == O.MOI_LOCALLY_SOLVED and r["term_rule"] == 0, (r["status"], r["ipm_iters"])
    _within(EC.errors(q, r), EC.elastic_tol(name, mu))


# ------------------------------------------------------------------ 3. the oracle's verdict on the certificate cases
@pytest.mark.parametrize("setting", ["default", "dense"])
@pytest.mark.parametrize("case", EC.farkas_list(), ids=ids)
def test_oracle_reports_every_certificate_case_infeasible(case, setting):
    name, kind, place = case
    q = EC.case("farkas", name, kind, place)
    for md in EC.FARKAS_MODES[place]:
        it = []
        for ph in (0, 1):
            r = _solve(q, MODE[md], PQ.MU_L1QP, ipm_phase1=ph, **SETTINGS[setting])
            it.append(r["ipm_iters"])
            if kind == "zero-row-1" and ph == 0:
                # the escalation rule cannot see a certificate on a row without coefficients: the penalty goes up to 1e10,
                # the last run ends LOCALLY_INFEASIBLE or ITERATION_LIMIT (tests/test_gpu_elastic_cases.py)
                assert r["status"] in (O.MOI_LOCALLY_INFEASIBLE, O.MOI_ITERATION_LIMIT) and EC.all_zero(r), (md, ph, r["status"])
                continue
            assert r["status"] == O.MOI_LOCALLY_INFEASIBLE and EC.all_zero(r), (md, ph, r["status"])
        assert it[1] > it[0] or kind == "zero-row-1", (md, it)                       # the phase-1 run happened
    if place == "high":                                      # certificate rows soft: a feasible programme
        for ph in (0, 1):
            r = _solve(q, O.MODE_L1QP, PQ.MU_L1QP, ipm_phase1=ph, **SETTINGS[setting])
            assert r["status"] == O.MOI_LOCALLY_SOLVED
            _within(EC.hard_rows_of(q, r), EC.SOFT_TOL)
            assert sum(r["slack"][i] + r["slack"][q.m + i] for i in q.rows) >= EC.MARGIN_MIN / 2   # (sum |y_i| v_i >= margin, |y_i| <= 2)


# ------------------------------------------------------------------ 4. the oracle on the restart cases
@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("case", EC.restart_list(), ids=ids)
def test_oracle_solves_every_restart_case_in_a_second_run(case, setting):
    name, k = case
    q = EC.case("restart", name, k)
    r0 = _solve(PQ.case(name), O.MODE_QP, 1.0, **SETTINGS[setting])
    for ph in (0, 1):
        r = _solve(q, O.MODE_QP, 1.0, ipm_phase1=ph, **SETTINGS[setting])
        assert r["status"] == O.MOI_LOCALLY_SOLVED, (ph, r["status"], r["ipm_iters"])
        _within(EC.errors(q, r), EC.RESTART_TOL)
        assert r["ipm_iters"] > r0["ipm_iters"], (ph, r["ipm_iters"], r0["ipm_iters"])
