"""The decision at the end of every interior-point run of the sub-problem seat (`b_qp_finish`, csrc/ipm.hip: accept,
restart with rho_big * 100, phase 1 under options.ipm_phase1, or LOCALLY_INFEASIBLE) and the elastic variables it reads
and returns, on the cases of tests/elastic_cases.py:

  1. a planted elastic optimum under L1QP: `slack` entry-wise, all 2 m entries, t+ before t-; multipliers +-mu on the violated
     soft rows at mu = 3, 10 and 1000 (at 1000 the objective scale sf = 100 / max|c| < 1 enters the soft weight mu * sf and
     is divided out of every multiplier);
  2. programmes with a Farkas certificate, its rows below index 64 or far out (from index 256 on; from 1024 on in the
     case of 1100 rows, past the 1024 threads whose strided loops reduce the elastic mass): LOCALLY_INFEASIBLE and exact
     zeros in every mode in which the rows are hard, under ipm_phase1 = 0 and 1; LOCALLY_SOLVED where they are soft;
  3. a feasible programme with one or two rows scaled by 1e-4 (multipliers of 1.2e4 .. 2e4, above the penalty 1e4): solved
     after a restart, also by way of phase 1;
  4. all of these side by side in one batched call, against the scalar call bit for bit.

References: the planted values (arithmetic; tolerances EC.*_TOL = 10 x the oracle's own worst error, see elastic_cases.py)
and the oracle run of the same programme (status, iteration count, TOL = 1e-8 on the five vectors).  The verdict cases
have no tolerance; their reference is the certificate, evaluated in np.longdouble by the generator
(tests/test_elastic_cases_cpu.py asserts it for every case)."""
import dataclasses

import numpy as np
import pytest

import sqpsolver_jl_amd as pkg
from oracle import oracle as O
import planted_qps as PQ
import elastic_cases as EC
from test_gpu_planted_qps import SETTINGS, _ctx, _oracle

pytestmark = pytest.mark.gpu
TOL = 1e-8
MODE = dict(QP=O.MODE_QP, SOC=O.MODE_SOC, L1QP=O.MODE_L1QP, INFEAS=O.MODE_INFEAS)
ids = lambda v: "-".join(str(a) for a in v) if isinstance(v, tuple) else str(v)


def _device(q, mode, mu, bounds=(), **kw):
    """One seat call on a context of its own; `bounds`: further cases of the same structure, each solved on the same
    context after `set_bounds` (their requests as (case, mode, mu))."""
    ctx = _ctx(q, **kw)
    out = [ctx.qp_solve(*q.seat_args(mode, mu))]
    for q2, mode2, mu2 in bounds:
        ctx.set_bounds(0, q2)
        out.append(ctx.qp_solve(*q2.seat_args(mode2, mu2)))
    ctx.close()
    return out if bounds else out[0]


def _meets_planted(q, rg, tol, what):
    errs = EC.errors(q, rg)
    print(what, "status", rg["status"], "iters", rg["ipm_iters"], "rule", rg["term_rule"], "planted errors", errs)
    assert rg["status"] == O.MOI_LOCALLY_SOLVED, (what, rg["status"], rg["ipm_iters"])
    for k, e in errs.items():
        assert e <= tol[k], (what, k, e)


def _meets_oracle(ro, rg, what):
    errs = {k: PQ.rel(rg[k], ro[k]) for k in EC.VECS}
    print(what, "oracle status", ro["status"], "iters", ro["ipm_iters"], "rule", ro["term_rule"], "device iters", rg["ipm_iters"],
          "rule", rg["term_rule"], "device against oracle", errs)
    # (the rule that ended the last run: 0 on every elastic case; the two-row restart case at 65x33 ends by the first
    # acceptable-termination rule at a scaled error of 1.06e-9 in both implementations)
    assert (rg["status"], rg["ipm_iters"], rg["term_rule"]) == (ro["status"], ro["ipm_iters"], ro["term_rule"]), what
    for k, e in errs.items():
        assert e < TOL, (what, k, e)


def _bits(r):
    return tuple(r[k].tobytes() for k in EC.VECS) + (r["status"], r["ipm_iters"])


# ------------------------------------------------------------------ 1. planted elastic optimum
ELASTIC = [(nm, 10.0, st) for nm in EC.ELASTIC_SIZES for st in SETTINGS] + \
          [(nm, mu, st) for nm in EC.ELASTIC_MU_SIZES for mu in (3.0, 1000.0) for st in ("sparse-condensed", "dense-full")] + \
          [("long-rows", 10.0, "sparse-condensed"), ("dups", 10.0, "dense-condensed-tiled"), (EC.STRIDE_NAME, 10.0, "sparse-condensed")]


@pytest.mark.parametrize("case", ELASTIC, ids=ids)
def test_planted_elastic_optimum(case):
    name, mu, setting = case
    q = EC.case("elastic", name, mu); kw = SETTINGS[setting]; what = f"elastic {name} mu {mu} {setting}"
    rg = _device(q, O.MODE_L1QP, mu, **kw)
    _meets_planted(q, rg, EC.elastic_tol(name, mu), what)
    assert rg["term_rule"] == 0, what
    _meets_oracle(_oracle(q, O.MODE_L1QP, mu, **kw), rg, what)


# ------------------------------------------------------------------ 2. planted infeasibility
FARKAS = [c + (st,) for c in EC.farkas_list() if c[0] in EC.FARKAS_SIZES for st in ("sparse-condensed", "dense-condensed-tiled")] + \
         [c + (st,) for c in EC.farkas_list() if c[0] == "257x300" and c[1] != "zero-row-1" for st in ("sparse-full", "dense-full")] + \
         [c + ("sparse-condensed",) for c in EC.farkas_list() if c[0] in EC.FARKAS_STRUCTURES] + \
         [tuple(a) + ("sparse-condensed",) for g, *a in EC.stride_list() if g == "farkas"]


@pytest.mark.parametrize("case", FARKAS, ids=ids)
def test_certified_infeasible_programme(case):
    """LOCALLY_INFEASIBLE with exact zeros in every mode in which the certificate rows are hard, by the oracle's
    iterations; with ipm_phase1 = 1 the verdict needs the phase-1 run, which shows in the iteration count.  Certificate
    rows among the non-linear rows ('high') are soft under L1QP: that programme is feasible, the returned point satisfies
    every hard row and carries the certified violation on the soft ones.

    'zero-row-1' (one row with all-zero coefficients on the wrong side of its bound) is the case whose ONLY elastic mass sits
    on the certificate row, the last one (index 1099 >= 1024 in the case of 1100 rows): the other rows keep their planted optimum.  With
    ipm_phase1 = 1 the phase-1 run decides it like every other case.  With ipm_phase1 = 0 the rule that tells a small
    penalty from an infeasible programme compares |H p + c| with the terms |J_ij y_i|, which vanish on such a row: it
    raises the penalty up to 1e10 before giving up, and the run there may end LOCALLY_INFEASIBLE or ITERATION_LIMIT (the
    oracle does the same; a limit of the shared rule).  Asserted there: never LOCALLY_SOLVED, zeros."""
    name, kind, place, setting = case
    q = EC.case("farkas", name, kind, place); kw = SETTINGS[setting]; what = f"{name} {kind} {place} {setting}"
    iters = {}
    for ph in (0, 1):
        ctx = _ctx(q, ipm_phase1=ph, **kw)
        for md in EC.FARKAS_MODES[place]:
            rg = ctx.qp_solve(*q.seat_args(MODE[md], PQ.MU_L1QP))
            iters[md, ph] = rg["ipm_iters"]
            if kind == "zero-row-1" and ph == 0:            # (the escalation rule cannot see this certificate, see the docstring)
                print(what, md, "phase1", ph, "device", rg["status"], rg["ipm_iters"])
                assert rg["status"] != O.MOI_LOCALLY_SOLVED and EC.all_zero(rg), (what, md, ph, rg["status"])
                continue
            ro = _oracle(q, MODE[md], PQ.MU_L1QP, ipm_phase1=ph, **kw)
            print(what, md, "phase1", ph, "device", rg["status"], rg["ipm_iters"], "oracle", ro["status"], ro["ipm_iters"])
            assert rg["status"] == O.MOI_LOCALLY_INFEASIBLE and EC.all_zero(rg), (what, md, ph, rg["status"])
            assert (rg["status"], rg["ipm_iters"]) == (ro["status"], ro["ipm_iters"]), (what, md, ph)
        if place == "high":
            rg = ctx.qp_solve(*q.seat_args(O.MODE_L1QP, PQ.MU_L1QP))
            ro = _oracle(q, O.MODE_L1QP, PQ.MU_L1QP, ipm_phase1=ph, **kw)
            hr = EC.hard_rows_of(q, rg)
            mass = sum(rg["slack"][i] + rg["slack"][q.m + i] for i in q.rows)
            print(what, "soft, phase1", ph, "device", rg["status"], rg["ipm_iters"], "oracle", ro["status"], ro["ipm_iters"], hr, "mass", mass)
            assert rg["status"] == O.MOI_LOCALLY_SOLVED
            for k, v in hr.items():
                assert v <= EC.SOFT_TOL[k], (what, k, v)
            # sum |y_i| v_i >= margin for the violations v of every point of the box, |y_i| <= 2
            assert mass >= EC.MARGIN_MIN / 2
            assert (rg["status"], rg["ipm_iters"]) == (ro["status"], ro["ipm_iters"]), (what, "soft", ph)
        ctx.close()
    for md in EC.FARKAS_MODES[place]:
        assert iters[md, 1] > iters[md, 0] or kind == "zero-row-1", (what, md, iters)


# ------------------------------------------------------------------ 3. penalty restart
RESTART = [c + (st,) for c in EC.restart_list() for st in SETTINGS] + [(EC.STRIDE_NAME, 2, "sparse-condensed")]


@pytest.mark.parametrize("case", RESTART, ids=ids)
def test_badly_scaled_row_is_solved_after_a_restart(case):
    """|lambda_i| of 1.2e4 .. 2e4 on a row scaled by 1e-4: the first run (rho_big = 1e4) leaves elastic mass on it, the
    second (1e6) solves the programme -- more iterations than the unscaled case of the same name, which needs one run.
    With ipm_phase1 = 1 a phase-1 run in between finds the rows feasible and hands back to stage 0 with the larger penalty."""
    name, k, setting = case
    q = EC.case("restart", name, k); q0 = EC.base(name); kw = SETTINGS[setting]; what = f"restart {name} {k} {setting}"
    for ph in (0, 1):
        rg, r0 = _device(q, O.MODE_QP, 1.0, bounds=[(q0, O.MODE_QP, 1.0)], ipm_phase1=ph, **kw)
        # (the unscaled programme runs second on the same context: the penalty is back at 1e4, the oracle's iterations)
        ro0 = _oracle(q0, O.MODE_QP, 1.0, ipm_phase1=ph, **kw)
        assert (r0["status"], r0["ipm_iters"]) == (ro0["status"], ro0["ipm_iters"]) == (O.MOI_LOCALLY_SOLVED, ro0["ipm_iters"])
        _meets_planted(q, rg, EC.RESTART_TOL, f"{what} phase1 {ph}")
        print(what, "iterations", rg["ipm_iters"], "unscaled", r0["ipm_iters"])
        assert rg["ipm_iters"] > r0["ipm_iters"]
        _meets_oracle(_oracle(q, O.MODE_QP, 1.0, ipm_phase1=ph, **kw), rg, f"{what} phase1 {ph}")


# ------------------------------------------------------------------ 4. batch with mixed outcomes
@pytest.mark.parametrize("phase1", [0, 1])
def test_batch_with_mixed_outcomes(phase1):
    """Five requests on one structure in one `qp_solve_batch` call -- one run, an elastic optimum, an infeasible
    programme, a restart (two runs, while its neighbours are idle), another infeasible one under SOC -- on a context of six
    instances whose sixth holds an earlier result: every listed result is the scalar `qp_solve` of the same request on a
    fresh one-instance context, bit for bit, and the sixth instance is untouched."""
    name = EC.BATCH_NAME; q0 = PQ.case(name); nl = q0.m - q0.m // 2
    nlin = lambda q: dataclasses.replace(q, num_linear=nl)
    reqs = [(nlin(q0), O.MODE_QP, 1.0, O.MOI_LOCALLY_SOLVED),
            (EC.case("elastic", name, 3.0), O.MODE_L1QP, 3.0, O.MOI_LOCALLY_SOLVED),
            (EC.case("farkas", name, "combo-5", "low"), O.MODE_QP, 1.0, O.MOI_LOCALLY_INFEASIBLE),
            (nlin(EC.case("restart", name, 2)), O.MODE_QP, 1.0, O.MOI_LOCALLY_SOLVED),
            (EC.case("farkas", name, "unreachable-1", "high"), O.MODE_SOC, 1.0, O.MOI_LOCALLY_INFEASIBLE)]
    held = (EC.case("elastic", name, 10.0), O.MODE_L1QP, 10.0)
    for q, *_ in reqs + [held]:
        assert q.num_linear == nl and np.array_equal(q.jrow, q0.jrow) and np.array_equal(q.jcol, q0.jcol)
    kw = dict(ipm_phase1=phase1, **SETTINGS["sparse-condensed"])
    inst = [3, 0, 4, 1, 2]
    ctx = _ctx(nlin(q0), batch=6, **kw)
    col = lambda rs, f: [f(q, md, mu) for q, md, mu, *_ in rs]
    call = lambda ins, rs: ctx.qp_solve_batch(ins, col(rs, lambda q, md, mu: md), col(rs, lambda q, md, mu: q.x_k),
                                              col(rs, lambda q, md, mu: q.delta), col(rs, lambda q, md, mu: mu),
                                              col(rs, lambda q, md, mu: q.c), col(rs, lambda q, md, mu: q.b),
                                              col(rs, lambda q, md, mu: q.jval), col(rs, lambda q, md, mu: q.hval))
    ctx.set_bounds(5, held[0])
    first = call([5], [held])[0]
    assert first["status"] == O.MOI_LOCALLY_SOLVED
    for k, (q, *_) in enumerate(reqs):
        ctx.set_bounds(inst[k], q)
    rs = call(inst, reqs)
    after = ctx.seat_peek(5)
    ctx.close()
    for k in EC.VECS:
        assert np.array_equal(after[k], first[k]), k
    assert after["status"] == first["status"]
    for k, (q, md, mu, want) in enumerate(reqs):
        single = _device(q, md, mu, **kw)
        print("request", k, "instance", inst[k], "status", rs[k]["status"], "iters", rs[k]["ipm_iters"], "scalar iters", single["ipm_iters"])
        assert rs[k]["status"] == want, k
        assert _bits(rs[k]) == _bits(single), k
    _meets_planted(reqs[1][0], rs[1], EC.ELASTIC_TOL, "batched elastic request")
    _meets_planted(reqs[3][0], rs[3], EC.RESTART_TOL, "batched restart request")
    assert EC.all_zero(rs[2]) and EC.all_zero(rs[4])
    assert rs[3]["ipm_iters"] > rs[0]["ipm_iters"]
