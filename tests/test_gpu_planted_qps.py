"""The sub-problem seat (`sqphip_qp_solve`, `sqphip_qp_solve_batch`) on QPs with a planted optimum (tests/planted_qps.py),
at the size edges of the vector stages of csrc/ipm.hip: one 256-thread workgroup per instance, loops strided by 256 over
n, m and the entry counts, reductions over waves of 64 -- so n and m of 1, 63 / 64 / 65, 255 / 256 / 257, m > n, m = 0, a
completely dense Hessian, rows too long to eliminate, an empty row, repeated COO entries, and the last instance whose
vectors are staged in LDS.

Two references.  The planted values are arithmetic (closed form), independent of the oracle: tolerances
PQ.PLANTED_TOL / PQ.KKT_TOL = 10 x the oracle's own worst error (tests/test_planted_qps_cpu.py holds the oracle to a
tenth of them).  The oracle run of the same programme is the tight one: same status, same iteration count, TOL = 1e-8 on
all four vectors -- convex, strictly complementary, non-degenerate programmes leave no optimal face to wander on.

A row unbounded on both sides is refused at creation (asserted below), so no case has one."""
import numpy as np
import pytest

import sqpsolver_jl_amd as pkg
from sqpsolver_jl_amd.host import SqpHipError
from oracle import oracle as O
import planted_qps as PQ

pytestmark = pytest.mark.gpu
TOL = 1e-8
VECS = ("p", "lam", "mult_x_L", "mult_x_U")
# kkt_mode, kkt_condense, kkt_tile_order
SETTINGS = {"sparse-condensed": dict(kkt_mode=2, kkt_condense=1, kkt_tile_order=0),
            "sparse-full": dict(kkt_mode=2, kkt_condense=0, kkt_tile_order=0),
            "dense-condensed-tiled": dict(kkt_mode=1, kkt_condense=1, kkt_tile_order=1),
            "dense-full": dict(kkt_mode=1, kkt_condense=0, kkt_tile_order=0)}


def _ctx(q, batch=1, **kw):
    return pkg.Context(q.n, q.m, q.num_linear, q.jrow, q.jcol, q.hrow, q.hcol, q.xL, q.xU, q.gL, q.gU,
                       pkg.default_options(**kw), batch=batch)


def _oracle(q, mode=O.MODE_QP, mu=1.0, **kw):
    O.set_kkt_order(None)            # (the order hook is process-wide: QpSolver sets it again where kkt_tile_order asks for it)
    return PQ.oracle_solver(q, O.default_options(**kw))(q, mode, mu)


def _device(q, mode=O.MODE_QP, mu=1.0, **kw):
    ctx = _ctx(q, **kw)
    r = ctx.qp_solve(*q.seat_args(mode, mu))
    r["counters"] = ctx.counters()
    ctx.close()
    return r


def _meets_planted(q, rg, what=""):
    errs = {k: PQ.rel(rg[k], v) for k, v in q.planted().items()}
    print(what, "status", rg["status"], "iters", rg["ipm_iters"], "rule", rg["term_rule"], "planted errors", errs)
    assert rg["status"] == O.MOI_LOCALLY_SOLVED, (what, rg["status"], rg["ipm_iters"])
    for k, e in errs.items():
        assert e <= PQ.PLANTED_TOL[k], (what, k, e)
    assert rg["term_rule"] == 0, what


def _meets_oracle(ro, rg, what=""):
    errs = {k: PQ.rel(rg[k], ro[k]) for k in VECS}
    print(what, "oracle status", ro["status"], "iters", ro["ipm_iters"], "device against oracle", errs)
    assert (rg["status"], rg["ipm_iters"]) == (ro["status"], ro["ipm_iters"]), what
    for k, e in errs.items():
        assert e < TOL, (what, k, e)


def _meets_kkt(q, rg, what=""):
    k = PQ.kkt_residuals(q, rg)
    print(what, "KKT residuals", k)
    for name, v in k.items():
        assert v <= PQ.KKT_TOL[name], (what, name, v)


def _bits(r):
    return tuple(r[k].tobytes() for k in VECS) + (r["status"], r["ipm_iters"])


# ------------------------------------------------------------------ 1. the planted optimum at every size edge
@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("name", PQ.SIZE_NAMES)
def test_planted_optimum_at_every_size_edge(name, setting):
    q = PQ.case(name); kw = SETTINGS[setting]
    rg = _device(q, **kw)
    assert rg["counters"]["sparse"] == (kw["kkt_mode"] == 2)
    _meets_planted(q, rg, f"{name} {setting}")
    _meets_kkt(q, rg, f"{name} {setting}")
    _meets_oracle(_oracle(q, **kw), rg, f"{name} {setting}")


# ------------------------------------------------------------------ 2. structures
@pytest.mark.parametrize("name", ["hfull-2", "hfull-64", "hfull-65"])
def test_completely_dense_hessian(name):
    """All n (n + 1) / 2 entries: `hess_row` reads the mirrored column.  kkt_mode = 0 lets the library choose the solver: a
    dense Hessian is one clique of n variables, the multifrontal plan saves nothing and the dense LDL' is chosen."""
    q = PQ.case(name)
    rg = _device(q, kkt_mode=0)
    assert rg["counters"]["sparse"] == 0
    _meets_planted(q, rg, name); _meets_kkt(q, rg, name)
    _meets_oracle(_oracle(q, kkt_mode=1), rg, name)
    for kw in (SETTINGS["sparse-condensed"], SETTINGS["dense-full"]):
        rg = _device(q, **kw)
        _meets_planted(q, rg, f"{name} {kw}"); _meets_oracle(_oracle(q, **kw), rg, f"{name} {kw}")


@pytest.mark.parametrize("kkt_mode", [1, 2])
def test_rows_too_long_to_eliminate_stay_in_the_condensed_matrix(kkt_mode):
    """Inequality rows of 33 and 40 entries (more than KKT_LONG_ROW = 32) under kkt_condense = 1: they keep their unknowns,
    with a genuine -D block; one of them is active at gU."""
    q = PQ.case("long-rows"); kw = dict(kkt_mode=kkt_mode, kkt_condense=1, kkt_tile_order=0)      # (the tile order pads the matrix)
    rg = _device(q, **kw)
    assert rg["counters"]["kkt_order"] == q.n + int(np.sum(q.gL == q.gU)) + 2
    _meets_planted(q, rg, "long rows"); _meets_kkt(q, rg, "long rows")
    _meets_oracle(_oracle(q, **kw), rg, "long rows")
    assert rg["lam"][0] < 0 and q.lam[1] == 0           # the long row active at its upper side: lambda <= 0 in the JuMP sign


@pytest.mark.parametrize("name", ["empty-row", "dups", "no-rows-257"])
@pytest.mark.parametrize("setting", ["sparse-condensed", "dense-condensed-tiled", "dense-full"])
def test_empty_row_repeated_entries_and_no_rows(name, setting):
    q = PQ.case(name); kw = SETTINGS[setting]
    rg = _device(q, **kw)
    _meets_planted(q, rg, f"{name} {setting}"); _meets_kkt(q, rg, f"{name} {setting}")
    _meets_oracle(_oracle(q, **kw), rg, f"{name} {setting}")
    if name == "no-rows-257":
        assert rg["lam"].shape == (0,)
        assert rg["counters"]["kkt_order"] == q.n or kw["kkt_tile_order"]          # (the tile order pads the matrix)


def test_a_row_unbounded_on_both_sides_is_refused():
    """ROW_FREE exists on the device for the LP phase (non-linear rows are switched off there), but a row with gL = -Inf and
    gU = +Inf is refused by `sqphip_create` and `sqphip_set_bounds`: the planted cases have none."""
    q = PQ.case("7x3")
    gL, gU = q.gL.copy(), q.gU.copy(); gL[1], gU[1] = -np.inf, np.inf
    with pytest.raises(SqpHipError):
        pkg.Context(q.n, q.m, q.num_linear, q.jrow, q.jcol, q.hrow, q.hcol, q.xL, q.xU, gL, gU, pkg.default_options())
    ctx = _ctx(q)
    with pytest.raises(SqpHipError):
        ctx.set_bounds(0, PQ.dataclasses.replace(q, gL=gL, gU=gU))
    _meets_planted(q, ctx.qp_solve(*q.seat_args()), "after the refused bounds")      # the context keeps its bounds
    ctx.close()


# ------------------------------------------------------------------ 3. vector-stage paths
@pytest.mark.parametrize("name", ["65x33", "257x300", "300x600"])
def test_vector_stage_paths_give_the_same_bits(name, monkeypatch):
    """The fused stages with their vectors in LDS (default at these sizes), the fused stages reading global memory
    (SQPHIP_NO_VSTAGE=1) and the flat sparse-product kernels (SQPHIP_VEC_FLAT=1): the same sums by the same routines."""
    q = PQ.case(name); got = {}
    for path in ("lds", "no-lds", "flat"):
        monkeypatch.delenv("SQPHIP_VEC_FLAT", raising=False); monkeypatch.delenv("SQPHIP_NO_VSTAGE", raising=False)
        if path == "no-lds": monkeypatch.setenv("SQPHIP_NO_VSTAGE", "1")
        if path == "flat": monkeypatch.setenv("SQPHIP_VEC_FLAT", "1")
        got[path] = _device(q, **SETTINGS["sparse-condensed"])
        _meets_planted(q, got[path], f"{name} {path}")
    assert _bits(got["lds"]) == _bits(got["no-lds"]) == _bits(got["flat"])
    _meets_oracle(_oracle(q, **SETTINGS["sparse-condensed"]), got["lds"], name)


@pytest.mark.parametrize("name", list(PQ.LDS_EDGE))
def test_last_instance_staged_in_lds_and_first_that_is_not(name):
    """n + N = 2 n + m = 7000 doubles (56 000 bytes of dynamic LDS beside the static LDS of the reductions) is the last
    instance whose vectors are staged, 7001 the first that runs the flat kernels; no switches.  n = 3400 with 200 / 201
    equality rows, banded pattern: the library's own choice (kkt_mode = 0) is the sparse solver on both sides."""
    q = PQ.case(name)
    assert 2 * q.n + q.m == int(name.split("-")[1])
    rg = _device(q)
    assert rg["counters"]["sparse"] == 1 and rg["counters"]["kkt_order"] == q.n + q.m
    _meets_planted(q, rg, name); _meets_kkt(q, rg, name)
    _meets_oracle(_oracle(q), rg, name)


# ------------------------------------------------------------------ 4. the start point on its bounds
ON_BOUND = ["1x0", "2x1", "7x3", "65x33", "on-bound-257"]


@pytest.mark.parametrize("name", ON_BOUND)
def test_start_point_on_its_bounds(name):
    """x_k exactly on the bound the step moves away from (the normal state of an SQP iterate), monotone rule (default)."""
    q = PQ.on_bound(PQ.case(name))
    lb, ub = q.box()
    assert np.any(lb == 0) or np.any(ub == 0)
    for kw in (dict(), SETTINGS["sparse-condensed"]):
        rg = _device(q, **kw)
        _meets_planted(q, rg, f"{name} on bound {kw}"); _meets_kkt(q, rg, f"{name} on bound {kw}")
        _meets_oracle(_oracle(q, **kw), rg, f"{name} on bound {kw}")


# ------------------------------------------------------------------ 5. other modes
@pytest.mark.parametrize("mode", ["SOC", "L1QP"])
@pytest.mark.parametrize("name", ["7x3", "65x33", "257x300"])
def test_soc_and_l1qp_return_the_planted_optimum(name, mode):
    """The second-order-correction programme (the QP under half the iteration limit) and the l1-penalty programme with
    mu = 10 above every planted |lambda| <= 2: the same p and multipliers, no elastic mass."""
    q = PQ.case(name)
    md, mu = (O.MODE_SOC, 1.0) if mode == "SOC" else (O.MODE_L1QP, PQ.MU_L1QP)
    for kw in (SETTINGS["sparse-condensed"], SETTINGS["dense-full"]):
        rg = _device(q, md, mu, **kw)
        _meets_planted(q, rg, f"{name} {mode} {kw}")
        print("largest slack", np.abs(rg["slack"]).max())
        assert np.abs(rg["slack"]).max() <= PQ.SLACK_TOL
        _meets_oracle(_oracle(q, md, mu, **kw), rg, f"{name} {mode} {kw}")


# ------------------------------------------------------------------ 6. non-convex variants
@pytest.mark.parametrize("setting", ["sparse-condensed", "dense-condensed-tiled"])
@pytest.mark.parametrize("name", ["7x3", "65x33", "256x256", "300x600"])
def test_nonconvex_variants_return_kkt_points(name, setting):
    """A third of the Hessian's diagonal negated: inertia corrections on the way; whatever local solution is returned
    satisfies the KKT conditions, and the run is the oracle's (status, iteration count)."""
    q = PQ.nonconvex(PQ.case(name)); kw = SETTINGS[setting]
    rg = _device(q, **kw)
    assert rg["status"] == O.MOI_LOCALLY_SOLVED
    _meets_kkt(q, rg, f"{name} non-convex {setting}")
    ro = _oracle(q, **kw)
    print("device", rg["status"], rg["ipm_iters"], rg["n_factor"], "oracle", ro["status"], ro["ipm_iters"], ro["n_factor"])
    assert (rg["status"], rg["ipm_iters"]) == (ro["status"], ro["ipm_iters"])


# ------------------------------------------------------------------ 7. batch
@pytest.mark.parametrize("name", ["65x33", "257x300"])
def test_batch_of_five_value_sets_on_one_structure(name):
    """Five value seeds on one structure, bounds per instance through set_bounds, one qp_solve_batch call with a permuted
    instance list: each request meets its own planted optimum and is bit-equal to the single qp_solve of the same
    programme on a context of its own."""
    n, m = (int(v) for v in name.split("x"))
    qs = [PQ.case(name, vseed=s) for s in range(5)]
    for q in qs[1:]:
        assert np.array_equal(q.jrow, qs[0].jrow) and np.array_equal(q.hcol, qs[0].hcol) and np.array_equal(q.rkind, qs[0].rkind)
        assert not np.array_equal(q.jval, qs[0].jval) and not np.array_equal(q.xL, qs[0].xL)
    kw = SETTINGS["sparse-condensed"]
    inst = [3, 0, 4, 1, 2]
    ctx = _ctx(qs[0], batch=5, **kw)
    for k, q in enumerate(qs):
        ctx.set_bounds(inst[k], q)
    rs = ctx.qp_solve_batch(inst, [O.MODE_QP] * 5, [q.x_k for q in qs], [q.delta for q in qs], 1.0, [q.c for q in qs],
                            [q.b for q in qs], [q.jval for q in qs], [q.hval for q in qs])
    ctx.close()
    for k, q in enumerate(qs):
        _meets_planted(q, rs[k], f"{name} request {k} on instance {inst[k]}")
        single = _device(q, **kw)
        assert _bits(rs[k]) == _bits(single), k
    assert len({r["p"].tobytes() for r in rs}) == 5


# ------------------------------------------------------------------ 8. the predictor-corrector rule
@pytest.mark.parametrize("on_bound", [0, 1])
@pytest.mark.parametrize("name", ON_BOUND)
def test_predictor_corrector_rule(name, on_bound):
    q = PQ.on_bound(PQ.case(name)) if on_bound else PQ.case(name)
    rg = _device(q, ipm_corrector=1)
    _meets_planted(q, rg, f"{name} corrector"); _meets_kkt(q, rg, f"{name} corrector")
    _meets_oracle(_oracle(q, ipm_corrector=1), rg, f"{name} corrector")


# min 0.5 h p^2 + c p, no rows, delta = 1: the start point on, just inside or just outside its upper bound, optimum -c / h
ONE_VAR = dict(h=1.17659791, c=0.76824136, x_k=0.62845148, xL=-1.56303591, delta=1.0, p=-0.6529344931)
ONE_VAR_XU = (0.59494881, 0.62, 0.6284, 0.63)


def _one_var(xU, corrector):
    e = np.zeros(0); ei = np.zeros(0, dtype=np.int64)
    ctx = pkg.Context(1, 0, 0, ei, ei, [1], [1], [ONE_VAR["xL"]], [xU], e, e, pkg.default_options(ipm_corrector=corrector))
    rg = ctx.qp_solve(O.MODE_QP, [ONE_VAR["x_k"]], ONE_VAR["delta"], 1.0, [ONE_VAR["c"]], e, e, [ONE_VAR["h"]])
    ctx.close()
    s = O.QpSolver(1, 0, 0, np.array([0, 0]), ei, np.array([0, 1]), np.array([0]), [ONE_VAR["xL"]], [xU], [], [],
                   O.default_options(ipm_corrector=corrector))
    ro = s.solve(O.MODE_QP, [ONE_VAR["x_k"]], ONE_VAR["delta"], 1.0, [ONE_VAR["c"]], e, e, [ONE_VAR["h"]])
    print("xU", xU, "device", rg["status"], rg["ipm_iters"], rg["p"], "oracle", ro["status"], ro["ipm_iters"], ro["p"])
    return rg, ro


@pytest.mark.parametrize("corrector", [0, 1])
@pytest.mark.parametrize("xU", ONE_VAR_XU)
def test_one_variable_programme(xU, corrector):
    """The predictor-corrector rule used to repeat four iterates for ever on this programme (ITERATION_LIMIT after 200
    iterations, zeroed outputs); its stall guard (b_ipm_prepare; oracle ipm_run) hands over to the monotone rule after
    eight iterations without progress.  Both rules reach the optimum, by the oracle's iterations."""
    rg, ro = _one_var(xU, corrector)
    assert rg["status"] == O.MOI_LOCALLY_SOLVED and rg["term_rule"] == 0 and rg["ipm_iters"] <= 20
    assert abs(rg["p"][0] - ONE_VAR["p"]) <= PQ.PLANTED_TOL["p"]
    assert abs(rg["mult_x_L"][0]) <= PQ.PLANTED_TOL["mult_x_L"] and abs(rg["mult_x_U"][0]) <= PQ.PLANTED_TOL["mult_x_U"]
    _meets_oracle(ro, rg, f"one variable, xU = {xU}, corrector {corrector}")
