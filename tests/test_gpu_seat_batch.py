"""GPU tests of the batched drop-in seat (sqphip_qp_solve_batch, sqphip_qp_stats_batch and the *_batch merit calls).

The yardstick is the scalar seat: request k of a batch call on instance inst[k] must return bit for bit what
sqphip_qp_solve returns for the same request on a one-instance context that carries the bounds of inst[k] -- every
comparison with it is exact (np.array_equal, integer equality).  The oracle is consulted once more for the tiny NLPs, at
the tolerances test_gpu_parity.py documents for the scalar seat (restated below)."""
import ctypes as C

import numpy as np
import pytest

import sqpsolver_jl_amd as pkg
from sqpsolver_jl_amd.host import SqpHipError
from sqpsolver_jl_amd.acopf_synth import acopf_synth, acopf_layout, contingency, CASES
from oracle import oracle as O
import host_mirror as HM
import host_mirror_batch as HMB

pytestmark = pytest.mark.gpu

TOL = 1e-8
VEC = ("p", "lam", "mult_x_U", "mult_x_L", "slack")
NUM = ("status", "ipm_iters", "n_factor", "term_rule", "scaled_error")
ALL_MODES = (O.MODE_QP, O.MODE_FR, O.MODE_SOC, O.MODE_LP, O.MODE_L1QP, O.MODE_INFEAS)


def rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(1.0, np.abs(np.asarray(b)).max()))


def _same(rb, rs, what=""):
    """a batched result against the scalar seat: every bit"""
    for k in VEC:
        assert np.array_equal(rb[k], rs[k]), (what, k, float(np.abs(rb[k] - rs[k]).max()))
    for k in NUM:
        assert rb[k] == rs[k], (what, k, rb[k], rs[k])


def _ctx(S, bounds=None, batch=1, **opt):
    b = bounds or S
    return pkg.Context(S["n"], S["m"], S["num_linear"], S["jrow"], S["jcol"], S["hrow"], S["hcol"], b["xL"], b["xU"],
                       b["gL"], b["gU"], pkg.default_options(**opt), batch=batch)


def _lay_struct(lay):
    return dict(n=lay.n, m=lay.m, num_linear=lay.num_linear, jrow=lay.jrow, jcol=lay.jcol, hrow=lay.hrow, hcol=lay.hcol,
                xL=lay.xL, xU=lay.xU, gL=lay.gL, gU=lay.gU)


def _scalar(S, req, bounds=None, **opt):
    """the request through sqphip_qp_solve on a fresh one-instance context with the given bounds"""
    ctx = _ctx(S, bounds, 1, **opt)
    r = ctx.qp_solve(*req)
    ctx.close()
    return r


def _batch(ctx, inst, reqs):
    col = lambda j: [r[j] for r in reqs]
    return ctx.qp_solve_batch(inst, col(0), col(1), col(2), col(3), col(4), col(5), col(6), col(7))


def _request(P, S, x, lam, mode, delta, mu):
    return (mode, x, delta, mu, P.eval_grad_f(x), P.eval_g(x), P.eval_jac_g(x), P.eval_h(x, 1.0, lam))


# ---- the oracle side of test 1: _oracle_qp, _compare_qp and _tols of tests/test_gpu_parity.py, restated
def _oracle_qp(S, opts=None):
    n = S["n"]
    jcp, jrv, jslot, _ = O.coo_to_csc(n, S["jrow"], S["jcol"])
    hcp, hrv, hslot, hslot_t = O.coo_to_csc(n, S["hrow"], S["hcol"], sym=True)
    q = O.QpSolver(n, S["m"], S["num_linear"], jcp, jrv, hcp, hrv, S["xL"], S["xU"], S["gL"], S["gU"], opts)

    def solve(mode, x, delta, mu, df, E, jcoo, hcoo):
        jv = np.zeros(len(jrv)); np.add.at(jv, jslot, jcoo)
        hv = np.zeros(len(hrv))
        if hcoo is not None and len(hcoo):
            np.add.at(hv, hslot, hcoo); ok = hslot_t >= 0; np.add.at(hv, hslot_t[ok], hcoo[ok])
        return q.solve(mode, x, delta, mu, df, E, jv, hv, want_slack=True)
    return solve


# FR and INFEAS minimise the elastic mass only (a non-trivial optimal face): p at 1e-5, the optimal value at 1e-8, the
# iteration count within a half; everything else at 1e-8 with equal counts.  With the monotone barrier rule (the default,
# used here) the multipliers of the LP-like modes are pinned to 1e-8 as well.
def _tols(mode):
    return dict(mult_tol=TOL, p_tol=1e-5 if mode in (O.MODE_FR, O.MODE_INFEAS) else TOL)


def _compare_oracle(ro, rg, mult_tol=TOL, p_tol=TOL):
    assert rg["status"] == ro["status"]
    for k in ("p", "lam", "mult_x_U", "mult_x_L"):
        assert rel(rg[k], ro[k]) < (p_tol if k == "p" else mult_tol), k
    if p_tol > TOL and ro["status"] == O.MOI_LOCALLY_SOLVED:
        vo, vg = float(np.sum(ro["slack"])), float(np.sum(rg["slack"]))
        assert abs(vg - vo) <= TOL * max(1.0, abs(vo))
    if ro["status"] == O.MOI_LOCALLY_SOLVED:
        if p_tol > TOL:
            assert abs(rg["ipm_iters"] - ro["ipm_iters"]) <= max(2, ro["ipm_iters"] // 2)
        else:
            assert rg["ipm_iters"] == ro["ipm_iters"]
    else:
        assert not rg["p"].any() and not rg["lam"].any()


# ------------------------------------------------------------------ 1: all modes, tiny NLPs
@pytest.mark.parametrize("name", ["toy", "readme1", "hs071"])
def test_all_modes_on_tiny_nlps_in_one_call(name):
    """Eight requests -- the six modes, two radii, three points as test_qp_modes_small_problems builds them -- in one call on
    a context of eight instances: each equals the scalar seat exactly and the oracle at the documented tolerances."""
    P = getattr(O, "problem_" + name)(); S = P.structure()
    rng = np.random.default_rng(1)
    pts = []
    for trial in range(3):
        x = P.x0 + (0.3 * rng.standard_normal(S["n"]) if trial else 0)
        x = np.clip(x, np.maximum(S["xL"], -1e3), np.minimum(S["xU"], 1e3))
        pts.append((x, rng.standard_normal(S["m"]) * (trial > 0)))
    plan = [(O.MODE_QP, 10.0, 0), (O.MODE_FR, 0.5, 1), (O.MODE_SOC, 10.0, 2), (O.MODE_LP, 0.5, 0), (O.MODE_L1QP, 10.0, 1),
            (O.MODE_INFEAS, 0.5, 2), (O.MODE_QP, 0.5, 1), (O.MODE_L1QP, 0.5, 2)]
    reqs = [_request(P, S, *pts[t], mode, delta, 7.0) for mode, delta, t in plan]
    ctx = _ctx(S, batch=8)
    out = _batch(ctx, list(range(8)), reqs)
    ctx.close()
    osolve = _oracle_qp(S, O.default_options())
    for k, req in enumerate(reqs):
        _same(out[k], _scalar(S, req), (name, k))
        _compare_oracle(osolve(*req), out[k], **_tols(req[0]))


# ------------------------------------------------------------------ 2 and 9: sparse path, per-instance bounds; counters
def _contingency_requests(case, count, plan, seed=2, spread=0.02):
    nb, ng, nl, sd = CASES[case]
    net = acopf_synth(nb, ng, nl, sd); lay0 = acopf_layout(net)
    rng = np.random.default_rng(seed)
    lays, reqs = [], []
    for k in range(count):
        nk = contingency(net, k + 1, 7); lk = acopf_layout(nk)
        P = O.problem_acopf(nk, lk); S = P.structure()
        x = np.clip(lk.x0 + spread * rng.standard_normal(lk.n), lk.xL, lk.xU)
        mode, delta = plan[k % len(plan)]
        reqs.append(_request(P, S, x, 50 * rng.standard_normal(lk.m), mode, delta, 3.0))
        lays.append(lk)
    return lay0, lays, reqs


CASE14_PLAN = [(O.MODE_QP, 10.0), (O.MODE_QP, 0.2), (O.MODE_FR, 0.2), (O.MODE_SOC, 1.0), (O.MODE_L1QP, 1.0),
               (O.MODE_INFEAS, 1.0), (O.MODE_LP, 10.0), (O.MODE_QP, 1.0)]


@pytest.fixture(scope="module")
def case14_call():
    """One batch call of eight contingency networks of the case14 structure on the multifrontal path, each instance with
    its own bounds; with the counters before and after it."""
    lay0, lays, reqs = _contingency_requests("case14", 8, CASE14_PLAN)
    ctx = _ctx(_lay_struct(lay0), batch=8, kkt_mode=2)
    for k, lk in enumerate(lays):
        ctx.set_bounds(k, lk)
    c0 = ctx.counters()
    out = _batch(ctx, list(range(8)), reqs)
    c1 = ctx.counters()
    it, nf = C.c_int32(), C.c_int32()
    ctx.L.sqphip_qp_stats(ctx.h, C.byref(it), C.byref(nf))
    ctx.close()
    scalar, n_solve = [], 0
    for k, req in enumerate(reqs):          # eight one-instance contexts created with the bounds of the eight networks
        c1k = _ctx(_lay_struct(lay0), _lay_struct(lays[k]), 1, kkt_mode=2)
        scalar.append(c1k.qp_solve(*req))
        n_solve += c1k.counters()["n_solve"]
        c1k.close()
    return dict(lay0=lay0, lays=lays, reqs=reqs, out=out, c0=c0, c1=c1, last=(it.value, nf.value), scalar=scalar,
                scalar_n_solve=n_solve)


def test_sparse_path_with_per_instance_bounds(case14_call):
    """Exact against eight one-instance contexts created with the bounds of the eight networks."""
    c = case14_call
    assert c["c1"]["sparse"] == 1
    for k in range(8):
        _same(c["out"][k], c["scalar"][k], ("case14", k))
    assert len({r["ipm_iters"] for r in c["out"]}) > 1          # (the requests are not eight copies of one)


def test_sparse_path_on_taller_fronts():
    """case118, four contingency networks, QP mode: fronts taller than any of case14."""
    lay0, lays, reqs = _contingency_requests("case118", 4, [(O.MODE_QP, 10.0), (O.MODE_QP, 2.0)], spread=0.005)
    S = _lay_struct(lay0)
    ctx = _ctx(S, batch=4, kkt_mode=2)
    for k, lk in enumerate(lays):
        ctx.set_bounds(k, lk)
    out = _batch(ctx, [0, 1, 2, 3], reqs)
    ctx.close()
    for k, req in enumerate(reqs):
        assert out[k]["status"] == O.MOI_LOCALLY_SOLVED
        _same(out[k], _scalar(S, req, _lay_struct(lays[k]), kkt_mode=2), ("case118", k))


def test_counters_advance_by_the_sums_over_the_batch(case14_call):
    c = case14_call
    d = {k: c["c1"][k] - c["c0"][k] for k in ("n_qp", "n_ipm_iter", "n_factor", "n_solve", "total_seconds")}
    assert d["n_qp"] == 8
    assert d["n_ipm_iter"] == sum(r["ipm_iters"] for r in c["out"])
    assert d["n_factor"] == sum(r["n_factor"] for r in c["out"])
    assert d["n_solve"] == c["scalar_n_solve"] > 0          # (not in the per-request stats: against the eight scalar contexts)
    assert d["total_seconds"] > 0.0
    # sqphip_qp_stats describes request count - 1
    assert c["last"] == (c["out"][7]["ipm_iters"], c["out"][7]["n_factor"])


# ------------------------------------------------------------------ 3: subset, order, isolation
def test_subset_order_and_isolation():
    P = O.problem_hs071(); S = P.structure()
    rng = np.random.default_rng(3)

    def req(mode, delta):
        x = np.clip(P.x0 + 0.3 * rng.standard_normal(S["n"]), S["xL"], S["xU"])
        return _request(P, S, x, rng.standard_normal(S["m"]), mode, delta, 7.0)
    ctx = _ctx(S, batch=8)
    first = [req(ALL_MODES[k % 6], (10.0, 0.5)[k % 2]) for k in range(8)]
    saved = _batch(ctx, list(range(8)), first)
    # three requests on instances 5, 0, 2: results in request order, the other five instances untouched
    sub = [req(O.MODE_QP, 10.0), req(O.MODE_L1QP, 0.5), req(O.MODE_FR, 10.0)]
    out = _batch(ctx, [5, 0, 2], sub)
    for k in range(3):
        _same(out[k], _scalar(S, sub[k]), ("subset", k))
    rest = [1, 3, 4, 6, 7]
    stats = ctx.qp_stats_batch(rest)
    for j, b in enumerate(rest):
        held = ctx.seat_peek(b)
        for key in VEC:
            assert np.array_equal(held[key], saved[b][key]), (b, key)
        assert held["status"] == saved[b]["status"]
        assert stats[j] == {key: saved[b][key] for key in ("ipm_iters", "n_factor", "term_rule", "scaled_error")}, b
    assert ctx.qp_stats_batch([2, 5]) == [{key: out[k][key] for key in ("ipm_iters", "n_factor", "term_rule", "scaled_error")}
                                          for k in (2, 0)]
    # a second subset
    sub2 = [req(O.MODE_SOC, 0.5), req(O.MODE_QP, 0.5)]
    out2 = _batch(ctx, [7, 1], sub2)
    for k in range(2):
        _same(out2[k], _scalar(S, sub2[k]), ("second subset", k))
    # misuse: refused with the index, nothing modified
    before = [ctx.seat_peek(b) for b in range(8)]
    for bad, idx in (([2, 4, 2], 2), ([0, 8], 1), ([3, -1, 4], 1)):
        with pytest.raises(SqpHipError, match=r"inst\[%d\]" % idx):
            _batch(ctx, bad, sub[:len(bad)])
    with pytest.raises(SqpHipError, match=r"mode\[1\]"):
        _batch(ctx, [0, 1], [sub[0], (9,) + sub[1][1:]])
    with pytest.raises(SqpHipError, match="count"):
        _batch(ctx, list(range(8)) + [0], first + [first[0]])
    after = [ctx.seat_peek(b) for b in range(8)]
    for b in range(8):
        for key in VEC:
            assert np.array_equal(before[b][key], after[b][key])
        assert before[b]["status"] == after[b]["status"]
    ctx.close()


# ------------------------------------------------------------------ 4: unequal work, an infeasible neighbour
HS071_INFEASIBLE_RADIUS = 0.1
# hs071 at x0 = (1, 5, 5, 1): the equality row reads 52 + (2, 10, 10, 2)'p = 40, and |(2, 10, 10, 2)'p| <= 24 delta inside
# the trust region -- inconsistent for every delta < 0.5 (the oracle returns LOCALLY_INFEASIBLE at 0.1, checked below)


def test_unequal_work_and_an_infeasible_neighbour():
    P = O.problem_hs071(); S = P.structure()
    rng = np.random.default_rng(4)
    x1 = np.clip(P.x0 + 0.3 * rng.standard_normal(S["n"]), S["xL"], S["xU"])
    x2 = np.clip(P.x0 + 0.3 * rng.standard_normal(S["n"]), S["xL"], S["xU"])
    lam = rng.standard_normal(S["m"])
    reqs = [_request(P, S, x1, lam, O.MODE_QP, 10.0, 7.0),
            _request(P, S, P.x0, 0 * lam, O.MODE_QP, HS071_INFEASIBLE_RADIUS, 7.0),
            _request(P, S, x2, lam, O.MODE_FR, 0.5, 7.0),
            _request(P, S, x2, lam, O.MODE_LP, 10.0, 7.0)]
    assert _oracle_qp(S, O.default_options())(*reqs[1])["status"] == O.MOI_LOCALLY_INFEASIBLE
    ctx = _ctx(S, batch=4)
    out = _batch(ctx, [0, 1, 2, 3], reqs)
    stats = ctx.qp_stats_batch([0, 1, 2, 3])
    ctx.close()
    assert out[1]["status"] == O.MOI_LOCALLY_INFEASIBLE
    for key in VEC:
        assert not out[1][key].any(), key
    for k, req in enumerate(reqs):
        _same(out[k], _scalar(S, req), ("unequal", k))
    assert [s["ipm_iters"] for s in stats] == [r["ipm_iters"] for r in out]
    assert len({s["ipm_iters"] for s in stats}) >= 2            # differing work: the call lasted as long as its slowest request


# ------------------------------------------------------------------ 5: more instances than one wave of the request kernel
def test_more_instances_than_one_wave():
    P = O.problem_toy(); S = P.structure()
    rng = np.random.default_rng(5)
    reqs = []
    for k in range(70):
        # around the solution (-1, -1): at the start point (0, 0) the linearised row x0 x1 = 1 has no solution in any radius
        x = np.array([-1.0, -1.0]) + 0.1 * rng.standard_normal(S["n"])
        reqs.append(_request(P, S, x, rng.standard_normal(S["m"]), O.MODE_QP, (10.0, 0.5)[k % 2], 7.0))
    ctx = _ctx(S, batch=70)
    fwd = _batch(ctx, list(range(70)), reqs)
    rev = _batch(ctx, list(range(69, -1, -1)), reqs)
    ctx.close()
    assert [r["status"] for r in fwd] == [O.MOI_LOCALLY_SOLVED] * 70
    assert [r["status"] for r in rev] == [O.MOI_LOCALLY_SOLVED] * 70
    for k in (0, 1, 63, 64, 69):
        _same(fwd[k], rev[k], ("order", k))
    for k in (0, 37, 64, 69):
        rs = _scalar(S, reqs[k])
        _same(fwd[k], rs, ("identity", k))
        _same(rev[k], rs, ("reversed", k))


# ------------------------------------------------------------------ 6: merit batch
def test_merit_batch_equals_the_scalar_calls():
    lay0, lays, reqs = _contingency_requests("case14", 4, CASE14_PLAN, seed=6)
    S = _lay_struct(lay0)
    rng = np.random.default_rng(6)
    n, m = lay0.n, lay0.m
    ops = []
    for k in range(4):
        _, x, _, _, df, E, jv, hv = reqs[k]
        ops.append(dict(x=x + 0.05 * rng.standard_normal(n), E=E + 0.1 * rng.standard_normal(m), df=df, jv=jv, hv=hv,
                        lam=rng.standard_normal(m), mxU=-np.abs(rng.standard_normal(n)), mxL=np.abs(rng.standard_normal(n)),
                        p=0.1 * rng.standard_normal(n), mu=float(1.0 + 10 * rng.random()), f=float(rng.standard_normal()),
                        muv=np.abs(rng.standard_normal(m)) + 0.5, slack=np.abs(rng.standard_normal(2 * m))))
    col = lambda key: [o[key] for o in ops]
    inst = [2, 0, 3, 1]
    ctx = _ctx(S, batch=4)
    for k in range(4):
        ctx.set_bounds(inst[k], lays[k])
    got = {}
    for pn in (1, 2, "inf"):
        got["nv", pn] = ctx.norm_violations_batch(inst, col("E"), col("x"), pn)
        got["nc", pn] = ctx.norm_complementarity_batch(inst, col("E"), col("lam"), pn)
    got["kt"] = ctx.kt_residuals_batch(inst, col("df"), col("lam"), col("mxU"), col("mxL"), col("jv"))
    for fr in (0, 1):
        got["phi", fr] = ctx.compute_phi_batch(inst, col("f"), col("E"), col("x"), col("mu"), fr)
        got["qm", fr] = ctx.compute_qmodel_batch(inst, col("x"), col("p"), col("df"), col("E"), col("jv"), col("hv"), col("mu"), fr)
        for vec in (0, 1):
            got["dd", fr, vec] = ctx.compute_derivative_full_batch(inst, col("df"), col("p"), col("E"), col("mu"),
                                                                   col("muv") if vec else None, fr, col("slack"))
    ctx.close()
    for k, o in enumerate(ops):
        c1 = _ctx(S, _lay_struct(lays[k]), 1)
        want = {}
        for pn in (1, 2, "inf"):
            want["nv", pn] = c1.norm_violations(o["E"], o["x"], pn)
            want["nc", pn] = c1.norm_complementarity(o["E"], o["lam"], pn)
        want["kt"] = c1.kt_residuals(o["df"], o["lam"], o["mxU"], o["mxL"], o["jv"])
        for fr in (0, 1):
            want["phi", fr] = c1.compute_phi(o["f"], o["E"], o["x"], o["mu"], fr)
            want["qm", fr] = c1.compute_qmodel(o["x"], o["p"], o["df"], o["E"], o["jv"], o["hv"], o["mu"], fr)
            for vec in (0, 1):
                want["dd", fr, vec] = c1.compute_derivative_full(o["df"], o["p"], o["E"], o["mu"], o["muv"] if vec else None,
                                                                 fr, o["slack"])
        c1.close()
        for key, v in want.items():
            assert got[key][k] == v, (key, k, got[key][k], v)
    assert len(set(got["nv", 1])) == 4 and len(set(got["qm", 1])) == 4


# ------------------------------------------------------------------ 7: warm start
def test_warm_start_per_instance():
    """options.ipm_warm_start: two consecutive batch calls on the same instances equal two consecutive scalar calls per
    instance on one-instance contexts."""
    P = O.problem_hs071(); S = P.structure()
    rng = np.random.default_rng(7)

    def req(mode, delta):
        x = np.clip(P.x0 + 0.2 * rng.standard_normal(S["n"]), S["xL"], S["xU"])
        return _request(P, S, x, rng.standard_normal(S["m"]), mode, delta, 7.0)
    modes = [(O.MODE_QP, 10.0), (O.MODE_L1QP, 0.5), (O.MODE_QP, 0.5)]
    a = [req(*md) for md in modes]; b = [req(*md) for md in modes]
    inst = [3, 0, 2]
    ctx = _ctx(S, batch=4, ipm_warm_start=1)
    ra = _batch(ctx, inst, a); rb = _batch(ctx, inst, b)
    ctx.close()
    cold = 0
    for k in range(3):
        c1 = _ctx(S, None, 1, ipm_warm_start=1)
        sa = c1.qp_solve(*a[k]); sb = c1.qp_solve(*b[k])
        c1.close()
        _same(ra[k], sa, ("first call", k))
        _same(rb[k], sb, ("second call", k))
        sc = _scalar(S, b[k])
        cold += int(sb["ipm_iters"] != sc["ipm_iters"] or any(not np.array_equal(sb[key], sc[key]) for key in VEC))
    assert cold > 0          # the warm start took part: a second call differs from a cold solve of the same request


# ------------------------------------------------------------------ 8: whole solves in lockstep
def _models(name, starts, max_iter=200):
    P = getattr(O, "problem_" + name)(); S = P.structure()
    out = []
    for x0 in starts(P, S):
        mdl = HM.Model(S["n"], S["m"], S["xL"], S["xU"], S["gL"], S["gU"],
                       list(zip(S["jrow"].tolist(), S["jcol"].tolist())), list(zip(S["hrow"].tolist(), S["hcol"].tolist())),
                       P.eval_f, P.eval_g, P.eval_grad_f, P.eval_jac_g, P.eval_h, S["num_linear"],
                       HM.Parameters(max_iter=max_iter))
        mdl.x[:] = x0
        out.append(mdl)
    return out


def _starts(P, S):
    rng = np.random.default_rng(8)
    lo, hi = np.maximum(S["xL"], -1e3), np.minimum(S["xU"], 1e3)
    return [np.clip(P.x0 + (0.4 * k) * rng.standard_normal(S["n"]), lo, hi) for k in range(4)]


@pytest.mark.parametrize("name", ["hs071", "toy"])
def test_whole_solves_in_lockstep(name):
    """Four models from four starts, one context of four instances, one batch call per round and kind of request: final point,
    multipliers, status, iteration count and the trace of every iteration (radius, step norm, merit, infeasibilities,
    sub-problem status) equal four independent runs over the scalar seat."""
    lock, calls = HMB.run_lockstep(_models(name, _starts))
    lock[0].ctx.close()
    solo = _models(name, _starts)
    n_scalar = 0
    for k, mdl in enumerate(solo):
        s = HM.optimize(mdl)
        s.ctx.close()
        b = lock[k]
        assert b.problem.status == mdl.status and b.iter == s.iter, (k, b.problem.status, mdl.status)
        for key in ("x", "g", "mult_g", "mult_x_L", "mult_x_U"):
            assert np.array_equal(getattr(b.problem, key), getattr(mdl, key)), (k, key)
        assert b.problem.obj_val == mdl.obj_val
        assert b.trace == s.trace, k
        n_scalar += sum(1 for _ in s.trace)
    assert any(m_.status == 0 for m_ in solo)
    # the rounds were shared: fewer sub-problem calls than sub-problems solved
    assert calls["qp"] < n_scalar
