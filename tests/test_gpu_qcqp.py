"""The general sparse QCQP in the batched device SQP loop (sqphip_qcqp_attach / _set_instance, csrc/qcqp_dev.hpp): the
device evaluator against the numpy reference and against the dedicated ACR / ACWR evaluators, batched runs against the
oracle (which runs on the same data through ctypes callbacks, tests/qcqp_ref.py), the generic path against the dedicated
ACR path on contingency scenarios, known optima, determinism and misuse."""
import dataclasses
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import sqpsolver_jl_amd as pkg                                        # noqa: E402
from sqpsolver_jl_amd.acopf_synth import acopf_synth, acr_layout, acwr_layout, contingency, CASES   # noqa: E402
from sqpsolver_jl_amd.qcqp import make_qcqp, qcqp_layout, qcqp_scenario, qcqp_synth   # noqa: E402
from oracle import oracle as O                                        # noqa: E402
from qcqp_ref import OracleQcqp, QcqpRef, coo_sum, extract           # noqa: E402
from hs_qps import HS_QPS                                             # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-8
SQP_KW = dict(tol_infeas=1e-6, tol_residual=1e-4)


# ---- copied from tests/test_gpu_parity.py (a test module is not imported)
def rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(1.0, np.abs(np.asarray(b)).max()))


def _same_decisions(ro, tr):
    return [(a["iter"], a["accepted"], a["fr"], a["sub_status"]) for a in ro["trace"]] == \
           [(t["iter"], t["accepted"], t["fr"], t["sub_status"]) for t in tr]


def _ipm_counts_close(ro, tr):
    return all(abs(a["ipm_iters"] - t["ipm_iters"]) <= max(2, (0.5 if t["fr"] else 0.25) * a["ipm_iters"])
               for a, t in zip(ro["trace"], tr))


# ---- helpers
def _ctx(lay, batch, **kw):
    return pkg.Context(lay.n, lay.m, lay.num_linear, lay.jrow, lay.jcol, lay.hrow, lay.hcol, lay.xL, lay.xU, lay.gL, lay.gU,
                       pkg.default_options(**kw), batch=batch)


def _net(case, s=5):
    nb, ng, nl, seed = CASES[case.split("-")[0]]
    base = acopf_synth(nb, ng, nl, seed)
    net = base if s == 0 else contingency(base, s, seed)
    rng = np.random.default_rng(seed)
    if "taps" in case:
        tr = rng.random(net.nl) < 0.33
        net = dataclasses.replace(net, tap=np.where(tr, rng.uniform(0.93, 1.07, net.nl), 1.0),
                                  shift=np.where(tr & (rng.random(net.nl) < 0.3), rng.uniform(-0.08, 0.08, net.nl), 0.0))
    if "shunts" in case:
        net = dataclasses.replace(net, gs=np.where(rng.random(net.nb) < 0.3, rng.uniform(0, 0.03, net.nb), 0.0),
                                  bs=np.where(rng.random(net.nb) < 0.4, rng.uniform(-0.05, 0.19, net.nb), 0.0))
    return net


def _qcqp_ctx(q, lay, batch, qs=None, **kw):
    ctx = _ctx(lay, batch, **kw)
    ctx.qcqp_attach(q)
    for b in range(batch):
        ctx.qcqp_set_instance(b, (qs or [q] * batch)[b])
    return ctx


def _results(ctx, b):
    return ctx.sqp_get(b), ctx.sqp_trace(b)


# ---- 1. evaluator parity
@pytest.mark.parametrize("case", ["case14-acr-taps-shunts", "case14-acwr"])
def test_evaluator_matches_reference_and_dedicated_evaluators(case):
    net = _net(case)
    lay = acwr_layout(net) if "acwr" in case else acr_layout(net)
    q = extract(O.problem_acopf(net, lay))
    cq = _ctx(lay, 2); cq.qcqp_attach(q); cq.qcqp_set_instance(1, q)
    cd = _ctx(lay, 2); cd.acopf_attach(net, lay); cd.acopf_set_instance(1, net, lay)
    R = QcqpRef(q)
    rng = np.random.default_rng(2)
    x = lay.x0 + 0.05 * rng.standard_normal(lay.n); lam = rng.standard_normal(lay.m)
    eq, ed = cq.acopf_eval(1, x, 0.7, lam), cd.acopf_eval(1, x, 0.7, lam)
    J = lambda v: coo_sum(v, lay.jrow, lay.jcol, lay.n)
    H = lambda v: coo_sum(v, lay.hrow, lay.hcol, lay.n, lower=True)
    for want in (dict(f=R.f(x), grad=R.grad(x), g=R.g(x), jval=R.jac(x, lay.jrow, lay.jcol), hval=R.hess(0.7, lam, lay.hrow, lay.hcol)), ed):
        assert abs(eq["f"] - want["f"]) <= 1e-13 * max(1.0, abs(want["f"]))
        assert rel(eq["grad"], want["grad"]) < 1e-13 and rel(eq["g"], want["g"]) < 1e-13
        assert rel(J(eq["jval"]), J(want["jval"])) < 1e-13 and rel(H(eq["hval"]), H(want["hval"])) < 1e-13
    cq.close(); cd.close()


def test_evaluator_on_a_synthetic_qcqp_with_per_instance_values():
    q = qcqp_synth(24, 14, seed=5)
    lay = qcqp_layout(q)
    qs = [qcqp_scenario(q, s, 5) for s in range(3)]
    ctx = _qcqp_ctx(q, lay, 3, qs)
    rng = np.random.default_rng(3)
    x = q.x0 + 0.3 * rng.standard_normal(q.n); lam = rng.standard_normal(q.m)
    for b in range(3):
        R, ev = QcqpRef(qs[b]), ctx.acopf_eval(b, x, 1.3, lam)
        assert abs(ev["f"] - R.f(x)) <= 1e-13 * max(1.0, abs(R.f(x)))
        assert rel(ev["grad"], R.grad(x)) < 1e-13 and rel(ev["g"], R.g(x)) < 1e-13
        assert rel(ev["jval"], R.jac(x, lay.jrow, lay.jcol)) < 1e-13
        assert rel(ev["hval"], R.hess(1.3, lam, lay.hrow, lay.hcol)) < 1e-13
    # a NULL part keeps what the instance had
    ctx.qcqp_set_instance(2, c=np.zeros(q.n))
    ev = ctx.acopf_eval(2, x, 1.3, lam)
    assert rel(ev["g"], QcqpRef(qs[2]).g(x)) < 1e-13
    assert rel(ev["grad"], QcqpRef(dataclasses.replace(qs[2], c=np.zeros(q.n))).grad(x)) < 1e-13
    ctx.close()


# ---- 2. batched run against the oracle
@pytest.mark.parametrize("kkt_mode,literal_quirks", [(2, 0), (2, 1), (1, 0), (1, 1)])
def test_batched_run_matches_oracle(kkt_mode, literal_quirks):
    q = qcqp_synth(24, 14, seed=5)
    lay = qcqp_layout(q)
    qs = [qcqp_scenario(q, s, 5) for s in range(4)]
    kw = dict(max_iter=8 if literal_quirks else 30, literal_quirks=literal_quirks, **SQP_KW)
    ctx = _qcqp_ctx(q, lay, 4, qs, kkt_mode=kkt_mode, **kw)
    ctx.sqp_reset(); ctx.sqp_run(0)
    lin = dict(kkt_mode=2) if kkt_mode == 2 else dict(kkt_mode=1, kkt_tile_order=1)
    try:
        for b in range(4):
            ro = O.sqp_solve(OracleQcqp(qs[b], lay), O.default_options(**lin, **kw))
            rg, tr = _results(ctx, b)
            assert (rg["status"], rg["iter"]) == (ro["status"], ro["iter"]), b
            assert _same_decisions(ro, tr) and _ipm_counts_close(ro, tr), b
            assert rel(rg["x"], ro["x"]) < TOL and abs(rg["obj_val"] - ro["obj_val"]) <= TOL * max(1.0, abs(ro["obj_val"])), b
    finally:
        O.set_kkt_order(None)
    ctx.close()


# ---- 3. generic path = dedicated path
def test_generic_path_equals_dedicated_acr_path_on_contingencies():
    nets = [_net("case118-taps-shunts", s) for s in range(8)]
    lays = [acr_layout(nt) for nt in nets]
    qs = extract([O.problem_acopf(nt, ly) for nt, ly in zip(nets, lays)])
    kw = dict(max_iter=60, use_soc=1, literal_quirks=0, **SQP_KW)
    cg = _ctx(lays[0], 8, **kw); cg.qcqp_attach(qs[0])
    cd = _ctx(lays[0], 8, **kw); cd.acopf_attach(nets[0], lays[0])
    for b in range(8):
        cg.qcqp_set_instance(b, qs[b]); cd.acopf_set_instance(b, nets[b], lays[b])
    for c in (cg, cd):
        c.sqp_reset(); c.sqp_run(0)
    assert np.array_equal(cg.sqp_status()[0], cd.sqp_status()[0]) and np.array_equal(cg.sqp_status()[1], cd.sqp_status()[1])
    for b in range(8):
        (rg, tg), (rd, td) = _results(cg, b), _results(cd, b)
        assert (rg["status"], rg["iter"]) == (rd["status"], rd["iter"]), b
        assert [(t["iter"], t["accepted"], t["fr"], t["sub_status"]) for t in tg] == \
               [(t["iter"], t["accepted"], t["fr"], t["sub_status"]) for t in td], b
        assert rel(rg["x"], rd["x"]) < TOL, b
    cg.close(); cd.close()


def test_generic_path_equals_dedicated_acwr_path():
    net = _net("case14-acwr", 3)
    lay = acwr_layout(net)
    q = extract(O.problem_acopf(net, lay))
    kw = dict(max_iter=60, use_soc=1, literal_quirks=0, **SQP_KW)
    cg = _ctx(lay, 1, **kw); cg.qcqp_attach(q); cg.qcqp_set_instance(0, q)
    cd = _ctx(lay, 1, **kw); cd.acopf_attach(net, lay); cd.acopf_set_instance(0, net, lay)
    for c in (cg, cd):
        c.sqp_reset(); c.sqp_run(0)
    (rg, tg), (rd, td) = _results(cg, 0), _results(cd, 0)
    assert (rg["status"], rg["iter"]) == (rd["status"], rd["iter"])
    assert [(t["iter"], t["accepted"], t["fr"], t["sub_status"]) for t in tg] == \
           [(t["iter"], t["accepted"], t["fr"], t["sub_status"]) for t in td]
    assert rel(rg["x"], rd["x"]) < TOL
    cg.close(); cd.close()


# ---- 4. known optima
def _solve_known(q, max_iter=60):
    """Both solvers with the textbook Hessian sign (literal_quirks = 0): with the reference's sign the sub-problems of a
    convex constraint are non-convex and the disc ends at the iteration limit (status 6) a few 1e-6 from its optimum."""
    lay = qcqp_layout(q)
    kw = dict(max_iter=max_iter, literal_quirks=0, **SQP_KW)
    ctx = _qcqp_ctx(q, lay, 1, **kw)
    ctx.sqp_reset(); ctx.sqp_run(0)
    rg = ctx.sqp_get(0)
    ctx.close()
    ro = O.sqp_solve(OracleQcqp(q, lay), O.default_options(kkt_mode=2, **kw))
    return rg, ro


def test_known_optimum_of_a_disc():
    """min x + y  s.t.  x^2 + y^2 <= 1  ->  (-1/sqrt 2, -1/sqrt 2)"""
    q = make_qcqp(2, 1, 0, Q=([1, 1], [1, 2], [1, 2], [2.0, 2.0]), c=[1.0, 1.0], gU=[1.0], xL=[-5.0, -5.0], xU=[5.0, 5.0],
                  x0=[0.1, 0.2])
    rg, ro = _solve_known(q)
    assert rg["status"] == ro["status"] == 0
    assert np.abs(rg["x"] - [-2 ** -0.5, -2 ** -0.5]).max() <= 1e-6 and abs(rg["obj_val"] + 2 ** 0.5) <= 1e-6


@pytest.mark.parametrize("name", ["hs035", "hs076"])
def test_known_optima_of_hock_schittkowski_qps(name):
    h = HS_QPS[name]
    Hl = np.tril(h["H"]); r, c = np.nonzero(Hl)
    ar, ac = np.nonzero(h["A"])
    n, m = len(h["c"]), len(h["gL"])
    q = make_qcqp(n, m, m, Q0=(r + 1, c + 1, Hl[r, c]), A=(ar + 1, ac + 1, h["A"][ar, ac]), c=h["c"], f0=h["f0"],
                  xL=h["xL"], xU=h["xU"], gL=h["gL"], gU=h["gU"], x0=np.full(n, 0.5))
    rg, ro = _solve_known(q)
    assert rg["status"] == ro["status"] == 0
    assert np.abs(rg["x"] - h["x"]).max() <= 1e-6 and abs(rg["obj_val"] - h["f"]) <= 1e-6


def test_infeasible_qcqp_returns_the_oracles_code():
    """x^2 + y^2 <= 1 with x >= 2"""
    q = make_qcqp(2, 1, 0, Q=([1, 1], [1, 2], [1, 2], [2.0, 2.0]), c=[1.0, 1.0], gU=[1.0], xL=[2.0, -5.0], xU=[5.0, 5.0],
                  x0=[2.0, 0.0])
    rg, ro = _solve_known(q, max_iter=30)
    assert rg["status"] == ro["status"] and rg["status"] != 0


# ---- 5. determinism
def test_same_instance_in_two_slots_and_two_runs_is_bit_identical():
    q = qcqp_synth(24, 14, seed=5)
    lay = qcqp_layout(q)
    qs = [qcqp_scenario(q, s, 5) for s in (1, 2, 3, 4, 5, 1)]           # slots 0 and 5: the same instance
    ctx = _qcqp_ctx(q, lay, 6, qs, max_iter=30, **SQP_KW)
    outs = []
    for _ in range(2):
        ctx.sqp_reset(); ctx.sqp_run(0)
        outs.append([(ctx.sqp_get(b), ctx.sqp_trace(b)) for b in (0, 5)])
    ctx.close()
    ref = outs[0][0]
    for rg, tr in outs[0][1:] + outs[1]:
        for k in ("x", "g", "mult_g", "mult_x_L", "mult_x_U"):
            assert np.array_equal(rg[k], ref[0][k]), k
        assert (rg["obj_val"], rg["status"], rg["iter"]) == (ref[0]["obj_val"], ref[0]["status"], ref[0]["iter"])
        assert tr == ref[1]


# ---- 6. misuse
def _expect(rc, code, words, ctx):
    assert rc == code, rc
    msg = ctx.L.sqphip_last_error(ctx.h).decode()
    assert all(w in msg for w in words), msg


def _attach_rc(ctx, q):
    try:
        ctx.qcqp_attach(q)
        return 0
    except pkg.SqpHipError as e:
        return int(str(e).split("error ")[1].split(":")[0])


def test_misuse_is_refused_with_a_message():
    q = qcqp_synth(16, 10, seed=2)
    lay = qcqp_layout(q)
    EINVAL, ESTATE = -1, -4
    # a Jacobian slot missing (one of a Q term's)
    k = int(np.flatnonzero((lay.jrow == q.qi[0]) & (lay.jcol == q.qr[0]))[0])
    short = dataclasses.replace(lay, jrow=np.delete(lay.jrow, k), jcol=np.delete(lay.jcol, k))
    ctx = _ctx(short, 1); _expect(_attach_rc(ctx, q), EINVAL, ["Q term 1", "Jacobian"], ctx); ctx.close()
    # a Hessian slot missing
    short = dataclasses.replace(lay, hrow=lay.hrow[1:], hcol=lay.hcol[1:])
    ctx = _ctx(short, 1); _expect(_attach_rc(ctx, q), EINVAL, ["Hessian"], ctx); ctx.close()
    # a quadratic term in a linear row
    lin = dataclasses.replace(lay, num_linear=int(q.qi.min()))
    ctx = _ctx(lin, 1); _expect(_attach_rc(ctx, q), EINVAL, ["Q term 1", "linear"], ctx); ctx.close()
    # an index out of range
    bad = dataclasses.replace(q, ac=q.ac.copy()); bad.ac[2] = q.n + 1
    ctx = _ctx(lay, 1); _expect(_attach_rc(ctx, bad), EINVAL, ["A term 3", "out of range"], ctx)
    # the refused attach left the context unattached: a good one goes in, a second one is refused
    ctx.qcqp_attach(q)
    _expect(_attach_rc(ctx, q), ESTATE, ["already"], ctx)
    # the ACOPF-only entry points on a QCQP context
    L = ctx.L
    _expect(L.sqphip_acopf_set_instance(ctx.h, 0, None, None, None, None), EINVAL, ["QCQP"], ctx)
    _expect(L.sqphip_acopf_set_shunts(ctx.h, 0, None, None, None), EINVAL, ["QCQP"], ctx)
    _expect(L.sqphip_acopf_set_dclines(ctx.h, 0, None), EINVAL, ["QCQP"], ctx)
    _expect(L.sqphip_sqp_stream_begin(ctx.h, 4), EINVAL, ["QCQP"], ctx)
    ctx.close()
