"""Variables shared across the factors of a term and the kinds SQRT .. POWR in the batched device SQP loop
(sqphip_nlp_attach_general, csrc/nlp_dev.hpp): the device evaluator against the ordered-pair numpy reference
(tests/nlp_general_ref.py) on hand-made and generated models and at saturated arguments, models of the old class through all
three entry points bit for bit, generated batches against the oracle, three models with known answers, determinism, the
scenario queue against the batch, the Armijo probe and the refusals.  tests/test_nlp_general_cpu.py holds the oracle's word
for the generated instances.

Evaluator tolerance: 1e-13 relative to the largest entry, the one of tests/test_gpu_nlp_affine.py, for every kind."""
import dataclasses
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import sqpsolver_jl_amd as pkg                                        # noqa: E402
from sqpsolver_jl_amd.nlp_terms import (LOG, POW, POWR, SIN, cobb_douglas_model, entropy_model, logistic_model,   # noqa: E402
                                        make_nlp_terms, needs_general, nlp_affine_synth, nlp_general_synth, nlp_terms_args,
                                        nlp_terms_layout, nlp_terms_scenario, nlp_terms_synth)
from oracle import oracle as O                                        # noqa: E402
from nlp_general_ref import (NEW_KINDS, QUEUE_NOISE, QUEUE_SCENARIOS, SATURATION_SHIFTS, SQP_KW, NlpGeneralRef,   # noqa: E402
                             OracleGeneralTerms, general_edge_model, gpu_model, gpu_scenarios, saturation_model)
from qcqp_ref import coo_sum                                          # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-8                                                            # points and objective against the oracle (tests/test_gpu_nlp_affine.py)
EVAL_TOL = 1e-13                                                      # _check_eval of tests/test_gpu_nlp_affine.py
EINVAL, ESTATE = -1, -4
FULL = ("x", "g", "mult_g", "mult_x_L", "mult_x_U")


# ---- helpers (tests/test_gpu_nlp_affine.py; a test module is not imported)
def rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(1.0, np.abs(np.asarray(b)).max()))


def _decisions(tr):
    return [(t["iter"], t["accepted"], t["fr"], t["sub_status"]) for t in tr]


def _ipm_counts_close(ro, tr):
    return all(abs(a["ipm_iters"] - t["ipm_iters"]) <= max(2, (0.5 if t["fr"] else 0.25) * a["ipm_iters"])
               for a, t in zip(ro["trace"], tr))


def _ctx(lay, batch, **kw):
    return pkg.Context(lay.n, lay.m, lay.num_linear, lay.jrow, lay.jcol, lay.hrow, lay.hcol, lay.xL, lay.xU, lay.gL, lay.gU,
                       pkg.default_options(**kw), batch=batch)


def _nlp_ctx(p, lay, batch, ps=None, general=None, **kw):
    ctx = _ctx(lay, batch, **kw)
    ctx.nlp_attach(p, general=general)
    for b in range(batch):
        ctx.nlp_set_instance(b, (ps or [p] * batch)[b])
    return ctx


def _lin(kkt_mode):
    return dict(kkt_mode=2) if kkt_mode == 2 else dict(kkt_mode=1, kkt_tile_order=1)


def _check_eval(ev, R, x, sigma, lam, lay, tol=EVAL_TOL, summed=False):
    J = (lambda v: coo_sum(v, lay.jrow, lay.jcol, lay.n)) if summed else (lambda v: v)
    H = (lambda v: coo_sum(v, lay.hrow, lay.hcol, lay.n, lower=True)) if summed else (lambda v: v)
    want = dict(f=R.f(x), grad=R.grad(x), g=R.g(x), jval=J(R.jac(x, lay.jrow, lay.jcol)), hval=H(R.hess(x, sigma, lam, lay.hrow, lay.hcol)))
    got = dict(ev, jval=J(ev["jval"]), hval=H(ev["hval"]))
    err = {k: rel(got[k], want[k]) for k in want}
    print("evaluator errors", err)
    assert all(np.all(np.isfinite(np.asarray(got[k]))) for k in want)
    assert all(e <= tol for e in err.values()), err


def _as_affine(q):
    """the one-argument model q with argument arrays"""
    aptr, avar, acoef = nlp_terms_args(q)
    return dataclasses.replace(q, aptr=aptr.copy(), avar=avar.copy(), acoef=acoef.copy())


# ---- 1. plan edges, evaluator only
def test_evaluator_at_the_plan_edges():
    p, lay = general_edge_model()
    assert needs_general(p) and np.diff(p.tptr).max() == 8 and np.diff(p.aptr)[:8].tolist() == [8, 1, 2, 3, 2, 2, 2, 2]
    assert set(NEW_KINDS) <= set(p.fkind.tolist())
    p1 = dataclasses.replace(p, tcoef=p.tcoef * np.array([1.2, 0.8, -1.0, 0.5, 1.5, -0.7, 2.0, 0.9]), g0=p.g0 + 0.1, f0=-0.5)
    ctx = _nlp_ctx(p, lay, 2, [p, p1])
    rng = np.random.default_rng(8)
    lam = rng.standard_normal(p.m)
    pairs = set(zip(lay.hrow.tolist(), lay.hcol.tolist()))
    assert {(1, 1), (9, 9), (10, 10), (11, 10), (11, 11), (23, 23), (26, 26), (27, 27), (28, 27)} <= pairs
    for b, (q, x) in enumerate(((p, rng.uniform(0.5, 1.6, p.n)), (p1, rng.uniform(0.4, 2.0, p.n)))):
        ev = ctx.acopf_eval(b, x, 1.3, lam)
        _check_eval(ev, NlpGeneralRef(q), x, 1.3, lam, lay)
        _check_eval(ev, NlpGeneralRef(q), x, 1.3, lam, lay, summed=True)
        assert ev["jval"][-1] == 0.0 and ev["hval"][-2] == 0.0 and ev["hval"][-1] == 0.0     # unused slots, the copy of a slot
        assert ev["grad"][29] != 0.0 and ev["hval"][0] != 0.0                                # variable 30; the slot (1, 1) of 64 entries
    ctx.close()


# ---- 2. beyond one stride of the thread loops
def test_evaluator_beyond_one_stride_of_the_thread_loops():
    p = nlp_general_synth(600, 500, seed=2)
    lay = nlp_terms_layout(p)
    assert len(p.trow) > 1024 and len(lay.jrow) > 1024 and len(p.fkind) > 2048 and len(p.avar) > 4096 and needs_general(p)
    ctx = _nlp_ctx(p, lay, 1)
    rng = np.random.default_rng(5)
    x = np.clip(p.x0 + 0.2 * rng.standard_normal(p.n), 0.25, 2.9); lam = rng.standard_normal(p.m)
    _check_eval(ctx.acopf_eval(0, x, 1.3, lam), NlpGeneralRef(p), x, 1.3, lam, lay)
    ctx.close()


# ---- 3. saturation
def test_saturated_factors_stay_finite_and_equal_the_reference():
    p, lay = saturation_model()
    assert sorted(set(np.abs(p.fshift[p.fkind != POW]).tolist())) == [40.0, 750.0] and SATURATION_SHIFTS == (40.0, -40.0, 750.0, -750.0)
    ctx = _nlp_ctx(p, lay, 1)
    R = NlpGeneralRef(p)
    lam = np.array([0.7])
    for x in (p.x0, np.array([0.2, 3.0, 0.2, 3.0]), np.array([3.0, 0.2, 3.0, 0.2])):
        ev = ctx.acopf_eval(0, x, 1.3, lam)
        for k in ("f", "grad", "g", "jval", "hval"):
            assert np.all(np.isfinite(np.asarray(ev[k]))), k
        _check_eval(ev, R, x, 1.3, lam, lay)
    assert ev["g"][0] > 700.0                                                                # (softplus at 750 took part)
    ctx.close()


# ---- 4. the old class: all entry points file the same bits
@pytest.mark.parametrize("model", ["one_argument", "affine"])
def test_a_model_of_the_old_class_files_the_same_bits_through_every_entry_point(model):
    if model == "one_argument":
        q = nlp_terms_synth(24, 14, seed=5)
        qs = [nlp_terms_scenario(q, s, 5) for s in range(3)]
        routes = [(lambda m: m, None), (_as_affine, None), (lambda m: m, True)]              # sqphip_nlp_attach, _affine, _general
    else:
        q = nlp_affine_synth(24, 14, seed=1)
        qs = [nlp_terms_scenario(q, s, 1) for s in range(3)]
        routes = [(lambda m: m, None), (lambda m: m, True)]                                  # sqphip_nlp_attach_affine, _general
    assert not needs_general(q)
    lay = nlp_terms_layout(q)
    ctxs = [_nlp_ctx(f(q), lay, 3, [f(s) for s in qs], general=g, **SQP_KW) for f, g in routes]
    rng = np.random.default_rng(3)
    x = np.clip(q.x0 + 0.3 * rng.standard_normal(q.n), 0.25, 2.9); lam = rng.standard_normal(q.m)
    for b in range(3):
        evs = [c.acopf_eval(b, x, 1.3, lam) for c in ctxs]
        for ev in evs[1:]:
            for k in ("f", "grad", "g", "jval", "hval"):
                assert np.array_equal(np.asarray(evs[0][k]), np.asarray(ev[k])), (b, k)
    for c in ctxs:
        c.sqp_reset(); c.sqp_run(0)
    for b in range(3):
        ro = ctxs[0].sqp_get(b)
        assert ro["status"] == 0
        for c in ctxs[1:]:
            ra = c.sqp_get(b)
            for k in FULL:
                assert np.array_equal(ro[k], ra[k]), (b, k)
            assert (ro["obj_val"], ro["status"], ro["iter"]) == (ra["obj_val"], ra["status"], ra["iter"]), b
            assert ctxs[0].sqp_trace(b) == c.sqp_trace(b), b
    for c in ctxs:
        c.close()


# ---- 5. a generated batch against the oracle
@pytest.mark.parametrize("kkt_mode", [2, 1])
def test_generated_batch_matches_oracle(kkt_mode):
    p, lay = gpu_model()
    ps = gpu_scenarios(p)
    assert needs_general(p)
    ctx = _nlp_ctx(p, lay, 4, ps, kkt_mode=kkt_mode, **SQP_KW)
    ctx.sqp_reset(); ctx.sqp_run(0)
    try:
        for b in range(4):
            ro = O.sqp_solve(OracleGeneralTerms(ps[b], lay), O.default_options(**_lin(kkt_mode), **SQP_KW))
            assert ro["status"] == 0
            rg, tr = ctx.sqp_get(b), ctx.sqp_trace(b)
            print("instance", b, "status", rg["status"], ro["status"], "iter", rg["iter"], ro["iter"], "x", rel(rg["x"], ro["x"]),
                  "obj", abs(rg["obj_val"] - ro["obj_val"]))
            assert (rg["status"], rg["iter"]) == (ro["status"], ro["iter"]), b
            assert _decisions(ro["trace"]) == _decisions(tr) and _ipm_counts_close(ro, tr), b
            assert rel(rg["x"], ro["x"]) < TOL and abs(rg["obj_val"] - ro["obj_val"]) <= TOL * max(1.0, abs(ro["obj_val"])), b
    finally:
        O.set_kkt_order(None)
    ctx.close()


# ---- 6. known answers
def _solve(p):
    lay = nlp_terms_layout(p)
    ctx = _nlp_ctx(p, lay, 1, max_iter=60, literal_quirks=0, tol_infeas=1e-8, tol_residual=1e-8)
    ctx.sqp_reset(); ctx.sqp_run(0)
    r = ctx.sqp_get(0)
    ctx.close()
    print("status", r["status"], "iter", r["iter"], "x", r["x"])
    assert r["status"] == 0
    return r["x"]


def test_entropy_and_cobb_douglas_reach_their_closed_forms():
    c = np.array([0.3, -0.5, 1.2, 0.0, 0.8, -1.0])
    assert np.abs(_solve(entropy_model(c)) - np.exp(-c) / np.exp(-c).sum()).max() <= 1e-6
    alpha, prices, wealth = np.array([0.2, 0.3, 0.4]), np.array([1.0, 2.0, 0.5]), 10.0
    assert np.abs(_solve(cobb_douglas_model(alpha, prices, wealth)) - alpha * wealth / (prices * alpha.sum())).max() <= 1e-6


def test_logistic_regression_matches_scipy():
    import scipy.optimize
    rng = np.random.default_rng(4)
    X = np.c_[np.ones(12), rng.standard_normal((12, 2))]
    y = (X @ np.array([0.3, 1.0, -0.7]) + 0.5 * rng.standard_normal(12) > 0).astype(float)
    reg = 0.5
    loss = lambda w: float(np.sum(np.logaddexp(0.0, X @ w) - y * (X @ w)) + 0.5 * reg * (w @ w))
    want = scipy.optimize.minimize(loss, np.zeros(3), method="BFGS", options=dict(gtol=1e-10)).x
    assert np.abs(_solve(logistic_model(X, y, reg)) - want).max() <= 1e-6


# ---- 7. determinism and the scenario queue
def test_same_instance_in_two_slots_and_two_runs_is_bit_identical():
    p, lay = gpu_model()
    ps = gpu_scenarios(p, (1, 2, 1))                                        # slots 0 and 2: the same instance
    ctx = _nlp_ctx(p, lay, 3, ps, **SQP_KW)
    outs = []
    for _ in range(2):
        ctx.sqp_reset(); ctx.sqp_run(0)
        outs.append([(ctx.sqp_get(b), ctx.sqp_trace(b)) for b in (0, 2)])
    ctx.close()
    ref = outs[0][0]
    assert ref[0]["status"] == 0
    for rg, tr in outs[0][1:] + outs[1]:
        for k in FULL:
            assert np.array_equal(rg[k], ref[0][k]), k
        assert (rg["obj_val"], rg["status"], rg["iter"]) == (ref[0]["obj_val"], ref[0]["status"], ref[0]["iter"])
        assert tr == ref[1]


def test_queue_files_the_bits_of_the_batch_with_multipliers():
    p, lay = gpu_model()
    ps = gpu_scenarios(p, QUEUE_SCENARIOS, QUEUE_NOISE)
    M = len(ps)
    assert M == 6
    cb = _nlp_ctx(p, lay, M, ps, kkt_mode=2, **SQP_KW)
    cb.sqp_reset(); cb.sqp_run(0)
    ref = [cb.sqp_get(b) for b in range(M)]
    cb.close()
    ctx = _ctx(lay, 2, kkt_mode=2, **SQP_KW)
    ctx.nlp_attach(p)
    ctx.nlp_stream_begin(M, keep_multipliers=True)
    for s in range(M):
        ctx.nlp_stream_set(s, ps[s])
    ctx.stream_run()
    for s in range(M):
        r = ctx.stream_get_full(s)
        print("scenario", s, "status", r["status"], "iter", r["iter"], "batch", ref[s]["iter"])
        assert r["status"] == 0, s
        for k in FULL:
            assert np.array_equal(r[k], ref[s][k]), (s, k)
        assert (r["obj_val"], r["status"], r["iter"]) == (ref[s]["obj_val"], ref[s]["status"], ref[s]["iter"]), s
    assert any(np.abs(r["mult_g"]).max() > 0 for r in ref)                 # (the comparison is not one of zeros)
    ctx.close()


# ---- 8. the Armijo probe
def test_armijo_on_a_general_context_matches_a_backtracking_loop_over_the_reference():
    p, lay = gpu_model()
    ps = [p, gpu_scenarios(p, (1,))[0]]
    ctx = _nlp_ctx(p, lay, 2, ps)
    R = NlpGeneralRef(ps[1])
    rng = np.random.default_rng(6)
    x = np.clip(p.x0 + 0.1 * rng.standard_normal(p.n), 0.3, 2.8)
    eta, tau, min_alpha = 0.4, 0.9, 1e-6
    seen = set()
    for mu, fr, scale, slope in ((0.0, False, 0.2, None), (0.0, False, 1.5, None), (5.0, False, 1.0, 1.0), (1.0, True, 1.0, 1e6)):
        step = -scale * R.grad(x) if mu == 0.0 else scale * rng.standard_normal(p.n)
        step = np.clip(step, 0.25 - x, 2.95 - x)                           # x + alpha step stays inside the box: every factor's domain
        phi = lambda a: (0.0 if fr else R.f(x + a * step)) + (1.0 if fr else mu) * O.norm_violations(
            R.g(x + a * step), p.gL, p.gU, x + a * step, p.xL, p.xU, 1)
        phi0 = phi(0.0)
        D = float(R.grad(x) @ step) if slope is None else -slope * (1.0 + abs(phi0))
        alpha, valid, nev = 1.0, True, 0
        while True:
            v = phi(alpha); nev += 1
            if not (v > phi0 + eta * alpha * D):
                break
            if alpha < min_alpha:
                valid = False
                break
            alpha *= tau
        got = ctx.acopf_armijo(1, x, step, mu, phi0, D, eta, tau, min_alpha, fr)
        print("armijo", (mu, fr, scale, slope), got, (alpha, valid, nev))
        assert got == (alpha, valid, nev), (mu, fr, scale, slope)
        seen.add((valid, nev > 1))
    assert (True, True) in seen and (False, True) in seen                   # a backtracked valid step and an exhausted one
    ctx.close()


# ---- 9. refusals
def _expect(rc, code, words, ctx):
    assert rc == code, rc
    msg = ctx.L.sqphip_last_error(ctx.h).decode()
    assert all(w in msg for w in words), msg


def _attach_rc(ctx, p):
    try:
        ctx.nlp_attach(p, general=True)
        return 0
    except pkg.SqpHipError as e:
        return int(str(e).split("error ")[1].split(":")[0])


def _refused(lay, p, words, code=EINVAL):
    ctx = _ctx(lay, 1)
    _expect(_attach_rc(ctx, p), code, ["sqphip_nlp_attach_general"] + words, ctx)
    ctx.close()


def _with(p, k, **kw):
    out = dataclasses.replace(p, **{name: getattr(p, name).copy() for name in kw})
    for name, v in kw.items():
        getattr(out, name)[k] = v
    return out


def _model(terms, n=6, m=2, nlin=1):
    return make_nlp_terms(n, m, nlin, terms, xL=np.full(n, 0.2), xU=np.full(n, 3.0), gL=np.full(m, -5.0), gU=np.full(m, 5.0), x0=np.ones(n))


def test_every_refusal_names_the_term_and_the_factor():
    A = lambda *vs: [(v, 1.0) for v in vs]
    # term 2: sin(x1 + x2) (x1 + x3)^0.5 x2: variables 1 and 2 shared; term 3: (x4 + x5)(x4 - x6), both plain linear
    good = _model([(1, 1.0, [(1, POW)]), (2, 0.5, [(A(1, 2), SIN), (A(1, 3), POWR, 0.5, 0.1), (2, POW)]),
                   (0, 1.0, [(A(4, 5), POW, 1, 0.0), ([(4, 1.0), (6, -1.0)], POW, 1, 0.0)])])
    lay = nlp_terms_layout(good)
    T, F = "term 2", "factor 1"
    assert needs_general(good) and good.avar.tolist() == [1, 1, 2, 1, 3, 2, 4, 5, 4, 6]
    # a variable twice in one factor stays refused; twice in one term is what the call is for
    _refused(lay, _with(good, 2, avar=1), [T, F, "variable 1", "twice in one factor"])
    # POWR: without fpar, exponent 0, exponent NaN
    _refused(lay, dataclasses.replace(good, fpar=None), [T, "factor 2", "fpar"])
    _refused(lay, _with(good, 2, fpar=0.0), [T, "factor 2", "exponent"])
    _refused(lay, _with(good, 2, fpar=np.nan), [T, "factor 2", "exponent"])
    _refused(lay, _with(good, 2, fpar=np.inf), [T, "factor 2", "exponent"])
    # kinds, factor counts
    _refused(lay, _with(good, 1, fkind=11), [T, F, "kind 11"])
    _refused(lay, _with(good, 1, fkind=-1), [T, F, "kind"])
    nine = _model([(2, 1.0, [(A(1), POW) for _ in range(9)])], n=2)
    _refused(nlp_terms_layout(nine), nine, ["term 1", "8 factors"])
    # a linear row still takes a single plain one-argument factor only
    bad = _model([(1, 1.0, [(A(1), POWR, 1.0, 0.0)])])
    _refused(nlp_terms_layout(bad), bad, ["term 1", "factor 1", "linear"])
    # Hessian entries: (4, 4) is needed because variable 4 sits in two plain linear factors; (1, 1) and (2, 1) by sharing
    for (r, c), fac in (((4, 4), "term 3 factor 2"), ((6, 5), "term 3 factor 2"), ((1, 1), "term 2"), ((3, 2), "term 2 factor 2")):
        h = int(np.flatnonzero((lay.hrow == r) & (lay.hcol == c))[0])
        _refused(dataclasses.replace(lay, hrow=np.delete(lay.hrow, h), hcol=np.delete(lay.hcol, h)), good, [fac, "Hessian", f"({r}, {c})"])
    j = int(np.flatnonzero((lay.jrow == 2) & (lay.jcol == 3))[0])
    _refused(dataclasses.replace(lay, jrow=np.delete(lay.jrow, j), jcol=np.delete(lay.jcol, j)), good, [T, "factor 2", "Jacobian", "(2, 3)"])
    # the older call keeps refusing a shared variable; left to itself Context.nlp_attach takes such a model to the new one
    shared = _model([(2, 1.0, [(A(1, 2), SIN), (1, POW)])])
    ctx = _ctx(nlp_terms_layout(shared), 1)
    with pytest.raises(pkg.SqpHipError):
        ctx.nlp_attach(shared, general=False)
    msg = ctx.L.sqphip_last_error(ctx.h).decode()
    assert "sqphip_nlp_attach_affine" in msg and "term 1 factor 2" in msg and "twice in one term" in msg
    ctx.nlp_attach(shared)
    ctx.close()
    ctx = _ctx(lay, 1)
    L = ctx.L
    # a refused attach leaves the context unattached: a good one goes in, a second one is refused
    _expect(_attach_rc(ctx, _with(good, 1, fkind=11)), EINVAL, [T, "kind 11"], ctx)
    ctx.nlp_attach(good)
    _expect(_attach_rc(ctx, good), ESTATE, ["sqphip_nlp_attach_general", "already"], ctx)
    # it is an NLP context to the other evaluators' entry points
    _expect(L.sqphip_acopf_set_instance(ctx.h, 0, None, None, None, None), EINVAL, ["sqphip_acopf_set_instance", "NLP"], ctx)
    _expect(L.sqphip_qcqp_set_instance(ctx.h, 0, None, None, None, None, None, None, None), EINVAL, ["sqphip_qcqp_set_instance", "QCQP"], ctx)
    _expect(L.sqphip_sqp_stream_begin(ctx.h, 4), EINVAL, ["sqphip_sqp_stream_begin", "NLP"], ctx)
    R = NlpGeneralRef(good)
    lam = np.array([0.3, -1.1])
    _check_eval(ctx.acopf_eval(0, good.x0, 1.3, lam), R, good.x0, 1.3, lam, lay)             # ... and it evaluates
    ctx.close()
