"""Shifts, argument coefficients and real exponents owned by the instance (sqphip_nlp_attach_data, csrc/nlp_dev.hpp
NlpDev::data): the device evaluator with different data in every slot against the reference of that slot's own model, the
bit rule against sqphip_nlp_attach_general, batches against the oracle, logistic folds and Cobb-Douglas consumers in one
batch against their known answers, slot independence, the scenario queue against the batch, the Armijo probe, the refusals
and the untouched older calls.  tests/nlp_data_cases.py holds the cases, tests/test_nlp_data_cpu.py the oracle's word for
them.

Tolerances are those of tests/test_gpu_nlp_general.py: EVAL_TOL for the evaluator, TOL and the decision / IPM-count rules
of its test_generated_batch_matches_oracle for the batches, 1e-6 for the known answers."""
import dataclasses
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import sqpsolver_jl_amd as pkg                                        # noqa: E402
from sqpsolver_jl_amd.host import _d, _f                              # noqa: E402
from sqpsolver_jl_amd.nlp_terms import (POW, POWR, SIN, make_nlp_terms, nlp_affine_synth, nlp_terms_args,   # noqa: E402
                                        nlp_terms_layout, nlp_terms_scenario, nlp_terms_synth)
from oracle import oracle as O                                        # noqa: E402
from nlp_general_ref import QUEUE_NOISE, SQP_KW, NlpGeneralRef, OracleGeneralTerms, gpu_model   # noqa: E402
from nlp_data_cases import (BATCH_SCENARIOS, QUEUE_DATA_SCENARIOS, block_count, consumers_case, data_differs,   # noqa: E402
                            data_model, data_scenarios, edge_model, folds_case, same_structure, wide_model)

pytestmark = pytest.mark.gpu
TOL = 1e-8                                                            # tests/test_gpu_nlp_general.py
EVAL_TOL = 1e-13                                                      # tests/test_gpu_nlp_general.py
EINVAL, ESTATE = -1, -4
FULL = ("x", "g", "mult_g", "mult_x_L", "mult_x_U")
CALLBACKS = ("f", "grad", "g", "jval", "hval")


# ---- helpers (tests/test_gpu_nlp_general.py; a test module is not imported)
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


def _data_ctx(p, lay, batch, ps=None, **kw):
    ctx = _ctx(lay, batch, **kw)
    ctx.nlp_attach(p, instance_data=True)
    for b in range(batch):
        ctx.nlp_set_instance(b, (ps or [p] * batch)[b])
    return ctx


def _lin(kkt_mode):
    return dict(kkt_mode=2) if kkt_mode == 2 else dict(kkt_mode=1, kkt_tile_order=1)


def _check_eval(ev, R, x, sigma, lam, lay, tol=EVAL_TOL):
    want = dict(f=R.f(x), grad=R.grad(x), g=R.g(x), jval=R.jac(x, lay.jrow, lay.jcol), hval=R.hess(x, sigma, lam, lay.hrow, lay.hcol))
    err = {k: rel(ev[k], want[k]) for k in want}
    print("evaluator errors", err)
    assert all(np.all(np.isfinite(np.asarray(ev[k]))) for k in want)
    assert all(e <= tol for e in err.values()), err


def _same_result(ra, rb, where):
    for k in FULL:
        assert np.array_equal(ra[k], rb[k]), (where, k)
    assert (ra["obj_val"], ra["status"], ra["iter"]) == (rb["obj_val"], rb["status"], rb["iter"]), where


def _run(ctx):
    ctx.sqp_reset(); ctx.sqp_run(0)


# ---- 1. the evaluator with different data in every slot
@pytest.mark.parametrize("model", ["synth", "edge", "wide"])
def test_evaluator_reads_the_data_of_its_own_slot(model):
    p, lay = dict(synth=data_model, edge=edge_model, wide=wide_model)[model]()
    ps = data_scenarios(p)
    # the padding double: used by the edge model, not by the generated one
    assert block_count(p) % 2 == dict(synth=0, edge=1).get(model, block_count(p) % 2)
    assert model != "wide" or len(p.fkind) > 1024                     # SQPHIP_VEC_THREADS: beyond one stride of the thread loops
    assert all(same_structure(p, q) for q in ps)
    assert min(data_differs(a, b) for a, b in itertools.combinations([p] + ps, 2)) > 1e-3      # first, last and every other
    ctx = _data_ctx(p, lay, 4, ps)
    rng = np.random.default_rng(8)
    lam = rng.standard_normal(p.m)
    for point in range(3):
        x = rng.uniform(0.5, 1.6, p.n) if model == "edge" else np.clip(p.x0 + 0.2 * rng.standard_normal(p.n), 0.25, 2.9)
        for b, q in enumerate(ps):
            R = NlpGeneralRef(q)
            assert R.domain_margin(x) > 0
            ev = ctx.acopf_eval(b, x, 1.3, lam)
            _check_eval(ev, R, x, 1.3, lam, lay)
            if point == 0 and b == 0:                                   # the data matters at the tolerance of the check
                assert rel(ev["g"], NlpGeneralRef(ps[-1]).g(x)) > 1e3 * EVAL_TOL
    ctx.close()


# ---- 2. the bit rule
@pytest.mark.parametrize("model", ["one_argument", "affine", "general"])
def test_a_data_context_with_the_data_of_the_attach_files_the_bits_of_the_general_call(model):
    if model == "one_argument":
        q, seed = nlp_terms_synth(24, 14, seed=5), 5
    elif model == "affine":
        q, seed = nlp_affine_synth(24, 14, seed=1), 1
    else:
        q, seed = gpu_model()[0], 1
    qs = [nlp_terms_scenario(q, s, seed) for s in range(4)]           # other f0 | g0 | c, the data of the attach
    lay = nlp_terms_layout(q)
    cg = _ctx(lay, 4, **SQP_KW)
    cg.nlp_attach(q, general=True)
    for b in range(4):
        cg.nlp_set_instance(b, qs[b])
    cd = _data_ctx(q, lay, 4, qs, **SQP_KW)
    rng = np.random.default_rng(3)
    x = np.clip(q.x0 + 0.3 * rng.standard_normal(q.n), 0.25, 2.9); lam = rng.standard_normal(q.m)
    for b in range(4):
        eg, ed = cg.acopf_eval(b, x, 1.3, lam), cd.acopf_eval(b, x, 1.3, lam)
        for k in CALLBACKS:
            assert np.array_equal(np.asarray(eg[k]), np.asarray(ed[k])), (b, k)
    _run(cg); _run(cd)
    for b in range(4):
        assert cg.sqp_get(b)["status"] == 0
        _same_result(cg.sqp_get(b), cd.sqp_get(b), b)
        assert cg.sqp_trace(b) == cd.sqp_trace(b), b
    for wg, wd in zip(cg.sqp_work(), cd.sqp_work()):
        assert np.array_equal(wg, wd) and wg.sum() > 0
    kg, kd = cg.counters(), cd.counters()
    assert all(kg[k] == kd[k] for k in ("n_qp", "n_ipm_iter", "n_factor", "n_solve", "n_sweeps")), (kg, kd)
    cg.close(); cd.close()


# ---- 3. a batch of data scenarios against the oracle
@pytest.mark.parametrize("kkt_mode", [2, 1])
def test_data_batch_matches_oracle(kkt_mode):
    p, lay = data_model()
    ps = data_scenarios(p)
    ctx = _data_ctx(p, lay, 4, ps, kkt_mode=kkt_mode, **SQP_KW)
    _run(ctx)
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


# ---- 4. known answers, four datasets in one batch
def _solve_batch(models):
    lay = nlp_terms_layout(models[0])
    ctx = _data_ctx(models[0], lay, len(models), models, max_iter=60, literal_quirks=0, tol_infeas=1e-8, tol_residual=1e-8)
    _run(ctx)
    out = [ctx.sqp_get(b) for b in range(len(models))]
    ctx.close()
    print("status", [r["status"] for r in out], "iter", [r["iter"] for r in out])
    assert all(r["status"] == 0 for r in out)
    return [r["x"] for r in out]


def _visibly_different(xs):
    return min(np.abs(a - b).max() for a, b in itertools.combinations(xs, 2)) > 1e-3


def test_logistic_folds_in_one_batch_match_scipy_per_fold():
    import scipy.optimize
    X, y, reg, folds, idx = folds_case(4)
    assert len(folds) == 4 and all(same_structure(folds[0], f) for f in folds)
    want = []
    for tr, _ in idx:
        Xf, yf = X[tr], y[tr]
        loss = lambda w: float(np.sum(np.logaddexp(0.0, Xf @ w) - yf * (Xf @ w)) + 0.5 * reg * (w @ w))
        want.append(scipy.optimize.minimize(loss, np.zeros(X.shape[1]), method="BFGS", options=dict(gtol=1e-10)).x)
    assert _visibly_different(want)                                   # a context that ignores the data cannot pass
    got = _solve_batch(folds)
    for f in range(4):
        assert np.abs(got[f] - want[f]).max() <= 1e-6, f


def test_cobb_douglas_consumers_in_one_batch_reach_their_closed_forms():
    alphas, prices, wealth, models = consumers_case()
    want = [a * wealth / (prices * a.sum()) for a in alphas]
    assert _visibly_different(want)
    got = _solve_batch(models)
    for b in range(4):
        assert np.abs(got[b] - want[b]).max() <= 1e-6, b


# ---- 5. slot independence
def test_an_instance_does_not_depend_on_its_slot_its_neighbours_the_run_or_the_groups():
    p, lay = data_model()
    ps = data_scenarios(p, (1, 2, 3, 1))                              # slots 0 and 3: the same instance, other neighbours
    ctx = _data_ctx(p, lay, 4, ps, kkt_mode=2, **SQP_KW)              # (the sparse path: the one that forms instance groups)
    runs = []
    for _ in range(2):
        _run(ctx)
        runs.append([(ctx.sqp_get(b), ctx.sqp_trace(b)) for b in range(4)])
    assert ctx.counters()["n_groups"] == 1
    ctx.close()
    assert all(r[0]["status"] == 0 for r in runs[0])
    _same_result(runs[0][0][0], runs[0][3][0], "slots 0 and 3")
    assert runs[0][0][1] == runs[0][3][1]
    assert not np.array_equal(runs[0][0][0]["x"], runs[0][1][0]["x"])  # (the neighbours are other problems)
    for b in range(4):
        _same_result(runs[0][b][0], runs[1][b][0], ("second run", b))
        assert runs[0][b][1] == runs[1][b][1]
    os.environ["SQPHIP_GROUPS"] = "2"
    try:
        ctx = _data_ctx(p, lay, 4, ps, kkt_mode=2, **SQP_KW)
        _run(ctx)
    finally:
        del os.environ["SQPHIP_GROUPS"]
    assert ctx.counters()["n_groups"] == 2
    for b in range(4):
        _same_result(runs[0][b][0], ctx.sqp_get(b), ("two groups", b))
        assert runs[0][b][1] == ctx.sqp_trace(b)
    ctx.close()


# ---- 6. the scenario queue
def test_queue_files_the_bits_of_the_batch_and_stream_set_restores_the_data_of_the_attach():
    p, lay = data_model()
    ps = data_scenarios(p, QUEUE_DATA_SCENARIOS, QUEUE_NOISE)
    M = len(ps)
    assert M == 6 and ps[0] is p
    cb = _data_ctx(p, lay, M, ps, kkt_mode=2, **SQP_KW)
    _run(cb)
    ref = [cb.sqp_get(b) for b in range(M)]
    cb.close()
    assert all(r["status"] == 0 for r in ref)
    assert min(np.abs(a["x"] - b["x"]).max() for a, b in itertools.combinations(ref, 2)) > 1e-6     # the data is read
    ctx = _ctx(lay, 2, kkt_mode=2, **SQP_KW)
    ctx.nlp_attach(p, instance_data=True)
    ctx.nlp_stream_begin(M, keep_multipliers=True)
    for s in range(M):
        ctx.nlp_stream_set(s, ps[s])
    ctx.stream_run()
    for s in range(M):
        r = ctx.stream_get_full(s)
        print("scenario", s, "status", r["status"], "iter", r["iter"], "batch", ref[s]["iter"])
        _same_result(r, ref[s], s)
    assert any(np.abs(r["mult_g"]).max() > 0 for r in ref)
    ctx.close()
    # _stream_set after _stream_set_data writes the whole block: scenario 0 is back at the data of the attach
    ctx = _ctx(lay, 2, kkt_mode=2, **SQP_KW)
    ctx.nlp_attach(p, instance_data=True)
    ctx.nlp_stream_begin(2, keep_multipliers=True)
    ctx.nlp_stream_set(0, ps[3]); ctx.nlp_stream_set(1, ps[3])
    assert ctx.L.sqphip_nlp_stream_set(ctx.h, 0, None, None, None, None, None, None, None, _d(_f(p.x0))) == 0
    ctx.stream_run()
    _same_result(ctx.stream_get_full(0), ref[0], "restored")
    _same_result(ctx.stream_get_full(1), ref[3], "overlaid")
    ctx.close()


# ---- 7. the Armijo probe
def test_armijo_on_a_data_context_matches_a_backtracking_loop_over_the_reference_of_the_instance():
    p, lay = data_model()
    ps = [p, data_scenarios(p, (2,), QUEUE_NOISE)[0]]
    ctx = _data_ctx(p, lay, 2, ps)
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


# ---- 8. refusals
def _expect(rc, code, words, ctx):
    assert rc == code, rc
    msg = ctx.L.sqphip_last_error(ctx.h).decode()
    assert all(w in msg for w in words), msg


def _model(terms, n=6, m=2, nlin=1):
    return make_nlp_terms(n, m, nlin, terms, xL=np.full(n, 0.2), xU=np.full(n, 3.0), gL=np.full(m, -5.0), gU=np.full(m, 5.0), x0=np.ones(n))


def _good():
    A = lambda *vs: [(v, 1.0) for v in vs]
    # term 1: the linear row; term 2: sin(x1 + x2) (x1 + x3 + 0.1)^0.5 x2; term 3: (x4 + x5)(x4 - x6)
    return _model([(1, 1.0, [(1, POW)]), (2, 0.5, [(A(1, 2), SIN), (A(1, 3), POWR, 0.5, 0.1), (2, POW)]),
                   (0, 1.0, [(A(4, 5), POW, 1, 0.0), ([(4, 1.0), (6, -1.0)], POW, 1, 0.0)])])


def _changed(a, k, v):
    out = np.array(a, dtype=np.float64)
    out[k] = v
    return out


def test_every_refusal_of_the_data_calls_has_its_message():
    good = _good()
    lay = nlp_terms_layout(good)
    assert good.avar.tolist() == [1, 1, 2, 1, 3, 2, 4, 5, 4, 6] and good.fkind[2] == POWR
    # the attach is the general call under another name: the class, the checks, the messages, ESTATE
    ctx = _ctx(lay, 2)
    with pytest.raises(pkg.SqpHipError):
        ctx.nlp_attach(dataclasses.replace(good, fkind=_changed(good.fkind, 1, 11).astype(np.int32)), instance_data=True)
    _expect(EINVAL, EINVAL, ["sqphip_nlp_attach_data", "term 2", "factor 1", "kind 11"], ctx)
    with pytest.raises(pkg.SqpHipError):
        ctx.nlp_attach(dataclasses.replace(good, fpar=_changed(good.fpar, 2, 0.0)), instance_data=True)
    _expect(EINVAL, EINVAL, ["sqphip_nlp_attach_data", "term 2", "factor 2", "exponent"], ctx)
    ctx.nlp_attach(good, instance_data=True)
    with pytest.raises(pkg.SqpHipError):
        ctx.nlp_attach(good, instance_data=True)
    _expect(ESTATE, ESTATE, ["sqphip_nlp_attach_data", "already"], ctx)
    L, h = ctx.L, ctx.h
    sh, ac, par = _f(good.fshift), _f(good.acoef), _f(good.fpar)
    for fn, who, first in ((L.sqphip_nlp_set_instance_data, "sqphip_nlp_set_instance_data", 0),
                           (L.sqphip_nlp_stream_set_data, "sqphip_nlp_stream_set_data", 1)):
        if first:
            # the queue call: refused before sqphip_nlp_stream_begin and outside the queue
            _expect(fn(h, 0, _d(sh), _d(ac), _d(par)), EINVAL, [who, "sqphip_nlp_stream_begin"], ctx)
            ctx.nlp_stream_begin(3)
            _expect(fn(h, 3, _d(sh), _d(ac), _d(par)), EINVAL, [who, "scenario 3"], ctx)
            _expect(fn(h, -1, None, None, None), EINVAL, [who, "scenario -1"], ctx)
        else:
            _expect(fn(h, 2, _d(sh), _d(ac), _d(par)), EINVAL, [who, "instance 2"], ctx)
            _expect(fn(h, -1, None, None, None), EINVAL, [who, "instance -1"], ctx)
        for bad in (0.0, np.nan, np.inf):
            _expect(fn(h, 0, None, None, _d(_changed(par, 2, bad))), EINVAL, [who, "term 2", "factor 2", "exponent"], ctx)
        _expect(fn(h, 0, None, _d(_changed(ac, 0, 2.0)), None), EINVAL, [who, "term 1", "linear"], ctx)
        _expect(fn(h, 0, _d(_changed(sh, 0, 0.1)), None, None), EINVAL, [who, "term 1", "linear"], ctx)
        # the exponent of a factor that is not POWR is not read; a zero coefficient is allowed outside the linear rows
        assert fn(h, 0, _d(sh), _d(_changed(ac, 2, 0.0)), _d(_changed(par, 0, 0.0))) == 0
        assert fn(h, 0, None, None, None) == 0 and fn(h, 1, _d(sh), _d(ac), _d(par)) == 0
    # what was refused changed nothing; instance 0 carries the zero coefficient, instance 1 the data of the attach
    lam = np.array([0.3, -1.1])
    x = np.linspace(0.8, 1.3, good.n)
    zeroed = dataclasses.replace(good, acoef=_changed(ac, 2, 0.0))
    for b, q in ((0, zeroed), (1, good)):
        _check_eval(ctx.acopf_eval(b, x, 1.3, lam), NlpGeneralRef(q), x, 1.3, lam, lay)
    # Context: a model of another structure is refused before anything is sent
    other = dataclasses.replace(good, avar=_changed(good.avar, 4, 5).astype(np.int64))
    for call in (lambda: ctx.nlp_set_instance(0, other), lambda: ctx.nlp_stream_set(0, other)):
        with pytest.raises(pkg.SqpHipError, match="structure"):
            call()
    ctx.close()
    # fpar on a model without a POWR factor
    q = nlp_affine_synth(24, 14, seed=1)
    ctx = _ctx(nlp_terms_layout(q), 1)
    ctx.nlp_attach(q, instance_data=True)
    zeros = np.zeros(len(q.fkind))
    _expect(ctx.L.sqphip_nlp_set_instance_data(ctx.h, 0, None, None, _d(zeros)), EINVAL, ["sqphip_nlp_set_instance_data", "fpar", "POWR"], ctx)
    ctx.nlp_stream_begin(1)
    _expect(ctx.L.sqphip_nlp_stream_set_data(ctx.h, 0, None, None, _d(zeros)), EINVAL, ["sqphip_nlp_stream_set_data", "fpar", "POWR"], ctx)
    ctx.close()


# ---- 9. the older calls
@pytest.mark.parametrize("model", ["one_argument", "affine", "general"])
def test_contexts_of_the_older_calls_refuse_the_data_calls_and_keep_their_set_instance(model):
    q, seed = dict(one_argument=(nlp_terms_synth(24, 14, seed=5), 5), affine=(nlp_affine_synth(24, 14, seed=1), 1),
                   general=(gpu_model()[0], 1))[model]
    lay = nlp_terms_layout(q)
    q1 = nlp_terms_scenario(q, 1, seed)
    ctx = _ctx(lay, 2)
    ctx.nlp_attach(q)
    ctx.nlp_set_instance(0, q); ctx.nlp_set_instance(1, q1)
    _, _, acoef = nlp_terms_args(q)
    sh, ac = _f(q.fshift), _f(acoef)
    _expect(ctx.L.sqphip_nlp_set_instance_data(ctx.h, 0, _d(sh), _d(ac), None), EINVAL, ["sqphip_nlp_set_instance_data", "sqphip_nlp_attach_data"], ctx)
    _expect(ctx.L.sqphip_nlp_stream_set_data(ctx.h, 0, _d(sh), _d(ac), None), EINVAL, ["sqphip_nlp_stream_set_data", "sqphip_nlp_attach_data"], ctx)
    with pytest.raises(TypeError):
        ctx.nlp_set_instance(0, q, fshift=sh)
    rng = np.random.default_rng(3)
    x = np.clip(q.x0 + 0.3 * rng.standard_normal(q.n), 0.25, 2.9); lam = rng.standard_normal(q.m)
    # a model with other data changes nothing on such a context: the structure, data included, is the batch's
    ctx.nlp_set_instance(1, dataclasses.replace(q1, fshift=q1.fshift + 0.25))
    for b, m in ((0, q), (1, q1)):
        _check_eval(ctx.acopf_eval(b, x, 1.3, lam), NlpGeneralRef(m), x, 1.3, lam, lay)
    ctx.nlp_stream_begin(2)
    _expect(ctx.L.sqphip_nlp_stream_set_data(ctx.h, 0, _d(sh), _d(ac), None), EINVAL, ["sqphip_nlp_stream_set_data", "sqphip_nlp_attach_data"], ctx)
    ctx.close()
