"""Factors with affine multi-variable arguments in the batched device SQP loop (sqphip_nlp_attach_affine, csrc/nlp_dev.hpp):
the device evaluator against the term-by-term numpy reference (tests/nlp_affine_ref.py) on generated and hand-made models,
generated batches against the oracle, the joint polar restatement v_f v_t cos(th_f - th_t) against the dedicated polar
ACOPF path, a one-argument model through both entry points bit for bit, determinism, the scenario queue against the batch,
the Armijo probe and every refusal.  tests/test_nlp_affine_cpu.py holds the oracle's word for the generated instances."""
import dataclasses
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import sqpsolver_jl_amd as pkg                                        # noqa: E402
from sqpsolver_jl_amd.acopf_synth import acopf_layout, acopf_synth, contingency, CASES   # noqa: E402
from sqpsolver_jl_amd.nlp_terms import (POW, SIN, from_polar_acopf, make_nlp_terms, nlp_affine_synth, nlp_terms_args,   # noqa: E402
                                        nlp_terms_layout, nlp_terms_scenario, nlp_terms_synth)
from oracle import oracle as O                                        # noqa: E402
from nlp_affine_ref import (QUEUE_NOISE, QUEUE_SCENARIOS, SQP_KW, NlpAffineRef, OracleAffineTerms, affine_edge_model,   # noqa: E402
                            gpu_model, gpu_scenarios)
from qcqp_ref import coo_sum                                          # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-8
EINVAL, ESTATE = -1, -4
FULL = ("x", "g", "mult_g", "mult_x_L", "mult_x_U")


# ---- helpers (tests/test_gpu_nlp.py; a test module is not imported)
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


def _nlp_ctx(p, lay, batch, ps=None, **kw):
    ctx = _ctx(lay, batch, **kw)
    ctx.nlp_attach(p)
    for b in range(batch):
        ctx.nlp_set_instance(b, (ps or [p] * batch)[b])
    return ctx


def _lin(kkt_mode):
    return dict(kkt_mode=2) if kkt_mode == 2 else dict(kkt_mode=1, kkt_tile_order=1)


def _check_eval(ev, R, x, sigma, lam, lay, tol=1e-13, summed=False):
    J = (lambda v: coo_sum(v, lay.jrow, lay.jcol, lay.n)) if summed else (lambda v: v)
    H = (lambda v: coo_sum(v, lay.hrow, lay.hcol, lay.n, lower=True)) if summed else (lambda v: v)
    want = dict(f=R.f(x), grad=R.grad(x), g=R.g(x), jval=J(R.jac(x, lay.jrow, lay.jcol)), hval=H(R.hess(x, sigma, lam, lay.hrow, lay.hcol)))
    got = dict(ev, jval=J(ev["jval"]), hval=H(ev["hval"]))
    err = {k: rel(got[k], want[k]) for k in want}
    print("evaluator errors", err)
    assert all(e <= tol for e in err.values()), err


def _as_affine(q):
    """the one-argument model q with argument arrays: the same model through sqphip_nlp_attach_affine"""
    aptr, avar, acoef = nlp_terms_args(q)
    return dataclasses.replace(q, aptr=aptr.copy(), avar=avar.copy(), acoef=acoef.copy())


# ---- 1. the evaluator against the reference
def test_evaluator_on_a_generated_model_with_per_instance_values():
    p, lay = gpu_model()
    assert p.affine and np.diff(p.aptr).max() == 3
    ps = gpu_scenarios(p, range(3))
    ctx = _nlp_ctx(p, lay, 3, ps)
    rng = np.random.default_rng(3)
    x = np.clip(p.x0 + 0.3 * rng.standard_normal(p.n), 0.25, 2.9); lam = rng.standard_normal(p.m)
    for b in range(3):
        _check_eval(ctx.acopf_eval(b, x, 1.3, lam), NlpAffineRef(ps[b]), x, 1.3, lam, lay)
    # a NULL part keeps what the instance had
    c2 = ps[2].tcoef * 0.5
    ctx.nlp_set_instance(2, tcoef=c2)
    _check_eval(ctx.acopf_eval(2, x, 1.3, lam), NlpAffineRef(dataclasses.replace(ps[2], tcoef=c2)), x, 1.3, lam, lay)
    assert ctx.acopf_eval(2, x, 1.3, lam)["f"] != ctx.acopf_eval(1, x, 1.3, lam)["f"]
    ctx.close()


# ---- 2. plan edges, evaluator only
def test_evaluator_at_the_plan_edges():
    p, lay = affine_edge_model()
    nargs, nfac = np.diff(p.aptr), np.diff(p.tptr)
    assert nfac.max() == 8 and nargs[:8].tolist() == [8, 1, 2, 3, 2, 2, 2, 2] and set(p.fkind[:8].tolist()) == {0, 1, 2, 3, 4}
    p1 = dataclasses.replace(p, tcoef=p.tcoef * np.array([1.2, 0.8, -1.0, 0.5, 1.5, -0.7]), g0=p.g0 + 0.1, f0=-0.5)
    ctx = _nlp_ctx(p, lay, 2, [p, p1])
    rng = np.random.default_rng(8)
    x = rng.uniform(0.5, 1.6, p.n); lam = rng.standard_normal(p.m)
    pairs = set(zip(lay.hrow.tolist(), lay.hcol.tolist()))
    # the plain linear factor on variables 25, 26, 27: no entries within the factor, cross entries with 28 and with 1, 29
    assert not {(26, 25), (27, 25), (27, 26), (25, 25), (26, 26), (27, 27)} & pairs
    assert {(28, 25), (28, 26), (28, 27), (25, 1), (29, 27), (28, 28), (29, 1)} <= pairs
    for b, q in enumerate((p, p1)):
        ev = ctx.acopf_eval(b, x, 1.3, lam)
        _check_eval(ev, NlpAffineRef(q), x, 1.3, lam, lay)
        _check_eval(ev, NlpAffineRef(q), x, 1.3, lam, lay, summed=True)
        assert ev["jval"][-1] == 0.0 and ev["hval"][-2] == 0.0 and ev["hval"][-1] == 0.0     # unused slots, the copy of a slot
        assert np.all(ev["jval"][:-1] != 0.0) and np.all(ev["hval"][:-2] != 0.0)
        assert ev["grad"][29] != 0.0 and np.all(ev["grad"][2:8] == 0.0) and np.all(ev["grad"][9:22] == 0.0)
    ctx.close()


def test_evaluator_beyond_one_stride_of_the_thread_loops():
    p = nlp_affine_synth(600, 500, seed=2)
    lay = nlp_terms_layout(p)
    assert len(p.trow) > 1024 and len(lay.jrow) > 1024 and len(p.fkind) > 2048 and len(p.avar) > 4096
    ctx = _nlp_ctx(p, lay, 1)
    rng = np.random.default_rng(5)
    x = np.clip(p.x0 + 0.2 * rng.standard_normal(p.n), 0.25, 2.9); lam = rng.standard_normal(p.m)
    _check_eval(ctx.acopf_eval(0, x, 1.3, lam), NlpAffineRef(p), x, 1.3, lam, lay)
    ctx.close()


# ---- 4. a generated batch against the oracle
@pytest.mark.parametrize("kkt_mode", [2, 1])
def test_generated_batch_matches_oracle(kkt_mode):
    p, lay = gpu_model()
    ps = gpu_scenarios(p)
    ctx = _nlp_ctx(p, lay, 4, ps, kkt_mode=kkt_mode, **SQP_KW)
    ctx.sqp_reset(); ctx.sqp_run(0)
    try:
        for b in range(4):
            ro = O.sqp_solve(OracleAffineTerms(ps[b], lay), O.default_options(**_lin(kkt_mode), **SQP_KW))
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


# ---- 5. joint polar restatement = dedicated polar path
def test_joint_polar_restatement_equals_dedicated_polar_path_on_contingencies():
    nb, ng, nl, seed = CASES["case14"]
    base = acopf_synth(nb, ng, nl, seed)
    nets = [base, contingency(base, 2, seed), contingency(base, 5, seed)]
    lays = [acopf_layout(nt) for nt in nets]
    ps = [from_polar_acopf(nt, ly, joint=True) for nt, ly in zip(nets, lays)]
    assert ps[0].affine and np.diff(ps[0].aptr).max() == 2
    kw = dict(max_iter=60, use_soc=1, literal_quirks=0, tol_infeas=1e-6, tol_residual=1e-4)
    cg = _ctx(lays[0], 3, **kw); cg.nlp_attach(ps[0])
    cd = _ctx(lays[0], 3, **kw); cd.acopf_attach(nets[0], lays[0])
    for b in range(3):
        cg.nlp_set_instance(b, ps[b]); cd.acopf_set_instance(b, nets[b], lays[b])
    rng = np.random.default_rng(2)
    x = lays[0].x0 + 0.05 * rng.standard_normal(lays[0].n); lam = rng.standard_normal(lays[0].m)
    eg, ed = cg.acopf_eval(1, x, 0.7, lam), cd.acopf_eval(1, x, 0.7, lam)
    J = lambda v: coo_sum(v, lays[0].jrow, lays[0].jcol, lays[0].n)
    H = lambda v: coo_sum(v, lays[0].hrow, lays[0].hcol, lays[0].n, lower=True)
    err = dict(f=rel(eg["f"], ed["f"]), grad=rel(eg["grad"], ed["grad"]), g=rel(eg["g"], ed["g"]),
               jval=rel(J(eg["jval"]), J(ed["jval"])), hval=rel(H(eg["hval"]), H(ed["hval"])))
    print("joint against dedicated evaluator", err)
    assert all(e <= 1e-12 for e in err.values()), err
    for c in (cg, cd):
        c.sqp_reset(); c.sqp_run(0)
    assert np.array_equal(cg.sqp_status()[0], cd.sqp_status()[0]) and np.array_equal(cg.sqp_status()[1], cd.sqp_status()[1])
    for b in range(3):
        rg, rd = cg.sqp_get(b), cd.sqp_get(b)
        print("instance", b, "status", rg["status"], "iter", rg["iter"], "x", rel(rg["x"], rd["x"]))
        assert (rg["status"], rg["iter"]) == (rd["status"], rd["iter"]), b
        assert _decisions(cg.sqp_trace(b)) == _decisions(cd.sqp_trace(b)), b
        assert rel(rg["x"], rd["x"]) < TOL, b
    cg.close(); cd.close()


# ---- 6. one argument per factor: both entry points file the same bits
def test_a_one_argument_model_files_the_same_bits_through_both_entry_points():
    q = nlp_terms_synth(24, 14, seed=5)
    lay = nlp_terms_layout(q)
    qs = [nlp_terms_scenario(q, s, 5) for s in range(3)]
    co = _nlp_ctx(q, lay, 3, qs, **SQP_KW)
    ca = _nlp_ctx(_as_affine(q), lay, 3, [_as_affine(s) for s in qs], **SQP_KW)
    rng = np.random.default_rng(3)
    x = np.clip(q.x0 + 0.3 * rng.standard_normal(q.n), 0.25, 2.9); lam = rng.standard_normal(q.m)
    for b in range(3):
        eo, ea = co.acopf_eval(b, x, 1.3, lam), ca.acopf_eval(b, x, 1.3, lam)
        for k in ("f", "grad", "g", "jval", "hval"):
            assert np.array_equal(np.asarray(eo[k]), np.asarray(ea[k])), (b, k)
    for c in (co, ca):
        c.sqp_reset(); c.sqp_run(0)
    for b in range(3):
        ro, ra = co.sqp_get(b), ca.sqp_get(b)
        assert ro["status"] == 0
        for k in FULL:
            assert np.array_equal(ro[k], ra[k]), (b, k)
        assert (ro["obj_val"], ro["status"], ro["iter"]) == (ra["obj_val"], ra["status"], ra["iter"]), b
        assert co.sqp_trace(b) == ca.sqp_trace(b), b
    co.close(); ca.close()


# ---- 7. determinism
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


# ---- 8. the scenario queue
def test_queue_files_the_bits_of_the_batch_with_multipliers():
    p, lay = gpu_model()
    ps = gpu_scenarios(p, QUEUE_SCENARIOS, QUEUE_NOISE)
    M = len(ps)
    cb = _nlp_ctx(p, lay, M, ps, kkt_mode=2, **SQP_KW)
    cb.sqp_reset(); cb.sqp_run(0)
    ref = [cb.sqp_get(b) for b in range(M)]
    cb.close()
    ctx = _ctx(lay, 4, kkt_mode=2, **SQP_KW)
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
    assert len({r["iter"] for r in ref}) > 1                               # the slots refill at different times
    assert any(np.abs(r["mult_g"]).max() > 0 for r in ref)                 # (the comparison is not one of zeros)
    ctx.close()


# ---- 9. the Armijo probe
def test_armijo_on_an_affine_context_matches_a_backtracking_loop_over_the_reference():
    p, lay = gpu_model()
    ps = [p, gpu_scenarios(p, (1,))[0]]
    ctx = _nlp_ctx(p, lay, 2, ps)
    R = NlpAffineRef(ps[1])
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


# ---- 10. refusals
def _expect(rc, code, words, ctx):
    assert rc == code, rc
    msg = ctx.L.sqphip_last_error(ctx.h).decode()
    assert all(w in msg for w in words), msg


def _attach_rc(ctx, p):
    try:
        ctx.nlp_attach(p)
        return 0
    except pkg.SqpHipError as e:
        return int(str(e).split("error ")[1].split(":")[0])


def _refused(lay, p, words, code=EINVAL):
    ctx = _ctx(lay, 1)
    _expect(_attach_rc(ctx, p), code, ["sqphip_nlp_attach_affine"] + words, ctx)
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
    good = _model([(1, 1.0, [(1, POW)]), (2, 0.5, [(A(1, 2), SIN), (3, POW, 2)]), (0, 1.0, [(A(4, 5, 6), POW, 2, -1.0)])])
    lay = nlp_terms_layout(good)
    T, F = "term 2", "factor 1"
    # aptr
    bad = dataclasses.replace(good, aptr=good.aptr + 1)
    _refused(lay, bad, ["aptr[0]"])
    bad = _with(good, 2, aptr=5)                                           # 0 1 5 4 7: decreasing at factor 2 of term 2
    _refused(lay, bad, [T, "factor 2", "aptr decreases"])
    bad = _with(good, 2, aptr=1)                                           # 0 1 1 4 7: factor 1 of term 2 has no arguments
    _refused(lay, bad, [T, F, "no arguments"])
    nine = _model([(2, 1.0, [(A(*range(1, 10)), SIN)])], n=9)
    _refused(nlp_terms_layout(nine), nine, ["term 1", F, "8 arguments"])
    # variables
    _refused(lay, _with(good, 2, avar=7), [T, F, "variable 7", "out of range"])
    _refused(lay, _with(good, 2, avar=0), [T, F, "variable 0", "out of range"])
    _refused(lay, _with(good, 2, avar=1), [T, F, "variable 1", "twice in one factor"])
    _refused(lay, _with(good, 3, avar=2), [T, "factor 2", "variable 2", "twice in one term"])
    # kinds and exponents
    _refused(lay, _with(good, 1, fkind=7), [T, F, "kind"])
    for e in (0, 33, -33):
        _refused(lay, _with(good, 2, fexp=e), [T, "factor 2", "exponent"])
    # terms
    _refused(lay, _with(good, 1, trow=3), [T, "out of range"])
    nine = _model([(2, 1.0, [(A(j), POW) for j in range(1, 10)])], n=9)
    _refused(nlp_terms_layout(nine), nine, ["term 1", "8 factors"])
    _refused(lay, dataclasses.replace(good, tptr=np.array([0, 0, 3, 4])), ["term 1", "no factors"])
    # a linear row takes a single plain one-argument factor with coefficient 1 and shift 0
    for bad in (_model([(1, 1.0, [(A(1, 2), POW)])]), _model([(1, 1.0, [([(1, 2.0)], POW)])]), _model([(1, 1.0, [(A(1), POW, 1, 0.5)])]),
                _model([(1, 1.0, [(A(1), POW, 2)])]), _model([(1, 1.0, [(A(1), SIN)])]), _model([(1, 1.0, [(A(1), POW), (A(2), POW)])])):
        _refused(nlp_terms_layout(bad), bad, ["term 1", "factor 1", "linear"])
    # a Jacobian entry missing: the second argument of the factor
    j = int(np.flatnonzero((lay.jrow == 2) & (lay.jcol == 2))[0])
    _refused(dataclasses.replace(lay, jrow=np.delete(lay.jrow, j), jcol=np.delete(lay.jcol, j)), good, [T, F, "Jacobian", "(2, 2)"])
    # a Hessian entry missing: two arguments of one factor, two factors, the diagonal of an argument
    for (r, c), fac in (((2, 1), F), ((3, 2), "factor 2"), ((2, 2), F), ((6, 4), "term 3 factor 1")):
        h = int(np.flatnonzero((lay.hrow == r) & (lay.hcol == c))[0])
        _refused(dataclasses.replace(lay, hrow=np.delete(lay.hrow, h), hcol=np.delete(lay.hcol, h)), good, [fac, "Hessian", f"({r}, {c})"])
    # without a Hessian structure only the Jacobian is checked
    ctx = _ctx(dataclasses.replace(lay, hrow=lay.hrow[:0], hcol=lay.hcol[:0]), 1)
    assert _attach_rc(ctx, good) == 0
    ctx.close()
    # a refused attach leaves the context unattached: a good one goes in, a second one of either kind is refused
    ctx = _ctx(lay, 1)
    _expect(_attach_rc(ctx, _with(good, 2, avar=0)), EINVAL, [T, "out of range"], ctx)
    ctx.nlp_attach(good)
    _expect(_attach_rc(ctx, good), ESTATE, ["sqphip_nlp_attach_affine", "already"], ctx)
    one = _model([(1, 1.0, [(1, POW)])])
    _expect(_attach_rc(ctx, one), ESTATE, ["sqphip_nlp_attach:", "already"], ctx)
    # it is an NLP context to the other evaluators' entry points
    L = ctx.L
    _expect(L.sqphip_acopf_set_instance(ctx.h, 0, None, None, None, None), EINVAL, ["sqphip_acopf_set_instance", "NLP"], ctx)
    _expect(L.sqphip_qcqp_set_instance(ctx.h, 0, None, None, None, None, None, None, None), EINVAL, ["sqphip_qcqp_set_instance", "QCQP"], ctx)
    _expect(L.sqphip_sqp_stream_begin(ctx.h, 4), EINVAL, ["sqphip_sqp_stream_begin", "NLP"], ctx)
    _expect(L.sqphip_qcqp_stream_begin(ctx.h, 4, 0), EINVAL, ["sqphip_qcqp_stream_begin", "QCQP"], ctx)
    R = NlpAffineRef(good)
    assert rel(ctx.acopf_eval(0, good.x0)["f"], R.f(good.x0)) <= 1e-13      # ... and it still evaluates
    ctx.close()
