"""The sparse factorable NLP in the batched device SQP loop (sqphip_nlp_attach / _set_instance, csrc/nlp_dev.hpp): the device
evaluator against the numpy reference (tests/nlp_ref.py) on generated and hand-made models, HS071 and generated batches
against the oracle (which runs on the same terms through ctypes callbacks), the generic path against the dedicated polar
ACOPF and QCQP paths, determinism, the Armijo probe and misuse."""
import dataclasses
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import sqpsolver_jl_amd as pkg                                        # noqa: E402
from sqpsolver_jl_amd.acopf_synth import acopf_layout, acopf_synth, contingency, CASES   # noqa: E402
from sqpsolver_jl_amd.nlp_terms import (COS, EXP, LOG, POW, SIN, from_polar_acopf, from_qcqp, make_nlp_terms,   # noqa: E402
                                        nlp_terms_layout, nlp_terms_scenario, nlp_terms_synth)
from sqpsolver_jl_amd.qcqp import qcqp_layout, qcqp_scenario, qcqp_synth   # noqa: E402
from oracle import oracle as O                                        # noqa: E402
from nlp_ref import GPU_SCENARIOS, GPU_SEED, NlpRef, OracleNlpTerms, first_term, hs071_terms   # noqa: E402
from qcqp_ref import coo_sum                                          # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-8
SQP_KW = dict(tol_infeas=1e-6, tol_residual=1e-4)
EINVAL, ESTATE = -1, -4


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


def _nlp_ctx(p, lay, batch, ps=None, **kw):
    ctx = _ctx(lay, batch, **kw)
    ctx.nlp_attach(p)
    for b in range(batch):
        ctx.nlp_set_instance(b, (ps or [p] * batch)[b])
    return ctx


def _results(ctx, b):
    return ctx.sqp_get(b), ctx.sqp_trace(b)


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


def _against_oracle(ctx, b, ro):
    rg, tr = _results(ctx, b)
    print("instance", b, "status", rg["status"], ro["status"], "iter", rg["iter"], ro["iter"], "x", rel(rg["x"], ro["x"]),
          "obj", abs(rg["obj_val"] - ro["obj_val"]))
    assert (rg["status"], rg["iter"]) == (ro["status"], ro["iter"]), b
    assert _same_decisions(ro, tr) and _ipm_counts_close(ro, tr), b
    assert rel(rg["x"], ro["x"]) < TOL and abs(rg["obj_val"] - ro["obj_val"]) <= TOL * max(1.0, abs(ro["obj_val"])), b
    return rg


# ---- 1. the evaluator against the reference
def test_evaluator_on_a_generated_model_with_per_instance_values():
    p = nlp_terms_synth(24, 14, seed=GPU_SEED)
    lay = nlp_terms_layout(p)
    ps = [nlp_terms_scenario(p, s, GPU_SEED) for s in range(3)]
    ctx = _nlp_ctx(p, lay, 3, ps)
    rng = np.random.default_rng(3)
    x = np.clip(p.x0 + 0.3 * rng.standard_normal(p.n), 0.25, 2.9); lam = rng.standard_normal(p.m)
    for b in range(3):
        _check_eval(ctx.acopf_eval(b, x, 1.3, lam), NlpRef(ps[b]), x, 1.3, lam, lay)
    # a NULL part keeps what the instance had
    c2 = ps[2].tcoef * 0.5
    ctx.nlp_set_instance(2, tcoef=c2)
    _check_eval(ctx.acopf_eval(2, x, 1.3, lam), NlpRef(dataclasses.replace(ps[2], tcoef=c2)), x, 1.3, lam, lay)
    assert ctx.acopf_eval(2, x, 1.3, lam)["f"] != ctx.acopf_eval(1, x, 1.3, lam)["f"]
    ctx.close()


# ---- 2. plan edges, evaluator only
def _edge_model():
    eight = [(1, POW, -2, 0.5, 0.3), (2, POW, -1, 1.0, 0.2), (3, SIN, 1, 2.0, 0.1), (4, COS, 1, -1.0, 0.3), (5, EXP, 1, 0.5, -0.2),
             (6, LOG, 1, 2.0, 0.5), (7, POW, 3, 1.0, -0.1), (8, POW, 5, 0.8, 0.0)]
    terms = [(1, 0.7, eight),                                  # exactly 8 factors, every kind
             (2, -1.3, [(9, POW, 1, 1.5, 0.2)]),               # one factor, linear with non-trivial a, b
             (0, 2.0, [(10, EXP, 1, 0.7, 0.1)]),               # variable 10: in the objective only
             (0, 1.1, [(1, POW, 2), (9, POW, 1)])]
    p = make_nlp_terms(10, 2, 0, terms, g0=[0.4, -0.6], f0=0.25, xL=np.full(10, 0.2), xU=np.full(10, 3.0),
                       gL=[-5.0, -5.0], gU=[5.0, 5.0], x0=np.linspace(0.7, 1.3, 10))
    assert (1 + p.m + len(p.trow)) % 2 == 1                   # an odd value count: the blocks are padded
    lay = nlp_terms_layout(p)
    # a Jacobian and a Hessian slot that no term needs, and a copy of the first Hessian slot
    lay = dataclasses.replace(lay, jrow=np.append(lay.jrow, 2), jcol=np.append(lay.jcol, 3),
                              hrow=np.concatenate([lay.hrow, [10], lay.hrow[:1]]), hcol=np.concatenate([lay.hcol, [9], lay.hcol[:1]]))
    return p, lay


def test_evaluator_at_the_plan_edges():
    p, lay = _edge_model()
    p1 = dataclasses.replace(p, tcoef=p.tcoef * np.array([1.2, 0.8, -1.0, 0.5]), g0=p.g0 + 0.1, f0=-0.5)
    ctx = _nlp_ctx(p, lay, 2, [p, p1])
    rng = np.random.default_rng(8)
    x = rng.uniform(0.5, 1.6, p.n); lam = rng.standard_normal(p.m)
    for b, q in enumerate((p, p1)):
        ev = ctx.acopf_eval(b, x, 1.3, lam)
        _check_eval(ev, NlpRef(q), x, 1.3, lam, lay)
        _check_eval(ev, NlpRef(q), x, 1.3, lam, lay, summed=True)
        assert ev["jval"][-1] == 0.0 and ev["hval"][-2] == 0.0 and ev["hval"][-1] == 0.0     # unused slots, the copy of a slot
        assert np.all(ev["jval"][:-1] != 0.0) and ev["grad"][9] != 0.0 and np.all(ev["grad"][1:8] == 0.0)
    ctx.close()


def test_evaluator_beyond_one_stride_of_the_thread_loops():
    p = nlp_terms_synth(600, 500, seed=2)
    lay = nlp_terms_layout(p)
    assert len(p.trow) > 1024 and len(lay.jrow) > 1024 and len(p.fvar) > 2048
    ctx = _nlp_ctx(p, lay, 1)
    rng = np.random.default_rng(5)
    x = np.clip(p.x0 + 0.2 * rng.standard_normal(p.n), 0.25, 2.9); lam = rng.standard_normal(p.m)
    _check_eval(ctx.acopf_eval(0, x, 1.3, lam), NlpRef(p), x, 1.3, lam, lay)
    ctx.close()


# ---- 3. HS071 on the device loop
HS_STARTS = [(1, 5, 5, 1), (2, 4, 4, 2), (1.5, 4.5, 3.5, 1.5), (3, 3, 3, 3)]


@pytest.mark.parametrize("kkt_mode", [2, 1])
def test_hs071_on_the_device_loop_matches_oracle_and_pin(kkt_mode):
    import json
    p, lay = hs071_terms()
    ps = [dataclasses.replace(p, x0=np.array(s, float)) for s in HS_STARTS]
    ctx = _nlp_ctx(p, lay, 4, ps, kkt_mode=kkt_mode, literal_quirks=0)
    ctx.sqp_reset(); ctx.sqp_run(0)
    pin = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_pins.json")))["reference_pins"]["hs071"]
    try:
        for b, s in enumerate(HS_STARTS):
            ro = O.sqp_solve(O.problem_hs071(), O.default_options(literal_quirks=0, **_lin(kkt_mode)), x0=np.array(s, float))
            assert ro["status"] == 0
            rg = _against_oracle(ctx, b, ro)
            assert np.allclose(rg["x"], pin["x"], rtol=pin["rtol"], atol=1e-8) and abs(rg["obj_val"] - pin["f"]) <= pin["rtol"] * pin["f"]
    finally:
        O.set_kkt_order(None)
    ctx.close()


# ---- 4. a generated batch against the oracle
@pytest.mark.parametrize("kkt_mode", [2, 1])
def test_generated_batch_matches_oracle(kkt_mode):
    p = nlp_terms_synth(24, 14, seed=GPU_SEED)
    lay = nlp_terms_layout(p)
    ps = [nlp_terms_scenario(p, s, GPU_SEED) for s in GPU_SCENARIOS]
    kw = dict(max_iter=30, literal_quirks=0, **SQP_KW)
    ctx = _nlp_ctx(p, lay, 4, ps, kkt_mode=kkt_mode, **kw)
    ctx.sqp_reset(); ctx.sqp_run(0)
    try:
        for b in range(4):
            ro = O.sqp_solve(OracleNlpTerms(ps[b], lay), O.default_options(**_lin(kkt_mode), **kw))
            assert ro["status"] == 0
            _against_oracle(ctx, b, ro)
    finally:
        O.set_kkt_order(None)
    ctx.close()


# ---- 5. generic path = dedicated path
def _same_runs(cg, cd, batch):
    for c in (cg, cd):
        c.sqp_reset(); c.sqp_run(0)
    assert np.array_equal(cg.sqp_status()[0], cd.sqp_status()[0]) and np.array_equal(cg.sqp_status()[1], cd.sqp_status()[1])
    for b in range(batch):
        (rg, tg), (rd, td) = _results(cg, b), _results(cd, b)
        print("instance", b, "status", rg["status"], "iter", rg["iter"], "x", rel(rg["x"], rd["x"]))
        assert (rg["status"], rg["iter"]) == (rd["status"], rd["iter"]), b
        assert [(t["iter"], t["accepted"], t["fr"], t["sub_status"]) for t in tg] == \
               [(t["iter"], t["accepted"], t["fr"], t["sub_status"]) for t in td], b
        assert rel(rg["x"], rd["x"]) < TOL, b


def test_generic_path_equals_dedicated_polar_path_on_contingencies():
    nb, ng, nl, seed = CASES["case14"]
    base = acopf_synth(nb, ng, nl, seed)
    nets = [base, contingency(base, 2, seed), contingency(base, 5, seed)]
    lays = [acopf_layout(nt) for nt in nets]
    ps = [from_polar_acopf(nt, ly) for nt, ly in zip(nets, lays)]
    kw = dict(max_iter=60, use_soc=1, literal_quirks=0, **SQP_KW)
    cg = _ctx(lays[0], 3, **kw); cg.nlp_attach(ps[0])
    cd = _ctx(lays[0], 3, **kw); cd.acopf_attach(nets[0], lays[0])
    for b in range(3):
        cg.nlp_set_instance(b, ps[b]); cd.acopf_set_instance(b, nets[b], lays[b])
    # the two evaluators agree on the summed COO entries (1e-12: two formulas for cos(th_f - th_t), tests/test_nlp_cpu.py)
    rng = np.random.default_rng(2)
    x = lays[0].x0 + 0.05 * rng.standard_normal(lays[0].n); lam = rng.standard_normal(lays[0].m)
    eg, ed = cg.acopf_eval(1, x, 0.7, lam), cd.acopf_eval(1, x, 0.7, lam)
    J = lambda v: coo_sum(v, lays[0].jrow, lays[0].jcol, lays[0].n)
    H = lambda v: coo_sum(v, lays[0].hrow, lays[0].hcol, lays[0].n, lower=True)
    assert rel(eg["f"], ed["f"]) <= 1e-12 and rel(eg["grad"], ed["grad"]) <= 1e-12 and rel(eg["g"], ed["g"]) <= 1e-12
    assert rel(J(eg["jval"]), J(ed["jval"])) <= 1e-12 and rel(H(eg["hval"]), H(ed["hval"])) <= 1e-12
    _same_runs(cg, cd, 3)
    cg.close(); cd.close()


def test_generic_path_equals_the_qcqp_path():
    q = qcqp_synth(24, 14, seed=5)
    lay = qcqp_layout(q)
    qs = [qcqp_scenario(q, s, 5) for s in range(3)]
    ps = [from_qcqp(s) for s in qs]
    kw = dict(max_iter=30, literal_quirks=0, **SQP_KW)
    cg = _ctx(lay, 3, **kw); cg.nlp_attach(ps[0])
    cd = _ctx(lay, 3, **kw); cd.qcqp_attach(q)
    for b in range(3):
        cg.nlp_set_instance(b, ps[b]); cd.qcqp_set_instance(b, qs[b])
    _same_runs(cg, cd, 3)
    cg.close(); cd.close()


# ---- 6. determinism
def test_same_instance_in_two_slots_and_two_runs_is_bit_identical():
    p = nlp_terms_synth(24, 14, seed=GPU_SEED)
    lay = nlp_terms_layout(p)
    ps = [nlp_terms_scenario(p, s, GPU_SEED) for s in (1, 2, 1)]           # slots 0 and 2: the same instance
    ctx = _nlp_ctx(p, lay, 3, ps, max_iter=30, literal_quirks=0, **SQP_KW)
    outs = []
    for _ in range(2):
        ctx.sqp_reset(); ctx.sqp_run(0)
        outs.append([(ctx.sqp_get(b), ctx.sqp_trace(b)) for b in (0, 2)])
    ctx.close()
    ref = outs[0][0]
    assert ref[0]["status"] == 0
    for rg, tr in outs[0][1:] + outs[1]:
        for k in ("x", "g", "mult_g", "mult_x_L", "mult_x_U"):
            assert np.array_equal(rg[k], ref[0][k]), k
        assert (rg["obj_val"], rg["status"], rg["iter"]) == (ref[0]["obj_val"], ref[0]["status"], ref[0]["iter"])
        assert tr == ref[1]


# ---- 7. the Armijo probe
def test_armijo_on_an_nlp_context_matches_a_backtracking_loop_over_the_reference():
    p = nlp_terms_synth(24, 14, seed=GPU_SEED)
    lay = nlp_terms_layout(p)
    ps = [p, nlp_terms_scenario(p, 1, GPU_SEED)]
    ctx = _nlp_ctx(p, lay, 2, ps)
    R = NlpRef(ps[1])
    rng = np.random.default_rng(6)
    x = np.clip(p.x0 + 0.1 * rng.standard_normal(p.n), 0.3, 2.8)
    eta, tau, min_alpha = 0.4, 0.9, 1e-6
    seen = set()
    for mu, fr, scale, slope in ((0.0, False, 0.2, None), (0.0, False, 1.5, None), (5.0, False, 1.0, 1.0), (1.0, True, 1.0, 1e6)):
        step = -scale * R.grad(x) if mu == 0.0 else scale * rng.standard_normal(p.n)
        step = np.maximum(step, 0.25 - x)                                  # x + alpha step stays inside every factor's domain
        phi = lambda a: (0.0 if fr else R.f(x + a * step)) + (1.0 if fr else mu) * O.norm_violations(
            R.g(x + a * step), p.gL, p.gU, x + a * step, p.xL, p.xU, 1)
        phi0 = phi(0.0)
        # the true slope of f along a descent step, or a claimed one (1e6: no step length delivers it -- backtracks to the end)
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


# ---- 8. misuse
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
    _expect(_attach_rc(ctx, p), code, words, ctx)
    ctx.close()


def _with_factor(p, k, **kw):
    out = dataclasses.replace(p, **{name: getattr(p, name).copy() for name in kw})
    for name, v in kw.items():
        getattr(out, name)[k] = v
    return out


def test_misuse_is_refused_with_a_message_naming_the_term():
    p = nlp_terms_synth(16, 10, seed=2)
    lay = nlp_terms_layout(p)
    t = int(np.flatnonzero((p.trow > p.num_linear) & (np.diff(p.tptr) >= 2))[0])       # a term of a nonlinear row with two factors
    k = int(p.tptr[t]); T = f"term {t + 1}"
    _refused(lay, _with_factor(p, k, fvar=p.n + 1), [T, "factor 1", "out of range"])
    _refused(lay, _with_factor(p, t, trow=p.m + 1), [T, "out of range"])
    _refused(lay, _with_factor(p, k + 1, fkind=7), [T, "factor 2", "kind"])
    _refused(lay, _with_factor(_with_factor(p, k, fkind=POW), k, fexp=0), [T, "factor 1", "exponent"])
    _refused(lay, _with_factor(_with_factor(p, k, fkind=POW), k, fexp=33), [T, "factor 1", "exponent"])
    _refused(lay, _with_factor(_with_factor(p, k, fkind=POW), k, fexp=-33), [T, "factor 1", "exponent"])
    _refused(lay, _with_factor(p, k + 1, fvar=p.fvar[k]), [T, "factor 2", "twice"])
    # a term with no factors, a term with nine
    tp = p.tptr.copy(); tp[t + 1:] -= (p.tptr[t + 1] - p.tptr[t])
    cut = slice(int(p.tptr[t]), int(p.tptr[t + 1]))
    empty = dataclasses.replace(p, tptr=tp, **{n_: np.delete(getattr(p, n_), cut) for n_ in ("fvar", "fkind", "fexp", "fscale", "fshift")})
    _refused(lay, empty, [T, "no factors"])
    nine = make_nlp_terms(p.n, p.m, p.num_linear, [(p.m, 1.0, [(j, POW) for j in range(1, 10)])])
    _refused(lay, nine, ["term 1", "8 factors"])
    # a linear row takes single plain factors only
    tl = int(np.flatnonzero(p.trow == 1)[0]); kl = int(p.tptr[tl])
    _refused(lay, _with_factor(p, kl, fexp=2), [f"term {tl + 1}", "linear"])
    _refused(lay, _with_factor(p, kl, fscale=2.0), [f"term {tl + 1}", "linear"])
    _refused(lay, _with_factor(p, kl, fkind=SIN), [f"term {tl + 1}", "linear"])
    # a Jacobian slot missing
    j = int(np.flatnonzero((lay.jrow == p.trow[t]) & (lay.jcol == p.fvar[k]))[0])
    Tj = first_term(p, lambda row, vs, cv: row == p.trow[t] and p.fvar[k] in vs)
    _refused(dataclasses.replace(lay, jrow=np.delete(lay.jrow, j), jcol=np.delete(lay.jcol, j)), p, [f"term {Tj} ", "Jacobian"])
    # a Hessian slot missing: the pair of two factors of a term, the diagonal of a curved factor
    v, w = int(p.fvar[k]), int(p.fvar[k + 1])
    h = int(np.flatnonzero((lay.hrow == max(v, w)) & (lay.hcol == min(v, w)))[0])
    Th = first_term(p, lambda row, vs, cv: v in vs and w in vs)
    _refused(dataclasses.replace(lay, hrow=np.delete(lay.hrow, h), hcol=np.delete(lay.hcol, h)), p, [f"term {Th} ", "Hessian"])
    kc = int(np.flatnonzero((p.fkind != POW) & (p.trow[np.repeat(np.arange(len(p.trow)), np.diff(p.tptr))] > 0))[0])
    h = int(np.flatnonzero((lay.hrow == p.fvar[kc]) & (lay.hcol == p.fvar[kc]))[0])
    Th = first_term(p, lambda row, vs, cv: any(a == p.fvar[kc] and c for a, c in zip(vs, cv)))
    _refused(dataclasses.replace(lay, hrow=np.delete(lay.hrow, h), hcol=np.delete(lay.hcol, h)), p, [f"term {Th} ", "Hessian"])
    # without a Hessian structure only the Jacobian is checked
    ctx = _ctx(dataclasses.replace(lay, hrow=lay.hrow[:0], hcol=lay.hcol[:0]), 1)
    assert _attach_rc(ctx, p) == 0
    ctx.close()
    # a refused attach leaves the context unattached: a good one goes in, a second one is refused
    ctx = _ctx(lay, 1)
    _expect(_attach_rc(ctx, _with_factor(p, k, fvar=0)), EINVAL, [T, "out of range"], ctx)
    ctx.nlp_attach(p)
    _expect(_attach_rc(ctx, p), ESTATE, ["already"], ctx)
    # the entry points of the other evaluators and both scenario queues on an NLP context
    L = ctx.L
    z = np.zeros(max(p.n, p.m)); d = z.ctypes.data_as(L.sqphip_set_bounds.argtypes[2])
    _expect(L.sqphip_acopf_set_instance(ctx.h, 0, None, None, None, None), EINVAL, ["sqphip_acopf_set_instance", "NLP"], ctx)
    _expect(L.sqphip_acopf_set_shunts(ctx.h, 0, None, None, None), EINVAL, ["sqphip_acopf_set_shunts", "NLP"], ctx)
    _expect(L.sqphip_acopf_set_dclines(ctx.h, 0, None), EINVAL, ["sqphip_acopf_set_dclines", "NLP"], ctx)
    _expect(L.sqphip_qcqp_set_instance(ctx.h, 0, None, None, None, None, None, None, None), EINVAL, ["sqphip_qcqp_set_instance", "QCQP"], ctx)
    _expect(L.sqphip_sqp_stream_begin(ctx.h, 4), EINVAL, ["sqphip_sqp_stream_begin", "NLP"], ctx)
    _expect(L.sqphip_sqp_stream_set(ctx.h, 0, d, d, d, d, d, d, d, d), EINVAL, ["sqphip_sqp_stream_set", "NLP"], ctx)
    _expect(L.sqphip_qcqp_stream_begin(ctx.h, 4, 0), EINVAL, ["sqphip_qcqp_stream_begin", "QCQP"], ctx)
    _expect(L.sqphip_qcqp_stream_set(ctx.h, 0, d, d, d, d, None, None, None, None, None, None, d), EINVAL, ["sqphip_qcqp_stream_set", "QCQP"], ctx)
    # ... and the context still evaluates
    assert np.isfinite(ctx.acopf_eval(0, p.x0)["f"])
    ctx.close()


def test_acopf_only_entry_points_are_refused_on_a_dense_context():
    from sqpsolver_jl_amd.dense_synth import dense_synth, dense_layout
    nlp = dense_synth(16, 4, 7)
    lay = dense_layout(nlp)
    ctx = _ctx(lay, 1)
    ctx.dense_attach(nlp)
    ctx.dense_set_instance(0, nlp, lay)
    L = ctx.L
    z = np.zeros(max(lay.n, lay.m)); d = z.ctypes.data_as(L.sqphip_set_bounds.argtypes[2])
    _expect(L.sqphip_acopf_set_instance(ctx.h, 0, d, d, d, d), EINVAL, ["sqphip_acopf_set_instance", "dense"], ctx)
    _expect(L.sqphip_acopf_set_shunts(ctx.h, 0, None, None, None), EINVAL, ["sqphip_acopf_set_shunts", "dense"], ctx)
    _expect(L.sqphip_acopf_set_dclines(ctx.h, 0, None), EINVAL, ["sqphip_acopf_set_dclines", "dense"], ctx)
    _expect(L.sqphip_sqp_stream_begin(ctx.h, 4), EINVAL, ["sqphip_sqp_stream_begin", "dense"], ctx)
    _expect(L.sqphip_sqp_stream_set(ctx.h, 0, d, d, d, d, d, d, d, d), EINVAL, ["sqphip_sqp_stream_set", "dense"], ctx)
    _expect(L.sqphip_qcqp_stream_begin(ctx.h, 4, 0), EINVAL, ["sqphip_qcqp_stream_begin", "QCQP"], ctx)
    _expect(L.sqphip_qcqp_set_instance(ctx.h, 0, None, None, None, None, None, None, None), EINVAL, ["sqphip_qcqp_set_instance", "QCQP"], ctx)
    # the context is unharmed
    x = np.random.default_rng(1).uniform(-0.5, 0.5, nlp.n)
    assert np.isfinite(ctx.acopf_eval(0, x, 1.0, np.zeros(nlp.m))["f"])
    ctx.close()
