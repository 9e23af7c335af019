"""Dense data blocks of a factorable NLP in the batched device SQP loop (sqphip_nlp_add_block, csrc/nlp_block_dev.hpp): the
evaluator against the 50-digit reference and its forward error bound (tests/nlp_block_ref.py) at the shape edges, two blocks
on overlapping columns, a model through both paths, cross-validation folds beyond the old limits, the scenario queue against
the batch, a block under rows against the oracle, slot independence and every refusal.  tests/test_nlp_block_cpu.py holds
the oracle's and Newton's word for the solved cases."""
import ctypes as C
import dataclasses
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import sqpsolver_jl_amd as pkg                                        # noqa: E402
from sqpsolver_jl_amd.acopf_synth import acopf_layout, acopf_synth, CASES   # noqa: E402
from sqpsolver_jl_amd.nlp_terms import (POW, POWR, SOFTPLUS, NlpBlock, logistic_block_model, make_nlp_terms,   # noqa: E402
                                        nlp_terms_layout, poisson_block_model)
from sqpsolver_jl_amd.qcqp import qcqp_layout, qcqp_synth              # noqa: E402
from oracle import oracle as O                                        # noqa: E402
from nlp_block_ref import (EDGE_CASES, SQP_TIGHT, NlpBlockRef, OracleBlockTerms, both_paths_case, check_outputs,   # noqa: E402
                           edge_model, folds_case, newton_logistic, newton_poisson, poisson_case, rows_case, two_block_model)

pytestmark = pytest.mark.gpu
TOL = 1e-8
EINVAL, ESTATE = -1, -4
FULL = ("x", "g", "mult_g", "mult_x_L", "mult_x_U")
_dp = C.POINTER(C.c_double)


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


def _lin(kkt_mode):
    return dict(kkt_mode=2) if kkt_mode == 2 else dict(kkt_mode=1, kkt_tile_order=1)


def _d(a):
    return None if a is None else a.ctypes.data_as(_dp)


def _with(p, k, weight=None, shift=None):
    """p with other data in block k"""
    b = p.blocks[k]
    nb = dataclasses.replace(b, weight=b.weight if weight is None else weight, shift=b.shift if shift is None else shift)
    return dataclasses.replace(p, blocks=p.blocks[:k] + [nb] + p.blocks[k + 1:])


def _fg_only(ctx, inst, x):
    """the f / g-only call: gradient, Jacobian and Hessian pointers NULL"""
    f = C.c_double(); g = np.zeros(ctx.m); xx = np.ascontiguousarray(x, dtype=np.float64)
    ctx._ck(ctx.L.sqphip_acopf_eval(ctx.h, inst, _d(xx), 1.0, None, C.byref(f), None, _d(g), None, None))
    return f.value, g


def _same_result(ra, rb, where):
    for k in FULL:
        assert np.array_equal(ra[k], rb[k]), (where, k)
    assert (ra["obj_val"], ra["status"], ra["iter"]) == (rb["obj_val"], rb["status"], rb["iter"]), where


def _visibly_different(xs):
    return min(np.abs(a - b).max() for a, b in itertools.combinations(xs, 2)) > 1e-3


# ---- 1. the evaluator at the shape edges
@pytest.mark.parametrize("N,d,kind,e", EDGE_CASES, ids=[f"N{N}-d{d}-k{k}e{e}" for N, d, k, e in EDGE_CASES])
def test_evaluator_at_the_shape_edges(N, d, kind, e):
    p, lay, inst = edge_model(N, d, kind, e)
    ctx = _ctx(lay, 3)
    ctx.nlp_attach(p)
    for b, (w, s) in enumerate(inst):
        ctx.nlp_set_instance(b, p, weight=w, shift=s)
    rng = np.random.default_rng(N + d)
    x = rng.uniform(0.6, 1.4, p.n); lam = np.array([0.8]); sigma = 0.7
    fs = []
    for b, (w, s) in enumerate(inst):
        ev = ctx.acopf_eval(b, x, sigma, lam)
        val, bnd = NlpBlockRef(_with(p, 0, w, s)).want(x, sigma, lam, lay)
        check_outputs(ev, val, bnd, f"(N, d, kind, e) = {(N, d, kind, e)} instance {b}")
        assert np.all(ev["hval"][-2:] == 0.0)                         # the copies of a slot: the first copy owns the entry
        f, g = _fg_only(ctx, b, x)
        assert f == ev["f"] and np.array_equal(g, ev["g"])
        fs.append(ev["f"])
    assert len(set(fs)) == 3                                          # every slot reads its own weights and shifts
    ctx.close()


# ---- 2. two blocks on overlapping columns
def test_two_blocks_on_overlapping_columns_share_slots_and_gradient_entries():
    p, lay = two_block_model()
    rng = np.random.default_rng(2)
    w1, s0 = rng.uniform(0.0, 1.0, 22), 0.1 * rng.standard_normal(37)
    ctx = _ctx(lay, 2)
    ctx.nlp_attach(p)
    ctx.nlp_set_instance(1, p, weight={1: w1}, shift={0: s0})
    x = rng.uniform(-1.0, 1.0, p.n); lam = np.zeros(0)
    for b, q in enumerate((p, _with(_with(p, 1, weight=w1), 0, shift=s0))):
        ev = ctx.acopf_eval(b, x, 1.3, lam)
        val, bnd = NlpBlockRef(q).want(x, 1.3, lam, lay)
        check_outputs(ev, val, bnd, f"two blocks, instance {b}")
    # each block alone moves the shared entries: both contribute
    only0 = NlpBlockRef(p).want(x, 1.3, lam, lay, blocks=p.blocks[:1])[0]
    assert np.abs(only0["grad"][[2, 4, 6]] - ev["grad"][[2, 4, 6]]).min() > 1e-3
    ctx.close()


# ---- 3. the same model by both paths
def test_block_and_per_point_terms_agree_and_reach_the_scipy_optimum():
    import scipy.optimize
    X, y, reg, pb, pt = both_paths_case()
    layb, layt = nlp_terms_layout(pb), nlp_terms_layout(pt)
    assert np.array_equal(layb.hrow, layt.hrow) and np.array_equal(layb.hcol, layt.hcol)
    cb, ct = _ctx(layb, 1, **SQP_TIGHT), _ctx(layt, 1, **SQP_TIGHT)
    cb.nlp_attach(pb); cb.nlp_set_instance(0, pb)
    ct.nlp_attach(pt); ct.nlp_set_instance(0, pt)
    x = np.random.default_rng(6).uniform(-1.0, 1.0, 6)
    eb, et = cb.acopf_eval(0, x, 0.9, np.zeros(0)), ct.acopf_eval(0, x, 0.9, np.zeros(0))
    val, bnd = NlpBlockRef(pb).want(x, 0.9, np.zeros(0), layb)
    check_outputs(eb, val, bnd, "block path")
    check_outputs(et, val, bnd, "per-point terms")
    for k in ("f", "grad", "hval"):                                   # within the sum of the two bounds
        lim = 2.0 * (4.0 * np.asarray(bnd[k]) + 1e-13 * np.abs(val[k]).max())
        assert np.all(np.abs(np.asarray(eb[k]) - np.asarray(et[k])) <= lim), k
    loss = lambda w: float(np.sum(np.logaddexp(0.0, X @ w) - y * (X @ w)) + 0.5 * reg * (w @ w))
    want = scipy.optimize.minimize(loss, np.zeros(6), method="BFGS", options=dict(gtol=1e-10)).x
    for c in (cb, ct):
        c.sqp_reset(); c.sqp_run(0)
        r = c.sqp_get(0)
        print("status", r["status"], "iter", r["iter"], "x", np.abs(r["x"] - want).max())
        assert r["status"] == 0 and np.abs(r["x"] - want).max() <= 1e-6
        c.close()


# ---- 4. folds beyond the old limit: 20 features, 150 points
@pytest.mark.parametrize("kkt_mode", [1, 2])
def test_four_folds_of_a_150_by_20_fit_in_one_batch(kkt_mode):
    X, y, reg, W = folds_case()
    want = [newton_logistic(X, y, reg, w)[0] for w in W]
    assert _visibly_different(want)                                   # a context that ignores the weights cannot pass
    p = logistic_block_model(X, y, reg, W[0])
    ctx = _ctx(nlp_terms_layout(p), 4, **_lin(kkt_mode), **SQP_TIGHT)
    ctx.nlp_attach(p)
    for f in range(4):
        ctx.nlp_set_instance(f, p, weight=W[f])
    ctx.sqp_reset(); ctx.sqp_run(0)
    out = [ctx.sqp_get(f) for f in range(4)]
    ctx.close()
    print("status", [r["status"] for r in out], "iter", [r["iter"] for r in out], "err", [np.abs(r["x"] - w).max() for r, w in zip(out, want)])
    assert all(r["status"] == 0 for r in out)
    for f in range(4):
        assert np.abs(out[f]["x"] - want[f]).max() <= 1e-6, f
    assert _visibly_different([r["x"] for r in out])


# ---- 5. the scenario queue: six Poisson bootstraps on two slots
def test_queue_of_poisson_bootstraps_equals_the_batch_and_newton():
    X, c, reg, W = poisson_case()
    ps = [poisson_block_model(X, c, reg, w) for w in W]
    p1 = poisson_block_model(X, c, reg)                               # unit weights: what the add call sets
    lay = nlp_terms_layout(p1)
    want = [newton_poisson(X, c, reg, w)[0] for w in W] + [newton_poisson(X, c, reg, np.ones(150))[0]]
    ctx = _ctx(lay, 2, kkt_mode=2, **SQP_TIGHT)
    ctx.nlp_attach(p1)
    ctx.nlp_stream_begin(6, keep_multipliers=True)
    for s in range(6):
        ctx.nlp_stream_set(s, tcoef=ps[s].tcoef, x0=p1.x0)
        ctx.nlp_stream_set_block(s, 0, weight=W[s])
    ctx.nlp_stream_set(5, tcoef=p1.tcoef, x0=p1.x0)                   # alone: the add call's weights are back
    ctx.stream_run()
    got = [ctx.stream_get_full(s) for s in range(6)]
    ctx.close()
    ps[5], W5 = p1, np.ones(150)
    ref = _ctx(lay, 2, kkt_mode=2, **SQP_TIGHT)
    ref.nlp_attach(p1)
    for s0 in (0, 2, 4):
        for b in range(2):
            ref.nlp_set_instance(b, ps[s0 + b])
        ref.sqp_reset(); ref.sqp_run(0)
        for b in range(2):
            s = s0 + b
            r = ref.sqp_get(b)
            w = want[6] if s == 5 else want[s]
            print("scenario", s, "status", got[s]["status"], "iter", got[s]["iter"], "err", np.abs(got[s]["x"] - w).max())
            _same_result(got[s], r, ("scenario", s))
            assert got[s]["status"] == 0 and np.abs(got[s]["x"] - w).max() <= 1e-6, s
    ref.close()
    assert np.abs(want[5] - want[6]).max() > 1e-3                     # (the restored weights are visible)


# ---- 6. a block under rows, against the oracle
def test_least_squares_block_under_rows_matches_the_oracle():
    p, lay, shifts = rows_case()
    ctx = _ctx(lay, 3, kkt_mode=2, **SQP_TIGHT)
    ctx.nlp_attach(p)
    for b in range(3):
        ctx.nlp_set_instance(b, p, shift=shifts[b])
    ctx.sqp_reset(); ctx.sqp_run(0)
    try:
        for b in range(3):
            ro = O.sqp_solve(OracleBlockTerms(_with(p, 0, shift=shifts[b]), lay), O.default_options(kkt_mode=2, **SQP_TIGHT))
            assert ro["status"] == 0
            rg, tr = ctx.sqp_get(b), ctx.sqp_trace(b)
            print("instance", b, "status", rg["status"], ro["status"], "iter", rg["iter"], ro["iter"], "x", rel(rg["x"], ro["x"]),
                  "obj", abs(rg["obj_val"] - ro["obj_val"]), "multipliers", [rel(rg[k], ro[k]) for k in FULL[2:]])
            assert (rg["status"], rg["iter"]) == (ro["status"], ro["iter"]), b
            assert _decisions(ro["trace"]) == _decisions(tr) and _ipm_counts_close(ro, tr), b
            assert rel(rg["x"], ro["x"]) < TOL and abs(rg["obj_val"] - ro["obj_val"]) <= TOL * max(1.0, abs(ro["obj_val"])), b
            assert (np.abs(rg["x"] - p.xL) < 1e-7).any() or (np.abs(rg["x"] - p.xU) < 1e-7).any(), b
            # multipliers through sqp_get: those of the last sub-problem, which both sides solve to ipm_tol from iterates
            # 1e-8 apart -- 1e-6 leaves two digits for the conditioning of that sub-problem
            assert all(rel(rg[k], ro[k]) <= 1e-6 for k in FULL[2:]), b
    finally:
        O.set_kkt_order(None)
    ctx.close()


# ---- 7. slot independence
def test_an_instance_does_not_depend_on_its_slot_its_neighbours_the_run_or_the_groups():
    X, y, reg, W = folds_case()
    p = logistic_block_model(X, y, reg, W[0])
    lay = nlp_terms_layout(p)
    order = (0, 1, 2, 0)                                              # slots 0 and 3: the same instance, other neighbours

    def run(ctx):
        ctx.sqp_reset(); ctx.sqp_run(0)
        return [(ctx.sqp_get(b), ctx.sqp_trace(b)) for b in range(4)]

    def make():
        ctx = _ctx(lay, 4, kkt_mode=2, **SQP_TIGHT)
        ctx.nlp_attach(p)
        for b, f in enumerate(order):
            ctx.nlp_set_instance(b, p, weight=W[f])
        return ctx

    ctx = make()
    runs = [run(ctx), run(ctx)]
    assert ctx.counters()["n_groups"] == 1
    ctx.close()
    assert all(r[0]["status"] == 0 for r in runs[0])
    _same_result(runs[0][0][0], runs[0][3][0], "slots 0 and 3")
    assert runs[0][0][1] == runs[0][3][1]
    assert not np.array_equal(runs[0][0][0]["x"], runs[0][1][0]["x"])
    for b in range(4):
        _same_result(runs[0][b][0], runs[1][b][0], ("second run", b))
        assert runs[0][b][1] == runs[1][b][1]
    os.environ["SQPHIP_GROUPS"] = "2"
    try:
        ctx = make()
        grouped = run(ctx)
        assert ctx.counters()["n_groups"] == 2
        ctx.close()
    finally:
        del os.environ["SQPHIP_GROUPS"]
    for b in range(4):
        _same_result(runs[0][b][0], grouped[b][0], ("two groups", b))
        assert runs[0][b][1] == grouped[b][1]


# ---- 8. refusals
def _expect(rc, code, words, ctx):
    msg = ctx.L.sqphip_last_error(ctx.h).decode()
    assert rc == code, (rc, msg)
    assert all(w in msg for w in words), msg


def test_refusals():
    n = 6
    terms = [(0, 1.0, [(j + 1, POW, 2)]) for j in range(n)]
    p = make_nlp_terms(n, 0, 0, terms, xL=np.full(n, -1.0), xU=np.ones(n), blocks=[NlpBlock(SOFTPLUS, [2, 4, 5], np.ones((3, 3)))])
    lay = nlp_terms_layout(p)
    who = "sqphip_nlp_add_block"
    A = np.ones((4, 3)); cols = np.array([2, 4, 5], dtype=np.int64)
    lp = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))

    def add(ctx, kind=9, e=1, par=0.0, N=4, d=3, c=cols, a=A):
        return ctx.L.sqphip_nlp_add_block(ctx.h, kind, e, par, N, d, lp(np.ascontiguousarray(c, dtype=np.int64)), _d(a), None, None, None)

    ctx = _ctx(lay, 2)
    _expect(add(ctx), EINVAL, [who, "no factorable NLP"], ctx)       # before any attach
    ctx.nlp_attach(dataclasses.replace(p, blocks=[]))
    big = np.ones((1, 129))
    _expect(add(ctx, d=0), EINVAL, [who, "block 1", "d = 0"], ctx)
    _expect(add(ctx, d=129, c=np.arange(1, 130), a=big), EINVAL, [who, "block 1", "d = 129"], ctx)
    _expect(add(ctx, N=0), EINVAL, [who, "block 1", "N = 0"], ctx)
    _expect(add(ctx, N=2 ** 31 // 3 + 1), EINVAL, [who, "block 1", "too large"], ctx)
    _expect(add(ctx, c=[2, 7, 5]), EINVAL, [who, "block 1", "column 2", "variable 7", "out of range"], ctx)
    _expect(add(ctx, c=[2, 4, 2]), EINVAL, [who, "block 1", "column 3", "variable 2", "twice"], ctx)
    _expect(add(ctx, kind=11), EINVAL, [who, "block 1", "kind 11"], ctx)
    _expect(add(ctx, kind=0, e=1), EINVAL, [who, "block 1", "plain linear"], ctx)
    _expect(add(ctx, kind=0, e=0), EINVAL, [who, "block 1", "exponent 0"], ctx)
    _expect(add(ctx, kind=0, e=33), EINVAL, [who, "block 1", "exponent 33"], ctx)
    _expect(add(ctx, kind=POWR, par=0.0), EINVAL, [who, "block 1", "real exponent"], ctx)
    _expect(add(ctx, kind=POWR, par=float("inf")), EINVAL, [who, "block 1", "real exponent"], ctx)
    _expect(add(ctx, c=[2, 4, 6]), EINVAL, [who, "block 1", "entry (3, 1)", "Hessian entry (6, 2)"], ctx)
    for k in range(4):
        assert add(ctx) == 0
    _expect(add(ctx), EINVAL, [who, "block 5", "at most 4"], ctx)
    w = np.ones(4)
    si, ss = "sqphip_nlp_set_instance_block", "sqphip_nlp_stream_set_block"
    _expect(ctx.L.sqphip_nlp_set_instance_block(ctx.h, 0, 4, _d(w), None), EINVAL, [si, "block 4"], ctx)
    _expect(ctx.L.sqphip_nlp_set_instance_block(ctx.h, 0, -1, _d(w), None), EINVAL, [si, "block -1"], ctx)
    _expect(ctx.L.sqphip_nlp_set_instance_block(ctx.h, 2, 0, _d(w), None), EINVAL, [si, "instance 2"], ctx)
    assert ctx.L.sqphip_nlp_set_instance_block(ctx.h, 1, 3, _d(w), None) == 0
    _expect(ctx.L.sqphip_nlp_stream_set_block(ctx.h, 0, 0, _d(w), None), EINVAL, [ss, "sqphip_nlp_stream_begin"], ctx)
    ctx.nlp_stream_begin(3)
    _expect(ctx.L.sqphip_nlp_stream_set_block(ctx.h, 3, 0, _d(w), None), EINVAL, [ss, "scenario 3"], ctx)
    _expect(ctx.L.sqphip_nlp_stream_set_block(ctx.h, 0, 4, _d(w), None), EINVAL, [ss, "block 4"], ctx)
    _expect(add(ctx), ESTATE, [who, "sqphip_nlp_stream_begin"], ctx)  # the queue has seen the layout
    ctx.close()
    # after sqphip_sqp_reset
    ctx = _ctx(lay, 1)
    ctx.nlp_attach(p)
    ctx.sqp_reset()
    _expect(add(ctx), ESTATE, [who, "sqphip_sqp_reset"], ctx)
    ctx.close()
    # an ACOPF context and a QCQP context
    nb, ng, nl, seed = CASES["case14"]
    net = acopf_synth(nb, ng, nl, seed)
    al = acopf_layout(net)
    ctx = _ctx(al, 1)
    ctx.acopf_attach(net, al)
    _expect(add(ctx), EINVAL, [who, "no factorable NLP"], ctx)
    ctx.close()
    q = qcqp_synth(8, 4, seed=1)
    ql = qcqp_layout(q)
    ctx = _ctx(ql, 1)
    ctx.qcqp_attach(q)
    _expect(add(ctx), EINVAL, [who, "no factorable NLP"], ctx)
    ctx.close()
