"""Cox partial-likelihood data blocks of a factorable NLP in the batched device SQP loop (sqphip_nlp_add_cox_block,
csrc/nlp_cox_dev.hpp): the evaluator against the 50-digit reference and its forward error bound (tests/nlp_cox_ref.py) at the
shape edges, over every risk and event pattern and with logits spread over +-300, a scalar and a Cox block on overlapping columns
in both orders, four folds of one dataset under both linear solvers and the same model under a linear row against the oracle,
the scenario queue against the batch, slot independence and every refusal.  tests/test_nlp_cox_cpu.py vouches for the cases."""
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
from sqpsolver_jl_amd.nlp_terms import POW, NlpCoxBlock, make_nlp_terms, nlp_terms_layout   # noqa: E402
from oracle import oracle as O                                        # noqa: E402
from nlp_general_ref import general_edge_model                        # noqa: E402
from nlp_cox_ref import (EDGE_CASES, IDS, NO_EVENT, SQP_TIGHT, NlpCoxRef, OracleCoxTerms, check_outputs, edge_model,   # noqa: E402
                         edge_point, edge_reference, folds_case, mixed_model, queue_case, rows_case, with_block)

pytestmark = pytest.mark.gpu
TOL = 1e-8
EINVAL, ESTATE = -1, -4
FULL = ("x", "g", "mult_g", "mult_x_L", "mult_x_U")
_dp = C.POINTER(C.c_double)


# ---- helpers (tests/test_gpu_nlp_softmax.py; a test module is not imported)
def rel(a, b):
    if not np.size(b):
        return 0.0                                                    # (a model without rows: no multipliers to compare)
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


def _eval_some(ctx, inst, x, sigma, lam, grad):
    """the evaluation entry point with the Hessian pointer NULL: f and g alone (the Armijo probe's path), or f, g and the
    gradient"""
    f = C.c_double(); g = np.zeros(ctx.m); gr = np.zeros(ctx.n) if grad else None
    xx = np.ascontiguousarray(x, dtype=np.float64); ll = np.ascontiguousarray(lam, dtype=np.float64)
    ctx._ck(ctx.L.sqphip_acopf_eval(ctx.h, inst, _d(xx), float(sigma), _d(ll), C.byref(f), _d(gr), _d(g), None, None))
    return f.value, g, gr


def _same_result(ra, rb, where):
    for k in FULL:
        assert np.array_equal(ra[k], rb[k]), (where, k)
    assert (ra["obj_val"], ra["status"], ra["iter"]) == (rb["obj_val"], rb["status"], rb["iter"]), where


def _visibly_different(xs):
    return min(np.abs(a - b).max() for a, b in itertools.combinations(xs, 2)) > 1e-3


# ---- 1. the evaluator at the shape edges, over the risk and event patterns
@pytest.mark.parametrize("case", EDGE_CASES, ids=IDS)
def test_evaluator_at_the_shape_edges(case):
    p, lay, inst = edge_model(*case)
    ctx = _ctx(lay, 3)
    ctx.nlp_attach(p)
    for b, (w, s) in enumerate(inst):
        ctx.nlp_set_instance(b, p, weight=w, shift=s)
    fs = []
    for b in range(3):
        q, _, x, sigma, lam, val, bnd, _ = edge_reference(case, b)
        ev = ctx.acopf_eval(b, x, sigma, lam)
        assert all(np.all(np.isfinite(ev[k])) for k in ("f", "grad", "g", "jval", "hval"))
        check_outputs(ev, val, bnd, f"{case} instance {b}")           # prints err / B
        assert np.all(ev["hval"][-2:] == 0.0)                         # the copies of a slot: the first copy owns the entry
        f, g, _ = _eval_some(ctx, b, x, sigma, lam, grad=False)        # f alone: the same bits
        assert f == ev["f"] and np.array_equal(g, ev["g"])
        f, g, gr = _eval_some(ctx, b, x, sigma, lam, grad=True)        # f and the gradient, no Hessian: the same bits
        assert f == ev["f"] and np.array_equal(g, ev["g"]) and np.array_equal(gr, ev["grad"])
        fs.append(ev["f"])
    assert len(set(fs)) == 3                                          # every slot reads its own weights and offsets
    ctx.close()


def test_a_block_without_any_event_adds_exactly_zero():
    p, lay, inst = edge_model(*NO_EVENT)
    x, sigma, lam = edge_point(p, NO_EVENT[0], NO_EVENT[1])
    out = []
    for q in (p, dataclasses.replace(p, blocks=[])):
        ctx = _ctx(lay, 2)
        ctx.nlp_attach(q)
        if q.blocks:
            ctx.nlp_set_instance(1, q, weight=inst[1][0], shift=inst[1][1])
        out.append([ctx.acopf_eval(b, x, sigma, lam) for b in range(2)])
        ctx.close()
    for b in range(2):
        for k in ("f", "grad", "g", "jval", "hval"):
            assert np.array_equal(np.asarray(out[0][b][k]), np.asarray(out[1][b][k])), (b, k)


# ---- 2. a scalar and a Cox block on overlapping columns, in both block orders
@pytest.mark.parametrize("cox_first", [False, True])
def test_scalar_and_cox_blocks_share_slots_and_gradient_entries(cox_first):
    p, lay = mixed_model(cox_first)
    kc = 0 if cox_first else 1                                        # the Cox block's number
    rng = np.random.default_rng(2)
    w = rng.uniform(0.0, 1.0, 22)
    s = 0.1 * rng.standard_normal(37)
    ctx = _ctx(lay, 2)
    ctx.nlp_attach(p)
    ctx.nlp_set_instance(1, p, weight={kc: w}, shift={1 - kc: s})
    x = rng.uniform(-1.0, 1.0, p.n); lam = np.zeros(0)
    for b, q in enumerate((p, with_block(with_block(p, kc, weight=w), 1 - kc, shift=s))):
        ev = ctx.acopf_eval(b, x, 1.3, lam)
        val, bnd = NlpCoxRef(q).want(x, 1.3, lam, lay)
        check_outputs(ev, val, bnd, f"mixed blocks, Cox first = {cox_first}, instance {b}")
    # each block alone moves the shared entries (variables 3, 5, 7): both contribute
    for k in range(2):
        only = NlpCoxRef(q).want(x, 1.3, lam, lay, blocks=q.blocks[k:k + 1])[0]
        assert np.abs(only["grad"][[2, 4, 6]] - ev["grad"][[2, 4, 6]]).min() > 1e-3
    ctx.close()


# ---- 3. four folds of one dataset in one batch, and the model under a linear row, against the oracle
def _against_the_oracle(ctx, b, q, lay, kkt_mode):
    ro = O.sqp_solve(OracleCoxTerms(q, lay), O.default_options(**_lin(kkt_mode), **SQP_TIGHT))
    assert ro["status"] == 0
    rg, tr = ctx.sqp_get(b), ctx.sqp_trace(b)
    print("instance", b, "status", rg["status"], ro["status"], "iter", rg["iter"], ro["iter"], "x", rel(rg["x"], ro["x"]),
          "obj", abs(rg["obj_val"] - ro["obj_val"]), "multipliers", [rel(rg[k], ro[k]) for k in FULL[2:]])
    assert (rg["status"], rg["iter"]) == (ro["status"], ro["iter"]), b
    assert _decisions(ro["trace"]) == _decisions(tr) and _ipm_counts_close(ro, tr), b
    assert rel(rg["x"], ro["x"]) < TOL and abs(rg["obj_val"] - ro["obj_val"]) <= TOL * max(1.0, abs(ro["obj_val"])), b
    # multipliers through sqp_get: those of the last sub-problem, which both sides solve to ipm_tol from iterates 1e-8 apart --
    # 1e-6 leaves two digits for the conditioning of that sub-problem
    assert all(rel(rg[k], ro[k]) <= 1e-6 for k in FULL[2:]), b
    return rg["x"]


@pytest.mark.parametrize("kkt_mode", [1, 2])
def test_four_folds_in_one_batch_match_the_oracle(kkt_mode):
    p, W = folds_case()
    lay = nlp_terms_layout(p)
    ctx = _ctx(lay, 4, **_lin(kkt_mode), **SQP_TIGHT)
    ctx.nlp_attach(p)
    for f in range(4):
        ctx.nlp_set_instance(f, p, weight=W[f])
    ctx.sqp_reset(); ctx.sqp_run(0)
    try:
        xs = [_against_the_oracle(ctx, f, with_block(p, 0, weight=W[f]), lay, kkt_mode) for f in range(4)]
    finally:
        O.set_kkt_order(None)
    ctx.close()
    assert _visibly_different(xs)                                     # a context that ignores the weights cannot pass


def test_cox_block_under_a_linear_row_matches_the_oracle():
    p, lay, shifts = rows_case()
    ctx = _ctx(lay, 3, kkt_mode=2, **SQP_TIGHT)
    ctx.nlp_attach(p)
    for b in range(3):
        ctx.nlp_set_instance(b, p, shift=shifts[b])
    ctx.sqp_reset(); ctx.sqp_run(0)
    try:
        xs = [_against_the_oracle(ctx, b, with_block(p, 0, shift=shifts[b]), lay, 2) for b in range(3)]
    finally:
        O.set_kkt_order(None)
    ctx.close()
    assert all(abs(x.sum() - 0.3) <= 1e-8 for x in xs) and _visibly_different(xs)


# ---- 4. the scenario queue against the batch; slot independence; a second reset + run
def test_queue_of_five_scenarios_on_two_slots_equals_the_batch():
    p, lay, scen = queue_case()
    ctx = _ctx(lay, 2, kkt_mode=2, **SQP_TIGHT)
    ctx.nlp_attach(p)
    ctx.nlp_stream_begin(5, keep_multipliers=True)
    for s, (w, sh) in enumerate(scen):
        ctx.nlp_stream_set(s, tcoef=p.tcoef, x0=p.x0)
        ctx.nlp_stream_set_block(s, 0, weight=w, shift=sh)
    ctx.stream_run()
    got = [ctx.stream_get_full(s) for s in range(5)]
    ctx.close()
    assert all(r["status"] == 0 for r in got) and _visibly_different([r["x"] for r in got])
    ref = _ctx(lay, 2, kkt_mode=2, **SQP_TIGHT)
    ref.nlp_attach(p)
    for s0 in (0, 2, 4):
        for b in range(2):
            w, sh = scen[min(s0 + b, 4)]
            ref.nlp_set_instance(b, p, weight=w, shift=sh)
        ref.sqp_reset(); ref.sqp_run(0)
        for b in range(2):
            if s0 + b < 5:
                _same_result(got[s0 + b], ref.sqp_get(b), ("scenario", s0 + b))
    ref.close()


def test_stream_set_restores_the_data_of_the_add_call():
    p, lay, scen = queue_case()
    q = with_block(p, 0, weight=scen[0][0], shift=scen[0][1])          # the add call's data: not ones and zeros
    ctx = _ctx(lay, 1, kkt_mode=2, **SQP_TIGHT)
    ctx.nlp_attach(q)
    ctx.nlp_stream_begin(2, keep_multipliers=True)
    ctx.nlp_stream_set(0, tcoef=p.tcoef, x0=p.x0)
    ctx.nlp_stream_set_block(0, 0, weight=scen[1][0], shift=scen[1][1])
    ctx.nlp_stream_set(0, tcoef=p.tcoef, x0=p.x0)                      # ... and back to the add call's
    ctx.nlp_stream_set(1, tcoef=p.tcoef, x0=p.x0)
    ctx.nlp_stream_set_block(1, 0, weight=scen[0][0], shift=scen[0][1])
    ctx.stream_run()
    ra, rb = ctx.stream_get_full(0), ctx.stream_get_full(1)
    ctx.close()
    assert ra["status"] == 0 and np.array_equal(ra["x"], rb["x"]) and ra["obj_val"] == rb["obj_val"]


def test_an_instance_does_not_depend_on_its_slot_its_neighbours_or_the_run():
    p, lay, scen = queue_case()
    order = (0, 1, 2, 0)                                              # slots 0 and 3: the same instance, other neighbours
    ctx = _ctx(lay, 4, kkt_mode=2, **SQP_TIGHT)
    ctx.nlp_attach(p)
    for b, f in enumerate(order):
        ctx.nlp_set_instance(b, p, weight=scen[f][0], shift=scen[f][1])
    runs = []
    for _ in range(2):
        ctx.sqp_reset(); ctx.sqp_run(0)
        runs.append([(ctx.sqp_get(b), ctx.sqp_trace(b)) for b in range(4)])
    ctx.close()
    assert all(r[0]["status"] == 0 for r in runs[0])
    _same_result(runs[0][0][0], runs[0][3][0], "slots 0 and 3")
    assert runs[0][0][1] == runs[0][3][1]
    assert not np.array_equal(runs[0][0][0]["x"], runs[0][1][0]["x"])
    for b in range(4):
        _same_result(runs[0][b][0], runs[1][b][0], ("second run", b))
        assert runs[0][b][1] == runs[1][b][1]


def test_evaluations_do_not_depend_on_the_slot():
    case = (1025, 3, "groups", "mixed", 0)
    p, lay, inst = edge_model(*case)
    x, sigma, lam = edge_point(p, case[0], case[1])
    ctx = _ctx(lay, 3)
    ctx.nlp_attach(p)
    for b, k in enumerate((0, 1, 0)):
        ctx.nlp_set_instance(b, p, weight=inst[k][0], shift=inst[k][1])
    ev = [ctx.acopf_eval(b, x, sigma, lam) for b in (0, 1, 2, 0)]
    ctx.close()
    for k in ("f", "grad", "hval"):
        assert np.array_equal(np.asarray(ev[0][k]), np.asarray(ev[2][k])) and np.array_equal(np.asarray(ev[0][k]), np.asarray(ev[3][k])), k
    assert ev[0]["f"] != ev[1]["f"]


# ---- 5. refusals
def _expect(rc, code, words, ctx):
    msg = ctx.L.sqphip_last_error(ctx.h).decode()
    assert rc == code, (rc, msg)
    assert all(w in msg for w in words), msg


def test_refusals():
    n = 8
    terms = [(0, 1.0, [(j + 1, POW, 2)]) for j in range(n)]
    blk = NlpCoxBlock([2, 4, 5, 7], np.ones((4, 4)), [1, 3, 3, 4], [1, 0, 1, 1])
    p = make_nlp_terms(n, 0, 0, terms, xL=np.full(n, -1.0), xU=np.ones(n), blocks=[blk])
    lay = nlp_terms_layout(p)
    who = "sqphip_nlp_add_cox_block"
    A = np.ones((4, 4)); cols = [2, 4, 5, 7]; risk = [1, 3, 3, 4]; event = [1.0, 0.0, 1.0, 1.0]
    lp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int64))
    ip = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))

    def add(ctx, N=4, d=4, c=cols, a=A, r=risk, e=event):
        c = None if c is None else np.ascontiguousarray(c, dtype=np.int64)
        r = None if r is None else np.ascontiguousarray(r, dtype=np.int32)
        e = None if e is None else np.ascontiguousarray(e, dtype=np.float64)
        return ctx.L.sqphip_nlp_add_cox_block(ctx.h, N, d, lp(c), _d(a), ip(r), _d(e), None, None, None)

    ctx = _ctx(lay, 2)
    _expect(add(ctx), EINVAL, [who, "no factorable NLP"], ctx)       # before any attach
    ctx.nlp_attach(dataclasses.replace(p, blocks=[]))
    _expect(add(ctx, d=0), EINVAL, [who, "block 1", "d = 0"], ctx)
    _expect(add(ctx, d=129), EINVAL, [who, "block 1", "d = 129"], ctx)
    _expect(add(ctx, N=0), EINVAL, [who, "block 1", "N = 0"], ctx)
    _expect(add(ctx, N=2 ** 31 // 4 + 1), EINVAL, [who, "block 1", "too large"], ctx)
    for gone in ("c", "a", "r", "e"):
        _expect(add(ctx, **{gone: None}), EINVAL, [who, "block 1", "null"], ctx)
    _expect(add(ctx, r=[1, 1, 3, 4]), EINVAL, [who, "block 1", "point 2", "risk 1", "outside 2..4"], ctx)
    _expect(add(ctx, r=[1, 3, 3, 5]), EINVAL, [who, "block 1", "point 4", "risk 5", "outside 4..4"], ctx)
    _expect(add(ctx, r=[0, 3, 3, 4]), EINVAL, [who, "block 1", "point 1", "risk 0", "outside 1..4"], ctx)
    _expect(add(ctx, r=[4, 3, 3, 4]), EINVAL, [who, "block 1", "point 2", "risk 3", "decreases from 4"], ctx)
    _expect(add(ctx, e=[1.0, -1.0, 1.0, 1.0]), EINVAL, [who, "block 1", "point 2", "event -1"], ctx)
    _expect(add(ctx, e=[1.0, 0.0, np.nan, 1.0]), EINVAL, [who, "block 1", "point 3", "event nan"], ctx)
    _expect(add(ctx, e=[1.0, 0.0, 1.0, np.inf]), EINVAL, [who, "block 1", "point 4", "event inf"], ctx)
    _expect(add(ctx, c=[2, 9, 5, 7]), EINVAL, [who, "block 1", "column 2", "variable 9", "out of range"], ctx)
    _expect(add(ctx, c=[2, 4, 5, 2]), EINVAL, [who, "block 1", "column 4", "variable 2", "twice"], ctx)
    _expect(add(ctx, c=[2, 4, 5, 8]), EINVAL, [who, "block 1", "entry (4, 1)", "Hessian entry (8, 2)"], ctx)
    for k in range(4):
        assert add(ctx) == 0
    _expect(add(ctx), EINVAL, [who, "block 5", "at most 4"], ctx)
    # the existing block calls serve a Cox block: weight [N], offsets [N]
    w, sh = np.ones(4), np.zeros(4)
    assert ctx.L.sqphip_nlp_set_instance_block(ctx.h, 1, 3, _d(w), _d(sh)) == 0
    _expect(ctx.L.sqphip_nlp_set_instance_block(ctx.h, 0, 4, _d(w), None), EINVAL, ["sqphip_nlp_set_instance_block", "block 4"], ctx)
    ctx.nlp_stream_begin(3)
    assert ctx.L.sqphip_nlp_stream_set_block(ctx.h, 2, 0, _d(w), _d(sh)) == 0
    _expect(add(ctx), ESTATE, [who, "sqphip_nlp_stream_begin"], ctx)  # the queue has seen the layout
    ctx.close()
    ctx = _ctx(lay, 1)
    ctx.nlp_attach(p)
    ctx.sqp_reset()
    _expect(add(ctx), ESTATE, [who, "sqphip_sqp_reset"], ctx)
    ctx.close()
    # an ACOPF context
    nb, ng, nl, seed = CASES["case14"]
    net = acopf_synth(nb, ng, nl, seed)
    al = acopf_layout(net)
    ctx = _ctx(al, 1)
    ctx.acopf_attach(net, al)
    _expect(add(ctx), EINVAL, [who, "no factorable NLP"], ctx)
    ctx.close()


# ---- a context without a Cox block files the bytes the parent filed (the record of tests/test_gpu_nlp_exact.py's library,
# tests/golden/nlp_exact_general_edge.npz, which the parent reproduces bit for bit)
def test_a_context_without_a_cox_block_files_the_parents_bytes():
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    rec = np.load(os.path.join(here, "nlp_exact_general_edge.npz"))
    p, lay = general_edge_model()
    ctx = _ctx(lay, 1)
    ctx.nlp_attach(p, general=True); ctx.nlp_set_instance(0, p)
    ev = ctx.acopf_eval(0, rec["x"], 0.7, rec["lam"])
    ctx.close()
    for k in ("f", "grad", "g", "jval", "hval"):
        assert np.array_equal(np.asarray(ev[k]), rec[k]), k
