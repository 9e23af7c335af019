"""Multinomial (softmax) data blocks of a factorable NLP in the batched device SQP loop (sqphip_nlp_add_softmax_block,
csrc/nlp_softmax_dev.hpp): the evaluator against the 50-digit reference and its forward error bound (tests/nlp_softmax_ref.py)
at the shape edges and with logits of +-800, a scalar and a softmax block on overlapping columns in both orders, four folds of
a 3-class fit under both linear solvers, a block under rows against the oracle, the scenario queue against the batch, slot
independence and every refusal.  tests/test_nlp_softmax_cpu.py holds the oracle's and Newton's word for the solved cases."""
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
from sqpsolver_jl_amd.nlp_terms import (POW, NlpSoftmaxBlock, logistic_block_model, make_nlp_terms,   # noqa: E402
                                        multinomial_block_model, nlp_terms_layout)
from oracle import oracle as O                                        # noqa: E402
from nlp_general_ref import general_edge_model                        # noqa: E402
from nlp_softmax_ref import (BIG_LOGITS, EDGE_CASES, SQP_TIGHT, NlpSoftmaxRef, OracleSoftmaxTerms, check_outputs,   # noqa: E402
                             edge_model, edge_reference, folds_case3, mixed_model, newton_multinomial, queue_case, rows_case,
                             with_block)

pytestmark = pytest.mark.gpu
TOL = 1e-8
EINVAL, ESTATE = -1, -4
FULL = ("x", "g", "mult_g", "mult_x_L", "mult_x_U")
_dp = C.POINTER(C.c_double)
ALL_EDGES = [(c, False) for c in EDGE_CASES] + [(BIG_LOGITS, True)]
IDS = ["N%d-d%d-K%d-pinned%d" % c + ("-big" if big else "") for c, big in ALL_EDGES]


# ---- helpers (tests/test_gpu_nlp_block.py; a test module is not imported)
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
@pytest.mark.parametrize("case,big", ALL_EDGES, ids=IDS)
def test_evaluator_at_the_shape_edges(case, big):
    p, lay, inst = edge_model(*case, big=big)
    ctx = _ctx(lay, 3)
    ctx.nlp_attach(p)
    for b, (w, s) in enumerate(inst):
        ctx.nlp_set_instance(b, p, weight=w, shift=s)
    fs = []
    for b in range(3):
        q, _, x, sigma, lam, val, bnd = edge_reference(case, b, big)
        ev = ctx.acopf_eval(b, x, sigma, lam)
        assert all(np.all(np.isfinite(ev[k])) for k in ("f", "grad", "g", "jval", "hval"))
        check_outputs(ev, val, bnd, f"(N, d, K, pinned) = {case} big = {big} instance {b}")
        assert np.all(ev["hval"][-2:] == 0.0)                         # the copies of a slot: the first copy owns the entry
        f, g = _fg_only(ctx, b, x)
        assert f == ev["f"] and np.array_equal(g, ev["g"])
        fs.append(ev["f"])
    assert len(set(fs)) == 3                                          # every slot reads its own weights and offsets
    ctx.close()


# ---- 2. a scalar and a softmax block on overlapping columns, in both block orders
@pytest.mark.parametrize("softmax_first", [False, True])
def test_scalar_and_softmax_blocks_share_slots_and_gradient_entries(softmax_first):
    p, lay = mixed_model(softmax_first)
    ks = 0 if softmax_first else 1                                    # the softmax block's number
    rng = np.random.default_rng(2)
    w = rng.uniform(0.0, 1.0, 22)
    s = 0.1 * rng.standard_normal(37)
    ctx = _ctx(lay, 2)
    ctx.nlp_attach(p)
    ctx.nlp_set_instance(1, p, weight={ks: w}, shift={1 - ks: s})
    x = rng.uniform(-1.0, 1.0, p.n); lam = np.zeros(0)
    for b, q in enumerate((p, with_block(with_block(p, ks, weight=w), 1 - ks, shift=s))):
        ev = ctx.acopf_eval(b, x, 1.3, lam)
        val, bnd = NlpSoftmaxRef(q).want(x, 1.3, lam, lay)
        check_outputs(ev, val, bnd, f"mixed blocks, softmax first = {softmax_first}, instance {b}")
    # each block alone moves the shared entries (variables 3, 5, 7): both contribute
    for k in range(2):
        only = NlpSoftmaxRef(q).want(x, 1.3, lam, lay, blocks=q.blocks[k:k + 1])[0]
        assert np.abs(only["grad"][[2, 4, 6]] - ev["grad"][[2, 4, 6]]).min() > 1e-3
    ctx.close()


# ---- 3. four folds of a 3-class fit in one batch
@pytest.mark.parametrize("pinned", [True, False], ids=["pinned", "unpinned"])
@pytest.mark.parametrize("kkt_mode", [1, 2])
def test_four_folds_of_a_three_class_fit_in_one_batch(kkt_mode, pinned):
    X, y, reg, W = folds_case3()
    want = [newton_multinomial(X, y, 3, reg, w, pinned)[0] for w in W]
    assert _visibly_different(want)                                   # a context that ignores the weights cannot pass
    p = multinomial_block_model(X, y, 3, reg, pinned, W[0])
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


def test_two_classes_pinned_reach_the_optimum_of_the_logistic_block_model():
    X, y, reg, W = folds_case3(2)
    ps = multinomial_block_model(X, y, 2, reg, True, W[0])
    pl = logistic_block_model(X, (y == 0).astype(float), reg, W[0])    # class 0 carries the variables
    want = newton_multinomial(X, y, 2, reg, W[0], True)[0]
    xs = []
    for p in (ps, pl):
        ctx = _ctx(nlp_terms_layout(p), 1, kkt_mode=2, **SQP_TIGHT)
        ctx.nlp_attach(p); ctx.nlp_set_instance(0, p)
        ctx.sqp_reset(); ctx.sqp_run(0)
        r = ctx.sqp_get(0)
        ctx.close()
        print("status", r["status"], "iter", r["iter"], "err", np.abs(r["x"] - want).max())
        assert r["status"] == 0 and np.abs(r["x"] - want).max() <= 1e-6
        xs.append(r["x"])
    assert np.abs(xs[0] - xs[1]).max() <= 1e-6


# ---- 4. a softmax block under rows, against the oracle
def test_softmax_block_under_rows_matches_the_oracle():
    p, lay, shifts = rows_case()
    ctx = _ctx(lay, 3, kkt_mode=2, **SQP_TIGHT)
    ctx.nlp_attach(p)
    for b in range(3):
        ctx.nlp_set_instance(b, p, shift=shifts[b])
    ctx.sqp_reset(); ctx.sqp_run(0)
    try:
        for b in range(3):
            ro = O.sqp_solve(OracleSoftmaxTerms(with_block(p, 0, shift=shifts[b]), lay), O.default_options(kkt_mode=2, **SQP_TIGHT))
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


# ---- 5. the scenario queue against the batch; slot independence; a second reset + run
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


# ---- 6. refusals
def _expect(rc, code, words, ctx):
    msg = ctx.L.sqphip_last_error(ctx.h).decode()
    assert rc == code, (rc, msg)
    assert all(w in msg for w in words), msg


def test_refusals():
    n = 8
    terms = [(0, 1.0, [(j + 1, POW, 2)]) for j in range(n)]
    blk = NlpSoftmaxBlock([[2, 4], [5, 7]], np.ones((3, 2)), [0, 1, 2], 3)
    p = make_nlp_terms(n, 0, 0, terms, xL=np.full(n, -1.0), xU=np.ones(n), blocks=[blk])
    lay = nlp_terms_layout(p)
    who = "sqphip_nlp_add_softmax_block"
    A = np.ones((4, 2)); cols = np.array([2, 4, 5, 7], dtype=np.int64); y = np.array([0, 1, 2, 1], dtype=np.int32)
    lp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int64))
    ip = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))

    def add(ctx, N=4, d=2, K=3, pinned=1, c=cols, a=A, lab=y):
        c = None if c is None else np.ascontiguousarray(c, dtype=np.int64)
        lab = None if lab is None else np.ascontiguousarray(lab, dtype=np.int32)
        return ctx.L.sqphip_nlp_add_softmax_block(ctx.h, N, d, K, pinned, lp(c), _d(a), ip(lab), None, None, None)

    ctx = _ctx(lay, 2)
    _expect(add(ctx), EINVAL, [who, "no factorable NLP"], ctx)       # before any attach
    ctx.nlp_attach(dataclasses.replace(p, blocks=[]))
    _expect(add(ctx, K=1), EINVAL, [who, "block 1", "K = 1"], ctx)
    _expect(add(ctx, K=65), EINVAL, [who, "block 1", "K = 65"], ctx)
    _expect(add(ctx, d=0), EINVAL, [who, "block 1", "d = 0"], ctx)
    _expect(add(ctx, N=0), EINVAL, [who, "block 1", "N = 0"], ctx)
    _expect(add(ctx, d=65, K=3), EINVAL, [who, "block 1", "Kf d = 2 x 65"], ctx)
    _expect(add(ctx, d=43, K=3, pinned=0), EINVAL, [who, "block 1", "Kf d = 3 x 43"], ctx)
    _expect(add(ctx, N=2 ** 31 // 2 + 1), EINVAL, [who, "block 1", "too large"], ctx)
    _expect(add(ctx, c=None), EINVAL, [who, "block 1", "null"], ctx)
    _expect(add(ctx, a=None), EINVAL, [who, "block 1", "null"], ctx)
    _expect(add(ctx, lab=None), EINVAL, [who, "block 1", "null"], ctx)
    _expect(add(ctx, lab=[0, 1, 3, 1]), EINVAL, [who, "block 1", "point 3", "label 3"], ctx)
    _expect(add(ctx, lab=[0, -1, 2, 1]), EINVAL, [who, "block 1", "point 2", "label -1"], ctx)
    _expect(add(ctx, c=[2, 9, 5, 7]), EINVAL, [who, "block 1", "column 2", "variable 9", "out of range"], ctx)
    _expect(add(ctx, c=[2, 4, 5, 2]), EINVAL, [who, "block 1", "column 4", "variable 2", "twice"], ctx)     # across two classes
    _expect(add(ctx, c=[2, 4, 5, 8]), EINVAL, [who, "block 1", "entry (4, 1)", "Hessian entry (8, 2)"], ctx)
    for k in range(4):
        assert add(ctx) == 0
    _expect(add(ctx), EINVAL, [who, "block 5", "at most 4"], ctx)
    # the existing block calls serve a softmax block: weight [N], offsets [Kf N]
    w, sh = np.ones(4), np.zeros((2, 4))
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


# ---- a context without a softmax block files the bytes it filed before the call existed: one generic case, recorded from the
# parent library (tests/golden/nlp_softmax_parent_general_edge.npz)
def test_a_context_without_a_softmax_block_files_the_parents_bytes():
    """Two records of general_edge_model at one point: nlp_softmax_parent_general_edge.npz from the library before the softmax
    blocks, nlp_exact_general_edge.npz from the library whose nlp_kappa_wide forms tanh', tanh'', sigmoid'' and atan'' without
    cancellation.  Against the older record: bit equality on every entry that reads none of those four stored values (the
    set comes from the model's plans); every entry under the exact bound of tests/nlp_exact.py; against the newer record: bit
    equality on every entry."""
    import nlp_exact as X
    from sqpsolver_jl_amd.nlp_terms import ATAN, SIGMOID, TANH
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    gold = np.load(os.path.join(here, "nlp_softmax_parent_general_edge.npz"))
    rec = np.load(os.path.join(here, "nlp_exact_general_edge.npz"))
    p, lay = general_edge_model()
    assert np.array_equal(gold["x"], rec["x"]) and np.array_equal(gold["lam"], rec["lam"])
    ctx = _ctx(lay, 1)
    ctx.nlp_attach(p, general=True); ctx.nlp_set_instance(0, p)
    ev = ctx.acopf_eval(0, gold["x"], 0.7, gold["lam"])
    ctx.close()
    changed = lambda k, q: (p.fkind[k] == TANH and q >= 1) or (p.fkind[k] in (SIGMOID, ATAN) and q == 2)
    same, moved = 0, 0
    for key, entries in X.plans(p, lay).items():
        got, old = np.atleast_1d(np.asarray(ev[key])), np.atleast_1d(gold[key])
        for i, entry in enumerate(entries):
            if not any(changed(k, q) for t, a, b, _, _, _ in entry for k, q in X._orders(p, t, a, b)):
                assert got[i] == old[i], (key, i)
                same += 1
            else:
                moved += 1
    print("entries held to the older record's bits:", same, "others:", moved)
    assert same > 100 and 0 < moved < 60
    R = X.NlpExact(p)
    val, bnd = R.want(gold["x"], 0.7, gold["lam"], lay)
    X.check_entries(ev, val, bnd, R.exact, label="general_edge_model")
    X.check_entries({k: gold[k] for k in X.KEYS}, val, bnd, R.exact, label="general_edge_model, the older record")
    for k in ("f", "grad", "g", "jval", "hval"):
        assert np.array_equal(np.asarray(ev[k]), rec[k]), k
