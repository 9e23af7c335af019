"""The scenario queue on a factorable-NLP context (sqphip_nlp_stream_begin / _set, sqphip_sqp_stream_get_full): more
scenarios than slots for any sparse factorable NLP.  The queue against the ordinary batched run bit for bit (the evaluator
does not depend on the slot), the multipliers filed with a result, NULL parts of a scenario, the loader's block copy at its
stride edges, the generic queue against the dedicated polar ACOPF queue, a queue shared between two contexts, misuse.  The
inputs are those of tests/nlp_queue_cases.py; tests/test_nlp_stream_cpu.py holds the oracle's word for them."""
import functools
import os
import sys
import threading

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import sqpsolver_jl_amd as pkg                                        # noqa: E402
from sqpsolver_jl_amd.acopf_synth import acopf_layout, acopf_synth, contingency, CASES   # noqa: E402
from sqpsolver_jl_amd.nlp_terms import from_polar_acopf, nlp_terms_layout   # noqa: E402
from sqpsolver_jl_amd.qcqp import qcqp_layout, qcqp_synth            # noqa: E402
from sqpsolver_jl_amd.shard import run_shared_queue                    # noqa: E402
from nlp_ref import NlpRef                                            # noqa: E402
import nlp_queue_cases as QC                                          # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-8                                   # tests/test_gpu_nlp.py, between the generic and the dedicated evaluator
EVAL_TOL = 1e-13                             # tests/test_gpu_nlp.py, the device evaluator against the numpy reference
SQP_KW = dict(tol_infeas=1e-6, tol_residual=1e-4)
EINVAL, ESTATE = -1, -4
M = QC.M
FULL = ("x", "g", "mult_g", "mult_x_L", "mult_x_U")


# ---- helpers (tests/test_gpu_qcqp_stream.py; a test module is not imported)
def rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(1.0, np.abs(np.asarray(b)).max()))


def _ctx(lay, batch, **kw):
    return pkg.Context(lay.n, lay.m, lay.num_linear, lay.jrow, lay.jcol, lay.hrow, lay.hcol, lay.xL, lay.xU, lay.gL, lay.gU,
                       pkg.default_options(**kw), batch=batch)


def _expect(rc, code, words, ctx):
    assert rc == code, rc
    msg = ctx.L.sqphip_last_error(ctx.h).decode()
    assert all(w in msg for w in words), msg


def _kw(kkt_mode):
    return dict(kkt_mode=kkt_mode, **QC.OPTIONS)


def _run_batch(p, lay, ps, **kw):
    """ps in an ordinary batch of len(ps): (sqp_get of every instance, the work counters)."""
    ctx = _ctx(lay, len(ps), **kw)
    ctx.nlp_attach(p)
    for b, q in enumerate(ps):
        ctx.nlp_set_instance(b, q)
    ctx.sqp_reset(); ctx.sqp_run(0)
    ref = [ctx.sqp_get(b) for b in range(len(ps))]
    c = ctx.counters()
    ctx.close()
    return ref, (c["n_qp"], c["n_ipm_iter"], c["n_factor"])


@functools.lru_cache(maxsize=None)
def _batch(kkt_mode):
    """The 12 scenarios in an ordinary batch of 12 (computed once per solver, shared, not modified)."""
    base, lay, ps = QC.queue_problem()
    return _run_batch(base, lay, ps, **_kw(kkt_mode))


def _queue(kkt_mode, slots, keep=False):
    base, lay, ps = QC.queue_problem()
    ctx = _ctx(lay, slots, **_kw(kkt_mode))
    ctx.nlp_attach(base)
    ctx.nlp_stream_begin(M, keep_multipliers=keep)
    for s in range(M):
        ctx.nlp_stream_set(s, ps[s])
    return ctx


def _same_result(r, ref):
    return (r["status"], r["iter"]) == (ref["status"], ref["iter"]) and r["obj_val"] == ref["obj_val"] and \
        np.array_equal(r["x"], ref["x"])


def _same_full(r, ref):
    return all(np.array_equal(r[k], ref[k]) for k in FULL) and \
        (r["obj_val"], r["status"], r["iter"]) == (ref["obj_val"], ref["status"], ref["iter"])


# ---- 1. queue = batch, bit for bit
@pytest.mark.parametrize("kkt_mode", [2, 1])
@pytest.mark.parametrize("slots", [4, 64])
def test_nlp_queue_gives_the_batch_results(kkt_mode, slots):
    """12 scenarios of the generated NLP through 4 slots (three per slot, refilled on the device) and through 64 slots (more
    slots than scenarios; on the sparse path four instance groups): status, iterations, objective and point of the
    ordinary batch of 12, bit for bit, and the same totals of sub-problems, interior-point iterations, factorisations.
    Scenarios 3, 7 and 11 carry a tighter lower bound that is active at their optimum: the loader carries bounds."""
    ref, tot = _batch(kkt_mode)
    base, lay, ps = QC.queue_problem()
    ctx = _queue(kkt_mode, slots)
    ctx.stream_run()
    for s in range(M):
        r = ctx.stream_get(s)
        print(f"kkt_mode {kkt_mode} slots {slots} scenario {s}: status {r['status']} iter {r['iter']} (batch {ref[s]['iter']}, "
              f"oracle {QC.ORACLE_ITERS[s]}) |dx| {np.abs(r['x'] - ref[s]['x']).max():.1e} min x {r['x'].min():.6f}")
        assert _same_result(r, ref[s]), s
        assert r["status"] == 0, s
    assert len({ref[s]["iter"] for s in range(M)}) >= 4               # the slots refill at different times
    for s in (3, 7, 11):
        assert abs(ctx.stream_get(s)["x"].min() - QC.TIGHT_XL) <= 1e-6, s
    c = ctx.counters()
    if kkt_mode == 2 and slots == 64:
        assert c["n_groups"] == 4
    assert (c["n_qp"], c["n_ipm_iter"], c["n_factor"]) == tot
    assert ctx.sqp_status()[2].all()
    ctx.stream_run()                                     # a second pass over the same queue: the same results
    for s in range(M):
        assert _same_result(ctx.stream_get(s), ref[s]), s
    ctx.close()


# ---- 2. multipliers
@pytest.mark.parametrize("kkt_mode,slots", [(2, 4), (2, 64), (1, 4)])
def test_nlp_queue_files_the_multipliers(kkt_mode, slots):
    ref, _ = _batch(kkt_mode)
    ctx = _queue(kkt_mode, slots, keep=True)
    ctx.stream_run()
    for s in range(M):
        r = ctx.stream_get_full(s)
        for k in FULL:
            assert np.array_equal(r[k], ref[s][k]), (s, k)
        assert (r["obj_val"], r["status"], r["iter"]) == (ref[s]["obj_val"], ref[s]["status"], ref[s]["iter"]), s
        assert _same_result(ctx.stream_get(s), ref[s]), s
    assert any(np.abs(ref[s]["mult_g"]).max() > 0 for s in range(M))        # (the comparison is not one of zeros)
    assert all(np.abs(ref[s]["mult_x_L"]).max() > 0 for s in (3, 7, 11))    # (the active tightened bound has its multiplier)
    ctx.close()


def test_get_full_without_the_tables_is_a_state_error():
    ctx = _queue(2, 4, keep=False)
    ctx.stream_run()
    x = np.zeros(ctx.n)
    rc = ctx.L.sqphip_sqp_stream_get_full(ctx.h, 0, x.ctypes.data_as(pkg.host._dp), None, None, None, None, None, None, None)
    _expect(rc, ESTATE, ["keep_multipliers", "sqphip_nlp_stream_begin", "sqphip_qcqp_stream_begin"], ctx)
    with pytest.raises(pkg.SqpHipError):
        ctx.stream_get_full(0)
    ctx.close()


# ---- 3. NULL parts mean the values of the attach
def test_null_parts_of_a_scenario_are_the_values_of_the_attach():
    base, lay, ps = QC.queue_problem()
    tcoef, two = QC.null_part_terms(base, ps)
    ref, _ = _run_batch(base, lay, two, **_kw(2))
    ctx = _ctx(lay, 4, **_kw(2))
    ctx.nlp_attach(base)
    for b in range(4):                                   # every slot's block now holds other values than the attach gave
        ctx.nlp_set_instance(b, ps[1 + b])
    ctx.nlp_stream_begin(2, keep_multipliers=True)
    ctx.nlp_stream_set(0, tcoef=tcoef, x0=base.x0)       # bounds: those of the context; values: the attach's, and tcoef
    ctx.nlp_stream_set(1, x0=base.x0)
    ctx.stream_run()
    for s in range(2):
        assert _same_full(ctx.stream_get_full(s), ref[s]), s
        assert ref[s]["status"] == 0, s
    assert not np.array_equal(ref[0]["x"], ref[1]["x"])
    ctx.close()


# ---- 4. the block copy at its stride edges
@pytest.mark.parametrize("nvals", QC.EDGE_COUNTS)
def test_block_copy_at_its_stride_edges(nvals):
    """1 + m + nterms doubles at the odd / padded tail of the double2 copy, at one against two accesses in flight per thread
    and in a second trip of the loop.  Three scenarios that differ in every coefficient run through ONE slot, so the slot
    always holds the previous scenario's values when the next is loaded: the results are those of a batch of three, and
    afterwards the evaluator of slot 0 is the reference evaluator of the last scenario -- a loader that drops or misplaces
    part of the block fails both."""
    p = QC.edge_model(nvals)
    lay = nlp_terms_layout(p)
    ps = QC.edge_scenarios(p)
    ref, _ = _run_batch(p, lay, ps, **_kw(2))
    ctx = _ctx(lay, 1, **_kw(2))
    ctx.nlp_attach(p)
    ctx.nlp_stream_begin(3, keep_multipliers=True)
    for s in range(3):
        ctx.nlp_stream_set(s, ps[s])
    ctx.stream_run()
    for s in range(3):
        r = ctx.stream_get_full(s)
        print(f"nvals {nvals} scenario {s}: status {r['status']} iter {r['iter']} (batch {ref[s]['iter']}) obj {r['obj_val']:.12g}")
        assert _same_full(r, ref[s]), s
    assert len({ref[s]["obj_val"] for s in range(3)}) == 3
    rng = np.random.default_rng(nvals)
    x = rng.uniform(0.5, 1.6, p.n); lam = rng.standard_normal(p.m); sigma = 1.3
    ev, R = ctx.acopf_eval(0, x, sigma, lam), NlpRef(ps[2])
    want = dict(f=R.f(x), grad=R.grad(x), g=R.g(x), jval=R.jac(x, lay.jrow, lay.jcol), hval=R.hess(x, sigma, lam, lay.hrow, lay.hcol))
    err = {k: rel(ev[k], want[k]) for k in want}
    print(f"nvals {nvals} evaluator of slot 0 against the last scenario:", err)
    assert all(e <= EVAL_TOL for e in err.values()), err
    assert rel(ev["f"], NlpRef(ps[1]).f(x)) > 1e-3                    # (the scenarios are told apart by the probe)
    ctx.close()


# ---- 5. generic queue = dedicated queue
def test_generic_queue_equals_dedicated_polar_queue_on_contingencies():
    """IEEE-14-shaped contingencies restated by from_polar_acopf through the NLP queue and through the ACOPF queue, 2 slots
    each: the same status and iteration count, the point within the tolerance the two evaluators are held to in a batch
    (tests/test_gpu_nlp.py: the base net and contingencies 2 and 5).  Contingencies tried in a batch of both evaluators: 0
    (the base net) to 11; the two agree on status and iteration count of every one of them (iterations 18, 16, 18, 34, 61,
    28, 14, 18, 30, 46, 8, 22), so none had to be left out; 0 to 7 are used.  Contingency 4 reaches the iteration limit
    (status -1) on both: the queue files such a run like any other."""
    nb, ng, nl, seed = CASES["case14"]
    base = acopf_synth(nb, ng, nl, seed)
    nets = [base if s == 0 else contingency(base, s, seed) for s in QC.POLAR_SCENARIOS]
    n_sc = len(nets)
    assert n_sc >= 6
    lays = [acopf_layout(nt) for nt in nets]
    ps = [from_polar_acopf(nt, ly) for nt, ly in zip(nets, lays)]
    kw = dict(max_iter=60, use_soc=1, literal_quirks=0, **SQP_KW)
    cg = _ctx(lays[0], 2, **kw); cg.nlp_attach(ps[0]); cg.nlp_stream_begin(n_sc)
    cd = _ctx(lays[0], 2, **kw); cd.acopf_attach(nets[0], lays[0]); cd.stream_begin(n_sc)
    for s in range(n_sc):
        cg.nlp_stream_set(s, ps[s]); cd.stream_set(s, nets[s], lays[s])
    cg.stream_run(); cd.stream_run()
    for s in range(n_sc):
        rg, rd = cg.stream_get(s), cd.stream_get(s)
        print(f"contingency {QC.POLAR_SCENARIOS[s]}: status {rg['status']} / {rd['status']} iter {rg['iter']} / {rd['iter']} "
              f"rel |dx| {rel(rg['x'], rd['x']):.1e}")
        assert rd["iter"] >= 1
        assert (rg["status"], rg["iter"]) == (rd["status"], rd["iter"]), s
        assert rel(rg["x"], rd["x"]) < TOL, s
    cg.close(); cd.close()


# ---- 6. a queue shared between two contexts
class _Rank:
    """What run_shared_queue drives, with a record of the ids that moved."""

    def __init__(self, ctx):
        self.ctx, self.released, self.appended = ctx, [], []

    def run_some(self, k):
        return self.ctx.stream_run_some(k)

    def release(self, n):
        ids = self.ctx.stream_release(n)
        self.released += [int(v) for v in ids]
        return ids

    def append(self, ids):
        self.appended += [int(v) for v in ids]
        self.ctx.stream_append(ids)


def test_nlp_queue_shared_between_two_contexts():
    """Two contexts of one process standing in for two ranks (4 slots each, the tables of all 12 scenarios on both, ids
    split 10 / 2), driven by shard.run_shared_queue over an in-process exchange: every scenario is filed by exactly one
    of them with the bits of the batched run, and ids moved from the long queue to the short one."""
    ref, _ = _batch(2)
    ranks = [_Rank(_queue(2, 4)) for _ in range(2)]
    ranks[0].ctx.stream_assign(list(range(10))); ranks[1].ctx.stream_assign([10, 11])
    bar, box, errs = threading.Barrier(2, timeout=300), [None, None], []

    def exchange_of(rank):
        def exchange(obj):
            box[rank] = obj
            bar.wait()
            out = list(box)
            bar.wait()
            return out
        return exchange

    def drive(rank):
        try:
            run_shared_queue(ranks[rank], rank, 2, 4, chunk=2, exchange=exchange_of(rank), max_rounds=500)
        except BaseException as e:                       # noqa: BLE001  (reported below; the other thread must not wait for ever)
            errs.append((rank, repr(e)))
            bar.abort()

    th = [threading.Thread(target=drive, args=(r,)) for r in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs
    first = [[rk.ctx.stream_get(s) for s in range(M)] for rk in ranks]
    for s in range(M):
        its = [first[r][s]["iter"] for r in range(2)]
        assert sorted(its)[0] == -1 and sorted(its)[1] >= 1, (s, its)
        assert _same_result(first[int(its[1] >= 1)][s], ref[s]), s
    print("moved:", ranks[0].released, "->", ranks[1].appended)
    assert len(ranks[0].released) >= 1 and sorted(ranks[0].released) == sorted(ranks[1].appended) and not ranks[1].released
    for rk in ranks:
        rk.ctx.close()


# ---- 7. misuse
def test_queue_misuse_is_refused_with_a_message():
    base, lay, ps = QC.queue_problem()
    dp = pkg.host._dp
    P = lambda a: np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(dp)
    # _begin on an unattached, an ACOPF and a QCQP context
    ctx = _ctx(lay, 2, kkt_condense=1)
    L = ctx.L
    _expect(L.sqphip_nlp_stream_begin(ctx.h, 4, 0), EINVAL, ["sqphip_nlp_stream_begin", "sqphip_nlp_attach"], ctx)
    nb, ng, nl, seed = CASES["case14"]
    net = acopf_synth(nb, ng, nl, seed); al = acopf_layout(net)
    ca = _ctx(al, 2); ca.acopf_attach(net, al)
    _expect(L.sqphip_nlp_stream_begin(ca.h, 4, 0), EINVAL, ["sqphip_nlp_stream_begin", "sqphip_nlp_attach"], ca)
    _expect(L.sqphip_nlp_stream_set(ca.h, 0, *([None] * 7), P(al.x0)), EINVAL, ["sqphip_nlp_stream_set", "sqphip_nlp_stream_begin"], ca)
    ca.close()
    q = qcqp_synth(24, 14, seed=5); ql = qcqp_layout(q)
    cq = _ctx(ql, 2); cq.qcqp_attach(q)
    _expect(L.sqphip_nlp_stream_begin(cq.h, 4, 0), EINVAL, ["sqphip_nlp_stream_begin", "sqphip_nlp_attach"], cq)
    cq.qcqp_stream_begin(4)                              # ... whose own queue does not open the NLP one
    _expect(L.sqphip_nlp_stream_set(cq.h, 0, *([None] * 7), P(q.x0)), EINVAL, ["sqphip_nlp_stream_set", "sqphip_nlp_stream_begin"], cq)
    cq.close()
    ctx.nlp_attach(base)
    # _set before _begin, a queue without scenarios, then the per-call checks
    x0 = P(base.x0)
    nulls = [None] * 7
    _expect(L.sqphip_nlp_stream_set(ctx.h, 0, *nulls, x0), EINVAL, ["sqphip_nlp_stream_set", "sqphip_nlp_stream_begin"], ctx)
    _expect(L.sqphip_nlp_stream_begin(ctx.h, 0, 0), EINVAL, ["sqphip_nlp_stream_begin", "n_scenarios", "positive"], ctx)
    _expect(L.sqphip_nlp_stream_begin(ctx.h, -3, 1), EINVAL, ["sqphip_nlp_stream_begin", "n_scenarios", "positive"], ctx)
    ctx.nlp_stream_begin(4)
    _expect(L.sqphip_nlp_stream_set(ctx.h, 4, *nulls, x0), EINVAL, ["sqphip_nlp_stream_set", "scenario 4"], ctx)
    _expect(L.sqphip_nlp_stream_set(ctx.h, -1, *nulls, x0), EINVAL, ["sqphip_nlp_stream_set", "scenario -1"], ctx)
    _expect(L.sqphip_nlp_stream_set(ctx.h, 0, *nulls, None), EINVAL, ["sqphip_nlp_stream_set", "x0"], ctx)
    i = int(np.flatnonzero(base.gL != base.gU)[0])       # an inequality row
    gL, gU = base.gL.copy(), base.gU.copy(); gL[i], gU[i] = -np.inf, np.inf
    _expect(L.sqphip_nlp_stream_set(ctx.h, 0, None, None, P(gL), P(gU), None, None, None, x0), EINVAL,
            ["sqphip_nlp_stream_set", f"row {i} ", "unbounded"], ctx)
    gL, gU = base.gL.copy(), base.gU.copy(); gL[i] = gU[i]
    _expect(L.sqphip_nlp_stream_set(ctx.h, 0, None, None, P(gL), P(gU), None, None, None, x0), EINVAL,
            ["sqphip_nlp_stream_set", f"row {i} ", "equality", "kkt_condense"], ctx)
    assert L.sqphip_nlp_stream_set(ctx.h, 0, *nulls, x0) == 0
    with pytest.raises(TypeError):
        ctx.nlp_stream_set(0, x0=base.x0, av=base.tcoef)   # (a QCQP keyword)
    # the queue calls of the other evaluators still refuse an NLP context
    z = np.zeros(max(base.n, base.m)); d = P(z)
    _expect(L.sqphip_sqp_stream_begin(ctx.h, 4), EINVAL, ["sqphip_sqp_stream_begin", "NLP"], ctx)
    _expect(L.sqphip_sqp_stream_set(ctx.h, 0, d, d, d, d, d, d, d, d), EINVAL, ["sqphip_sqp_stream_set", "NLP"], ctx)
    _expect(L.sqphip_qcqp_stream_begin(ctx.h, 4, 0), EINVAL, ["sqphip_qcqp_stream_begin", "QCQP"], ctx)
    _expect(L.sqphip_qcqp_stream_set(ctx.h, 0, d, d, d, d, None, None, None, None, None, None, d), EINVAL, ["sqphip_qcqp_stream_set", "QCQP"], ctx)
    # ... and the queue still runs
    for s in range(1, 4):
        ctx.nlp_stream_set(s, ps[s])
    ctx.stream_run()
    assert ctx.stream_get(0)["iter"] >= 1
    ctx.close()
