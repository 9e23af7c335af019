"""The scenario queue on a QCQP context (sqphip_qcqp_stream_begin / _set, sqphip_sqp_stream_get_full): more scenarios than
slots for any sparse QCQP.  The queue against the ordinary batched run bit for bit (the QCQP evaluator does not depend on
the slot), the multipliers filed with a result, NULL parts of a scenario, the generic queue against the dedicated ACOPF
queue, a queue shared between two contexts, misuse."""
import dataclasses
import functools
import os
import sys
import threading

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import sqpsolver_jl_amd as pkg                                        # noqa: E402
from sqpsolver_jl_amd.acopf_synth import acopf_synth, acr_layout, contingency, CASES   # noqa: E402
from sqpsolver_jl_amd.qcqp import qcqp_layout, qcqp_scenario, qcqp_synth   # noqa: E402
from sqpsolver_jl_amd.shard import run_shared_queue                    # noqa: E402
from oracle import oracle as O                                        # noqa: E402
from qcqp_ref import extract                                          # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-8                                   # tests/test_gpu_qcqp.py, between the generic and the dedicated evaluator
SQP_KW = dict(tol_infeas=1e-6, tol_residual=1e-4)
EINVAL, ESTATE = -1, -4
M = 12
FULL = ("x", "g", "mult_g", "mult_x_L", "mult_x_U")


# ---- helpers (tests/test_gpu_qcqp.py; a test module is not imported)
def rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(1.0, np.abs(np.asarray(b)).max()))


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


def _expect(rc, code, words, ctx):
    assert rc == code, rc
    msg = ctx.L.sqphip_last_error(ctx.h).decode()
    assert all(w in msg for w in words), msg


def _problem():
    q = qcqp_synth(24, 14, seed=5)
    return q, qcqp_layout(q), [qcqp_scenario(q, s, 5) for s in range(M)]


def _kw(kkt_mode):
    """The options of test_scenario_queue_gives_the_batch_results: with the textbook Hessian sign the scenarios converge, after
    different numbers of iterations, so the slots of the queue refill at different times (with the reference's sign every run
    of this problem lasts to the iteration limit)."""
    return dict(kkt_mode=kkt_mode, max_iter=60, use_soc=1, literal_quirks=0, **SQP_KW)


@functools.lru_cache(maxsize=None)
def _batch(kkt_mode):
    """The 12 scenarios in an ordinary batch of 12: (sqp_get of every instance, the work counters)."""
    q, lay, qs = _problem()
    ctx = _ctx(lay, M, **_kw(kkt_mode))
    ctx.qcqp_attach(q)
    for b in range(M):
        ctx.qcqp_set_instance(b, qs[b])
    ctx.sqp_reset(); ctx.sqp_run(0)
    ref = [ctx.sqp_get(b) for b in range(M)]
    c = ctx.counters()
    ctx.close()
    return ref, (c["n_qp"], c["n_ipm_iter"], c["n_factor"])


def _queue(kkt_mode, slots, keep=False):
    q, lay, qs = _problem()
    ctx = _ctx(lay, slots, **_kw(kkt_mode))
    ctx.qcqp_attach(q)
    ctx.qcqp_stream_begin(M, keep_multipliers=keep)
    for s in range(M):
        ctx.qcqp_stream_set(s, qs[s])
    return ctx


def _same_result(r, ref):
    return (r["status"], r["iter"]) == (ref["status"], ref["iter"]) and r["obj_val"] == ref["obj_val"] and \
        np.array_equal(r["x"], ref["x"])


# ---- 1. queue = batch, bit for bit
@pytest.mark.parametrize("kkt_mode", [2, 1])
@pytest.mark.parametrize("slots", [4, 64])
def test_qcqp_queue_gives_the_batch_results(kkt_mode, slots):
    """12 scenarios of the synthetic QCQP through 4 slots (three per slot, refilled on the device) and through 64 slots (more
    slots than scenarios; on the sparse path four instance groups): status, iterations, objective and point of the
    ordinary batch of 12, bit for bit, and the same totals of sub-problems, interior-point iterations, factorisations."""
    ref, tot = _batch(kkt_mode)
    ctx = _queue(kkt_mode, slots)
    ctx.stream_run()
    for s in range(M):
        r = ctx.stream_get(s)
        print(f"kkt_mode {kkt_mode} slots {slots} scenario {s}: status {r['status']} iter {r['iter']} (batch {ref[s]['iter']}) "
              f"|dx| {np.abs(r['x'] - ref[s]['x']).max():.1e}")
        assert _same_result(r, ref[s]), s
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
def test_qcqp_queue_files_the_multipliers(kkt_mode, slots):
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
    ctx.close()


def test_get_full_without_the_tables_is_a_state_error():
    ctx = _queue(2, 4, keep=False)
    ctx.stream_run()
    x = np.zeros(ctx.n)
    rc = ctx.L.sqphip_sqp_stream_get_full(ctx.h, 0, x.ctypes.data_as(pkg.host._dp), None, None, None, None, None, None, None)
    _expect(rc, ESTATE, ["keep_multipliers"], ctx)
    with pytest.raises(pkg.SqpHipError):
        ctx.stream_get_full(0)
    ctx.close()


# ---- 3. NULL parts mean the values of the attach
def test_null_parts_of_a_scenario_are_the_values_of_the_attach():
    q, lay, qs = _problem()
    kw = _kw(2)
    av = qs[5].av
    ref_ctx = _ctx(lay, 2, **kw)
    ref_ctx.qcqp_attach(q)
    ref_ctx.qcqp_set_instance(0, dataclasses.replace(q, av=av))
    ref_ctx.qcqp_set_instance(1, q)
    ref_ctx.sqp_reset(); ref_ctx.sqp_run(0)
    ref = [ref_ctx.sqp_get(b) for b in range(2)]
    ref_ctx.close()
    ctx = _ctx(lay, 4, **kw)
    ctx.qcqp_attach(q)
    for b in range(4):                                   # every slot's block now holds other values than the attach gave
        ctx.qcqp_set_instance(b, qs[1 + b])
    ctx.qcqp_stream_begin(2, keep_multipliers=True)
    ctx.qcqp_stream_set(0, av=av, x0=q.x0)               # bounds: those of the context; values: the attach's, and av
    ctx.qcqp_stream_set(1, x0=q.x0)
    ctx.stream_run()
    for s in range(2):
        r = ctx.stream_get_full(s)
        for k in FULL:
            assert np.array_equal(r[k], ref[s][k]), (s, k)
        assert (r["obj_val"], r["status"], r["iter"]) == (ref[s]["obj_val"], ref[s]["status"], ref[s]["iter"]), s
    assert not np.array_equal(ref[0]["x"], ref[1]["x"])
    ctx.close()


# ---- 4. generic queue = dedicated queue
def test_generic_queue_equals_dedicated_acr_queue_on_contingencies():
    """8 IEEE-14-shaped contingencies in rectangular coordinates through the QCQP queue and through the ACOPF queue, 4 slots
    each: the same status and iteration count, the point within the tolerance the two evaluators are held to in a batch."""
    nets = [_net("case14-taps-shunts", s) for s in range(8)]
    lays = [acr_layout(nt) for nt in nets]
    qs = extract([O.problem_acopf(nt, ly) for nt, ly in zip(nets, lays)])
    kw = dict(max_iter=60, use_soc=1, literal_quirks=0, **SQP_KW)
    cg = _ctx(lays[0], 4, **kw); cg.qcqp_attach(qs[0]); cg.qcqp_stream_begin(8)
    cd = _ctx(lays[0], 4, **kw); cd.acopf_attach(nets[0], lays[0]); cd.stream_begin(8)
    for s in range(8):
        cg.qcqp_stream_set(s, qs[s]); cd.stream_set(s, nets[s], lays[s])
    cg.stream_run(); cd.stream_run()
    for s in range(8):
        rg, rd = cg.stream_get(s), cd.stream_get(s)
        print(f"scenario {s}: status {rg['status']} / {rd['status']} iter {rg['iter']} / {rd['iter']} rel |dx| {rel(rg['x'], rd['x']):.1e}")
        assert rd["iter"] >= 1
        assert (rg["status"], rg["iter"]) == (rd["status"], rd["iter"]), s
        assert rel(rg["x"], rd["x"]) < TOL, s
    cg.close(); cd.close()


# ---- 5. a queue shared between two contexts
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


def test_qcqp_queue_shared_between_two_contexts():
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
    # a second pass on one context: its queue holds the ids it solved, and it files them again with the same bits
    ranks[1].ctx.stream_run()
    for s in range(M):
        a, b = first[1][s], ranks[1].ctx.stream_get(s)
        assert a["iter"] == b["iter"], s
        if a["iter"] >= 1:
            assert _same_result(b, ref[s]), s
    for rk in ranks:
        rk.ctx.close()


# ---- 6. misuse
def test_queue_misuse_is_refused_with_a_message():
    q, lay, qs = _problem()
    dp = pkg.host._dp
    P = lambda a: np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(dp)
    # the new _begin on an unattached context and on an ACOPF context
    ctx = _ctx(lay, 2, kkt_condense=1)
    L = ctx.L
    _expect(L.sqphip_qcqp_stream_begin(ctx.h, 4, 0), EINVAL, ["sqphip_qcqp_attach"], ctx)
    net = _net("case14", 0); al = acr_layout(net)
    ca = _ctx(al, 2); ca.acopf_attach(net, al)
    _expect(L.sqphip_qcqp_stream_begin(ca.h, 4, 0), EINVAL, ["sqphip_qcqp_attach"], ca)
    ca.close()
    ctx.qcqp_attach(q)
    # _set before _begin, then the per-call checks
    x0 = P(q.x0)
    nulls = [None] * 10
    _expect(L.sqphip_qcqp_stream_set(ctx.h, 0, *nulls, x0), EINVAL, ["sqphip_qcqp_stream_begin"], ctx)
    ctx.qcqp_stream_begin(4)
    _expect(L.sqphip_qcqp_stream_set(ctx.h, 4, *nulls, x0), EINVAL, ["scenario 4"], ctx)
    _expect(L.sqphip_qcqp_stream_set(ctx.h, -1, *nulls, x0), EINVAL, ["scenario -1"], ctx)
    _expect(L.sqphip_qcqp_stream_set(ctx.h, 0, *nulls, None), EINVAL, ["x0"], ctx)
    i = int(np.flatnonzero(q.gL != q.gU)[0])             # an inequality row
    gL, gU = q.gL.copy(), q.gU.copy(); gL[i], gU[i] = -np.inf, np.inf
    _expect(L.sqphip_qcqp_stream_set(ctx.h, 0, None, None, P(gL), P(gU), *([None] * 6), x0), EINVAL, [f"row {i} ", "unbounded"], ctx)
    gL, gU = q.gL.copy(), q.gU.copy(); gL[i] = gU[i]
    _expect(L.sqphip_qcqp_stream_set(ctx.h, 0, None, None, P(gL), P(gU), *([None] * 6), x0), EINVAL, [f"row {i} ", "equality"], ctx)
    assert L.sqphip_qcqp_stream_set(ctx.h, 0, *nulls, x0) == 0
    # the ACOPF queue calls still refuse a QCQP context
    _expect(L.sqphip_sqp_stream_begin(ctx.h, 4), EINVAL, ["QCQP"], ctx)
    _expect(L.sqphip_sqp_stream_set(ctx.h, 0, *([None] * 8)), EINVAL, ["QCQP"], ctx)
    ctx.close()
