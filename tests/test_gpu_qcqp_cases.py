"""The general sparse QCQP path on the device (sqphip_qcqp_attach's plan builder, csrc/qcqp_dev.hpp qcqp_eval, k_armijo<ARMIJO_QCQP>,
the SQP loop and the scenario queue on a QCQP context) on the cases of tests/qcqp_cases.py:

    plan edges      the hand-made edge model and its variants (no Q0 terms, no A terms, no Hessian structure), both
                    instances, every entry of f, grad, g, J and H against the exact rational reference
    past a stride   qcqp_synth with every loop of qcqp_eval in its third trip, slot 1, entry by entry
    partial outputs the outputs the SQP loop and the Armijo probe ask for: the bits of the all-outputs call, nothing else written
    Armijo          sqphip_acopf_armijo on a QCQP context against the backtracking loop over the exact reference
    SQP loop        1030 discs (n = 2060, m = 1030) against the closed form and the oracle
    queue           three disc scenarios through one slot: the bits of a batch of three, the block of the last one in the slot

The bound is |got - exact| <= max(gamma(L + 4) S, 2^-1074) per entry and an exact constant where no product feeds an entry
(tests/qcqp_cases.py): derived from the number formats, shown attainable on the CPU by tests/test_qcqp_cases_cpu.py, never
taken from device output."""
import ctypes as C

import numpy as np
import pytest

import sqpsolver_jl_amd as pkg
from sqpsolver_jl_amd.host import _d, _f
from sqpsolver_jl_amd.qcqp import qcqp_layout
import qcqp_cases as QC

pytestmark = pytest.mark.gpu
TOL = 1e-8                                   # tests/test_gpu_qcqp.py, against the oracle
SENTINEL = -7.25e300
FULL = ("x", "g", "mult_g", "mult_x_L", "mult_x_U")


def rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(1.0, np.abs(np.asarray(b)).max()))


def _ctx(lay, batch, **kw):
    return pkg.Context(lay.n, lay.m, lay.num_linear, lay.jrow, lay.jcol, lay.hrow, lay.hcol, lay.xL, lay.xU, lay.gL, lay.gU,
                       pkg.default_options(**kw), batch=batch)


def _case_ctx(cs):
    ctx = _ctx(cs.lay, len(cs.qs))
    ctx.qcqp_attach(cs.qs[0])
    for b, q in enumerate(cs.qs):
        ctx.qcqp_set_instance(b, q)
    return ctx


@pytest.fixture(scope="module")
def stride():
    cs = QC.stride_model()
    ctx = _case_ctx(cs)
    yield cs, ctx
    ctx.close()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ------------------------------------------------------------------------------------------------ 1. plan edges
@pytest.mark.parametrize("kind", QC.EDGE_KINDS)
def test_evaluator_at_the_plan_edges(kind):
    name = "edge-" + kind
    cs = QC.case(name)
    p = cs.point
    ctx = _case_ctx(cs)
    try:
        for slot in cs.slots:
            ev = ctx.acopf_eval(slot, p.x, p.sigma, p.lam)
            assert (ev["hval"] is None) == (kind == "noH")
            msgs, ratio = QC.check_all(ev, QC.exact(name, slot), cs.lay)
            print(name, "slot", slot, "largest |got - exact| / bound:", {k: round(v, 4) for k, v in ratio.items()})
            assert not msgs, f"{name} slot {slot}: {len(msgs)} entries, " + "; ".join(msgs[:8])
        other, _ = QC.check_all(ev, QC.exact(name, cs.slots[0]), cs.lay)          # the instances are told apart
        assert len(other) > 50
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ 2. past one stride
def test_evaluator_past_one_stride(stride):
    cs, ctx = stride
    p = cs.point
    ev = ctx.acopf_eval(1, p.x, p.sigma, p.lam)
    msgs, ratio = QC.check_all(ev, QC.exact("stride", 1), cs.lay)
    print("stride slot 1 largest |got - exact| / bound:", {k: round(v, 4) for k, v in ratio.items()})
    assert not msgs, f"{len(msgs)} entries, " + "; ".join(msgs[:8])
    other, _ = QC.check_all(ev, QC.exact("stride", 0), cs.lay)                    # slot 1 does not hold slot 0's values
    assert {m.split("[")[0] for m in other} == {"f", "grad", "g", "jval", "hval", "jsum", "hsum"} and len(other) > 1000


# ------------------------------------------------------------------------------------------------ 3. partial outputs
def _raw(ctx, inst, p, want, lam=True):
    """sqphip_acopf_eval with exactly the outputs `want`; every host buffer starts as the sentinel.  (rc, buffers)"""
    f = C.c_double(SENTINEL)
    buf = dict(grad=np.full(ctx.n, SENTINEL), g=np.full(ctx.m, SENTINEL), jval=np.full(ctx.nnzj, SENTINEL),
               hval=np.full(ctx.nnzh, SENTINEL))
    ptr = lambda k: _d(buf[k]) if k in want else None
    x, lm = _f(p.x), _f(p.lam)
    rc = ctx.L.sqphip_acopf_eval(ctx.h, inst, _d(x), float(p.sigma), _d(lm) if lam else None,
                                 C.byref(f) if "f" in want else None, ptr("grad"), ptr("g"), ptr("jval"), ptr("hval"))
    buf["f"] = np.array([f.value])
    return rc, buf


def test_partial_outputs_are_the_bits_of_the_full_call(stride):
    """All outputs, all but the Hessian with lambda = NULL (the loop before its first multipliers) and f and g alone (what
    k_armijo<ARMIJO_QCQP> asks of qcqp_eval).  An all-outputs call at another point goes before each, so that an entry a partial
    call failed to write shows as a value of the wrong point."""
    cs, ctx = stride
    p = cs.point
    other = QC.Point(p.x[::-1].copy(), 0.4, p.lam[::-1].copy())
    everything = ("f", "grad", "g", "jval", "hval")
    rc, full = _raw(ctx, 1, p, everything)
    assert rc == 0
    for k, v in full.items():
        assert not (v == SENTINEL).any(), f"output {k} of the all-outputs call has entries nobody wrote"
    msgs, _ = QC.check_all(dict(full, f=full["f"][0]), QC.exact("stride", 1), cs.lay)
    assert not msgs, msgs[:8]
    for want, lam in ((("f", "grad", "g", "jval"), False), (("f", "g"), False), (("f", "g"), True)):
        assert _raw(ctx, 1, other, everything)[0] == 0
        rc, got = _raw(ctx, 1, p, want, lam=lam)
        assert rc == 0, want
        for k, v in got.items():
            if k in want:
                assert np.array_equal(_bits(v), _bits(full[k])), f"request {want}: output {k} differs from the all-outputs call"
            else:
                assert (v == SENTINEL).all(), f"request {want}: output {k} was not requested and was written"
    ev = ctx.acopf_eval(1, p.x, p.sigma, None)                                    # the wrapper's lam = None
    assert ev["hval"] is None and all(np.array_equal(_bits(ev[k]), _bits(full[k])) for k in ("f", "grad", "g", "jval"))


# ------------------------------------------------------------------------------------------------ 4. Armijo
def test_armijo_on_a_qcqp_context_matches_a_backtracking_loop_over_the_exact_reference(stride):
    cs, ctx = stride
    x = QC.armijo_point()
    seen = set()
    for a in QC.armijo_cases():
        want, margin, phi0, D = QC.armijo_expected(a.name)
        got = ctx.acopf_armijo(QC.ARMIJO_SLOT, x, a.step, a.mu, phi0, D, a.eta, a.tau, a.min_alpha, a.fr)
        print("armijo", a.name, (a.mu, a.fr), got, want, "margin", margin)
        assert got == want, a.name
        seen.add((want[1], want[2] > 1))
    assert (True, True) in seen and (False, True) in seen                         # a backtracked valid step and an exhausted one


# ------------------------------------------------------------------------------------------------ 5. the SQP loop
def _disc_ctx(batch):
    q = QC.disc_model()
    ctx = _ctx(qcqp_layout(q), batch, kkt_mode=2, **QC.DISC_KW)
    ctx.qcqp_attach(q)
    return ctx


def test_sqp_loop_past_one_stride_reaches_the_closed_form():
    qs = [QC.disc_model(s=s) for s in (0, 1)]
    ctx = _disc_ctx(2)
    try:
        for b in range(2):
            ctx.qcqp_set_instance(b, qs[b])
        ctx.sqp_reset(); ctx.sqp_run(0)
        for b in range(2):
            rg, ro = ctx.sqp_get(b), QC.disc_oracle(b)
            x, obj, mult = QC.disc_optimum(qs[b])
            print(f"disc scenario {b}: status {rg['status']} iter {rg['iter']} (oracle {ro['status']}, {ro['iter']}) "
                  f"|x - closed form| {np.abs(rg['x'] - x).max():.2e} |obj - closed form| {abs(rg['obj_val'] - obj):.2e} "
                  f"|mult_g - closed form| {np.abs(rg['mult_g'] - mult).max():.2e} rel |x - oracle| {rel(rg['x'], ro['x']):.2e}")
            assert rg["status"] == 0, b
            assert np.abs(rg["x"] - x).max() <= 1e-6 and abs(rg["obj_val"] - obj) <= 1e-6, b
            assert (rg["status"], rg["iter"]) == (ro["status"], ro["iter"]), b
            assert rel(rg["x"], ro["x"]) < TOL and abs(rg["obj_val"] - ro["obj_val"]) <= TOL * max(1.0, abs(ro["obj_val"])), b
            assert np.abs(rg["mult_g"] - mult).max() <= 1e-6, b                   # the sign: qcqp_cases.disc_optimum
        assert not np.array_equal(ctx.sqp_get(0)["x"], ctx.sqp_get(1)["x"])
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ 6. the queue
def test_queue_copies_a_qcqp_block_past_two_trips():
    """5151 values padded to 5152 = 2576 double2: the copy of the block makes a second trip that ends in its one-access tail.
    Three scenarios run through ONE slot, so the slot holds the previous scenario's block when the next is loaded."""
    qs = [QC.disc_model(s=s) for s in range(3)]
    assert QC.nvalues(qs[0]) == 5151
    cb = _disc_ctx(3)
    for b in range(3):
        cb.qcqp_set_instance(b, qs[b])
    cb.sqp_reset(); cb.sqp_run(0)
    ref = [cb.sqp_get(b) for b in range(3)]
    cb.close()
    ctx = _disc_ctx(1)
    try:
        ctx.qcqp_stream_begin(3, keep_multipliers=True)
        for s in range(3):
            ctx.qcqp_stream_set(s, qs[s])
        ctx.stream_run()
        for s in range(3):
            r = ctx.stream_get_full(s)
            print(f"scenario {s}: status {r['status']} iter {r['iter']} (batch {ref[s]['iter']}) obj {r['obj_val']:.12g}")
            assert r["status"] == 0, s
            for k in FULL:
                assert np.array_equal(r[k], ref[s][k]), (s, k)
            assert (r["obj_val"], r["status"], r["iter"]) == (ref[s]["obj_val"], ref[s]["status"], ref[s]["iter"]), s
        assert len({ref[s]["obj_val"] for s in range(3)}) == 3
        rng = np.random.default_rng(51)
        lay = qcqp_layout(qs[0])
        x, sigma, lam = rng.uniform(-2.0, 2.0, lay.n), 1.3, rng.standard_normal(lay.m)
        ev = ctx.acopf_eval(0, x, sigma, lam)
        msgs, ratio = QC.check_all(ev, QC.QcqpExact(qs[2]).all(x, sigma, lam, lay), lay)
        print("slot 0 against the last scenario, largest |got - exact| / bound:", {k: round(v, 4) for k, v in ratio.items()})
        assert not msgs, f"{len(msgs)} entries, " + "; ".join(msgs[:8])
        second, _ = QC.check_all(ev, QC.QcqpExact(qs[1]).all(x, sigma, lam, lay), lay)
        assert {m.split("[")[0] for m in second} == {"f", "grad"} and len(second) > 2000     # (the scenarios differ in c)
    finally:
        ctx.close()
