"""The three dedicated ACOPF evaluators of csrc/acopf_dev.hpp (the polar body of acopf_eval_dedicated, acr_eval, acwr_eval)
through `sqphip_acopf_eval`, on the cases of tests/acopf_cases.py:

    small cases     the topologies of real case files (parallel and reversed branches, br_sig = -1, a reference bus in the
                    middle, several or no generators at a bus, a hub, outages, phase shifters, shunts, dc lines), every
                    form and point, every entry of f, grad, g, J and H against the 50-digit reference of tests/acopf_ref.py
    stride cases    every thread loop (buses, generators, shunts, dc lines, branches, bus pairs) just below, at and just
                    above one stride of 1024 threads, the branch loop past two: every entry against the oracle under the
                    same scaled bound, f and g against the 50-digit reference as well
    partial requests  the subsets of outputs the SQP loop asks for: bit-identical to the all-outputs call, nothing else
                    written, H without lambda refused
    slots           three different networks in a batch of three, each against its own reference; no slot sees another

The bound is |got - ref| <= K 2^-52 scale per entry and an exact zero where the reference has one, with the scales of
acopf_ref.py and the constants of acopf_cases.py -- measured on the CPU oracle by tests/test_acopf_cases_cpu.py, never
against device output."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import sqpsolver_jl_amd as pkg
from sqpsolver_jl_amd.host import _d, _f
import acopf_cases as AC
import acopf_ref as AR

pytestmark = pytest.mark.gpu

SMALL = [(n, f) for n in AC.SMALL_NAMES for f in AC.FORMS]
STRIDE = [(n, f) for n in AC.STRIDE_NAMES for f in AC.FORMS]
EINVAL = -1
SENTINEL = -7.25e300
SUBSETS = (("f",), ("g",), ("f", "g"), ("grad", "J"), ("H",), ("f", "grad", "g", "J", "H"))


def _context(net, lay, batch):
    ctx = pkg.Context(lay.n, lay.m, lay.num_linear, lay.jrow, lay.jcol, lay.hrow, lay.hcol, lay.xL, lay.xU, lay.gL, lay.gU,
                      batch=batch)
    ctx.acopf_attach(net, lay)
    for b in range(batch):
        ctx.acopf_set_instance(b, net, lay)
    return ctx


@pytest.fixture(scope="module", params=SMALL, ids=[f"{n}-{f}" for n, f in SMALL])
def small(request):
    """One context of batch 2 per (case, form): every point is evaluated on it"""
    name, form = request.param
    ctx = _context(AC.net_of(name), AC.layout(name, form), 2)
    yield name, form, ctx
    ctx.close()


@pytest.fixture(scope="module", params=STRIDE, ids=[f"{n}-{f}" for n, f in STRIDE])
def stride(request):
    name, form = request.param
    ctx = _context(AC.net_of(name), AC.layout(name, form), 1)
    yield name, form, ctx
    ctx.close()


def _raw(ctx, inst, p, want, lam=True):
    """sqphip_acopf_eval with exactly the outputs `want`; every host buffer starts as the sentinel.  (rc, buffers)"""
    f = C.c_double(SENTINEL)
    buf = dict(grad=np.full(ctx.n, SENTINEL), g=np.full(ctx.m, SENTINEL), J=np.full(ctx.nnzj, SENTINEL),
               H=np.full(ctx.nnzh, SENTINEL))
    ptr = lambda k: _d(buf[k]) if k in want else None
    x, lm = _f(p.x), _f(p.lam)
    rc = ctx.L.sqphip_acopf_eval(ctx.h, inst, _d(x), float(p.sigma), _d(lm) if lam else None,
                                 C.byref(f) if "f" in want else None, ptr("grad"), ptr("g"), ptr("J"), ptr("H"))
    buf["f"] = np.array([f.value])
    return rc, buf


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _partial_requests(ctx, inst, p, other):
    """`other`: another point.  The instance's device buffers keep what the last call left in them, so an all-outputs call
    at `other` goes before every partial request: an entry the partial call failed to write then shows as a value of the
    wrong point, not as the right one left over."""
    rc, full = _raw(ctx, inst, p, SUBSETS[-1])
    assert rc == 0
    for k, v in full.items():
        assert not (v == SENTINEL).any(), f"output {k} of the all-outputs call has entries nobody wrote"
    for want in SUBSETS[:-1]:
        assert _raw(ctx, inst, other, SUBSETS[-1])[0] == 0
        rc, got = _raw(ctx, inst, p, want)
        assert rc == 0, want
        for k, v in got.items():
            if k in want:
                assert np.array_equal(_bits(v), _bits(full[k])), f"request {want}: output {k} differs from the all-outputs call"
            else:
                assert (v == SENTINEL).all(), f"request {want}: output {k} was not requested and was written"
    rc, got = _raw(ctx, inst, p, ("H",), lam=False)
    assert rc == EINVAL and (got["H"] == SENTINEL).all()
    rc, again = _raw(ctx, inst, p, SUBSETS[-1])
    assert rc == 0 and all(np.array_equal(_bits(again[k]), _bits(full[k])) for k in full)


# ------------------------------------------------------------------------------------------------ small cases
def test_small_cases_match_the_reference_entry_by_entry(small):
    name, form, ctx = small
    M, lay = AC.model(name, form), AC.layout(name, form)
    for k in range(AC.NPOINTS):
        p = AC.points(name, form)[k]
        ev = ctx.acopf_eval(1, p.x, p.sigma, p.lam)
        msgs = AC.check(M, lay, AC.reference(name, form, k), ev)
        assert not msgs, f"{name} {form} point {k}: " + "; ".join(msgs[:8])


def test_small_cases_partial_requests(small):
    name, form, ctx = small
    pts = AC.points(name, form)
    for inst, k in ((0, 0), (1, 2)):
        _partial_requests(ctx, inst, pts[k], pts[1])


# ------------------------------------------------------------------------------------------------ stride cases
def test_stride_cases_match_the_oracle_entry_by_entry(stride):
    name, form, ctx = stride
    M = AC.model(name, form)
    for k in (1, 2):
        p = AC.points(name, form)[k]
        ev = ctx.acopf_eval(0, p.x, p.sigma, p.lam)
        msgs = AC.check_against_oracle(name, form, k, ev)
        assert not msgs, f"{name} {form} point {k}: {len(msgs)} entries, " + "; ".join(msgs[:8])
    f, g, fscale = AC.reference_values(name, form, 2)
    R = AC.oracle_reference(name, form, 2)
    msgs = AR.compare(M, "f", ev["f"], f, fscale, AC.K["f"]) + AR.compare(M, "g", ev["g"], g, R.gscale, AC.K["g"])
    assert not msgs, f"{name} {form} against the 50-digit values: " + "; ".join(msgs[:8])


def test_stride_cases_partial_requests(stride):
    name, form, ctx = stride
    pts = AC.points(name, form)
    _partial_requests(ctx, 0, pts[2], pts[1])


# ------------------------------------------------------------------------------------------------ slots
def _variants(net):
    """(base, an outage contingency with scaled loads, a tap / shift / cost variant): one topology, three instances"""
    out = dataclasses.replace(net, status=net.status.copy(), pd=1.05 * net.pd, qd=1.05 * net.qd)
    out.status[int(np.flatnonzero(net.status)[4])] = 0.0
    rng = np.random.default_rng(5)
    tap = np.ones(net.nl) if net.tap is None else net.tap
    shift = np.zeros(net.nl) if net.shift is None else net.shift
    var = dataclasses.replace(net, tap=tap * rng.uniform(0.95, 1.05, net.nl), shift=shift + rng.uniform(-0.05, 0.05, net.nl),
                              c2=net.c2 * rng.uniform(0.5, 2.0, net.ng), c1=net.c1 * rng.uniform(0.5, 2.0, net.ng))
    return net, out, var


@pytest.mark.parametrize("form", AC.FORMS)
def test_slots_hold_their_own_networks(form):
    name = "combined"
    nets = _variants(AC.net_of(name))
    lays = [AC.LAYOUT[form](nt) for nt in nets]
    lay = lays[0]
    p = AC.points(name, form)[2]
    ctx = pkg.Context(lay.n, lay.m, lay.num_linear, lay.jrow, lay.jcol, lay.hrow, lay.hcol, lay.xL, lay.xU, lay.gL, lay.gU,
                      batch=3)
    try:
        ctx.acopf_attach(nets[0], lay)
        for b in range(3):
            ctx.acopf_set_instance(b, nets[b], lays[b])
        first = []
        for b in range(3):
            M = AR.Model(nets[b], form)
            ref = AC.reference(name, form, 2) if b == 0 else AR.combine(M, AR.derivatives(M, p.x), p.sigma, p.lam)
            ev = ctx.acopf_eval(b, p.x, p.sigma, p.lam)
            msgs = AC.check(M, lays[b], ref, ev)
            assert not msgs, f"slot {b}: " + "; ".join(msgs[:8])
            first.append(ev)
        assert not np.array_equal(first[0]["g"], first[1]["g"]) and not np.array_equal(first[0]["hval"], first[2]["hval"])
        # evaluating slot 1 does not change what slot 0 then returns
        again = ctx.acopf_eval(0, p.x, p.sigma, p.lam)
        for k in ("grad", "g", "jval", "hval"):
            assert np.array_equal(_bits(again[k]), _bits(first[0][k])), k
        assert again["f"] == first[0]["f"]
        # the same network in slots 0 and 2: the same bits
        ctx.acopf_set_instance(2, nets[0], lays[0])
        e0, e2 = ctx.acopf_eval(0, p.x, p.sigma, p.lam), ctx.acopf_eval(2, p.x, p.sigma, p.lam)
        for k in ("grad", "g", "jval", "hval"):
            assert np.array_equal(_bits(e0[k]), _bits(e2[k])) and np.array_equal(_bits(e0[k]), _bits(first[0][k])), k
        assert e0["f"] == e2["f"] == first[0]["f"]
        # ... and slot 1 still holds the contingency
        e1 = ctx.acopf_eval(1, p.x, p.sigma, p.lam)
        assert all(np.array_equal(_bits(e1[k]), _bits(first[1][k])) for k in ("grad", "g", "jval", "hval"))
    finally:
        ctx.close()
