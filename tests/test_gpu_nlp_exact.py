"""The term evaluator of a factorable NLP (csrc/nlp_dev.hpp nlp_eval, nlp_factor, nlp_kappa_wide) against the exact reference
of tests/nlp_exact.py, entry by entry under its forward error bound -- no floor relative to the largest entry: the menu at
its edge arguments through every attach entry point, the partial requests of pass 1, products, more than one stride of the
thread loops, the per-instance data of sqphip_nlp_attach_data, and the menu through the blocks' nlp_block_kappa.
tests/test_nlp_exact_cpu.py vouches for the reference and the cases."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import sqpsolver_jl_amd as pkg                                        # noqa: E402
from sqpsolver_jl_amd.nlp_terms import (ATAN, COS, POW, POWR, SIN, SQRT, TANH, NlpBlock, make_nlp_terms,   # noqa: E402
                                        needs_general, nlp_terms_layout)
import nlp_exact as X                                                  # noqa: E402
from nlp_block_ref import NlpBlockRef, check_outputs, edge_block_data, kappa_mp   # noqa: E402

pytestmark = pytest.mark.gpu
_dp = C.POINTER(C.c_double)


def _d(a):
    return None if a is None else a.ctypes.data_as(_dp)


def _ctx(lay, batch):
    return pkg.Context(lay.n, lay.m, lay.num_linear, lay.jrow, lay.jcol, lay.hrow, lay.hcol, lay.xL, lay.xU, lay.gL, lay.gU,
                       pkg.default_options(), batch=batch)


def _partial(ctx, inst, x, sigma, want_grad):
    """sqphip_acopf_eval without the Hessian (want_grad) or with f and g alone: the d2 and d1 switches of pass 1"""
    f = C.c_double(); g = np.zeros(ctx.m); xx = np.ascontiguousarray(x, dtype=np.float64)
    grad, jv = (np.zeros(ctx.n), np.zeros(ctx.nnzj)) if want_grad else (None, None)
    ctx._ck(ctx.L.sqphip_acopf_eval(ctx.h, inst, _d(xx), float(sigma), None, C.byref(f), _d(grad), _d(g), _d(jv), None))
    return dict(f=f.value, g=g, grad=grad, jval=jv)


def _check(ctx, inst, c, label):
    """the full call under the bound; the f / g-only call and the call without the Hessian return its bits"""
    R = X.NlpExact(c.p)
    val, bnd = R.want(c.x, c.sigma, c.lam, c.lay)
    assert R.domain_ok()
    ev = ctx.acopf_eval(inst, c.x, c.sigma, c.lam)
    worst, per_kind = X.check_entries(ev, val, bnd, R.exact, R.entry_kind, label)
    for want_grad in (False, True):
        part = _partial(ctx, inst, c.x, c.sigma, want_grad)
        for k, v in part.items():
            assert v is None or np.array_equal(np.asarray(v), np.asarray(ev[k])), (label, want_grad, k)
    ev2 = ctx.acopf_eval(inst, c.x, c.sigma, c.lam)                       # (the partial calls left nothing behind)
    assert all(np.array_equal(np.asarray(ev[k]), np.asarray(ev2[k])) for k in X.KEYS), label
    return ev


def _one(c, label, **attach):
    ctx = _ctx(c.lay, 1)
    ctx.nlp_attach(c.p, **attach); ctx.nlp_set_instance(0, c.p)
    ev = _check(ctx, 0, c, label)
    ctx.close()
    return ev


# ---- 1. the menu through every entry point
@pytest.mark.parametrize("variant", ["plain", "chain"])
def test_menu_through_sqphip_nlp_attach(variant):
    c = X.menu_model(variant, X.OLD_KINDS)
    assert c.p.aptr is None and not needs_general(c.p)
    _one(c, f"sqphip_nlp_attach {variant}", general=False)


def test_menu_through_sqphip_nlp_attach_affine():
    c = X.menu_model("affine", X.OLD_KINDS)
    assert c.p.aptr is not None and not needs_general(c.p)
    _one(c, "sqphip_nlp_attach_affine", general=False)


@pytest.mark.parametrize("variant", ["plain", "chain", "affine"])
def test_menu_through_sqphip_nlp_attach_general(variant):
    _one(X.menu_model(variant), f"sqphip_nlp_attach_general {variant}", general=True)


def test_menu_through_sqphip_nlp_attach_data_and_a_swap_of_two_instances_data():
    cs = X.menu_model("data")
    ctx = _ctx(cs[0].lay, 3)
    ctx.nlp_attach(cs[0].p, instance_data=True)
    for b, c in enumerate(cs):
        ctx.nlp_set_instance(b, c.p)
    evs = [_check(ctx, b, c, f"sqphip_nlp_attach_data instance {b}") for b, c in enumerate(cs)]
    assert not np.array_equal(evs[0]["g"], evs[2]["g"]) and not np.array_equal(evs[0]["g"], evs[1]["g"])
    ctx.nlp_set_instance(0, cs[2].p); ctx.nlp_set_instance(2, cs[0].p)       # swap the data of slots 0 and 2
    for slot, src in ((0, 2), (2, 0), (1, 1)):
        ev = ctx.acopf_eval(slot, cs[src].x, cs[src].sigma, cs[src].lam)
        for k in X.KEYS:
            assert np.array_equal(np.asarray(ev[k]), np.asarray(evs[src][k])), (slot, k)
    ctx.close()


# ---- 2. products and strides
def test_products_shared_variables_and_the_slot_of_64_summands():
    c = X.product_model()
    ev = _one(c, "product_model")
    s11 = int(np.flatnonzero((c.lay.hrow == 1) & (c.lay.hcol == 1))[0])
    assert ev["jval"][-1] == 0.0 and ev["hval"][-2] == 0.0 and ev["hval"][-1] == 0.0 and ev["hval"][s11] != 0.0


def test_beyond_one_stride_of_every_thread_loop():
    c = X.stride_model()
    assert min(len(c.p.fkind), len(c.p.trow), c.p.n, c.p.m, len(c.lay.jrow), len(c.lay.hrow)) > 1024
    ev = _one(c, "stride_model")
    for k in ("grad", "g", "jval", "hval"):
        assert np.all(ev[k][1024:] != 0.0), k


# ---- 3. the menu through the blocks' nlp_block_kappa
# the kinds nlp_block_ref.EDGE_KINDS leaves out.  The arguments are the menu's within what block_reference's 2^-200 grids hold:
# kappa, kappa', kappa'' of a magnitude in [2^-100, 2^100] (or 0)
BLOCK_MENU = [(TANH, 0.0, [5.0, -5.0, 10.0, -10.0, 20.0, -20.0]), (ATAN, 0.0, X.MENU[ATAN]), (SQRT, 0.0, X.MENU[SQRT]),
              (SIN, 0.0, X.MENU[SIN]), (COS, 0.0, X.MENU[COS])] + [(POWR, p_, list(X.POWR_U)) for p_ in X.POWR_P]


def _in_grid(kind, par, u):
    with X.mp.workdps(50):
        ks = [abs(v) for v in kappa_mp(kind, 1, par, X.mp.mpf(u))]
    return all(v == 0 or 2.0 ** -100 <= v <= 2.0 ** 100 for v in ks) and 2.0 ** -100 <= abs(u) <= 2.0 ** 100


@pytest.mark.parametrize("kind,par,us", BLOCK_MENU, ids=[f"{X.KIND_NAMES[k]}-{p_}" for k, p_, _ in BLOCK_MENU])
def test_menu_through_one_point_one_column_blocks(kind, par, us):
    """N = 1, d = 1, A = 1, S = 0, W = 1: f, grad_1 and the Hessian slot are kappa, kappa', sigma kappa'' of x_1, so the floor
    of check_outputs is relative to the entry itself.  (Variable 2 carries a term of 2^-1000 x^2: an attach wants a term.)"""
    us = [u for u in us if _in_grid(kind, par, u)]
    assert len(us) >= 3
    p = make_nlp_terms(2, 0, 0, [(0, 2.0 ** -1000, [(2, POW, 2)])], blocks=[NlpBlock(kind, [1], [[1.0]], par=par)])
    lay = nlp_terms_layout(p)
    ctx = _ctx(lay, 1)
    ctx.nlp_attach(p); ctx.nlp_set_instance(0, p)
    R = NlpBlockRef(p)
    for u in us:
        x = np.array([u, 1.0])
        val, bnd = R.want(x, 0.7, np.zeros(0), lay)
        check_outputs(ctx.acopf_eval(0, x, 0.7, np.zeros(0)), val, bnd, f"{X.KIND_NAMES[kind]} {par} at {u}")
    ctx.close()


@pytest.mark.parametrize("kind,par", [(TANH, 0.0), (ATAN, 0.0), (SQRT, 0.0), (POWR, 1.5), (POWR, -0.7), (SIN, 0.0), (COS, 0.0)],
                         ids=lambda v: str(v))
def test_the_same_kinds_in_a_block_of_5_points_and_17_columns(kind, par):
    N, d = 5, 17
    A, inst = edge_block_data(N, d, kind, 1, positive=kind in (SQRT, POWR))
    w, s = inst[0]
    if kind == TANH:
        s = s + np.array([5.0, -10.0, 20.0, -5.0, 10.0])
    rng = np.random.default_rng([N, d, kind])
    p = make_nlp_terms(d, 0, 0, [(0, 0.3, [(j + 1, POW, 2, 1.0, -0.2)]) for j in range(d)],
                       blocks=[NlpBlock(kind, rng.permutation(d) + 1, A, s, w, par=par)])
    lay = nlp_terms_layout(p)
    ctx = _ctx(lay, 1)
    ctx.nlp_attach(p); ctx.nlp_set_instance(0, p)
    x = rng.uniform(0.6, 1.4, d)
    val, bnd = NlpBlockRef(p).want(x, 0.7, np.zeros(0), lay)
    check_outputs(ctx.acopf_eval(0, x, 0.7, np.zeros(0)), val, bnd, f"(5, 17) {X.KIND_NAMES[kind]} {par}")
    ctx.close()
