"""The exact reference of the term evaluator and its cases (tests/nlp_exact.py), without a GPU: the reference agrees with
itself at 60 and 400 digits, every case meets the domain condition, the ordered-pair numpy reference lies within the bound
where it is sound, the cases reach every kind at every derivative order, six wrong evaluators miss the bound exactly where
they are wrong, and the numpy mirror of the device formulas (nlp_terms._kappa3) meets it on the whole menu."""
import functools
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import nlp_exact as X                                                  # noqa: E402
from nlp_general_ref import NlpGeneralRef                              # noqa: E402
from sqpsolver_jl_amd.nlp_terms import ATAN, COS, POW, POWR, SIGMOID, SIN, TANH, _kappa3   # noqa: E402

CASES = ("plain", "chain", "affine", "data0", "data1", "data2", "product", "benign", "stride")


@functools.lru_cache(maxsize=None)
def _case(name):
    if name.startswith("data"):
        return X.menu_model("data")[int(name[4])]
    return dict(product=X.product_model, benign=lambda: X.product_model(True), stride=X.stride_model).get(name, lambda: X.menu_model(name))()


@functools.lru_cache(maxsize=None)
def _ref(name, dps=X.DPS):
    c = _case(name)
    R = X.NlpExact(c.p, dps)
    return R, R.want(c.x, c.sigma, c.lam, c.lay)


def _failing(name, got):
    """{output: entries that miss 2 B + 2^-1074}"""
    R, (val, bnd) = _ref(name)
    return {k: np.flatnonzero(r > 1.0).tolist() for k, r in X.entry_ratios(got, val, bnd, R.exact).items() if (r > 1.0).any()}


def _mirror(name, **kw):
    c = _case(name)
    return X.mirror_eval(c.p, c.x, c.sigma, c.lam, c.lay, **kw)


# ---- 1. the reference
@pytest.mark.parametrize("name", CASES)
def test_the_reference_agrees_with_itself_at_60_and_400_digits(name):
    a, b = _ref(name)[0].exact, _ref(name, 400)[0].exact
    worst = Fraction(0)
    for key in X.KEYS:
        assert len(a[key]) == len(b[key])
        for va, vb in zip(a[key], b[key]):
            assert (va == 0) == (vb == 0), key
            if vb:
                worst = max(worst, abs(va - vb) / abs(vb))
    print(name, "largest relative difference", float(worst))
    assert worst <= Fraction(1, 10 ** 40)


@pytest.mark.parametrize("name", CASES)
def test_every_case_meets_the_domain_condition(name):
    R = _ref(name)[0]
    lo, hi = R.span
    print(name, "2^%.1f .. 2^%.1f" % (float(X.mp.log(X._mpf(lo), 2)), float(X.mp.log(X._mpf(hi), 2))))
    assert X.DOMAIN[0] <= lo and hi <= X.DOMAIN[1] and R.domain_ok()
    val, bnd = _ref(name)[1]
    for key in X.KEYS:
        assert np.all(np.isfinite(np.atleast_1d(val[key]))) and np.all(np.isfinite(np.atleast_1d(bnd[key]))) and np.all(np.atleast_1d(bnd[key]) >= 0.0)


def test_the_numpy_reference_lies_within_the_bound_at_benign_points():
    c = _case("benign")
    R, (val, bnd) = _ref("benign")
    G = NlpGeneralRef(c.p)
    got = dict(f=G.f(c.x), grad=G.grad(c.x), g=G.g(c.x), jval=G.jac(c.x, c.lay.jrow, c.lay.jcol),
               hval=G.hess(c.x, c.sigma, c.lam, c.lay.hrow, c.lay.hcol))
    X.check_entries(got, val, bnd, R.exact, label="NlpGeneralRef on product_model(benign)")
    assert got["jval"][-1] == 0.0 and got["hval"][-2] == 0.0 and got["hval"][-1] == 0.0


# ---- 2. the cases
def test_the_cases_reach_every_kind_at_every_order_and_every_edge_of_the_plans():
    for variant in ("plain", "chain", "affine", "data0", "data1", "data2"):
        c = _case(variant)
        pl = X.plans(c.p, c.lay)
        reached = {q: set() for q in range(3)}
        for key in ("g", "jval", "hval"):
            for entry in pl[key]:
                for t, a, b, ja, jb, row in entry:
                    reached[(a >= 0) + (b >= 0)].add(int(c.p.fkind[a if a >= 0 else c.p.tptr[t]]))
                    assert a == b or b < 0                              # one factor per term: kappa, kappa', kappa'' alone
        assert all(reached[q] == set(X.ALL_KINDS) for q in range(3)), variant
    pairs = X.menu_pairs()
    assert len(pairs) == 174 and {k for k, _, _ in pairs} == set(X.ALL_KINDS)
    for kind, us in X.MENU.items():
        assert sorted(u for k, _, u in pairs if k == kind) == sorted(us)
    assert {(e, u) for k, e, u in pairs if k == POW} == {(e, u) for e in X.POW_E for u in X.POW_U}
    assert {(e, u) for k, e, u in pairs if k == POWR} == {(e, u) for e in X.POWR_P for u in X.POWR_U}
    # chain: a != 1 and b != 0 wherever u != 0; affine: 2, 3 and 8 arguments; data: every slot at other arguments
    c = _case("chain")
    assert np.all((c.p.fscale != 1.0) & ((c.p.fshift != 0.0) | (c.x[c.p.fvar - 1] == 0.0)))
    assert sorted(set(np.diff(_case("affine").p.aptr).tolist())) == [2, 3, 8]
    d = [_case(f"data{s}") for s in range(3)]
    for a, b in ((0, 1), (0, 2), (1, 2)):
        ua, ub = ([X._fr(s_) * X._fr(v) + X._fr(b_) for s_, v, b_ in zip(q.p.fscale, q.x[q.p.fvar - 1], q.p.fshift)] for q in (d[a], d[b]))
        assert all(va != vb for va, vb in zip(ua, ub)) and np.mean(d[a].p.fshift != d[b].p.fshift) > 0.9     # (-2 * 20 = -1 * 40: a few shifts coincide)
        assert np.all(d[a].p.fscale != d[b].p.fscale) and np.any(d[a].p.fpar != d[b].p.fpar)
        for name in ("trow", "tptr", "fvar", "fkind", "fexp"):
            assert np.array_equal(getattr(d[a].p, name), getattr(d[b].p, name))
    # products
    c = _case("product")
    pl = X.plans(c.p, c.lay)
    assert sorted(set(np.diff(c.p.tptr).tolist())) == [2, 3, 8] and set(X.ALL_KINDS) <= set(c.p.fkind.tolist())
    assert max(len(e) for e in pl["hval"]) == 64 and len(pl["hval"][int(np.flatnonzero((c.lay.hrow == 1) & (c.lay.hcol == 1))[0])]) == 64
    assert pl["jval"][-1] == [] and pl["hval"][-2] == [] and pl["hval"][-1] == [] and pl["hval"][0] != []
    # strides
    c = _case("stride")
    pl = X.plans(c.p, c.lay)
    assert min(len(c.p.fkind), len(c.p.trow), int((c.p.trow == 0).sum()), c.p.n, c.p.m, len(c.lay.jrow), len(c.lay.hrow)) > 1024
    assert c.p.n == 1025 and set(np.diff(c.p.tptr).tolist()) == {1, 2} and set(X.ALL_KINDS) == set(c.p.fkind.tolist())
    val = _ref("stride")[1][0]
    for key in ("grad", "g", "jval", "hval"):
        assert np.all(val[key][1024:] != 0.0) and len(val[key]) > 1024, key


# ---- 3. wrong evaluators miss the bound where they are wrong, and nowhere else
def _old_tanh(kind, e, par, u):
    if kind != TANH:
        return _kappa3(kind, e, par, u)
    t = np.tanh(u)
    return t, 1.0 - t * t, -2.0 * t * (1.0 - t * t)


def _old_sigmoid(kind, e, par, u):
    if kind != SIGMOID:
        return _kappa3(kind, e, par, u)
    e_ = np.exp(-np.abs(u))
    sg, sc = np.where(u < 0, e_ / (1.0 + e_), 1.0 / (1.0 + e_)), np.where(u < 0, 1.0 / (1.0 + e_), e_ / (1.0 + e_))
    return sg, sg * sc, sg * sc * (sc - sg)


def _old_atan(kind, e, par, u):
    if kind != ATAN:
        return _kappa3(kind, e, par, u)
    q = 1.0 / (1.0 + u * u)
    return np.arctan(u), q, -2.0 * u * (q * q)


def _rows(indices, which):
    """the (kind, |u|) of the menu pairs behind the entries `indices` of grad, jval or hval of menu_model("plain")"""
    c = _case("plain")
    lay = c.lay
    var = dict(grad=lambda i: i, jval=lambda i: int(lay.jcol[i]) - 1, hval=lambda i: int(lay.hcol[i]) - 1)[which]
    pairs = X.menu_pairs()
    return {(pairs[var(i)][0], abs(pairs[var(i)][2])) for i in indices}


def test_the_old_tanh_derivatives_miss_the_bound_from_u_5_on():
    bad = _failing("plain", _mirror("plain", kappa3=_old_tanh))
    assert set(bad) == {"grad", "jval", "hval"}
    want = {(TANH, u) for u in (5.0, 10.0, 19.0, 19.0615, 20.0, 40.0, 300.0)}
    assert _rows(bad["grad"], "grad") == want and _rows(bad["jval"], "jval") == want and _rows(bad["hval"], "hval") == want
    assert len(bad["jval"]) == 14                                       # both signs


def test_the_old_sigmoid_second_derivative_misses_the_bound_around_0():
    bad = _failing("plain", _mirror("plain", kappa3=_old_sigmoid))
    assert set(bad) == {"hval"}
    # (not at 2^-30: s and 1 - s are 1/2 +- 2^-32 to 2^-95 there, and their difference is exact)
    assert _rows(bad["hval"], "hval") == {(SIGMOID, u) for u in (1e-6, 1e-3)} and len(bad["hval"]) == 4


def test_the_old_arctangent_second_derivative_misses_the_bound_at_1e100():
    bad = _failing("plain", _mirror("plain", kappa3=_old_atan))
    assert set(bad) == {"hval"} and _rows(bad["hval"], "hval") == {(ATAN, 1e100)} and len(bad["hval"]) == 2


def test_a_chain_factor_a_in_the_place_of_a_squared_misses_every_second_derivative():
    c = _case("chain")
    bad = _failing("chain", _mirror("chain", chain2=lambda a: a))
    val = _ref("chain")[1][0]
    # every non-zero entry but those of SIN and COS at their zeros and at 1e15, where du kappa''' is as large as kappa'' itself
    every = set(np.flatnonzero(val["hval"] != 0.0).tolist())
    assert set(bad) == {"hval"} and set(bad["hval"]) <= every and len(bad["hval"]) >= 160
    pairs = X.menu_pairs()
    assert {pairs[int(c.lay.hcol[i]) - 1] for i in every - set(bad["hval"])} <= {(k, 1, u) for k in (SIN, COS) for u in (float(np.pi / 2), float(np.pi), 1e15)}
    assert not _failing("chain", _mirror("chain"))


def test_a_missing_weight_on_the_second_argument_of_a_hessian_pair_misses_the_bound():
    c = _case("affine")
    bad = _failing("affine", _mirror("affine", drop_second_weight=True))
    val = _ref("affine")[1][0]
    # every entry whose second argument has a weight other than 1.0 and whose value is not 0
    aw = c.p.acoef[[int(np.flatnonzero(c.p.avar == v)[0]) for v in c.lay.hcol]]
    # ... but those of SIN and COS at their zeros and at 1e15 (see above)
    every = set(np.flatnonzero((aw != 1.0) & (val["hval"] != 0.0)).tolist())
    assert set(bad) == {"hval"} and set(bad["hval"]) <= every and len(bad["hval"]) > 2000
    fac = {int(v): k for k in range(len(c.p.fkind)) for v in c.p.avar[c.p.aptr[k]:c.p.aptr[k + 1]]}
    pairs = X.menu_pairs()
    assert {pairs[fac[int(c.lay.hcol[i])] // 2] for i in every - set(bad["hval"])} <= {(k, 1, u) for k in (SIN, COS) for u in (float(np.pi / 2), float(np.pi), 1e15)}
    assert not _failing("affine", _mirror("affine"))


def test_a_summand_dropped_from_the_slot_of_64_misses_the_bound_there():
    c = _case("product")
    bad = _failing("product", _mirror("product", drop_last_of=64))
    assert bad == {"hval": [int(np.flatnonzero((c.lay.hrow == 1) & (c.lay.hcol == 1))[0])]}
    assert not _failing("product", _mirror("product"))


# ---- 4. the mirror of the device formulas
@pytest.mark.parametrize("name", CASES)
def test_the_mirror_of_the_device_formulas_meets_the_bound(name):
    c = _case(name)
    R, (val, bnd) = _ref(name)
    worst, _ = X.check_entries(_mirror(name), val, bnd, R.exact, R.entry_kind, name)
    assert max(worst.values()) <= 2.0
