"""The cases of tests/qcqp_cases.py validated without a GPU: tests/test_gpu_qcqp_cases.py then holds the device to the same
exact reference and the same derived bound.

    presence        every feature the edge model promises, read off the model; the counts of the stride model
    attainable      QcqpRef (numpy, double precision) meets the bound of QcqpExact on every model and slot
    derivatives     QcqpExact's gradient, Jacobian and Hessian against central differences of its own f and g in rationals:
                    the functions are quadratic, so the differences are exact
    mutants         a dropped 1/2, a constant multiplied by x, sigma and lambda swapped: each fails the bound
    disc            the oracle's run against the closed form
    armijo          every probe of every case decides by at least 1e3 bounds
    determinism     every generator twice"""
import dataclasses
from fractions import Fraction

import numpy as np
import pytest

import qcqp_cases as QC
from qcqp_ref import QcqpRef
from sqpsolver_jl_amd.qcqp import qcqp_layout


def _keys(rows, cols, lower=False):
    r, c = np.asarray(rows).tolist(), np.asarray(cols).tolist()
    return [(max(a, b), min(a, b)) if lower else (a, b) for a, b in zip(r, c)]


def _needs(q):
    """(Jacobian entries, lower Hessian entries) the terms of q need, with the terms that feed each"""
    J, H = {}, {}
    for t, (i, j) in enumerate(zip(q.ar.tolist(), q.ac.tolist())):
        J.setdefault((i, j), []).append(("A", t))
    for t, (i, r, c) in enumerate(zip(q.qi.tolist(), q.qr.tolist(), q.qc.tolist())):
        for v in {r, c}:
            J.setdefault((i, v), []).append(("Q", t))
        H.setdefault((max(r, c), min(r, c)), []).append(("Q", i))
    for t, (r, c) in enumerate(zip(q.q0r.tolist(), q.q0c.tolist())):
        H.setdefault((max(r, c), min(r, c)), []).append(("Q0", t))
    return J, H


# ------------------------------------------------------------------------------------------------ presence
@pytest.mark.parametrize("kind", QC.EDGE_KINDS)
def test_edge_structure_holds_what_the_terms_need_and_names_the_rest(kind):
    cs = QC.edge_model(kind)
    q, lay = cs.qs[0], cs.lay
    J, H = _needs(q)
    jk, hk = _keys(lay.jrow, lay.jcol), _keys(lay.hrow, lay.hcol)
    assert all(r >= c for r, c in zip(lay.hrow, lay.hcol))
    assert set(J) <= set(jk) and set(jk) - set(J) == {(7, 10)}
    assert sorted(k for k in set(jk) if jk.count(k) > 1) == [(3, 3), (20, 5)]
    if kind == "noH":
        assert len(hk) == 0
    else:
        assert set(H) <= set(hk) and set(hk) - set(H) == {(12, 10)}
        assert [k for k in set(hk) if hk.count(k) > 1] == [(5, 4)]
    for other in cs.qs[1:]:                                  # one structure, other values
        for k in ("q0r", "q0c", "ar", "ac", "qi", "qr", "qc"):
            assert np.array_equal(getattr(q, k), getattr(other, k))
        assert not np.array_equal(q.qv, other.qv) and not np.array_equal(q.c, other.c) and not np.array_equal(q.g0, other.g0)


def test_edge_model_holds_every_feature():
    cs = QC.edge_model("full")
    q, lay = cs.qs[0], cs.lay
    assert (q.n, q.m, len(cs.qs)) == (12, 49, 2)
    J, H = _needs(q)
    rows_with_terms = set(q.ar.tolist()) | set(q.qi.tolist())
    assert 2 not in rows_with_terms                                               # a row with no term at all
    in_obj = set(q.q0r.tolist()) | set(q.q0c.tolist())
    in_any = in_obj | set(q.ac.tolist()) | set(q.qr.tolist()) | set(q.qc.tolist())
    assert 11 not in in_obj and 11 in in_any and q.c[10] != 0.0                   # a variable in no objective term
    assert 12 not in in_any and q.c[11] != 0.0                                    # a variable in no term whatsoever
    assert sorted(k for k, _ in J[(3, 3)]) == ["A", "Q", "Q"]                     # an A entry and two Q entries in one slot
    assert [k for k, _ in J[(1, 1)]] == ["A", "A"]                                # the same (row, col) twice in A
    trip = list(zip(q.qi.tolist(), q.qr.tolist(), q.qc.tolist()))
    assert (4, 6, 7) in trip and (4, 7, 6) in trip                                # a pair once in each triangle
    assert (3, 3, 3) in trip                                                      # a diagonal Q_i term
    q0 = list(zip(q.q0r.tolist(), q.q0c.tolist()))
    assert any(r < c for r, c in q0) and any(r == c for r, c in q0)               # Q0: upper triangle, diagonal
    jk, hk = _keys(lay.jrow, lay.jcol), _keys(lay.hrow, lay.hcol)
    assert jk.count((3, 3)) == 2 and (7, 10) in jk and (7, 10) not in J           # J: a duplicated and an unneeded slot
    assert hk.count((5, 4)) == 2 and (12, 10) in hk and (12, 10) not in H         # H: the same
    feeders = H[(5, 4)]
    assert ("Q0", q0.index((5, 4))) in feeders and len({i for k, i in feeders if k == "Q"}) >= 40
    assert q.ar.tolist().count(QC.EDGE_LONG) + q.qi.tolist().count(QC.EDGE_LONG) >= 300   # a long plan row
    for inst in cs.qs:
        assert (inst.q0v == 0.0).any() and (inst.av == 0.0).any() and (inst.qv == 0.0).any()
    assert QC.nvalues(q) == 483 and QC.nvalues(q) % 2 == 1                        # the block is padded


def test_edge_variants_drop_a_term_kind_and_keep_the_rest():
    full = QC.edge_model("full").qs[0]
    noq0, noa, noh = (QC.edge_model(k) for k in ("noQ0", "noA", "noH"))
    assert len(noq0.qs[0].q0v) == 0 and len(noq0.qs[0].av) == len(full.av) and QC.nvalues(noq0.qs[0]) % 2 == 0
    assert len(noa.qs[0].av) == 0 and len(noa.qs[0].q0v) == len(full.q0v) and QC.nvalues(noa.qs[0]) % 2 == 0
    assert noa.qs[0].qi.tolist().count(QC.EDGE_LONG) >= 300
    assert not {1, 2, 7} & set(noa.qs[0].qi.tolist())                             # without A three rows are empty
    assert len(noh.lay.hrow) == 0 and noh.point.lam is None and len(noh.qs[0].q0v) == len(full.q0v)
    assert len(noq0.lay.hrow) < len(QC.edge_model("full").lay.hrow) and len(noa.lay.jrow) < len(noh.lay.jrow)


def test_stride_model_makes_a_third_partial_trip_of_every_loop():
    cs = QC.stride_model()
    q, lay = cs.qs[0], cs.lay
    counts = dict(n=q.n, nnzQ0=len(q.q0v), m=q.m, nnzJ=len(lay.jrow), nnzH=len(lay.hrow))
    print(counts, "values per instance", QC.nvalues(q))
    for k, v in counts.items():
        assert v > 2048 and v % 64 != 0, (k, v)
    assert len(cs.qs) == 2 and cs.slots == (1,)
    assert not np.array_equal(cs.qs[0].qv, cs.qs[1].qv) and not np.array_equal(cs.qs[0].c, cs.qs[1].c)
    ex = QC.exact("stride", 1)                                # the entries past index 1024 of every output are not zeros
    for k in ("grad", "g", "jval", "hval"):
        v = ex[k].floats()
        assert np.count_nonzero(v[1024:]) > 0.9 * (len(v) - 1024) and np.count_nonzero(v[2048:]) > 0.9 * (len(v) - 2048), k


# ------------------------------------------------------------------------------------------------ attainable
@pytest.mark.parametrize("name", QC.CASE_NAMES)
def test_numpy_reference_meets_the_derived_bound(name):
    cs = QC.case(name)
    p = cs.point
    for slot in cs.slots:
        msgs, ratio = QC.check_all(QC.ref_eval(QcqpRef(cs.qs[slot]), p.x, p.sigma, p.lam, cs.lay), QC.exact(name, slot), cs.lay)
        print(name, "slot", slot, "largest |got - exact| / bound:", {k: round(v, 4) for k, v in ratio.items()})
        assert not msgs, f"{name} slot {slot}: {len(msgs)} entries, " + "; ".join(msgs[:8])
    if name == "stride":                                      # the probe tells the instances apart
        msgs, _ = QC.check_all(QC.ref_eval(QcqpRef(cs.qs[1]), p.x, p.sigma, p.lam, cs.lay), QC.exact(name, 0), cs.lay)
        assert len(msgs) > 1000


def test_entries_without_a_product_are_exact_constants():
    cs = QC.case("edge-full")
    for slot in cs.slots:
        q, ex = cs.qs[slot], QC.exact("edge-full", slot)
        assert ex["g"].L[1] == 0 and ex["g"].val[1] == Fraction(q.g0[1])
        assert ex["grad"].L[10] == 0 and ex["grad"].val[10] == Fraction(q.c[10]) and ex["grad"].L[11] == 0
        assert ex["grad"].val[9] == 0 and ex["grad"].L[9] == 0
        jk, hk = _keys(cs.lay.jrow, cs.lay.jcol), _keys(cs.lay.hrow, cs.lay.hcol)
        for keys, e, dup, unused in ((jk, ex["jval"], (3, 3), (7, 10)), (hk, ex["hval"], (5, 4), (12, 10))):
            first, later = [k for k, key in enumerate(keys) if key == dup]
            assert e.L[first] > 0 and e.val[first] != 0 and e.L[later] == 0 and e.val[later] == 0
            assert e.L[keys.index(unused)] == 0 and e.val[keys.index(unused)] == 0
        assert ex["hval"].L[hk.index((5, 4))] >= 41 and max(ex["g"].L) >= 300
        assert ex["f"].L[0] == q.n + len(q.q0v)


# ------------------------------------------------------------------------------------------------ derivatives
def test_exact_derivatives_are_exact_differences_of_the_exact_functions():
    cs = QC.case("edge-full")
    q, p, lay = cs.qs[1], cs.point, cs.lay
    E, ex = QC.QcqpExact(q), QC.exact("edge-full", 1)
    x = [Fraction(float(v)) for v in p.x]
    h = Fraction(1, 8)
    at = lambda d: [a + b for a, b in zip(x, d)]             # a rational point
    unit = lambda j, s=1: [s * h if k == j else Fraction(0) for k in range(q.n)]
    jk = _keys(lay.jrow, lay.jcol)
    Jd = {}
    for k, key in enumerate(jk):
        Jd[key] = Jd.get(key, 0) + ex["jval"].val[k]
    for j in range(q.n):
        fp, fm, gp, gm = E.f(at(unit(j))), E.f(at(unit(j, -1))), E.g(at(unit(j))), E.g(at(unit(j, -1)))
        assert (fp.val[0] - fm.val[0]) / (2 * h) == ex["grad"].val[j], j
        for i in range(q.m):
            assert (gp.val[i] - gm.val[i]) / (2 * h) == Jd.get((i + 1, j + 1), 0), (i, j)
    # the Hessian of the Lagrangian: second differences of L(x) = sigma f + lam'g
    sigma, lam = Fraction(float(p.sigma)), [Fraction(float(v)) for v in p.lam]
    lag = lambda d: (lambda f, g: sigma * f.val[0] + sum(a * b for a, b in zip(lam, g.val)))(*E.fg(at(d)))
    Hd = {}
    for k, key in enumerate(_keys(lay.hrow, lay.hcol, lower=True)):
        Hd[key] = Hd.get(key, 0) + ex["hval"].val[k]
    l0 = lag([Fraction(0)] * q.n)
    for r in range(q.n):
        for c in range(r + 1):
            d = lambda sr, sc: [a + b for a, b in zip(unit(r, sr), unit(c, sc))]
            second = (lag(d(1, 1)) - lag(d(1, 0)) - lag(d(0, 1)) + l0) / (h * h) if r != c else \
                (lag(unit(r)) - 2 * l0 + lag(unit(r, -1))) / (h * h)
            assert second == Hd.get((r + 1, c + 1), 0), (r, c)


# ------------------------------------------------------------------------------------------------ mutants
class _NoHalf(QcqpRef):
    def __init__(self, q):
        super().__init__(q)
        self.off = np.ones(len(q.q0r), bool)                  # f: no 1/2 on a diagonal Q0 term

    def grad(self, x):
        return QcqpRef(self.q).grad(x)

    def g(self, x):
        q = self.q
        out = q.g0.copy()
        np.add.at(out, q.ar - 1, q.av * x[q.ac - 1])
        np.add.at(out, q.qi - 1, q.qv * x[q.qr - 1] * x[q.qc - 1])
        return out


class _ConstantTimesX(QcqpRef):
    def jac(self, x, jrow, jcol):                             # the constant A entry multiplied like a Q entry
        return QcqpRef(dataclasses.replace(self.q, av=self.q.av * x[self.q.ac - 1])).jac(x, jrow, jcol)


class _SigmaLamSwapped(QcqpRef):
    def hess(self, sigma, lam, hrow, hcol):
        q = self.q
        lam2 = np.full(q.m, sigma)
        as_q0 = QcqpRef(q).hess(0.0, lam2, hrow, hcol)        # every Q_i term times sigma
        q0_by_lam = super().hess(float(lam[0]), np.zeros(q.m), hrow, hcol)     # every Q0 term times a lambda
        return as_q0 + q0_by_lam


@pytest.mark.parametrize("mutant,outputs", [(_NoHalf, {"f", "g"}), (_ConstantTimesX, {"jval", "jsum"}), (_SigmaLamSwapped, {"hval", "hsum"})])
def test_a_wrong_evaluator_fails_the_bound(mutant, outputs):
    for name in ("edge-full", "stride"):
        cs = QC.case(name)
        p, slot = cs.point, cs.slots[-1]
        msgs, _ = QC.check_all(QC.ref_eval(mutant(cs.qs[slot]), p.x, p.sigma, p.lam, cs.lay), QC.exact(name, slot), cs.lay)
        assert {m.split("[")[0] for m in msgs} == outputs, (name, msgs[:4])


# ------------------------------------------------------------------------------------------------ the disc
@pytest.mark.parametrize("s", [0, 1, 2])
def test_oracle_solves_the_disc_to_its_closed_form(s):
    q = QC.disc_model(s=s)
    assert (q.n, q.m, QC.nvalues(q)) == (2060, 1030, 5151)
    x, obj, mult = QC.disc_optimum(q)
    assert np.abs(QcqpRef(q).g(x) - q.gU).max() <= 1e-14 * q.gU.max() and abs(QcqpRef(q).f(x) - obj) <= 1e-12 * abs(obj)
    assert np.abs(QcqpRef(q).grad(x) + QcqpRef(q).dense_jac(x).T @ mult).max() <= 1e-14       # stationarity, this sign
    ro = QC.disc_oracle(s)
    print("scenario", s, "status", ro["status"], "iter", ro["iter"], "|x - closed form|", np.abs(ro["x"] - x).max(),
          "|mult_g - closed form|", np.abs(ro["mult_g"] - mult).max())
    assert ro["status"] == 0
    assert np.abs(ro["x"] - x).max() <= 1e-6 and abs(ro["obj_val"] - obj) <= 1e-6 and np.abs(ro["mult_g"] - mult).max() <= 1e-6


def test_disc_scenarios_share_the_structure_and_differ_in_c_and_r():
    qs = [QC.disc_model(s=s) for s in range(3)]
    for q in qs[1:]:
        for k in ("qi", "qr", "qc", "qv"):
            assert np.array_equal(getattr(q, k), getattr(qs[0], k))
        assert not np.array_equal(q.c, qs[0].c) and not np.array_equal(q.gU, qs[0].gU)


# ------------------------------------------------------------------------------------------------ the Armijo probe
def test_armijo_cases_decide_every_probe_by_a_safe_margin():
    q, x = QC.stride_model().qs[QC.ARMIJO_SLOT], QC.armijo_point()
    seen, smallest = {}, np.inf
    for a in QC.armijo_cases():
        (alpha, valid, nev), margin, phi0, D = QC.armijo_expected(a.name)
        print(f"armijo {a.name}: mu {a.mu} fr {a.fr} -> alpha {alpha:.6g} valid {valid} n_eval {nev}; smallest margin {margin:.3g} bounds")
        assert margin >= QC.MARGIN, a.name
        smallest = min(smallest, margin)
        seen[a.name] = (alpha, valid, nev)
    print(f"smallest Armijo margin: {smallest:.3g} bounds")
    assert seen["descent"] == (1.0, True, 1) and seen["zero"] == (1.0, True, 0)
    for name in ("backtracked", "penalty", "restoration", "outside"):             # backtracked and valid
        assert seen[name][1] and seen[name][2] > 1 and seen[name][0] < 1.0, name
    assert not seen["exhausted"][1] and seen["exhausted"][2] > 1 and seen["exhausted"][0] < 0.05
    # the step of "outside" leaves the box past index 1024 at alpha = 1, and the outcome depends on those bounds
    a = {c.name: c for c in QC.armijo_cases()}["outside"]
    xt = x + a.step
    out = np.flatnonzero((xt > q.xU) | (xt < q.xL))
    assert len(out) == 40 and out.min() > 1024 and (xt[out] > q.xU[out]).any() and (xt[out] < q.xL[out]).any()
    assert QC.armijo_reference(q, x, a, box=False)[0] != seen["outside"]


# ------------------------------------------------------------------------------------------------ determinism
def test_generators_are_deterministic():
    same = lambda a, b: all(np.array_equal(getattr(a, f), getattr(b, f)) for f in
                            ("q0r", "q0c", "q0v", "ar", "ac", "av", "qi", "qr", "qc", "qv", "c", "g0", "xL", "xU", "gL", "gU", "x0")) \
        and a.f0 == b.f0
    for kind in QC.EDGE_KINDS:
        a, b = QC.edge_model(kind), QC.edge_model(kind)
        assert all(same(u, v) for u, v in zip(a.qs, b.qs)) and np.array_equal(a.point.x, b.point.x)
        assert np.array_equal(a.lay.jrow, b.lay.jrow) and np.array_equal(a.lay.hcol, b.lay.hcol)
    a, b = QC._stride_case(), QC._stride_case()
    assert all(same(u, v) for u, v in zip(a.qs, b.qs)) and np.array_equal(a.point.lam, b.point.lam)
    assert np.array_equal(a.lay.jrow, qcqp_layout(b.qs[1]).jrow)
    for s in range(3):
        assert same(QC.disc_model(s=s), QC.disc_model(s=s))
    for u, v in zip(QC._armijo_cases(), QC._armijo_cases()):
        assert u.name == v.name and np.array_equal(u.step, v.step)
