"""The merit cases of tests/merit_cases.py and the exact reference of tests/merit_ref.py, checked without a GPU:

1. the reference agrees, at every case and both operand sets, with two independent float64 implementations -- the
   oracle's restatements (oracle/common.c) and a numpy evaluation of the q-model -- within the tolerance rule the GPU test
   (tests/test_gpu_merit_cases.py) holds the kernels to, so that rule is checked on the CPU first;
2. the case table has the edges it was made for;
3. every case has every bound kind and every operand position;
4. the Armijo inputs of the GPU test reach all four exits of the backtracking loop, each comparison by a margin that
   rounding in the device evaluator cannot flip.
Conditions on the inputs, not measurements: a later change to a generator that breaks one fails here."""
import dataclasses
import math

import numpy as np
import pytest
import scipy.sparse as sp

import merit_cases as MC
import merit_ref as MR
from oracle import oracle as O

PNORMS = (1, 2, math.inf)
PCODE = {1: 1, 2: 2, math.inf: 0}


def _oracle_values(c, o):
    """Every merit quantity of case c, operand set o, by the oracle (sequential float64 sums) and numpy"""
    P, B = c.P, c.B; n, m = P.n, P.m
    L = O.lib(); gL, gU = O.f64(B.gL), O.f64(B.gU)
    out = {}
    for pn in PNORMS:
        out["viol", pn] = O.norm_violations(o.E, B.gL, B.gU, o.x, B.xL, B.xU, pn)
        out["compl", pn] = L.ora_norm_complementarity(m, O._d(o.E), O._d(gL), O._d(gU), O._d(o.lam), PCODE[pn])
    jcp, jrv, jslot, _ = O.coo_to_csc(n, P.jrow, P.jcol)
    jv = np.zeros(len(jrv)); np.add.at(jv, jslot, o.Jval)
    out["kt"] = O.kt_residuals(o.df, o.lam, o.mult_x_U, o.mult_x_L, jcp, jrv, jv, m)
    v1 = out["viol", 1]
    out["phi", 0], out["phi", 1] = o.f + o.mu * v1, v1
    J = sp.coo_matrix((o.Jval, (P.jrow - 1, P.jcol - 1)), shape=(m, n)).tocsr()
    Hl = sp.coo_matrix((o.Hval, (P.hrow - 1, P.hcol - 1)), shape=(n, n)).tocsr()
    H = Hl + sp.tril(Hl, -1).T
    step = O.norm_violations(o.E + J @ o.p, B.gL, B.gU, o.x + o.p, B.xL, B.xU, 1)
    out["q", "step"] = o.df @ o.p + 0.5 * o.p @ (H @ o.p) + o.mu * step
    out["q", "nohess"] = o.df @ o.p + o.mu * step
    out["q", "nostep"] = o.mu * v1
    out["D5"] = o.df @ o.p - o.mu * np.maximum(0, np.maximum(o.E - B.gU, B.gL - o.E)).sum()      # compute_derivative of test_gpu_parity.py
    for vec in (None, o.mu_vec):
        for fr in (0, 1):
            out["D", vec is not None, fr] = L.ora_compute_derivative_full(
                n, m, O._d(o.df), O._d(o.p), O._d(o.E), O._d(gL), O._d(gU), o.mu, O._d(vec) if vec is not None else None, fr,
                O._d(o.slack), 2 * m)
    for rule in (1, 2, 3):
        for it in (1, 4):
            want = o.mu_vec.copy()
            L.ora_compute_mu_rule(rule, it, o.rho, v1, float(o.df @ o.p), float(0.5 * o.p @ (H @ o.p)), m, O._d(o.lam), O._d(want))
            out["mu", rule, it] = want
    return out


# ------------------------------------------------------------------ 1. the reference against the oracle
@pytest.mark.parametrize("oset", [0, 1])
@pytest.mark.parametrize("name", MC.ALL_NAMES)
def test_reference_agrees_with_the_oracle_within_the_tolerance_rule(name, oset):
    c = MC.case(name); o = c.ops[oset]
    ref, got = MR.reference_values(c.P, c.B, o), _oracle_values(c, o)
    MR.check_against(ref, got, f"{name} set {oset}")
    # the rule is no blanket: it is of the order of the rounding of the sums it bounds
    for key, r in ref.items():
        if key[0] != "mu" and not r.exact and r.value != 0.0:
            assert r.tol <= 1e-9 * max(abs(r.value), r.mag), (name, key, r)
    assert ref["viol", math.inf].exact and ref["viol", math.inf].value == got["viol", math.inf]


def test_a_missing_term_is_outside_the_tolerance():
    """What the GPU test must notice: the last trip of a strided loop dropped (entries from index 1024 on), at both operand sets"""
    on = lambda lo, hi: np.where(np.isfinite(hi), hi, lo)
    for name in ("1025x1023", "1023x1025"):
        c = MC.case(name); B = c.B
        for o in c.ops:
            ref = MR.reference_values(c.P, c.B, o)
            E, x = o.E.copy(), o.x.copy()
            E[MC.TPB:], x[MC.TPB:] = on(B.gL, B.gU)[MC.TPB:], on(B.xL, B.xU)[MC.TPB:]          # no violation beyond the first trip
            got = _oracle_values(c, dataclasses.replace(o, E=E, x=x))
            for key in (("viol", 1), ("viol", 2), ("viol", math.inf), ("phi", 0), ("q", "nostep")):
                assert abs(got[key] - ref[key].value) > 100 * max(ref[key].tol, 1e-300), (name, key)


# ------------------------------------------------------------------ 2. the case table has its edges
def test_case_table_has_its_edges():
    cs = {nm: MC.case(nm) for nm in MC.ALL_NAMES}
    assert (MC.WAVE, MC.TPB, MC.STAGE_PASS) == (64, 1024, 16384)
    for dim in ("n", "m"):
        rem = {getattr(c.P, dim) % MC.TPB for c in cs.values() if getattr(c.P, dim) > MC.TPB}
        assert 1 in rem and 1023 in {getattr(c.P, dim) % MC.TPB for c in cs.values()}, dim
        assert {63, 64, 65} <= {getattr(c.P, dim) for c in cs.values()}, dim
        assert any(getattr(c.P, dim) > 2 * MC.TPB for c in cs.values()), dim
    assert [(c.P.n, c.P.m) for c in cs.values()][:len(MC.SIZES)] == MC.SIZES
    assert any(c.P.m == 0 and len(c.P.jrow) == 0 for c in cs.values())
    for nm in ("65x63-dups", "1025x1023-dups"):
        P, plain = cs[nm].P, cs[nm.replace("-dups", "")].P
        for r, c_, r0, every in ((P.jrow, P.jcol, plain.jrow, 5), (P.hrow, P.hcol, plain.hrow, 7)):
            keys, cnt = np.unique(r * (P.n + 1) + c_, return_counts=True)
            assert len(keys) == len(r0) and set(cnt) == {1, 2} and (cnt == 2).sum() == len(r0[::every])
    P = cs["holes"].P
    assert len(P.empty_rows) and len(P.empty_cols)
    assert not np.isin(P.empty_rows + 1, P.jrow).any()
    assert not (np.isin(P.empty_cols + 1, P.jcol).any() or np.isin(P.empty_cols + 1, P.hrow).any() or np.isin(P.empty_cols + 1, P.hcol).any())
    assert all(len(np.unique(c.P.jrow)) == c.P.m for nm, c in cs.items() if nm != "holes")
    P = cs["hfull-65"].P
    assert (P.n, P.m) == (65, 33) and len(P.hrow) == 65 * 66 // 2 and MC.hessian_is_dense(P)
    assert not any(MC.hessian_is_dense(c.P) for nm, c in cs.items() if nm != "hfull-65")
    c = cs["long-row"]
    assert c.row_doubles() > MC.STAGE_PASS and all(v % 2 == 1 for v in (c.P.n, c.P.m, len(c.P.jrow), len(c.P.hrow)))
    # k_seat_stage loops per field: its threads take a second trip only where ONE field is longer than a pass
    assert c.longest_field() == len(c.P.hrow) > MC.STAGE_PASS
    assert all(cc.longest_field() <= MC.STAGE_PASS for nm, cc in cs.items() if nm != "long-row")
    assert (c.P.n, c.P.m) == (2049, 2047)
    for c in cs.values():                                       # banded: at most 4 columns per row, near i n / m; lower triangle
        if c.P.m:
            assert np.bincount(c.P.jrow - 1, minlength=c.P.m).max() <= 4 * (2 if "dups" in c.name else 1)
            assert np.abs((c.P.jcol - 1) - (c.P.jrow - 1) * c.P.n // c.P.m).max() <= 4
        assert np.all(c.P.hrow >= c.P.hcol)


# ------------------------------------------------------------------ 3. every case has every pattern
@pytest.mark.parametrize("name", MC.ALL_NAMES)
def test_every_case_has_every_bound_kind_and_operand_position(name):
    """Sizes below four entries carry as many kinds and positions as fit (1x1, 2049x3, 3x2049)."""
    c = MC.case(name); B = c.B

    def kind(lo, hi):
        return np.where(lo == hi, MC.K_EQ, np.where(np.isfinite(lo) & np.isfinite(hi), MC.K_RANGE, np.where(np.isfinite(lo), MC.K_LOWER, MC.K_UPPER)))

    def position(v, lo, hi):
        return np.where(v > hi, MC.P_ABOVE, np.where(v < lo, MC.P_BELOW, np.where((v == lo) | (v == hi), MC.P_ON, MC.P_INSIDE)))
    assert not np.any(np.isneginf(B.gL) & np.isposinf(B.gU)) and np.all(B.gL <= B.gU) and np.all(B.xL <= B.xU)
    for k, lo, hi in ((c.P.m, B.gL, B.gU), (c.P.n, B.xL, B.xU)):
        assert len(set(kind(lo, hi))) == min(k, 4)
    for o in c.ops:
        for k, v, lo, hi in ((c.P.m, o.E, B.gL, B.gU), (c.P.n, o.x, B.xL, B.xU)):
            pos, kd = position(v, lo, hi), kind(lo, hi)
            assert len(set(pos)) >= min(k, 4) - (1 if k < 4 else 0)
            if k >= 16:                                          # every kind meets every position it can hold
                have = set(zip(kd.tolist(), pos.tolist()))
                assert {(a, b) for a in range(4) for b in range(4)} - have == {(MC.K_EQ, MC.P_INSIDE), (MC.K_LOWER, MC.P_ABOVE), (MC.K_UPPER, MC.P_BELOW)}
            if k >= 32:                                          # a range entry exactly on its lower and one exactly on its upper bound
                rng_ = kd == MC.K_RANGE
                assert np.any(rng_ & (v == lo)) and np.any(rng_ & (v == hi))
        assert np.all(o.mult_x_U <= 0) and np.all(o.mult_x_L >= 0) and np.all(o.mu_vec >= 0) and np.all(o.slack >= 0)
        # the largest terms sit at an index >= 1024 wherever the size has one
        viol_r = np.maximum(0, np.maximum(o.E - B.gU, B.gL - o.E)); viol_x = np.maximum(0, np.maximum(o.x - B.xU, B.xL - o.x))
        if c.P.m > MC.TPB:
            assert int(np.argmax(viol_r)) == o.ibig >= MC.TPB and viol_r.max() > viol_x.max()
            J = sp.coo_matrix((o.Jval, (c.P.jrow - 1, c.P.jcol - 1)), shape=(c.P.m, c.P.n)).tocsr()      # (copies summed)
            rown = np.sqrt(np.asarray(J.multiply(J).sum(axis=1)).ravel())
            assert int(np.argmax(np.abs(o.lam) * rown)) == o.ibig
            assert int(np.argmax(np.abs(o.lam))) == o.ibig and B.gL[o.ibig] != B.gU[o.ibig]
        elif c.P.n > MC.TPB:
            assert int(np.argmax(viol_x)) == o.jbig >= MC.TPB and viol_x.max() > viol_r.max(initial=0.0)
        if c.P.n > MC.TPB:
            assert int(np.argmax(np.abs(o.df))) == o.jbig >= MC.TPB
    a, b = c.ops
    assert np.abs(np.log10(np.abs(b.Jval[b.Jval != 0]))).max(initial=6.0) <= 6.0 + 1e-9
    if c.P.n >= 64: assert np.log10(np.abs(b.df)).min() < -4 and np.log10(np.abs(b.df)).max() > 4 and np.abs(a.df).max() <= 30.0


# ------------------------------------------------------------------ 4. the Armijo inputs
def test_armijo_inputs_reach_every_exit_by_a_safe_margin():
    exits = set()
    for name in MC.ARMIJO_NAMES:
        pr = MC.armijo_problem(name)
        assert pr.n > MC.TPB and pr.m > MC.TPB
        for mu, fr, step, phi0, D in pr.steps:
            alpha, valid, nev, margin = MR.compute_alpha(MC.armijo_phi(pr, mu, fr, step), phi0, D, float(np.abs(step).max()),
                                                         MC.TOL_DIRECTION, **pr.kw)
            print(name, (mu, fr), "alpha", alpha, "valid", valid, "evaluations", nev, "smallest margin", margin)
            assert margin >= 1e-9, (name, mu, fr, margin)
            exits.add("at once" if nev == 0 else "invalid" if not valid else "alpha = 1" if nev == 1 else
                      "backtracks >= 3" if nev >= 4 else "backtracks")
    assert {"at once", "invalid", "alpha = 1", "backtracks >= 3"} <= exits, exits
