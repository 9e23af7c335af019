"""A general sparse quadratically constrained quadratic programme for the batched device run (sqphip_qcqp_attach):

    min  f0 + c'x + 1/2 x'Q0 x     s.t.  gL_i <= g0_i + a_i'x + 1/2 x'Q_i x <= gU_i   (i = 1..m),   xL <= x <= xU

Q0 and every Q_i are sparse symmetric, given as 1-based triplets in either triangle, duplicates summed; an entry folds into
the lower triangle with the value convention of the Hessian COO: an off-diagonal v contributes v x_r x_c, a diagonal v
contributes 1/2 v x_r^2.  A is given as triplets (row, column, value).  Rows 1..num_linear carry no quadratic term.

    Qcqp            the data (terms, values, bounds, start)
    qcqp_layout     the structures a Context is created with (1-based Jacobian COO, lower Hessian COO, bounds, start)
    qcqp_synth      a seeded sparse test problem: a few linear rows first, convex and non-convex quadratic rows, a feasible start
    qcqp_scenario   scenario s of a problem: the same structure, other coefficients, the same feasible start

Device evaluator: csrc/qcqp_dev.hpp qcqp_eval."""
from __future__ import annotations

import dataclasses

import numpy as np


@dataclasses.dataclass
class Qcqp:
    n: int
    m: int
    num_linear: int
    q0r: np.ndarray        # Q0 triplets (1-based)
    q0c: np.ndarray
    q0v: np.ndarray
    ar: np.ndarray         # A triplets: row, column (1-based), value
    ac: np.ndarray
    av: np.ndarray
    qi: np.ndarray         # Q_i triplets: row i, then (r, c) (1-based), value
    qr: np.ndarray
    qc: np.ndarray
    qv: np.ndarray
    c: np.ndarray          # [n]
    g0: np.ndarray         # [m]
    f0: float
    xL: np.ndarray
    xU: np.ndarray
    gL: np.ndarray
    gU: np.ndarray
    x0: np.ndarray


@dataclasses.dataclass
class QcqpLayout:
    """What SqpSolver.Model holds for this problem (1-based COO structures, bounds, start)."""
    n: int
    m: int
    num_linear: int
    jrow: np.ndarray
    jcol: np.ndarray
    hrow: np.ndarray
    hcol: np.ndarray
    xL: np.ndarray
    xU: np.ndarray
    gL: np.ndarray
    gU: np.ndarray
    x0: np.ndarray


def _i64(a):
    return np.ascontiguousarray(a, dtype=np.int64)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def make_qcqp(n, m, num_linear, Q0=((), (), ()), A=((), (), ()), Q=((), (), (), ()), c=None, g0=None, f0=0.0,
              xL=None, xU=None, gL=None, gU=None, x0=None) -> Qcqp:
    """A Qcqp from triplet tuples (1-based); missing vectors are zeros, missing bounds infinite."""
    inf = np.inf
    full = lambda v, k, d: _f64(np.full(k, d) if v is None else v)
    return Qcqp(n, m, num_linear, *(_i64(a) for a in Q0[:2]), _f64(Q0[2]), *(_i64(a) for a in A[:2]), _f64(A[2]),
                *(_i64(a) for a in Q[:3]), _f64(Q[3]), full(c, n, 0.0), full(g0, m, 0.0), float(f0),
                full(xL, n, -inf), full(xU, n, inf), full(gL, m, -inf), full(gU, m, inf), full(x0, n, 0.0))


def qcqp_layout(q: Qcqp) -> QcqpLayout:
    """Jacobian COO: the union of A's entries and of (i, r), (i, c) of every Q_i term, row-major; Hessian COO: the union of
    the folded lower entries of Q0 and of every Q_i, column-major.  Each structural entry once."""
    n = q.n
    jr = np.concatenate([q.ar, q.qi, q.qi]).astype(np.int64)
    jc = np.concatenate([q.ac, q.qr, q.qc]).astype(np.int64)
    jkey = np.unique((jr - 1) * n + (jc - 1))
    hr = np.concatenate([np.maximum(q.q0r, q.q0c), np.maximum(q.qr, q.qc)]).astype(np.int64)
    hc = np.concatenate([np.minimum(q.q0r, q.q0c), np.minimum(q.qr, q.qc)]).astype(np.int64)
    hkey = np.unique((hc - 1) * n + (hr - 1))
    return QcqpLayout(n, q.m, q.num_linear, jkey // n + 1, jkey % n + 1, hkey % n + 1, hkey // n + 1,
                      q.xL.copy(), q.xU.copy(), q.gL.copy(), q.gU.copy(), q.x0.copy())


def qcqp_rows(q: Qcqp, x) -> np.ndarray:
    """g(x) (the same sums as the device, in numpy; used to place the bounds of generated problems)."""
    x = _f64(x)
    g = q.g0.copy()
    np.add.at(g, q.ar - 1, q.av * x[q.ac - 1])
    w = np.where(q.qr == q.qc, 0.5, 1.0)
    np.add.at(g, q.qi - 1, w * q.qv * x[q.qr - 1] * x[q.qc - 1])
    return g


def qcqp_synth(n: int = 40, m: int = 24, seed: int = 1, num_linear: int | None = None, terms_per_row: int = 3) -> Qcqp:
    """Seeded sparse QCQP: a convex objective (diagonal-dominant Q0 with a few couplings), num_linear linear rows (equalities
    and ranges), then quadratic rows cycling through a convex ball-type upper bound, a non-convex bilinear range and a
    quadratic equality.  Bounds are placed around a start x0 that satisfies every row and bound."""
    rng = np.random.default_rng(seed)
    nlin = max(1, m // 6) if num_linear is None else num_linear
    x0 = rng.uniform(-0.5, 0.5, n)
    # objective
    q0r, q0c, q0v = list(range(1, n + 1)), list(range(1, n + 1)), list(rng.uniform(1.0, 2.0, n))
    for _ in range(n // 2):
        r, c_ = rng.choice(n, 2, replace=False) + 1
        q0r.append(int(r)); q0c.append(int(c_)); q0v.append(float(rng.uniform(-0.3, 0.3)))
    c = rng.standard_normal(n)
    ar, ac, av, qi, qr, qc, qv = [], [], [], [], [], [], []
    kinds = []
    for i in range(1, m + 1):
        cols = rng.choice(n, terms_per_row, replace=False) + 1
        for j in cols:
            ar.append(i); ac.append(int(j)); av.append(float(rng.standard_normal()))
        if i <= nlin:
            kinds.append("eq" if i % 2 else "range")
            continue
        kind = ("ball", "bilinear", "qeq")[(i - nlin - 1) % 3]
        kinds.append(kind)
        vs = rng.choice(n, 2, replace=False) + 1
        if kind == "ball":                       # convex: positive diagonal, <= bound
            for j in vs:
                qi.append(i); qr.append(int(j)); qc.append(int(j)); qv.append(float(rng.uniform(0.5, 2.0)))
        elif kind == "bilinear":                 # indefinite: x_r x_c (either triangle) and a negative square
            qi.append(i); qr.append(int(vs[0])); qc.append(int(vs[1])); qv.append(float(rng.uniform(0.5, 1.5)))
            qi.append(i); qr.append(int(vs[1])); qc.append(int(vs[1])); qv.append(float(-rng.uniform(0.2, 1.0)))
        else:                                    # quadratic equality with a duplicated term (summed)
            qi.append(i); qr.append(int(vs[1])); qc.append(int(vs[0])); qv.append(float(rng.uniform(0.2, 0.8)))
            qi.append(i); qr.append(int(vs[0])); qc.append(int(vs[1])); qv.append(float(rng.uniform(0.2, 0.8)))
            qi.append(i); qr.append(int(vs[0])); qc.append(int(vs[0])); qv.append(float(rng.uniform(0.5, 1.0)))
    q = make_qcqp(n, m, nlin, (q0r, q0c, q0v), (ar, ac, av), (qi, qr, qc, qv), c=c, g0=np.zeros(m), f0=float(rng.standard_normal()),
                  xL=np.full(n, -2.0), xU=np.full(n, 2.0), x0=x0)
    q.g0 = rng.uniform(-0.2, 0.2, m)
    g = qcqp_rows(q, x0)
    q.gL, q.gU = np.empty(m), np.empty(m)
    for i, kind in enumerate(kinds):
        s = rng.uniform(0.2, 1.0)
        if kind in ("eq", "qeq"):
            q.gL[i] = q.gU[i] = g[i]
        elif kind == "ball":
            q.gL[i], q.gU[i] = -np.inf, g[i] + s
        else:
            q.gL[i], q.gU[i] = g[i] - s, g[i] + s
    return q


def qcqp_scenario(q: Qcqp, s: int, seed: int = 1) -> Qcqp:
    """Scenario s of q (s = 0: q itself): every coefficient scaled by 1 + 5 % noise, one in fifty of the A and Q values set
    to zero, g0 moved so that every row keeps its value at x0 -- the bounds (and the feasibility of x0) stay."""
    if s == 0:
        return q
    rng = np.random.default_rng(seed * 1000 + s)
    sc = lambda v: v * (1.0 + 0.05 * rng.standard_normal(len(v)))
    drop = lambda v: np.where(rng.random(len(v)) < 0.02, 0.0, v)
    out = dataclasses.replace(q, c=sc(q.c), q0v=sc(q.q0v), av=drop(sc(q.av)), qv=drop(sc(q.qv)), f0=q.f0 + 0.1 * s)
    out.g0 = q.g0 + (qcqp_rows(q, q.x0) - qcqp_rows(dataclasses.replace(out, g0=q.g0), q.x0))
    return out
