"""Seeded sparse structures and Newton-matrix values for the multifrontal tests (numpy only).

A structure is what sqphip_create takes: (n, m, jrow, jcol, hrow, hcol, gL, gU), 1-based COO.  It is built from dense Hessian
cliques (a clique of k variables is one front of k rows), separators shared by several cliques, equality rows (kept in the
factorised matrix), short inequality rows (eliminated in the condensed form) and inequality rows of more than 32 entries
(kept in both forms).  Every family names the plan shape it is built to produce; tests/test_mf_structures_cpu.py checks
each claim through sqphip_mf_plan_info.

Values: the inputs of the Newton matrix per instance (Jv, Hv, Dd, sigp, hd, rtype, hsc; the tests add dw and rhs) in three sets -- "well"
(well scaled, positive definite H block), "indef" (indefinite H: fewer positive pivots than variables) and "ipm" (the
scales at the end of an interior-point run: inequality Dd over 1e-9 .. 1e9, equality Dd = 0)."""
from __future__ import annotations

import dataclasses

import numpy as np


@dataclasses.dataclass
class Structure:
    name: str
    n: int
    m: int
    jrow: np.ndarray
    jcol: np.ndarray
    hrow: np.ndarray
    hcol: np.ndarray
    gL: np.ndarray
    gU: np.ndarray
    target: dict              # what the plan must show (checked by the CPU test)
    kkt_mode: int = 2         # sqphip_create option the device tests use (fronts above 512 rows need 2)

    @property
    def eq(self):
        return self.gL == self.gU

    def kept(self, cond):
        cnt = np.bincount(self.jrow - 1, minlength=self.m)
        return (self.eq | (cnt > 32)) if cond else np.ones(self.m, bool)

    def nu(self, cond):
        return self.n + int(self.kept(cond).sum())


class _Builder:
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.n = 0
        self.h = []               # (row, col) 0-based, row >= col
        self.rows = []            # (vars, kind) kind in {"eq", "ineq"}

    def vars(self, k):
        v = np.arange(self.n, self.n + k)
        self.n += k
        self.h += [(int(i), int(i)) for i in v]
        return v

    def clique(self, k):
        v = self.vars(k)
        self.h += [(int(v[i]), int(v[j])) for i in range(k) for j in range(i)]
        return v

    def couple(self, a, b):
        self.h += [(int(max(i, j)), int(min(i, j))) for i in a for j in b if i != j]

    def row(self, v, kind):
        self.rows.append((np.asarray(v), kind))

    def tail(self):
        """a small second component (a chain of six variables and an equality row): the Hessian is never full"""
        v = self.vars(6)
        self.h += [(int(v[i + 1]), int(v[i])) for i in range(5)]
        self.row(v[:3], "eq")
        self.row(v[3:], "ineq")

    def done(self, name, target, kkt_mode=2):
        h = sorted(set(self.h))
        hr = np.array([a for a, _ in h], dtype=np.int64) + 1
        hc = np.array([b for _, b in h], dtype=np.int64) + 1
        jr, jc = [], []
        for i, (v, _) in enumerate(self.rows):
            jr += [i + 1] * len(v); jc += [int(x) + 1 for x in v]
        m = len(self.rows)
        gL = np.array([0.0 if k == "eq" else -1.0 for _, k in self.rows])
        gU = np.array([0.0 if k == "eq" else 1.0 for _, k in self.rows])
        return Structure(name, self.n, m, np.array(jr, dtype=np.int64), np.array(jc, dtype=np.int64), hr, hc, gL, gU,
                         target, kkt_mode)


def single_front(rows, seed=0):
    """One front of exactly `rows` rows (condensed form): a Hessian clique, equality rows on it, from 40 rows on an
    inequality row of 33 entries (kept), short inequality rows (eliminated: they add nothing to the front's rows)."""
    b = _Builder(seed)
    e = min(3, rows // 8)
    long_row = rows >= 40
    k = rows - e - int(long_row)
    v = b.clique(k)
    for q in range(e):
        b.row(b.rng.choice(v, size=min(3, k), replace=False), "eq")
    if long_row:
        b.row(b.rng.choice(v, size=33, replace=False), "ineq")
    for q in range(2):
        b.row(b.rng.choice(v, size=min(2, k), replace=False), "ineq")
    b.tail()
    T = (rows + 1 + 15) // 16
    return b.done(f"front{rows}", {"max_rows": rows, "max_tiles": T}, kkt_mode=2)


def single_front_family():
    """rows + 1 = 16 T - 1, 16 T, 16 T + 1 for T = 1 .. 14, and 300, 511, about 1000 rows"""
    out = []
    for T in range(1, 15):
        for r1 in (16 * T - 1, 16 * T, 16 * T + 1):
            if r1 - 1 >= 4:
                out.append(single_front(r1 - 1, seed=T))
    for rows in (300, 511, 1000):
        out.append(single_front(rows, seed=rows))
    return out


def siblings(sizes, sep, touch, seed=0, name=None, target=None):
    """Cliques of the given sizes, each coupled to `touch` variables of a separator clique of `sep` variables (the parent of
    all of them): one level of sibling fronts of (size + touch) rows under the separator's front."""
    b = _Builder(seed)
    s = b.clique(sep)
    for i, k in enumerate(sizes):
        v = b.clique(k)
        t = s[(np.arange(touch) + touch * i) % sep]
        b.couple(v, t)
        b.row(np.concatenate([v[:2], t[:1]]), "eq")
    b.row(s[:3], "eq")
    b.tail()
    return b.done(name or f"sib{len(sizes)}", target or {})


def level_families():
    """narrow levels (eight fronts or fewer: one launch of the tallest front's kernel) and wide ones (per class, or merged
    at small batches), whose fronts differ in T within the level"""
    return [
        siblings([10, 25, 40, 70, 100], 48, 4, seed=1, name="narrow_mixed_T",
                 target={"mixed_launch": True, "narrow": True}),
        siblings([130, 150, 190], 48, 4, seed=2, name="narrow_class8",
                 target={"mixed_launch": True, "min_tiles": 9}),
        siblings([8, 12, 20, 30, 40, 12, 24, 36, 44, 16], 56, 4, seed=3, name="wide_small_T",
                 target={"wide": "merged", "mixed_launch": True}),
        siblings([12, 45, 60, 75, 90, 110, 120, 30, 100, 66, 20], 64, 4, seed=4, name="wide_classes",
                 target={"wide": "classes", "mixed_launch": True}),
    ]


def nc_mod4_family():
    """fronts whose column count is 1 / 2 / 3 modulo 4 (a partial last four-column block), with contribution rows (siblings
    under a separator) and without (a root front); and fronts of ONE column: a variable that no row and no Hessian entry
    couples to anything else (a QCQP variable that appears in no constraint) is a root front of one column and no rows.  A
    one-column front WITH contribution rows is not among them: a one-column child adds at most one column of explicit zeros
    to its parent, so the amalgamation of symbolic.hip (merged front within 32 rows, or explicit zeros within 25 %) absorbs
    it unless the parent already carries nearly the allowed zeros; none of these structures gives one."""
    out = []
    for r in (1, 2, 3):
        out.append(siblings([20 + r, 36 + r, 52 + r], 40, 4, seed=10 + r, name=f"nc_mod4_{r}_rows", target={"nc_mod4": r}))
        out.append(single_front(44 + r, seed=20 + r))
    for S_ in out[1::2]:
        S_.target["nc_mod4"] = S_.target["max_rows"] % 4
    for k, nsingle in ((20, 1), (40, 3)):
        b = _Builder(40 + k)
        v = b.clique(k)
        b.row(v[:3], "eq")
        for q in range(nsingle):
            w = b.vars(1)
            if q == 2:
                b.row(w, "ineq")              # (an inequality row of one entry: eliminated, the front stays 1 x 0)
        b.tail()
        out.append(b.done(f"single_var_{nsingle}", {"nc1": nsingle}))
    return out


def top_family():
    """the root front has 84 / 85 columns: k_mf_solve_top2 (the streamed top-of-tree solve, which also tests the inertia)
    takes fronts of up to 84 columns, k_mf_solve_top and k_inertia the rest.  The largest clique ends up at the root."""
    return [siblings([big, 30, 40, 20], 60, 4, seed=5, name=f"top_{big + 6}", target={"root_cols": big + 6, "top2": big + 6 <= 84})
            for big in (78, 79)]


def families():
    return single_front_family() + level_families() + nc_mod4_family() + top_family()


# ------------------------------------------------------------------ values
VALUE_SETS = ("well", "indef", "ipm")


def values(S: Structure, kind: str, seed: int, free_frac=0.1):
    """(Jv, Hv, Dd, sigp, hd, rtype, hsc): the inputs of the Newton matrix of sqphip_mf_host_solve for one instance"""
    rng = np.random.default_rng(seed)
    n, m = S.n, S.m
    deg = np.bincount(np.concatenate([S.hrow, S.hcol]) - 1, minlength=n)
    diag = S.hrow == S.hcol
    scale = 1.0 / np.sqrt(np.maximum(deg[S.hrow - 1], deg[S.hcol - 1]))
    Jv = rng.normal(size=len(S.jrow))
    eq = S.eq
    rt = np.where(eq, 1, 2).astype(np.int32)
    rt[(~eq) & (rng.uniform(size=m) < free_frac)] = 0
    hd = rng.uniform(0, 1, n)
    if kind == "well":
        Hv = np.where(diag, rng.uniform(1, 2, len(S.hrow)), 0.5 * scale * rng.normal(size=len(S.hrow)))
        Dd = rng.uniform(0.1, 10, m); Dd[eq] = rng.uniform(0, 1e-3, eq.sum())
        sigp = rng.uniform(1, 20, n)
        hsc = 0.7
    elif kind == "indef":
        # a fifth of the diagonal negative, kept away from zero: pivots without pivoting stay of moderate size
        sgn = np.where(rng.uniform(size=len(S.hrow)) < 0.2, -1.0, 1.0)
        Hv = np.where(diag, sgn * rng.uniform(1, 2, len(S.hrow)), 0.3 * scale * rng.normal(size=len(S.hrow)))
        Dd = rng.uniform(0.5, 10, m); Dd[eq] = rng.uniform(1e-4, 1e-3, eq.sum())
        sigp = rng.uniform(0.1, 0.5, n)
        hd = np.zeros(n)
        hsc = 1.0
    elif kind == "ipm":
        Hv = np.where(diag, rng.uniform(1, 2, len(S.hrow)), 0.5 * scale * rng.normal(size=len(S.hrow)))
        Dd = 10.0 ** rng.uniform(-9, 9, m); Dd[eq] = 0.0
        sigp = 10.0 ** rng.uniform(-9, 9, n)
        hsc = 1.0
    else:
        raise ValueError(kind)
    return Jv, Hv, Dd, sigp, hd, rt, hsc


def dense_newton(S: Structure, cond, Jv, Hv, Dd, sigp, hd, rt, hsc, dw):
    """The matrix sqphip_mf_host_solve and the kernels factorise, assembled densely by an independent route (unknowns:
    variables, then the kept rows in row order)."""
    n, m = S.n, S.m
    J = np.zeros((m, n)); np.add.at(J, (S.jrow - 1, S.jcol - 1), Jv)
    H = np.zeros((n, n)); np.add.at(H, (S.hrow - 1, S.hcol - 1), Hv); H = H + H.T - np.diag(np.diag(H))
    kept = S.kept(cond)
    J = J * (rt != 0)[:, None]
    W = hsc * H + np.diag(hd + sigp + dw + 1e-8)
    el = ~kept & (rt != 0)
    W = W + J[el].T @ (J[el] / (Dd[el] + 1e-8)[:, None])
    Dk = np.where(rt[kept] != 0, Dd[kept] + 1e-8, 1.0)
    return np.block([[W, J[kept].T], [J[kept], -np.diag(Dk)]])


def next_shift(dw, dw_last):
    """dev_util.hpp next_shift: the next delta_w of the inertia-correction schedule"""
    if dw == 0.0:
        return 1e-4 if dw_last == 0.0 else max(1e-20, dw_last / 3.0)
    return dw * (100.0 if dw_last == 0.0 else 8.0)


def backward_error(K, x, b):
    """normwise backward error |Kx - b|_inf / (|K|_inf |x|_inf + |b|_inf), residual in long double"""
    Kl = K.astype(np.longdouble)
    r = Kl @ x.astype(np.longdouble) - b.astype(np.longdouble)
    knorm = float(np.abs(K).sum(axis=1).max())
    return float(np.abs(r).max()) / (knorm * float(np.abs(x).max()) + float(np.abs(b).max()))
