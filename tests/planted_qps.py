"""Trust-region QPs with a planted optimum, for the sub-problem seat (`sqphip_qp_solve`, oracle `ora_qp_solve`).

    min  c'p + 1/2 p'Hp   s.t.  gL <= b + J p <= gU,   max(xL - x_k, -delta) <= p <= min(xU - x_k, delta)

The generator chooses the answer first -- a step p*, row multipliers lambda*, bound multipliers zL* >= 0 >= zU* in the
JuMP sign of include/sqphip.h (stationarity  H p + c = J'lambda + zL + zU) -- places bounds so that exactly the chosen
constraints are active with strict complementarity, and then sets  c = J'lambda* + zL* + zU* - H p*.  H is symmetric and
strictly diagonally dominant, so p* is the unique optimum; the multipliers are unique because the active rows, restricted
to the variables not on a bound, have full row rank (smallest singular value above SIGMA_MIN; the generator redraws the
values until it is).  The reference of every comparison is therefore arithmetic, not another solver.

The sparsity pattern and the kind of every row come from `pseed`, every value (and the kind of every variable) from
`vseed`: instances with one pseed share a structure (one context, `set_bounds` per instance).

Options of a case: hfull (all n(n+1)/2 Hessian entries), long_rows (inequality rows of 33 and 40 entries: they stay in
the condensed matrix), empty_row (an inequality row without entries, bounds loose around b_i), dups (repeated COO
entries in both structures, whose values sum), local (entries near the diagonal: a banded pattern for large n).
A row unbounded on both sides is NOT among the options: `sqphip_create` and `sqphip_set_bounds` refuse such a row
(it creates no constraint upstream and would shift the row indexing), which tests/test_gpu_planted_qps.py asserts.

Every row is declared linear (num_linear = m).  Under L1QP a non-linear row is soft with weight mu = 10, and a barrier method
that stops at a barrier value of ipm_tol / 10 = 1e-10 leaves elastic mass 1e-10 / (mu - |lambda|), about 1e-11, on it --
above the 1e-12 the tests hold the slacks to; a hard row carries the weight 1e4 and leaves 1e-14.

Pure numpy.  The oracle binding is imported only inside `oracle_solver`.
"""
from __future__ import annotations

import dataclasses
import numpy as np

inf = np.inf
LD = np.longdouble
SIGMA_MIN = 0.1
DELTA = 1.0
MU_L1QP = 10.0                      # above every planted |lambda| (<= 2): the l1 penalty is exact, all slacks vanish

# variable kinds
V_NONE, V_BOX, V_AT_XL, V_AT_XU, V_AT_PDELTA, V_AT_MDELTA = range(6)
V_NAMES = ("no bounds", "box inside", "at xL", "at xU", "at +delta", "at -delta")
# row kinds
R_EQ, R_AT_GU, R_AT_GL, R_IN_BELOW, R_IN_ABOVE, R_IN_RANGE = range(6)
R_NAMES = ("equality", "active at gU", "active at gL", "inactive, one-sided below", "inactive, one-sided above", "inactive, range")

# ---- tolerances.  None of them comes from the code under test: each is 10 x the worst error of the ORACLE
# (oracle/qp_ipm.c) over the committed case list, rounded up to one significant digit.  The factor 10 is the room
# between two correct implementations of one method that stop at the same ipm_tol on different last digits; the
# device-against-oracle comparison at 1e-8 is the tight one.  tests/test_planted_qps_cpu.py asserts the oracle at one
# tenth of each constant, so a change of the generator that moves the reference's own error cannot loosen the GPU test
# unnoticed.  Errors are `rel` (largest absolute difference over max(1, largest reference entry)).
# Measured over ALL_NAMES (on_bound variants included) under the default options, kkt_condense = 0, kkt_mode = 1 and
# ipm_corrector = 1, modes QP / SOC / L1QP; the KKT figures over the convex, on_bound and nonconvex variants:
ORACLE_WORST = dict(p=7.44e-9, lam=5.48e-9, mult_x_L=8.87e-9, mult_x_U=9.75e-9)
PLANTED_TOL = dict(p=8e-8, lam=6e-8, mult_x_L=9e-8, mult_x_U=1e-7)
ORACLE_WORST_KKT = dict(stationarity=8.22e-10, feasibility=1.48e-12, complementarity=9.9995e-10, sign=0.0, infinite_side=0.0)
KKT_TOL = dict(stationarity=9e-9, feasibility=2e-11, complementarity=1e-8, sign=0.0, infinite_side=0.0)
SLACK_TOL = 1e-12                   # elastic variables of the SOC / L1QP runs (a requirement, not a measurement: the oracle leaves 1.4e-14)


def rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(1.0, np.abs(np.asarray(b)).max())) if len(b) else 0.0


@dataclasses.dataclass
class PlantedQp:
    n: int
    m: int
    num_linear: int
    jrow: np.ndarray            # 1-based COO, as the seat takes it
    jcol: np.ndarray
    hrow: np.ndarray            # lower triangle
    hcol: np.ndarray
    jval: np.ndarray
    hval: np.ndarray
    xL: np.ndarray
    xU: np.ndarray
    gL: np.ndarray
    gU: np.ndarray
    x_k: np.ndarray
    delta: float
    c: np.ndarray
    b: np.ndarray
    p: np.ndarray               # the planted optimum ...
    lam: np.ndarray             # ... and its multipliers (JuMP sign)
    mult_x_L: np.ndarray
    mult_x_U: np.ndarray
    vkind: np.ndarray
    rkind: np.ndarray
    sigma: float                # smallest singular value of the active rows on the free variables (inf: no active row)
    redraws: int
    convex: bool = True

    def dense(self, dtype=np.float64):
        """(H, J) as dense matrices: duplicates summed, the Hessian mirrored."""
        H = np.zeros((self.n, self.n), dtype=dtype); J = np.zeros((self.m, self.n), dtype=dtype)
        np.add.at(H, (self.hrow - 1, self.hcol - 1), self.hval.astype(dtype))
        H = H + np.tril(H, -1).T
        np.add.at(J, (self.jrow - 1, self.jcol - 1), self.jval.astype(dtype))
        return H, J

    def hess_mul(self, v):
        """H v in np.longdouble from the COO entries (duplicates sum, off-diagonal entries count on both sides)."""
        v = np.asarray(v, dtype=LD); out = np.zeros(self.n, dtype=LD); r, c, a = self.hrow - 1, self.hcol - 1, self.hval.astype(LD)
        np.add.at(out, r, a * v[c]); off = r != c; np.add.at(out, c[off], a[off] * v[r[off]])
        return out

    def jac_mul(self, v):
        out = np.zeros(self.m, dtype=LD); np.add.at(out, self.jrow - 1, self.jval.astype(LD) * np.asarray(v, dtype=LD)[self.jcol - 1])
        return out

    def jact_mul(self, w):
        out = np.zeros(self.n, dtype=LD); np.add.at(out, self.jcol - 1, self.jval.astype(LD) * np.asarray(w, dtype=LD)[self.jrow - 1])
        return out

    def box(self):
        """(lb, ub) of the step as both implementations form it (x_k inside [xL, xU] or on it)."""
        return np.maximum(self.xL - self.x_k, -self.delta), np.minimum(self.xU - self.x_k, self.delta)

    def seat_args(self, mode=0, mu=1.0):
        return (mode, self.x_k, self.delta, mu, self.c, self.b, self.jval, self.hval)

    def planted(self):
        return dict(p=self.p, lam=self.lam, mult_x_L=self.mult_x_L, mult_x_U=self.mult_x_U)


# ------------------------------------------------------------------------------------------------ structure
@dataclasses.dataclass
class Pattern:
    n: int
    m: int
    jrow: np.ndarray
    jcol: np.ndarray
    hrow: np.ndarray
    hcol: np.ndarray
    jdup: np.ndarray            # per COO entry: index of the entry it repeats, -1 for a first occurrence
    hdup: np.ndarray
    rkind: np.ndarray
    empty: int                  # index of the row without entries, -1: none


def pattern(n, m, pseed, hfull=False, long_rows=False, empty_row=False, dups=False, local=False, all_eq=False) -> Pattern:
    rng = np.random.default_rng([11, n, m, pseed])
    win = 8                                                     # local: neighbours within this distance
    # Hessian, lower triangle: the diagonal, and about 3 entries below it per column
    if hfull:
        hr, hc = np.tril_indices(n)
    else:
        hr, hc = [np.arange(n)], [np.arange(n)]
        for j in range(n - 1):
            hi = min(n, j + 1 + win) if local else n
            k = min(3, hi - j - 1)
            hr.append(rng.choice(np.arange(j + 1, hi), size=k, replace=False)); hc.append(np.full(k, j))
        hr, hc = np.concatenate(hr), np.concatenate(hc)
    # Jacobian: about 4 entries per row
    jr, jc = [], []
    n_long = 2 if long_rows else 0
    assert not long_rows or (n >= 40 and m >= 3)
    empty = m - 1 if empty_row else -1
    for i in range(m):
        k = (33, 40)[i] if i < n_long else (0 if i == empty else min(n, int(rng.integers(3, 6))))
        if local and k:
            lo = int(rng.integers(0, max(1, n - win))); cols = lo + rng.choice(min(win, n - lo), size=min(k, win, n - lo), replace=False)
        else:
            cols = rng.choice(n, size=k, replace=False)
        jr.append(np.full(len(cols), i)); jc.append(np.sort(cols))
    jr = np.concatenate(jr).astype(np.int64) if m else np.zeros(0, dtype=np.int64)
    jc = np.concatenate(jc).astype(np.int64) if m else np.zeros(0, dtype=np.int64)
    hr, hc = hr.astype(np.int64), hc.astype(np.int64)
    jdup, hdup = np.full(len(jr), -1), np.full(len(hr), -1)
    if dups:                                                    # repeat about a quarter of the entries, in shuffled order
        rng_dup = np.random.default_rng([29, n, m, pseed])      # (a generator of its own: the rest of the structure stays the plain one)

        def repeat(r, c, d):
            pick = rng_dup.choice(len(r), size=max(1, len(r) // 4), replace=False) if len(r) else np.zeros(0, dtype=int)
            r, c, d = np.concatenate([r, r[pick]]), np.concatenate([c, c[pick]]), np.concatenate([d, pick])
            perm = rng_dup.permutation(len(r)); inv = np.empty(len(r), dtype=int); inv[perm] = np.arange(len(r))
            d = d[perm]; d[d >= 0] = inv[d[d >= 0]]
            return r[perm], c[perm], d
        jr, jc, jdup = repeat(jr, jc, jdup)
        hr, hc, hdup = repeat(hr, hc, hdup)
    # row kinds: at most n/3 rows are active (equalities included), the rest inactive
    rk = rng.integers(R_IN_BELOW, R_IN_RANGE + 1, size=m)
    if all_eq:
        assert m <= n // 3
        rk[:] = R_EQ
    else:
        special = {}
        if long_rows: special.update({0: R_AT_GU, 1: R_IN_RANGE})      # inequality rows by definition: one active, one not
        if empty_row: special[empty] = R_IN_RANGE
        others = np.array([i for i in range(m) if i not in special], dtype=int)
        n_act = min(n // 3, (2 * m + 2) // 3) - sum(k <= R_AT_GL for k in special.values())
        act = rng.choice(others, size=max(0, min(n_act, len(others))), replace=False) if len(others) else others
        rk[act] = rng.integers(R_EQ, R_AT_GL + 1, size=len(act))
        for i, k in special.items(): rk[i] = k
    return Pattern(n, m, jr + 1, jc + 1, hr + 1, hc + 1, jdup, hdup, rk, empty)


# ------------------------------------------------------------------------------------------------ values
def _mag(rng, lo, hi, size):
    return rng.uniform(lo, hi, size=size)


def _sign(rng, size):
    return rng.choice([-1.0, 1.0], size=size)


def _draw(P: Pattern, rng):
    n, m = P.n, P.m
    # --- matrices: first occurrences get their values in the order (column, row), whatever the order of the COO entries,
    # so that a structure with repeated entries describes the same matrices as the plain one
    rng_dup = np.random.default_rng(int(rng.integers(2 ** 31)))
    canon = lambda r, c, mask: np.nonzero(mask)[0][np.lexsort((r[mask], c[mask]))]
    first = P.hdup < 0
    hv = np.zeros(len(P.hrow)); off = P.hrow != P.hcol
    sc = min(1.0, 8.0 / n)                                      # keeps the row sums (and with them c) of order 1 for dense H
    idx = canon(P.hrow, P.hcol, first & off)
    hv[idx] = _sign(rng, len(idx)) * _mag(rng, 0.1, 1.0, len(idx)) * sc
    Hs = np.zeros((n, n)); np.add.at(Hs, (P.hrow - 1, P.hcol - 1), hv)
    rowsum = np.abs(Hs).sum(axis=1) + np.abs(Hs).sum(axis=0)
    idx = canon(P.hrow, P.hcol, first & ~off)
    hv[idx] = rowsum[P.hrow[idx] - 1] + _mag(rng, 0.5, 1.5, len(idx))            # strictly diagonally dominant
    jv = np.zeros(len(P.jrow))
    idx = canon(P.jrow, P.jcol, P.jdup < 0)
    jv[idx] = _sign(rng, len(idx)) * _mag(rng, 0.5, 2.0, len(idx))
    for val, dup in ((hv, P.hdup), (jv, P.jdup)):               # a repeated entry takes a share of its original's value
        for k in np.nonzero(dup >= 0)[0]:
            share = rng_dup.uniform(-1.0, 1.0) * val[dup[k]]
            val[k] = share; val[dup[k]] -= share
    # --- point, kinds, multipliers
    x_k = rng.uniform(-1.0, 1.0, size=n)
    p = rng.uniform(-0.8, 0.8, size=n)
    vk = rng.choice([V_NONE, V_BOX], size=n)
    n_act = int(rng.integers(n // 6, n // 3 + 1))              # active bounds: at most n/3
    act = rng.choice(n, size=n_act, replace=False)
    vk[act] = rng.integers(V_AT_XL, V_AT_MDELTA + 1, size=n_act)
    if n_act >= 4: vk[act[:4]] = (V_AT_XL, V_AT_XU, V_AT_PDELTA, V_AT_MDELTA)     # every active kind where there is room
    xL, xU = np.full(n, -inf), np.full(n, inf)
    zL, zU = np.zeros(n), np.zeros(n)
    gap = lambda: rng.uniform(0.2, 1.0)
    for j in range(n):
        k = vk[j]
        if k == V_BOX:                                          # p* strictly inside, and x_k inside the box
            xL[j] = x_k[j] + min(p[j], 0.0) - gap(); xU[j] = x_k[j] + max(p[j], 0.0) + gap()
        elif k == V_AT_XL:
            xL[j] = x_k[j] + p[j]; p[j] = xL[j] - x_k[j]        # the step to the bound as both implementations compute it
            if rng.random() < 0.5: xU[j] = x_k[j] + max(p[j], 0.0) + gap()
            zL[j] = rng.uniform(0.1, 2.0)
        elif k == V_AT_XU:
            xU[j] = x_k[j] + p[j]; p[j] = xU[j] - x_k[j]
            if rng.random() < 0.5: xL[j] = x_k[j] + min(p[j], 0.0) - gap()
            zU[j] = -rng.uniform(0.1, 2.0)
        elif k == V_AT_PDELTA:
            p[j] = DELTA
            if rng.random() < 0.5: xU[j] = x_k[j] + DELTA + gap()
            if rng.random() < 0.5: xL[j] = x_k[j] - gap()
            zU[j] = -rng.uniform(0.1, 2.0)
        elif k == V_AT_MDELTA:
            p[j] = -DELTA
            if rng.random() < 0.5: xL[j] = x_k[j] - DELTA - gap()
            if rng.random() < 0.5: xU[j] = x_k[j] + gap()
            zL[j] = rng.uniform(0.1, 2.0)
    b = rng.uniform(-1.0, 1.0, size=m)
    return hv, jv, x_k, p, vk, xL, xU, zL, zU, b


def generate(n, m, pseed=0, vseed=0, pat: Pattern | None = None, max_tries=200, **opts) -> PlantedQp:
    P = pat if pat is not None else pattern(n, m, pseed, **opts)
    for tries in range(max_tries):
        rng = np.random.default_rng([13, n, m, pseed, vseed, tries])
        hv, jv, x_k, p, vk, xL, xU, zL, zU, b = _draw(P, rng)
        J = np.zeros((m, n)); np.add.at(J, (P.jrow - 1, P.jcol - 1), jv)
        act_rows = np.nonzero(P.rkind <= R_AT_GL)[0]
        free = np.nonzero(vk <= V_BOX)[0]
        if len(act_rows):
            A = J[np.ix_(act_rows, free)]
            sigma = float(np.linalg.svd(A, compute_uv=False).min()) if min(A.shape) and A.shape[0] <= A.shape[1] else 0.0
        else:
            sigma = inf
        if sigma > SIGMA_MIN:
            break
    else:
        raise RuntimeError(f"planted QP ({n}, {m}, pseed {pseed}, vseed {vseed}): no independent active set in {max_tries} draws")
    # --- rows: activity (in extended precision, then rounded once), bounds, multipliers
    q = PlantedQp(n, m, m, P.jrow, P.jcol, P.hrow, P.hcol, jv, hv, xL, xU, np.zeros(m), np.zeros(m), x_k, DELTA,
                  np.zeros(n), b, p, np.zeros(m), zL, zU, vk, P.rkind.copy(), sigma, tries)
    r = (b.astype(LD) + q.jac_mul(p)).astype(np.float64)     # b + J p*: the bound of an active row
    lam = np.zeros(m); gL, gU = np.full(m, -inf), np.full(m, inf)
    for i in range(m):
        k, u, w = P.rkind[i], rng.uniform(0.5, 2.0), rng.uniform(0.5, 2.0)
        if k == R_EQ: gL[i] = gU[i] = r[i]; lam[i] = rng.choice([-1.0, 1.0]) * rng.uniform(0.1, 2.0)
        elif k == R_AT_GU:
            gU[i] = r[i]; lam[i] = -rng.uniform(0.1, 2.0)
            if rng.random() < 0.5: gL[i] = r[i] - u
        elif k == R_AT_GL:
            gL[i] = r[i]; lam[i] = rng.uniform(0.1, 2.0)
            if rng.random() < 0.5: gU[i] = r[i] + u
        elif k == R_IN_BELOW: gL[i] = r[i] - u
        elif k == R_IN_ABOVE: gU[i] = r[i] + u
        else: gL[i] = r[i] - u; gU[i] = r[i] + w
    q.gL, q.gU, q.lam = gL, gU, lam
    q.c = (q.jact_mul(lam) + zL.astype(LD) + zU.astype(LD) - q.hess_mul(p)).astype(np.float64)
    return q


def nonconvex(q: PlantedQp, seed=0) -> PlantedQp:
    """About a third of H's diagonal negated (every COO entry on those diagonal positions): the planted point is no longer
    the answer, only the KKT conditions of whatever local solution is returned can be checked."""
    rng = np.random.default_rng([17, q.n, q.m, seed])
    flip = np.zeros(q.n, dtype=bool); flip[rng.choice(q.n, size=max(1, q.n // 3), replace=False)] = True
    hv = q.hval.copy(); on = (q.hrow == q.hcol) & flip[q.hrow - 1]
    hv[on] = -hv[on]
    return dataclasses.replace(q, hval=hv, convex=False)


def on_bound(q: PlantedQp, seed=0) -> PlantedQp:
    """For about n/6 (at least one) of the variables that have an inactive side, the bound they move AWAY from is put
    exactly at x_k (an SQP iterate sitting on a bound): the optimum and its multipliers stay the planted ones."""
    rng = np.random.default_rng([19, q.n, q.m, seed])
    up_ok = (q.p > 0.05) & ~np.isin(q.vkind, (V_NONE, V_AT_XL, V_AT_MDELTA))     # moves up: the lower bound goes to x_k
    dn_ok = (q.p < -0.05) & ~np.isin(q.vkind, (V_NONE, V_AT_XU, V_AT_PDELTA))
    cand = np.nonzero(up_ok | dn_ok)[0]
    if not len(cand):                                           # (a case of unbounded variables only: bound one of them)
        cand = np.nonzero(np.abs(q.p) > 0.05)[0]
        up_ok = q.p > 0.05
    pick = rng.choice(cand, size=min(len(cand), max(1, q.n // 6)), replace=False)
    xL, xU = q.xL.copy(), q.xU.copy()
    for j in pick:
        if up_ok[j]: xL[j] = q.x_k[j]
        else: xU[j] = q.x_k[j]
    return dataclasses.replace(q, xL=xL, xU=xU)


# ------------------------------------------------------------------------------------------------ checks
def kkt_residuals(q: PlantedQp, r) -> dict:
    """KKT residuals of a returned (p, lam, mult_x_L, mult_x_U) in np.longdouble: stationarity  H p + c - J'lam - zL - zU
    over max(1, largest multiplier); primal infeasibility against rows and box; sign violations (zL >= 0 >= zU);
    complementarity (bound multipliers against the box, lam+ against the lower and lam- against the upper side of its
    row); multiplier mass on an infinite side of a row."""
    p, lam, zL, zU = (np.asarray(r[k], dtype=LD) for k in ("p", "lam", "mult_x_L", "mult_x_U"))
    big = max([1.0] + [float(np.abs(v).max()) for v in (lam, zL, zU) if len(v)])
    stat = float(np.abs(q.hess_mul(p) + q.c.astype(LD) - q.jact_mul(lam) - zL - zU).max()) / big
    lb, ub = (v.astype(LD) for v in q.box())
    row = q.b.astype(LD) + q.jac_mul(p)
    gL, gU = q.gL.astype(LD), q.gU.astype(LD)
    feas = max([0.0, float((lb - p).max()), float((p - ub).max())] + ([float((gL - row).max()), float((row - gU).max())] if q.m else []))
    sign = max(0.0, float((-zL).max()), float(zU.max()))
    comp = max(float((np.abs(zL) * np.abs(p - lb)).max()), float((np.abs(zU) * np.abs(ub - p)).max()))
    mass = 0.0
    lp, ln = np.maximum(lam, 0), np.maximum(-lam, 0)
    ineq = q.gL != q.gU
    for mult, gapv, fin in ((lp, row - gL, np.isfinite(q.gL)), (ln, gU - row, np.isfinite(q.gU))):
        a, bnd = ineq & fin, ineq & ~fin
        if a.any(): comp = max(comp, float((mult[a] * np.abs(gapv[a])).max()))
        if bnd.any(): mass = max(mass, float(mult[bnd].max()))
    return dict(stationarity=stat, feasibility=feas, complementarity=comp, sign=sign, infinite_side=mass)


def structure(q: PlantedQp) -> dict:
    return dict(n=q.n, m=q.m, num_linear=q.num_linear, jrow=q.jrow, jcol=q.jcol, hrow=q.hrow, hcol=q.hcol,
                xL=q.xL, xU=q.xU, gL=q.gL, gU=q.gU)


def oracle_solver(q: PlantedQp, opts=None):
    """The CPU oracle's seat for q's structure and bounds: solve(q2, mode=0, mu=1.0) -> result dict with slacks, for any q2
    that shares them.  COO -> CSC as Julia's sparse(I, J, V) (duplicates summed, the Hessian mirrored)."""
    from oracle import oracle as O
    jcp, jrv, jslot, _ = O.coo_to_csc(q.n, q.jrow, q.jcol)
    hcp, hrv, hslot, hslot_t = O.coo_to_csc(q.n, q.hrow, q.hcol, sym=True)
    s = O.QpSolver(q.n, q.m, q.num_linear, jcp, jrv, hcp, hrv, q.xL, q.xU, q.gL, q.gU, opts)

    def solve(q2, mode=0, mu=1.0):
        jv = np.zeros(len(jrv)); np.add.at(jv, jslot, q2.jval)
        hv = np.zeros(len(hrv)); np.add.at(hv, hslot, q2.hval); ok = hslot_t >= 0; np.add.at(hv, hslot_t[ok], q2.hval[ok])
        return s.solve(mode, q2.x_k, q2.delta, mu, q2.c, q2.b, jv, hv, want_slack=True)
    return solve


# ------------------------------------------------------------------------------------------------ the committed cases
SIZES = [(1, 0), (1, 1), (2, 1), (7, 3), (63, 40), (64, 64), (65, 33), (255, 100), (256, 256), (257, 300), (300, 600), (513, 257)]
STRUCTURES = {                                                  # name: (n, m, options)
    "hfull-2": (2, 1, dict(hfull=True)), "hfull-64": (64, 64, dict(hfull=True)), "hfull-65": (65, 33, dict(hfull=True)),
    "long-rows": (65, 33, dict(long_rows=True)), "empty-row": (65, 33, dict(empty_row=True)),
    "dups": (63, 40, dict(dups=True)), "no-rows-257": (257, 0, dict()), "on-bound-257": (257, 100, dict()),
}
# the last instance whose vectors are staged in LDS (2 n + m = 7000 doubles) and the first that is not
LDS_EDGE = {"lds-7000": (3400, 200, dict(local=True, all_eq=True)), "lds-7001": (3400, 201, dict(local=True, all_eq=True))}

_cache: dict = {}


def case(name, vseed=0) -> PlantedQp:
    """A committed case by name ('65x33', 'hfull-64', 'lds-7000', ...); generated once and shared: treat it as read-only."""
    key = (name, vseed)
    if key not in _cache:
        if name in STRUCTURES: n, m, o = STRUCTURES[name]
        elif name in LDS_EDGE: n, m, o = LDS_EDGE[name]
        else: n, m = (int(v) for v in name.split("x")); o = {}
        _cache[key] = generate(n, m, pseed=0, vseed=vseed, **o)
    return _cache[key]


SIZE_NAMES = [f"{n}x{m}" for n, m in SIZES]
ALL_NAMES = SIZE_NAMES + list(STRUCTURES) + list(LDS_EDGE)
