"""Sub-problems whose outcome is decided by the elastic variables of the seat (`sqphip_qp_solve`, oracle `ora_qp_solve`):
every row carries t+ >= 0 and t- >= 0 (b + J p + t+ - t- inside [gL, gU]), priced at rho_big = 1e4 on a hard row and at
mu_pen * sf on a soft one, and `b_qp_finish` (csrc/ipm.hip) accepts the run, restarts it with rho_big * 100, runs a
phase 1 (options.ipm_phase1) or reports LOCALLY_INFEASIBLE.  Three generators on top of tests/planted_qps.py (same
patterns, same seeds, same `PlantedQp`), each with an arithmetic reference that needs no solver:

  elastic(name, mu)          mode L1QP.  The last m // 2 rows are declared non-linear (soft); about half of the inactive
                             ones are violated at the planted point by t* in [0.1, 1]: from below (gL_i = r_i + t*, lam_i = +mu,
                             slack[i] = t*) or from above (gU_i = r_i - t*, lam_i = -mu, slack[m + i] = t*), r = b + J p*.
                             c = J'lam + zL + zU - H p* is formed again.  H is strictly diagonally dominant, so p* is the
                             unique minimiser of the l1-penalised programme; the multipliers of the violated rows are pinned
                             at +-mu and the rank condition of planted_qps.py on the active rows carries over: the planted
                             (p, lam, zL, zU, slack) is THE answer.  mu = 1000 pushes max|c| above 100, where both
                             implementations scale the objective by sf = 100 / max|c|.
  farkas(name, kind, place)  an infeasible programme with its certificate: y over k rows with
                                 sum_{y_i>0} y_i (gL_i - b_i) + sum_{y_i<0} y_i (gU_i - b_i) - sum_j max(w_j lb_j, w_j ub_j) >= 0.1,
                             w = J'y, [lb, ub] the (always bounded) step box; `certificate_margin` evaluates it in
                             np.longdouble.  The expected answer has no tolerance: LOCALLY_INFEASIBLE and zeros.
                             Kinds: one row out of the box's reach, two rows reachable alone and inconsistent together,
                             five rows with y of mixed signs, one row with all-zero coefficients.
  restart(name, nrows)       one or two active rows scaled by 1e-4 (entries, b_i, gL_i, gU_i) with multipliers of
                             1.2e4 .. 2e4: above RHO_BIG0 = 1e4, far below 1e6, so the first run leaves elastic mass on a
                             feasible hard row and exactly one restart solves it.

Tolerances follow the convention at the top of planted_qps.py: each is 10 x the ORACLE's worst error over the committed
cases, rounded up to one digit, per class (the mu = 1000 cases, the restart cases and the one case of 1100 rows are
less accurate and have constants of their own); tests/test_elastic_cases_cpu.py holds the oracle to a tenth of each.  p, mult_x_L, mult_x_U are
`PQ.rel`; lam is entry-wise |d_i| / max(1, |lam_i*|) (one entry of 2e4 would hide every other under `rel`); slack is
entry-wise over max(1, max t*) = 1, all 2 m entries.

Pure numpy.  The oracle binding is imported only inside `PQ.oracle_solver`.
"""
from __future__ import annotations

import dataclasses
import numpy as np

import planted_qps as PQ
from planted_qps import LD, inf

MARGIN_MIN = 0.1                    # certificate margin in row units: seven orders above ELASTIC_TOL = 1e-8
ROW_SCALE = 1e-4                    # restart cases (below it ELASTIC_TOL, which is absolute, limits the method itself)
RHO_BIG0 = 1e4
VECS = ("p", "lam", "mult_x_L", "mult_x_U", "slack")

# ---- the oracle's own worst errors (oracle/qp_ipm.c), measured over the committed cases below under the default options,
# kkt_condense = 0, kkt_mode = 1 and ipm_corrector = 1 (restart cases: ipm_phase1 = 0 and 1 as well; the cases of
# stride-1100 under the sparse solver, kkt_mode = 2, alone, with kkt_condense = 0 and with ipm_corrector = 1), and 10 x
# that, rounded up to one digit:
ORACLE_WORST_ELASTIC = dict(p=1.06e-8, lam=4.15e-9, mult_x_L=2.88e-9, mult_x_U=2.21e-9, slack=2.88e-8)         # mu = 3, 10
ORACLE_WORST_ELASTIC_STRIDE = dict(p=3.04e-8, lam=8.69e-8, mult_x_L=5.50e-8, mult_x_U=1.35e-7, slack=5.13e-8)  # stride-1100
ORACLE_WORST_ELASTIC_SF = dict(p=1.27e-7, lam=7.83e-8, mult_x_L=8.09e-8, mult_x_U=4.29e-8, slack=3.03e-7)      # mu = 1000 (sf < 1)
ORACLE_WORST_RESTART = dict(p=6.64e-6, lam=9.76e-6, mult_x_L=9.71e-6, mult_x_U=2.57e-6)
ORACLE_WORST_SOFT = dict(feasibility=5.17e-13, hard_slack=1.0014e-14)   # soft certificate rows: the hard rows of the returned point
ELASTIC_TOL = dict(p=2e-7, lam=5e-8, mult_x_L=3e-8, mult_x_U=3e-8, slack=3e-7)
ELASTIC_STRIDE_TOL = dict(p=4e-7, lam=9e-7, mult_x_L=6e-7, mult_x_U=2e-6, slack=6e-7)
ELASTIC_SF_TOL = dict(p=2e-6, lam=8e-7, mult_x_L=9e-7, mult_x_U=5e-7, slack=4e-6)
# the slacks of a restart case all vanish: PQ.SLACK_TOL, a requirement (the oracle leaves 1.1e-16 after its second run at
# rho_big = 1e6)
RESTART_TOL = dict(p=7e-5, lam=1e-4, mult_x_L=1e-4, mult_x_U=3e-5, slack=PQ.SLACK_TOL)
SOFT_TOL = dict(feasibility=6e-12, hard_slack=2e-13)


_cache: dict = {}


@dataclasses.dataclass
class ElasticCase(PQ.PlantedQp):
    slack: np.ndarray | None = None     # planted [t+; t-] (elastic, restart); None for a certificate case
    mu: float = 1.0
    rows: tuple = ()                    # the violated / certificate / scaled rows
    y: np.ndarray | None = None         # Farkas vector over all m rows (zero off `rows`)
    kind: str = ""

    def planted(self):
        return dict(p=self.p, lam=self.lam, mult_x_L=self.mult_x_L, mult_x_U=self.mult_x_U, slack=self.slack)


def _derive(q: PQ.PlantedQp, **changes) -> ElasticCase:
    f = {fd.name: getattr(q, fd.name) for fd in dataclasses.fields(PQ.PlantedQp)}
    for k in ("jrow", "jcol", "jval", "b", "gL", "gU", "lam", "c"):
        f[k] = f[k].copy()
    f.update(changes)
    return ElasticCase(**f)


VEC_THREADS = 1024                  # threads of a vector stage of csrc/ipm.hip (SQPHIP_VEC_THREADS): its strided loops take a second trip from here
STRIDE_NAME = "stride-1100"
STRUCTURES = {STRIDE_NAME: (1030, 1100, dict(local=True))}    # n and m past VEC_THREADS; banded, so that the sparse solvers stay quick


def base(name) -> PQ.PlantedQp:
    """The planted QP a case is made from: a name of planted_qps.py, or one of STRUCTURES above."""
    if name not in STRUCTURES:
        return PQ.case(name)
    if ("base", name) not in _cache:
        n, m, o = STRUCTURES[name]
        _cache["base", name] = PQ.generate(n, m, pseed=0, vseed=0, **o)
    return _cache["base", name]


def far_index(m):
    """Where the 'far' rows of a case begin: at 1024 where m allows (the second trip of every loop of a vector stage
    strided by its 1024 threads); else at 256 (rows of the waves 4 .. 15: a block reduction that dropped part of the
    waves' partial results fails there); else anywhere."""
    return VEC_THREADS if m > VEC_THREADS else 256 if m > 256 else 0


def _dims(name):
    q = base(name)
    return q, q.n, q.m, q.m - q.m // 2


def _has_entries(q):
    return np.bincount(q.jrow - 1, minlength=q.m) > 0


def _stationarity_c(q):
    return (q.jact_mul(q.lam) + q.mult_x_L.astype(LD) + q.mult_x_U.astype(LD) - q.hess_mul(q.p)).astype(np.float64)


# ------------------------------------------------------------------------------------------------ 1. planted elastic optimum
def elastic(name, mu, seed=0) -> ElasticCase:
    """The rows and their t* do not depend on mu: the three mu values of one name differ in lam and c alone."""
    q0, n, m, nl = _dims(name)
    rng = np.random.default_rng([31, n, m, seed])
    elig = np.nonzero((np.arange(m) >= nl) & (q0.rkind >= PQ.R_IN_BELOW) & _has_entries(q0))[0]
    if not len(elig):
        raise RuntimeError(f"elastic case {name}: no inactive non-linear row")
    pick = rng.choice(elig, size=max(1, len(elig) // 2), replace=False)
    if m - 1 in elig and m - 1 not in pick:
        pick[0] = m - 1
    pick = np.sort(pick)
    q = _derive(q0, num_linear=nl, mu=float(mu), rows=tuple(int(i) for i in pick), kind="elastic")
    rx = q.b.astype(LD) + q.jac_mul(q.p); r = rx.astype(np.float64)    # b + J p*; the bounds are placed from its rounded value,
    slack = np.zeros(2 * m)                                             # the planted slack is what that leaves of the exact one
    for i in pick:
        t, below, both, w = rng.uniform(0.1, 1.0), rng.random() < 0.5, rng.random() < 0.5, rng.uniform(0.5, 2.0)
        if below:
            q.gL[i] = r[i] + t; q.gU[i] = q.gL[i] + w if both else inf
            q.lam[i] = mu; slack[i] = float(LD(q.gL[i]) - rx[i])
        else:
            q.gU[i] = r[i] - t; q.gL[i] = q.gU[i] - w if both else -inf
            q.lam[i] = -mu; slack[m + i] = float(rx[i] - LD(q.gU[i]))
    q.slack = slack
    q.c = _stationarity_c(q)
    return q


# ------------------------------------------------------------------------------------------------ 2. planted infeasibility
KINDS = ("unreachable-1", "pair", "combo-5", "zero-row-1")
PLACES = ("low", "high")


def place_range(m, nl, place):
    """'low': linear rows below index 64; 'high': non-linear rows, from `far_index(m)` on, the last row m - 1 always
    among the chosen ones."""
    return (0, min(64, nl)) if place == "low" else (max(far_index(m), nl), m)


def _row_reach(Jd, q, i):
    """[min, max] of b_i + J_i p over the step box, in np.longdouble."""
    lb, ub = (v.astype(LD) for v in q.box())
    a = Jd[i]
    return LD(q.b[i]) + np.minimum(a * lb, a * ub).sum(), LD(q.b[i]) + np.maximum(a * lb, a * ub).sum()


def _set_side(q, rng, i, lower, value):
    """Row i must lie at or above (lower) / at or below `value`; an equality row stays one, an inequality row keeps the
    other side infinite or gets a finite one further out (the row types of a structure are fixed at creation)."""
    value = float(value); w = rng.uniform(0.5, 2.0); both = rng.random() < 0.5
    if q.gL[i] == q.gU[i]: q.gL[i] = q.gU[i] = value
    elif lower: q.gL[i] = value; q.gU[i] = value + w if both else inf
    else: q.gU[i] = value; q.gL[i] = value - w if both else -inf


def certificate_margin(q: ElasticCase) -> float:
    """The left-hand side of the certificate inequality, in np.longdouble."""
    y = q.y.astype(LD); lb, ub = (v.astype(LD) for v in q.box())
    assert np.all(np.isfinite(q.gL[q.y > 0])) and np.all(np.isfinite(q.gU[q.y < 0]))
    w = q.jact_mul(y)
    pos, neg = q.y > 0, q.y < 0
    lhs = (y[pos] * (q.gL[pos].astype(LD) - q.b[pos].astype(LD))).sum() + (y[neg] * (q.gU[neg].astype(LD) - q.b[neg].astype(LD))).sum()
    return float(lhs - np.maximum(w * lb, w * ub).sum())


def row_reachable(q: PQ.PlantedQp, i) -> bool:
    """Row i alone can be satisfied inside the step box."""
    lo, hi = _row_reach(q.dense(LD)[1], q, i)
    return bool(lo <= LD(q.gU[i]) and hi >= LD(q.gL[i]))


def farkas(name, kind, place, seed=0) -> ElasticCase:
    q0, n, m, nl = _dims(name)
    rng = np.random.default_rng([37, n, m, KINDS.index(kind), PLACES.index(place), seed])
    lo_i, hi_i = place_range(m, nl, place)
    cand = np.array([i for i in range(lo_i, hi_i) if _has_entries(q0)[i]], dtype=int)
    k = {"unreachable-1": 1, "pair": 2, "combo-5": min(5, len(cand)), "zero-row-1": 1}[kind]
    if len(cand) < k or k == 0:
        raise RuntimeError(f"certificate case {name} {kind} {place}: {len(cand)} candidate rows")
    rows = rng.choice(cand, size=k, replace=False)
    long = cand[np.bincount(q0.jrow - 1, minlength=m)[cand] > 32]
    if kind == "combo-5" and len(long) and long[0] not in rows:
        rows[0] = long[0]                                               # a row too long to eliminate (it stays in the condensed matrix)
    if place == "high" and m - 1 not in rows:
        if m - 1 not in cand: raise RuntimeError(f"certificate case {name} {kind} {place}: the last row has no entries")
        rows[-1] = m - 1
    q = _derive(q0, num_linear=nl, rows=tuple(int(i) for i in rows), kind=kind, lam=np.zeros(m), p=np.zeros(n),
                mult_x_L=np.zeros(n), mult_x_U=np.zeros(n))
    y = np.zeros(m)
    margin = rng.uniform(0.2, 1.0)
    if kind == "unreachable-1":
        i = rows[0]; lo, hi = _row_reach(q.dense(LD)[1], q, i)
        if rng.random() < 0.5: _set_side(q, rng, i, True, hi + margin); y[i] = 1.0
        else: _set_side(q, rng, i, False, lo - margin); y[i] = -1.0
    elif kind == "zero-row-1":
        # 0'p on the wrong side of its bound by `margin`, whatever p: the violation is a constant, so the point of least
        # elastic cost is the planted optimum of all the other rows and the ONLY elastic mass of the whole programme sits
        # on this row -- at index m - 1 >= far_index(m) ('high') a verdict that looked at the rows of its first trip alone would accept it
        i = rows[0]; q.jval[q.jrow - 1 == i] = 0.0
        if rng.random() < 0.5: _set_side(q, rng, i, True, LD(q.b[i]) + margin); y[i] = 1.0
        else: _set_side(q, rng, i, False, LD(q.b[i]) - margin); y[i] = -1.0
    elif kind == "pair":
        # row i2 := -kappa x (the coefficients of row i1): its own entries stay in the structure with the value 0, the
        # new ones are appended (a structure of its own).  J_i1 p >= a + d and J_i1 p <= a - d contradict by 2 d, each
        # alone can be met inside the box (asserted by the tests through `row_reachable`).
        i1, i2 = rows; kappa = rng.uniform(0.5, 2.0); sgn = 1.0 if rng.random() < 0.5 else -1.0
        e1 = np.nonzero(q.jrow - 1 == i1)[0]
        q.jval[q.jrow - 1 == i2] = 0.0
        q.jrow = np.concatenate([q.jrow, np.full(len(e1), i2 + 1)]); q.jcol = np.concatenate([q.jcol, q.jcol[e1]])
        q.jval = np.concatenate([q.jval, -kappa * q.jval[e1]])
        lo, hi = _row_reach(q.dense(LD)[1], q, i1)
        lo, hi = lo - LD(q.b[i1]), hi - LD(q.b[i1])                      # range of J_i1 p
        d = LD(margin) / 2
        if hi - lo < 4 * d: raise RuntimeError(f"certificate case {name} pair {place}: row {i1} spans {float(hi - lo)}")
        a = lo + LD(rng.uniform(0.35, 0.65)) * (hi - lo)
        # sgn = +1: row i1 from below, row i2 from below (J_i1 p <= (b_i2 - gL_i2) / kappa); sgn = -1: both from above
        _set_side(q, rng, i1, sgn > 0, LD(q.b[i1]) + a + sgn * d)
        _set_side(q, rng, i2, sgn > 0, LD(q.b[i2]) - LD(kappa) * (a - sgn * d))
        y[i1] = sgn; y[i2] = sgn / kappa
    else:
        sg = PQ._sign(rng, k)
        if k >= 2 and abs(sg.sum()) == k: sg[0] = -sg[0]              # mixed signs
        y[rows] = sg * rng.uniform(0.5, 2.0, size=k)
        lb, ub = (v.astype(LD) for v in q.box())
        w = q.jact_mul(y)
        phat = np.where(w > 0, ub, lb)                                  # the box maximiser of w'p
        v = q.b.astype(LD) + q.jac_mul(phat)
        for i in rows:
            _set_side(q, rng, i, y[i] > 0, v[i] + (margin if y[i] > 0 else -margin))
    q.y = y
    q.c = q0.c.copy()
    if certificate_margin(q) < MARGIN_MIN:
        raise RuntimeError(f"certificate case {name} {kind} {place}: margin {certificate_margin(q)}")
    return q


def hard_rows_of(q: ElasticCase, r) -> dict:
    """Of a returned point: the largest violation of a hard (linear) row and of the step box, and the largest elastic
    variable of a hard row -- in np.longdouble.  For the soft variant of a certificate case (rows non-linear, mode L1QP)."""
    nl, m = q.num_linear, q.m
    p = np.asarray(r["p"], dtype=LD); row = q.b.astype(LD) + q.jac_mul(p)
    lb, ub = (v.astype(LD) for v in q.box())
    feas = max([0.0, float((lb - p).max()), float((p - ub).max())] +
               ([float((q.gL[:nl].astype(LD) - row[:nl]).max()), float((row[:nl] - q.gU[:nl].astype(LD)).max())] if nl else []))
    sl = np.asarray(r["slack"])
    return dict(feasibility=feas, hard_slack=float(max(np.abs(sl[:nl]).max(initial=0.0), np.abs(sl[m:m + nl]).max(initial=0.0))))


# ------------------------------------------------------------------------------------------------ 3. penalty restart
def restart(name, nrows, seed=0) -> ElasticCase:
    q0 = base(name); n, m = q0.n, q0.m
    rng = np.random.default_rng([41, n, m, nrows, seed])
    act = np.nonzero((q0.rkind <= PQ.R_AT_GL) & _has_entries(q0))[0]
    far, near = act[act >= max(256, far_index(m))], act[act < 256]
    if len(near) < nrows:
        raise RuntimeError(f"restart case {name}: no {nrows} active rows")
    rows = [int(rng.choice(near))]
    if nrows == 2:                                                      # the second one from far_index(m) on where there is one
        rows.append(int(rng.choice(far if len(far) else near[near != rows[0]])))
    q = _derive(q0, rows=tuple(sorted(rows)), kind="restart", slack=np.zeros(2 * m))
    for i in q.rows:
        lam1 = np.sign(q0.lam[i]) * rng.uniform(1.2, 2.0)
        r_old = float((LD(q0.b[i]) + q0.jac_mul(q0.p)[i]).astype(np.float64))
        q.jval[q.jrow - 1 == i] *= ROW_SCALE; q.b[i] *= ROW_SCALE
        r_new = float((LD(q.b[i]) + q.jac_mul(q.p)[i]).astype(np.float64))
        for g0, g in ((q0.gL, q.gL), (q0.gU, q.gU)):                    # the active side at the new row value, the other scaled
            g[i] = r_new if g0[i] == r_old else (g0[i] if not np.isfinite(g0[i]) else r_new + (g0[i] - r_old) * ROW_SCALE)
        q.lam[i] = lam1 / ROW_SCALE
    q.c = _stationarity_c(q)
    return q


# ------------------------------------------------------------------------------------------------ checks
def elastic_tol(name, mu) -> dict:
    return ELASTIC_STRIDE_TOL if name == STRIDE_NAME else ELASTIC_SF_TOL if mu == 1000.0 else ELASTIC_TOL


def errors(q: ElasticCase, r) -> dict:
    e = {k: PQ.rel(r[k], getattr(q, k)) for k in ("p", "mult_x_L", "mult_x_U")}
    e["lam"] = float((np.abs(np.asarray(r["lam"]) - q.lam) / np.maximum(1.0, np.abs(q.lam))).max(initial=0.0))
    e["slack"] = float(np.abs(np.asarray(r["slack"]) - q.slack).max(initial=0.0) / max(1.0, np.abs(q.slack).max(initial=0.0)))
    return e


def all_zero(r) -> bool:
    return all(not np.any(r[k]) for k in VECS)


# ------------------------------------------------------------------------------------------------ the committed cases
ELASTIC_SIZES = ["65x33", "256x256", "257x300", "300x600", "513x257"]
ELASTIC_MU_SIZES = ["65x33", "257x300"]                       # mu = 3 and mu = 1000
ELASTIC_STRUCTURES = ["long-rows", "dups"]
FARKAS_SIZES = ["7x3", "65x33", "257x300", "300x600"]
ZERO_ROW_SIZES = ["257x300", "300x600"]                       # m > 256
FARKAS_STRUCTURES = ["long-rows", "dups"]                     # combo-5
RESTART_SIZES = ["65x33", "257x300"]
BATCH_NAME = "257x300"
# (mode name, the verdict under it) per placement: the certificate rows are linear ('low': hard in every mode) or
# non-linear ('high': soft under L1QP, where the programme is feasible)
FARKAS_MODES = {"low": ("QP", "SOC", "L1QP", "INFEAS"), "high": ("QP", "SOC")}

def case(gen, *args) -> ElasticCase:
    """A committed case, generated once and shared: treat it as read-only."""
    key = (gen,) + args
    if key not in _cache:
        _cache[key] = {"elastic": elastic, "farkas": farkas, "restart": restart}[gen](*args)
    return _cache[key]


def elastic_list():
    out = [(nm, 10.0) for nm in ELASTIC_SIZES + ELASTIC_STRUCTURES]
    return out + [(nm, mu) for nm in ELASTIC_MU_SIZES for mu in (3.0, 1000.0)]


def farkas_list():
    # (7x3 has m // 2 = 1 non-linear row: no pair among them; its combo-5 has min(5, rows in range) = 2 and 1 rows)
    return [(nm, kd, pl) for nm in FARKAS_SIZES for kd in KINDS[:3] for pl in PLACES if (nm, kd, pl) != ("7x3", "pair", "high")] + \
           [(nm, "zero-row-1", pl) for nm in ZERO_ROW_SIZES for pl in PLACES] + \
           [(nm, "combo-5", pl) for nm in FARKAS_STRUCTURES for pl in PLACES]


def stride_list():
    """One case of every generator past the 1024 threads of a vector stage (run under the sparse solver only)."""
    return [("elastic", STRIDE_NAME, 10.0), ("farkas", STRIDE_NAME, "unreachable-1", "high"), ("farkas", STRIDE_NAME, "combo-5", "high"),
            ("farkas", STRIDE_NAME, "zero-row-1", "high"), ("restart", STRIDE_NAME, 2)]


def restart_list():
    return [(nm, k) for nm in RESTART_SIZES for k in (1, 2)]
