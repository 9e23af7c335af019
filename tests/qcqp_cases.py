"""Cases for the general sparse QCQP path (sqphip_qcqp_attach, csrc/qcqp_dev.hpp qcqp_eval, k_armijo<ARMIJO_QCQP> and the device SQP
loop on a QCQP context) at the edges of the plan builder and past one stride of the 1024-thread workgroup.  Used by
tests/test_qcqp_cases_cpu.py (no GPU) and tests/test_gpu_qcqp_cases.py.

    QcqpExact       f, grad f, g, the Jacobian and the Lagrangian-Hessian values of a Qcqp at a point in exact rational
                    arithmetic (fractions.Fraction over the term lists; neither the device's plans nor QcqpRef), with the
                    device's slot convention: the first copy of a duplicated COO slot carries the value, later copies and
                    slots no term needs are 0.  Every entry comes with L, the number of products summed into it, and S, the
                    exact sum of the absolute values of its addends.
    check           |got - exact| <= max(gamma(L + 4) S, 2^-1074) per entry, gamma(k) = k u / (1 - k u), u = 2^-53; an entry
                    with L = 0 must be the exact constant (0, c_j, g0_i).  The bound is derived, not measured:

                    an entry is a constant (f0, c_j, g0_i or nothing) plus L products of at most four doubles each (the 1/2 of
                    a diagonal term is one of them and is exact).  A product takes at most 3 roundings, and in ANY summation
                    order -- a sequential plan row, numpy's pairwise sums, the reduction tree of f -- an addend passes through
                    at most L additions, so it carries a factor (1 + d)^k with k <= L + 3 and |d| <= u, and
                    |got - exact| <= gamma(L + 3) (|constant| + sum |product|) <= gamma(L + 4) S.  S therefore counts the
                    constant among the addends (a sum g0_i + p rounds by up to u |g0_i| however small p is), L counts the
                    products alone.  A fused multiply-add only removes roundings.  2^-1074 is the spacing of the subnormals.
    edge_model      a hand-made model that holds every branch of the plan builder (the list in its docstring), its variants
                    without Q0 terms, without A terms and with an empty Hessian structure
    stride_model    qcqp_synth with n, nnzQ0, m, nnzJ and nnzH past two strides (a third, partial trip of every loop)
    disc_model      1030 independent discs min c'x s.t. |x_k|^2 <= r_k^2 with a closed-form optimum: n = 2060, m = 1030
    armijo_cases    steps for sqphip_acopf_armijo on stride_model with the backtracking loop over QcqpExact as reference"""
from __future__ import annotations

import dataclasses
import functools
from fractions import Fraction

import numpy as np

from oracle import oracle as O
from qcqp_ref import OracleQcqp, coo_sum
from sqpsolver_jl_amd.qcqp import Qcqp, QcqpLayout, make_qcqp, qcqp_layout, qcqp_scenario, qcqp_synth

U = Fraction(1, 2 ** 53)
TINY = Fraction(1, 2 ** 1074)
OUTPUTS = ("f", "grad", "g", "jval", "hval")


def gamma(k: int) -> Fraction:
    return k * U / (1 - k * U)


# ------------------------------------------------------------------------------------------------ the exact reference
@dataclasses.dataclass
class Exact:
    """One output: per entry the exact value, the number of products in it and the sum of the absolute addends"""
    val: list
    L: list
    S: list

    def floats(self):
        """the values rounded to double (float(Fraction) rounds correctly)"""
        return np.array([float(v) for v in self.val])

    def bound(self, k):
        return max(gamma(self.L[k] + 4) * self.S[k], TINY)


class _Acc:
    def __init__(self, const):
        self.val = [Fraction(c) for c in const]
        self.S = [abs(v) for v in self.val]
        self.L = [0] * len(self.val)

    def add(self, k, p):
        self.val[k] += p
        self.S[k] += abs(p)
        self.L[k] += 1

    def done(self):
        return Exact(self.val, self.L, self.S)


HALF = Fraction(1, 2)


class QcqpExact:
    def __init__(self, q: Qcqp):
        self.q = q
        fr = lambda a: [Fraction(float(v)) for v in a]
        self.q0v, self.av, self.qv, self.c, self.g0 = fr(q.q0v), fr(q.av), fr(q.qv), fr(q.c), fr(q.g0)
        self.q0 = list(zip((q.q0r - 1).tolist(), (q.q0c - 1).tolist()))
        self.a = list(zip((q.ar - 1).tolist(), (q.ac - 1).tolist()))
        self.qq = list(zip((q.qi - 1).tolist(), (q.qr - 1).tolist(), (q.qc - 1).tolist()))

    @staticmethod
    def _x(x):
        """a point as rationals: doubles, or rationals as they are (the exact differences of the CPU test)"""
        return [v if isinstance(v, Fraction) else Fraction(float(v)) for v in x]

    def f(self, x, _x=None):
        x = _x or self._x(x)
        acc = _Acc([self.q.f0])
        for cj, xj in zip(self.c, x):
            acc.add(0, cj * xj)
        for (r, c), v in zip(self.q0, self.q0v):
            acc.add(0, (HALF * v if r == c else v) * x[r] * x[c])
        return acc.done()

    def grad(self, x):
        x = self._x(x)
        acc = _Acc(self.c)
        for (r, c), v in zip(self.q0, self.q0v):
            acc.add(r, v * x[c])
            if r != c:
                acc.add(c, v * x[r])
        return acc.done()

    def g(self, x, _x=None):
        x = _x or self._x(x)
        acc = _Acc(self.g0)
        for (i, j), v in zip(self.a, self.av):
            acc.add(i, v * x[j])
        for (i, r, c), v in zip(self.qq, self.qv):
            acc.add(i, (HALF * v if r == c else v) * x[r] * x[c])
        return acc.done()

    def fg(self, x):
        xs = self._x(x)
        return self.f(x, xs), self.g(x, xs)

    @staticmethod
    def _first(keys):
        first = {}
        for k, key in enumerate(keys):
            first.setdefault(key, k)
        return first

    def jac(self, x, jrow, jcol):
        x = self._x(x)
        slot = self._first(zip((np.asarray(jrow) - 1).tolist(), (np.asarray(jcol) - 1).tolist()))
        acc = _Acc([0] * len(jrow))
        for (i, j), v in zip(self.a, self.av):
            acc.add(slot[(i, j)], v)
        for (i, r, c), v in zip(self.qq, self.qv):
            acc.add(slot[(i, r)], v * x[c])
            if r != c:
                acc.add(slot[(i, c)], v * x[r])
        return acc.done()

    def hess(self, sigma, lam, hrow, hcol):
        hr, hc = (np.asarray(hrow) - 1).tolist(), (np.asarray(hcol) - 1).tolist()
        slot = self._first((max(r, c), min(r, c)) for r, c in zip(hr, hc))
        acc = _Acc([0] * len(hr))
        if not len(hr):                                     # no Hessian structure: nothing is asked for
            return acc.done()
        sigma, lam = Fraction(float(sigma)), self._x(lam)
        for (r, c), v in zip(self.q0, self.q0v):
            acc.add(slot[(max(r, c), min(r, c))], sigma * v)
        for (i, r, c), v in zip(self.qq, self.qv):
            acc.add(slot[(max(r, c), min(r, c))], lam[i] * v)
        return acc.done()

    def all(self, x, sigma, lam, lay):
        out = dict(f=self.f(x), grad=self.grad(x), g=self.g(x), jval=self.jac(x, lay.jrow, lay.jcol))
        if lam is not None:
            out["hval"] = self.hess(sigma, lam, lay.hrow, lay.hcol)
        return out


def coo_sum_exact(ex: Exact, rows, cols, n, lower=False) -> Exact:
    """The exact twin of qcqp_ref.coo_sum: the copies of a slot summed, on the sorted distinct entries.  The copies after
    the first are exact zeros, so the sum of the device's values adds nothing to the error and the bound is the entry's."""
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    if lower:
        rows, cols = np.maximum(rows, cols), np.minimum(rows, cols)
    uniq, inv = np.unique((rows - 1) * n + cols - 1, return_inverse=True)
    acc = Exact([Fraction(0)] * len(uniq), [0] * len(uniq), [Fraction(0)] * len(uniq))
    for k, u in enumerate(inv.tolist()):
        acc.val[u] += ex.val[k]; acc.L[u] += ex.L[k]; acc.S[u] += ex.S[k]
    return acc


def check(kind, got, ex: Exact):
    """(messages, the largest |got - exact| / bound): every entry of one output against the bound of the module docstring"""
    got = np.atleast_1d(np.asarray(got, dtype=np.float64))
    if len(got) != len(ex.val):
        return [f"{kind}: {len(got)} entries, {len(ex.val)} expected"], np.inf
    msgs, worst = [], 0.0
    for k, v in enumerate(ex.val):
        gk = float(got[k])
        if ex.L[k] == 0:
            if not gk == float(v):
                msgs.append(f"{kind}[{k}] = {gk!r}, no product feeds it: exactly {float(v)!r} expected")
            continue
        if not np.isfinite(gk):
            msgs.append(f"{kind}[{k}] = {gk!r}")
            continue
        err, b = abs(Fraction(gk) - v), ex.bound(k)
        worst = max(worst, float(err / b))
        if err > b:
            msgs.append(f"{kind}[{k}] = {gk!r}, exact {float(v)!r}: off by {float(err / b):.3g} bounds (L = {ex.L[k]})")
    return msgs, worst


def check_all(ev, ex, lay):
    """An evaluator's dict (f, grad, g, jval, hval) against QcqpExact.all, the summed COO views of J and H included.
    (messages, {output: largest ratio})"""
    msgs, ratio = [], {}
    for k, e in ex.items():
        mk, ratio[k] = check(k, ev[k], e)
        msgs += mk
    views =[("jsum", "jval", lay.jrow, lay.jcol, False)] + ([("hsum", "hval", lay.hrow, lay.hcol, True)] if "hval" in ex else [])
    for name, k, rows, cols, lower in views:
        mk, ratio[name] = check(name, coo_sum(ev[k], rows, cols, lay.n, lower), coo_sum_exact(ex[k], rows, cols, lay.n, lower))
        msgs += mk
    return msgs, ratio


def ref_eval(R, x, sigma, lam, lay):
    """The dict of Context.acopf_eval from a qcqp_ref.QcqpRef (or anything with its methods)"""
    return dict(f=R.f(x), grad=R.grad(x), g=R.g(x), jval=R.jac(x, lay.jrow, lay.jcol),
                hval=None if lam is None else R.hess(sigma, lam, lay.hrow, lay.hcol))


@dataclasses.dataclass
class Point:
    x: np.ndarray
    sigma: float
    lam: np.ndarray | None


@dataclasses.dataclass
class Case:
    name: str
    lay: QcqpLayout
    qs: list                 # one Qcqp per instance of the batch: one structure, different values
    point: Point
    slots: tuple             # the instances the evaluator is probed on


# ------------------------------------------------------------------------------------------------ the edge model
EDGE_N, EDGE_ROWS, EDGE_FAN, EDGE_LONG = 12, 9, 40, 6
EDGE_KINDS = ("full", "noQ0", "noA", "noH")
_LONG_A, _LONG_Q = 100, {"full": 220, "noQ0": 220, "noA": 301, "noH": 220}


def _edge_terms(kind, seed):
    """The term lists of the edge model, instance values of `seed` (the structure does not depend on it).
    Rows 1..9 are written out; rows 10..49 are the fan: 40 rows whose one quadratic term sits on the pair (5, 4)."""
    rng, where = np.random.default_rng(seed), np.random.default_rng(5)      # the values of the instance; the long row's places
    val = lambda v: float(v * rng.uniform(0.5, 1.5))                        # a zero stays an exact zero in every instance
    fan = range(EDGE_ROWS + 1, EDGE_ROWS + EDGE_FAN + 1)
    Q0 = [] if kind == "noQ0" else [
        (1, 1, val(1.5)),                                                   # a diagonal Q0 term
        (2, 5, val(-0.4)),                                                  # a Q0 term in the upper triangle
        (5, 4, val(0.8)),                                                   # the Hessian slot the fan rows share
        (6, 6, 0.0),                                                        # a coefficient that is exactly 0.0
        (7, 3, val(0.3))]
    A = [(1, 1, val(0.7)), (1, 2, val(-1.1)), (1, 1, val(0.25)),            # the same (row, col) twice
         (3, 3, val(0.9)),                                                  # a Jacobian slot shared with two Q entries
         (4, 11, val(-0.6)),
         (5, 8, 0.0),
         (7, 1, val(1.3)),
         (9, 11, val(0.45))]
    A += [(EDGE_LONG, int(j), val(rng.standard_normal())) for j in where.integers(1, 12, _LONG_A)]
    A += [(i, 1 + i % 11, val(0.2 + 0.01 * i)) for i in fan]
    if kind == "noA":
        A = []
    Q = [(3, 3, 4, val(0.6)), (3, 3, 3, val(-0.8)),                         # two Q entries on slot (3, 3); a diagonal term
         (4, 6, 7, val(0.5)), (4, 7, 6, val(0.35)),                         # one pair, once in each triangle
         (5, 8, 9, 0.0), (5, 9, 9, val(1.2)),
         (8, 1, 2, val(0.9)),                                               # r < c
         (9, 11, 11, val(0.7))]
    Q += [(EDGE_LONG, int(r), int(c), val(rng.standard_normal())) for r, c in where.integers(1, 7, (_LONG_Q[kind], 2))]
    Q += [(i, 5, 4, val(0.1 + 0.02 * i)) for i in fan]
    return Q0, A, Q


def _edge_structure(kind):
    """The COO structures, entry by entry (not qcqp_layout): (row, col, who feeds the slot).  A variant without A (Q0) terms
    leaves out the slots only A (Q0) feeds."""
    fan = range(EDGE_ROWS + 1, EDGE_ROWS + EDGE_FAN + 1)
    J = [(1, 1, "A"), (1, 2, "A"),
         (3, 3, "AQ"), (3, 4, "Q"),
         (4, 7, "Q"), (4, 6, "Q"), (4, 11, "A"),
         (5, 8, "AQ"), (5, 9, "Q"),
         (7, 10, "none"),                                                   # a slot no term needs
         (7, 1, "A"),
         (8, 2, "Q"), (8, 1, "Q"),
         (9, 11, "AQ"),
         (20, 5, "Q")]                                                      # the first copy of a duplicated slot
    J += [(EDGE_LONG, j, "AQ" if j <= 6 else "A") for j in range(11, 0, -1)]
    for i in fan:
        J += [(i, 5, "Q"), (i, 4, "Q")] + ([(i, 1 + i % 11, "A")] if 1 + i % 11 not in (4, 5) else [])
    J += [(3, 3, "AQ")]                                                     # a later copy of a duplicated slot
    H = [(5, 4, "Q0Q")]
    H += [(r, c, "Q") for r in range(1, 7) for c in range(1, r + 1) if (r, c) != (5, 4)]     # the pairs of the long row
    H += [(7, 3, "Q0"), (7, 6, "Q"), (9, 8, "Q"), (9, 9, "Q"),
          (12, 10, "none"),                                                 # a slot no term needs
          (11, 11, "Q"),
          (5, 4, "Q0Q")]                                                    # a later copy of a duplicated slot
    if kind == "noA":
        J = [e for e in J if e[2] != "A"]
    if kind == "noQ0":
        H = [e for e in H if e[2] != "Q0"]
    if kind == "noH":
        H = []
    return J, H


def _edge_qcqp(kind, seed):
    n, m = EDGE_N, EDGE_ROWS + EDGE_FAN
    Q0, A, Q = _edge_terms(kind, seed)
    rng = np.random.default_rng(1000 + seed)
    c = rng.standard_normal(n)
    c[9] = 0.0                                                              # variable 10: no objective term and c = 0
    cols = lambda T: tuple(list(col) for col in zip(*T)) if T else None
    kw = {k: v for k, v in (("Q0", cols(Q0)), ("A", cols(A)), ("Q", cols(Q))) if v is not None}
    return make_qcqp(n, m, 2, c=c, g0=rng.standard_normal(m), f0=float(rng.standard_normal()), xL=np.full(n, -3.0),
                     xU=np.full(n, 3.0), gL=np.full(m, -10.0), gU=np.full(m, 10.0), x0=np.zeros(n), **kw)


def edge_model(kind="full") -> Case:
    """n = 12, m = 49 (nine rows written out and a fan of 40), two instances with different values.  It holds
      - row 2 without any term (g = g0 exactly, an empty plan row); without A terms rows 1 and 7 as well
      - variable 11 in no objective term (grad = c_j), variable 10 with c_j = 0 as well, variable 12 in no term whatsoever
      - the Jacobian slot (3, 3) fed by an A entry and by two Q entries of row 3
      - (1, 1) twice in A
      - the pair (6, 7) of row 4 once in each triangle
      - diagonal Q_i terms (rows 3, 5, 9 and the long row)
      - the Q0 term (2, 5) in the upper triangle, the diagonal Q0 term (1, 1)
      - the Jacobian slots (3, 3) and (20, 5) twice in the structure, (7, 10) that no term needs
      - the Hessian slot (5, 4) twice in the structure, (12, 10) that no term needs
      - the Hessian slot (5, 4) fed by Q0 and by the 40 fan rows
      - row 6 with more than 300 terms
      - coefficients that are exactly 0.0 in Q0, A and Q
      - an odd number of values per instance (483: the block is padded); the variants have an even number"""
    assert kind in EDGE_KINDS
    qs = [_edge_qcqp(kind, seed) for seed in (11, 12)]
    J, H = _edge_structure(kind)
    i64 = lambda v: np.array(v, dtype=np.int64)
    q = qs[0]
    lay = QcqpLayout(q.n, q.m, q.num_linear, i64([e[0] for e in J]), i64([e[1] for e in J]), i64([e[0] for e in H]),
                     i64([e[1] for e in H]), q.xL.copy(), q.xU.copy(), q.gL.copy(), q.gU.copy(), q.x0.copy())
    rng = np.random.default_rng(21)
    p = Point(rng.uniform(-1.5, 1.5, q.n), 0.7, None if kind == "noH" else rng.standard_normal(q.m))
    return Case("edge-" + kind, lay, qs, p, (0, 1))


def nvalues(q: Qcqp) -> int:
    """doubles in an instance's block before padding: f0 | c | Q0 | g0 | A | Q"""
    return 1 + q.n + len(q.q0v) + q.m + len(q.av) + len(q.qv)


# ------------------------------------------------------------------------------------------------ the stride model
STRIDE_N, STRIDE_M, STRIDE_SEED, STRIDE_TERMS = 2100, 2090, 9, 2


def _stride_qcqps():
    q = qcqp_synth(STRIDE_N, STRIDE_M, seed=STRIDE_SEED, terms_per_row=STRIDE_TERMS)
    return [q, qcqp_scenario(q, 1, STRIDE_SEED)]


def _stride_case():
    qs = _stride_qcqps()
    q = qs[0]
    rng = np.random.default_rng(31)
    p = Point(q.x0 + 0.3 * rng.standard_normal(q.n), 1.3, rng.standard_normal(q.m))
    return Case("stride", qcqp_layout(q), qs, p, (1,))


@functools.lru_cache(maxsize=None)
def stride_model() -> Case:
    """qcqp_synth past two strides of 1024 in every loop of qcqp_eval, two instances; probed on slot 1"""
    return _stride_case()


_MAKERS = {**{"edge-" + k: functools.partial(edge_model, k) for k in EDGE_KINDS}, "stride": _stride_case}
CASE_NAMES = tuple(_MAKERS)


@functools.lru_cache(maxsize=None)
def case(name) -> Case:
    return _MAKERS[name]()


@functools.lru_cache(maxsize=None)
def exact(name, slot) -> dict:
    """QcqpExact.all of instance `slot` of a case at the case's point: computed once, shared, never changed"""
    cs = case(name)
    return QcqpExact(cs.qs[slot]).all(cs.point.x, cs.point.sigma, cs.point.lam, cs.lay)


# ------------------------------------------------------------------------------------------------ the disc model
def disc_model(C=1030, s=0) -> Qcqp:
    """C independent copies of  min c'x  s.t.  x_{2k-1}^2 + x_{2k}^2 <= r_k^2  inside the box [-5, 5], start (0.1, 0.2);
    scenario s has its own c and r (r enters through the row bounds).  Optimum: disc_optimum."""
    rng = np.random.default_rng(7100 + s)
    r = rng.uniform(0.5, 2.0, C)
    c = rng.uniform(0.5, 2.0, 2 * C) * rng.choice([-1.0, 1.0], 2 * C)
    v = np.arange(1, 2 * C + 1)
    return make_qcqp(2 * C, C, 0, Q=(np.repeat(np.arange(1, C + 1), 2), v, v, np.full(2 * C, 2.0)), c=c, gU=r * r,
                     xL=np.full(2 * C, -5.0), xU=np.full(2 * C, 5.0), x0=np.tile([0.1, 0.2], C))


def disc_optimum(q: Qcqp):
    """(x, objective, multipliers): x_k = -r_k c_k / |c_k|, f = -sum r_k |c_k|, and from c_k + 2 mult_k x_k = 0 the
    multiplier |c_k| / (2 r_k) of the Lagrangian f + sum mult_i g_i -- the sign of sqp_get's mult_g, which is -lambda of
    the run (sqphip_sqp_get; oracle/sqp_tr.c), lambda <= 0 on a row at its upper bound."""
    r = np.sqrt(q.gU)
    ck = q.c.reshape(-1, 2)
    nc = np.hypot(ck[:, 0], ck[:, 1])
    return (-r[:, None] * ck / nc[:, None]).ravel(), float(-(r * nc).sum()), nc / (2.0 * r)


DISC_KW = dict(max_iter=60, tol_infeas=1e-8, tol_residual=1e-8, literal_quirks=0)


@functools.lru_cache(maxsize=None)
def disc_oracle(s):
    """The CPU oracle's run of scenario s (kkt_mode = 2)"""
    q = disc_model(s=s)
    return O.sqp_solve(OracleQcqp(q, qcqp_layout(q)), O.default_options(kkt_mode=2, **DISC_KW))


# ------------------------------------------------------------------------------------------------ the Armijo probe
@dataclasses.dataclass
class ArmijoCase:
    name: str
    mu: float
    fr: bool
    step: np.ndarray
    slope: float | None      # D = slope w viol1(x), w the weight of the violations in phi; None: D = grad f(x)'step
    eta: float = 0.4
    tau: float = 0.9
    min_alpha: float = 1e-6


ARMIJO_SLOT = 1
MARGIN = 1e3
OUTSIDE_SLOPE = 9.0      # "outside": the leaps raise phi along the whole step, so D > 0 (an argument like any other) is placed where
#                          the full step passes without the bounds on x and fails with them; the CPU test asserts both outcomes
_FG = {}


def _exact_fg(q, x):
    """QcqpExact.fg, kept per point: the cases share x and some of them their probes"""
    key = (id(q), np.asarray(x, dtype=np.float64).tobytes())
    if key not in _FG:
        _FG[key] = (q, QcqpExact(q).fg(x))              # (q is held so that its id stays its own)
    return _FG[key][1]


def armijo_point():
    q = stride_model().qs[ARMIJO_SLOT]
    return q.x0 + 0.1 * np.random.default_rng(41).standard_normal(q.n)


def _armijo_cases():
    """Steps on stride_model, slot 1, from x = armijo_point(), a point 0.1 sigma off the start x0, which satisfies every
    row: `back` = 1.8 (x0 - x) heads for x0 and past it, so the violations fall to zero near alpha = 0.56 and are back at
    0.8 of their size at alpha = 1, and (phi(alpha) - phi0) / alpha falls from about -0.2 w viol1(x) at alpha = 1 to
    -1.8 w viol1(x).  D = -2 w viol1(x) (0.4 D = -0.8 w viol1(x)) therefore rejects the first probes and accepts a later
    one.  tau and min_alpha are arguments of the call; the exhausted case halves alpha down to 0.05 (6 probes) so that
    the exact reference stays quick.  In "outside" 40 variables past index 1500 leap over their bounds at alpha = 1."""
    cs = stride_model()
    q, x = cs.qs[ARMIJO_SLOT], armijo_point()
    grad = QcqpExact(q).grad(x).floats()
    back = 1.8 * (q.x0 - x)
    out = [ArmijoCase("descent", 0.0, False, -0.2 * grad, None),
           ArmijoCase("backtracked", 0.0, False, -0.85 * grad, None),
           ArmijoCase("penalty", 5.0, False, back, -2.0),
           ArmijoCase("exhausted", 5.0, False, back, -1e6, tau=0.5, min_alpha=0.05),
           ArmijoCase("restoration", 1.0, True, back, -2.0)]
    step = back.copy()
    far = np.arange(1500, q.n, 15)                                          # past one stride of the bound loop of viol1
    step[far] = np.where(far % 2 == 0, q.xU[far] + 0.5 - x[far], q.xL[far] - 0.3 - x[far])
    out.append(ArmijoCase("outside", 5.0, False, step, OUTSIDE_SLOPE))
    out.append(ArmijoCase("zero", 5.0, False, np.zeros(q.n), -2.0))
    return out


@functools.lru_cache(maxsize=None)
def armijo_cases():
    return tuple(_armijo_cases())


def armijo_reference(q: Qcqp, x, a: ArmijoCase, box=True):
    """compute_alpha (the loop of tests/test_gpu_nlp_general.py) over QcqpExact rounded to double, with the oracle's 1-norm
    of the violations.  (alpha, valid, n_eval), the smallest |phi(alpha) - (phi0 + eta alpha D)| / B over the probes with
    B = gamma(n + nnzQ0 + 4) S_f + mu sum_i gamma(L_i + 4) S_i (mu = 1 in feasibility restoration), phi0, D.
    box = False leaves the bounds on x out of the violations (to show that a case depends on them)."""
    xL, xU = (q.xL, q.xU) if box else (np.full(q.n, -np.inf), np.full(q.n, np.inf))
    w = 1.0 if a.fr else a.mu

    def phi(alpha):
        xt = x + alpha * a.step
        f, g = _exact_fg(q, xt)
        assert f.L[0] == q.n + len(q.q0v)
        B = gamma(f.L[0] + 4) * f.S[0] + Fraction(w) * sum(gamma(L + 4) * S for L, S in zip(g.L, g.S))
        return (0.0 if a.fr else float(f.val[0])) + w * O.norm_violations(g.floats(), q.gL, q.gU, xt, xL, xU, 1), float(B)

    phi0, _ = phi(0.0)
    if a.slope is None:
        D = float(QcqpExact(q).grad(x).floats() @ a.step)
    else:
        D = a.slope * w * O.norm_violations(_exact_fg(q, x)[1].floats(), q.gL, q.gU, x, q.xL, q.xU, 1)
    if not np.abs(a.step).max() > 0.0:
        return (1.0, True, 0), np.inf, phi0, D
    alpha, valid, nev, margin = 1.0, True, 0, np.inf
    while True:
        v, B = phi(alpha); nev += 1
        margin = min(margin, abs(v - (phi0 + a.eta * alpha * D)) / B)
        if not (v > phi0 + a.eta * alpha * D):
            break
        if alpha < a.min_alpha:
            valid = False
            break
        alpha *= a.tau
    return (alpha, valid, nev), margin, phi0, D


@functools.lru_cache(maxsize=None)
def armijo_expected(name):
    a = {c.name: c for c in armijo_cases()}[name]
    return armijo_reference(stride_model().qs[ARMIJO_SLOT], armijo_point(), a)
