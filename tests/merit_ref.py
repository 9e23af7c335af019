"""Reference of the merit and line-search functions, in exact rational arithmetic.

A plain restatement of
    common.jl:14-77               KT_residuals, norm_complementarity, norm_violations (p = 1, 2, inf)
    sqp.jl:170-213                compute_phi; compute_derivative with scalar and vector penalty and its restoration branch
    sqp_trust_region.jl:487-508   compute_qmodel with and without the step
    sqp_line_search.jl:270-334    compute_mu_rule1! / 2! / 3!, compute_alpha
written from those lines, not from the kernels.  Operands are float64; every sum and product is formed with
`fractions.Fraction` (exact), and a result is rounded to a double once, at the very end: by `float(Fraction)` (correctly
rounded), through one `math.sqrt` for the 2-norms and the row norms, by exact rational division for the quotients.

Every function returns a `Ref(value, mag, depth, tol, exact)`:
    mag     the sum of the absolute values of the elementary terms (products, differences) that enter the result
    depth   the number of floating-point operations on the longest chain from an operand to the result when the same
            quantity is formed in float64 in ANY order: the length of the longest sum, plus the inner sums (a matrix row,
            the copies of a repeated COO entry), plus the few final steps
    tol     2 * depth * 2^-53 * mag -- the first-order bound of a float64 evaluation (Higham, Accuracy and Stability of
            Numerical Algorithms, section 4.2: |fl(sum) - sum| <= (k - 1) u sum |t_i| for every order of summation), times 2
            for the second-order terms and the final square root or division.  For the quotients (KT_residuals,
            norm_complementarity, the penalty rules) the rule is applied to numerator and denominator and propagated:
            |d(N/D)| <= (tol_N + |N/D| tol_D) / (|D| - tol_D) + 2 u |N/D|.
    exact   the result involves only comparisons, differences of two operands and a max: a float64 evaluation must return
            this very double (tol = 0).
The violation functions are piecewise linear with slope 1, so an intermediate that rounding moves across a bound still
moves the result by no more than its own error: `mag` takes the terms of a violated intermediate and its bound, and those
of one that lies within its own rounding error of a bound; an intermediate safely inside adds nothing.

Infinite bounds (+-inf) are sides that do not exist: a comparison against them is false, a minimum skips them."""
from __future__ import annotations

import math
from fractions import Fraction as Fr
from typing import NamedTuple

import numpy as np

U = 2.0 ** -53
ZERO = Fr(0)
HALF = Fr(1, 2)


class Ref(NamedTuple):
    value: float
    mag: float
    depth: int
    tol: float
    exact: bool = False


def _ref(value, mag, depth):
    return Ref(float(value), float(mag), int(depth), 2.0 * depth * U * float(mag))


def _exact(value):
    return Ref(float(value), abs(float(value)), 0, 0.0, True)


def _quot(N, tolN, D, tolD, mag, depth):
    """N / D by exact rational division; N, D Fractions (a float is converted exactly)"""
    N, D = Fr(N), Fr(D)
    q = float(N / D)
    tol = (tolN + abs(q) * tolD) / (float(D) - tolD) + 2.0 * U * abs(q)
    return Ref(q, float(mag), int(depth), tol)


# Conversions of one array object are made once: an entry keeps its arrays alive, so an id is not reused while it is held.
# The operands of the committed cases are read-only; `forget` drops everything.
_memo: dict = {}


def _once(kind, arrays, make):
    if not all(isinstance(a, np.ndarray) for a in arrays): return make()
    key = (kind,) + tuple(id(a) for a in arrays)
    if key not in _memo: _memo[key] = (arrays, make())
    return _memo[key][1]


def forget():
    _memo.clear()


def F(a):
    """exact values of a float64 vector (a shared list: read only)"""
    return _once("F", (a,), lambda: [Fr(float(v)) for v in np.asarray(a, dtype=np.float64)])


def Fb(a):
    """bounds: None for an infinite side"""
    return _once("Fb", (a,), lambda: [Fr(float(v)) if math.isfinite(v) else None for v in np.asarray(a, dtype=np.float64)])


def _abs(a):
    return _once("abs", (a,), lambda: [abs(v) for v in F(a)])


def _dot(xs, ys):
    """sum of x_i y_i, exact, for the long sums.  Every value here is a dyadic rational (a float64, or sums and products of
    such), so its reduced denominator is a power of two: the products are formed on the numerators and summed as Python
    integers over the largest denominator -- the value `sum(x * y)` gives with Fractions, without a gcd per term."""
    nums = [a.numerator * b.numerator for a, b in zip(xs, ys)]
    if not nums: return ZERO
    shift = [a.denominator.bit_length() + b.denominator.bit_length() - 2 for a, b in zip(xs, ys)]
    top = max(shift)
    return Fr(sum(v << (top - k) for v, k in zip(nums, shift)), 1 << top)


def _viol(e, lo, hi):
    """(violation of [lo, hi] by e, |the bound violated|)"""
    if hi is not None and e > hi: return e - hi, abs(hi)
    if lo is not None and e < lo: return lo - e, abs(lo)
    return ZERO, ZERO


def _viols(E, gL, gU, x, xL, xU):
    return _once("viols", (E, gL, gU, x, xL, xU), lambda: [_viol(e, l, h) for e, l, h in zip(F(E), Fb(gL), Fb(gU))] +
                 [_viol(e, l, h) for e, l, h in zip(F(x), Fb(xL), Fb(xU))])


def sparse(rows1, cols1, vals, nrows, sym=False):
    """Rows of a COO matrix (1-based): {column: [sum of the copies, sum of their absolute values, copies]}; sym mirrors the
    off-diagonal entries of a lower triangle.  vals None: zeros."""
    rows1, cols1 = np.asarray(rows1), np.asarray(cols1)
    return _once(("sparse", nrows, sym), (rows1, cols1) + (() if vals is None else (vals,)), lambda: _sparse(rows1, cols1, vals, nrows, sym))


def _sparse(rows1, cols1, vals, nrows, sym):
    M = [dict() for _ in range(nrows)]
    vals = [ZERO] * len(rows1) if vals is None else F(vals)
    for r, c, v in zip(np.asarray(rows1).tolist(), np.asarray(cols1).tolist(), vals):
        for a, b in (((r - 1, c - 1), (c - 1, r - 1)) if sym and r != c else ((r - 1, c - 1),)):
            e = M[a].get(b)
            if e is None: M[a][b] = [v, abs(v), 1]
            else: e[0] += v; e[1] += abs(v); e[2] += 1
    return M


def _shape(M):
    """(longest row, most copies of one entry)"""
    return max([len(r) for r in M] + [0]), max([e[2] for r in M for e in r.values()] + [1])


# ------------------------------------------------------------------------------------------------ common.jl
def norm_violations(E, gL, gU, x, xL, xU, p=1) -> Ref:
    """common.jl:54-77"""
    v = [a for a, _ in _viols(E, gL, gU, x, xL, xU)]
    if p == math.inf: return _exact(max(v + [ZERO]))
    if p == 1: s = sum(v, ZERO); return _ref(s, s, len(v) + 1)
    r = math.sqrt(sum((a * a for a in v), ZERO))            # one difference (twice in the square), the square, the sum
    return _ref(r, r, len(v) + 3)


def norm_complementarity(E, gL, gU, lam, p=math.inf) -> Ref:
    """common.jl:30-47.  The inf-norm of the numerator is a difference of two operands, one product and a max: formed here in
    float64, operation by operation, it is the double every float64 evaluation returns (tol_N = 0)."""
    Ef, lo, hi, lf = F(E), Fb(gL), Fb(gU), F(lam)
    c, den, k = [], ZERO, 0
    for i in range(len(Ef)):
        if lo[i] is not None and hi[i] is not None and lo[i] == hi[i]: c.append(ZERO); continue
        sides = ([Ef[i] - lo[i]] if lo[i] is not None else []) + ([hi[i] - Ef[i]] if hi[i] is not None else [])
        c.append(abs(min(sides) * lf[i])); den += lf[i] * lf[i]; k += 1
    D = 1.0 + math.sqrt(den); tolD = 2.0 * (k + 3) * U * D
    if p == math.inf:
        Ev, l, h, lv = (np.asarray(a, dtype=np.float64) for a in (E, gL, gU, lam))
        with np.errstate(invalid="ignore"):
            N = float(np.max(np.where(l != h, np.abs(np.minimum(Ev - l, h - Ev) * lv), 0.0), initial=0.0))
        assert abs(N - float(max(c + [ZERO]))) <= 4 * U * N
        return _quot(Fr(N), 0.0, D, tolD, N, 2)
    if p == 1:
        s = sum(c, ZERO); return _quot(s, 2.0 * (len(c) + 2) * U * float(s), D, tolD, s, len(c) + 2)
    r = math.sqrt(sum((a * a for a in c), ZERO))
    return _quot(r, 2.0 * (len(c) + 5) * U * r, D, tolD, r, len(c) + 5)


def kt_residuals(df, lam, mult_x_U, mult_x_L, n, m, jrow, jcol, jval) -> Ref:
    """common.jl:14-23"""
    J = sparse(jrow, jcol, jval, m); width, copies = _shape(J)
    dff, lf, uf, wf = F(df), F(lam), F(mult_x_U), F(mult_x_L)
    jtl, mg, cnt = [ZERO] * n, [ZERO] * n, [0] * n
    for i, row in enumerate(J):
        for j, (v, a, _) in row.items():
            jtl[j] += v * lf[i]; mg[j] += a * abs(lf[i]); cnt[j] += 1
    res = [abs(dff[j] + jtl[j] + uf[j] - wf[j]) for j in range(n)]
    magN = max(abs(dff[j]) + mg[j] + abs(uf[j]) + abs(wf[j]) for j in range(n))
    depthN = max(cnt) + copies + 4                            # the copies, the product, the column sum, three more terms
    N = max(res)
    cand = [1.0] + [float(max(abs(v) for v in a)) for a in (dff, uf, wf)]
    cand += [abs(float(lf[i])) * math.sqrt(sum((e[0] * e[0] for e in row.values()), ZERO)) for i, row in enumerate(J)]
    D = max(cand); depthD = width + copies + 4                # the copies, the square, the row sum, the root, the product
    return _quot(N, 2.0 * depthN * U * float(magN), D, 2.0 * depthD * U * D, magN, depthN)


# ------------------------------------------------------------------------------------------------ sqp.jl
def compute_phi(f, E, gL, gU, x, xL, xU, mu, fr) -> Ref:
    """sqp.jl:170-183 at given trial values"""
    v = [a for a, _ in _viols(E, gL, gU, x, xL, xU)]; s = sum(v, ZERO)
    if fr: return _ref(s, s, len(v) + 1)
    f, mu = Fr(float(f)), Fr(float(mu))
    return _ref(f + mu * s, abs(f) + abs(mu) * s, len(v) + 3)


def compute_derivative(df, p, E, gL, gU, mu, mu_vec=None, fr=False, slack=None) -> Ref:
    """sqp.jl:190-213 over merit.jl:13-17.  In the restoration branch the violation of E - viol is zero in exact arithmetic;
    a float64 evaluation leaves up to u (|E_i - g_i| + |g_i|) on a violated row, which `mag` carries."""
    Ef, lo, hi = F(E), Fb(gL), Fb(gU); m = len(Ef)
    w = F(mu_vec) if mu_vec is not None else [Fr(float(mu))] * m
    if fr:
        s = F(slack); dfp, mag, depth = sum(s, ZERO), sum((abs(a) for a in s), ZERO), len(s)
    else:
        t = [a * b for a, b in zip(F(df), F(p))]; dfp, mag, depth = sum(t, ZERO), sum((abs(a) for a in t), ZERO), len(t) + 1
    cv = ZERO
    for i in range(m):
        v, b = _viol(Ef[i], lo[i], hi[i])
        if fr:
            v2, _ = _viol(Ef[i] - v, lo[i], hi[i])
            cv += w[i] * v2; mag += abs(w[i]) * (abs(Ef[i]) + 2 * b if v else ZERO)
        else:
            cv += w[i] * v; mag += abs(w[i]) * v
    return _ref(dfp - cv, mag, max(depth, m + 4) + 1)


# ------------------------------------------------------------------------------------------------ sqp_trust_region.jl
def _quadratic(df, p, n, hrow, hcol, hval):
    """(df'p, 1/2 p'Hp, sum of the absolute terms of both, depth) with H the mirrored lower COO"""
    return _once(("quadratic", n), (df, p, np.asarray(hrow), np.asarray(hcol)) + (() if hval is None else (hval,)),
                 lambda: _quadratic_(df, p, n, hrow, hcol, hval))


def _quadratic_(df, p, n, hrow, hcol, hval):
    H = sparse(hrow, hcol, hval, n, sym=True); width, copies = _shape(H)
    dff, pf, adf, ap = F(df), F(p), _abs(df), _abs(p)
    dfp = _dot(dff, pf)
    php = HALF * _dot(pf, [_dot([e[0] for e in H[j].values()], [pf[k] for k in H[j]]) for j in range(n)])
    mag = _dot(adf, ap) + HALF * _dot(ap, [_dot([e[1] for e in H[j].values()], [ap[k] for k in H[j]]) for j in range(n)])
    return dfp, php, mag, n + width + copies + 4


def compute_qmodel(x, p, df, E, n, m, jrow, jcol, jval, hrow, hcol, hval, gL, gU, xL, xU, mu, with_step) -> Ref:
    """sqp_trust_region.jl:487-508; hval None: no Hessian"""
    muf = Fr(float(mu))
    if not with_step:
        v = [a for a, _ in _viols(E, gL, gU, x, xL, xU)]; s = sum(v, ZERO)
        return _ref(muf * s, abs(muf) * s, len(v) + 2)
    dfp, php, magA, depthA = _quadratic(df, p, n, hrow, hcol, hval)
    J = sparse(jrow, jcol, jval, m); width, copies = _shape(J)
    pf, ap, Ef, xf = F(p), _abs(p), F(E), F(x)
    V, magB = ZERO, ZERO

    def term(t, tmag, chain, l, h):
        """violation of a trial value t (sum of absolute terms tmag, formed in `chain` operations) and what it adds to mag:
        its terms and the bound where it is violated, or lies within its own rounding error of a bound; nothing elsewhere"""
        v, b = _viol(t, l, h)
        if v: return v, tmag + b
        near = [abs(s) for s in (l, h) if s is not None and abs(t - s) <= Fr(2.0 * chain * U) * tmag]
        return v, (tmag + max(near) if near else ZERO)
    for i, (l, h) in enumerate(zip(Fb(gL), Fb(gU))):
        t = Ef[i] + _dot([e[0] for e in J[i].values()], [pf[k] for k in J[i]])
        v, a = term(t, abs(Ef[i]) + _dot([e[1] for e in J[i].values()], [ap[k] for k in J[i]]), width + copies + 2, l, h)
        V += v; magB += a
    for j, (l, h) in enumerate(zip(Fb(xL), Fb(xU))):
        v, a = term(xf[j] + pf[j], abs(xf[j]) + abs(pf[j]), 2, l, h)
        V += v; magB += a
    return _ref(dfp + php + muf * V, magA + abs(muf) * magB, max(depthA, n + m + width + copies + 4) + 2)


# ------------------------------------------------------------------------------------------------ sqp_line_search.jl
def mu_rule_quotient(rho, x, E, df, p, n, hrow, hcol, hval, gL, gU, xL, xU):
    """The quotient the penalty rules share, (df'p + max(1/2 p'Hp, 0)) / max((1 - rho) ||viol||_1, 1e-8) (:272-275, :281-284):
    (its Ref, its exact value)"""
    dfp, php, magN, depthN = _quadratic(df, p, n, hrow, hcol, hval)
    v = [a for a, _ in _viols(E, gL, gU, x, xL, xU)]; s = sum(v, ZERO)
    N = dfp + max(php, ZERO)
    D = max((1 - Fr(float(rho))) * s, Fr(1.0e-8))
    t = _quot(N, 2.0 * (depthN + 1) * U * float(magN), D, 2.0 * (len(v) + 3) * U * float(D), magN, depthN + 1)
    return t, N / D


def compute_mu_rule(rule, first, quotient, lam, mu_vec):
    """compute_mu_rule1! / 2! / 3! (:270-294); first: sqp.iter == 1; quotient: the exact value of `mu_rule_quotient`.  Returns
    the updated mu vector.  An entry that is not the quotient is a max of operands: exact."""
    out = []
    for mu_i, l in zip(F(mu_vec), F(lam)):
        if rule == 1: mu_i = max(mu_i, quotient, abs(l))
        elif rule == 2: mu_i = quotient if first else max(mu_i, abs(l))
        else: mu_i = max(mu_i, abs(l))
        out.append(float(mu_i))
    return np.asarray(out, dtype=np.float64)


def compute_alpha(phi, phi0, D, pnorm_inf, tol_direction, eta, tau, min_alpha):
    """compute_alpha (:303-334) over a merit function alpha -> phi(alpha), in float64 as the reference runs it.  Returns
    (alpha, is_valid, evaluations, the smallest relative margin |phi - (phi0 + eta alpha D)| / max(|phi|, |phi0|) of the
    comparisons made; inf when there was none)."""
    alpha, valid, nev, margin = 1.0, True, 0, math.inf
    if pnorm_inf <= tol_direction: return alpha, valid, nev, margin
    while True:
        v = phi(alpha); nev += 1
        rhs = phi0 + eta * alpha * D
        margin = min(margin, abs(v - rhs) / max(abs(v), abs(phi0)))
        if not (v > rhs): break
        if alpha < min_alpha: valid = False; break
        alpha *= tau
    return alpha, valid, nev, margin


# ------------------------------------------------------------------------------------------------ every quantity of one case
PNORMS = (1, 2, math.inf)


def reference_values(P, B, o) -> dict:
    """Every merit quantity of structure P (n, m, jrow, jcol, hrow, hcol), bounds B (xL, xU, gL, gU) and operands o
    (tests/merit_cases.py): {key: Ref}; the penalty rules as (updated vector, Ref of the quotient)."""
    n, m = P.n, P.m
    bx = (B.gL, B.gU, o.x, B.xL, B.xU)
    out = {}
    for pn in PNORMS:
        out["viol", pn] = norm_violations(o.E, *bx, pn)
        out["compl", pn] = norm_complementarity(o.E, B.gL, B.gU, o.lam, pn)
    out["kt"] = kt_residuals(o.df, o.lam, o.mult_x_U, o.mult_x_L, n, m, P.jrow, P.jcol, o.Jval)
    for fr in (0, 1):
        out["phi", fr] = compute_phi(o.f, o.E, *bx, o.mu, fr)
    q = lambda hv, ws: compute_qmodel(o.x, o.p, o.df, o.E, n, m, P.jrow, P.jcol, o.Jval, P.hrow, P.hcol, hv, B.gL, B.gU, B.xL, B.xU, o.mu, ws)
    out["q", "step"], out["q", "nohess"], out["q", "nostep"] = q(o.Hval, True), q(None, True), q(o.Hval, False)
    out["D5"] = compute_derivative(o.df, o.p, o.E, B.gL, B.gU, o.mu)
    for vec in (None, o.mu_vec):
        for fr in (0, 1):
            out["D", vec is not None, fr] = compute_derivative(o.df, o.p, o.E, B.gL, B.gU, o.mu, vec, bool(fr), o.slack)
    t, tf = mu_rule_quotient(o.rho, o.x, o.E, o.df, o.p, n, P.hrow, P.hcol, o.Hval, B.gL, B.gU, B.xL, B.xU)
    for rule in (1, 2, 3):
        for it in (1, 4):
            out["mu", rule, it] = (compute_mu_rule(rule, it == 1, tf, o.lam, o.mu_vec), t)
    forget()
    return out


def check_against(ref, got, what):
    """`got` ({key: float, or the vector of a penalty rule}) against `reference_values` under the tolerance rule: == where the
    reference is exact, |got - value| <= tol elsewhere.  An entry of a penalty vector that lies above the quotient by more
    than the quotient's tolerance is a max of operands under every float64 evaluation: compared bit for bit; the others
    (the quotient, or within its tolerance of it) by the quotient's tolerance.  Prints every figure before it asserts."""
    for key, r in ref.items():
        if key not in got: continue
        if key[0] == "mu":
            vec, t = r
            assert got[key].shape == vec.shape, (what, key)
            err = float(np.abs(got[key] - vec).max(initial=0.0))
            print(what, key, "largest difference", err, "tol", t.tol)
            if key[1] == 3 or (key[1] == 2 and key[2] != 1): assert np.array_equal(got[key], vec), (what, key)
            else:
                plain = vec > t.value + t.tol
                assert np.array_equal(got[key][plain], vec[plain]) and err <= t.tol, (what, key, err, t)
        else:
            err = abs(got[key] - r.value)
            print(what, key, "got", got[key], "reference", r.value, "difference", err, "tol", r.tol, "exact" if r.exact else "")
            assert (got[key] == r.value) if r.exact else (err <= r.tol), (what, key, got[key], r, err)
