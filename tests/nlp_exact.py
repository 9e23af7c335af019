"""Test helper for the term evaluator of a factorable NLP (csrc/nlp_dev.hpp nlp_eval passes 1 and 2, nlp_factor and
nlp_kappa_wide): an exact reference with an entry-wise forward error bound, and the cases that are held to it.

    NlpExact        want(x, sigma, lam, lay) -> (values, bounds) of f, grad, g, jval, hval of any NlpTerms without blocks (the
                    interface of nlp_block_ref.NlpBlockRef.want).  The arguments u* = sum a_j x_j + b are formed in rationals
                    from the doubles, kappa .. kappa''' come from closed forms without cancellation in mpmath (kappa_exact),
                    products and sums are exact (rationals) and every entry is rounded to a double once.
    the bound       first-order, absolute, bottom-up (u = 2^-53):
                        argument          du = (nargs + 1) u r,  r = sum |a_j x_j| + |b|
                        stored value      W_q = a^q kappa^(q)(u*) (a: the coefficient of a one-argument factor, else 1):
                                          E_q = c(kind, q) u |W_q| + |a^q kappa^(q+1)(u*)| du,  c = R + L (ROUNDINGS, LIBM)
                        plan entry        c_t prod_k W weights (sigma | lam_i):
                                          sum_k E_k prod_{others} |W| |c_t weights mult| + (nf + 4) u |summand|
                        output entry      of L summands and a constant: sum of the summand bounds + (L + 2) u (sum |summand| +
                                          |constant|)
    check_entries   |got - exact| <= 2 B + 2^-1074 for every entry, no floor relative to the largest entry; an entry without
                    a bound (no summand, or only exact ones) must equal its exact value bit for bit; returns the largest err / B
                    per output and per kind
    mirror_eval     the device's arithmetic in numpy doubles over the same plans, with the kappa function and three plan
                    mutations as parameters: what the CPU tests break on purpose
    menu_model, product_model, stride_model     the cases; tests/test_nlp_exact_cpu.py vouches for them

The domain condition of the cases: every exact W_q, every partial product in factor order, every summand and every output
entry is 0 or has a magnitude in [2^-1020, 2^1012].  (2^1012 and not 2^1000: exp(700) = 2^1009.9 and the Hessian entry
2 / u^2 at u = 2^-500 of the menu are beyond 2^1000; every double operation on them stays finite.)"""
from __future__ import annotations

import dataclasses
from fractions import Fraction

import mpmath as mp
import numpy as np

from sqpsolver_jl_amd.nlp_terms import (ATAN, COS, EXP, LOG, POW, POWR, SIGMOID, SIN, SOFTPLUS, SQRT, TANH, NlpTerms, _kappa3,
                                        make_nlp_terms, nlp_terms_args, nlp_terms_layout)

KEYS = ("f", "grad", "g", "jval", "hval")
KIND_NAMES = {POW: "POW", SIN: "SIN", COS: "COS", EXP: "EXP", LOG: "LOG", SQRT: "SQRT", TANH: "TANH", ATAN: "ATAN",
              SIGMOID: "SIGMOID", SOFTPLUS: "SOFTPLUS", POWR: "POWR"}
U = Fraction(1, 2 ** 53)
TINY = Fraction(1, 2 ** 1074)
DOMAIN = (Fraction(1, 2 ** 1020), Fraction(2 ** 1012))
DPS = 60

# R: the fp64 roundings the device spends on kappa^(q) after its libm calls, q = 0, 1, 2, the products with a and a a
# included (a rounding of a quantity that enters squared counts twice; sqrt and the divisions count as roundings here, their
# libm allowance is 0).  Counted in nlp_factor / nlp_kappa_wide:
#   SIN, COS  s | a c | (a a) s                                                          0, 1, 2
#   EXP       v | a v | a a v                                                            0, 1, 2
#   LOG       log u | a r, r = 1 / u | (a a) (r r)                                       0, 2, 5
#   SQRT      s | 0.5 / s | 0.25 / (u s); a, a a                                         1, 3, 5
#   TANH      t | d = 4 e / (p p), p = 1 + e | 2 t d; a, a a                             0, 5, 7
#   ATAN      atan u | q = 1 / (1 + u u) | 2 (u q) q; a, a a                             0, 4, 10
#   SIGMOID   e den, den = 1 / (1 + e) | s sc = e den den | (s sc) (expm1 den); a, a a   3, 7, 12
#   SOFTPLUS  max(u, 0) + log1p e | s | s sc; a, a a                                     1, 4, 8
#   POWR      v | p v / u | p (p - 1) v / (u u); a, a a                                  0, 3, 7
#   POW       |e| + 2 for every order (at most |e| + 1 factors u or 1 / u, the integer coefficient, a a)
ROUNDINGS = {SIN: (0, 1, 2), COS: (0, 1, 2), EXP: (0, 1, 2), LOG: (0, 2, 5), SQRT: (1, 3, 5), TANH: (0, 5, 7), ATAN: (0, 4, 10),
             SIGMOID: (3, 7, 12), SOFTPLUS: (1, 4, 8), POWR: (0, 3, 7)}
# L: the allowance of the libm calls behind kappa^(q), from the accuracy table of OpenCL 3.0 that the device math library is
# built to meet: sqrt, division 0; log1p 2; exp, log, expm1 3; sin, cos 4; tanh, atan 5; pow 16.  (e enters s, sc, d and
# log1p e with a condition of at most 1, so one exp costs 3 wherever it is used.)
LIBM = {POW: (0, 0, 0), SIN: (4, 4, 4), COS: (4, 4, 4), EXP: (3, 3, 3), LOG: (3, 0, 0), SQRT: (0, 0, 0), TANH: (5, 3, 5 + 3),
        ATAN: (5, 0, 0), SIGMOID: (3, 3, 3 + 3), SOFTPLUS: (3 + 2, 3, 3), POWR: (16, 16, 16)}


def roundings(kind, e, q):
    """c(kind, q) = R + L"""
    return (abs(int(e)) + 2 if kind == POW else ROUNDINGS[kind][q]) + LIBM[kind][q]


def _fr(v):
    """a double or an mpf as a rational, exactly"""
    if isinstance(v, mp.mpf):
        sign, man, ex, _ = v._mpf_
        man = int(man) * (-1 if sign else 1)
        return Fraction(man * 2 ** ex) if ex >= 0 else Fraction(man, 2 ** -ex)
    return Fraction(float(v))


def _mpf(fr):
    return mp.mpf(fr.numerator) / mp.mpf(fr.denominator)


def kappa_exact(kind, e, par, u):
    """kappa, kappa', kappa'', kappa''' at the mpf u from closed forms that do not cancel: sech^2 from exp(-2 |u|), the
    logistic complement from e^u, its difference from tanh(u / 2), log1p for the soft plus.  (kappa''' serves the bound
    alone; its forms vanish at true zeros only.)"""
    if kind == POW:
        e = int(e)
        c = (1, e, e * (e - 1), e * (e - 1) * (e - 2))
        return tuple(c[q] * u ** (e - q) if c[q] else mp.mpf(0) for q in range(4))
    if kind == POWR:
        p = mp.mpf(par)
        c = (1, p, p * (p - 1), p * (p - 1) * (p - 2))
        return tuple(c[q] * u ** (p - q) if c[q] else mp.mpf(0) for q in range(4))
    if kind == SIN:
        return mp.sin(u), mp.cos(u), -mp.sin(u), -mp.cos(u)
    if kind == COS:
        return mp.cos(u), -mp.sin(u), -mp.cos(u), mp.sin(u)
    if kind == EXP:
        return (mp.exp(u),) * 4
    if kind == LOG:
        return mp.log(u), 1 / u, -1 / (u * u), 2 / (u * u * u)
    if kind == SQRT:
        r = mp.sqrt(u)
        return r, 1 / (2 * r), -1 / (4 * u * r), 3 / (8 * u * u * r)
    if kind == TANH:
        t, e2 = mp.tanh(u), mp.exp(-2 * abs(u))
        d = 4 * e2 / (1 + e2) ** 2
        return t, d, -2 * t * d, d * (4 * t * t - 2 * d)
    if kind == ATAN:
        q = 1 / (1 + u * u)
        return mp.atan(u), q, -2 * u * q * q, 2 * q ** 3 * (3 * u * u - 1)
    s, sc, dm = 1 / (1 + mp.exp(-u)), 1 / (1 + mp.exp(u)), -mp.tanh(u / 2)
    if kind == SIGMOID:
        return s, s * sc, s * sc * dm, s * sc * (dm * dm - 2 * s * sc)
    assert kind == SOFTPLUS
    return (u if u > 0 else mp.mpf(0)) + mp.log1p(mp.exp(-abs(u))), s, s * sc, s * sc * dm


# ---- the plans: which summands make an output entry (the ordered-pair form of nlp_general_ref.NlpGeneralRef)
def plans(p: NlpTerms, lay):
    """{output: [entry]} with entry = [(term, factor a, factor b, argument of a, argument of b, row or 0)], factors and
    arguments by their global numbers, -1: none.  Gradient and Jacobian: one summand per (factor, argument) couple on the
    variable; Hessian slot (v, w), v >= w: one per ordered pair of couples on (v, w), the pair of a couple with itself included
    unless its factor is plain linear.  The first copy of a duplicated COO slot owns the entry, the others stay empty."""
    aptr, avar, _ = nlp_terms_args(p)
    n, nt = p.n, len(p.trow)
    plain = (p.fkind == POW) & (p.fexp == 1)
    out = dict(f=[[]], grad=[[] for _ in range(n)], g=[[] for _ in range(p.m)], jval=[[] for _ in lay.jrow], hval=[[] for _ in lay.hrow])
    jfirst, hfirst = {}, {}
    for s, (r, c) in enumerate(zip(np.asarray(lay.jrow).tolist(), np.asarray(lay.jcol).tolist())):
        jfirst.setdefault((r - 1, c - 1), s)
    for s, (r, c) in enumerate(zip(np.asarray(lay.hrow).tolist(), np.asarray(lay.hcol).tolist())):
        hfirst.setdefault((max(r, c) - 1, min(r, c) - 1), s)
    for t in range(nt):
        row = int(p.trow[t])
        (out["f"][0] if row == 0 else out["g"][row - 1]).append((t, -1, -1, -1, -1, row))
        couples = [(k, j, int(avar[j]) - 1) for k in range(int(p.tptr[t]), int(p.tptr[t + 1])) for j in range(int(aptr[k]), int(aptr[k + 1]))]
        for k, j, v in couples:
            (out["grad"][v] if row == 0 else out["jval"][jfirst[(row - 1, v)]]).append((t, k, -1, j, -1, row))
        for ka, ja, v in couples:
            for kb, jb, w in couples:
                if v < w or (ka == kb and plain[ka]):
                    continue
                out["hval"][hfirst[(v, w)]].append((t, ka, kb, ja, jb, row))
    return out


def _orders(p, t, a, b):
    return [(k, (k == a) + (k == b)) for k in range(int(p.tptr[t]), int(p.tptr[t + 1]))]


class NlpExact:
    """want(x, sigma, lam, lay) -> (values, bounds); afterwards .exact holds the rationals, .entry_kind the kind of an entry
    whose summands hold factors of one kind only (-1: mixed or none) and .span the smallest and largest non-zero magnitude
    among the W_q, the partial products, the summands and the outputs (the domain condition)."""

    def __init__(self, p: NlpTerms, dps: int = DPS):
        assert not getattr(p, "blocks", None), "terms only"
        self.p, self.dps = p, int(dps)

    def factors(self, x):
        """per factor: W_q (rationals, q = 0, 1, 2), |W_q| and E_q (mpf), whether it has one argument"""
        p = self.p
        aptr, avar, acoef = nlp_terms_args(p)
        W, aW, E = [], [], []
        single = np.diff(aptr) == 1
        for k in range(len(p.fkind)):
            js = range(int(aptr[k]), int(aptr[k + 1]))
            prods = [_fr(acoef[j]) * _fr(x[int(avar[j]) - 1]) for j in js]
            b = _fr(p.fshift[k])
            ustar = sum(prods, Fraction(0)) + b
            du = (len(js) + 1) * U * (sum((abs(v) for v in prods), Fraction(0)) + abs(b))
            a = _fr(acoef[js[0]]) if single[k] else Fraction(1)
            kind, e = int(p.fkind[k]), int(p.fexp[k])
            par = float(p.fpar[k]) if kind == POWR else 0.0
            with mp.workdps(self.dps):
                K = [_fr(v) for v in kappa_exact(kind, e, par, _mpf(ustar))]
            Wk = [a ** q * K[q] for q in range(3)]
            Ek = [roundings(kind, e, q) * U * abs(Wk[q]) + abs(a ** q * K[q + 1]) * du for q in range(3)]
            W.append(Wk)
            with mp.workdps(25):
                aW.append([_mpf(abs(v)) for v in Wk]); E.append([_mpf(v) for v in Ek])
        return W, aW, E, single

    def want(self, x, sigma, lam, lay, blocks=None):
        p = self.p
        x = np.asarray(x, float)
        _, _, acoef = nlp_terms_args(p)
        W, aW, E, single = self.factors(x)
        fac_of = np.repeat(np.arange(len(p.fkind)), np.diff(nlp_terms_args(p)[0]))
        weight = lambda j: Fraction(1) if j < 0 or single[fac_of[j]] else _fr(acoef[j])
        mults = [_fr(sigma)] + [_fr(v) for v in (lam if lam is not None else np.zeros(p.m))]
        consts = dict(f=[_fr(p.f0)], g=[_fr(v) for v in p.g0])
        lo, hi = [None], [None]

        def seen(v):
            v = abs(v)
            if v:
                lo[0] = v if lo[0] is None or v < lo[0] else lo[0]
                hi[0] = v if hi[0] is None or v > hi[0] else hi[0]

        for Wk, kind, e in zip(W, p.fkind, p.fexp):
            for v in Wk:
                seen(v)
        self.exact, self.entry_kind, val, bnd = {}, {}, {}, {}
        u25 = mp.mpf(2) ** -53
        for key, entries in plans(p, lay).items():
            if key == "hval" and lam is None:
                continue
            ex, bd, kd = [], [], []
            for i, entry in enumerate(entries):
                c0 = consts[key][i] if key in consts else Fraction(0)
                total, S, B = c0, abs(c0), mp.mpf(0)
                kinds = set()
                for t, a, b, ja, jb, row in entry:
                    od = _orders(p, t, a, b)
                    prod = Fraction(1)
                    for k, q in od:
                        prod *= W[k][q]
                        seen(prod)
                        kinds.add(int(p.fkind[k]))
                    outer = _fr(p.tcoef[t]) * weight(ja) * weight(jb) * (mults[row] if key == "hval" else 1)
                    summand = prod * outer
                    seen(summand)
                    total += summand; S += abs(summand)
                    with mp.workdps(25):
                        inner = mp.mpf(0)
                        for k, q in od:
                            term = E[k][q]
                            for k2, q2 in od:
                                if k2 != k:
                                    term = term * aW[k2][q2]
                            inner += term
                        B += inner * _mpf(abs(outer)) + (len(od) + 4) * u25 * _mpf(abs(summand))
                seen(total)
                with mp.workdps(25):
                    B += (len(entry) + 2) * u25 * _mpf(S) if entry else mp.mpf(0)
                    bd.append(float(B))
                ex.append(total); kd.append(kinds.pop() if len(kinds) == 1 else -1)
            self.exact[key] = ex
            self.entry_kind[key] = np.array(kd, dtype=np.int64)
            val[key] = np.array([float(v) for v in ex]); bnd[key] = np.array(bd)
        val["f"], bnd["f"] = float(val["f"][0]), float(bnd["f"][0])
        if "hval" not in val:
            val["hval"], bnd["hval"] = None, None
        self.span = (lo[0], hi[0])
        return val, bnd

    def domain_ok(self):
        return self.span[0] >= DOMAIN[0] and self.span[1] <= DOMAIN[1]


def entry_ratios(got, val, bnd, exact=None):
    """{output: (err / (2 B + 2^-1074) per entry in doubles, the entries without a bound that differ from the exact value)}.
    err is |got - exact| in rationals where `exact` (NlpExact.exact) is given, else |got - val|."""
    out = {}
    for key in KEYS:
        if val.get(key) is None or got.get(key) is None:
            continue
        g_, b_ = (np.atleast_1d(np.asarray(a, float)) for a in (got[key], bnd[key]))
        ex = exact[key] if exact is not None else [_fr(v) for v in np.atleast_1d(np.asarray(val[key], float))]
        assert len(g_) == len(ex) == len(b_) and np.all(np.isfinite(g_)), key
        r = np.zeros(len(g_))
        for i in range(len(g_)):
            err = abs(_fr(g_[i]) - ex[i])
            if b_[i] == 0.0:
                r[i] = 0.0 if err == 0 else np.inf
            else:
                r[i] = float(err / (2 * _fr(b_[i]) + TINY))
        out[key] = r
    return out


def check_entries(got, val, bnd, exact=None, kinds=None, label=""):
    """|got - exact| <= 2 B + 2^-1074 for every entry; an entry with B = 0 (no summand, or exact ones only) must equal the
    exact value bit for bit.  Returns and prints the largest err / B per output, and per kind where `kinds`
    (NlpExact.entry_kind) is given."""
    ratios = entry_ratios(got, val, bnd, exact)
    worst = {key: float(2.0 * r.max()) if len(r) else 0.0 for key, r in ratios.items()}
    per_kind = {}
    if kinds is not None:
        for key, r in ratios.items():
            for kd in np.unique(kinds[key]):
                if kd >= 0:
                    per_kind[(KIND_NAMES[int(kd)], key)] = round(float(2.0 * r[kinds[key] == kd].max()), 3)
    print("err / B", label, {k: round(v, 3) for k, v in worst.items()})
    if per_kind:
        print("err / B per kind", label, per_kind)
    for key, r in ratios.items():
        bad = np.flatnonzero(r > 1.0)
        assert not len(bad), (label, key, bad[:8].tolist(), (2.0 * r[bad[:8]]).tolist())
    return worst, per_kind


# ---- the device's arithmetic in doubles
def mirror_eval(p: NlpTerms, x, sigma, lam, lay, kappa3=_kappa3, chain2=None, drop_second_weight=False, drop_last_of=0):
    """f, grad, g, jval, hval as nlp_eval files them, in numpy doubles: u in argument order with the shift last, kappa3 for
    the menu, a and a a folded into a one-argument factor, every summand c (prod (w_a w_b)) mult in factor order, the sums in
    plan order.  The mutations: chain2(a) in the place of a a; no weight for the second argument of a Hessian pair; the last
    summand of every entry of at least drop_last_of summands left out."""
    aptr, avar, acoef = nlp_terms_args(p)
    x = np.asarray(x, float)
    nf = len(p.fkind)
    single = np.diff(aptr) == 1
    fac_of = np.repeat(np.arange(nf), np.diff(aptr))
    W = np.zeros((nf, 3))
    for k in range(nf):
        js = range(int(aptr[k]), int(aptr[k + 1]))
        if single[k]:
            a = float(acoef[js[0]])
            u = a * x[avar[js[0]] - 1] + p.fshift[k]
        else:
            a, u = 1.0, 0.0
            for j in js:
                u += acoef[j] * x[avar[j] - 1]
            u += p.fshift[k]
        par = float(p.fpar[k]) if p.fkind[k] == POWR else 0.0
        k0, k1, k2 = (float(np.asarray(v).reshape(-1)[0]) for v in kappa3(int(p.fkind[k]), int(p.fexp[k]), par, np.array([u])))
        W[k] = k0, a * k1, (a * a if chain2 is None else chain2(a)) * k2
    weight = lambda j: 1.0 if single[fac_of[j]] else float(acoef[j])
    out = {}
    for key, entries in plans(p, lay).items():
        if key == "hval" and lam is None:
            out[key] = None
            continue
        vals = np.zeros(len(entries))
        for i, entry in enumerate(entries):
            s = float(p.f0) if key == "f" else float(p.g0[i]) if key == "g" else 0.0
            if drop_last_of and len(entry) >= drop_last_of:
                entry = entry[:-1]
            for t, a, b, ja, jb, row in entry:
                prod = 1.0
                for k, q in _orders(p, t, a, b):
                    prod *= W[k, q]
                w = 1.0
                if ja >= 0:
                    w = weight(ja) * (1.0 if jb < 0 or drop_second_weight else weight(jb)) if key == "hval" else weight(ja)
                term = p.tcoef[t] * (prod * w)
                if key == "hval":
                    term = term * (sigma if row == 0 else lam[row - 1])
                s += term
            vals[i] = s
        out[key] = vals
    out["f"] = float(out["f"][0])
    return out


# ---- the cases
@dataclasses.dataclass
class Case:
    p: NlpTerms
    lay: object
    x: np.ndarray
    sigma: float
    lam: np.ndarray


_ROWS = lambda m: dict(gL=np.full(m, -1e30), gU=np.full(m, 1e30))      # (a context refuses a row without any bound)
_PM = lambda vs: [s * v for v in vs for s in (1.0, -1.0)]
_LOGISTIC = _PM([2.0 ** -30, 1e-6, 1e-3, 0.5, 5.0, 36.7, 37.0, 40.0, 700.0])
MENU = {TANH: _PM([2.0 ** -30, 0.5, 2.0, 5.0, 10.0, 19.0, 19.0615, 20.0, 40.0, 300.0]),
        SIGMOID: _LOGISTIC, SOFTPLUS: _LOGISTIC,
        ATAN: _PM([2.0 ** -30, 0.5, 1.0, 3.0, 1e8, 1e100]),
        EXP: [-700.0, -30.0, 0.0, 0.5, 30.0, 700.0],
        LOG: [2.0 ** -500, 1e-8, 0.5, 1.0 - 2.0 ** -53, 1.0, 1.0 + 2.0 ** -52, 3.0, 2.0 ** 500],
        SQRT: [2.0 ** -600, 1e-8, 0.5, 3.0, 2.0 ** 600],
        SIN: [2.0 ** -30, 0.3, float(np.pi / 2), float(np.pi), 1e5, 1e15],
        COS: [2.0 ** -30, 0.3, float(np.pi / 2), float(np.pi), 1e5, 1e15]}
POW_E, POW_U = (1, 2, 3, 4, 31, 32, -1, -2, -3, -32), (-1.7, 0.3, 1e-5, 50.0)
POWR_P, POWR_U = (1e-3, 0.5, 1.0, 1.5, 2.0, -0.7, 17.3), (1e-8, 0.3, 1.0, 50.0, 1e10)
OLD_KINDS = (POW, SIN, COS, EXP, LOG)                           # what sqphip_nlp_attach and _attach_affine take
ALL_KINDS = (POW, SIN, COS, EXP, LOG, SQRT, TANH, ATAN, SIGMOID, SOFTPLUS, POWR)


def menu_groups(kinds=ALL_KINDS):
    """[(kind, e or p, [u, ...])]: the arguments a factor of one structure may sit at (POW: the arguments of one exponent,
    POWR: one argument list per exponent, the exponents rotating with the arguments in the data variant)"""
    out = []
    for kind in kinds:
        if kind == POW:
            out += [(POW, e, list(POW_U)) for e in POW_E]
        elif kind == POWR:
            out += [(POWR, p_, list(POWR_U)) for p_ in POWR_P]
        else:
            out.append((kind, 1, list(MENU[kind])))
    return out


def menu_pairs(kinds=ALL_KINDS, rot=0):
    """[(kind, e or p, u)]; rot: every pair takes the argument rot places on in its group (POWR: the exponent moves on as well)"""
    groups = menu_groups(kinds)
    real = [g[1] for g in groups if g[0] == POWR]
    out = []
    for kind, e, us in groups:
        if kind == POWR:
            e = real[(real.index(e) + rot) % len(real)]
        out += [(kind, e, us[(i + rot) % len(us)]) for i in range(len(us))]
    return out


_CHAINS = ((0.75, 4.0, -2.0), (-0.625, -8.0, -4.0), (-0.5, -4.0, -1.0))      # (a, x / u, b / u): a x + b = u exactly, by cancellation
_AFFINE = {2: (0.75, -0.5), 3: (0.75, -0.5, 0.625), 8: (0.75, -0.5, 0.625, -0.875, 0.5, -0.75, 0.375, 1.0)}


def _shift_for(target, coefs, xs):
    """the double nearest to target - sum a_j x_j (exact)"""
    return float(_fr(target) - sum((_fr(a) * _fr(v) for a, v in zip(coefs, xs)), Fraction(0)))


def _menu_case(pairs, variant, chains):
    """One row g_i = 1.0 kappa(u_i) and one objective term 1.0 kappa(u_i) per pair, on variables of its own; sigma = 1, lam = 1."""
    terms, x = [], []
    for i, (kind, e, u) in enumerate(pairs):
        if variant == "plain":
            fac = (len(x) + 1, kind, e, 1.0, 0.0)
            x.append(u)
        elif variant == "chain":
            a, xm, bm = chains[i % len(chains)]
            fac = (len(x) + 1, kind, e, a, bm * u)
            x.append(xm * u)
        else:
            cs = _AFFINE[(2, 3, 8)[i % 3]]
            xs = [u] * len(cs)
            fac = ([(len(x) + 1 + j, c) for j, c in enumerate(cs)], kind, e, _shift_for(u, cs, xs))
            x += xs
        terms += [(i + 1, 1.0, [fac]), (0, 1.0, [fac])]
    n, m = len(x), len(pairs)
    p = make_nlp_terms(n, m, 0, terms, x0=np.array(x), **_ROWS(m))
    return Case(p, nlp_terms_layout(p), np.array(x), 1.0, np.ones(m))


def menu_model(variant="plain", kinds=ALL_KINDS):
    """The menu at its edge arguments, one factor per row: g_i, J_ii, H_ii / 2 and grad_i are kappa, kappa', kappa'' of one
    factor.  plain: a = 1, b = 0, u = x; chain: a x + b = u by cancellation with a = 0.75 and -0.625; affine: 2, 3 and 8
    arguments; data: three Cases of one structure (sqphip_nlp_attach_data) whose coefficients, shifts and real exponents
    differ, every factor at another argument of its list in every instance."""
    if variant == "data":
        return [_menu_case(menu_pairs(kinds, rot=s), "chain", _CHAINS[s:s + 1]) for s in range(3)]
    return _menu_case(menu_pairs(kinds), variant, _CHAINS[:2])


def product_model(benign=False):
    """Terms of 2, 3 and exactly 8 factors at arguments of the menu, kinds mixed.  Term 1 has eight factors with variable 1 in
    every one: 8 + 2 * 28 = 64 summands in the Hessian slot (1, 1).  x tanh x and sigmoid(x) softplus(x) share a variable
    between two factors.  A Jacobian slot and a Hessian slot that no term feeds and a copy of a Hessian slot must stay 0.
    benign: the same structure at arguments of order 1, where the numpy reference is sound as well."""
    n = 20
    x = np.array([0.5, 1.25, -0.75, 2.0, 0.375, 1.5, -1.25, 0.625, 2.0, -5.0, -30.0, 50.0, 0.3, 1e8, 0.3, 1e5, 3.0, 30.0, 0.7, 1.1])
    if benign:
        x[9:18] = [-0.5, -1.0, 1.5, 0.3, 2.0, 0.3, 1.25, 3.0, 0.5]
    tg = (lambda hard, easy: easy) if benign else (lambda hard, easy: hard)

    def aff(vs, cs, kind, e, target):
        return (list(zip(vs, cs)), kind, e, _shift_for(target, cs, [x[v - 1] for v in vs]))

    eight = [aff(range(1, 9), [0.5, 0.25, 1.0, 0.5, 2.0, 0.5, 1.0, 0.25], SQRT, 1, 3.0),
             (1, TANH, 1, 4.0, tg(0.0, -1.5)),                                     # tanh at 2 (0.5)
             aff([1, 2], [1.0, -1.0], ATAN, 1, tg(3.0, 1.0)),
             aff([3, 1, 4], [-1.0, 0.5, 1.0], SIGMOID, 1, tg(-5.0, 0.5)),
             aff([5, 1], [0.5, -0.25], SOFTPLUS, 1, tg(5.0, 0.5)),
             aff([1, 6], [2.0, 0.5], POWR, 1.5, 0.3),
             aff([7, 1], [1.0, 0.5], POW, -3, tg(-1.7, 0.3)),
             aff([1, 8], [0.8, 1.0], LOG, 1, 3.0)]
    terms = [(1, 0.7, eight),
             (2, 0.9, [(9, POW), (9, TANH)]),                                      # x tanh x at 2
             (0, 1.3, [(10, SIGMOID), (10, SOFTPLUS)]),                            # sigmoid(x) softplus(x) at -5
             (2, -1.1, [(11, EXP), (12, POW, -3), (13, COS)]),                     # exp(-30) 50^-3 cos 0.3
             (0, 2.0, [(14, ATAN), (15, POWR, 17.3), (16, SIN)]),                  # atan 1e8, 0.3^17.3, sin 1e5
             (1, 0.4, [(17, LOG, 1, 1.0, tg(-2.0 + 2.0 ** -52, -1.0)), (18, EXP)]),   # log(1 + 2^-52) exp 30
             (0, 0.8, [(19, POW), (19, EXP, 1, -1.0, 0.0)]),                       # x exp(-x)
             (2, 0.6, [(aff([19, 20], [1.0, -1.0], POW, 1, 0.25)), (aff([19, 20], [1.0, 1.0], POW, 1, 1.0))])]
    p = make_nlp_terms(n, 2, 0, terms, g0=[0.4, -0.6], f0=0.25, x0=x, **_ROWS(2))
    lay = nlp_terms_layout(p)
    lay = dataclasses.replace(lay, jrow=np.append(lay.jrow, 2), jcol=np.append(lay.jcol, 3),
                              hrow=np.concatenate([lay.hrow, [20], lay.hrow[:1]]), hcol=np.concatenate([lay.hcol, [17], lay.hcol[:1]]))
    return Case(p, lay, x, 1.3, np.array([0.7, -1.9]))


STRIDE = 1025


def stride_model():
    """The smallest generated model past one stride of 1024 threads in every loop of nlp_eval: n = m = 1025, row i with one
    term of one (odd i) or two (even i) factors, on variables i and i + 1, and one objective term per variable; kinds and
    arguments cycle through the menu's arguments of order 1.  More than 1024 factors, terms, objective terms, Jacobian
    slots and Hessian slots; every output entry is non-zero."""
    n = STRIDE
    # (no exponent 1 and no log 1: their kappa'' or kappa is an exact 0)
    pool = [(k, e, u) for k, e, u in menu_pairs() if 0.25 <= abs(u) <= 5.0 and abs(e) <= 4 and not (k in (POW, POWR) and e == 1)
            and not (k == LOG and u == 1.0)]
    assert len({k for k, _, _ in pool}) == len(ALL_KINDS)
    x = np.array([pool[(7 * i) % len(pool)][2] for i in range(n)])
    own = lambda i: (i + 1,) + pool[(7 * i) % len(pool)][:2]                       # a plain factor on variable i at its own argument
    terms = []
    for i in range(n):
        facs = [own(i)]
        if i % 2 == 0:
            j = (i + 1) % n
            kind, e, u = pool[(11 * i + 3) % len(pool)]
            a, xm, bm = _CHAINS[i % 3]
            facs.append((j + 1, kind, e, float(u / x[j]), 0.0) if i % 4 else ([(j + 1, a), (i + 1, 0.5)], kind, e, _shift_for(u, [a, 0.5], [x[j], x[i]])))
        terms.append((i + 1, 0.5 + (i % 5) / 4.0, facs))
        terms.append((0, 1.0 - (i % 3) / 4.0, [own(i)]))
    p = make_nlp_terms(n, n, 0, terms, g0=np.linspace(-0.5, 0.5, n), f0=-0.75, x0=x, **_ROWS(n))
    rng = np.random.default_rng(1025)
    return Case(p, nlp_terms_layout(p), x, 0.7, rng.uniform(0.5, 1.5, n) * rng.choice([-1.0, 1.0], n))
