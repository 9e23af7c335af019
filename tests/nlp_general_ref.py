"""Test helper for variables shared across the factors of a term and the kinds SQRT .. POWR (sqphip_nlp_attach_general,
sqpsolver.jl_amd/nlp_terms.py):

    NlpGeneralRef       numpy evaluator of any NlpTerms, written from the ordered-pair form of the chain and product rule:
                        with F(v) the (factor, argument) couples of a term c prod_k kappa_k(u_k) on variable v,
                            d/dx_v       = c sum_{(a,j) in F(v)} a_j kappa'_a prod_{k != a} kappa_k
                            d2/dx_v dx_w = c sum_{(a,j) in F(v)} sum_{(b,l) in F(w)} a_j a_l
                                             [a = b ? kappa''_a prod_{k != a} kappa_k : kappa'_a kappa'_b prod_{k != a, b} kappa_k]
                        The Hessian is accumulated over every ordered pair of arguments into a dense symmetric matrix and read
                        at the lower COO entries (the first copy of a duplicated slot carries the value).  The logistic pair
                        through scipy.special.expit and np.logaddexp.  Independent of nlp_terms.factor_values.
    OracleGeneralTerms  an ora_nlp over NlpGeneralRef, so the oracle's SQP-TR runs on such a model
    general_edge_model  the hand-made model of the plan-edge test
    saturation_model    TANH / SIGMOID / SOFTPLUS factors pushed to u = +-40 and +-750 by their shifts
    GPU_*               the generated instances the GPU tests run and tests/test_nlp_general_cpu.py vouches for"""
from __future__ import annotations

import dataclasses

import numpy as np
from scipy.special import expit

from nlp_affine_ref import NlpAffineRef
from nlp_ref import OracleNlpTerms
from sqpsolver_jl_amd.nlp_terms import (ATAN, COS, EXP, LOG, POW, POWR, SIGMOID, SIN, SOFTPLUS, SQRT, TANH, NlpTerms,
                                        make_nlp_terms, nlp_general_synth, nlp_terms_args, nlp_terms_layout, nlp_terms_scenario)

# the generated problem of the GPU tests: nlp_general_synth(24, 14, GPU_SEED); batch tests run the scenarios GPU_SCENARIOS at
# the default noise, the queue test runs QUEUE_SCENARIOS at QUEUE_NOISE
GPU_SEED, GPU_SCENARIOS = 1, (0, 1, 2, 3)
QUEUE_SCENARIOS, QUEUE_NOISE = tuple(range(6)), 0.4
SQP_KW = dict(max_iter=30, literal_quirks=0, tol_infeas=1e-6, tol_residual=1e-4)
NEW_KINDS = (SQRT, TANH, ATAN, SIGMOID, SOFTPLUS, POWR)


def gpu_model():
    p = nlp_general_synth(24, 14, seed=GPU_SEED)
    return p, nlp_terms_layout(p)


def gpu_scenarios(p, which=GPU_SCENARIOS, noise=0.05):
    return [nlp_terms_scenario(p, s, GPU_SEED, noise) for s in which]


def kappa(kind, e, par, u):
    """kappa, kappa', kappa'' at u (e: integer exponent of POW, par: real exponent of POWR)"""
    u = float(u)
    if kind == SIN:
        return np.sin(u), np.cos(u), -np.sin(u)
    if kind == COS:
        return np.cos(u), -np.sin(u), -np.cos(u)
    if kind == EXP:
        return np.exp(u), np.exp(u), np.exp(u)
    if kind == LOG:
        return np.log(u), 1.0 / u, -1.0 / (u * u)
    if kind == POW:
        e = int(e)
        return u ** e, (1.0 if e == 1 else e * u ** (e - 1)), (0.0 if e == 1 else e * (e - 1) * (1.0 if e == 2 else u ** (e - 2)))
    if kind == SQRT:
        s = np.sqrt(u)
        return s, 1.0 / (2.0 * s), -1.0 / (4.0 * u * s)
    if kind == TANH:
        t = np.tanh(u)
        return t, 1.0 - t * t, -2.0 * t * (1.0 - t * t)
    if kind == ATAN:
        return np.arctan(u), 1.0 / (1.0 + u * u), -2.0 * u / (1.0 + u * u) ** 2
    if kind in (SIGMOID, SOFTPLUS):
        s, sc = float(expit(u)), float(expit(-u))                      # s and 1 - s
        if kind == SIGMOID:
            return s, s * sc, s * sc * (sc - s)
        return float(np.logaddexp(0.0, u)), s, s * sc
    assert kind == POWR
    v = u ** float(par)
    return v, par * v / u, par * (par - 1.0) * v / (u * u)


class NlpGeneralRef(NlpAffineRef):
    def __init__(self, p: NlpTerms):
        super().__init__(p)
        par = p.fpar if p.fpar is not None else np.zeros(len(p.fkind))
        self.par = [[float(par[k]) for k in range(int(p.tptr[t]), int(p.tptr[t + 1]))] for t in range(len(p.trow))]

    def _eval(self, x, t):
        with np.errstate(all="ignore"):
            return [kappa(fac[0], fac[1], par, self._u(x, fac)) for fac, par in zip(self.terms[t][1], self.par[t])]

    def hess(self, x, sigma, lam, hrow, hcol):
        p, n = self.p, self.p.n
        x = np.asarray(x, float)
        H = np.zeros((n, n))
        used = set()
        for t, (row, facs) in enumerate(self.terms):
            wt = p.tcoef[t] * (sigma if row == 0 else lam[row - 1])
            K = self._eval(x, t)
            args = [(a, v, av) for a, fac in enumerate(facs) for v, av in zip(fac[4], fac[5])]
            for a, v, av in args:                                       # every ordered pair of (factor, argument) couples
                for b, w, aw in args:
                    if a == b and facs[a][3]:
                        continue                                        # kappa'' = 0 in a plain linear factor: no entry
                    H[v, w] += wt * av * aw * self._prod(K, {a: 2} if a == b else {a: 1, b: 1})
                    used.add(max(v, w) * n + min(v, w))
        hr, hc = np.asarray(hrow, np.int64) - 1, np.asarray(hcol, np.int64) - 1
        hi, lo = np.maximum(hr, hc), np.minimum(hr, hc)
        first = {}
        for s, key in enumerate((hi * n + lo).tolist()):
            first.setdefault(key, s)
        assert used <= set(first), "entry not in the structure"
        out = np.zeros(len(hr))
        for key, s in first.items():
            if key in used:
                out[s] = H[key // n, key % n]
        return out

    def domain_margin(self, x):
        """min of u over the LOG, SQRT, POWR and negative-power factors (inf when there are none)"""
        x = np.asarray(x, float)
        us = [self._u(x, fac) for _, facs in self.terms for fac in facs
              if fac[0] in (LOG, SQRT, POWR) or (fac[0] == POW and fac[1] < 0)]
        return float(min(us)) if us else np.inf


class OracleGeneralTerms(OracleNlpTerms):
    def __init__(self, p: NlpTerms, lay=None):
        super().__init__(p, lay)
        self.ref = NlpGeneralRef(p)


def general_edge_model():
    """Plan edges.  Term 1 has exactly 8 factors with 8, 1, 2, 3, 2, 2, 2, 2 arguments, none plain linear, and variable 1 in
    every one of them: it files 8 + 2 * 28 = 64 entries into the Hessian slot (1, 1).  x log x through two one-argument
    factors, (x + y)(x - y) through two plain affine ones, every new kind once with one argument and once with several, POWR
    with 0.5, 1.5 and -0.7, variable 30 in the objective only, an odd value count, a Jacobian and a Hessian slot that no term
    needs and a copy of a Hessian slot."""
    A = lambda vs, cs: list(zip(vs, cs))
    eight = [(A(range(1, 9), [0.5, 0.25, 1.0, 0.5, 2.0, 0.5, 1.0, 0.25]), SQRT, 1, 0.3),      # exactly 8 arguments
             (1, TANH, 1, 0.7, -0.2),                                                          # exactly 1
             (A([1, 10], [1.0, -1.0]), ATAN, 1, 0.1),
             (A([12, 1, 14], [-1.0, 0.5, 1.0]), SIGMOID, 1, 0.3),
             (A([15, 1], [0.5, -0.25]), SOFTPLUS, 1, -0.2),
             (A([1, 18], [2.0, 0.5]), POWR, 0.5, 0.5),
             (A([19, 1], [1.0, 0.5]), POWR, 1.5, 0.4),
             (A([1, 2], [0.8, 1.0]), LOG, 1, 0.6)]
    terms = [(1, 0.7, eight),
             (0, 1.3, [(9, POW), (9, LOG)]),                                                   # x log x
             (2, 0.9, [(A([10, 11], [1.0, 1.0]), POW, 1, 0.0), (A([10, 11], [1.0, -1.0]), POW, 1, 0.0)]),      # (x + y)(x - y)
             (2, -1.1, [(20, SQRT, 1, 2.0, 0.1), (A([21, 22, 20], [1.0, -0.5, 0.3]), TANH, 1, 0.2)]),
             (2, 0.6, [(23, ATAN, 1, -1.5, 0.3), (23, SIGMOID, 1, 2.0, -0.4), (24, SOFTPLUS, 1, -1.0, 0.5)]),
             (0, 2.0, [(25, POWR, -0.7, 1.5, 0.2), (A([30, 25], [0.7, 0.2]), EXP, 1, 0.1)]),   # variable 30: objective only
             (0, 0.8, [(26, POW), (26, EXP, 1, -1.0, 0.0)]),                                   # x exp(-x)
             (1, 0.4, [(27, SIN), (27, COS), (A([27, 28], [1.0, 1.0]), POW, -1, 1.0)])]        # sin x cos x / (1 + x + y)
    n = 30
    p = make_nlp_terms(n, 2, 0, terms, g0=[0.4, -0.6], f0=0.25, xL=np.full(n, 0.2), xU=np.full(n, 3.0),
                       gL=[-5.0, -5.0], gU=[5.0, 5.0], x0=np.linspace(0.7, 1.3, n))
    assert (1 + p.m + len(p.trow)) % 2 == 1                   # an odd value count: the blocks are padded
    lay = nlp_terms_layout(p)
    lay = dataclasses.replace(lay, jrow=np.append(lay.jrow, 2), jcol=np.append(lay.jcol, 3),
                              hrow=np.concatenate([lay.hrow, [30], lay.hrow[:1]]), hcol=np.concatenate([lay.hcol, [29], lay.hcol[:1]]))
    return p, lay


SATURATION_SHIFTS = (40.0, -40.0, 750.0, -750.0)


def saturation_model():
    """Every TANH / SIGMOID / SOFTPLUS factor sits at u = +-40 or +-750 (+ an x of order 1) through its shift: once alone
    with one argument in a row, once with two arguments times a plain x in the objective."""
    n = 4
    terms = []
    for kind in (TANH, SIGMOID, SOFTPLUS):
        for b in SATURATION_SHIFTS:
            terms.append((1, 1.0, [(1, kind, 1, 0.5, b)]))
            terms.append((0, 0.5, [([(2, 1.0), (3, -0.5)], kind, 1, b), (4, POW)]))
    p = make_nlp_terms(n, 1, 0, terms, xL=np.full(n, 0.2), xU=np.full(n, 3.0), gL=[-1e4], gU=[1e4], x0=np.linspace(0.7, 1.3, n))
    return p, nlp_terms_layout(p)
