"""Test helper for factors with affine multi-variable arguments (sqphip_nlp_attach_affine, sqpsolver.jl_amd/nlp_terms.py):

    NlpAffineRef      numpy evaluator of an NlpTerms of either form, written term by term from the chain and product rule:
                      with v in factor a and w in factor b of a term c prod_k kappa_k(u_k), u_k = sum_j a_j x_j + b_k,
                          d/dx_v      = c a_v kappa'_a prod_{k != a} kappa_k
                          d2/dx_v dx_w = c a_v a_w kappa'_a kappa'_b prod_{others}      (a != b)
                          d2/dx_v dx_w = c a_v a_w kappa''_a prod_{k != a} kappa_k      (a = b, v = w included)
                      u is summed in argument order, the shift added last (include/sqphip.h).  f, grad f, g and the
                      Jacobian / Lagrangian-Hessian values at any 1-based COO structure: the first copy of a duplicated
                      slot carries the value, the other copies are 0.  Independent of nlp_terms.factor_values.
    OracleAffineTerms an ora_nlp over NlpAffineRef (OracleNlpTerms with the evaluator swapped: its callbacks read self.ref
                      at call time), so the oracle's SQP-TR runs on such a model
    affine_edge_model the hand-made model of the plan-edge test
    GPU_*             the generated instances the GPU tests run and tests/test_nlp_affine_cpu.py vouches for"""
from __future__ import annotations

import dataclasses

import numpy as np

from nlp_ref import OracleNlpTerms
from sqpsolver_jl_amd.nlp_terms import (COS, EXP, LOG, POW, SIN, NlpTerms, make_nlp_terms, nlp_affine_synth, nlp_terms_args,
                                        nlp_terms_layout, nlp_terms_scenario)

# the generated problem of the GPU tests: nlp_affine_synth(24, 14, GPU_SEED); batch and determinism tests run the scenarios
# GPU_SCENARIOS at the default noise, the queue test runs QUEUE_SCENARIOS at QUEUE_NOISE (iteration counts that differ)
GPU_SEED, GPU_SCENARIOS = 1, (0, 1, 2, 3)
QUEUE_SCENARIOS, QUEUE_NOISE = tuple(range(12)), 0.4
SQP_KW = dict(max_iter=30, literal_quirks=0, tol_infeas=1e-6, tol_residual=1e-4)


def gpu_model():
    p = nlp_affine_synth(24, 14, seed=GPU_SEED)
    return p, nlp_terms_layout(p)


def gpu_scenarios(p, which=GPU_SCENARIOS, noise=0.05):
    return [nlp_terms_scenario(p, s, GPU_SEED, noise) for s in which]


def _kappa(kind, e, u):
    """kappa, kappa', kappa'' at u"""
    if kind == SIN:
        return np.sin(u), np.cos(u), -np.sin(u)
    if kind == COS:
        return np.cos(u), -np.sin(u), -np.cos(u)
    if kind == EXP:
        return np.exp(u), np.exp(u), np.exp(u)
    if kind == LOG:
        return np.log(u), 1.0 / u, -1.0 / (u * u)
    assert kind == POW
    e = int(e)
    return float(u) ** e, (1.0 if e == 1 else e * float(u) ** (e - 1)), (0.0 if e == 1 else e * (e - 1) * (1.0 if e == 2 else float(u) ** (e - 2)))


class NlpAffineRef:
    def __init__(self, p: NlpTerms):
        self.p = p
        aptr, avar, acoef = nlp_terms_args(p)
        self.terms = []                     # (row, [(kind, e, shift, plain, [variables, 0-based], [coefficients]), ...])
        for t in range(len(p.trow)):
            facs = []
            for k in range(int(p.tptr[t]), int(p.tptr[t + 1])):
                js = range(int(aptr[k]), int(aptr[k + 1]))
                kind, e = int(p.fkind[k]), int(p.fexp[k]) if p.fkind[k] == POW else 1
                facs.append((kind, e, float(p.fshift[k]), kind == POW and e == 1, [int(avar[j]) - 1 for j in js], [float(acoef[j]) for j in js]))
            self.terms.append((int(p.trow[t]), facs))

    @staticmethod
    def _u(x, fac):
        u = 0.0
        for v, a in zip(fac[4], fac[5]):
            u = u + a * x[v]
        return u + fac[2]

    def _eval(self, x, t):
        """kappa, kappa', kappa'' of the factors of term t"""
        with np.errstate(all="ignore"):
            return [_kappa(fac[0], fac[1], self._u(x, fac)) for fac in self.terms[t][1]]

    @staticmethod
    def _prod(K, order):
        """prod_k K[k][order.get(k, 0)]"""
        out = 1.0
        for k, kv in enumerate(K):
            out = out * kv[order.get(k, 0)]
        return out

    def _values(self, x):
        x = np.asarray(x, float)
        return np.array([self.p.tcoef[t] * self._prod(self._eval(x, t), {}) for t in range(len(self.terms))])

    def f(self, x):
        tv = self._values(x)
        return float(self.p.f0 + np.sum(tv[self.p.trow == 0]))

    def g(self, x):
        p, tv = self.p, self._values(x)
        g = p.g0.copy()
        k = p.trow > 0
        np.add.at(g, p.trow[k] - 1, tv[k])
        return g

    def _first(self, x, objective):
        """(row, variable, value) of every first derivative of the objective's terms or of the rows' terms"""
        x = np.asarray(x, float)
        for t, (row, facs) in enumerate(self.terms):
            if (row == 0) != objective:
                continue
            K = self._eval(x, t)
            for a, fac in enumerate(facs):
                d = self.p.tcoef[t] * self._prod(K, {a: 1})
                for v, av in zip(fac[4], fac[5]):
                    yield row, v, d * av

    def grad(self, x):
        out = np.zeros(self.p.n)
        for _, v, val in self._first(x, True):
            out[v] += val
        return out

    @staticmethod
    def _scatter(nnz, entries, slot_keys):
        first = {}
        for s, key in enumerate(slot_keys):
            first.setdefault(int(key), s)
        out = np.zeros(nnz)
        for key, val in entries:
            assert key in first, "entry not in the structure"
            out[first[key]] += val
        return out

    def jac(self, x, jrow, jcol):
        n = self.p.n
        return self._scatter(len(jrow), [((row - 1) * n + v, val) for row, v, val in self._first(x, False)],
                             (np.asarray(jrow, np.int64) - 1) * n + np.asarray(jcol, np.int64) - 1)

    def hess(self, x, sigma, lam, hrow, hcol):
        p, n = self.p, self.p.n
        x = np.asarray(x, float)
        lo = lambda r, c: max(r, c) * n + min(r, c)
        entries = []
        for t, (row, facs) in enumerate(self.terms):
            wt = p.tcoef[t] * (sigma if row == 0 else lam[row - 1])
            K = self._eval(x, t)
            args = [(a, v, av) for a, fac in enumerate(facs) for v, av in zip(fac[4], fac[5])]
            for i, (a, v, av) in enumerate(args):
                for b, w, aw in args[:i + 1]:
                    if a == b:
                        if facs[a][3]:
                            continue                                   # kappa'' = 0: no entry
                        entries.append((lo(v, w), wt * av * aw * self._prod(K, {a: 2})))
                    else:
                        entries.append((lo(v, w), wt * av * aw * self._prod(K, {a: 1, b: 1})))
        hr, hc = np.asarray(hrow, np.int64) - 1, np.asarray(hcol, np.int64) - 1
        return self._scatter(len(hrow), entries, np.maximum(hr, hc) * n + np.minimum(hr, hc))

    def domain_margin(self, x):
        """min of u over the LOG and negative-power factors (inf when there are none)"""
        x = np.asarray(x, float)
        us = [self._u(x, fac) for _, facs in self.terms for fac in facs if fac[0] == LOG or (fac[0] == POW and fac[1] < 0)]
        return float(min(us)) if us else np.inf


class OracleAffineTerms(OracleNlpTerms):
    def __init__(self, p: NlpTerms, lay=None):
        super().__init__(p, lay)
        self.ref = NlpAffineRef(p)


def affine_edge_model():
    """Plan edges: a term of exactly 8 factors (one with exactly 8 arguments, one with 1; every kind, each kind at least once
    with two or more arguments), a one-factor term with 2 arguments, a plain linear factor with 3 arguments and a shift inside
    a product (no Hessian entries within the factor, cross entries present), variable 30 in the objective only, an odd value
    count, a Jacobian and a Hessian slot that no term needs and a copy of a Hessian slot."""
    A = lambda vs, cs: list(zip(vs, cs))
    eight = [(A(range(1, 9), [0.5, 0.25, 1.0, 0.5, 2.0, 0.5, 1.0, 0.25]), POW, -2, 0.3),      # exactly 8 arguments
             (9, POW, -1, 1.0, 0.2),                                                           # exactly 1
             (A([10, 11], [2.0, -1.0]), SIN, 1, 0.1),
             (A([12, 13, 14], [-1.0, 0.5, 1.0]), COS, 1, 0.3),
             (A([15, 16], [0.5, -0.25]), EXP, 1, -0.2),
             (A([17, 18], [2.0, 0.5]), LOG, 1, 0.5),
             (A([19, 20], [1.0, -0.5]), POW, 3, 0.4),
             (A([21, 22], [0.8, 1.0]), POW, 1, 0.0)]
    terms = [(1, 0.7, eight),
             (2, -1.3, [(A([23, 24], [1.5, -0.5]), SIN, 1, 0.2)]),                             # one factor, two arguments
             (2, 0.9, [(A([25, 26, 27], [1.0, -2.0, 0.5]), POW, 1, 0.35), (28, POW, 2), (A([1, 29], [1.0, 1.0]), EXP, 1, 0.0)]),
             (0, 2.0, [(A([30, 2], [0.7, 0.2]), EXP, 1, 0.1)]),                                # variable 30: objective only
             (0, 1.1, [(1, POW, 2), (A([9, 23], [1.0, 1.0]), POW, 1, -0.1)]),
             (1, 0.4, [(9, LOG, 1, 1.0, 0.5)])]
    n = 30
    p = make_nlp_terms(n, 2, 0, terms, g0=[0.4, -0.6], f0=0.25, xL=np.full(n, 0.2), xU=np.full(n, 3.0),
                       gL=[-5.0, -5.0], gU=[5.0, 5.0], x0=np.linspace(0.7, 1.3, n))
    assert (1 + p.m + len(p.trow)) % 2 == 1                   # an odd value count: the blocks are padded
    lay = nlp_terms_layout(p)
    lay = dataclasses.replace(lay, jrow=np.append(lay.jrow, 2), jcol=np.append(lay.jcol, 3),
                              hrow=np.concatenate([lay.hrow, [30], lay.hrow[:1]]), hcol=np.concatenate([lay.hcol, [29], lay.hcol[:1]]))
    return p, lay
