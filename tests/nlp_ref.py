"""Test helper for the factorable-NLP path (sqpsolver.jl_amd/nlp_terms.py, csrc/nlp_dev.hpp):

    NlpRef            numpy evaluator of an NlpTerms, written straight from the product rule: f, grad f, g, and the Jacobian /
                      Lagrangian-Hessian values at any 1-based COO structure (the first occurrence of a duplicated slot
                      carries the value, the others 0)
    OracleNlpTerms    an ora_nlp with ctypes callbacks over NlpRef, so that the oracle's SQP-TR (ora_sqp_tr_solve through
                      oracle.sqp_solve) runs on any NlpTerms without a C twin of the evaluator
    hs071_terms       Hock-Schittkowski 71 as terms, on the structure of oracle.problem_hs071()"""
from __future__ import annotations

import ctypes as C

import numpy as np

from oracle import oracle as O
from sqpsolver_jl_amd.nlp_terms import COS, EXP, LOG, MAX_FACTORS, POW, SIN, NlpTerms, make_nlp_terms, nlp_terms_layout


# the generated problem the GPU tests run (tests/test_gpu_nlp.py) and the CPU tests vouch for (tests/test_nlp_cpu.py: the
# oracle converges on every one of these instances and stays inside the domain of LOG and of the negative powers)
GPU_SEED, GPU_SCENARIOS = 5, (0, 1, 2, 3)


class NlpRef:
    def __init__(self, p: NlpTerms):
        self.p = p
        T = len(p.trow)
        self.cnt = np.diff(p.tptr)
        self.tf = np.repeat(np.arange(T), self.cnt)
        self.pos = np.arange(len(p.fvar)) - p.tptr[self.tf]
        self.V = self._pad(p.fvar, 0).astype(np.int64)
        self.plain = self._pad(((p.fkind == POW) & (p.fexp == 1)).astype(float), 1.0) > 0

    def _pad(self, vals, fill=1.0):
        M = np.full((len(self.p.trow), MAX_FACTORS), fill, dtype=np.float64)
        M[self.tf, self.pos] = vals
        return M

    def phis(self, x):
        """phi, phi', phi'' of every factor (chain factors a, a^2 included), padded to [nterms][8] with ones"""
        p = self.p
        a = p.fscale
        u = a * np.asarray(x, float)[p.fvar - 1] + p.fshift
        p0, p1, p2 = np.empty(len(u)), np.empty(len(u)), np.empty(len(u))
        with np.errstate(all="ignore"):
            k = p.fkind == SIN
            p0[k], p1[k], p2[k] = np.sin(u[k]), a[k] * np.cos(u[k]), -a[k] ** 2 * np.sin(u[k])
            k = p.fkind == COS
            p0[k], p1[k], p2[k] = np.cos(u[k]), -a[k] * np.sin(u[k]), -a[k] ** 2 * np.cos(u[k])
            k = p.fkind == EXP
            p0[k], p1[k], p2[k] = np.exp(u[k]), a[k] * np.exp(u[k]), a[k] ** 2 * np.exp(u[k])
            k = p.fkind == LOG
            p0[k], p1[k], p2[k] = np.log(u[k]), a[k] / u[k], -a[k] ** 2 / u[k] ** 2
            k = p.fkind == POW
            e = p.fexp[k].astype(float)
            p0[k] = u[k] ** e
            p1[k] = np.where(e == 1, 1.0, e * u[k] ** (e - 1)) * a[k]
            p2[k] = np.where((e == 1) | (e == 2), e * (e - 1), e * (e - 1) * u[k] ** (e - 2)) * a[k] ** 2
        return self._pad(p0), self._pad(p1), self._pad(p2)

    @staticmethod
    def _with(P0, a, Pa, b=None, Pb=None):
        M = P0.copy()
        M[:, a] = Pa[:, a]
        if b is not None:
            M[:, b] = Pb[:, b]
        return M.prod(axis=1)

    def f(self, x):
        p = self.p
        P0, _, _ = self.phis(x)
        return float(p.f0 + np.sum((p.tcoef * P0.prod(axis=1))[p.trow == 0]))

    def g(self, x):
        p = self.p
        P0, _, _ = self.phis(x)
        tv = p.tcoef * P0.prod(axis=1)
        g = p.g0.copy()
        k = p.trow > 0
        np.add.at(g, p.trow[k] - 1, tv[k])
        return g

    def grad(self, x):
        p = self.p
        P0, P1, _ = self.phis(x)
        out = np.zeros(p.n)
        for a in range(MAX_FACTORS):
            k = (p.trow == 0) & (self.cnt > a)
            np.add.at(out, self.V[k, a] - 1, (p.tcoef * self._with(P0, a, P1))[k])
        return out

    @staticmethod
    def _scatter(nnz, keys, slot_keys, vals):
        uniq, first = np.unique(slot_keys, return_index=True)
        out = np.zeros(nnz)
        if len(keys):
            pos = np.searchsorted(uniq, keys)
            assert np.all(pos < len(uniq)) and np.all(uniq[np.minimum(pos, len(uniq) - 1)] == keys), "entry not in the structure"
            np.add.at(out, first[pos], vals)
        return out

    def jac(self, x, jrow, jcol):
        p, n = self.p, self.p.n
        P0, P1, _ = self.phis(x)
        keys, vals = [np.zeros(0, np.int64)], [np.zeros(0)]
        for a in range(MAX_FACTORS):
            k = (p.trow > 0) & (self.cnt > a)
            keys.append((p.trow[k] - 1) * n + self.V[k, a] - 1)
            vals.append((p.tcoef * self._with(P0, a, P1))[k])
        return self._scatter(len(jrow), np.concatenate(keys), (np.asarray(jrow) - 1) * n + np.asarray(jcol) - 1, np.concatenate(vals))

    def hess(self, x, sigma, lam, hrow, hcol):
        p, n = self.p, self.p.n
        P0, P1, P2 = self.phis(x)
        wt = np.where(p.trow == 0, sigma, np.concatenate([[0.0], np.asarray(lam, float)])[p.trow]) * p.tcoef
        lo = lambda r, c: (np.maximum(r, c) - 1) * n + np.minimum(r, c) - 1
        keys, vals = [np.zeros(0, np.int64)], [np.zeros(0)]
        for b in range(MAX_FACTORS):
            k = (self.cnt > b) & ~self.plain[:, b]                      # phi'' of a plain linear factor is 0: no entry
            keys.append(lo(self.V[k, b], self.V[k, b])); vals.append((wt * self._with(P0, b, P2))[k])
            for a in range(b):
                k = self.cnt > b
                keys.append(lo(self.V[k, a], self.V[k, b])); vals.append((wt * self._with(P0, a, P1, b, P1))[k])
        return self._scatter(len(hrow), np.concatenate(keys), lo(np.asarray(hrow), np.asarray(hcol)), np.concatenate(vals))

    def dense_jac(self, x):
        p = self.p
        J = np.zeros((p.m, p.n))
        lay = nlp_terms_layout(p)
        J[lay.jrow - 1, lay.jcol - 1] = self.jac(x, lay.jrow, lay.jcol)
        return J

    def domain_margin(self, x):
        """min of a x + b over the LOG and negative-power factors (inf when there are none)"""
        p = self.p
        k = (p.fkind == LOG) | ((p.fkind == POW) & (p.fexp < 0))
        u = p.fscale * np.asarray(x, float)[p.fvar - 1] + p.fshift
        return float(u[k].min()) if k.any() else np.inf


def first_term(p: NlpTerms, need) -> int:
    """1-based number of the first term t for which need(row, variables, curved flags) holds"""
    for t in range(len(p.trow)):
        ks = slice(int(p.tptr[t]), int(p.tptr[t + 1]))
        if need(int(p.trow[t]), p.fvar[ks].tolist(), (~((p.fkind[ks] == POW) & (p.fexp[ks] == 1))).tolist()):
            return t + 1
    raise LookupError("no such term")


def hs071_terms() -> tuple[NlpTerms, "object"]:
    """min x1 x4 (x1 + x2 + x3) + x3  s.t.  x1 x2 x3 x4 >= 25,  x1^2 + x2^2 + x3^2 + x4^2 = 40,  1 <= x <= 5, as terms, and
    a layout with the full 8 + 10 entries of the oracle's problem."""
    P = O.problem_hs071()
    S = P.structure()
    lin = lambda j: (j, POW)
    terms = [(0, 1.0, [(1, POW, 2), lin(4)]), (0, 1.0, [lin(1), lin(2), lin(4)]), (0, 1.0, [lin(1), lin(3), lin(4)]), (0, 1.0, [lin(3)]),
             (1, 1.0, [lin(1), lin(2), lin(3), lin(4)])] + [(2, 1.0, [(j, POW, 2)]) for j in (1, 2, 3, 4)]
    p = make_nlp_terms(4, 2, int(S["num_linear"]), terms, xL=S["xL"], xU=S["xU"], gL=S["gL"], gU=S["gU"], x0=P.x0)
    lay = nlp_terms_layout(p)
    lay = type(lay)(4, 2, p.num_linear, S["jrow"].astype(np.int64), S["jcol"].astype(np.int64), S["hrow"].astype(np.int64),
                    S["hcol"].astype(np.int64), p.xL.copy(), p.xU.copy(), p.gL.copy(), p.gU.copy(), p.x0.copy())
    return p, lay


_F = C.CFUNCTYPE(C.c_double, C.c_void_p, C.POINTER(C.c_double))
_V2 = C.CFUNCTYPE(None, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double))
_H = C.CFUNCTYPE(None, C.c_void_p, C.POINTER(C.c_double), C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double))


class OracleNlpTerms:
    """Duck-types oracle.Problem (nlp, n, m, x0, structure(), eval_*) over NlpRef: oracle.sqp_solve(OracleNlpTerms(p, lay))
    runs the CPU oracle's SQP-TR on the terms.  The callbacks and arrays stay referenced by the object."""

    def __init__(self, p: NlpTerms, lay=None):
        lay = lay or nlp_terms_layout(p)
        self.p, self.ref, self.n, self.m = p, NlpRef(p), p.n, p.m
        self.x0 = np.asarray(lay.x0, float).copy()
        self._arr = [np.ascontiguousarray(a, dtype=np.int64) for a in (lay.jrow, lay.jcol, lay.hrow, lay.hcol)] + \
                    [np.ascontiguousarray(a, dtype=np.float64) for a in (lay.xL, lay.xU, lay.gL, lay.gU)]
        jr, jc, hr, hc, xL, xU, gL, gU = self._arr
        n, m = self.n, self.m
        X = lambda q: np.ctypeslib.as_array(q, shape=(n,)).copy()

        def ef(ud, x):
            return self.ref.f(X(x))

        def eg(ud, x, out):
            np.ctypeslib.as_array(out, shape=(n,))[:] = self.ref.grad(X(x))

        def eG(ud, x, out):
            if m:
                np.ctypeslib.as_array(out, shape=(m,))[:] = self.ref.g(X(x))

        def ej(ud, x, out):
            if len(jr):
                np.ctypeslib.as_array(out, shape=(len(jr),))[:] = self.ref.jac(X(x), jr, jc)

        def eh(ud, x, sigma, lam, out):
            if len(hr):
                lm = np.ctypeslib.as_array(lam, shape=(m,)).copy() if m else np.zeros(0)
                np.ctypeslib.as_array(out, shape=(len(hr),))[:] = self.ref.hess(X(x), sigma, lm, hr, hc)

        self._cb = [_F(ef), _V2(eg), _V2(eG), _V2(ej), _H(eh)]
        p64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))
        pd = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        vp = lambda f: C.cast(f, C.c_void_p)
        self._nlp = O.Nlp(n, m, lay.num_linear, len(jr), len(hr), p64(jr), p64(jc), p64(hr), p64(hc), pd(xL), pd(xU),
                          pd(gL), pd(gU), vp(self._cb[0]), vp(self._cb[1]), vp(self._cb[2]), vp(self._cb[3]),
                          vp(self._cb[4]) if len(hr) else None, None)
        self.nlp = C.pointer(self._nlp)

    def structure(self):
        jr, jc, hr, hc, xL, xU, gL, gU = self._arr
        return dict(n=self.n, m=self.m, num_linear=int(self._nlp.num_linear), jrow=jr.copy(), jcol=jc.copy(),
                    hrow=hr.copy(), hcol=hc.copy(), xL=xL.copy(), xU=xU.copy(), gL=gL.copy(), gU=gU.copy())

    def eval_f(self, x):
        return self.ref.f(np.asarray(x, float))

    def eval_grad_f(self, x):
        return self.ref.grad(np.asarray(x, float))

    def eval_g(self, x):
        return self.ref.g(np.asarray(x, float))

    def eval_jac_g(self, x):
        return self.ref.jac(np.asarray(x, float), self._arr[0], self._arr[1])

    def eval_h(self, x, sigma, lam):
        return self.ref.hess(np.asarray(x, float), sigma, np.asarray(lam, float), self._arr[2], self._arr[3])
