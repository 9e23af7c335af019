"""Test helper for the general QCQP path (sqpsolver.jl_amd/qcqp.py, csrc/qcqp_dev.hpp):

    QcqpRef        numpy evaluator of a Qcqp: f, grad f, g, and the Jacobian / Lagrangian-Hessian values at any 1-based COO
                   structure (the first occurrence of a duplicated slot carries the value, the others 0)
    extract        exact QCQP data of oracle Problems whose functions are quadratic (ACR, ACWR): c = grad f(0), f0 = f(0),
                   g0 = g(0), A = J(0), Q0 = H(0; 1, 0), Q_i = H(0; 0, e_i); one common term structure for a batch
    OracleQcqp     an ora_nlp with ctypes callbacks over QcqpRef, so that the oracle's SQP-TR (ora_sqp_tr_solve through
                   oracle.sqp_solve) runs on any Qcqp without a C twin of the evaluator"""
from __future__ import annotations

import ctypes as C

import numpy as np

from oracle import oracle as O
from sqpsolver_jl_amd.qcqp import Qcqp, qcqp_layout, qcqp_rows


class QcqpRef:
    def __init__(self, q: Qcqp):
        self.q = q
        self.off = q.q0r != q.q0c
        self.qoff = q.qr != q.qc

    def f(self, x):
        q = self.q
        w = np.where(self.off, 1.0, 0.5)
        return float(q.f0 + q.c @ x + np.sum(w * q.q0v * x[q.q0r - 1] * x[q.q0c - 1]))

    def grad(self, x):
        q = self.q
        g = q.c.copy()
        np.add.at(g, q.q0r - 1, q.q0v * x[q.q0c - 1])
        np.add.at(g, q.q0c[self.off] - 1, q.q0v[self.off] * x[q.q0r[self.off] - 1])
        return g

    def g(self, x):
        return qcqp_rows(self.q, x)

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
        q, n = self.q, self.q.n
        o = self.qoff
        keys = np.concatenate([(q.ar - 1) * n + q.ac - 1, (q.qi - 1) * n + q.qr - 1, (q.qi[o] - 1) * n + q.qc[o] - 1])
        vals = np.concatenate([q.av, q.qv * x[q.qc - 1], q.qv[o] * x[q.qr[o] - 1]])
        return self._scatter(len(jrow), keys, (np.asarray(jrow) - 1) * n + np.asarray(jcol) - 1, vals)

    def hess(self, sigma, lam, hrow, hcol):
        q, n = self.q, self.q.n
        lo = lambda r, c: (np.maximum(r, c) - 1) * n + np.minimum(r, c) - 1
        keys = np.concatenate([lo(q.q0r, q.q0c), lo(q.qr, q.qc)])
        vals = np.concatenate([sigma * q.q0v, np.asarray(lam)[q.qi - 1] * q.qv])
        return self._scatter(len(hrow), keys, lo(np.asarray(hrow), np.asarray(hcol)), vals)

    def dense_jac(self, x):
        q = self.q
        J = np.zeros((q.m, q.n))
        lay = qcqp_layout(q)
        J[lay.jrow - 1, lay.jcol - 1] = self.jac(x, lay.jrow, lay.jcol)
        return J


def coo_sum(vals, rows, cols, n, lower=False):
    """COO values summed over duplicated slots (the matrix gather_csc builds), on the sorted distinct entries: two
    evaluators that split a value differently between copies of one slot compare equal here."""
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    if lower:
        rows, cols = np.maximum(rows, cols), np.minimum(rows, cols)
    uniq, inv = np.unique((rows - 1) * n + cols - 1, return_inverse=True)
    out = np.zeros(len(uniq))
    np.add.at(out, inv, np.asarray(vals, dtype=np.float64))
    return out


def extract(problems, num_linear=None):
    """Qcqp data of one oracle Problem or of a list of them sharing one structure (a batch of scenarios): every list gets
    the same terms -- those non-zero in any of the problems -- and its own values.  Candidate Q_i terms are the Hessian
    slots whose two variables both appear in row i of the Jacobian structure; rows 1..num_linear carry none."""
    single = not isinstance(problems, (list, tuple))
    probs = [problems] if single else list(problems)
    S = probs[0].structure()
    n, m = S["n"], S["m"]
    nlin = S["num_linear"] if num_linear is None else num_linear
    jr, jc, hr, hc = (np.asarray(S[k], dtype=np.int64) for k in ("jrow", "jcol", "hrow", "hcol"))
    z = np.zeros(n)
    rows_of = [set() for _ in range(n)]                # variable -> rows whose Jacobian structure holds it
    for i, j in zip(jr, jc):
        rows_of[j - 1].add(int(i) - 1)
    cand = [[] for _ in range(m)]
    for k in range(len(hr)):
        for i in sorted(rows_of[hr[k] - 1] & rows_of[hc[k] - 1]):
            if i >= nlin:
                cand[i].append(k)
    # rows whose candidate slots are disjoint are read off one Hessian evaluation: a slot only ever holds terms of rows
    # whose Jacobian structure has both its variables, so the other rows of a group add exact zeros there
    groups, used = [], []
    for i in range(m):
        if not cand[i]:
            continue
        ci = set(cand[i])
        for g, u in zip(groups, used):
            if not (u & ci):
                g.append(i); u |= ci
                break
        else:
            groups.append([i]); used.append(set(ci))
    per = []
    for P in probs:
        Jv = P.eval_jac_g(z)
        H0 = P.eval_h(z, 1.0, np.zeros(m))
        Hi = [np.zeros(0)] * m
        for rows in groups:                            # H(0; 0, sum of e_i over rows that share no candidate slot)
            e = np.zeros(m); e[rows] = 1.0
            h = P.eval_h(z, 0.0, e)
            for i in rows:
                Hi[i] = h[cand[i]]
        per.append((P.eval_f(z), P.eval_grad_f(z), P.eval_g(z), Jv, H0, Hi))
    keepA = np.any([p[3] != 0 for p in per], axis=0)
    keep0 = np.any([p[4] != 0 for p in per], axis=0)
    keepQ = [np.any([p[5][i] != 0 for p in per], axis=0) if cand[i] else np.zeros(0, bool) for i in range(m)]
    qi = np.concatenate([np.full(int(keepQ[i].sum()), i + 1) for i in range(m)] + [np.zeros(0)]).astype(np.int64)
    qk = np.concatenate([np.asarray(cand[i], dtype=np.int64)[keepQ[i]] for i in range(m)] + [np.zeros(0, np.int64)])
    out = []
    for P, (f0, c, g0, Jv, H0, Hi) in zip(probs, per):
        S = P.structure()
        qv = np.concatenate([Hi[i][keepQ[i]] for i in range(m)] + [np.zeros(0)])
        out.append(Qcqp(n, m, nlin, hr[keep0].copy(), hc[keep0].copy(), H0[keep0].copy(), jr[keepA].copy(), jc[keepA].copy(),
                        Jv[keepA].copy(), qi, hr[qk].copy(), hc[qk].copy(), qv, np.asarray(c, float).copy(),
                        np.asarray(g0, float).copy(), float(f0), S["xL"].astype(float), S["xU"].astype(float),
                        S["gL"].astype(float), S["gU"].astype(float), np.asarray(P.x0, float).copy()))
    return out[0] if single else out


_F = C.CFUNCTYPE(C.c_double, C.c_void_p, C.POINTER(C.c_double))
_V2 = C.CFUNCTYPE(None, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double))
_H = C.CFUNCTYPE(None, C.c_void_p, C.POINTER(C.c_double), C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double))


class OracleQcqp:
    """Duck-types oracle.Problem (nlp, n, m, x0, structure(), eval_*) over QcqpRef: oracle.sqp_solve(OracleQcqp(q, lay))
    runs the CPU oracle's SQP-TR on the QCQP.  The callbacks and arrays stay referenced by the object."""

    def __init__(self, q: Qcqp, lay=None):
        lay = lay or qcqp_layout(q)
        self.q, self.ref, self.n, self.m = q, QcqpRef(q), q.n, q.m
        self.x0 = np.asarray(lay.x0, float).copy()
        self._arr = [np.ascontiguousarray(a, dtype=np.int64) for a in (lay.jrow, lay.jcol, lay.hrow, lay.hcol)] + \
                    [np.ascontiguousarray(a, dtype=np.float64) for a in (lay.xL, lay.xU, lay.gL, lay.gU)]
        jr, jc, hr, hc, xL, xU, gL, gU = self._arr
        n, m = self.n, self.m
        X = lambda p: np.ctypeslib.as_array(p, shape=(n,))

        def ef(ud, x):
            return self.ref.f(X(x).copy())

        def eg(ud, x, out):
            np.ctypeslib.as_array(out, shape=(n,))[:] = self.ref.grad(X(x).copy())

        def eG(ud, x, out):
            if m:
                np.ctypeslib.as_array(out, shape=(m,))[:] = self.ref.g(X(x).copy())

        def ej(ud, x, out):
            if len(jr):
                np.ctypeslib.as_array(out, shape=(len(jr),))[:] = self.ref.jac(X(x).copy(), jr, jc)

        def eh(ud, x, sigma, lam, out):
            if len(hr):
                lm = np.ctypeslib.as_array(lam, shape=(m,)).copy() if m else np.zeros(0)
                np.ctypeslib.as_array(out, shape=(len(hr),))[:] = self.ref.hess(sigma, lm, hr, hc)

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
        return self.ref.hess(sigma, np.asarray(lam, float), self._arr[2], self._arr[3])
