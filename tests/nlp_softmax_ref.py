"""Test helper for the multinomial (softmax) data blocks of a factorable NLP (sqpsolver.jl_amd/nlp_terms.py NlpSoftmaxBlock,
csrc/nlp_softmax_dev.hpp):

    softmax_reference   f, grad and Hessian of one softmax block at 50 digits -- the logits exact (integers on the 2^-400 grid),
                        log-sum-exp and the probabilities in mpmath, the sums over the points in exact integer arithmetic on
                        2^-200 grids -- and the first-order forward error bound B of every output entry (below)
    NlpSoftmaxRef       the five outputs of a problem with scalar and softmax blocks: NlpGeneralRef for the terms,
                        nlp_block_ref.block_reference for the scalar blocks, softmax_reference for the softmax blocks
    NlpSoftmaxNumpy     the same outputs in plain numpy (nlp_terms.block_eval): what the oracle's callbacks evaluate
    OracleSoftmaxTerms  oracle.sqp_solve on a problem with such blocks
    the cases of tests/test_gpu_nlp_softmax.py, which tests/test_nlp_softmax_cpu.py vouches for

The bound.  U = 2^-53.  For point i let r_ik = sum_j |A_ij x_{col[k][j]}| + |S_ki| and E_i = (d + 2) U max_k r_ik: a logit
computed by d fused multiply-adds and one addition is off by at most (d + 1) U r_ik to first order, (d + 2) leaves one ulp for
the operand handed on.  Carried through the softmax's own derivatives:
    lse_i = log sum_k exp(u_ik) moves by at most max_k |du_ik| <= E_i (its gradient is a probability vector), and so does
          u_{i, y_i}: the value W_i (lse_i - u_{i, y_i}) moves by at most 2 |W_i| E_i;
    p_ik  moves by p_ik |du_ik - sum_l p_il du_il| <= 2 E_i p_ik: relative to p_ik, twice the largest logit error.
The arithmetic behind the logits -- the subtraction of the maximum, one exp per class, the class sum of K terms, the log or the
divide -- costs at most K + 8 ulp relative to s = sum_k exp(u_ik - m) and to each p_ik: a = (K + 8) U.  On lse this is
a (1 + |lse_i|): a relative to s is a absolute on log s, and the roundings of log s, of m + log s and of the subtraction of
u_{i, y_i} are ulps of numbers no larger than |lse_i| + r.  The sums over the points are recursive sums of N terms in some
order plus a few roundings of the summand's own products, (N + 8) U sum_i |summand_i|.  So
    B_f    = (N + 8) U sum_i |W_i (lse_i - u_{i, y_i})| + sum_i |W_i| (2 E_i + a (1 + |lse_i|))
    B_g,q  = (N + 8) U sum_i |W_i (p_ik - [y_i = k]) A_ij| + sum_i |W_i| p_ik (2 E_i + a) |A_ij|
    B_H,qq' = |sigma| sum_i h_i ((N + 8) U + 4 E_i + 2 a),   h_i = |W_i| p_ik ([k = l] + p_il) |A_ij| |A_ij'|
The Hessian's summand is bounded by h_i, not by |W_i p_ik ([k = l] - p_il)| |A_ij A_ij'|: the device (and numpy) form the
[k = l] part and the p_ik p_il part as separate sums, so 1 - p_il is never formed and its cancellation is paid for; both
parts move by at most (4 E_i + 2 a) relative to themselves (two probabilities each at most).
The acceptance rule is the project's, nlp_block_ref.check_outputs: |got - want| <= 4 B + 1e-13 max |want|."""
from __future__ import annotations

import dataclasses

import mpmath as mp
import numpy as np

from nlp_block_ref import DPS, SQP_TIGHT, U, _SHIFT, _first_slots, _int, _ints, block_reference, check_outputs   # noqa: F401
from nlp_general_ref import NlpGeneralRef, OracleGeneralTerms
from sqpsolver_jl_amd.nlp_terms import (EXP, POW, SOFTPLUS, NlpBlock, NlpSoftmaxBlock, NlpTerms, block_eval, fold_weights,
                                        make_nlp_terms, multinomial_block_model, nlp_terms_layout)


def softmax_reference(b: NlpSoftmaxBlock, x, sigma):
    """(f, grad [Kf d], H [Kf d, Kf d]) of one softmax block at 50 digits, rounded to doubles, and their bounds
    (Bf, Bg [Kf d], BH [Kf d, Kf d]); the Hessian and its bound carry sigma.  Flat index k d + j, the block's own order."""
    x = np.asarray(x, float)
    N, d = b.A.shape
    Kf, K = b.Kf, b.K
    with mp.workdps(DPS):
        Ai = _ints(b.A)
        one = mp.mpf(2) ** (2 * _SHIFT)
        ui = [Ai.dot(_ints(x[b.cols[k] - 1])) + _ints(b.shift[k]) * (1 << _SHIFT) for k in range(Kf)]      # u 2^400, exact
        lse = np.empty(N, dtype=object)
        uy = np.empty(N, dtype=object)
        P = np.empty((Kf, N), dtype=object)
        for i in range(N):
            u = [mp.mpf(int(ui[k][i])) / one for k in range(Kf)] + ([mp.mpf(0)] if b.pinned else [])
            m = max(u)
            e = [mp.exp(v - m) for v in u]
            s = mp.fsum(e)
            lse[i] = m + mp.log(s)
            uy[i] = u[int(b.labels[i])]
            for k in range(Kf):
                P[k, i] = e[k] / s
        w = [mp.mpf(v) for v in b.weight]
        back = lambda v, p: np.array([float(mp.mpf(int(t)) / mp.mpf(2) ** (p * _SHIFT)) for t in np.ravel(v)]).reshape(np.shape(v))
        f = float(back(sum(_int(w[i] * (lse[i] - uy[i])) for i in range(N)), 1))
        g = np.zeros(Kf * d)
        H = np.zeros((Kf * d, Kf * d))
        for k in range(Kf):
            z1 = np.array([_int(w[i] * (P[k, i] - (1 if b.labels[i] == k else 0))) for i in range(N)], dtype=object)
            g[k * d:(k + 1) * d] = back(Ai.T.dot(z1), 2)
            for l in range(k + 1):
                z2 = np.array([_int(w[i] * P[k, i] * ((1 if k == l else 0) - P[l, i])) for i in range(N)], dtype=object)
                blk = float(sigma) * back(Ai.T.dot(z2[:, None] * Ai), 3)
                H[k * d:(k + 1) * d, l * d:(l + 1) * d] = blk
                H[l * d:(l + 1) * d, k * d:(k + 1) * d] = blk.T
        Pf = np.array([[float(t) for t in row] for row in P]).reshape(Kf, N)
        lsef = np.array([float(t) for t in lse])
        fi = np.array([float(lse[i] - uy[i]) for i in range(N)])
    aA, aW = np.abs(b.A), np.abs(b.weight)
    r = np.stack([aA @ np.abs(x[b.cols[k] - 1]) + np.abs(b.shift[k]) for k in range(Kf)])      # [Kf, N]
    E = (d + 2) * U * r.max(axis=0)
    a = (K + 8) * U
    Y = (b.labels[None, :] == np.arange(Kf)[:, None]).astype(float)
    Bf = (N + 8) * U * float(aW @ np.abs(fi)) + float(aW @ (2.0 * E + a * (1.0 + np.abs(lsef))))
    Bg = np.concatenate([(N + 8) * U * (aA.T @ (aW * np.abs(Pf[k] - Y[k]))) + aA.T @ (aW * Pf[k] * (2.0 * E + a)) for k in range(Kf)])
    BH = np.zeros((Kf * d, Kf * d))
    rel = (N + 8) * U + 4.0 * E + 2.0 * a
    for k in range(Kf):
        for l in range(Kf):
            h = aW * Pf[k] * ((1.0 if k == l else 0.0) + Pf[l])
            BH[k * d:(k + 1) * d, l * d:(l + 1) * d] = abs(float(sigma)) * (aA.T @ ((h * rel)[:, None] * aA))
    return (f, g, H), (Bf, Bg, BH)


def _is_softmax(b):
    return isinstance(b, NlpSoftmaxBlock)


class NlpSoftmaxRef:
    """want(x, sigma, lam, lay) -> (values, bounds) of f, grad, g, jval, hval: terms by NlpGeneralRef, blocks at 50 digits."""

    def __init__(self, p: NlpTerms):
        self.p, self.terms = p, NlpGeneralRef(dataclasses.replace(p, blocks=[]))

    def want(self, x, sigma, lam, lay, blocks=None):
        p, T = self.p, self.terms
        val = dict(f=T.f(x), grad=T.grad(x), g=T.g(x), jval=T.jac(x, lay.jrow, lay.jcol), hval=T.hess(x, sigma, lam, lay.hrow, lay.hcol))
        bnd = dict(f=0.0, grad=np.zeros(p.n), g=np.zeros(p.m), jval=np.zeros(len(lay.jrow)), hval=np.zeros(len(lay.hrow)))
        first = _first_slots(lay)
        for b in (p.blocks if blocks is None else blocks):
            (f, g, H), (Bf, Bg, BH) = (softmax_reference if _is_softmax(b) else block_reference)(b, x, sigma)
            c = np.ravel(b.cols) - 1
            val["f"] += f; bnd["f"] += Bf
            np.add.at(val["grad"], c, g); np.add.at(bnd["grad"], c, Bg)
            for r in range(len(c)):
                for q in range(r + 1):
                    s = first[max(c[r], c[q]) * p.n + min(c[r], c[q])]
                    val["hval"][s] += H[r, q]; bnd["hval"][s] += BH[r, q]
        return val, bnd


class NlpSoftmaxNumpy:
    """f, grad, g, jac, hess of a problem with blocks of either sort in plain numpy (the interface of NlpRef)."""

    def __init__(self, p: NlpTerms):
        self.p, self.terms = p, NlpGeneralRef(dataclasses.replace(p, blocks=[]))

    def f(self, x):
        return self.terms.f(x) + block_eval(self.p, x)[0]

    def grad(self, x):
        return self.terms.grad(x) + block_eval(self.p, x)[1]

    def g(self, x):
        return self.terms.g(x)

    def jac(self, x, jrow, jcol):
        return self.terms.jac(x, jrow, jcol)

    def hess(self, x, sigma, lam, hrow, hcol):
        p = self.p
        out = self.terms.hess(x, sigma, lam, hrow, hcol)
        H = sigma * block_eval(p, x)[2]
        first = _first_slots(type("L", (), dict(n=p.n, hrow=hrow, hcol=hcol)))
        pairs = {(max(r, q), min(r, q)) for b in p.blocks for r in (np.ravel(b.cols) - 1).tolist() for q in (np.ravel(b.cols) - 1).tolist()}
        for r, q in pairs:
            out[first[r * p.n + q]] += H[r, q]
        return out

    def outputs(self, x, sigma, lam, lay):
        return dict(f=self.f(x), grad=self.grad(x), g=self.g(x), jval=self.jac(x, lay.jrow, lay.jcol),
                    hval=self.hess(x, sigma, lam, lay.hrow, lay.hcol))


class OracleSoftmaxTerms(OracleGeneralTerms):
    def __init__(self, p: NlpTerms, lay=None):
        lay = lay or nlp_terms_layout(p)
        super().__init__(dataclasses.replace(p, blocks=[]), lay)
        self.p, self.ref = p, NlpSoftmaxNumpy(p)


# ---- the cases of the GPU tests
# (N, d, K, pinned): one variable; tile and class boundaries -- class = tile, a class boundary mid-tile with a remainder tile,
# six classes across two tiles, 117 columns, 128 columns twice; past one thread stride
EDGE_CASES = [(1, 1, 2, 1), (3, 2, 3, 0), (4, 16, 2, 0), (5, 17, 2, 0), (65, 5, 7, 1), (63, 9, 14, 1), (64, 8, 16, 0), (130, 64, 2, 0),
              (1027, 3, 5, 0)]
BIG_LOGITS = (65, 5, 7, 1)                   # the case whose instances carry offsets of +-800 on a few points


def with_block(p, k, **kw):
    """p with other data in block k"""
    return dataclasses.replace(p, blocks=p.blocks[:k] + [dataclasses.replace(p.blocks[k], **kw)] + p.blocks[k + 1:])


def edge_data(N, d, K, pinned, big=False):
    """A [N, d], labels [N], three (weight [N], offsets [Kf, N]) pairs: weights with zeros and a negative one where N allows;
    big: offsets of +-800 on a few points of every instance."""
    rng = np.random.default_rng([N, d, K, pinned, 3])
    Kf = K - 1 if pinned else K
    A = rng.standard_normal((N, d)) / np.sqrt(d)
    y = rng.integers(0, K, N).astype(np.int32)
    inst = []
    for b in range(3):
        w = rng.uniform(0.5, 1.5, N)
        w[b::5] = 0.0
        w[(b + 1) % N] = -0.7
        s = 0.3 * rng.standard_normal((Kf, N))
        if big:
            for t, i in enumerate(range(3 + b, N, 11)):
                s[(t + b) % Kf, i] = 800.0 if t % 2 == 0 else -800.0
        inst.append((w, s))
    return A, y, inst


def edge_model(N, d, K, pinned, big=False):
    """One softmax block on an unsorted, non-contiguous choice of Kf d of n = Kf d + 5 variables, a ridge term on every
    variable (the block's diagonal slots are shared with terms), a cross term, one linear row; the Hessian COO carries two
    duplicated slots.  Returns (p, lay, [(weight, offsets)] * 3)."""
    Kf = K - 1 if pinned else K
    D = Kf * d
    n = D + 5
    rng = np.random.default_rng([N, d, K, 7])
    cols = (rng.permutation(n)[:D] + 1).reshape(Kf, d)
    A, y, inst = edge_data(N, d, K, pinned, big)
    terms = [(0, 0.3 + 0.1 * (j % 3), [(j + 1, POW, 2, 1.0, -0.2)]) for j in range(n)]
    terms += [(0, 0.5, [(int(cols[0, 0]), POW), (n, EXP, 1, 0.5, 0.0)]), (1, 1.0, [(1, POW)]), (1, -1.0, [(n, POW)])]
    blk = NlpSoftmaxBlock(cols, A, y, K, bool(pinned), inst[0][1], inst[0][0])
    p = make_nlp_terms(n, 1, 1, terms, f0=0.25, xL=np.full(n, 0.5), xU=np.full(n, 1.5), gL=[-1.0], gU=[1.0],
                       x0=np.linspace(0.7, 1.3, n), blocks=[blk])
    lay = nlp_terms_layout(p)
    lay = dataclasses.replace(lay, hrow=np.concatenate([lay.hrow, lay.hrow[:2]]), hcol=np.concatenate([lay.hcol, lay.hcol[:2]]))
    return p, lay, inst


def edge_point(p, N, d):
    """where the edge tests evaluate: (x, sigma, lam)"""
    rng = np.random.default_rng(N + d)
    return rng.uniform(0.6, 1.4, p.n), 0.7, np.array([0.8])


def mixed_model(softmax_first):
    """One scalar (softplus) block and one softmax block (K = 3, unpinned, d = 3) on overlapping columns -- variables 3, 5, 7
    in both -- in either block order."""
    n = 14
    rng = np.random.default_rng(12)
    c0 = np.array([7, 3, 1, 5, 9, 10, 2])
    c1 = np.array([[5, 12, 3], [7, 4, 14], [13, 6, 8]])
    b0 = NlpBlock(SOFTPLUS, c0, rng.standard_normal((37, 7)) / 2, 0.2 * rng.standard_normal(37), rng.uniform(0.0, 2.0, 37))
    b1 = NlpSoftmaxBlock(c1, rng.standard_normal((22, 3)), rng.integers(0, 3, 22), 3, False, 0.2 * rng.standard_normal((3, 22)),
                         rng.uniform(0.5, 1.0, 22))
    terms = [(0, 0.4, [(j + 1, POW, 2)]) for j in range(n)]
    p = make_nlp_terms(n, 0, 0, terms, xL=np.full(n, -3.0), xU=np.full(n, 3.0), x0=np.linspace(-0.5, 0.5, n),
                       blocks=[b1, b0] if softmax_first else [b0, b1])
    return p, nlp_terms_layout(p)


def folds_case3(K=3):
    """N = 150, d = 6, reg = 0.5 from default_rng(31): an intercept plus five normal features, labels the argmax of
    X B + 0.8 Gumbel over K classes; the four fold weight vectors.  (X, y, reg, W [4, 150])"""
    rng = np.random.default_rng(31)
    X = np.column_stack([np.ones(150), rng.standard_normal((150, 5))])
    B = rng.standard_normal((6, K))
    y = np.argmax(X @ B + 0.8 * rng.gumbel(size=(150, K)), axis=1).astype(np.int32)
    return X, y, 0.5, fold_weights(150, 4)


def newton_multinomial(X, y, K, reg, w, pinned):
    """argmin sum_i w_i [lse(X_i'b) - X_i'b_{y_i}] + reg / 2 |b|^2 over b [Kf, d] (class-major, flat) by Newton's method;
    (b, iterations, smallest Hessian eigenvalue at the optimum)"""
    N, d = X.shape
    Kf = K - 1 if pinned else K
    b = np.zeros(Kf * d)
    Y = (np.asarray(y)[None, :] == np.arange(Kf)[:, None]).astype(float)
    for it in range(1, 60):
        u = b.reshape(Kf, d) @ X.T
        if pinned:
            u = np.vstack([u, np.zeros(N)])
        e = np.exp(u - u.max(axis=0))
        P = (e / e.sum(axis=0))[:Kf]
        g = ((w * (P - Y)) @ X).ravel() + reg * b
        H = reg * np.eye(Kf * d)
        for k in range(Kf):
            for l in range(Kf):
                H[k * d:(k + 1) * d, l * d:(l + 1) * d] += X.T @ ((w * P[k] * ((k == l) - P[l]))[:, None] * X)
        step = np.linalg.solve(H, g)
        b = b - step
        if np.abs(step).max() < 1e-13:
            return b, it, float(np.linalg.eigvalsh(H).min())
    raise RuntimeError("Newton did not converge")


def rows_case():
    """A softmax block (N = 40, d = 3, K = 3 pinned: six variables, three offset sets) under the linear row sum x = 0.6 and the
    quadratic row |x|^2 <= 0.2 of ordinary terms, -0.05 <= x <= 0.3: bounds active at the optimum.  (p, lay, [offsets] * 3)"""
    rng = np.random.default_rng(34)
    X = np.column_stack([np.ones(40), rng.standard_normal((40, 2))])
    y = np.argmax(X @ rng.standard_normal((3, 3)) + 0.8 * rng.gumbel(size=(40, 3)), axis=1)
    shifts = [0.5 * rng.standard_normal((2, 40)) for _ in range(3)]
    n = 6
    terms = [(0, 0.05, [(j + 1, POW, 2)]) for j in range(n)] + [(1, 1.0, [(j + 1, POW)]) for j in range(n)] + \
            [(2, 1.0, [(j + 1, POW, 2)]) for j in range(n)]
    blk = NlpSoftmaxBlock(np.arange(1, n + 1).reshape(2, 3), X, y, 3, True, shifts[0], None)
    p = make_nlp_terms(n, 2, 1, terms, xL=np.full(n, -0.05), xU=np.full(n, 0.3), gL=[0.6, -np.inf], gU=[0.6, 0.2],
                       x0=np.full(n, 0.1), blocks=[blk])
    return p, nlp_terms_layout(p), shifts


def queue_case():
    """Five scenarios of the 3-class folds data for a queue of two slots: the four fold weights and unit weights, each with its
    own small per-class offsets.  (p with unit weights and zero offsets, lay, [(weight, offsets)] * 5)"""
    X, y, reg, W = folds_case3()
    rng = np.random.default_rng(35)
    p = multinomial_block_model(X, y, 3, reg, True)
    scen = [(w, 0.2 * rng.standard_normal((2, 150))) for w in list(W) + [np.ones(150)]]
    return p, nlp_terms_layout(p), scen


_REF = {}


def edge_reference(case, b, big=False):
    """(p, lay, x, sigma, lam, val, bnd) of instance b of an edge case, computed once per session and left unchanged"""
    key = (tuple(case), b, big)
    if key not in _REF:
        p, lay, inst = edge_model(*case, big=big)
        x, sigma, lam = edge_point(p, case[0], case[1])
        q = with_block(p, 0, weight=inst[b][0], shift=inst[b][1])
        val, bnd = NlpSoftmaxRef(q).want(x, sigma, lam, lay)
        _REF[key] = (q, lay, x, sigma, lam, val, bnd)
    return _REF[key]
