"""Test helper for the dense data blocks with several outputs of a factorable NLP (sqpsolver.jl_amd/nlp_terms.py NlpRowBlock,
csrc/nlp_rowblock_dev.hpp):

    rowblock_reference  per output r the value and the Jacobian row, and the Hessian of the Lagrangian of all outputs, at 50
                        digits by block_reference's recipe (u_i, kappa .. kappa''' in mpmath, the sums over the points in exact
                        integer arithmetic on 2^-200 grids), with the first-order forward error bound of every entry:
                            Bf, Bg of tests/nlp_block_ref.py with the weights W_r;
                            BH with w_abs_i = sum_r |mu_r W_r[i]| in place of |sigma w_i| and N + 8 + R in place of N + 8,
                            for the R fused steps of e_i = sum_r mu_r W_r[i]   (mu_r = sigma on row 0, lam[row - 1] elsewhere)
    NlpRowBlockRef      the five outputs of a problem with such blocks: NlpGeneralRef for the terms, block_reference for the
                        objective's blocks, rowblock_reference for the rest, with the bound of every entry
    NlpRowBlockNumpy    the same outputs in plain numpy (nlp_terms.block_eval, row_block_eval): what the oracle's callbacks
                        evaluate
    OracleRowBlockTerms oracle.sqp_solve on a problem with such blocks
    the cases of tests/test_gpu_nlp_rowblock.py, which tests/test_nlp_rowblock_cpu.py vouches for"""
from __future__ import annotations

import dataclasses

import mpmath as mp
import numpy as np

from nlp_block_ref import DPS, U, _first_slots, _int, _ints, _SHIFT, block_reference, check_outputs, kappa_mp   # noqa: F401
from nlp_general_ref import NlpGeneralRef, OracleGeneralTerms
from sqpsolver_jl_amd.nlp_terms import (EXP, LOG, POW, SIGMOID, SOFTPLUS, NlpBlock, NlpRowBlock, NlpTerms, block_eval, fold_weights,
                                        make_nlp_terms, neyman_pearson_model, nlp_terms_layout, rate_constrained_logistic_model,
                                        row_block_eval)

SQP_TIGHT = dict(max_iter=60, literal_quirks=0, tol_infeas=1e-8, tol_residual=1e-8)
EDGE_KINDS = [(SOFTPLUS, 1), (SIGMOID, 1), (EXP, 1), (POW, 2), (POW, -1), (LOG, 1)]


def _mu(b: NlpRowBlock, sigma, lam):
    return np.array([float(sigma) if i == 0 else float(lam[i - 1]) for i in b.rows.tolist()])


def rowblock_reference(b: NlpRowBlock, x, sigma, lam):
    """(F [R], G [R, d], H [d, d]) of one block at 50 digits, rounded to doubles, and their bounds (BF [R], BG [R, d],
    BH [d, d]); H is the block's part of the Hessian of the Lagrangian.  Columns in the block's own order."""
    R = len(b.rows)
    mu = _mu(b, sigma, lam)
    with mp.workdps(DPS):
        xs = np.asarray(x, float)[b.cols - 1]
        N, d = b.A.shape
        Ai, xi = _ints(b.A), _ints(xs)
        ui = Ai.dot(xi) + _ints(b.shift) * (1 << _SHIFT)                 # u 2^400, exact
        k = np.empty((N, 4), dtype=object)
        h = mp.mpf(10) ** -20
        for i in range(N):
            u = mp.mpf(int(ui[i])) / mp.mpf(2) ** (2 * _SHIFT)
            k[i, :3] = kappa_mp(b.kind, b.exp, b.par, u)
            k[i, 3] = (kappa_mp(b.kind, b.exp, b.par, u + h)[2] - kappa_mp(b.kind, b.exp, b.par, u - h)[2]) / (2 * h)   # kappa''' for the bound
        back = lambda v, p: np.array([float(mp.mpf(int(t)) / mp.mpf(2) ** (p * _SHIFT)) for t in np.ravel(v)]).reshape(np.shape(v))
        F, G = np.zeros(R), np.zeros((R, d))
        for r in range(R):
            w = [mp.mpf(v) for v in b.weight[r]]
            z = np.array([[_int(w[i] * k[i, q]) for q in range(2)] for i in range(N)], dtype=object).reshape(N, 2)
            F[r] = float(back(z[:, 0].sum(), 1))
            G[r] = back(Ai.T.dot(z[:, 1]), 2)
        e = [sum((mp.mpf(mu[r]) * mp.mpf(b.weight[r, i]) for r in range(R)), mp.mpf(0)) for i in range(N)]
        z2 = np.array([_int(e[i] * k[i, 2]) for i in range(N)], dtype=object)
        H = back(Ai.T.dot(z2[:, None] * Ai), 3)
        kf = np.array([[float(t) for t in row] for row in k])
    r_ = np.abs(b.A * xs).sum(axis=1) + np.abs(b.shift)
    aA = np.abs(b.A)
    akf = np.abs(kf)
    BF, BG = np.zeros(R), np.zeros((R, d))
    for r in range(R):
        aw = np.abs(b.weight[r])
        BF[r] = U * ((N + 8) * (aw * akf[:, 0]).sum() + (d + 2) * (aw * akf[:, 1] * r_).sum())
        BG[r] = U * ((N + 8) * aA.T @ (aw * akf[:, 1]) + (d + 2) * aA.T @ (aw * akf[:, 2] * r_))
    wabs = np.abs(mu[:, None] * b.weight).sum(axis=0)
    BH = U * ((N + 8 + R) * aA.T @ ((wabs * akf[:, 2])[:, None] * aA) + (d + 2) * aA.T @ ((wabs * akf[:, 3] * r_)[:, None] * aA))
    return (F, G, H), (BF, BG, BH)


def _first_jslots(lay):
    n = lay.n
    first = {}
    for s, key in enumerate(((np.asarray(lay.jrow, np.int64) - 1) * n + np.asarray(lay.jcol, np.int64) - 1).tolist()):
        first.setdefault(key, s)
    return first


def _split(p):
    return [b for b in p.blocks if not isinstance(b, NlpRowBlock)], [b for b in p.blocks if isinstance(b, NlpRowBlock)]


class NlpRowBlockRef:
    """want(x, sigma, lam, lay) -> (values, bounds) of f, grad, g, jval, hval: terms by NlpGeneralRef, blocks at 50 digits."""

    def __init__(self, p: NlpTerms):
        self.p, self.terms = p, NlpGeneralRef(dataclasses.replace(p, blocks=[]))

    def want(self, x, sigma, lam, lay, blocks=None):
        p, T = self.p, self.terms
        val = dict(f=T.f(x), grad=T.grad(x), g=T.g(x), jval=T.jac(x, lay.jrow, lay.jcol), hval=T.hess(x, sigma, lam, lay.hrow, lay.hcol))
        bnd = dict(f=0.0, grad=np.zeros(p.n), g=np.zeros(p.m), jval=np.zeros(len(lay.jrow)), hval=np.zeros(len(lay.hrow)))
        first, jfirst = _first_slots(lay), _first_jslots(lay)

        def hess(c, H, BH):
            for r in range(len(c)):
                for q in range(r + 1):
                    s = first[max(c[r], c[q]) * p.n + min(c[r], c[q])]
                    val["hval"][s] += H[r, q]; bnd["hval"][s] += BH[r, q]

        for b in (p.blocks if blocks is None else blocks):
            c = b.cols - 1
            if not isinstance(b, NlpRowBlock):
                (f, g, H), (Bf, Bg, BH) = block_reference(b, x, sigma)
                val["f"] += f; bnd["f"] += Bf
                np.add.at(val["grad"], c, g); np.add.at(bnd["grad"], c, Bg)
                hess(c, H, BH)
                continue
            (F, G, H), (BF, BG, BH) = rowblock_reference(b, x, sigma, lam)
            for r, i in enumerate(b.rows.tolist()):
                if i == 0:
                    val["f"] += F[r]; bnd["f"] += BF[r]
                    np.add.at(val["grad"], c, G[r]); np.add.at(bnd["grad"], c, BG[r])
                else:
                    val["g"][i - 1] += F[r]; bnd["g"][i - 1] += BF[r]
                    s = [jfirst[(i - 1) * p.n + v] for v in c.tolist()]
                    np.add.at(val["jval"], s, G[r]); np.add.at(bnd["jval"], s, BG[r])
            hess(c, H, BH)
        return val, bnd


class NlpRowBlockNumpy:
    """f, grad, g, jac, hess of a problem with blocks of either sort in plain numpy (the interface of NlpRef)."""

    def __init__(self, p: NlpTerms):
        self.p, self.terms = p, NlpGeneralRef(dataclasses.replace(p, blocks=[]))

    def f(self, x):
        return self.terms.f(x) + block_eval(self.p, x)[0] + row_block_eval(self.p, x)[0]

    def grad(self, x):
        return self.terms.grad(x) + block_eval(self.p, x)[1] + row_block_eval(self.p, x)[1]

    def g(self, x):
        return self.terms.g(x) + row_block_eval(self.p, x)[2]

    def jac(self, x, jrow, jcol):
        p = self.p
        out = self.terms.jac(x, jrow, jcol)
        J = row_block_eval(p, x)[3]
        jfirst = _first_jslots(type("L", (), dict(n=p.n, jrow=jrow, jcol=jcol)))
        for i, v in sorted({(int(i), int(v)) for b in _split(p)[1] for i in b.rows if i >= 1 for v in b.cols - 1}):
            out[jfirst[(i - 1) * p.n + v]] += J[i - 1, v]
        return out

    def hess(self, x, sigma, lam, hrow, hcol):
        p = self.p
        out = self.terms.hess(x, sigma, lam, hrow, hcol)
        H = sigma * block_eval(p, x)[2] + row_block_eval(p, x, sigma, lam)[4]
        first = _first_slots(type("L", (), dict(n=p.n, hrow=hrow, hcol=hcol)))
        pairs = {(max(r, q), min(r, q)) for b in p.blocks for r in np.ravel(b.cols - 1).tolist() for q in np.ravel(b.cols - 1).tolist()}
        for r, q in sorted(pairs):
            out[first[r * p.n + q]] += H[r, q]
        return out


class OracleRowBlockTerms(OracleGeneralTerms):
    def __init__(self, p: NlpTerms, lay=None):
        lay = lay or nlp_terms_layout(p)
        super().__init__(dataclasses.replace(p, blocks=[]), lay)
        self.p, self.ref = p, NlpRowBlockNumpy(p)


def per_point_terms(p: NlpTerms) -> NlpTerms:
    """p with every block with several outputs written as one term per point and output (d <= 8 arguments per factor)"""
    terms = []
    aptr_p = p.aptr
    assert aptr_p is None and len(_split(p)[0]) == 0
    for t in range(len(p.trow)):
        ks = range(int(p.tptr[t]), int(p.tptr[t + 1]))
        terms.append((int(p.trow[t]), float(p.tcoef[t]), [(int(p.fvar[k]), int(p.fkind[k]), int(p.fexp[k]), float(p.fscale[k]), float(p.fshift[k])) for k in ks]))
    for b in _split(p)[1]:
        for r, i in enumerate(b.rows.tolist()):
            for q in range(b.A.shape[0]):
                terms.append((i, float(b.weight[r, q]), [([(int(v), float(a)) for v, a in zip(b.cols, b.A[q])], b.kind, b.exp, float(b.shift[q]))]))
    return make_nlp_terms(p.n, p.m, p.num_linear, terms, g0=p.g0, f0=p.f0, xL=p.xL, xU=p.xU, gL=p.gL, gU=p.gU, x0=p.x0)


# ---- the cases of the GPU tests
M_EDGE = 9                                      # row 1 linear, rows 2..9 nonlinear
EDGE_SHAPES = [(1, 1, [5]), (5, 17, [0, 3]), (63, 15, [4, 0, 2]), (64, 16, [5, 0, 9, 2, 3, 8, 4, 7]), (65, 33, [3, 2]),
               (1027, 20, [2, 0, 5]), (130, 128, [0, 9])]
EDGE_CASES = [(N, d, tuple(rows)) + EDGE_KINDS[i % 6] for i, (N, d, rows) in enumerate(EDGE_SHAPES)]
EDGE_LAM = np.array([0.4, 0.0, -0.8, 1.1, 0.6, 0.9, -0.3, 1.3, 0.7])     # row 2: zero, rows 3 and 7: negative


def edge_row_data(N, d, R, kind, e):
    """A [N, d] and three (weight [R, N], shift [N]) pairs: weights with zeros and a negative one per output where N allows,
    shifts that keep u > 0 on 0.5 <= x <= 1.5 for the kinds that need it (A >= 0 there)."""
    rng = np.random.default_rng([N, d, R, kind, e + 40])
    positive = kind == LOG or (kind == POW and e < 0)
    A = rng.uniform(0.1, 1.0, (N, d)) / d if positive else rng.standard_normal((N, d)) / np.sqrt(d)
    inst = []
    for b in range(3):
        w = rng.uniform(0.5, 1.5, (R, N))
        w[:, b::5] = 0.0
        for r in range(R):
            w[r, (b + 1 + r) % N] = -0.7
        s = rng.uniform(0.5, 1.0, N) if positive else 0.3 * rng.standard_normal(N)
        inst.append((w, s))
    return A, inst


def edge_row_model(N, d, rows, kind, e):
    """One block with len(rows) outputs on an unsorted, non-contiguous subset of n = d + 5 variables; a ridge term on every
    variable (the diagonal slots of the block are shared with terms), a cross term, one linear row, and a squared term on
    the block's first column in every target row (block and plan share that row's value, a Jacobian slot and a Hessian
    slot).  The Hessian COO carries two duplicated slots, the Jacobian COO two duplicated slots of a target row.
    Returns (p, lay, [(weight, shift)] * 3)."""
    n, m = d + 5, M_EDGE
    rng = np.random.default_rng([N, d, 7])
    cols = rng.permutation(n)[:d] + 1
    A, inst = edge_row_data(N, d, len(rows), kind, e)
    terms = [(0, 0.3 + 0.1 * (j % 3), [(j + 1, POW, 2, 1.0, -0.2)]) for j in range(n)]
    terms += [(0, 0.5, [(int(cols[0]), POW), (n, EXP, 1, 0.5, 0.0)]), (1, 1.0, [(1, POW)]), (1, -1.0, [(n, POW)])]
    terms += [(i, 0.5, [(int(cols[0]), POW, 2)]) for i in rows if i >= 1]
    p = make_nlp_terms(n, m, 1, terms, f0=0.25, g0=0.1 * np.arange(m), xL=np.full(n, 0.5), xU=np.full(n, 1.5), gL=np.full(m, -50.0),
                       gU=np.full(m, 50.0), x0=np.linspace(0.7, 1.3, n),
                       blocks=[NlpRowBlock(kind, cols, A, list(rows), inst[0][1], inst[0][0], exp=e)])
    lay = nlp_terms_layout(p)
    i0 = max(rows)
    dup = np.resize(np.flatnonzero(lay.jrow == i0)[:2], 2)          # (d = 1: the one entry twice more)
    lay = dataclasses.replace(lay, hrow=np.concatenate([lay.hrow, lay.hrow[:2]]), hcol=np.concatenate([lay.hcol, lay.hcol[:2]]),
                              jrow=np.concatenate([lay.jrow, lay.jrow[dup]]), jcol=np.concatenate([lay.jcol, lay.jcol[dup]]))
    return p, lay, inst


def with_block(p, k, weight=None, shift=None):
    """p with other data in block k"""
    b = p.blocks[k]
    nb = dataclasses.replace(b, weight=b.weight if weight is None else weight, shift=b.shift if shift is None else shift)
    return dataclasses.replace(p, blocks=p.blocks[:k] + [nb] + p.blocks[k + 1:])


def overlap_model():
    """An objective block of sqphip_nlp_add_block and a block with outputs on rows 0 and 2 on overlapping columns (variables
    3, 5, 7 in both): shared gradient entries and Hessian slots."""
    n = 12
    rng = np.random.default_rng(12)
    c0, c1 = np.array([7, 3, 1, 5, 9, 10, 2]), np.array([5, 12, 3, 7, 4])
    b0 = NlpBlock(SOFTPLUS, c0, rng.standard_normal((37, 7)) / 2, 0.2 * rng.standard_normal(37), rng.uniform(0.0, 2.0, 37))
    b1 = NlpRowBlock(POW, c1, rng.standard_normal((22, 5)) / 2, [2, 0], -rng.standard_normal(22), rng.uniform(0.5, 1.0, (2, 22)), exp=2)
    terms = [(0, 0.4, [(j + 1, POW, 2)]) for j in range(n)] + [(1, 1.0, [(1, POW)]), (2, 1.0, [(3, POW, 2)])]
    p = make_nlp_terms(n, 2, 1, terms, xL=np.full(n, -3.0), xU=np.full(n, 3.0), gL=[-5.0, -np.inf], gU=[5.0, 40.0],
                       x0=np.linspace(-0.5, 0.5, n), blocks=[b0, b1])
    return p, nlp_terms_layout(p)


def np_data():
    """N = 60, d = 6: an intercept plus 5 standard-normal features from default_rng(31), labels from a random unit direction
    plus 0.8 noise.  (X, y)"""
    rng = np.random.default_rng(31)
    X = np.column_stack([np.ones(60), rng.standard_normal((60, 5))])
    w = rng.standard_normal(6)
    y = (X @ (w / np.linalg.norm(w)) + 0.8 * rng.standard_normal(60) > 0).astype(float)
    return X, y


NP_REG, NP_ALPHA = 0.5, 0.3
# The l1 merit of the SQP needs a penalty above the row's multiplier (34.6; 14.9 .. 37.3 on the folds).  From the default
# start init_mu = 1 the update rule of the reference algorithm stops 1e-3 short of it (34.5760) and the run stalls in
# restoration, oracle and device alike; a start above the multipliers is the user's remedy there as here.
NP_OPTS = dict(SQP_TIGHT, init_mu=100.0)
NP_ALPHAS = (0.3, 0.4, 0.25, 0.35)


def np_case():
    X, y = np_data()
    return X, y, neyman_pearson_model(X, y, NP_ALPHA, NP_REG)


def np_fold_models(extra=0):
    """the model of np_case with the four fold weight vectors on both outputs and four levels; extra: further scenarios
    (all points, other levels) for the queue"""
    X, y = np_data()
    W = fold_weights(60, 4)
    ps = [neyman_pearson_model(X, y, a, NP_REG, w) for a, w in zip(NP_ALPHAS, W)]
    ps += [neyman_pearson_model(X, y, a, NP_REG) for a in (0.32, 0.45)[:extra]]
    return ps


def np_scipy(X, y, alpha, reg, weight=None):
    """(x, multiplier of the row) by SLSQP, polished by trust-constr"""
    import scipy.optimize as so
    w = np.ones(len(y)) if weight is None else weight
    w1, w0 = w * (y == 1), w * (y == 0) / (w * (y == 0)).sum()
    sp = lambda u: np.logaddexp(0.0, u)
    sg = lambda u: 0.5 * (1.0 + np.tanh(0.5 * u))
    f = lambda b: float(w1 @ (sp(X @ b) - X @ b) + 0.5 * reg * (b @ b))
    df = lambda b: X.T @ (w1 * (sg(X @ b) - 1.0)) + reg * b
    c = lambda b: float(alpha - w0 @ sp(X @ b))
    dc = lambda b: -X.T @ (w0 * sg(X @ b))
    r1 = so.minimize(f, np.zeros(X.shape[1]), jac=df, method="SLSQP", constraints=[dict(type="ineq", fun=c, jac=dc)],
                     options=dict(ftol=1e-15, maxiter=500))
    nl = so.NonlinearConstraint(lambda b: w0 @ sp(X @ b), -np.inf, alpha, jac=lambda b: (X.T @ (w0 * sg(X @ b)))[None, :])
    r2 = so.minimize(f, r1.x, jac=df, method="trust-constr", constraints=[nl], options=dict(gtol=1e-12, xtol=1e-14, maxiter=2000))
    return r1.x, r2.x, float(r2.v[0][0])


RATE_SEED = 1                                   # seeds 1 .. 8 were tried: the oracle ends with status 0 inside SQP_TIGHT on each; seed 1 has the
                                                # largest multiplier of the row (49.0), seed 3 an almost idle row (0.008)


def rate_case(seed=RATE_SEED, tol=0.0):
    """N = 50, d = 4: intercept plus three features, a group flag correlated with the first feature; the predicted rates of the
    two groups are held equal (tol = 0).  (X, y, group, p)"""
    rng = np.random.default_rng(seed)
    X = np.column_stack([np.ones(50), rng.standard_normal((50, 3))])
    group = (X[:, 1] + 0.7 * rng.standard_normal(50) > 0).astype(float)
    w = rng.standard_normal(4)
    y = (X @ (w / np.linalg.norm(w)) + 0.8 * rng.standard_normal(50) > 0).astype(float)
    return X, y, group, rate_constrained_logistic_model(X, y, group, 0.5, tol)
