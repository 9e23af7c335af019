"""Test helper for the dense data blocks of a factorable NLP (sqpsolver.jl_amd/nlp_terms.py NlpBlock, csrc/nlp_block_dev.hpp):

    block_reference     f, grad and the Hessian entries of the blocks of a problem at 50 digits -- u_i, kappa, kappa', kappa''
                        in mpmath, the sums over the points in exact integer arithmetic on 2^-200 grids -- and, for every
                        output entry, the first-order forward error bound
                            B = 2^-53 [(N + 8) sum_i |summand_i| + (d + 2) sum_i |d summand_i / d u_i| (sum_j |A_ij x_j| + |b_i|)]
                        (recursive summation in any order plus a few ulp for the libm call and the products; the rounding
                        of u_i carried through kappa)
    NlpBlockRef         the five outputs of a problem with blocks: NlpGeneralRef for the terms plus block_reference, with
                        the bound of every entry
    NlpBlockNumpy       the same outputs in plain numpy (nlp_terms.block_eval): what the oracle's callbacks evaluate
    OracleBlockTerms    oracle.sqp_solve on a problem with blocks
    the cases of tests/test_gpu_nlp_block.py, which tests/test_nlp_block_cpu.py vouches for"""
from __future__ import annotations

import dataclasses

import mpmath as mp
import numpy as np

from nlp_general_ref import NlpGeneralRef, OracleGeneralTerms
from sqpsolver_jl_amd.nlp_terms import (ATAN, COS, EXP, LOG, POW, POWR, SIGMOID, SIN, SOFTPLUS, SQRT, TANH, NlpBlock, NlpTerms,
                                        block_eval, fold_weights, least_squares_block_model, logistic_block_model,
                                        logistic_model, make_nlp_terms, nlp_terms_layout, poisson_block_model)

DPS = 50
_SHIFT = 200                                   # the integer grids: 2^-200
U = 2.0 ** -53


def _int(v):
    """floor(v 2^200) of a double or an mpf (exact for a double above 2^-147)"""
    return int(mp.floor(mp.mpf(v) * mp.mpf(2) ** _SHIFT))


def _ints(a):
    a = np.asarray(a)
    out = np.empty(a.shape, dtype=object)
    for idx in np.ndindex(a.shape):
        out[idx] = _int(a[idx])
    return out


def kappa_mp(kind, e, par, u):
    """kappa, kappa', kappa'' at the mpf u"""
    if kind == POW:
        e = int(e)
        return u ** e, e * u ** (e - 1), e * (e - 1) * u ** (e - 2)
    if kind == POWR:
        p = mp.mpf(par)
        return u ** p, p * u ** (p - 1), p * (p - 1) * u ** (p - 2)
    if kind == SIN:
        return mp.sin(u), mp.cos(u), -mp.sin(u)
    if kind == COS:
        return mp.cos(u), -mp.sin(u), -mp.cos(u)
    if kind == EXP:
        return mp.exp(u), mp.exp(u), mp.exp(u)
    if kind == LOG:
        return mp.log(u), 1 / u, -1 / (u * u)
    if kind == SQRT:
        r = mp.sqrt(u)
        return r, 1 / (2 * r), -1 / (4 * u * r)
    if kind == TANH:
        t, e2 = mp.tanh(u), mp.exp(-2 * abs(u))
        d = 4 * e2 / (1 + e2) ** 2                            # sech^2 u without 1 - t t
        return t, d, -2 * t * d
    if kind == ATAN:
        q = 1 / (1 + u * u)
        return mp.atan(u), q, -2 * u * q * q
    s, sc = 1 / (1 + mp.exp(-u)), 1 / (1 + mp.exp(u))     # the complement from e^u: 1 - s is wrong beyond u = 115 at 50 digits
    if kind == SIGMOID:
        return s, s * sc, -s * sc * mp.tanh(u / 2)        # (1 - s) - s = -tanh(u / 2)
    assert kind == SOFTPLUS
    return (u if u > 0 else 0) + mp.log1p(mp.exp(-abs(u))), s, s * sc


def block_reference(b: NlpBlock, x, sigma):
    """(f, grad [d], H [d, d]) of one block at 50 digits, rounded to doubles, and their bounds (Bf, Bg [d], BH [d, d]); the
    Hessian and its bound carry sigma.  Columns in the block's own order."""
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
        w = [mp.mpf(v) for v in b.weight]
        z = np.array([[_int(w[i] * k[i, q]) for q in range(3)] for i in range(N)], dtype=object).reshape(N, 3)
        back = lambda v, p: np.array([float(mp.mpf(int(t)) / mp.mpf(2) ** (p * _SHIFT)) for t in np.ravel(v)]).reshape(np.shape(v))
        f = float(back(z[:, 0].sum(), 1))
        g = back(Ai.T.dot(z[:, 1]), 2)
        H = float(sigma) * back(Ai.T.dot(z[:, 2][:, None] * Ai), 3)
        kf = np.array([[float(t) for t in row] for row in k])
    wk = np.abs(b.weight[:, None] * kf)                                  # |w kappa^(q)|
    r = np.abs(b.A * xs).sum(axis=1) + np.abs(b.shift)
    aA = np.abs(b.A)
    Bf = U * ((N + 8) * wk[:, 0].sum() + (d + 2) * (wk[:, 1] * r).sum())
    Bg = U * ((N + 8) * aA.T @ wk[:, 1] + (d + 2) * aA.T @ (wk[:, 2] * r))
    BH = abs(float(sigma)) * U * ((N + 8) * aA.T @ (wk[:, 2][:, None] * aA) + (d + 2) * aA.T @ ((wk[:, 3] * r)[:, None] * aA))
    return (f, g, H), (Bf, Bg, BH)


def _first_slots(lay):
    n = lay.n
    hr, hc = np.asarray(lay.hrow, np.int64) - 1, np.asarray(lay.hcol, np.int64) - 1
    first = {}
    for s, key in enumerate((np.maximum(hr, hc) * n + np.minimum(hr, hc)).tolist()):
        first.setdefault(key, s)
    return first


class NlpBlockRef:
    """want(x, sigma, lam, lay) -> (values, bounds) of f, grad, g, jval, hval: terms by NlpGeneralRef, blocks at 50 digits."""

    def __init__(self, p: NlpTerms):
        self.p, self.terms = p, NlpGeneralRef(dataclasses.replace(p, blocks=[]))

    def want(self, x, sigma, lam, lay, blocks=None):
        p, T = self.p, self.terms
        val = dict(f=T.f(x), grad=T.grad(x), g=T.g(x), jval=T.jac(x, lay.jrow, lay.jcol), hval=T.hess(x, sigma, lam, lay.hrow, lay.hcol))
        bnd = dict(f=0.0, grad=np.zeros(p.n), g=np.zeros(p.m), jval=np.zeros(len(lay.jrow)), hval=np.zeros(len(lay.hrow)))
        first = _first_slots(lay)
        for b in (p.blocks if blocks is None else blocks):
            (f, g, H), (Bf, Bg, BH) = block_reference(b, x, sigma)
            c = b.cols - 1
            val["f"] += f; bnd["f"] += Bf
            np.add.at(val["grad"], c, g); np.add.at(bnd["grad"], c, Bg)
            for r in range(len(c)):
                for q in range(r + 1):
                    s = first[max(c[r], c[q]) * p.n + min(c[r], c[q])]
                    val["hval"][s] += H[r, q]; bnd["hval"][s] += BH[r, q]
        return val, bnd


def check_outputs(got, val, bnd, label="", floor=1e-13):
    """|got - want| <= 4 B + 1e-13 max|want| for every entry of the five outputs; returns the largest err / B per output over
    the entries with a bound (the figure DESIGN 5.7 records)."""
    ratios = {}
    for key in ("f", "grad", "g", "jval", "hval"):
        g_, w_, b_ = (np.atleast_1d(np.asarray(a, float)) for a in (got[key], val[key], bnd[key]))
        if not len(w_):
            continue
        err = np.abs(g_ - w_)
        k = b_ > 0
        ratios[key] = float((err[k] / b_[k]).max()) if k.any() else 0.0
        lim = 4.0 * b_ + floor * np.abs(w_).max()
        assert np.all(err <= lim), (label, key, float((err - lim).max()), int(np.argmax(err - lim)))
    print("err / B", label, {k: round(v, 3) for k, v in ratios.items()})
    return ratios


class NlpBlockNumpy:
    """f, grad, g, jac, hess of a problem with blocks in plain numpy (the interface of NlpRef)."""

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
        pairs = {(max(r, q), min(r, q)) for b in p.blocks for r in (b.cols - 1).tolist() for q in (b.cols - 1).tolist()}
        for r, q in pairs:
            out[first[r * p.n + q]] += H[r, q]
        return out


class OracleBlockTerms(OracleGeneralTerms):
    def __init__(self, p: NlpTerms, lay=None):
        lay = lay or nlp_terms_layout(p)
        super().__init__(dataclasses.replace(p, blocks=[]), lay)
        self.p, self.ref = p, NlpBlockNumpy(p)


# ---- the cases of the GPU tests
EDGE_SHAPES = [(1, 1), (3, 2), (4, 16), (5, 17), (63, 15), (64, 16), (65, 33), (1027, 20), (130, 128)]
EDGE_KINDS = [(SOFTPLUS, 1), (SIGMOID, 1), (EXP, 1), (POW, 2), (POW, -1), (LOG, 1)]
EDGE_CASES = [(N, d) + EDGE_KINDS[i % 6] for i, (N, d) in enumerate(EDGE_SHAPES)] + [(5, 17) + k for k in EDGE_KINDS if k != EDGE_KINDS[3]]
SQP_TIGHT = dict(max_iter=60, literal_quirks=0, tol_infeas=1e-8, tol_residual=1e-8)


def edge_block_data(N, d, kind, e, seed=0, positive=None):
    """A [N, d], three (weight, shift) pairs: weights with zeros and a negative one where N allows, shifts that keep u > 0
    on 0.5 <= x <= 1.5 for the kinds that need it (A >= 0 there)."""
    rng = np.random.default_rng([N, d, kind, e + 40, seed])
    positive = (kind == LOG or (kind == POW and e < 0)) if positive is None else positive
    A = rng.uniform(0.1, 1.0, (N, d)) / d if positive else rng.standard_normal((N, d)) / np.sqrt(d)
    inst = []
    for b in range(3):
        w = rng.uniform(0.5, 1.5, N)
        w[b::5] = 0.0
        w[(b + 1) % N] = -0.7
        s = rng.uniform(0.5, 1.0, N) if positive else 0.3 * rng.standard_normal(N)
        inst.append((w, s))
    return A, inst


def edge_model(N, d, kind, e):
    """One block on an unsorted, non-contiguous subset of n = d + 5 variables, a ridge term on every variable (the diagonal
    slots of the block are shared with terms), a cross term, one linear row; the Hessian COO carries two duplicated slots.
    Returns (p, lay, [(weight, shift)] * 3)."""
    n = d + 5
    rng = np.random.default_rng([N, d, 7])
    cols = rng.permutation(n)[:d] + 1
    A, inst = edge_block_data(N, d, kind, e)
    terms = [(0, 0.3 + 0.1 * (j % 3), [(j + 1, POW, 2, 1.0, -0.2)]) for j in range(n)]
    terms += [(0, 0.5, [(int(cols[0]), POW), (n, EXP, 1, 0.5, 0.0)]), (1, 1.0, [(1, POW)]), (1, -1.0, [(n, POW)])]
    p = make_nlp_terms(n, 1, 1, terms, f0=0.25, xL=np.full(n, 0.5), xU=np.full(n, 1.5), gL=[-1.0], gU=[1.0],
                       x0=np.linspace(0.7, 1.3, n), blocks=[NlpBlock(kind, cols, A, inst[0][1], inst[0][0], exp=e)])
    lay = nlp_terms_layout(p)
    lay = dataclasses.replace(lay, hrow=np.concatenate([lay.hrow, lay.hrow[:2]]), hcol=np.concatenate([lay.hcol, lay.hcol[:2]]))
    return p, lay, inst


def two_block_model():
    """Two blocks on overlapping columns (variables 3, 5, 7 in both): shared gradient entries and Hessian slots."""
    n = 12
    rng = np.random.default_rng(11)
    c0, c1 = np.array([7, 3, 1, 5, 9, 10, 2]), np.array([5, 12, 3, 7, 4])
    b0 = NlpBlock(SOFTPLUS, c0, rng.standard_normal((37, 7)) / 2, 0.2 * rng.standard_normal(37), rng.uniform(0.0, 2.0, 37))
    b1 = NlpBlock(POW, c1, rng.standard_normal((22, 5)) / 2, -rng.standard_normal(22), rng.uniform(0.5, 1.0, 22), exp=2)
    terms = [(0, 0.4, [(j + 1, POW, 2)]) for j in range(n)]
    p = make_nlp_terms(n, 0, 0, terms, xL=np.full(n, -3.0), xU=np.full(n, 3.0), x0=np.linspace(-0.5, 0.5, n), blocks=[b0, b1])
    return p, nlp_terms_layout(p)


def both_paths_case():
    """d = 6, N = 40: (X, y, reg, the block model, logistic_model's per-point terms)"""
    rng = np.random.default_rng(40)
    X = np.column_stack([np.ones(40), rng.standard_normal((40, 5))])
    y = (X @ rng.standard_normal(6) + 0.8 * rng.standard_normal(40) > 0).astype(float)
    return X, y, 0.5, logistic_block_model(X, y, 0.5), logistic_model(X, y, 0.5)


def folds_case():
    """N = 150, d = 20: an intercept plus 19 standard-normal features from default_rng(23), labels from a random unit-scale
    direction plus 0.8 noise, reg = 0.5; the four fold weight vectors.  (X, y, reg, W [4, 150])"""
    rng = np.random.default_rng(23)
    X = np.column_stack([np.ones(150), rng.standard_normal((150, 19))])
    w = rng.standard_normal(20)
    y = (X @ (w / np.linalg.norm(w)) + 0.8 * rng.standard_normal(150) > 0).astype(float)
    return X, y, 0.5, fold_weights(150, 4)


def newton_logistic(X, y, reg, w):
    """argmin sum_i w_i [softplus(X_i'b) - y_i X_i'b] + reg / 2 |b|^2 by Newton's method; (b, iterations)"""
    b = np.zeros(X.shape[1])
    for it in range(1, 60):
        s = 1.0 / (1.0 + np.exp(-(X @ b)))
        g = X.T @ (w * (s - y)) + reg * b
        H = X.T @ ((w * s * (1.0 - s))[:, None] * X) + reg * np.eye(len(b))
        step = np.linalg.solve(H, g)
        b = b - step
        if np.abs(step).max() < 1e-13:
            return b, it
    raise RuntimeError("Newton did not converge")


def poisson_case():
    """The X of folds_case, counts from default_rng(5) (Poisson with rate exp(X b), b = 0.2 N(0, 1)), six bootstrap weight
    vectors with integer entries 0..2.  (X, counts, reg, W [6, 150])"""
    X = folds_case()[0]
    rng = np.random.default_rng(5)
    b = 0.2 * rng.standard_normal(20)
    counts = rng.poisson(np.exp(X @ b)).astype(float)
    return X, counts, 0.5, rng.integers(0, 3, (6, 150)).astype(float)


def newton_poisson(X, c, reg, w):
    b = np.zeros(X.shape[1])
    for it in range(1, 60):
        e = np.exp(X @ b)
        g = X.T @ (w * (e - c)) + reg * b
        H = X.T @ ((w * e)[:, None] * X) + reg * np.eye(len(b))
        step = np.linalg.solve(H, g)
        b = b - step
        if np.abs(step).max() < 1e-13:
            return b, it
    raise RuntimeError("Newton did not converge")


def rows_case():
    """A least-squares block (N = 33, d = 9, three measurement vectors) under the linear row sum x = 1 and the quadratic row
    |x|^2 <= 0.13 of ordinary terms, 0.03 <= x <= 0.18: bounds active at the optimum.  (p, lay, [shift] * 3)"""
    rng = np.random.default_rng(33)
    A = rng.standard_normal((33, 9))
    xs = rng.dirichlet(np.ones(9))
    bs = [A @ xs + 0.3 * rng.standard_normal(33) for _ in range(3)]
    p = least_squares_block_model(A, bs[0], 0.1)
    terms = [(0, 0.05, [(j + 1, POW, 2)]) for j in range(9)] + [(1, 1.0, [(j + 1, POW)]) for j in range(9)] + \
            [(2, 1.0, [(j + 1, POW, 2)]) for j in range(9)]
    p = make_nlp_terms(9, 2, 1, terms, xL=np.full(9, 0.03), xU=np.full(9, 0.18), gL=[1.0, -np.inf], gU=[1.0, 0.13],
                       x0=np.full(9, 1.0 / 9), blocks=p.blocks)
    return p, nlp_terms_layout(p), [-b for b in bs]
