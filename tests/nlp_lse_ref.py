"""Test helper for the log-sum-exp row blocks of a factorable NLP (sqpsolver.jl_amd/nlp_terms.py NlpLseBlock,
csrc/nlp_lse_dev.hpp):

    lse_reference       per output r the value and the Jacobian row, and the Hessian of the Lagrangian of all outputs, at 50
                        digits -- the logits exact (integers on the 2^-400 grid), exp, log and the segment sums T in mpmath, the
                        sums over the points in exact integer arithmetic on 2^-200 grids -- with the first-order forward error
                        bound B of every entry (below); also the two parts of the Hessian, sum_r mu_r A_r'diag(p) A_r and
                        sum_r mu_r G_r G_r', apart
    NlpLseRef           the five outputs of a problem with blocks of any sort: NlpGeneralRef for the terms, lse_reference,
                        rowblock_reference, softmax_reference or block_reference for the blocks
    NlpLseNumpy, OracleLseTerms   the same outputs in plain numpy (nlp_terms.block_eval, row_block_eval, lse_block_eval) and
                        oracle.sqp_solve on them
    the cases of tests/test_gpu_nlp_lse.py, which tests/test_nlp_lse_cpu.py vouches for

The bound.  U = 2^-53; the weights are not negative.  Notation of the header: in segment r, over its n_r points, of which the
weighted ones (W_i != 0) count: m_r = max u_i, e_i = W_i exp(u_i - m_r), T_r = sum e_i, p_i = e_i / T_r, G_r = A_r'p,
mu_r = sigma on row 0 and lam[row - 1] elsewhere.
    Logits.  E_i = (d + 2) U (sum_j |A_ij x_j| + |S_i|): d fused multiply-adds and one addition are off by at most (d + 1) U times
that sum of magnitudes to first order, (d + 2) leaves one ulp for the operand handed on.  The exponent u_i - m_r carries one
more rounding, at most U (max u - min u).  So every exponent of segment r is off by at most D_r = max E_i + U (max u - min u),
both over the weighted points.
    T.  Its summands are not negative, so a sum of n_r of them in any order has the relative error a_r = (n_r + 8) U (the 8:
exp, the product with W, the butterfly's six levels counted in n_r + 8 with room to spare).  The value of m_r cancels from every
output: moving the exponents by at most D_r moves log T_r + m_r by at most D_r and a ratio p_i by at most 2 D_r p_i.  Hence p_i
is off by rel_r p_i with rel_r = 2 D_r + a_r + 8 U (the divide and the roundings of exp and W e among the 8).
    Outputs.  With lse_r = m_r + log T_r and Mabs_r = sum_i p_i |A_i| (the p-weighted mean of the rows' magnitudes):
    B_value,r  = D_r + a_r + 8 U (1 + |m_r| + |lse_r|)      (the roundings of log T, of m + log T: ulps of numbers no larger
                 than |m| + |lse|)
    B_G,rk     = (rel_r + a_r) Mabs_rk                        (a signed sum of n_r products: (n_r + 8) U of its magnitudes added)
    B_H,kl     = sum_r |mu_r| [ (rel_r + aN + 2 U) sum_i p_i |A_ik A_il| + (2 (rel_r + a_r) + 2 U + aR) Mabs_rk Mabs_rl ]
with aN = (N + 8) U and aR = (R + 8) U: chain 1 of the device is one sum over all N points of the block, whatever their segment
(z = mu p and z A: the 2 U), chain 2 one sum over the R outputs of products of two entries of G, each off by (rel_r + a_r) Mabs
(the roundings of -mu G and of the product: the 2 U).  The Hessian is bounded by the magnitudes of its two parts added, not by
their difference: device and numpy form A'diag(z) A and the covariance part as separate sums, and their cancellation is paid for.
The acceptance rule is the project's, nlp_block_ref.check_outputs: |got - want| <= 4 B + 1e-13 max |want|."""
from __future__ import annotations

import dataclasses

import mpmath as mp
import numpy as np

from nlp_block_ref import DPS, SQP_TIGHT, U, _SHIFT, _first_slots, _int, _ints, block_reference, check_outputs   # noqa: F401
from nlp_general_ref import NlpGeneralRef, OracleGeneralTerms
from nlp_rowblock_ref import NlpRowBlockNumpy, _first_jslots, rowblock_reference, with_block   # noqa: F401
from nlp_softmax_ref import softmax_reference
from sqpsolver_jl_amd.nlp_terms import (EXP, POW, SOFTPLUS, NlpBlock, NlpLseBlock, NlpRowBlock, NlpSoftmaxBlock, NlpTerms,   # noqa: F401
                                        block_eval, geometric_program_model, gp_scenario, gp_synth, lse_block_eval, make_nlp_terms,
                                        nlp_terms_layout, row_block_eval)


def _mu(b, sigma, lam):
    return np.array([float(sigma) if i == 0 else float(lam[i - 1]) for i in b.rows.tolist()])


def lse_reference(b: NlpLseBlock, x, sigma, lam):
    """((F [R], G [R, d], H [d, d]), (BF [R], BG [R, d], BH [d, d]), (H1, H2)) of one block: the values at 50 digits rounded to
    doubles, their bounds, and the two parts of the Hessian of the Lagrangian, H = H1 - H2 with H2 = sum_r mu_r G_r G_r'.  Columns
    in the block's own order."""
    x = np.asarray(x, float)
    xs = x[b.cols - 1]
    N, d = b.A.shape
    R = len(b.rows)
    mu = _mu(b, sigma, lam)
    aA = np.abs(b.A)
    E = (d + 2) * U * (aA @ np.abs(xs) + np.abs(b.shift))
    F, G, BF, BG = np.zeros(R), np.zeros((R, d)), np.zeros(R), np.zeros((R, d))
    BH = np.zeros((d, d))
    aN, aR = (N + 8) * U, (R + 8) * U
    with mp.workdps(DPS):
        Ai = _ints(b.A)
        one2, one3 = mp.mpf(2) ** (2 * _SHIFT), mp.mpf(2) ** (3 * _SHIFT)
        ui = Ai.dot(_ints(xs)) + _ints(b.shift) * (1 << _SHIFT)          # u 2^400, exact
        H1m = [[mp.mpf(0)] * d for _ in range(d)]
        H2m = [[mp.mpf(0)] * d for _ in range(d)]
        for r in range(R):
            s0, s1 = int(b.seg[r]), int(b.seg[r + 1])
            on = [i for i in range(s0, s1) if b.weight[i] != 0.0]
            u = {i: mp.mpf(int(ui[i])) / one2 for i in on}
            m = max(u.values())
            e = {i: mp.mpf(float(b.weight[i])) * mp.exp(u[i] - m) for i in on}
            T = sum(e.values(), mp.mpf(0))
            p = {i: e[i] / T for i in on}
            lse = m + mp.log(T)
            F[r] = float(lse)
            pi = np.array([_int(p[i]) for i in on], dtype=object)
            Ar = Ai[on]
            Gm = [mp.mpf(int(t)) / one2 for t in Ar.T.dot(pi)]
            G[r] = [float(t) for t in Gm]
            H1r = Ar.T.dot(pi[:, None] * Ar)
            mr = mp.mpf(float(mu[r]))
            for k in range(d):
                for l in range(k + 1):
                    H1m[k][l] += mr * (mp.mpf(int(H1r[k, l])) / one3)
                    H2m[k][l] += mr * Gm[k] * Gm[l]
            # the bound
            pf = np.array([float(p[i]) for i in on])
            uf = np.array([float(u[i]) for i in on])
            D = E[on].max() + U * (uf.max() - uf.min())
            a = (s1 - s0 + 8) * U
            rel = 2.0 * D + a + 8.0 * U
            Mabs = aA[on].T @ pf
            BF[r] = D + a + 8.0 * U * (1.0 + abs(float(m)) + abs(F[r]))
            BG[r] = (rel + a) * Mabs
            BH += abs(mu[r]) * ((rel + aN + 2.0 * U) * (aA[on].T @ (pf[:, None] * aA[on])) + (2.0 * (rel + a) + 2.0 * U + aR) * np.outer(Mabs, Mabs))
        low = lambda M: np.array([[float(M[max(k, l)][min(k, l)]) for l in range(d)] for k in range(d)])
        H = low([[H1m[k][l] - H2m[k][l] if l <= k else mp.mpf(0) for l in range(d)] for k in range(d)])
        H1, H2 = low(H1m), low(H2m)
    return (F, G, H), (BF, BG, BH), (H1, H2)


class NlpLseRef:
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
            c = np.ravel(b.cols) - 1
            if not isinstance(b, (NlpRowBlock, NlpLseBlock)):
                (f, g, H), (Bf, Bg, BH) = (softmax_reference if isinstance(b, NlpSoftmaxBlock) else block_reference)(b, x, sigma)
                val["f"] += f; bnd["f"] += Bf
                np.add.at(val["grad"], c, g); np.add.at(bnd["grad"], c, Bg)
                hess(c, H, BH)
                continue
            (F, G, H), (BF, BG, BH) = (lse_reference if isinstance(b, NlpLseBlock) else rowblock_reference)(b, x, sigma, lam)[:2]
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


class NlpLseNumpy(NlpRowBlockNumpy):
    """f, grad, g, jac, hess of a problem with blocks of any sort but Cox in plain numpy (the interface of NlpRef)."""

    def outputs(self, x, sigma, lam, lay):
        return dict(f=self.f(x), grad=self.grad(x), g=self.g(x), jval=self.jac(x, lay.jrow, lay.jcol),
                    hval=self.hess(x, sigma, lam, lay.hrow, lay.hcol))

    def f(self, x):
        return super().f(x) + lse_block_eval(self.p, x)[0]

    def grad(self, x):
        return super().grad(x) + lse_block_eval(self.p, x)[1]

    def g(self, x):
        return super().g(x) + lse_block_eval(self.p, x)[2]

    def jac(self, x, jrow, jcol):
        p = self.p
        out = super().jac(x, jrow, jcol)
        J = lse_block_eval(p, x)[3]
        jfirst = _first_jslots(type("L", (), dict(n=p.n, jrow=jrow, jcol=jcol)))
        for i, v in sorted({(int(i), int(v)) for b in p.blocks if isinstance(b, NlpLseBlock) for i in b.rows if i >= 1 for v in b.cols - 1}):
            out[jfirst[(i - 1) * p.n + v]] += J[i - 1, v]
        return out

    def hess(self, x, sigma, lam, hrow, hcol):
        p = self.p
        out = super().hess(x, sigma, lam, hrow, hcol)
        H = lse_block_eval(p, x, sigma, lam)[4]
        first = _first_slots(type("L", (), dict(n=p.n, hrow=hrow, hcol=hcol)))
        pairs = {(max(r, q), min(r, q)) for b in p.blocks if isinstance(b, NlpLseBlock) for r in (b.cols - 1).tolist() for q in (b.cols - 1).tolist()}
        for r, q in sorted(pairs):
            out[first[r * p.n + q]] += H[r, q]
        return out


class OracleLseTerms(OracleGeneralTerms):
    def __init__(self, p: NlpTerms, lay=None):
        lay = lay or nlp_terms_layout(p)
        super().__init__(dataclasses.replace(p, blocks=[]), lay)
        self.p, self.ref = p, NlpLseNumpy(p)


# ---- the cases of the GPU tests
M_EDGE = 19                                     # row 1 linear, rows 2..19 nonlinear
# (N, d, segment lengths, rows)
EDGE_CASES = [(1, 1, (1,), (5,)),
              (5, 17, (2, 3), (0, 3)),
              (193, 15, (1, 63, 64, 65), (4, 2, 9, 7)),
              (133, 16, (1,) * 5 + (128,), (5, 0, 9, 2, 3, 8)),
              (68, 33, (4,) * 17, (3, 0, 2) + tuple(range(4, 18))),
              (1030, 20, (1027, 3), (2, 0)),
              (130, 128, (129, 1), (0, 9))]
IDS = ["N%d-d%d-R%d" % (c[0], c[1], len(c[2])) for c in EDGE_CASES]
# row 2: zero, rows 3 and 7: negative
EDGE_LAM = np.array([0.4, 0.0, -0.8, 1.1, 0.6, 0.9, -0.3, 1.3, 0.7, 0.5, 1.2, 0.35, 0.85, 0.45, 1.05, 0.65, 0.95, 0.55, 0.75])


def _seg(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def edge_lse_data(N, d, lens):
    """A [N, d] and three (weight [N], shift [N]) pairs: weights with zeros scattered in, every segment keeping a weighted
    point (a single-point segment its one point)."""
    rng = np.random.default_rng([N, d, len(lens), 61])
    A = rng.standard_normal((N, d)) / np.sqrt(d)
    seg = _seg(lens)
    inst = []
    for b in range(3):
        w = rng.uniform(0.5, 1.5, N)
        w[b::5] = 0.0
        for r, n_r in enumerate(lens):
            if not w[seg[r]:seg[r + 1]].any():
                w[seg[r] + (b + r) % n_r] = 0.75 + 0.25 * b
        inst.append((w, 0.3 * rng.standard_normal(N)))
    return A, inst


def edge_lse_model(N, d, lens, rows, data=None):
    """One log-sum-exp block on an unsorted, non-contiguous subset of n = d + 5 variables; a ridge term on every variable (the
    diagonal slots of the block are shared with terms), a cross term, one linear row, and a squared term on the block's first
    column in every target row (block and plan share that row's value, a Jacobian slot and a Hessian slot).  The Hessian COO
    carries two duplicated slots, the Jacobian COO two duplicated slots of a target row.  Returns (p, lay, [(weight, shift)] * 3)."""
    n, m = d + 5, M_EDGE
    rng = np.random.default_rng([N, d, 7])
    cols = rng.permutation(n)[:d] + 1
    A, inst = data or edge_lse_data(N, d, lens)
    terms = [(0, 0.3 + 0.1 * (j % 3), [(j + 1, POW, 2, 1.0, -0.2)]) for j in range(n)]
    terms += [(0, 0.5, [(int(cols[0]), POW), (n, EXP, 1, 0.5, 0.0)]), (1, 1.0, [(1, POW)]), (1, -1.0, [(n, POW)])]
    terms += [(i, 0.5, [(int(cols[0]), POW, 2)]) for i in rows if i >= 1]
    p = make_nlp_terms(n, m, 1, terms, f0=0.25, g0=0.1 * np.arange(m), xL=np.full(n, 0.5), xU=np.full(n, 1.5), gL=np.full(m, -50.0),
                       gU=np.full(m, 50.0), x0=np.linspace(0.7, 1.3, n),
                       blocks=[NlpLseBlock(cols, A, list(rows), _seg(lens), inst[0][1], inst[0][0])])
    lay = nlp_terms_layout(p)
    i0 = max(rows)
    dup = np.resize(np.flatnonzero(lay.jrow == i0)[:2], 2)          # (d = 1: the one entry twice more)
    lay = dataclasses.replace(lay, hrow=np.concatenate([lay.hrow, lay.hrow[:2]]), hcol=np.concatenate([lay.hcol, lay.hcol[:2]]),
                              jrow=np.concatenate([lay.jrow, lay.jrow[dup]]), jcol=np.concatenate([lay.jcol, lay.jcol[dup]]))
    return p, lay, inst


def edge_point(p, N, d):
    """where the edge tests evaluate"""
    return np.random.default_rng(N + d).uniform(0.6, 1.4, p.n)


_REF = {}


def edge_reference(case, b):
    """(p, lay, x, sigma, lam, val, bnd) of instance b of an edge case, computed once per session and left unchanged"""
    key = (tuple(case), b)
    if key not in _REF:
        p, lay, inst = edge_lse_model(*case)
        x = edge_point(p, case[0], case[1])
        sigma = 0.0 if b == 2 else 0.7
        q = with_block(p, 0, weight=inst[b][0], shift=inst[b][1])
        val, bnd = NlpLseRef(q).want(x, sigma, EDGE_LAM, lay)
        _REF[key] = (q, lay, x, sigma, EDGE_LAM, val, bnd)
    return _REF[key]


STABLE = (70, 5, (5, 65), (0, 2))


def stable_case():
    """N = 70, d = 5, segments of 5 and 65 points on rows 0 and 2, two instances: shifts that spread the logits of each segment
    over +-300 with both ends taken; and a zero-weight point per segment 800 above the rest.  Returns (p, lay, [(weight,
    shift)] * 2, the zero-weight points, p with those points' rows of A zeroed)."""
    N, d, lens, rows = STABLE
    rng = np.random.default_rng(62)
    A = rng.standard_normal((N, d)) / np.sqrt(d)
    seg = _seg(lens)
    s1 = rng.uniform(-300.0, 300.0, N)
    for r in range(2):
        s1[seg[r]], s1[seg[r + 1] - 1] = 300.0, -300.0
    w1 = rng.uniform(0.5, 1.5, N)
    s2, w2 = 0.3 * rng.standard_normal(N), rng.uniform(0.5, 1.5, N)
    gone = [int(seg[0]) + 2, int(seg[1]) + 40]
    for i in gone:
        s2[i] += 800.0
        w2[i] = 0.0
    inst = [(w1, s1), (w2, s2)]
    p, lay, _ = edge_lse_model(N, d, lens, rows, data=(A, inst + inst[:1]))
    A0 = A.copy()
    A0[gone] = 0.0
    p0 = dataclasses.replace(p, blocks=[dataclasses.replace(p.blocks[0], A=A0)])
    return p, lay, inst, gone, p0


def overlap_model(lse_first):
    """A log-sum-exp block (outputs on rows 2 and 0) and a block with several outputs (rows 0 and 2) on overlapping columns --
    variables 3, 5, 7 in both -- in either block order."""
    n = 12
    rng = np.random.default_rng(13)
    c0, c1 = np.array([7, 3, 1, 5, 9, 10, 2]), np.array([5, 12, 3, 7, 4])
    b0 = NlpRowBlock(SOFTPLUS, c0, rng.standard_normal((37, 7)) / 2, [0, 2], 0.2 * rng.standard_normal(37), rng.uniform(0.0, 2.0, (2, 37)))
    b1 = NlpLseBlock(c1, rng.standard_normal((22, 5)), [2, 0], [0, 9, 22], 0.3 * rng.standard_normal(22), rng.uniform(0.5, 1.0, 22))
    terms = [(0, 0.4, [(j + 1, POW, 2)]) for j in range(n)] + [(1, 1.0, [(1, POW)]), (2, 1.0, [(3, POW, 2)])]
    p = make_nlp_terms(n, 2, 1, terms, xL=np.full(n, -3.0), xU=np.full(n, 3.0), gL=[-5.0, -np.inf], gU=[5.0, 40.0],
                       x0=np.linspace(-0.5, 0.5, n), blocks=[b1, b0] if lse_first else [b0, b1])
    return p, nlp_terms_layout(p)


def box_gp():
    """The box design GP in the log variables (h, w, d): min 1 / (h w d) + 0.1 h + 0.1 w s.t. 0.02 h w + 0.02 h d <= 1,
    0.1 w d <= 1 (a single-point output), ridge 1e-3, -5 <= x <= 5, from 0."""
    pos = [([1.0, 0.1, 0.1], [[-1, -1, -1], [1, 0, 0], [0, 1, 0]]), ([0.02, 0.02], [[1, 1, 0], [1, 0, 1]]), ([0.1], [[0, 1, 1]])]
    return geometric_program_model(3, pos, bounds=(-5.0, 5.0), ridge=1e-3)


GP_N, GP_LENS, GP_SEEDS, GP_NOISE = 12, [5, 1, 70, 3, 64, 9], (1, 2, 3), (0.0, 0.1)


def gp_cases(seed):
    """the two scenarios of gp_synth(12, GP_LENS, seed) that run as one batch: noise 0 and 0.1"""
    p = gp_synth(GP_N, GP_LENS, seed)
    return [gp_scenario(p, 1, seed, noise) for noise in GP_NOISE]


def gp_queue_case():
    """six scenarios of gp_synth(12, GP_LENS, 1) for a queue of two slots; scenario 0 is the programme itself"""
    p = gp_synth(GP_N, GP_LENS, 1)
    return p, [gp_scenario(p, s, 1, 0.15) for s in range(6)]


def gp_scipy(p):
    """the optimum of a GP model by SLSQP on the numpy evaluation"""
    import scipy.optimize as so
    R = NlpLseNumpy(p)
    lay = nlp_terms_layout(p)

    def jac(x):
        J = np.zeros((p.m, p.n))
        J[lay.jrow - 1, lay.jcol - 1] = R.jac(x, lay.jrow, lay.jcol)
        return J

    cons = []
    for i in range(p.m):
        if np.isfinite(p.gU[i]):
            cons.append(dict(type="eq" if p.gL[i] == p.gU[i] else "ineq", fun=lambda x, i=i: p.gU[i] - R.g(x)[i], jac=lambda x, i=i: -jac(x)[i]))
        if np.isfinite(p.gL[i]) and p.gL[i] != p.gU[i]:
            cons.append(dict(type="ineq", fun=lambda x, i=i: R.g(x)[i] - p.gL[i], jac=lambda x, i=i: jac(x)[i]))
    r = so.minimize(R.f, p.x0, jac=R.grad, method="SLSQP", bounds=list(zip(p.xL, p.xU)), constraints=cons,
                    options=dict(ftol=1e-15, maxiter=1000))
    return r.x
