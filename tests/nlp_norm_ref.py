"""Test helper for the Euclidean-norm row blocks of a factorable NLP (sqpsolver.jl_amd/nlp_terms.py NlpNormBlock,
csrc/nlp_norm_dev.hpp):

    norm_reference      per output r the value and the Jacobian row, and the Hessian of the Lagrangian of all outputs, at 50
                        digits -- the residuals exact (integers on the square of the 2^-200 grid), the sums over the points (sum W v^2,
                        sum W v A, sum W A A') in exact integer arithmetic, square roots and quotients in mpmath -- with the
                        first-order forward error bound B of every entry (below); also the two parts of the Hessian apart
    NlpNormRef          the five outputs of a problem with blocks of any sort but Cox: NlpLseRef for the terms and the other
                        blocks, norm_reference for the norm blocks, whose outputs may share a target
    NlpNormNumpy, OracleNormTerms   the same outputs in plain numpy (nlp_terms.norm_block_eval beside the others) and
                        oracle.sqp_solve on them
    the cases of tests/test_gpu_nlp_norm.py, which tests/test_nlp_norm_cpu.py vouches for

The bound.  U = 2^-53; the weights are not negative.  Notation of the header: in segment r, over its n_r points, of which the
weighted ones (W_i != 0) count: m_r = max |v_i|, y_i = v_i / m_r, s_r = sum W_i y_i^2, f_r = m_r sqrt(s_r), q_i = W_i v_i / f_r,
G_r = A_r'q, mu_r = sigma on row 0 and lam[row - 1] elsewhere.  An output with f_r = 0 has the value 0, no derivative and no bound.
    Residuals.  E_i = (d + 2) U (sum_j |A_ij x_j| + |S_i|): d fused multiply-adds and one addition are off by at most (d + 1) U
times that sum of magnitudes to first order, (d + 2) leaves one ulp for the operand handed on.
    f.  df / dv_i = q_i, so the residual errors move f_r by at most Ev_r = sum_i |q_i| E_i.  The scale m_r cancels from every
output; the summands of s_r are not negative, so a sum of n_r of them in any order, their three roundings (y, y^2, W y^2), the
butterfly, the root and the product with m_r are covered by the relative error a_r = (n_r + 8) U with room to spare:
    B_F,r   = Ev_r + (a_r + 8 U) f_r,        rel_r = B_F,r / f_r   (the relative error of f_r and of sqrt(s_r)).
Here a_r = (n_r + 8) U is the term of the segment sum itself; the further 8 U are for the operations behind the sum -- the root,
the product with m_r, the rounding of the value handed on -- so that the sum's term stays what it is for every family.
    q and G.  q_i = W_i y_i / sqrt(s_r) is off by at most W_i E_i / f_r + (rel_r + 4 U) |q_i|; G_rk is a signed sum of n_r
products q_i A_ik, (n_r + 8) U of its magnitudes added.  With Mabs_rk = sum_i |q_i| |A_ik| and Ea_rk = sum_i W_i E_i |A_ik| / f_r:
    B_G,rk  = Ea_rk + (rel_r + a_r + 4 U) Mabs_rk.
    Hessian.  With aN = (N + 8) U and aR = (R + 8) U: chain 1 of the device is one sum over all N points of the block, whatever
their segment, of (mu_r W_i / f_r) A_ik A_il (the roundings of mu W, of the quotient and of z A: 3 U); chain 2 one sum over the R
outputs of (-mu_r / f_r) G_rk G_rl, each G off by B_G (the quotient, the product with G: 2 U; the final addition of the two
chains: one more U on each):
    B_H,kl  = sum_r |mu_r| / f_r [ (rel_r + aN + 4 U) sum_i W_i |A_ik A_il|
                                   + B_G,rk Mabs_rl + Mabs_rk B_G,rl + (rel_r + aR + 4 U) Mabs_rk Mabs_rl ].
The Hessian is bounded by the magnitudes of its two parts added, not by their difference: device and numpy form A'diag(z) A and
the rank-one part as separate sums, and their cancellation (complete for a single-point output, whose norm is linear) is paid for.
    Targets.  The K_t outputs of a target are added in one more sum: K_t U times the magnitudes added, sum_r f_r for a value and
sum_r Mabs_rk for a first derivative, on top of the outputs' own bounds.
The acceptance rule is the project's, nlp_block_ref.check_outputs: |got - want| <= 4 B + 1e-13 max |want|."""
from __future__ import annotations

import dataclasses

import mpmath as mp
import numpy as np

from nlp_block_ref import DPS, SQP_TIGHT, U, _first_slots, check_outputs   # noqa: F401
from nlp_general_ref import OracleGeneralTerms
from nlp_lse_ref import EDGE_LAM, M_EDGE, NlpLseNumpy, NlpLseRef, _seg   # noqa: F401
from nlp_rowblock_ref import _first_jslots, with_block   # noqa: F401
from sqpsolver_jl_amd.nlp_terms import (EXP, POW, SOFTPLUS, NlpLseBlock, NlpNormBlock, NlpRowBlock, NlpTerms, make_nlp_terms,   # noqa: F401
                                        nlp_terms_layout, norm_block_eval, norm_scenario, robust_lp_model, socp_synth,
                                        sum_of_norms_model)

GRID = 200                                      # the integer grid of the data: 2^-200 (the stability case: 2^-1100)


def _exact(a, shift):
    """the doubles a times 2^shift as Python integers, exact (every double is a multiple of 2^-1074)"""
    a = np.asarray(a, float)
    out = np.empty(a.shape, dtype=object)
    for idx in np.ndindex(a.shape):
        num, den = float(a[idx]).as_integer_ratio()
        k = den.bit_length() - 1
        assert k <= shift, (a[idx], shift)
        out[idx] = num << (shift - k)
    return out


def _mu(b, sigma, lam):
    return np.array([float(sigma) if i == 0 else float(lam[i - 1]) for i in b.rows.tolist()])


def norm_reference(b: NlpNormBlock, x, sigma, lam, shift=GRID):
    """((F [R], G [R, d], H [d, d]), (BF [R], BG [R, d], BH [d, d]), (H1, H2), Mabs [R, d]) of one block: the values at 50 digits
    rounded to doubles, their bounds, the two parts of the Hessian of the Lagrangian, H = H1 - H2 with H2 = sum_r mu_r G_r G_r' / f_r,
    and the magnitudes sum_i |q_i| |A_ik| of the Jacobian rows.  Columns in the block's own order.  shift: the grid 2^-shift that
    holds A, x, S and W exactly."""
    x = np.asarray(x, float)
    xs = x[b.cols - 1]
    N, d = b.A.shape
    R = len(b.rows)
    mu = _mu(b, sigma, lam)
    aA = np.abs(b.A)
    F, G, BF, BG, Mab = np.zeros(R), np.zeros((R, d)), np.zeros(R), np.zeros((R, d)), np.zeros((R, d))
    BH = np.zeros((d, d))
    aN, aR = (N + 8) * U, (R + 8) * U
    xi = _exact(xs, shift)
    with mp.workdps(DPS):
        two = lambda k: mp.mpf(2) ** (k * shift)
        H1m = [[mp.mpf(0)] * d for _ in range(d)]
        H2m = [[mp.mpf(0)] * d for _ in range(d)]
        for r in range(R):
            s0, s1 = int(b.seg[r]), int(b.seg[r + 1])
            on = [i for i in range(s0, s1) if b.weight[i] != 0.0]
            if not on:
                continue
            Ar, Wr = _exact(b.A[on], shift), _exact(b.weight[on], shift)
            v = Ar.dot(xi) + _exact(b.shift[on], shift) * (1 << shift)        # v 2^(2 shift), exact
            S2 = int(np.sum(Wr * v * v))                                       # sum W v^2 2^(5 shift), exact
            if S2 == 0:
                continue                                                       # the apex
            f = mp.sqrt(mp.mpf(S2) / two(5))
            F[r] = float(f)
            Gm = [mp.mpf(int(t)) / two(4) / f for t in Ar.T.dot(Wr * v)]       # sum W v A / f
            G[r] = [float(t) for t in Gm]
            H1r = Ar.T.dot(Wr[:, None] * Ar)                                   # sum W A A' 2^(3 shift), exact
            mr = mp.mpf(float(mu[r]))
            for k in range(d):
                for l in range(k + 1):
                    H1m[k][l] += mr * (mp.mpf(int(H1r[k, l])) / two(3)) / f
                    H2m[k][l] += mr * Gm[k] * Gm[l] / f
            # the bound
            ff = F[r]
            Af, Wf = aA[on], b.weight[on]
            E = (d + 2) * U * (Af @ np.abs(xs) + np.abs(b.shift[on]))
            q = np.array([float(mp.mpf(int(Wr[k] * v[k])) / two(3) / f) for k in range(len(on))])
            a = (s1 - s0 + 8) * U
            BF[r] = float(np.abs(q) @ E) + (a + 8.0 * U) * ff
            rel = BF[r] / ff
            Mabs = Af.T @ np.abs(q)
            Mab[r] = Mabs
            BG[r] = Af.T @ (Wf * E) / ff + (rel + a + 4.0 * U) * Mabs
            BH += abs(mu[r]) / ff * ((rel + aN + 4.0 * U) * (Af.T @ (Wf[:, None] * Af)) + np.outer(BG[r], Mabs) + np.outer(Mabs, BG[r])
                                     + (rel + aR + 4.0 * U) * np.outer(Mabs, Mabs))
        low = lambda M: np.array([[float(M[max(k, l)][min(k, l)]) for l in range(d)] for k in range(d)])
        H = low([[H1m[k][l] - H2m[k][l] if l <= k else mp.mpf(0) for l in range(d)] for k in range(d)])
        H1, H2 = low(H1m), low(H2m)
    return (F, G, H), (BF, BG, BH), (H1, H2), Mab


class NlpNormRef:
    """want(x, sigma, lam, lay) -> (values, bounds) of f, grad, g, jval, hval: terms and the other blocks by NlpLseRef, the norm
    blocks at 50 digits; shift: the grid of norm_reference."""

    def __init__(self, p: NlpTerms, shift=GRID):
        self.p, self.rest, self.shift = p, NlpLseRef(p), shift

    def want(self, x, sigma, lam, lay, blocks=None):
        p = self.p
        blocks = p.blocks if blocks is None else blocks
        val, bnd = self.rest.want(x, sigma, lam, lay, blocks=[b for b in blocks if not isinstance(b, NlpNormBlock)])
        first, jfirst = _first_slots(lay), _first_jslots(lay)
        for b in blocks:
            if not isinstance(b, NlpNormBlock):
                continue
            c = b.cols - 1
            (F, G, H), (BF, BG, BH), _, Mabs = norm_reference(b, x, sigma, lam, self.shift)
            rows = b.rows.tolist()
            for i in dict.fromkeys(rows):
                rs = [r for r in range(len(rows)) if rows[r] == i]
                K = len(rs) * U
                vF, bF = F[rs].sum(), BF[rs].sum() + K * np.abs(F[rs]).sum()
                vG, bG = G[rs].sum(axis=0), BG[rs].sum(axis=0) + K * Mabs[rs].sum(axis=0)
                if i == 0:
                    val["f"] += vF; bnd["f"] += bF
                    np.add.at(val["grad"], c, vG); np.add.at(bnd["grad"], c, bG)
                else:
                    val["g"][i - 1] += vF; bnd["g"][i - 1] += bF
                    s = [jfirst[(i - 1) * p.n + v] for v in c.tolist()]
                    np.add.at(val["jval"], s, vG); np.add.at(bnd["jval"], s, bG)
            for r in range(len(c)):
                for q in range(r + 1):
                    s = first[max(c[r], c[q]) * p.n + min(c[r], c[q])]
                    val["hval"][s] += H[r, q]; bnd["hval"][s] += BH[r, q]
        return val, bnd


class NlpNormNumpy(NlpLseNumpy):
    """f, grad, g, jac, hess of a problem with blocks of any sort but Cox in plain numpy (the interface of NlpRef)."""

    def f(self, x):
        return super().f(x) + norm_block_eval(self.p, x)[0]

    def grad(self, x):
        return super().grad(x) + norm_block_eval(self.p, x)[1]

    def g(self, x):
        return super().g(x) + norm_block_eval(self.p, x)[2]

    def jac(self, x, jrow, jcol):
        p = self.p
        out = super().jac(x, jrow, jcol)
        J = norm_block_eval(p, x)[3]
        jfirst = _first_jslots(type("L", (), dict(n=p.n, jrow=jrow, jcol=jcol)))
        for i, v in sorted({(int(i), int(v)) for b in p.blocks if isinstance(b, NlpNormBlock) for i in b.rows if i >= 1 for v in b.cols - 1}):
            out[jfirst[(i - 1) * p.n + v]] += J[i - 1, v]
        return out

    def hess(self, x, sigma, lam, hrow, hcol):
        p = self.p
        out = super().hess(x, sigma, lam, hrow, hcol)
        H = norm_block_eval(p, x, sigma, lam)[4]
        first = _first_slots(type("L", (), dict(n=p.n, hrow=hrow, hcol=hcol)))
        pairs = {(max(r, q), min(r, q)) for b in p.blocks if isinstance(b, NlpNormBlock) for r in (b.cols - 1).tolist() for q in (b.cols - 1).tolist()}
        for r, q in sorted(pairs):
            out[first[r * p.n + q]] += H[r, q]
        return out


class OracleNormTerms(OracleGeneralTerms):
    def __init__(self, p: NlpTerms, lay=None):
        lay = lay or nlp_terms_layout(p)
        super().__init__(dataclasses.replace(p, blocks=[]), lay)
        self.p, self.ref = p, NlpNormNumpy(p)


# ---- the cases of the GPU tests
# (N, d, segment lengths, rows) on the 19-row model of the log-sum-exp helper (row 1 linear, rows 2..19 nonlinear)
EDGE_CASES = [(1, 1, (1,), (5,)),
              (5, 17, (2, 3), (0, 0)),
              (193, 15, (1, 63, 64, 65), (4, 2, 4, 7)),
              (133, 16, (1,) * 5 + (128,), (0, 0, 9, 0, 3, 0)),
              (68, 33, (4,) * 17, (0,) * 17),
              (1030, 20, (1027, 3), (2, 0)),
              (130, 128, (129, 1), (0, 9)),
              (1100, 2, (1,) * 1100, tuple((0, 2, 3)[r % 3] for r in range(1100)))]
IDS = ["N%d-d%d-R%d" % (c[0], c[1], len(c[2])) for c in EDGE_CASES]


def edge_norm_data(N, d, lens):
    """A [N, d] and three (weight [N], shift [N]) pairs: weights with zeros scattered in, every segment keeping a weighted
    point (a single-point segment its one point).  The shifts keep the residuals of an output away from zero (1 + 0.3 N(0, 1)
    against |A_i'x| of about 0.5): the Hessian of a norm grows as 1 / f, and with it the bound against the other entries; past 64
    outputs A shrinks as 1 / sqrt(R / 64), since the magnitudes of the Hessian parts of all outputs add up in the bound while the
    parts themselves cancel (completely for single-point outputs)."""
    rng = np.random.default_rng([N, d, len(lens), 67])
    A = 0.5 * rng.standard_normal((N, d)) / np.sqrt(d * max(1.0, len(lens) / 64.0))
    seg = _seg(lens)
    inst = []
    for b in range(3):
        w = rng.uniform(0.5, 1.5, N)
        w[b::5] = 0.0
        for r, n_r in enumerate(lens):
            if not w[seg[r]:seg[r + 1]].any():
                w[seg[r] + (b + r) % n_r] = 0.75 + 0.25 * b
        inst.append((w, (1.0 + 0.3 * rng.standard_normal(N)) * rng.choice([-1.0, 1.0], N)))
    return A, inst


def edge_norm_model(N, d, lens, rows, data=None):
    """One norm block on an unsorted, non-contiguous subset of n = d + 5 variables; a ridge term on every variable (the diagonal
    slots of the block are shared with terms), a cross term, one linear row, and a squared term on the block's first column in
    every target row (block and plan share that row's value, a Jacobian slot and a Hessian slot).  The Hessian COO carries two
    duplicated slots, the Jacobian COO two duplicated slots (of the largest target row; of the linear row when every output sits
    on the objective).  Returns (p, lay, [(weight, shift)] * 3)."""
    n, m = d + 5, M_EDGE
    rng = np.random.default_rng([N, d, 7])
    cols = rng.permutation(n)[:d] + 1
    if d > 1 and cols.tolist() == sorted(cols.tolist()):
        cols = cols[::-1].copy()                                      # (unsorted in every case)
    A, inst = data or edge_norm_data(N, d, lens)
    terms = [(0, 0.3 + 0.1 * (j % 3), [(j + 1, POW, 2, 1.0, -0.2)]) for j in range(n)]
    terms += [(0, 0.5, [(int(cols[0]), POW), (n, EXP, 1, 0.5, 0.0)]), (1, 1.0, [(1, POW)]), (1, -1.0, [(n, POW)])]
    terms += [(i, 0.5, [(int(cols[0]), POW, 2)]) for i in sorted(set(rows)) if i >= 1]
    p = make_nlp_terms(n, m, 1, terms, f0=0.25, g0=0.1 * np.arange(m), xL=np.full(n, 0.5), xU=np.full(n, 1.5), gL=np.full(m, -50.0),
                       gU=np.full(m, 50.0), x0=np.linspace(0.7, 1.3, n),
                       blocks=[NlpNormBlock(cols, A, list(rows), _seg(lens), inst[0][1], inst[0][0])])
    lay = nlp_terms_layout(p)
    i0 = max(rows) or 1
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
        p, lay, inst = edge_norm_model(*case)
        x = edge_point(p, case[0], case[1])
        sigma = 0.0 if b == 2 else 0.7
        q = with_block(p, 0, weight=inst[b][0], shift=inst[b][1])
        val, bnd = NlpNormRef(q).want(x, sigma, EDGE_LAM, lay)
        _REF[key] = (q, lay, x, sigma, EDGE_LAM, val, bnd)
    return _REF[key]


STABLE = (70, 5, (5, 65), (0, 2))
STABLE_GRID = 1100


def stable_case():
    """N = 70, d = 5, segments of 5 and 65 points on rows 0 and 2, two instances.  Instance 0: the residuals of each segment
    spread over 1e-200 .. 1e200 with both ends taken -- shifts +-10^k, the rows of A of the points with k < 0 zeroed, so that
    their residuals are the shifts.  Instance 1: ordinary shifts, and one zero-weight point per segment whose row of A is 1.7e308
    throughout, so that its residual overflows to inf.  Returns (p, lay, [(weight, shift)] * 2, the zero-weight points, p with
    those points' rows of A zeroed)."""
    N, d, lens, rows = STABLE
    rng = np.random.default_rng(68)
    A = 0.5 * rng.standard_normal((N, d)) / np.sqrt(d)
    seg = _seg(lens)
    k = rng.uniform(-200.0, 200.0, N)
    for r in range(2):
        k[seg[r]], k[seg[r + 1] - 1] = 200.0, -200.0
    k = np.round(k)
    s1 = rng.choice([-1.0, 1.0], N) * 10.0 ** k
    gone = [int(seg[0]) + 2, int(seg[1]) + 40]
    tiny = [i for i in range(N) if k[i] < 0 and i not in gone]
    A[tiny] = 0.0
    w1 = rng.uniform(0.5, 1.5, N)
    s2, w2 = (1.0 + 0.3 * rng.standard_normal(N)), rng.uniform(0.5, 1.5, N)
    A[gone] = 1.7e308
    w1[gone] = 0.0
    w2[gone] = 0.0
    inst = [(w1, s1), (w2, s2)]
    p, lay, _ = edge_norm_model(N, d, lens, rows, data=(A, inst + inst[:1]))
    A0 = A.copy()
    A0[gone] = 0.0
    p0 = dataclasses.replace(p, blocks=[dataclasses.replace(p.blocks[0], A=A0)])
    return p, lay, inst, gone, p0


APEX = (40, 6, (7, 20, 9, 3, 1), (0, 4, 4, 0, 4))


def apex_case():
    """N = 40, d = 6: three ordinary outputs on rows 0, 4, 4, then an output of three points whose weighted residuals are exactly
    zero (rows (1, -1, 0, ..) of A on two columns that hold the same value at apex_point, a zero row, shifts 0; row 0) and a
    single-point output of weight 0 (row 4).  Returns (p, lay, p without the last two outputs): lay serves both."""
    N, d, lens, rows = APEX
    A, inst = edge_norm_data(N, d, lens)
    A, (w, s) = A.copy(), (inst[0][0].copy(), inst[0][1].copy())
    A[36:39] = 0.0
    A[36, 0], A[36, 1] = 1.0, -1.0
    A[37, 0], A[37, 1] = -2.0, 2.0
    s[36:39] = 0.0
    w[36:39] = (1.0, 0.5, 2.0)
    w[39] = 0.0
    p, lay, _ = edge_norm_model(N, d, lens, rows, data=(A, [(w, s)] * 3))
    b = p.blocks[0]
    cut = NlpNormBlock(b.cols, A[:36], rows[:3], _seg(lens[:3]), s[:36], w[:36])
    return p, lay, dataclasses.replace(p, blocks=[cut])


def apex_point(p):
    """a point at which the first two columns of the block hold the same value"""
    x = np.linspace(0.6, 1.4, p.n)
    c = p.blocks[0].cols - 1
    x[c[1]] = x[c[0]]
    return x


def overlap_model(norm_first):
    """A norm block (outputs on rows 2, 0 and 2) and a block with several outputs (rows 0 and 2) on overlapping columns --
    variables 3, 5, 7 in both -- in either block order."""
    n = 12
    rng = np.random.default_rng(14)
    c0, c1 = np.array([7, 3, 1, 5, 9, 10, 2]), np.array([5, 12, 3, 7, 4])
    b0 = NlpRowBlock(SOFTPLUS, c0, rng.standard_normal((37, 7)) / 2, [0, 2], 0.2 * rng.standard_normal(37), rng.uniform(0.0, 2.0, (2, 37)))
    b1 = NlpNormBlock(c1, rng.standard_normal((22, 5)), [2, 0, 2], [0, 9, 20, 22], 1.0 + 0.3 * rng.standard_normal(22), rng.uniform(0.5, 1.0, 22))
    terms = [(0, 0.4, [(j + 1, POW, 2)]) for j in range(n)] + [(1, 1.0, [(1, POW)]), (2, 1.0, [(3, POW, 2)])]
    p = make_nlp_terms(n, 2, 1, terms, xL=np.full(n, -3.0), xU=np.full(n, 3.0), gL=[-5.0, -np.inf], gU=[5.0, 40.0],
                       x0=np.linspace(-0.5, 0.5, n), blocks=[b1, b0] if norm_first else [b0, b1])
    return p, nlp_terms_layout(p)


def fermat_weber():
    """Fermat-Weber with five anchors in the plane, weights 1 .. 2, smoothed by 1e-3, a ridge of 1e-3, -10 <= x <= 10"""
    anchors = np.array([[0.0, 0.0], [4.0, 0.0], [4.0, 3.0], [1.0, 5.0], [-2.0, 2.0]])
    return sum_of_norms_model(anchors, weights=[1.0, 1.5, 1.0, 2.0, 1.25], smooth=1e-3, bounds=(-10.0, 10.0), ridge=1e-3)


def robust_lp():
    """min c'x under three rows a_k'x + kappa_k |P_k x| <= b_k (smoothed by 1e-3) on four variables in -5 .. 5, a ridge of 1e-2: at
    least two cone rows are active at the optimum (tests/test_nlp_norm_cpu.py)"""
    rng = np.random.default_rng(5)
    n = 4
    c = -np.array([1.0, 0.8, 0.6, 0.9])
    a = np.array([[1.0, 0.5, 0.2, 0.1], [0.2, 1.0, 0.4, 0.3], [0.3, 0.2, 1.0, 0.8]])
    P = [0.3 * rng.standard_normal((3, n)), 0.3 * rng.standard_normal((2, n)), 0.3 * rng.standard_normal((4, n))]
    return robust_lp_model(c, a, P, [1.0, 1.5, 0.8], [1.0, 1.2, 0.9], bounds=(-5.0, 5.0), smooth=1e-3, ridge=1e-2)


SOCP_N, SOCP_LENS, SOCP_SEEDS, SOCP_NOISE = 10, [4, 3, 70, 1, 64], (1, 2, 3), (0.0, 0.1)


def socp_cases(seed):
    """the two scenarios of socp_synth(10, SOCP_LENS, seed) that run as one batch: noise 0 and 0.1"""
    p = socp_synth(SOCP_N, SOCP_LENS, seed)
    return [norm_scenario(p, 1, seed, noise) for noise in SOCP_NOISE]


def socp_queue_case():
    """six scenarios of socp_synth(10, SOCP_LENS, 1) for a queue of two slots; scenario 0 is the programme itself"""
    p = socp_synth(SOCP_N, SOCP_LENS, 1)
    return p, [norm_scenario(p, s, 1, 0.15) for s in range(6)]


def norm_scipy(p):
    """the optimum of a model by SLSQP on the numpy evaluation"""
    import scipy.optimize as so
    R = NlpNormNumpy(p)
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
