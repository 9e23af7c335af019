"""Test helper for the Cox partial-likelihood data blocks of a factorable NLP (sqpsolver.jl_amd/nlp_terms.py NlpCoxBlock,
csrc/nlp_cox_dev.hpp):

    cox_reference       f, grad and Hessian of one Cox block at 50 digits -- the logits exact (integers on the 2^-400 grid), exp,
                        log and the running sums T, Q, P in mpmath, the sums over the points in exact integer arithmetic on
                        2^-200 grids -- and the first-order forward error bound B of every output entry (below); also the two
                        parts of the Hessian, A'diag(e Q) A and the covariance part, apart
    NlpCoxRef           the five outputs of a problem with blocks of any sort: NlpGeneralRef for the terms, cox_reference,
                        softmax_reference or block_reference for the blocks
    NlpCoxNumpy, OracleCoxTerms   the same outputs in plain numpy (nlp_terms.block_eval) and oracle.sqp_solve on them
    the cases of tests/test_gpu_nlp_cox.py, which tests/test_nlp_cox_cpu.py vouches for

The bound.  U = 2^-53; weights and events are not negative.  Notation of the header: m = max u, e_j = W_j exp(u_j - m),
T_i = sum_{j < risk_i} e_j, c_i = W_i event_i, q_i = c_i / T_i, Q_j = sum_{i: risk_i > j} q_i, G_j = e_j Q_j.
    Logits.  r_i = sum_j |A_ij x_j| + |S_i| and E_i = (d + 2) U r_i: d fused multiply-adds and one addition are off by at most
(d + 1) U r_i to first order, (d + 2) leaves one ulp for the operand handed on.  The exponent u_j - m carries one more
rounding, U |u_j - m| <= U (max u - min u).  So every exponent is off by at most D = max_i E_i + U (max u - min u).
    T and Q.  Their summands are not negative, so a recursive sum of up to N of them in any order has the relative error
a = (N + 8) U (the 8: exp, the products with W and event, the divide).  The value of m cancels from every output, so what counts
is the error of the ratios p = e_j / T_i (a softmax over the risk set) and of log T_i + m: moving the exponents by at most D
moves log T_i + m by at most D and p by at most 2 D p -- twice the largest logit error.  Hence, relative to themselves,
    e_j / T_i: 2 D + a,      G_j = sum_i c_i e_j / T_i: rel = 2 D + 2 a + 8 U      (a second sum, over i),
    Mbar_i = P[risk_i - 1] / T_i (the p-weighted mean of the rows of A): off by at most rel Mabs_i, Mabs_i the same mean of |A|
(P is a signed sum: (N + 8) U sum |summand| is relative to its magnitudes added, which is what Mabs holds).
    Outputs.  With lse_i = log sum_{j < risk_i} W_j exp(u_j):
    B_f     = (N + 8) U sum_i |c_i (lse_i - u_i)| + sum_i c_i (2 D + a + E_i + 8 U (1 + |m| + |lse_i| + |u_i|))
              (the roundings of log T, of m + log T and of the subtraction are ulps of numbers no larger than |m| + |lse| + |u|)
    B_g,k   = (N + 8) U sum_j |G_j - c_j| |A_jk| + sum_j (rel G_j + 2 U c_j) |A_jk|
              (G_j - c_j cancels: the error of G_j is relative to G_j, not to the difference)
    B_H,kl  = |sigma| [ sum_j G_j |A_jk A_jl| (rel + (N + 8) U) + sum_i c_i Mabs_ik Mabs_il (2 rel + (N + 8) U) ]
The Hessian is bounded by the magnitudes of its two parts added, not by their difference: the device (and numpy) form
A'diag(G) A and the covariance part sum_i c_i Mbar_i Mbar_i' as separate sums, and their cancellation is paid for.
The acceptance rule is the project's, nlp_block_ref.check_outputs: |got - want| <= 4 B + 1e-13 max |want|."""
from __future__ import annotations

import dataclasses

import mpmath as mp
import numpy as np

from nlp_block_ref import DPS, SQP_TIGHT, U, _SHIFT, _first_slots, _int, _ints, block_reference, check_outputs   # noqa: F401
from nlp_general_ref import NlpGeneralRef
from nlp_softmax_ref import NlpSoftmaxNumpy as NlpCoxNumpy, OracleSoftmaxTerms as OracleCoxTerms, softmax_reference, with_block   # noqa: F401
from sqpsolver_jl_amd.nlp_terms import (EXP, POW, SOFTPLUS, NlpBlock, NlpCoxBlock, NlpSoftmaxBlock, NlpTerms, block_eval,   # noqa: F401
                                        cox_block_model, cox_risk, fold_weights, make_nlp_terms, nlp_terms_layout)


def cox_reference(b: NlpCoxBlock, x, sigma):
    """((f, grad [d], H [d, d]), (Bf, Bg [d], BH [d, d]), (H1, H2)) of one Cox block: the values at 50 digits rounded to doubles,
    their bounds, and the two parts of the Hessian, H = H1 - H2 with H2 the covariance part; all three Hessians and the bound
    carry sigma.  Columns in the block's own order."""
    x = np.asarray(x, float)
    xs = x[b.cols - 1]
    N, d = b.A.shape
    risk = np.asarray(b.risk, np.int64)
    first = np.searchsorted(risk, np.arange(N), side="right")
    with mp.workdps(DPS):
        Ai = _ints(b.A)
        one = mp.mpf(2) ** (2 * _SHIFT)
        ui = Ai.dot(_ints(xs)) + _ints(b.shift) * (1 << _SHIFT)          # u 2^400, exact
        u = [mp.mpf(int(t)) / one for t in ui]
        w = [mp.mpf(float(v)) for v in b.weight]
        c = [w[i] * mp.mpf(float(b.event[i])) for i in range(N)]
        m = max(u)
        e = [w[j] * mp.exp(u[j] - m) for j in range(N)]
        Am = [[mp.mpf(float(v)) for v in row] for row in b.A]
        # running sums of e, e A and e |A| down the points, kept at the ends of the risk sets only
        ends = set(int(r) - 1 for i, r in enumerate(risk) if c[i] != 0)
        T, P, Pa = {}, {}, {}
        t, pr, pa = mp.mpf(0), [mp.mpf(0)] * d, [mp.mpf(0)] * d
        for j in range(N):
            t += e[j]
            pr = [pr[k] + e[j] * Am[j][k] for k in range(d)]
            pa = [pa[k] + e[j] * abs(Am[j][k]) for k in range(d)]
            if j in ends:
                T[j], P[j], Pa[j] = t, pr, pa
        q = [c[i] / T[int(risk[i]) - 1] if c[i] != 0 else mp.mpf(0) for i in range(N)]
        sq, acc = [mp.mpf(0)] * (N + 1), mp.mpf(0)
        for i in range(N - 1, -1, -1):
            acc += q[i]
            sq[i] = acc
        G = [e[j] * sq[int(first[j])] for j in range(N)]
        lse = [m + mp.log(T[int(risk[i]) - 1]) if c[i] != 0 else mp.mpf(0) for i in range(N)]
        back = lambda v, p: np.array([float(mp.mpf(int(t_)) / mp.mpf(2) ** (p * _SHIFT)) for t_ in np.ravel(v)]).reshape(np.shape(v))
        f = float(back(sum(_int(c[i] * (lse[i] - u[i])) for i in range(N) if c[i] != 0), 1))
        g = back(Ai.T.dot(np.array([_int(G[j] - c[j]) for j in range(N)], dtype=object)), 2)
        H1 = back(Ai.T.dot(np.array([_int(v) for v in G], dtype=object)[:, None] * Ai), 3)
        on = [i for i in range(N) if c[i] != 0]
        if on:
            Mi = np.array([[_int(P[int(risk[i]) - 1][k] / T[int(risk[i]) - 1]) for k in range(d)] for i in on], dtype=object).reshape(len(on), d)
            ci = np.array([_int(c[i]) for i in on], dtype=object)
            H2 = back(Mi.T.dot(ci[:, None] * Mi), 3)
        else:
            H2 = np.zeros((d, d))
        Mabs = np.zeros((N, d))
        for i in on:
            Mabs[i] = [float(Pa[int(risk[i]) - 1][k] / T[int(risk[i]) - 1]) for k in range(d)]
        Gf, cf, uf = (np.array([float(v) for v in a_]) for a_ in (G, c, u))
        lsef, mf = np.array([float(v) for v in lse]), float(m)
        fi = np.array([float(c[i] * (lse[i] - u[i])) for i in range(N)])
    s = float(sigma)
    H1, H2 = s * H1, s * H2
    aA = np.abs(b.A)
    E = (d + 2) * U * (aA @ np.abs(xs) + np.abs(b.shift))
    D = E.max() + U * (uf.max() - uf.min())
    a = (N + 8) * U
    rel = 2.0 * D + 2.0 * a + 8.0 * U
    Bf = a * np.abs(fi).sum() + float(cf @ (2.0 * D + a + E + 8.0 * U * (1.0 + abs(mf) + np.abs(lsef) + np.abs(uf))))
    Bg = a * (aA.T @ np.abs(Gf - cf)) + aA.T @ (rel * Gf + 2.0 * U * cf)
    BH = abs(s) * ((rel + a) * (aA.T @ (Gf[:, None] * aA)) + (2.0 * rel + a) * (Mabs.T @ (cf[:, None] * Mabs)))
    return (f, g, H1 - H2), (Bf, Bg, BH), (H1, H2)


def _reference(b, x, sigma):
    if isinstance(b, NlpCoxBlock):
        return cox_reference(b, x, sigma)[:2]
    return (softmax_reference if isinstance(b, NlpSoftmaxBlock) else block_reference)(b, x, sigma)


class NlpCoxRef:
    """want(x, sigma, lam, lay) -> (values, bounds) of f, grad, g, jval, hval: terms by NlpGeneralRef, blocks at 50 digits."""

    def __init__(self, p: NlpTerms):
        self.p, self.terms = p, NlpGeneralRef(dataclasses.replace(p, blocks=[]))

    def want(self, x, sigma, lam, lay, blocks=None):
        p, T = self.p, self.terms
        val = dict(f=T.f(x), grad=T.grad(x), g=T.g(x), jval=T.jac(x, lay.jrow, lay.jcol), hval=T.hess(x, sigma, lam, lay.hrow, lay.hcol))
        bnd = dict(f=0.0, grad=np.zeros(p.n), g=np.zeros(p.m), jval=np.zeros(len(lay.jrow)), hval=np.zeros(len(lay.hrow)))
        first = _first_slots(lay)
        for b in (p.blocks if blocks is None else blocks):
            (f, g, H), (Bf, Bg, BH) = _reference(b, x, sigma)
            c = np.ravel(b.cols) - 1
            val["f"] += f; bnd["f"] += Bf
            np.add.at(val["grad"], c, g); np.add.at(bnd["grad"], c, Bg)
            for r in range(len(c)):
                for q in range(r + 1):
                    s = first[max(c[r], c[q]) * p.n + min(c[r], c[q])]
                    val["hval"][s] += H[r, q]; bnd["hval"][s] += BH[r, q]
        return val, bnd


# ---- the cases of the GPU tests
# (N, d, risk pattern, event pattern, spread).  risk: "untied" risk_i = i + 1; "tied" risk = N; "groups" tie groups of 3, 1, 5, 2,
# 7, 3, 1, ... points, which straddle the 4-point groups of the MFMA loop (4 | 5 .. 8 | 9), the 64-lane chunk of the scans
# (63, 64 | ) and the thread stride (1019 .. 1025).  event: "mixed" about two thirds events; "first" the only event at point 0;
# "none".  spread: offsets that spread the logits over +-300.
EDGE_CASES = [(1, 1, "untied", "mixed", 0), (3, 15, "untied", "mixed", 0), (4, 16, "tied", "mixed", 0), (5, 17, "groups", "mixed", 0),
              (63, 33, "groups", "mixed", 0), (64, 128, "untied", "mixed", 0), (65, 5, "groups", "mixed", 0), (1023, 3, "groups", "mixed", 0),
              (1024, 2, "tied", "mixed", 0), (1025, 3, "groups", "mixed", 0), (2049, 2, "groups", "mixed", 0), (65, 5, "groups", "first", 0),
              (65, 3, "groups", "mixed", 1)]
NO_EVENT = (65, 5, "groups", "none", 0)
GROUPS = (3, 1, 5, 2, 7)
IDS = ["N%d-d%d-%s-%s%s" % (c[0], c[1], c[2], c[3], "-spread" if c[4] else "") for c in EDGE_CASES]


def risk_pattern(N, kind):
    if kind == "untied":
        return np.arange(1, N + 1, dtype=np.int32)
    if kind == "tied":
        return np.full(N, N, dtype=np.int32)
    out, i, k = np.empty(N, dtype=np.int32), 0, 0
    while i < N:
        j = min(N, i + GROUPS[k % len(GROUPS)])
        out[i:j] = j
        i, k = j, k + 1
    return out


def edge_data(N, d, risk_kind, event_kind, spread):
    """A [N, d], risk, event, three (weight [N], offsets [N]) pairs: uniform weights with zeros scattered in -- one of them on
    the first point of a tie group, where N allows --, small integer weights (a resample), and 0 / 1 weights (a fold); every
    instance keeps a point with an event and a positive weight.  spread: offsets uniform in +-300."""
    rng = np.random.default_rng([N, d, len(risk_kind), len(event_kind), spread, 5])
    A = rng.standard_normal((N, d)) / np.sqrt(d)
    risk = risk_pattern(N, risk_kind)
    event = {"mixed": (rng.random(N) < 0.67).astype(float), "first": np.zeros(N), "none": np.zeros(N)}[event_kind]
    if event_kind != "none":
        event[0] = 1.0
    starts = np.flatnonzero(np.r_[True, risk[1:] != risk[:-1]] & (np.r_[risk[1:] == risk[:-1], False]))      # leaders of groups of 2 or more
    inst = []
    for b in range(3):
        w = [rng.uniform(0.5, 1.5, N), rng.integers(0, 4, N).astype(float), (rng.random(N) < 0.75).astype(float)][b]
        if b == 0 and N > 1:
            w[2::5] = 0.0
            if len(starts) > 1:
                w[starts[1]] = 0.0
        w[0] = max(w[0], 1.0)
        s = rng.uniform(-300.0, 300.0, N) if spread else 0.3 * rng.standard_normal(N)
        inst.append((w, s))
    return A, risk, event, inst


def edge_model(N, d, risk_kind, event_kind, spread):
    """One Cox block on an unsorted, non-contiguous choice of d of n = d + 5 variables, a ridge term on every variable (the
    block's diagonal slots are shared with terms), a cross term, one linear row; the Hessian COO carries two duplicated slots.
    Returns (p, lay, [(weight, offsets)] * 3)."""
    n = d + 5
    rng = np.random.default_rng([N, d, 7])
    cols = rng.permutation(n)[:d] + 1
    A, risk, event, inst = edge_data(N, d, risk_kind, event_kind, spread)
    terms = [(0, 0.3 + 0.1 * (j % 3), [(j + 1, POW, 2, 1.0, -0.2)]) for j in range(n)]
    terms += [(0, 0.5, [(int(cols[0]), POW), (n, EXP, 1, 0.5, 0.0)]), (1, 1.0, [(1, POW)]), (1, -1.0, [(n, POW)])]
    blk = NlpCoxBlock(cols, A, risk, event, inst[0][1], inst[0][0])
    p = make_nlp_terms(n, 1, 1, terms, f0=0.25, xL=np.full(n, 0.5), xU=np.full(n, 1.5), gL=[-1.0], gU=[1.0],
                       x0=np.linspace(0.7, 1.3, n), blocks=[blk])
    lay = nlp_terms_layout(p)
    lay = dataclasses.replace(lay, hrow=np.concatenate([lay.hrow, lay.hrow[:2]]), hcol=np.concatenate([lay.hcol, lay.hcol[:2]]))
    return p, lay, inst


def edge_point(p, N, d):
    """where the edge tests evaluate: (x, sigma, lam)"""
    rng = np.random.default_rng(N + d)
    return rng.uniform(0.6, 1.4, p.n), 0.7, np.array([0.8])


_REF = {}


def edge_reference(case, b):
    """(p, lay, x, sigma, lam, val, bnd, (H1, H2)) of instance b of an edge case, computed once per session and left unchanged"""
    key = (tuple(case), b)
    if key not in _REF:
        p, lay, inst = edge_model(*case)
        x, sigma, lam = edge_point(p, case[0], case[1])
        q = with_block(p, 0, weight=inst[b][0], shift=inst[b][1])
        val, bnd = NlpCoxRef(q).want(x, sigma, lam, lay)
        _REF[key] = (q, lay, x, sigma, lam, val, bnd, cox_reference(q.blocks[0], x, sigma)[2])
    return _REF[key]


def mixed_model(cox_first):
    """One scalar (softplus) block and one Cox block (N = 22, d = 3, tie groups) on overlapping columns -- variables 3, 5, 7 in
    both -- in either block order."""
    n = 10
    rng = np.random.default_rng(12)
    c0 = np.array([7, 3, 1, 5, 9, 10, 2])
    c1 = np.array([5, 7, 3])
    b0 = NlpBlock(SOFTPLUS, c0, rng.standard_normal((37, 7)) / 2, 0.2 * rng.standard_normal(37), rng.uniform(0.0, 2.0, 37))
    b1 = NlpCoxBlock(c1, rng.standard_normal((22, 3)), risk_pattern(22, "groups"), (rng.random(22) < 0.7).astype(float),
                     0.2 * rng.standard_normal(22), rng.uniform(0.5, 1.0, 22))
    terms = [(0, 0.4, [(j + 1, POW, 2)]) for j in range(n)]
    p = make_nlp_terms(n, 0, 0, terms, xL=np.full(n, -3.0), xU=np.full(n, 3.0), x0=np.linspace(-0.5, 0.5, n),
                       blocks=[b1, b0] if cox_first else [b0, b1])
    return p, nlp_terms_layout(p)


def survival_data(N=48, d=3, seed=41):
    """(A, time, event): exponential survival times with hazard exp(A beta), rounded to one decimal (ties), about a quarter
    censored"""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((N, d))
    t = rng.exponential(np.exp(-(A @ np.array([0.8, -0.5, 0.3][:d]))))
    cens = rng.exponential(2.5, N)
    return A, np.round(np.minimum(t, cens), 1), (t <= cens).astype(float)


def folds_case(ridge=0.5):
    """N = 48, d = 3: the model with unit weights and the four fold weight vectors in the block's (sorted) order.  (p, W [4, 48])"""
    A, t, ev = survival_data()
    p = cox_block_model(A, t, ev, ridge)
    return p, fold_weights(48, 4)


def rows_case():
    """folds_case under the linear row x1 + x2 + x3 = 0.3 and bounds -0.05 <= x <= 0.6: (p, lay, [offsets] * 3)"""
    A, t, ev = survival_data()
    base = cox_block_model(A, t, ev, 0.5)
    rng = np.random.default_rng(44)
    shifts = [0.5 * rng.standard_normal(48) for _ in range(3)]
    n = 3
    terms = [(0, 0.25, [(j + 1, POW, 2)]) for j in range(n)] + [(1, 1.0, [(j + 1, POW)]) for j in range(n)]
    p = make_nlp_terms(n, 1, 1, terms, xL=np.full(n, -0.05), xU=np.full(n, 0.6), gL=[0.3], gU=[0.3], x0=np.full(n, 0.1),
                       blocks=[dataclasses.replace(base.blocks[0], shift=shifts[0])])
    return p, nlp_terms_layout(p), shifts


def queue_case():
    """Five scenarios of the folds data for a queue of two slots: the four fold weights and unit weights, each with its own small
    offsets.  (p with unit weights and zero offsets, lay, [(weight, offsets)] * 5)"""
    p, W = folds_case()
    rng = np.random.default_rng(45)
    scen = [(w, 0.2 * rng.standard_normal(48)) for w in list(W) + [np.ones(48)]]
    return p, nlp_terms_layout(p), scen
