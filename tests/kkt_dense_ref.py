"""Reference of the dense Newton path for the tests (numpy only; nothing from the library).

Entry-wise reference of what k_kkt_assemble writes, in factorised order, from the list of TERMS of every entry:

    hsc * h                      a structural Hessian entry                              (one rounding on the device)
    hd, sigp, dw, 1e-8           the four summands of a variable's diagonal              (none)
    j                            the Jacobian entry of a row that stays in the matrix    (none)
    -(D), -(1e-8)  |  -1         the diagonal of such a row  |  of a free one            (none)
    j_a * j_b / (D + 1e-8)       the share of an eliminated row                          (three: D + reg, the quotient, the product)

For every position of the lower triangle: the sum of its terms in long double, the sum of their absolute values A and their
count T.  The device forms every term with at most three roundings and adds the T terms of an entry one after the other
(T - 1 roundings), so it lies within (T + 2) u A (1 + O(u)) of the exact sum, u = 2^-53; the tests allow (T + 4) u A,
which also covers the second-order terms and the long-double reference (2^-64 per operation).  A position without terms
(T = 0) is structurally zero and must hold exactly 0.0; padding columns are exactly the identity.

The working vector of the solves (solve_vector_at) the same way: src_u for a variable or a row in the matrix, plus
j * b_i / (D_i + 1e-8) per eliminated row of the variable (three roundings each)."""
from __future__ import annotations

import numpy as np

LD = np.longdouble
U = 2.0 ** -53
REG = 1e-8


def structure_lists(S, cond):
    """kept (bool per row), krow (rows in the matrix, in order), unknown of each row or -1"""
    kept = S.kept(cond)
    krow = np.flatnonzero(kept)
    urow = np.full(S.m, -1)
    urow[krow] = S.n + np.arange(len(krow))
    return kept, krow, urow


def _rows(S):
    """per row: (columns, indices into the COO arrays); the structures of the tests have no duplicate entries"""
    order = np.argsort(S.jrow, kind="stable")
    cnt = np.bincount(S.jrow - 1, minlength=S.m)
    ptr = np.concatenate([[0], np.cumsum(cnt)])
    out = []
    for i in range(S.m):
        k = order[ptr[i]:ptr[i + 1]]
        cols = S.jcol[k] - 1
        assert len(set(cols.tolist())) == len(cols), "duplicate Jacobian entry"
        out.append((cols, k))
    return out


def terms(S, cond, pos, vals, dw):
    """The terms of every entry as (row position, column position, value in long double), row >= column."""
    Jv, Hv, Dd, sigp, hd, rt, hsc = vals
    n = S.n
    kept, krow, urow = structure_lists(S, cond)
    pos = np.asarray(pos)
    R, Cc, V = [], [], []

    def add(pa, pb, v):
        pa = np.atleast_1d(pa); pb = np.atleast_1d(pb)
        R.append(np.maximum(pa, pb)); Cc.append(np.minimum(pa, pb)); V.append(np.broadcast_to(np.asarray(v, dtype=LD), pa.shape))

    assert len({(int(a), int(b)) for a, b in zip(S.hrow, S.hcol)}) == len(S.hrow), "duplicate Hessian entry"
    add(pos[S.hrow - 1], pos[S.hcol - 1], LD(hsc) * Hv.astype(LD))
    pv = pos[:n]
    for d in (hd, sigp, np.full(n, dw), np.full(n, REG)):
        add(pv, pv, np.asarray(d, dtype=LD))
    for i, (cols, k) in enumerate(_rows(S)):
        ji = Jv[k].astype(LD)
        if kept[i]:
            pr = pos[urow[i]]
            if rt[i] == 0:
                add(pr, pr, LD(-1.0))
                continue
            add(pr, pr, -LD(Dd[i])); add(pr, pr, -LD(REG))
            add(np.full(len(cols), pr), pos[cols], ji)
        elif rt[i] != 0:
            a, b = np.tril_indices(len(cols))
            add(pos[cols[a]], pos[cols[b]], ji[a] * ji[b] / (LD(Dd[i]) + LD(REG)))
    return np.concatenate(R), np.concatenate(Cc), np.concatenate(V)


def _accumulate(F, r, c, v):
    K = np.zeros((F, F), dtype=LD); A = np.zeros((F, F), dtype=LD); T = np.zeros((F, F), dtype=np.int64)
    np.add.at(K, (r, c), v); np.add.at(A, (r, c), np.abs(v)); np.add.at(T, (r, c), 1)
    return K, A, T


def reference_K(S, cond, pos, Fpad, vals, dw):
    """(K, A, T), each Fpad x Fpad, lower triangle in factorised order (column = the smaller position); the strict upper
    triangle is zero and means nothing.  Padding positions: K = 1 on the diagonal, T = 0 everywhere (compared exactly)."""
    r, c, v = terms(S, cond, pos, vals, dw)
    K, A, T = _accumulate(Fpad, r, c, v)
    pad = np.ones(Fpad, bool); pad[np.asarray(pos)] = False
    assert not T[pad].any() and not T[:, pad].any()
    K[pad, pad] = 1.0
    return K, A, T


def symmetric(K):
    """the full symmetric matrix of a lower triangle"""
    return np.tril(K) + np.tril(K, -1).T


def reference_xv(S, cond, pos, Fpad, vals, rhs):
    """(xv, A, T), each Fpad long: the working vector of the solves from the full-length right-hand side [g; b]"""
    Jv, Hv, Dd, sigp, hd, rt, hsc = vals
    n = S.n
    kept, krow, urow = structure_lists(S, cond)
    pos = np.asarray(pos)
    P, V = [pos[:n]], [rhs[:n].astype(LD)]
    P.append(pos[urow[krow]]); V.append(rhs[n + krow].astype(LD))
    for i, (cols, k) in enumerate(_rows(S)):
        if not kept[i] and rt[i] != 0:
            P.append(pos[cols]); V.append(Jv[k].astype(LD) * LD(rhs[n + i]) / (LD(Dd[i]) + LD(REG)))
    p = np.concatenate(P); v = np.concatenate(V)
    x = np.zeros(Fpad, dtype=LD); A = np.zeros(Fpad, dtype=LD); T = np.zeros(Fpad, dtype=np.int64)
    np.add.at(x, p, v); np.add.at(A, p, np.abs(v)); np.add.at(T, p, 1)
    return x, A, T


def bound(A, T):
    return (T + 4) * U * A.astype(np.float64)


def compare(got, ref, A, T, lower=True):
    """(largest err / bound over the positions with terms, number of positions without terms that are not exactly zero,
    number of positions with terms outside their bound).  got: float64, the shape of ref; lower: matrices, lower triangle only."""
    got = np.asarray(got, dtype=np.float64)
    m = np.tril(np.ones(ref.shape, bool)) if lower and ref.ndim == 2 else np.ones(ref.shape, bool)
    has = m & (T > 0)
    err = np.abs(got.astype(LD) - ref).astype(np.float64)
    bd = bound(A, T)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(has & (bd > 0), err / bd, 0.0)
    # a position whose terms are all zero has bound 0: it must be exact too
    outside = int((has & (err > bd)).sum())
    nonzero = int((m & (T == 0) & (ref == 0) & (got != 0.0)).sum())
    return float(ratio.max()) if ratio.size else 0.0, nonzero, outside


def ldlt_nopivot(K):
    """Plain LDL^T without pivoting of a full symmetric matrix, float64: (L unit lower, D)."""
    A = np.array(K, dtype=np.float64)
    F = A.shape[0]
    L = np.eye(F); D = np.zeros(F)
    with np.errstate(all="ignore"):
        for k in range(F):
            D[k] = A[k, k]
            if k + 1 < F:
                c = A[k + 1:, k].copy()
                l = c / D[k]
                L[k + 1:, k] = l
                A[k + 1:, k + 1:] -= np.outer(l, c)
    return L, D


def solve_with(L, D, b):
    """x = L^-T D^-1 L^-1 b by substitution in float64"""
    F = len(D)
    y = np.array(b, dtype=np.float64)
    for k in range(F):
        y[k + 1:] -= L[k + 1:, k] * y[k]
    y = y / D
    for k in range(F - 1, -1, -1):
        y[:k] -= L[k, :k] * y[k]
    return y


def solve_long_double(Kl, b, steps=4):
    """The solution of K x = b to long-double accuracy for a well-conditioned K (long double, full symmetric): a float64
    solve refined with residuals taken in long double."""
    K64 = Kl.astype(np.float64)
    x = np.linalg.solve(K64, np.asarray(b, dtype=np.float64)).astype(LD)
    bl = np.asarray(b, dtype=LD)
    for _ in range(steps):
        r = bl - Kl @ x
        x = x + np.linalg.solve(K64, r.astype(np.float64)).astype(LD)
    return x


def pair_lists(Ts, Tr, tmask):
    """the pair lists of a coupling mask [Tr][Ts], rebuilt: per remainder tile pair (ti >= tj) the leading tiles both couple to"""
    ptr, ks = [0], []
    for ti in range(Tr):
        for tj in range(ti + 1):
            ks += [k for k in range(Ts) if tmask[ti, k] and tmask[tj, k]]
            ptr.append(len(ks))
    return np.array(ptr, dtype=np.int32), np.array(ks, dtype=np.int32)
