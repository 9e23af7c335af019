"""Seeded matrices, a long-double reference and the error bounds of the dense LDL^T tests (numpy only).

Families (each with the inertia known by construction):
  well_scaled  the quasi-definite family of test_gpu_parity.py: condition number about 2, inertia (n1, N - n1)
  ipm_end      [[H + diag(|H| 1 + Sigma), J'], [J, -D]], Sigma = 10^U(-8, 8), D = 10^U(-8, 2): the scales at the end of an
               interior-point run; quasi-definite, so LDL^T without pivoting exists and the inertia is (n1, N - n1)
  flipped      strictly diagonally dominant, the sign of the diagonal flipped at {0, 63, 64, N // 2, N - 1}: the number of
               positive pivots is NOT n1
  tiled        Ts independent leading tiles (block-diagonal leading block, identity padding inside the last one), a dense
               remainder of Tr tiles (the last one partial) and coupling blocks by pattern; values of well_scaled or ipm_end

Reference: the textbook right-looking LDL^T without pivoting in numpy.longdouble (64-bit mantissa on x86), validated
against 50-digit mpmath in test_ldlt_cases_cpu.py.

Bounds (u = 2^-53): with L and D = 1 / dinv as a factorisation returned them,
  |L D L' - A| <= gamma_factor(N) |L||D||L'|            (Higham, Accuracy and Stability, Thm 10.3 and its proof)
  |b - A x|    <= gamma_solve(N)  |L||D||L'||x|         (Thm 10.4)
componentwise; see gamma_factor / gamma_solve for the constants."""
from __future__ import annotations

import numpy as np

LD = np.longdouble
U = 2.0 ** -53
FULL_LD_MAX = 257          # up to this order the device tests use the full long-double reference and product


# ------------------------------------------------------------------------------------------------ bounds
def gamma(k):
    return k * U / (1.0 - k * U)


def gamma_factor(N):
    """Entry (i, j) of L D L' is a sum of at most N products l_ik d_k l_jk; the elimination computed a_ij minus the first
    j of them and then one scaling by 1 / d_j.  Higham's Lemma 8.4 / Thm 10.3 bounds the accumulated error of that
    recurrence by gamma_{N+1} times sum |l_ik||d_k||l_jk| for ANY order of the summation (so the MFMA blocking, the
    left-looking panels and the rank-256 updates are covered).  Two more roundings are not in the textbook recurrence: the
    kernel multiplies by a Newton reciprocal 1 / d_j that is within 1 ulp (instead of dividing, half an ulp), and the
    test forms D = 1 / dinv (half an ulp): (1 + u)^2 more at most.  gamma_{N+1} + the two -> gamma_{N+4} (Lemma 3.3:
    gamma_j + gamma_k + gamma_j gamma_k <= gamma_{j+k}, with one unit to spare)."""
    return gamma(N + 4)


def gamma_solve(N):
    """Thm 10.4 for the two triangular solves and the diagonal scaling behind a factorisation with the bound above:
    gamma_{3N+1} in the textbook; the reciprocal pivots add the same three units as in gamma_factor."""
    return gamma(3 * N + 4)


# ------------------------------------------------------------------------------------------------ reference
def ldl_reference(A, dtype=LD):
    """Textbook right-looking LDL^T without pivoting: returns (L unit lower, d).  Same elimination order as the kernels
    (column j is finished, then its rank-1 update is applied to everything to its right)."""
    A = np.array(A, dtype=dtype)
    N = A.shape[0]
    d = np.zeros(N, dtype)
    for j in range(N):
        d[j] = A[j, j]
        l = A[j + 1:, j] / d[j]
        A[j + 1:, j + 1:] -= np.outer(l, A[j + 1:, j])
        A[j + 1:, j] = l
    return np.tril(A, -1) + np.eye(N, dtype=dtype), d


def solve_reference(L, d, b):
    """Forward elimination, diagonal scaling, backward substitution with (L, d): returns (y, v, x), y = L^-1 b,
    v = D^-1 y, x = L^-T v, in the precision of L."""
    dt = L.dtype
    N = L.shape[0]
    y = np.array(b, dtype=dt)
    for j in range(N):
        y[j + 1:] -= L[j + 1:, j] * y[j]
    v = y / d
    x = v.copy()
    for j in range(N - 1, -1, -1):
        x[:j] -= L[j, :j] * x[j]
    return y, v, x


def ldl_mpmath(A, digits=50):
    """The same elimination in mpmath (validation of the long-double routine at small N)."""
    import mpmath
    mpmath.mp.dps = digits
    N = A.shape[0]
    M = [[mpmath.mpf(float(A[i, j])) for j in range(N)] for i in range(N)]
    d = [None] * N
    for j in range(N):
        d[j] = M[j][j]
        for i in range(j + 1, N):
            M[i][j] = M[i][j] / d[j]
        for c in range(j + 1, N):
            w = M[c][j] * d[j]
            if w == 0:
                continue
            for i in range(c, N):
                M[i][c] -= M[i][j] * w
    return M, d


# ------------------------------------------------------------------------------------------------ families
def well_scaled(N, n1, seed):
    """quasi_definite of test_gpu_parity.py, unchanged."""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((N, N)) * 0.3
    A = (A + A.T) / 2
    A[np.diag_indices(N)] = np.concatenate([np.ones(n1), -np.ones(N - n1)]) * (
        0.9 * np.sqrt(N) + rng.uniform(0.5, 1.5, N))
    return A


def ipm_end(N, n1, seed):
    rng = np.random.default_rng(seed)
    m = N - n1
    J = rng.standard_normal((m, n1)) * (rng.uniform(size=(m, n1)) < min(1, 6 / max(n1, 1)))
    H = rng.standard_normal((n1, n1)) * (rng.uniform(size=(n1, n1)) < min(1, 4 / max(n1, 1)))
    H = 0.1 * (H + H.T)
    sig = 10.0 ** rng.uniform(-8, 8, n1)
    D = 10.0 ** rng.uniform(-8, 2, m)
    W = H + np.diag(np.abs(H).sum(1) + sig)
    return np.block([[W, J.T], [J, -np.diag(D)]])


FLIP_AT = (0, 63, 64)


def flip_positions(N):
    return sorted({i for i in FLIP_AT + (N // 2, N - 1) if 0 <= i < N})


def flipped(N, n1, seed):
    A = well_scaled(N, n1, seed)
    A[np.diag_indices(N)] = np.sign(np.diag(A)) * np.abs(A).sum(1)       # strictly dominant
    for i in flip_positions(N):
        A[i, i] = -A[i, i]
    return A


FAMILIES = {"well_scaled": well_scaled, "ipm_end": ipm_end, "flipped": flipped}


def default_n1(N):
    return max(1, N * 2 // 5) if N > 1 else 1


def expected_npos(family, N, n1):
    """Positive pivots by construction (Sylvester: quasi-definite -> n1; dominant -> positive diagonal entries)."""
    if family != "flipped":
        return n1
    s = np.concatenate([np.ones(n1), -np.ones(N - n1)])
    for i in flip_positions(N):
        s[i] = -s[i]
    return int((s > 0).sum())


def plain_sizes():
    """N = 64 T - 1, 64 T, 64 T + 1 for T = 1 .. 13 (every last-panel length, both parities of the panel solve's row pairs),
    the look-ahead threshold T = 23, 24, 25 at 64 T - 1 and 64 T, and the degenerate orders."""
    s = {1, 2, 63}
    for T in range(1, 14):
        s |= {64 * T - 1, 64 * T, 64 * T + 1}
    for T in (23, 24, 25):
        s |= {64 * T - 1, 64 * T}
    return sorted(s)


# ------------------------------------------------------------------------------------------------ tiled
PATTERNS = ("all", "half", "rem_none", "lead_none", "single")
LEAD_FILL = 40          # occupied slots of the last leading tile (the rest: identity rows, as order.hip pads)
REM_LAST = 37           # rows of the last (partial) remainder tile


def tiled_mask(Ts, Tr, pattern):
    """Intended coupling mask [Tr][Ts] (the same for every instance of a batch: a function of the shape only)."""
    rng = np.random.default_rng(1000 + 31 * Ts + Tr)
    m = np.ones((Tr, Ts), dtype=np.uint8)
    if pattern == "half":
        m = (rng.uniform(size=(Tr, Ts)) < 0.5).astype(np.uint8)
        if Tr and not m.any():
            m[Tr - 1, 0] = 1
    elif pattern == "rem_none" and Tr:
        m[Tr // 2, :] = 0               # one remainder tile coupled to no leading tile
    elif pattern == "lead_none" and Tr:
        m[:, Ts // 2] = 0               # one leading tile coupled to no remainder tile
    elif pattern == "single":           # remainder tile r -> leading tile r only (none when r >= Ts): no two remainder
        m[:] = 0                        # tiles share a leading tile, every off-diagonal pair list is empty
        for r in range(min(Tr, Ts)):
            m[r, r] = 1
    elif pattern not in PATTERNS:
        raise ValueError(pattern)
    return m


def tiled(Ts, Tr, pattern, seed, values="well_scaled"):
    """Returns (A, info): A of order N = 64 Ts + 64 (Tr - 1) + REM_LAST (64 Ts when Tr = 0); info: N, npos (by construction),
    mask (intended tmask).  Unknowns in the order [leading variables | remainder variables | remainder rows]; the slots
    64 (Ts - 1) + LEAD_FILL .. 64 Ts - 1 are identity rows."""
    nrem = 64 * (Tr - 1) + REM_LAST if Tr > 0 else 0
    N = 64 * Ts + nrem
    pad = np.arange(64 * (Ts - 1) + LEAD_FILL, 64 * Ts)
    real = np.setdiff1d(np.arange(N), pad)
    nvar = 64 * Ts - len(pad) + nrem // 3
    base = FAMILIES[values](len(real), nvar, seed)
    A = np.eye(N)
    A[np.ix_(real, real)] = base
    mask = tiled_mask(Ts, Tr, pattern)
    tile = np.arange(N) // 64
    for a in range(Ts):                                  # independent leading tiles
        for b in range(Ts):
            if a != b:
                A[np.ix_(tile == a, tile == b)] = 0.0
    for r in range(Tr):
        for k in range(Ts):
            if not mask[r, k]:
                A[np.ix_(tile == Ts + r, tile == k)] = 0.0
                A[np.ix_(tile == k, tile == Ts + r)] = 0.0
    return A, {"N": N, "npos": nvar + len(pad), "mask": mask, "Ts": Ts, "Tr": Tr}


# (Ts, Tr, pattern, values): every (Ts, Tr) of the list, every pattern at (2, 5) and (5, 4), one with the look-ahead
# running behind the leading tiles (Tr >= 24)
TILED_CASES = [
    (1, 1, "all", "well_scaled"), (1, 2, "half", "ipm_end"), (2, 1, "lead_none", "well_scaled"),
    (2, 5, "all", "ipm_end"), (2, 5, "half", "well_scaled"), (2, 5, "rem_none", "ipm_end"),
    (2, 5, "lead_none", "well_scaled"), (2, 5, "single", "ipm_end"),
    (5, 4, "all", "well_scaled"), (5, 4, "half", "ipm_end"), (5, 4, "rem_none", "well_scaled"),
    (5, 4, "lead_none", "ipm_end"), (5, 4, "single", "well_scaled"),
    (5, 9, "half", "well_scaled"), (5, 9, "single", "ipm_end"), (5, 9, "rem_none", "ipm_end"),
    (3, 0, "all", "well_scaled"), (3, 0, "all", "ipm_end"),
    (2, 24, "half", "well_scaled"),
]


def leading_block_is_block_diagonal(A, Ts):
    n = min(64 * Ts, A.shape[0])
    t = np.arange(n) // 64
    return not np.any(A[:n, :n][t[:, None] != t[None, :]])


def derived_mask(As, Ts):
    """tmask [Tr][Ts] from the zero blocks of a batch of matrices (what the hook does on the host)."""
    N = As[0].shape[0]
    T = (N + 63) // 64
    m = np.zeros((T - Ts, Ts), dtype=np.uint8)
    for A in As:
        for r in range(T - Ts):
            for k in range(Ts):
                if np.any(A[64 * (Ts + r):64 * (Ts + r + 1), 64 * k:64 * (k + 1)]):
                    m[r, k] = 1
    return m


# ------------------------------------------------------------------------------------------------ checks
def pad_to_tiles(A):
    """A with identity padding up to a multiple of 64 (what the device factorises)."""
    N = A.shape[0]
    Npad = (N + 63) // 64 * 64
    P = np.eye(Npad, dtype=A.dtype)
    P[:N, :N] = A
    return P


def backward_error_full(A, L, d, dtype=LD):
    """max over the lower triangle of |L D L' - A| / (|L||D||L'|), product in `dtype`; returns (ratio, (i, j))."""
    Lq = np.asarray(L, dtype=dtype)
    dq = np.asarray(d, dtype=dtype)
    E = np.abs((Lq * dq) @ Lq.T - np.asarray(A, dtype=dtype))
    S = (np.abs(Lq) * np.abs(dq)) @ np.abs(Lq).T
    R = np.tril(E / np.maximum(S, np.finfo(np.float64).tiny))
    k = int(np.argmax(R))
    return float(R.flat[k]), divmod(k, R.shape[1])


def stratified_sample(N, seed, per_tile=64):
    """The whole diagonal and per_tile seeded entries of every 64 x 64 tile of the lower triangle of an N x N matrix."""
    rng = np.random.default_rng(seed)
    T = (N + 63) // 64
    I, J = [np.arange(N)], [np.arange(N)]
    for ti in range(T):
        for tj in range(ti + 1):
            h, w = min(64, N - 64 * ti), min(64, N - 64 * tj)
            if ti == tj:
                ii, jj = np.tril_indices(h)
                pick = rng.permutation(len(ii))[:per_tile]
                ii, jj = ii[pick], jj[pick]
            else:
                pick = rng.permutation(h * w)[:per_tile]
                ii, jj = pick // w, pick % w
            I.append(64 * ti + ii)
            J.append(64 * tj + jj)
    return np.concatenate(I), np.concatenate(J)


def backward_error_sampled(A, L, d, seed, per_tile=64):
    """The same ratio on stratified_sample: returns (ratio, (i, j), number of entries).  The product (where the
    cancellation is) in long double, one tile column at a time over the columns k < 64 (tj + 1) that can contribute; the
    bound is a sum of non-negative terms and loses nothing in fp64."""
    N = A.shape[0]
    I, J = stratified_sample(N, seed, per_tile)
    L = np.asarray(L, dtype=np.float64)
    d = np.asarray(d, dtype=np.float64)
    Lq = L.astype(LD)
    Ld = Lq * d.astype(LD)
    aL, aLd = np.abs(L), np.abs(L * d)
    worst, where = 0.0, (0, 0)
    tiny = np.finfo(np.float64).tiny
    for tj in range((N + 63) // 64):
        sel = np.flatnonzero(J // 64 == tj)
        i, j, kmax = I[sel], J[sel], min(N, 64 * (tj + 1))
        prod = np.einsum("ek,ek->e", Ld[i, :kmax], Lq[j, :kmax])
        bound = np.einsum("ek,ek->e", aLd[i, :kmax], aL[j, :kmax])
        r = np.abs(prod - A[i, j].astype(LD)).astype(np.float64) / np.maximum(bound, tiny)
        k = int(np.argmax(r))
        if float(r[k]) > worst:
            worst, where = float(r[k]), (int(i[k]), int(j[k]))
    return worst, where, len(I)


def residual_ratio(A, L, d, x, b):
    """max_i |b - A x|_i / (|L||D||L'||x|)_i: the residual in long double, the bound (non-negative terms) in fp64."""
    r = np.abs(np.asarray(b, dtype=LD) - np.asarray(A, dtype=LD) @ np.asarray(x, dtype=LD)).astype(np.float64)
    aL = np.abs(np.asarray(L, dtype=np.float64))
    s = aL @ (np.abs(d) * (aL.T @ np.abs(x)))
    return float((r / np.maximum(s, np.finfo(np.float64).tiny)).max())


def rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.abs(a - b).max() / max(1.0, float(np.abs(b).max())))
