"""CPU checks of what the dense LDL^T device tests (test_gpu_ldlt_cases.py) stand on: the long-double reference against
50-digit arithmetic, the oracle's fp64 factorisation against the long-double reference within the bounds the device is
held to (so a family that breaks a bound by itself fails here, before any GPU is involved), the inertia of every family
against its construction and Sylvester's law, and the structure of the tiled cases together with the masks and pair
lists the device hook derives from them."""
import ctypes as C

import numpy as np
import pytest

import ldlt_cases as LC
from oracle import oracle as O
from sqpsolver_jl_amd import _lib

CPU_SIZES = [1, 2, 63, 64, 65, 257, 600]


def _oracle_factor(A):
    a, dinv, npos, _ = O.ldlt_factor(A, A.shape[0])
    return np.tril(a, -1) + np.eye(A.shape[0]), dinv, npos


@pytest.mark.parametrize("family", sorted(LC.FAMILIES))
@pytest.mark.parametrize("N", [1, 2, 63, 64, 65])
def test_long_double_reference_matches_mpmath(family, N):
    A = LC.FAMILIES[family](N, LC.default_n1(N), 3)
    L, d = LC.ldl_reference(A)
    M, dm = LC.ldl_mpmath(A, 50)
    eps = float(np.finfo(LC.LD).eps)
    assert eps <= 2.0 ** -63, "numpy.longdouble has no 64-bit mantissa on this host"
    # long double against the 50-digit factors, relative: L against max(1, max |L|), every pivot against itself
    scale = max(1.0, float(np.abs(L).max()))
    el = max((float(abs(M[i][j] - _mpf(L[i, j]))) for i in range(N) for j in range(i)), default=0.0) / scale
    ed = max(float(abs((dm[j] - _mpf(d[j])) / dm[j])) for j in range(N))
    print(f"{family} N={N}: long double vs mpmath: L {el:.1e} d {ed:.1e}")
    # long double carries 11 more bits than fp64: its error must sit far below the fp64 effects the tests measure (1e-12)
    assert el < 1e-14 and ed < 1e-14
    assert [int(x > 0) for x in dm] == (d > 0).astype(int).tolist()


def _mpf(x):
    """Exact conversion of a long double to mpmath (two fp64 pieces)."""
    import mpmath
    hi = float(x)
    return mpmath.mpf(hi) + mpmath.mpf(float(x - LC.LD(hi)))


@pytest.mark.parametrize("family", sorted(LC.FAMILIES))
@pytest.mark.parametrize("N", CPU_SIZES)
def test_oracle_factorisation_within_the_device_bounds(family, N):
    n1 = LC.default_n1(N)
    A = LC.FAMILIES[family](N, n1, 21)
    Lr, dr = LC.ldl_reference(A)
    Lo, dinv_o, npos_o = _oracle_factor(A)
    do = 1.0 / dinv_o
    be, at = LC.backward_error_full(A, Lo, do)
    eL, ed = LC.rel(Lo, Lr.astype(float)), LC.rel(dinv_o, (1 / dr).astype(float))
    print(f"{family} N={N}: oracle backward error {be / LC.U:.1f} u at {at} (bound {LC.gamma_factor(N) / LC.U:.0f} u), "
          f"e_ref L {eL:.1e} dinv {ed:.1e}")
    assert be <= LC.gamma_factor(N)
    assert np.array_equal(np.sign(dinv_o), np.sign(dr.astype(float)))
    assert npos_o == int((dr > 0).sum()) == LC.expected_npos(family, N, n1)
    if family != "ipm_end":
        assert eL < 1e-12 and ed < 1e-12
        assert int((np.linalg.eigvalsh(A) > 0).sum()) == npos_o            # Sylvester
    b = np.random.default_rng(5).standard_normal(N)
    a_o = np.asfortranarray(np.tril(Lo, -1) + np.diag(np.ones(N)))
    xo = O.ldlt_solve(a_o, dinv_o, b)
    rr = LC.residual_ratio(A, Lo, do, xo, b)
    print(f"   solution residual {rr / LC.U:.1f} u (bound {LC.gamma_solve(N) / LC.U:.0f} u)")
    assert rr <= LC.gamma_solve(N)
    if family != "ipm_end":
        _, _, xr = LC.solve_reference(Lr, dr, b)
        assert LC.rel(xo, xr.astype(float)) < 1e-11


def _tile_masks(As, Ts):
    L = _lib.lib()
    B, N = len(As), As[0].shape[0]
    T = (N + 63) // 64
    Tr = T - Ts
    Af = np.ascontiguousarray(np.stack([np.tril(a).ravel(order="F") for a in As]))
    tm = np.zeros(max(1, Tr * Ts), dtype=np.uint8)
    pp = np.zeros(Tr * (Tr + 1) // 2 + 1, dtype=np.int32)
    cap = max(1, Tr * (Tr + 1) // 2 * Ts)
    pk = np.zeros(cap, dtype=np.int32)
    nk = C.c_int32(-1)
    ip = C.POINTER(C.c_int32)
    rc = L.sqphip_ldlt_tile_masks(B, N, Af.ctypes.data_as(C.POINTER(C.c_double)), Ts, tm.ctypes.data_as(C.POINTER(C.c_uint8)),
                                  pp.ctypes.data_as(ip), pk.ctypes.data_as(ip), cap, C.byref(nk))
    return rc, tm[:Tr * Ts].reshape(Tr, Ts), pp, pk[:max(nk.value, 0)]


@pytest.mark.parametrize("case", LC.TILED_CASES, ids=lambda c: "-".join(map(str, c)))
def test_tiled_cases_structure_masks_and_inertia(case):
    Ts, Tr, pattern, values = case
    As, infos = zip(*[LC.tiled(Ts, Tr, pattern, 40 + b, values) for b in range(2)])
    info = infos[0]
    N = info["N"]
    assert (N + 63) // 64 == Ts + Tr and (Tr == 0 or N % 64 == LC.REM_LAST)
    for A, inf in zip(As, infos):
        assert np.array_equal(A, A.T) and LC.leading_block_is_block_diagonal(A, Ts)
        pad = np.arange(64 * (Ts - 1) + LC.LEAD_FILL, 64 * Ts)
        assert np.array_equal(A[pad], np.eye(N)[pad])                       # identity rows inside the last leading tile
        Lo, dinv_o, npos_o = _oracle_factor(A)
        be = LC.backward_error_full(A, Lo, 1.0 / dinv_o)[0] if N <= 600 else LC.backward_error_sampled(A, Lo, 1.0 / dinv_o, 3)[0]
        assert be <= LC.gamma_factor(N)
        assert npos_o == inf["npos"]
        if values == "well_scaled":
            assert int((np.linalg.eigvalsh(A) > 0).sum()) == npos_o
    rc, tm, pp, pk = _tile_masks(As, Ts)
    assert rc == 0
    assert np.array_equal(tm, LC.derived_mask(As, Ts))
    if values == "well_scaled":
        assert np.array_equal(tm, info["mask"])          # dense blocks: exactly the intended coupling
    else:
        assert not np.any(tm & ~info["mask"].astype(bool))
    assert len(pp) == Tr * (Tr + 1) // 2 + 1 and pp[0] == 0 and np.all(np.diff(pp) >= 0) and pp[-1] == len(pk)
    for ti in range(Tr):
        for tj in range(ti + 1):
            pi = ti * (ti + 1) // 2 + tj
            assert pk[pp[pi]:pp[pi + 1]].tolist() == np.flatnonzero(tm[ti] & tm[tj]).tolist()
    if pattern == "single":
        assert all(pp[ti * (ti + 1) // 2 + tj + 1] == pp[ti * (ti + 1) // 2 + tj] for ti in range(Tr) for tj in range(ti))


def test_tile_masks_refuse_coupled_leading_tiles():
    A, _ = LC.tiled(2, 1, "all", 7)
    A[70, 3] = A[3, 70] = 0.5
    rc, *_ = _tile_masks([A], 2)
    assert rc != 0


def test_stratified_sample_reaches_every_tile():
    for N in (65, 600, 833):
        I, J = LC.stratified_sample(N, 1)
        assert np.all(I >= J) and np.all(I < N)
        T = (N + 63) // 64
        cnt = np.zeros((T, T), int)
        np.add.at(cnt, (I // 64, J // 64), 1)
        for ti in range(T):
            for tj in range(ti + 1):
                h, w = min(64, N - 64 * ti), min(64, N - 64 * tj)
                full = h * (h + 1) // 2 if ti == tj else h * w
                assert cnt[ti, tj] >= min(64, full)
        A = LC.well_scaled(N, LC.default_n1(N), 2)
        Lo, dinv_o, _ = _oracle_factor(A)
        full, _ = LC.backward_error_full(A, Lo, 1 / dinv_o)
        samp, _, _ = LC.backward_error_sampled(A, Lo, 1 / dinv_o, 1)
        assert 0 < samp <= full
        # a wrong off-diagonal tile cannot hide from the sample: perturb tile (ti, tj), ti > tj, of L only -- in the lower
        # triangle of L D L' that changes tile row ti right of column tile tj - 1 (the diagonal tile (ti, ti) too) and the tiles
        # (r, ti) below it; judge the sample by the entries of the OFF-DIAGONAL tile (ti, tj) itself, without the diagonal's help
        for ti, tj in ((1, 0), (T - 1, 0), (T - 1, max(0, T - 3))):
            if ti <= tj or ti >= T:
                continue
            Lbad = Lo.copy()
            Lbad[64 * ti:64 * ti + 64, 64 * tj:64 * tj + 64] *= (1 + 1e-9)
            in_tile = (I // 64 == ti) & (J // 64 == tj)
            assert in_tile.sum() >= 64
            ratio = _sample_ratios(A, Lbad, 1 / dinv_o, I[in_tile], J[in_tile])
            assert ratio.max() > LC.gamma_factor(N), (N, ti, tj)
            assert LC.backward_error_sampled(A, Lbad, 1 / dinv_o, 1)[0] > LC.gamma_factor(N)


def _sample_ratios(A, L, d, I, J):
    Lq = L.astype(LC.LD)
    prod = np.einsum("ek,ek->e", Lq[I] * d.astype(LC.LD), Lq[J])
    bound = np.einsum("ek,ek->e", np.abs(L[I] * d), np.abs(L[J]))
    return np.abs(prod - A[I, J].astype(LC.LD)).astype(float) / np.maximum(bound, np.finfo(float).tiny)
