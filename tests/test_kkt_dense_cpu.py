"""The order, tiles and coupling masks of the dense Newton path (sqphip_kkt_order_info: what sqphip_create sets up, host
only) on the structures of tests/kkt_dense_cases.py, against the pattern of the entry-wise reference
(tests/kkt_dense_ref.py); and that reference against the independent dense assembly of tests/mf_structures.py."""
import numpy as np
import pytest

import sqpsolver_jl_amd as pkg
import mf_structures as MS
import kkt_dense_cases as KC
import kkt_dense_ref as KR

NAMES = list(KC.CASES)


def _info(case):
    S = case.S
    return pkg.kkt_order_info(S.n, S.m, S.jrow, S.jcol, S.hrow, S.hcol, S.gL, S.gU, case.cond, case.tile)


def _pattern(case, info):
    """T of the reference with every row active: the structural pattern of the lower triangle in factorised order"""
    S = case.S
    ones = (np.ones(len(S.jrow)), np.ones(len(S.hrow)), np.ones(S.m), np.ones(S.n), np.ones(S.n),
            np.where(S.eq, 1, 2).astype(np.int32), 1.0)
    return KR.reference_K(S, case.cond, info["pos"], info["Fpad"], ones, 0.0)[2]


@pytest.mark.parametrize("name", NAMES)
def test_order_and_padding(name):
    case = KC.CASES[name]
    info = _info(case)
    pos, Ts, Tr, Nf, Fpad = info["pos"], info["Ts"], info["Tr"], info["Nf"], info["Fpad"]
    assert info["nu"] == case.nu == len(pos)
    assert len(set(pos.tolist())) == len(pos) and pos.min() >= 0 and pos.max() < Nf <= Fpad == 64 * (Ts + Tr)
    if not (case.cond and case.tile):
        assert Ts == 0 and np.array_equal(pos, np.arange(case.nu))
    pad = np.setdiff1d(np.arange(Fpad), pos)
    assert all(p < 64 * Ts or p >= max(Nf, Fpad - 64) for p in pad), (name, pad)
    # the remainder is contiguous
    assert np.array_equal(np.sort(pos[pos >= 64 * Ts]), np.arange(64 * Ts, Nf))
    # every row that stays in the matrix lies behind every variable it couples to
    S = case.S
    kept, krow, urow = KR.structure_lists(S, case.cond)
    for i, (cols, _) in enumerate(KR._rows(S)):
        if kept[i]:
            assert (pos[urow[i]] > pos[cols]).all(), (name, i)


@pytest.mark.parametrize("name", NAMES)
def test_leading_tiles_are_independent_and_the_mask_is_sound(name, capsys):
    case = KC.CASES[name]
    info = _info(case)
    Ts, Tr, Fpad = info["Ts"], info["Tr"], info["Fpad"]
    T = _pattern(case, info)
    r, c = np.nonzero(np.tril(T))
    lead = 64 * Ts
    both = (r < lead) & (c < lead)
    assert (r[both] // 64 == c[both] // 64).all(), name
    panel = (r >= lead) & (c < lead)
    blocks = np.zeros((Tr, max(Ts, 1)), dtype=bool)
    blocks[(r[panel] - lead) // 64, c[panel] // 64] = True
    tm = info["tmask"].astype(bool)
    assert tm.shape == blocks.shape
    if info["masks"]:
        assert not (blocks & ~tm).any(), (name, np.argwhere(blocks & ~tm))
        with capsys.disabled():
            print(f"\n[mask] {name}: Ts {Ts} Tr {Tr} bits set {int(tm.sum())} of {tm.size}, set without an entry "
                  f"{int((tm & ~blocks).sum())} ({(tm & ~blocks).sum() / max(1, tm.sum()):.0%})")
    else:
        assert not tm.any()                # (no mask: the assembly zeroes the whole panel)
    ptr, ks = KR.pair_lists(Ts, Tr, tm)
    assert np.array_equal(ptr, info["pair_ptr"]) and np.array_equal(ks, info["pair_k"]), name


def test_the_tiled_structure_covers_every_branch_of_the_tile_order():
    case = KC.CASES["tiled8x24"]
    info = _info(case)
    S, pos, Ts, Tr = case.S, info["pos"], info["Ts"], info["Tr"]
    lead = 64 * Ts
    assert Ts >= 2 and Tr >= 2 and info["masks"]
    tm = info["tmask"]
    assert (tm == 0).any() and (tm == 1).any()
    pad = np.setdiff1d(np.arange(info["Fpad"]), pos)
    assert (pad < lead).any()                                        # a leading tile with padding slots
    kept, krow, urow = KR.structure_lists(S, 1)
    rows = KR._rows(S)
    assert any(pos[urow[i]] < lead for i in krow)                    # a kept row inside a leading tile
    assert any(not kept[i] and (pos[c] < lead).any() and (pos[c] >= lead).any() for i, (c, _) in enumerate(rows))
    assert any((pos[c] >= lead).all() for i, (c, _) in enumerate(rows))      # a row that touches no leading tile


@pytest.mark.parametrize("name", ["arrow256d", "arrow257d", "arrow257", "dense260"])
def test_the_long_column_cases_sit_where_they_claim(name):
    """the hub's column of the full symmetric pattern: 256 entries (serial walk) or 257 (long-column branch, `> 256`)"""
    for suffix in ("", "_tiled"):
        S = KC.CASES[name + suffix].S
        cnt = np.bincount(np.concatenate([S.hrow, S.hcol[S.hrow != S.hcol]]) - 1, minlength=S.n)
        want = {"arrow256d": 256, "arrow257d": 257, "arrow257": 257, "dense260": 260}[name]
        assert cnt[0] == want
        assert (cnt == 260).all() if name == "dense260" else cnt[1:].max() <= 2
        has_diag = bool(((S.hrow == 1) & (S.hcol == 1)).any())
        assert has_diag == (name != "arrow257")
    info = _info(KC.CASES[name + "_tiled"])
    assert info["Ts"] >= 1


def test_the_wide_case_is_above_the_vector_kernels_workgroup():
    assert _info(KC.CASES["wide1030"])["Fpad"] == 1088
    assert _info(KC.CASES["plain129"])["Fpad"] == 192 and _info(KC.CASES["plain65"])["Fpad"] == 128


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("kind", ["well", "ipm"])
def test_reference_matrix_unpermuted_is_the_dense_newton_matrix(name, kind):
    case = KC.CASES[name]
    info = _info(case)
    S, pos = case.S, info["pos"]
    v = KC.values(case, kind, 11)
    dw = 2e-3
    K, A, T = KR.reference_K(S, case.cond, pos, info["Fpad"], v, dw)
    Ks, As, Tsym = KR.symmetric(K), KR.symmetric(A), KR.symmetric(T)
    got = Ks[np.ix_(pos, pos)].astype(np.float64)
    want = MS.dense_newton(S, case.cond, *v[:6], v[6], dw)
    tol = 2 * KR.bound(As[np.ix_(pos, pos)], Tsym[np.ix_(pos, pos)])
    assert (np.abs(got - want) <= tol).all(), (name, float(np.abs(got - want).max()))
    if kind == "well":                 # (no term of this set is zero: the patterns agree)
        assert np.array_equal(want != 0, Tsym[np.ix_(pos, pos)] > 0)
    # padding: the identity
    pad = np.setdiff1d(np.arange(info["Fpad"]), pos)
    assert (np.diag(K)[pad] == 1).all() and not np.tril(K, -1)[:, pad].any() and not np.tril(K, -1)[pad, :].any()


def test_the_plain_ldlt_helper_solves():
    case = KC.CASES["plain65"]
    info = _info(case)
    v = KC.values(case, "well", 3)
    K = KR.symmetric(KR.reference_K(case.S, 1, info["pos"], info["Fpad"], v, 0.0)[0])
    L, D = KR.ldlt_nopivot(K.astype(np.float64))
    b = np.random.default_rng(0).normal(size=info["Fpad"])
    x = KR.solve_with(L, D, b)
    xl = KR.solve_long_double(K, b)
    assert np.abs(x - xl.astype(np.float64)).max() < 1e-12 * np.abs(x).max()
    assert int((D > 0).sum()) == case.S.n + (info["Fpad"] - info["nu"])
    xv, A, T = KR.reference_xv(case.S, 1, info["pos"], info["Fpad"], v, b[:case.S.n + case.S.m])
    pad = np.setdiff1d(np.arange(info["Fpad"]), info["pos"])
    assert not xv[pad].any() and not T[pad].any() and (T[info["pos"]] >= 1).all()
