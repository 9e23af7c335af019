"""CPU tests (no GPU) of the structures the multifrontal kernel tests run (tests/mf_structures.py): the generator builds the
plan shapes it names (sqphip_mf_plan_info), and on every family and value set the library's host reference of the numeric
phase agrees with numpy on an independently assembled dense Newton matrix -- inertia, log |det|, backward error."""
import numpy as np
import pytest

import sqpsolver_jl_amd as pkg
import mf_structures as MS

FAMILIES = MS.families()
# normwise backward error of the host reference, calibrated on these families (largest seen: well 9e-17, indef 1.7e-16,
# ipm 9e-19): a factor of about 100 above that
BE_BOUND = {"well": 1e-14, "indef": 2e-14, "ipm": 1e-16}


def _plan(S, cond=1, batch=5):
    return pkg.mf_plan_info(S.n, S.m, S.jrow, S.jcol, S.hrow, S.hcol, S.gL, S.gU, cond, batch)


def test_the_families_cover_every_front_height_and_launch_shape():
    """Every claim of a family holds for the plan sqphip_create builds: the single fronts have exactly the rows they name
    (rows + 1 = 16 T - 1, 16 T, 16 T + 1 for T = 1 .. 14, and 300 / 511 / 1000); the level families give launches whose
    fronts differ in T, narrow and wide, merged at small batches and per class at large ones; the column counts modulo 4
    and the top fronts on both sides of the streamed top-of-tree solve's limits occur."""
    heights = set()
    for S in FAMILIES:
        fr, la, top2, _ = _plan(S)
        rows = fr[:, 0] + fr[:, 1]
        t = S.target
        if "max_rows" in t:
            assert rows.max() == t["max_rows"], (S.name, rows.max())
            assert la[:, 1].max() == t["max_tiles"], S.name
            heights.add(int(rows.max()) + 1)
        # launches: (level, tiles of the kernel, fronts, tiles of the smallest front); a level of more than 8 fronts is wide
        wide = np.flatnonzero(np.bincount(fr[:, 2]) > 8)
        mixed = [L_ for L_ in la if L_[3] < L_[1]]          # launches that run a front in a kernel of more tiles
        if t.get("mixed_launch"):
            assert mixed, S.name
        if t.get("narrow"):
            # a narrow level (2 .. 8 fronts) in ONE launch of its tallest front's kernel, with a shorter front in it
            assert any(1 < L_[2] <= 8 and L_[3] < L_[1] for L_ in la), S.name
        if t.get("wide") == "merged":
            # batch <= 64: the wide level of small fronts is one launch, with shorter fronts in it; batch > 64: per class
            assert len(wide) == 1 and (la[:, 0] == wide[0]).sum() == 1, S.name
            assert any(L_[0] == wide[0] and L_[2] > 8 for L_ in mixed), S.name
            _, la_big, _, _ = _plan(S, batch=65)
            assert (la_big[:, 0] == wide[0]).sum() > 1, S.name
        if t.get("wide") == "classes":
            # the wide level goes per class at any batch, and a class launch runs a shorter front of its class
            assert len(wide) == 1 and (la[:, 0] == wide[0]).sum() > 1, S.name
            assert any(L_[0] == wide[0] and L_[2] > 1 for L_ in mixed), S.name
        if "min_tiles" in t:
            assert la[:, 1].max() >= t["min_tiles"], S.name
        if "nc_mod4" in t:
            assert any((fr[:, 0] % 4) == t["nc_mod4"]), S.name
        if "nc1" in t:
            # isolated variables: root fronts of one column and no rows, as many as the family has
            assert ((fr[:, 0] == 1) & (fr[:, 1] == 0)).sum() == t["nc1"], (S.name, fr)
        if "root_cols" in t:
            assert fr[fr[:, 1] == 0, 0].max() == t["root_cols"], S.name
            assert (top2 > 0) == t["top2"], (S.name, top2)
    for T in range(1, 15):
        assert {16 * T - 1, 16 * T, 16 * T + 1} - {1} <= heights | {1}, T
    assert {301, 512, 1001} <= heights


@pytest.mark.parametrize("kind", MS.VALUE_SETS)
def test_host_reference_matches_numpy_on_every_family(kind):
    """For every family, condensed and full form: inertia from the host reference's pivot signs = eigvalsh sign count,
    sum log |D| = slogdet, and the normwise backward error (residual in long double) below a bound calibrated here."""
    worst = 0.0
    for i, S in enumerate(FAMILIES):
        for cond in ((1, 0) if S.n <= 300 else (1,)):
            Jv, Hv, Dd, sigp, hd, rt, hsc = MS.values(S, kind, 100 + i)
            dw = 1e-3 if kind == "well" else 0.0
            K = MS.dense_newton(S, cond, Jv, Hv, Dd, sigp, hd, rt, hsc, dw)
            rhs = np.random.default_rng(i).normal(size=K.shape[0])
            sol, dinv, npos = pkg.mf_host_solve(S.n, S.m, S.jrow, S.jcol, S.hrow, S.hcol, S.gL, S.gU, cond, Jv, Hv, Dd, sigp,
                                                hd, rt, hsc, dw, rhs)
            assert np.all(np.isfinite(dinv)) and np.all(dinv != 0), S.name
            if kind != "ipm":       # eigenvalues down to ~1e-9 against a norm of 1e9 are below eigvalsh's resolution
                ev = np.linalg.eigvalsh(K)
                assert npos == int((ev > 0).sum()), (S.name, cond, npos)
            sign, logdet = np.linalg.slogdet(K)
            assert sign == np.prod(np.sign(dinv)), S.name          # det K = prod D, L unit lower
            assert abs(-np.log(np.abs(dinv)).sum() - logdet) <= 1e-8 * max(1.0, abs(logdet)) + 1e-6, (S.name, cond)
            be = MS.backward_error(K, sol, rhs)
            worst = max(worst, be)
            assert be <= BE_BOUND[kind], (S.name, cond, be)
            if kind == "well":
                assert npos == S.n
            if kind == "indef" and cond == 1 and S.n >= 40:
                assert npos < S.n, S.name
    print(f"{kind}: worst backward error {worst:.1e}")


def test_streamed_top_and_spine_replays_pass_wherever_they_exist(monkeypatch):
    """The host replays of the streamed top-of-tree solve (k_mf_solve_top2) and of the spine kernel's front assembly
    (k_mf_spine) from their own plan arrays reproduce the plain recursion on every family that has them."""
    monkeypatch.setenv("SQPHIP_MF_SPINE", "1")
    seen_top = seen_spine = 0
    for i, S in enumerate(FAMILIES):
        if S.n > 300:
            continue
        Jv, Hv, Dd, sigp, hd, rt, hsc = MS.values(S, "well", 7 + i)
        rhs = np.random.default_rng(i).normal(size=S.nu(1))
        pkg.mf_host_solve(S.n, S.m, S.jrow, S.jcol, S.hrow, S.hcol, S.gL, S.gU, 1, Jv, Hv, Dd, sigp, hd, rt, hsc, 1e-3, rhs)
        err, serr = pkg.mf_host_top2_err(), pkg.mf_host_spine_err()
        assert err == -1.0 or 0.0 <= err <= 1e-12, (S.name, err)
        assert serr == -1.0 or 0.0 <= serr <= 1e-13, (S.name, serr)
        seen_top += err >= 0; seen_spine += serr >= 0
    assert seen_top >= 4 and seen_spine >= 4, (seen_top, seen_spine)
