"""The dense Newton path between the sparse structure and the dense LDL^T (kkt_mode = 1): k_kkt_assemble in each of its
branches, the tile order and its masks, the working vector of the solves, the inertia test with identity padding inside
the matrix -- through sqphip_kkt_dense_test on the structures of tests/kkt_dense_cases.py, five distinct instances per
context with one inactive, against the entry-wise reference of tests/kkt_dense_ref.py.

Bounds.  Matrix and working vector: every entry within (T + 4) 2^-53 A of the long-double sum of its T terms (A: the sum
of their absolute values; derivation in tests/kkt_dense_ref.py), entries without terms exactly 0.0, padding exactly the
identity / 0.  Pivots, solutions and the decision: the rules and margins of tests/test_gpu_mf_structures.py."""
import numpy as np
import pytest

import sqpsolver_jl_amd as pkg
import mf_structures as MS
import kkt_dense_cases as KC
import kkt_dense_ref as KR

pytestmark = pytest.mark.gpu

B, IDLE, SENT = KC.B, KC.IDLE, KC.SENTINEL
_INFO = {}


def _info(case):
    if case.name not in _INFO:
        S = case.S
        _INFO[case.name] = pkg.kkt_order_info(S.n, S.m, S.jrow, S.jcol, S.hrow, S.hcol, S.gL, S.gU, case.cond, case.tile)
    return _INFO[case.name]


def _ctx(case):
    S = case.S
    return pkg.Context(S.n, S.m, 0, S.jrow, S.jcol, S.hrow, S.hcol, -np.ones(S.n), np.ones(S.n), S.gL, S.gU,
                       pkg.default_options(kkt_mode=1, kkt_condense=case.cond, kkt_tile_order=case.tile), batch=case.batch)


def rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(1.0, np.abs(np.asarray(b)).max()))


def _same_pivots(got, ref, kind, what):
    """the rule of tests/test_gpu_mf_structures.py::_same_pivots: 1 / D entry by entry, 1e-11 relative to the largest
    (well-scaled and indefinite sets); IPM-end scales: every pivot within 1e-7 of its own size and every sign exact"""
    if kind == "ipm":
        assert np.array_equal(got > 0, ref > 0), what
        err = np.abs(got - ref) / np.abs(ref)
        assert err.max() < 1e-7, (what, float(err.max()))
    else:
        assert rel(got, ref) < 1e-11, what


def _call(ctx, case, vals, dw, dw_last, fa, rhs, active):
    info = _info(case)
    st = lambda k: np.stack([v[k] for v in vals])
    return ctx.kkt_dense_test(active, st(0), st(1), st(2), st(3), st(4), st(5), np.array([v[6] for v in vals]),
                              np.asarray(dw, float), np.asarray(dw_last, float), np.asarray(fa), rhs, info["Fpad"], info["nu"],
                              sentinel=SENT)


def _check_assembly(case, out, b, v, dw, rhs, what):
    """matrix and working vector of instance b against the entry-wise reference; returns (K, xv) of the reference"""
    info = _info(case)
    S, pos, F = case.S, info["pos"], info["Fpad"]
    pad = np.setdiff1d(np.arange(F), pos)
    K, A, T = KR.reference_K(S, case.cond, pos, F, v, dw)
    got = out["K"][b]
    ratio, nonzero, outside = KR.compare(got, K, A, T)
    xr, xA, xT = KR.reference_xv(S, case.cond, pos, F, v, rhs)
    xratio, xnonzero, xoutside = KR.compare(out["xv"][b], xr, xA, xT, lower=False)
    print(f"[kkt-dense] {what}: K err/bound {ratio:.3f}, xv err/bound {xratio:.3f}")
    assert nonzero == 0, (what, "entries without terms that are not exactly zero", nonzero)
    assert outside == 0, (what, "entries outside (T + 4) u A", outside, ratio)
    assert (np.diag(got)[pad] == 1.0).all(), (what, "padding diagonal")
    assert xnonzero == 0 and xoutside == 0, (what, "working vector", xnonzero, xoutside, xratio)
    assert not out["xv"][b][pad].any(), (what, "working vector at padding positions")
    return K, (ratio, xratio)


def _run(case, kind, seed, ctx=None, dw=None, dw_last=None, fa=None, vals=None, want=None):
    """one call of the hook on `batch` distinct instances (IDLE inactive) and every comparison; returns the largest
    err / bound of (K, xv)"""
    own = ctx is None
    ctx = ctx or _ctx(case)
    info = _info(case)
    S, pos, F, nu, nb = case.S, info["pos"], info["Fpad"], info["nu"], case.batch
    pad = np.setdiff1d(np.arange(F), pos)
    vals = vals or [KC.values(case, kind, 1000 * seed + 17 * b + 1) for b in range(nb)]
    rhs = np.random.default_rng(seed).normal(size=(nb, S.n + S.m))
    active = np.array([b != IDLE or nb == 1 for b in range(nb)], dtype=np.int32)
    if dw is None:
        dw = np.array([1e-3 * (b + 1) for b in range(nb)]) if kind != "indef" else np.zeros(nb)
    dw_last = np.array([0.0, 1e-4, 0.0, 0.0, 5e-3])[:nb] if dw_last is None else dw_last
    fa = np.zeros(nb, dtype=int) if fa is None else fa
    out = _call(ctx, case, vals, dw, dw_last, fa, rhs, active)
    assert out["xv_mismatch"] == 0, (case.name, "k_sp_load_xv and load_solve_vector differ", out["xv_mismatch"])
    worst = [0.0, 0.0]
    for b in range(nb):
        what = (case.name, kind, b)
        dec = tuple(int(x) for x in out["decision"][b])
        if not active[b]:
            # untouched: the sentinels, and the matrix as it was (zero since the context was created: no call here makes it active)
            assert dec[:3] == (0, 0, 0), (what, dec)
            assert (out["xv"][b] == SENT).all() and (out["dinv_pad"][b] == SENT).all() and not out["K"][b].any(), what
            continue
        v = vals[b]
        K, r = _check_assembly(case, out, b, v, dw[b], rhs[b], what)
        worst = [max(worst[0], r[0]), max(worst[1], r[1])]
        if not case.solve:
            continue
        Ks = KR.symmetric(K)
        K64 = Ks.astype(np.float64)
        L, D = KR.ldlt_nopivot(K64)
        _same_pivots(out["dinv_pad"][b], 1.0 / D, kind, what)
        assert np.array_equal(out["dinv"][b], out["dinv_pad"][b][pos]), what
        # the decision by the rule (mf_dev.hpp inertia_decide, one candidate) on numpy's inertia of the reference matrix
        Ku = K64[np.ix_(pos, pos)]
        ok = int((np.linalg.eigvalsh(Ku) > 0).sum()) == S.n and bool(np.isfinite(D).all()) and bool((D != 0).all())
        exp = (2, 0, 1, int(fa[b]), dw[b]) if ok else (1, 0, 1, int(fa[b]) + 1, MS.next_shift(dw[b], dw_last[b]))
        assert dec == exp[:4] and out["dw"][b] == exp[4], (what, dec, out["dw"][b], exp)
        if want is not None:
            assert dec[0] == want[b], (what, dec, want[b])
        if kind != "indef":
            assert ok, what
        if not ok:
            continue
        # the solution of K x = xv (the vector the device loaded, held to its own reference above), in unknown order
        xv = out["xv"][b]
        bu = xv[pos]
        x = out["sol"][b]
        if kind == "ipm":
            bh = MS.backward_error(Ku, KR.solve_with(L, D, xv)[pos], bu)
            bd = MS.backward_error(Ku, x, bu)
            assert bd <= 10 * bh + 1e-15, (what, bd, bh)
        else:
            ref = KR.solve_long_double(Ks, xv).astype(np.float64)[pos]
            assert rel(x, ref) < 1e-11, (what, rel(x, ref))
            assert MS.backward_error(Ku, x, bu) <= 1e-13, what
    if own:
        ctx.close()
    return worst


@pytest.mark.parametrize("kind", ["well", "ipm"])
@pytest.mark.parametrize("name", list(KC.CASES))
def test_assembly_vector_pivots_and_solution(name, kind):
    """Every structure, distinct instances with one inactive: K and xv entry-wise, exact zeros and identity padding, the two
    loaders of the working vector bit for bit, pivots, decision and solution."""
    _run(KC.CASES[name], kind, seed=3 + len(name))


def _schur_min(case, v):
    """smallest eigenvalue of the Schur complement on the variables of K(0): K(dw) has n positive eigenvalues iff dw
    exceeds minus this"""
    S = case.S
    K = MS.dense_newton(S, case.cond, *v[:6], v[6], 0.0)
    n = S.n
    A, Bk, Ck = K[:n, :n], K[n:, :n], K[n:, n:]
    return float(np.linalg.eigvalsh(A - Bk.T @ np.linalg.solve(Ck, Bk)).min())


@pytest.mark.parametrize("name", ["plain63", "plain129", "full70", "tiled8x24", "arrow257_tiled"])
def test_inertia_decision_with_padding_inside_the_matrix(name):
    """The indefinite value set at delta_w = 0 (another shift: the next of the schedule, from 0 and from a last accepted
    shift) and at a passing delta_w; identity padding (pivot 1) in the middle of the matrix must not count."""
    case = KC.CASES[name]
    vals = [KC.values(case, "indef", 300 + b) for b in range(B)]
    lam = [-_schur_min(case, v) for v in vals]
    assert min(lam[b] for b in range(B) if b != IDLE) > 0
    dw = np.array([0.0, 2 * lam[1], 0.0, 0.0, 2 * lam[4]])
    dw_last = np.array([0.0, 0.0, 0.0, 6 * lam[3], 5e-3])
    fa = np.array([0, 0, 0, 1, 2])
    _run(case, "indef", 7, dw=dw, dw_last=dw_last, fa=fa, vals=vals, want={0: 1, 1: 2, 3: 1, 4: 2})


@pytest.mark.parametrize("no_mask", [False, True], ids=["masks", "SQPHIP_NO_TILE_MASK"])
@pytest.mark.parametrize("name", ["tiled8x24", "dense260_tiled"])
def test_a_second_assembly_leaves_nothing_of_the_first(name, no_mask, monkeypatch):
    """The point of the exact zeros: on one context, value set A, then set B (further rows free, a third of the Jacobian
    values zero, another Hessian scale).  The factorisation of the first call has overwritten the matrix in between; the
    second assembly is held entry-wise and zero-exact again.  Blocks between different leading tiles and panel blocks
    outside the mask are never written: they must still be zero.  With and without the tile masks (fresh context each)."""
    if no_mask:
        monkeypatch.setenv("SQPHIP_NO_TILE_MASK", "1")
    case = KC.CASES[name]
    ctx = _ctx(case)
    sets = [KC.stale_sets(case, 40 + b) for b in range(B)]
    _run(case, "well", 21, ctx=ctx, vals=[s[0] for s in sets])
    _run(case, "well", 22, ctx=ctx, vals=[s[1] for s in sets])
    ctx.close()


def test_the_hook_refuses_a_sparse_context():
    S = KC.CASES["plain65"].S
    ctx = pkg.Context(S.n, S.m, 0, S.jrow, S.jcol, S.hrow, S.hcol, -np.ones(S.n), np.ones(S.n), S.gL, S.gU,
                      pkg.default_options(kkt_mode=2), batch=1)
    v = KC.values(KC.CASES["plain65"], "well", 1)
    with pytest.raises(pkg.SqpHipError):
        ctx.kkt_dense_test([1], *[np.asarray(x)[None] for x in v[:6]], [v[6]], [0.0], [0.0], [0], np.zeros((1, S.n + S.m)), 128, 65)
    ctx.close()
