"""The multifrontal kernels (mfront.hip) on the structures of tests/mf_structures.py: every front height in 16-row tiles
(T = 1 .. 14 and fronts of 300 / 511 / 1000 rows), ragged and merged levels, partial four-column blocks, top fronts on
both sides of the streamed solve's limits -- with every instance of a batch active and distinct, one idle, through what
one interior-point sweep does (sqphip_mf_batch_test): factorisation of both candidate shifts, the inertia decision, the
fused and the stand-alone solves.  Compared with the library's host reference of the same plan and with numpy on an
independently assembled dense matrix.  The last test asserts that the launch census saw every kernel the factor, solve
and inertia paths can launch."""
import numpy as np
import pytest

import sqpsolver_jl_amd as pkg
from sqpsolver_jl_amd.acopf_synth import acopf_synth, acopf_layout, contingency, CASES
import mf_structures as MS

pytestmark = pytest.mark.gpu

FAMILIES = {S.name: S for S in MS.families()}
B, IDLE = 5, 3                       # odd batch, one idle instance: the candidate grid (2 B) and the early returns
CENSUS = {}                          # launches seen by the contexts of this module, summed (test_census_saw_every_kernel)
# kernels no test can reach by environment switches, with the reason: none -- every switch is read per call
CENSUS_EXCLUDED = {}
# the switches of test_gpu_parity.py::test_every_front_kernel_variant_matches_the_host_reference, and the spine
ENV_VARIANTS = [{}, {"SQPHIP_MF_STATIC_MIN": "1"}, {"SQPHIP_MF_STATIC": "0"},
                {"SQPHIP_MF_TOP2": "0", "SQPHIP_MF_LEVEL2": "0", "SQPHIP_MF_BIG_LDSIMG": "0"},
                {"SQPHIP_MF_NW4": "0", "SQPHIP_MF_NW8": "0"}, {"SQPHIP_MF_SPINE": "1"}]


def rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(1.0, np.abs(np.asarray(b)).max()))


def _ctx(S, cond=1, batch=B):
    n, m = S.n, S.m
    return pkg.Context(n, m, 0, S.jrow, S.jcol, S.hrow, S.hcol, -np.ones(n), np.ones(n), S.gL, S.gU,
                       pkg.default_options(kkt_mode=S.kkt_mode, kkt_condense=cond), batch=batch)


def _close(ctx):
    for k, v in ctx.mf_census().items():
        CENSUS[k] = CENSUS.get(k, 0) + v
    ctx.close()


def _host(S, cond, v, dw, rhs):
    Jv, Hv, Dd, sigp, hd, rt, hsc = v
    return pkg.mf_host_solve(S.n, S.m, S.jrow, S.jcol, S.hrow, S.hcol, S.gL, S.gU, cond, Jv, Hv, Dd, sigp, hd, rt, hsc, dw, rhs)


def _batch(ctx, S, cond, vals, dw, dw_last, fac_attempt, rhs, active):
    st = lambda k: np.stack([v[k] for v in vals])
    return ctx.mf_batch_test(active, st(0), st(1), st(2), st(3), st(4), st(5), np.array([v[6] for v in vals]),
                             np.asarray(dw, float), np.asarray(dw_last, float), np.asarray(fac_attempt), rhs)


def _same_pivots(got, ref, kind, what):
    """1 / D against the host reference, entry by entry.  Well-scaled and indefinite sets: 1e-11 relative to the largest.
    IPM-end scales (pivots from 1e-9 to 1e9): every pivot within 1e-7 of its own size -- a pivot of order one is formed from
    terms up to 1e9, so its last digits follow the summation order -- and every sign exact."""
    if kind == "ipm":
        assert np.array_equal(got > 0, ref > 0), what
        err = np.abs(got - ref) / np.abs(ref)
        assert err.max() < 1e-7, (what, float(err.max()))
    else:
        assert rel(got, ref) < 1e-11, what


def _run_family(S, kind, cond=1, seed=0):
    """B distinct instances (instance IDLE idle) of the family through one sweep; every output against the host reference
    at the shift each candidate factorised, the pivot signs and the solution against numpy"""
    ctx = _ctx(S, cond)
    nu = S.nu(cond)
    vals = [MS.values(S, kind, 1000 * seed + 17 * b + 1) for b in range(B)]
    rhs = np.random.default_rng(seed).normal(size=(B, nu))
    active = np.array([b != IDLE for b in range(B)], dtype=np.int32)
    dw = np.array([1e-3 * (b + 1) for b in range(B)]) if kind != "indef" else np.zeros(B)
    dw_last = np.array([0.0, 1e-4, 0.0, 0.0, 5e-3])
    fa = np.array([0, 0, 1, 0, 2]) if kind == "indef" else np.zeros(B, dtype=int)
    out = _batch(ctx, S, cond, vals, dw, dw_last, fa, rhs, active)
    for b in range(B):
        dec = out["decision"][b]
        if b == IDLE:
            assert tuple(dec[:3]) == (0, 0, 0), (S.name, dec)
            continue
        v = vals[b]
        dw1 = MS.next_shift(dw[b], dw_last[b])
        ref0, d0, np0 = _host(S, cond, v, dw[b], rhs[b])
        _same_pivots(out["dinv0"][b], d0, kind, (S.name, kind, b, 0))
        # candidate 1 is factorised exactly for the instances that speculate (mf_speculates: a retry, or a shift > 0): its
        # pivots are the host's at the next shift, elsewhere they stay untouched (zero in a fresh context)
        spec = fa[b] > 0 or dw[b] > 0
        assert bool(dec[4]) == spec
        if spec:
            ref1, d1, np1 = _host(S, cond, v, dw1, rhs[b])
            _same_pivots(out["dinv1"][b], d1, kind, (S.name, kind, b, 1))
        else:
            assert not out["dinv1"][b].any(), (S.name, kind, b)
        if kind != "ipm":
            K0 = MS.dense_newton(S, cond, *v[:6], v[6], dw[b])
            assert int((out["dinv0"][b] > 0).sum()) == int((np.linalg.eigvalsh(K0) > 0).sum()), (S.name, b)
        # the decision by the rule (mf_dev.hpp inertia_decide) on the host reference's pivot counts (the CPU tests hold those
        # to eigvalsh): well-scaled and IPM-end instances pass on candidate 0, so every solve below is checked
        ok0 = np0 == S.n
        ok1 = spec and np1 == S.n
        if ok0:
            exp = (2, 0, 1, fa[b], dw[b])
        elif ok1:
            exp = (2, 1, 2, fa[b] + 1, dw1)
        else:
            nf = 2 if spec else 1
            exp = (1, 0, nf, fa[b] + nf, MS.next_shift(dw1, dw_last[b]) if spec else dw1)
        assert tuple(int(x) for x in dec[:4]) == exp[:4] and out["dw"][b] == exp[4], (S.name, kind, b, dec, exp)
        if kind != "indef":
            assert exp[:2] == (2, 0), (S.name, kind, b)
        if dec[0] != 2:
            continue
        ref, dsh = (ref0, dw[b]) if dec[1] == 0 else (ref1, dw1)
        if kind == "ipm":
            # forward agreement cannot survive the conditioning: the device's backward error within a small factor of the
            # host reference's
            K = MS.dense_newton(S, cond, *v[:6], v[6], dsh)
            bh = MS.backward_error(K, ref, rhs[b])
            for x in (out["fused"][b], out["standalone"][b]):
                bd = MS.backward_error(K, x, rhs[b])
                assert bd <= 10 * bh + 1e-15, (S.name, b, bd, bh)
        else:
            assert rel(out["fused"][b], ref) < 1e-11 and rel(out["standalone"][b], ref) < 1e-11, (S.name, kind, b)
            K = MS.dense_newton(S, cond, *v[:6], v[6], dsh)
            assert MS.backward_error(K, out["fused"][b], rhs[b]) <= 1e-13, (S.name, b)
    _close(ctx)
    return out


@pytest.mark.parametrize("kind", MS.VALUE_SETS)
def test_every_family_matches_the_host_reference_with_distinct_instances(kind):
    """Every family, five distinct instances (one idle), condensed form; the smaller ones in the full form too."""
    for i, S in enumerate(FAMILIES.values()):
        _run_family(S, kind, 1, seed=i)
        if S.n <= 120 and kind == "well":
            _run_family(S, kind, 0, seed=i)


def test_indefinite_solutions_match_the_host_reference():
    """The solve on an indefinite matrix (no inertia decision in the way: sqphip_mf_solve_test), per instance of a batch
    loaded with different values, so that an instance that read another's data would differ."""
    for name in ("front207", "front224", "front300", "narrow_mixed_T", "wide_classes", "top_85"):
        S = FAMILIES[name]
        ctx = _ctx(S)
        for inst in (4, 1):
            v = MS.values(S, "indef", 50 + inst)
            rhs = np.random.default_rng(inst).normal(size=S.nu(1))
            ref, dref, npos = _host(S, 1, v, 0.0, rhs)
            fused, alone, dv = ctx.mf_solve_test(inst, *v[:6], v[6], 0.0, rhs)
            assert rel(fused, ref) < 1e-11 and rel(alone, ref) < 1e-11 and rel(dv, dref) < 1e-11, (name, inst)
            K = MS.dense_newton(S, 1, *v[:6], v[6], 0.0)
            assert int((dv > 0).sum()) == npos == int((np.linalg.eigvalsh(K) > 0).sum()) < S.n
        _close(ctx)


def _schur_min(S, v):
    """smallest eigenvalue of the Schur complement on the variables of K(0): K(dw) has n positive pivots iff dw exceeds
    minus this"""
    K = MS.dense_newton(S, 1, *v[:6], v[6], 0.0)
    n = S.n
    A, Bk, Ck = K[:n, :n], K[n:, :n], K[n:, n:]
    return float(np.linalg.eigvalsh(A - Bk.T @ np.linalg.solve(Ck, Bk)).min())


@pytest.mark.parametrize("name", ["front63", "front207", "front224", "narrow_mixed_T", "top_84", "top_85"])
def test_inertia_decision_follows_the_rule_on_both_candidates(name):
    """The decision (inertia_decide, in k_mf_solve_top2 or k_inertia) against the rule applied to numpy's inertia of K(dw)
    and K(next shift): instance 0 passes on candidate 0, 1 only on candidate 1, 2 fails both, 4 retries from delta_w = 0
    and passes on candidate 1 (the last accepted shift / 3); 3 is idle."""
    S = FAMILIES[name]
    ctx = _ctx(S)
    vals = [MS.values(S, "indef", 300 + b) for b in range(B)]
    lam = [-_schur_min(S, v) for v in vals]
    assert min(lam[b] for b in range(B) if b != IDLE) > 0
    dw = np.array([2 * lam[0], lam[1] / 10, lam[2] / 1000, 0.0, 0.0])
    dw_last = np.array([0.0, 0.0, 0.0, 0.0, 6 * lam[4]])
    fa = np.array([0, 0, 0, 0, 1])
    rhs = np.random.default_rng(3).normal(size=(B, S.nu(1)))
    active = np.array([b != IDLE for b in range(B)], dtype=np.int32)
    out = _batch(ctx, S, 1, vals, dw, dw_last, fa, rhs, active)
    want_outcome = {0: (2, 0), 1: (2, 1), 2: (1, None), 4: (2, 1)}
    for b in (0, 1, 2, 4):
        v, dec = vals[b], out["decision"][b]
        dw1 = MS.next_shift(dw[b], dw_last[b])
        ok = [int((np.linalg.eigvalsh(MS.dense_newton(S, 1, *v[:6], v[6], s)) > 0).sum()) == S.n for s in (dw[b], dw1)]
        spec = fa[b] > 0 or dw[b] > 0
        # the rule (mf_dev.hpp inertia_decide), one shift per candidate
        if ok[0]:
            exp = (2, 0, 1, fa[b], dw[b])
        elif spec and ok[1]:
            exp = (2, 1, 2, fa[b] + 1, dw1)
        else:
            nf = 2 if spec else 1
            exp = (1, 0, nf, fa[b] + nf, MS.next_shift(dw1, dw_last[b]) if spec else dw1)
        assert (dec[0], dec[1], dec[2], dec[3]) == exp[:4] and out["dw"][b] == exp[4], (name, b, dec, exp)
        assert (dec[0], dec[1] if dec[0] == 2 else None) == want_outcome[b], (name, b, dec)
        if dec[0] == 2:
            ref, _, _ = _host(S, 1, v, exp[4], rhs[b])
            assert rel(out["fused"][b], ref) < 1e-11 and rel(out["standalone"][b], ref) < 1e-11, (name, b)
    assert tuple(out["decision"][IDLE][:3]) == (0, 0, 0)
    _close(ctx)


CENSUS_FAMILIES = ["front15", "front31", "front47", "front63", "front95", "front127", "front143", "front207", "front224",
                   "front1000", "narrow_mixed_T", "narrow_class8", "wide_small_T", "wide_classes", "nc_mod4_1_rows",
                   "top_84", "top_85"]


@pytest.mark.parametrize("env", ENV_VARIANTS[1:], ids=lambda e: ",".join(f"{k}={v}" for k, v in e.items()))
def test_kernel_variants_on_the_families(env, monkeypatch):
    """The switches the variant test of test_gpu_parity.py flips, and the spine kernel, on the families: the same host
    comparison through the batched sweep."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    for i, name in enumerate(CENSUS_FAMILIES):
        _run_family(FAMILIES[name], "well", 1, seed=40 + i)


@pytest.mark.parametrize("env", ENV_VARIANTS, ids=lambda e: ",".join(f"{k}={v}" for k, v in e.items()) or "default")
def test_the_factor_census_of_a_sweep_is_the_predicted_choice(env, monkeypatch):
    """What the factorisation of a sweep launched, by the census, against what the host-only hook sqphip_mf_factor_kernels
    predicts for the plan under the same switches (big_lds = 1: the device grants 160 KB of LDS): the factor-side entries
    -- rank-1, generic and static front kernels, spine -- equal the predicted launches per kernel times one common integer
    >= 1, the mf_factor calls of the sweep; an entry predicted zero is zero."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    names = _census_names()
    factor_side = [k for k in names if k.startswith(("k_mf_factor", "k_mf_front", "k_mf_spine"))]
    assert len(factor_side) == 27
    for i, name in enumerate(CENSUS_FAMILIES):
        S = FAMILIES[name]
        before = dict(CENSUS)
        _run_family(S, "well", 1, seed=120 + i)
        seen = {k: CENSUS.get(k, 0) - before.get(k, 0) for k in factor_side}
        ker = pkg.mf_factor_kernels(S.n, S.m, S.jrow, S.jcol, S.hrow, S.hcol, S.gL, S.gU, 1, B, 1)
        want = dict.fromkeys(factor_side, 0)
        for kid, _packed, spine, _small in ker.tolist():
            if not spine:
                want[names[kid]] += 1
        want["k_mf_spine"] += int(ker[:, 2].any())
        print(name, {k: (seen[k], want[k]) for k in factor_side if seen[k] or want[k]})
        calls = {seen[k] // want[k] for k in factor_side if want[k]}
        assert len(calls) == 1 and min(calls) >= 1, (name, env, seen, want)
        assert all(seen[k] == want[k] * min(calls) for k in factor_side), (name, env, seen, want)


def test_census_saw_every_factor_and_solve_kernel(monkeypatch):
    """Every kernel instantiation that mf_factor, mf_solve and the inertia test can launch was launched by the tests of this
    module (the census of their contexts), but for the listed exclusions.  Families run again here under the switches
    only where a kernel is still missing, so that the test also stands alone."""
    for env in ENV_VARIANTS:
        names = _census_names()
        if all(CENSUS.get(k, 0) > 0 for k in names if k not in CENSUS_EXCLUDED):
            break
        for k in [k for k in env]:
            monkeypatch.setenv(k, env[k])
        for i, name in enumerate(CENSUS_FAMILIES):
            _run_family(FAMILIES[name], "well", 1, seed=80 + i)
        for k in env:
            monkeypatch.delenv(k)
    names = _census_names()
    seen = {k: CENSUS.get(k, 0) for k in names}
    print("launch census:", ", ".join(f"{k}: {c}" for k, c in seen.items()))
    print("excluded:", CENSUS_EXCLUDED)
    missing = [k for k in names if k not in CENSUS_EXCLUDED and seen[k] == 0]
    assert not missing, missing
    assert set(CENSUS_EXCLUDED) <= set(names)


def _census_names():
    S = FAMILIES["front15"]
    ctx = _ctx(S)
    names = list(ctx.mf_census())
    ctx.close()
    return names


def test_values_by_the_stage_kernel_with_the_tail_speculation_give_the_default_bits(monkeypatch):
    """above 192 instances the second candidate is switched on in the tail of a run only (spec_tail),
    between sweeps.  With the matrix values assembled by the stage kernel (SQPHIP_MF_VALS_INLINE=1) the sweep after the
    switch must not factorise candidate 1 from values that were never written.  256 IEEE-14 scenarios to termination:
    the same iterates bit for bit, the same logs and work counters as the default."""
    nb, ng, nl, seed = CASES["case14"]
    base = acopf_synth(nb, ng, nl, seed)
    nets = [base] + [contingency(base, 1 + s % 19, seed + s) for s in range(1, 256)]
    lays = [acopf_layout(nt) for nt in nets]
    kw = dict(max_iter=40, tol_infeas=1e-6, tol_residual=1e-4, use_soc=1, literal_quirks=1)
    got = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("SQPHIP_MF_VALS_INLINE", mode)
        ctx = pkg.Context(lays[0].n, lays[0].m, lays[0].num_linear, lays[0].jrow, lays[0].jcol, lays[0].hrow, lays[0].hcol,
                          lays[0].xL, lays[0].xU, lays[0].gL, lays[0].gU, pkg.default_options(**kw), batch=len(nets))
        ctx.acopf_attach(nets[0], lays[0])
        for b in range(len(nets)):
            ctx.acopf_set_instance(b, nets[b], lays[b])
        ctx.sqp_reset(); ctx.sqp_run(0)
        c = ctx.counters()
        assert c["sparse"] == 1
        got[mode] = ([ctx.sqp_get(b)["x"] for b in range(len(nets))], [ctx.sqp_qp_log(b) for b in range(len(nets))],
                     (c["n_qp"], c["n_ipm_iter"], c["n_factor"], c["n_solve"]))
        ctx.close()
    assert all(np.array_equal(a, b) for a, b in zip(got["1"][0], got["0"][0]))
    assert got["1"][1] == got["0"][1] and got["1"][2] == got["0"][2]
