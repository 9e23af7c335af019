"""The inertia test of a sweep (mf_dev.hpp: inertia_count, inertia_decide) as both of its callers run it: in the prologue of
the streamed top-of-tree solve (k_mf_solve_top2: pivots counted a chunk of 256 x 12 at a time, the record of the first front
of a non-speculating instance requested beside them, the decision published through LDS) and as k_inertia (1 024 threads,
chunks of eight per thread).  Everything goes through one sweep of sqphip_mf_batch_test on the structures of
tests/mf_structures.py, on three more built with its helpers (a streamed top below 256, above 256 and above one chunk of the
256-thread caller) and on the IEEE-118 structure in full form:

* the rule of inertia_decide, applied on the host to the pivots the device returns, gives the device's decision;
* SQPHIP_INERTIA_SERIAL=1 (the former loop and order) and the default agree bit for bit;
* an instance that is refused -- indefinite without a second candidate, or a NaN among its Hessian values -- leaves its
  neighbours' results bit-equal to a run in which it is idle;
* four IEEE-118 scenarios end to end: same iterates, logs and work counters under the switch and by default.

The outputs of a (structure, switch) pair are computed once and shared by the tests."""
import numpy as np
import pytest

import sqpsolver_jl_amd as pkg
from sqpsolver_jl_amd.acopf_synth import acopf_synth, acopf_layout, contingency, CASES
import mf_structures as MS

pytestmark = pytest.mark.gpu

FAMILIES = {S.name: S for S in MS.families()}
B, IDLE = 5, 3
KEYS = ("decision", "dw", "dinv0", "dinv1", "fused", "standalone")
# name -> condensed form?  Which kernel tests the inertia follows from the plan (a streamed top: k_mf_solve_top2, else
# k_inertia) and is asserted from the launch census.  Fpad is the order rounded up to 64.  Streamed top: small_top 192 (below
# 256), top_84 256 (one full pass of the 256 threads), mid_top 320 (no multiple of 256), big_top 3 200 (above the chunk of
# 256 x 12 = 3 072 and no multiple of 256: the second chunk and its clamped tail run).  k_inertia (chunks of 1 024 x 8):
# front63 128, top_85 256, narrow_mixed_T and front300 320, the IEEE-118 structure in full form 2 816 (fronts above 128 rows).
SHAPES = {"small_top": 1, "top_84": 1, "mid_top": 1, "big_top": 1,
          "front63": 1, "top_85": 1, "narrow_mixed_T": 1, "front300": 1, "case118_full": 0}
STREAMED = ("small_top", "top_84", "mid_top", "big_top")
_CACHE = {}


def _structure(name):
    if name == "small_top":
        return MS.siblings([60, 10], 70, 4, seed=3, name=name)
    if name == "mid_top":
        return MS.siblings([20, 30, 40, 50, 60], 60, 4, seed=8, name=name)
    if name == "big_top":
        return MS.siblings([70, 60, 50] + [45] * 64, 60, 4, seed=7, name=name)
    if name != "case118_full":
        return FAMILIES[name]
    nb, ng, nl, seed = CASES["case118"]
    lay = acopf_layout(acopf_synth(nb, ng, nl, seed))
    return MS.Structure("case118_full", lay.n, lay.m, np.asarray(lay.jrow), np.asarray(lay.jcol), np.asarray(lay.hrow),
                        np.asarray(lay.hcol), np.asarray(lay.gL, float), np.asarray(lay.gU, float), {})


def _plan(name):
    """(Fpad, the kernel that tests the inertia) from the host side of the library: the order of the symbolic analysis and
    whether the plan of a batch of B has a streamed top"""
    S, cond = _structure(name), SHAPES[name]
    _, st = pkg.kkt_symbolic(S.n, S.m, S.jrow, S.jcol, S.hrow, S.hcol, S.gL, S.gU, condense=bool(cond))
    top = pkg.mf_plan_info(S.n, S.m, S.jrow, S.jcol, S.hrow, S.hcol, S.gL, S.gU, condense=cond, batch=B)[2]
    return -(-st["order"] // 64) * 64, "k_mf_solve_top2" if top > 0 else "k_inertia"


def _threshold(S, cond, v):
    """A shift that gives K(dw) its n positive pivots, at most 1.5 times the smallest such shift (minus the smallest
    eigenvalue of the Schur complement on the variables): bisection on the host reference's pivot count."""
    rhs = np.zeros(S.nu(cond))
    ok = lambda dw: pkg.mf_host_solve(S.n, S.m, S.jrow, S.jcol, S.hrow, S.hcol, S.gL, S.gU, cond, *v[:6], v[6], dw, rhs)[2] == S.n
    lo, hi = 1e-6, 1e3
    assert not ok(lo) and ok(hi)
    while hi > 1.5 * lo:
        mid = np.sqrt(lo * hi)
        lo, hi = (lo, mid) if ok(mid) else (mid, hi)
    return hi


def _inputs(name):
    """Two batches of five, instance 3 idle.  Batch "both" (as test_inertia_decision_follows_the_rule_on_both_candidates): 0
    passes on candidate 0, 1 only on candidate 1, 2 fails both, 4 retries from delta_w = 0 and passes on candidate 1.  Batch
    "nospec": 0 (well scaled, delta_w = 0) does not speculate and passes, 1 (indefinite, delta_w = 0, first attempt) does not
    speculate and fails, 2 (well scaled with a shift) speculates and passes on candidate 0, 4 as in "both"."""
    key = ("inputs", name)
    if key not in _CACHE:
        S = _structure(name)
        cond = SHAPES[name]
        ind = [MS.values(S, "indef", 300 + b) for b in range(B)]
        lam = [_threshold(S, cond, v) for v in ind]
        rhs = np.random.default_rng(3).normal(size=(B, S.nu(cond)))
        active = np.array([b != IDLE for b in range(B)], dtype=np.int32)
        both = dict(vals=ind, dw=np.array([2 * lam[0], lam[1] / 10, lam[2] / 1000, 0.0, 0.0]),
                    dw_last=np.array([0.0, 0.0, 0.0, 0.0, 6 * lam[4]]), fa=np.array([0, 0, 0, 0, 1]), rhs=rhs, active=active)
        well = [MS.values(S, "well", 500 + b) for b in range(B)]
        nospec = dict(vals=[well[0], ind[1], well[2], ind[3], ind[4]], dw=np.array([0.0, 0.0, 1e-3, 0.0, 0.0]),
                      dw_last=np.array([0.0, 0.0, 0.0, 0.0, 6 * lam[4]]), fa=np.array([0, 0, 0, 0, 1]), rhs=rhs, active=active)
        _CACHE[key] = (S, cond, {"both": both, "nospec": nospec})
    return _CACHE[key]


def _sweep(ctx, I, active=None, vals=None):
    vals = I["vals"] if vals is None else vals
    st = lambda k: np.stack([v[k] for v in vals])
    return ctx.mf_batch_test(I["active"] if active is None else active, st(0), st(1), st(2), st(3), st(4), st(5),
                             np.array([v[6] for v in vals]), I["dw"], I["dw_last"], I["fa"], I["rhs"])


def _ctx(S, cond):
    return pkg.Context(S.n, S.m, 0, S.jrow, S.jcol, S.hrow, S.hcol, -np.ones(S.n), np.ones(S.n), S.gL, S.gU,
                       pkg.default_options(kkt_mode=S.kkt_mode, kkt_condense=cond), batch=B)


def _set_switch(monkeypatch, serial):
    if serial: monkeypatch.setenv("SQPHIP_INERTIA_SERIAL", "1")
    else: monkeypatch.delenv("SQPHIP_INERTIA_SERIAL", raising=False)


def _outputs(name, serial, monkeypatch):
    """both batches of a structure through one context: ({batch: outputs}, launch census); computed once"""
    key = (name, bool(serial))
    if key not in _CACHE:
        S, cond, batches = _inputs(name)
        _set_switch(monkeypatch, serial)
        ctx = _ctx(S, cond)
        out = {k: _sweep(ctx, I) for k, I in batches.items()}
        _CACHE[key] = (out, ctx.mf_census())
        ctx.close()
    return _CACHE[key]


def _passes(p, n):
    return bool(np.isfinite(p).all() and (p != 0).all() and int((p > 0).sum()) == n)


@pytest.mark.parametrize("name", list(SHAPES))
def test_the_rule_on_the_devices_own_pivots_gives_the_devices_decision(name, monkeypatch):
    """inertia_decide on the host, fed with the pivot arrays the hook returns: n positive pivots and none zero or non-finite
    passes; candidate 1 counts only where the instance speculates (a retry, or a shift > 0); the next shift from
    MS.next_shift.  The instances are those of test_inertia_decision_follows_the_rule_on_both_candidates
    (tests/test_gpu_mf_structures.py) and a batch without second candidates, the thresholds found by bisection.  Outcome, sel,
    n_factor, fac_attempt and delta_w must be the device's.  The census names the kernel."""
    S, cond, batches = _inputs(name)
    out, census = _outputs(name, False, monkeypatch)
    fpad, kernel = _plan(name)
    assert (kernel == "k_mf_solve_top2") == (name in STREAMED), (name, kernel)
    other = "k_inertia" if kernel == "k_mf_solve_top2" else "k_mf_solve_top2"
    print(name, "Fpad", fpad, kernel, {k: census[k] for k in (kernel, other)})
    assert census[kernel] > 0 and census[other] == 0, (name, census)
    seen = set()
    for bk, I in batches.items():
        o = out[bk]
        for b in range(B):
            dec = tuple(int(x) for x in o["decision"][b])
            if b == IDLE:
                assert dec[:3] == (0, 0, 0), (name, bk, dec)
                continue
            dw, dwl, fa = I["dw"][b], I["dw_last"][b], int(I["fa"][b])
            spec = fa > 0 or dw > 0
            assert bool(dec[4]) == spec, (name, bk, b)
            dw1 = MS.next_shift(dw, dwl)
            ok0 = _passes(o["dinv0"][b], S.n)
            ok1 = spec and _passes(o["dinv1"][b], S.n)
            if ok0:
                exp = (2, 0, 1, fa, dw)
            elif ok1:
                exp = (2, 1, 2, fa + 1, dw1)
            else:
                nf = 2 if spec else 1
                exp = (1, 0, nf, fa + nf, MS.next_shift(dw1, dwl) if spec else dw1)
            print(name, bk, b, "spec", spec, "positives", int((o["dinv0"][b] > 0).sum()), int((o["dinv1"][b] > 0).sum()), "of", S.n,
                  "decision", dec, "dw", o["dw"][b], "expected", exp)
            assert dec[:4] == exp[:4] and o["dw"][b] == exp[4], (name, bk, b, dec, o["dw"][b], exp)
            seen.add((spec, exp[0], exp[1]))
            if exp[0] == 2:
                assert not np.array_equal(o["fused"][b], I["rhs"][b]), (name, bk, b)
    # the comparison covers every branch of the rule: passes on candidate 0 / on candidate 1 / fails both while speculating,
    # passes / fails without a second candidate
    assert seen == {(True, 2, 0), (True, 2, 1), (True, 1, 0), (False, 2, 0), (False, 1, 0)}, (name, seen)


@pytest.mark.parametrize("name", list(SHAPES))
def test_the_default_and_the_serial_loop_agree_bit_for_bit(name, monkeypatch):
    """SQPHIP_INERTIA_SERIAL=1 (inertia_count_serial; in the streamed kernel also the former order: phase and sel re-read from
    global memory behind the decision, the first front's record requested after it)
    against the default on the same inputs: decisions, shifts, pivots of both candidates and both solutions."""
    new, census_new = _outputs(name, False, monkeypatch)
    old, census_old = _outputs(name, True, monkeypatch)
    assert census_new == census_old, name
    for bk in new:
        for k in KEYS:
            assert np.array_equal(new[bk][k], old[bk][k], equal_nan=True), (name, bk, k)


def test_the_shapes_cover_the_index_arithmetic_of_both_callers():
    """Fpad below 256, equal to it, above it and no multiple of it, and above one chunk of the 256-thread caller with a
    clamped tail -- on the streamed path; below and above 256 and no multiple of 1 024 on the k_inertia path."""
    fp = {name: _plan(name)[0] for name in SHAPES}
    st = sorted(fp[k] for k in STREAMED)
    assert st[0] < 256 and 256 in st and any(256 < f < 3072 and f % 256 for f in st) and st[-1] > 3072 and st[-1] % 256, fp
    ki = sorted(fp[k] for k in SHAPES if k not in STREAMED)
    assert ki[0] < 256 and ki[-1] > 1024 and ki[-1] % 1024, fp


@pytest.mark.parametrize("name", ["mid_top", "top_85"])
def test_a_refused_instance_leaves_its_neighbours_untouched(name, monkeypatch):
    """Batch "nospec" three times through the streamed kernel (mid_top) and through k_inertia (top_85): as it is --
    instance 1, indefinite without a second candidate, has requested the record of its first front when the count refuses
    it --, with instance 1 idle, and with a NaN among instance 1's Hessian values.  The refused instance comes back with outcome 1 (or 3
    with the NaN); every other instance's pivots, solutions, decision and shift are bit-equal in the three runs."""
    S, cond, batches = _inputs(name)
    I = batches["nospec"]
    _set_switch(monkeypatch, False)
    ran = _outputs(name, False, monkeypatch)[0]["nospec"]
    ctx = _ctx(S, cond)
    idle = I["active"].copy(); idle[1] = 0
    rest = _sweep(ctx, I, active=idle)
    v = list(I["vals"][1]); hv = v[1].copy(); hv[np.flatnonzero(S.hrow == S.hcol)[0]] = np.nan; v[1] = hv
    vals = list(I["vals"]); vals[1] = tuple(v)
    nan = _sweep(ctx, I, vals=vals)
    ctx.close()
    assert int(ran["decision"][1][0]) == 1 and tuple(ran["decision"][1][1:4]) == (0, 1, 1)
    assert int(nan["decision"][1][0]) in (1, 3) and not np.isfinite(nan["dinv0"][1]).all()
    assert tuple(rest["decision"][1][:3]) == (0, 0, 0)
    others = [b for b in range(B) if b != 1]
    assert int(ran["decision"][0][0]) == 2 and int(ran["decision"][2][0]) == 2 and int(ran["decision"][4][0]) == 2
    for k in KEYS:
        if k == "dinv1":
            continue        # (a context keeps the second candidate's pivots of an earlier sweep where the instance no longer speculates)
        assert np.array_equal(ran[k][others], rest[k][others]), (name, k, "failing against idle")
        assert np.array_equal(nan[k][others], rest[k][others]), (name, k, "NaN against idle")
    for b in (2, 4):        # the instances that speculate write their second candidate in every run
        assert np.array_equal(ran["dinv1"][b], rest["dinv1"][b]) and np.array_equal(nan["dinv1"][b], rest["dinv1"][b])


def test_four_ieee118_scenarios_end_to_end_under_the_switch_and_by_default(monkeypatch):
    """Four IEEE-118 scenarios, seven SQP iterations through sqphip_sqp_run: the same iterates bit for bit, the same
    per-sub-problem logs, work counters and launch census under SQPHIP_INERTIA_SERIAL=1 and by default."""
    nb, ng, nl, seed = CASES["case118"]
    base = acopf_synth(nb, ng, nl, seed)
    nets = [base, contingency(base, 7, seed), contingency(base, 3, seed), contingency(base, 100, seed)]
    lays = [acopf_layout(nt) for nt in nets]
    opts = dict(max_iter=7, tol_infeas=1e-6, tol_residual=1e-4, use_soc=1, literal_quirks=1)
    got = {}
    for serial in (True, False):
        _set_switch(monkeypatch, serial)
        ctx = pkg.Context(lays[0].n, lays[0].m, lays[0].num_linear, lays[0].jrow, lays[0].jcol, lays[0].hrow, lays[0].hcol,
                          lays[0].xL, lays[0].xU, lays[0].gL, lays[0].gU, pkg.default_options(**opts), batch=len(nets))
        ctx.acopf_attach(nets[0], lays[0])
        for b in range(len(nets)):
            ctx.acopf_set_instance(b, nets[b], lays[b])
        ctx.sqp_reset(); ctx.sqp_run(0)
        c = ctx.counters()
        got[serial] = ([ctx.sqp_get(b)["x"] for b in range(4)], [ctx.sqp_qp_log(b) for b in range(4)],
                       (c["n_qp"], c["n_ipm_iter"], c["n_factor"], c["n_solve"]), ctx.mf_census())
        ctx.close()
    old, new = got[True], got[False]
    assert all(np.array_equal(a, b) for a, b in zip(old[0], new[0]))
    assert old[1] == new[1] and old[2] == new[2] and old[3] == new[3]
    assert new[2][2] > 0 and new[3]["k_mf_solve_top2"] > 0 and new[3]["k_inertia"] == 0
