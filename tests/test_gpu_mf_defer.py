"""The deferral pass of the multifrontal plan (mf_build_plan, SQPHIP_MF_DEFER) on the device: a front that rides in a later
launch of the same kernel computes what it computed in a launch of its own, bit for bit.  Kernel level
(sqphip_mf_batch_test: one sweep's factorisation of both candidate shifts, inertia decision, fused and stand-alone solves)
on the IEEE-118 structure and on the smallest synthetic structure with a dissolvable launch (tests/mf_defer_structures.py),
and end to end on four IEEE-118 scenarios.  The contexts here hold three or four instances, where the plan merges the levels
up to four tiles (SymOptions::merge_tiles); SQPHIP_MF_MERGE_T=0, read when the plan is built, gives them the schedule of
the large batches, with both launches the pass removes there."""
import numpy as np
import pytest

import sqpsolver_jl_amd as pkg
from sqpsolver_jl_amd.acopf_synth import acopf_synth, acopf_layout, contingency, CASES
import mf_structures as MS
from mf_defer_structures import defer_leaf

pytestmark = pytest.mark.gpu

B, IDLE = 3, 1
FACTOR_KERNELS = ("k_mf_front<", "k_mf_factor2<", "k_mf_factor<")


def _case118_structure():
    nb, ng, nl, seed = CASES["case118"]
    lay = acopf_layout(acopf_synth(nb, ng, nl, seed))
    return MS.Structure("case118", lay.n, lay.m, np.asarray(lay.jrow), np.asarray(lay.jcol), np.asarray(lay.hrow),
                        np.asarray(lay.hcol), np.asarray(lay.gL, float), np.asarray(lay.gU, float), {})


def _sweep(S, vals, dw, dw_last, fa, rhs, active):
    ctx = pkg.Context(S.n, S.m, 0, S.jrow, S.jcol, S.hrow, S.hcol, -np.ones(S.n), np.ones(S.n), S.gL, S.gU,
                      pkg.default_options(kkt_mode=2, kkt_condense=1), batch=B)
    st = lambda k: np.stack([v[k] for v in vals])
    out = ctx.mf_batch_test(active, st(0), st(1), st(2), st(3), st(4), st(5), np.array([v[6] for v in vals]), dw, dw_last, fa, rhs)
    census = ctx.mf_census()
    ctx.close()
    return out, sum(c for k, c in census.items() if k.startswith(FACTOR_KERNELS))


@pytest.mark.parametrize("which,launches", [("case118", (18, 16)), ("defer_leaf", (5, 4))])
def test_a_front_that_rides_in_a_later_launch_keeps_its_bits(which, launches, monkeypatch):
    """Three instances through one sweep under SQPHIP_MF_DEFER=0 and by default, a fresh context each: instance 0 well
    scaled with a shift, so both candidates are factorised and the first passes; instance 1 idle; instance 2 indefinite on
    its second attempt from delta_w = 0.  Pivots of both candidates, both solutions, decisions and shifts are equal bit for
    bit; the idle instance comes back with its right-hand side and no pivots; the default runs fewer factor launches."""
    monkeypatch.setenv("SQPHIP_MF_MERGE_T", "0")
    S = _case118_structure() if which == "case118" else defer_leaf()
    vals = [MS.values(S, "well", 11), MS.values(S, "ipm", 12), MS.values(S, "indef", 13)]
    nu = S.nu(1)
    rhs = np.random.default_rng(5).normal(size=(B, nu))
    active = np.array([b != IDLE for b in range(B)], dtype=np.int32)
    dw, dw_last, fa = np.array([1e-3, 0.0, 0.0]), np.array([0.0, 0.0, 6e-3]), np.array([0, 0, 1])
    got = {}
    for mode in ("0", None):
        if mode is None: monkeypatch.delenv("SQPHIP_MF_DEFER")
        else: monkeypatch.setenv("SQPHIP_MF_DEFER", mode)
        got[mode] = _sweep(S, vals, dw, dw_last, fa, rhs, active)
    (old, n_old), (new, n_new) = got["0"], got[None]
    print(which, "factor launches", n_old, "->", n_new, "decisions", old["decision"].tolist())
    assert (n_old, n_new) == launches
    for k in ("dinv0", "dinv1", "fused", "standalone", "decision", "dw"):
        assert np.array_equal(old[k], new[k]), (which, k)
    for out in (old, new):
        assert tuple(out["decision"][IDLE][:3]) == (0, 0, 0)
        assert np.array_equal(out["fused"][IDLE], rhs[IDLE]) and np.array_equal(out["standalone"][IDLE], rhs[IDLE])
        assert not out["dinv0"][IDLE].any() and not out["dinv1"][IDLE].any()
        # the comparison is of real work: both candidates of the speculating instances factorised, instance 0 solved
        assert tuple(out["decision"][0][:2]) == (2, 0) and out["decision"][0][4] == 1 and out["decision"][2][4] == 1
        assert np.all(out["dinv0"][[0, 2]] != 0) and np.all(out["dinv1"][[0, 2]] != 0)
        assert not np.array_equal(out["fused"][0], rhs[0])


def test_deferred_launches_give_the_same_run_end_to_end(monkeypatch):
    """Four IEEE-118 scenarios, seven SQP iterations: the same iterates bit for bit, the same per-sub-problem logs and work
    counters under SQPHIP_MF_DEFER=0 and by default; by default two factor launches per factorisation fewer -- one of
    k_mf_front<5, 4, true> (level 2: two fronts) and one of k_mf_factor2<2, 5, true> (level 0: one leaf) --, every other entry
    of the launch census equal."""
    monkeypatch.setenv("SQPHIP_MF_MERGE_T", "0")
    nb, ng, nl, seed = CASES["case118"]
    base = acopf_synth(nb, ng, nl, seed)
    nets = [base, contingency(base, 7, seed), contingency(base, 3, seed), contingency(base, 100, seed)]
    lays = [acopf_layout(nt) for nt in nets]
    opts = dict(max_iter=7, tol_infeas=1e-6, tol_residual=1e-4, use_soc=1, literal_quirks=1)
    got = {}
    for mode in ("0", None):
        if mode is None: monkeypatch.delenv("SQPHIP_MF_DEFER")
        else: monkeypatch.setenv("SQPHIP_MF_DEFER", mode)
        ctx = pkg.Context(lays[0].n, lays[0].m, lays[0].num_linear, lays[0].jrow, lays[0].jcol, lays[0].hrow, lays[0].hcol,
                          lays[0].xL, lays[0].xU, lays[0].gL, lays[0].gU, pkg.default_options(**opts), batch=len(nets))
        ctx.acopf_attach(nets[0], lays[0])
        for b in range(len(nets)):
            ctx.acopf_set_instance(b, nets[b], lays[b])
        ctx.sqp_reset(); ctx.sqp_run(0)
        c = ctx.counters()
        got[mode] = ([ctx.sqp_get(b)["x"] for b in range(4)], [ctx.sqp_qp_log(b) for b in range(4)],
                     (c["n_qp"], c["n_ipm_iter"], c["n_factor"], c["n_solve"]), c["factor_launches"], ctx.mf_census())
        ctx.close()
    old, new = got["0"], got[None]
    assert all(np.array_equal(a, b) for a, b in zip(old[0], new[0]))
    assert old[1] == new[1] and old[2] == new[2]
    assert (old[3], new[3]) == (18, 16)
    # factorisations enqueued: the factor kernels' launches over the launches of one factorisation
    nfac = [sum(c for k, c in g[4].items() if k.startswith(FACTOR_KERNELS)) / g[3] for g in (old, new)]
    assert nfac[0] == nfac[1] == int(nfac[0]) > 0
    diff = {k: old[4][k] - new[4][k] for k in old[4] if old[4][k] != new[4][k]}
    assert diff == {"k_mf_front<5, 4, true>": nfac[0], "k_mf_factor2<2, 5, true>": nfac[0]}, diff
