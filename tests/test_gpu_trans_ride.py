"""Transitions between sub-problems inside the sweep's post launch (ipm.hip, k_ipm_post_ride; ipm_sweep).

With the monotone barrier rule on the sparse path, in groups of at least eight instances, the work of the three transition
kernels -- k_qp_finish, the stage kernel of run!, the start of the next sub-problem in k_ipm_head -- is done by the workgroups
of the post launch whose instances are between two sub-problems; only the first sweep of every run launches the three kernels
themselves.  SQPHIP_TRANS_RIDE (read at context creation): 0 = the inline launches every fourth sweep, 2 = two rides (finish
and stage in one post launch, the start in the next), 1 = one ride.  Which sweep an instance moves on in changes nothing it
computes: every case here runs all three ways and asks for the same bits, the same outer-iteration table after every call, the
same work, mode and termination counters; only the number of sweeps may differ.  The host counter of inline transition launch
groups (sqphip_trans_inline_groups) shows that riding happened: calls x groups with it, more without."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import sqpsolver_jl_amd as pkg                                                            # noqa: E402
from sqpsolver_jl_amd.acopf_synth import acopf_synth, acopf_layout, contingency, CASES    # noqa: E402
from sqpsolver_jl_amd.qcqp import qcqp_layout, qcqp_scenario, qcqp_synth                  # noqa: E402

pytestmark = pytest.mark.gpu

FIELDS = ("x", "g", "mult_g", "mult_x_L", "mult_x_U", "obj_val", "status", "iter")
WORK = ("n_qp", "n_ipm_iter", "n_factor", "n_solve")
RIDES = ("0", "2", "1")
SQP_KW = dict(tol_infeas=1e-6, tol_residual=1e-4)


def _nets(case, count):
    nb, ng, nl, seed = CASES[case]
    base = acopf_synth(nb, ng, nl, seed)
    nets = [base] + [contingency(base, s, seed) for s in range(1, count)]
    return nets, [acopf_layout(nt) for nt in nets]


def _context(lay, kw, batch):
    return pkg.Context(lay.n, lay.m, lay.num_linear, lay.jrow, lay.jcol, lay.hrow, lay.hcol, lay.xL, lay.xU, lay.gL, lay.gU,
                       pkg.default_options(**kw), batch=batch)


def _work(ctx):
    c = ctx.counters()
    assert c["sparse"] == 1
    return ({k: c[k] for k in WORK}, ctx.mode_counters(), ctx.termination_counters()), c["n_sweeps"], c["n_groups"], \
        ctx.trans_inline_groups()


def _three_ways(monkeypatch, run):
    """run() under SQPHIP_TRANS_RIDE = 0, 2 and 1 (contexts are created inside run)"""
    out = {}
    for ride in RIDES:
        monkeypatch.setenv("SQPHIP_TRANS_RIDE", ride)
        out[ride] = run()
    monkeypatch.delenv("SQPHIP_TRANS_RIDE")
    return out


def _batched(monkeypatch, case, batch, kw):
    """The batch in three calls of two outer iterations and one to the end: per setting (results, iteration tables, work,
    sweeps, groups, inline transition launch groups)."""
    nets, lays = _nets(case, batch)

    def run():
        ctx = _context(lays[0], kw, batch)
        ctx.acopf_attach(nets[0], lays[0])
        for b in range(batch):
            ctx.acopf_set_instance(b, nets[b], lays[b])
        ctx.sqp_reset()
        its = []
        for _ in range(3):
            ctx.sqp_run(2)
            its.append(ctx.sqp_status()[1].copy())
        ctx.sqp_run(0)
        ret, it, done = ctx.sqp_status()
        assert done.all()
        its.append(it.copy())
        res = [ctx.sqp_get(b) for b in range(batch)]
        out = (res, its) + _work(ctx)
        ctx.close()
        return out

    return _three_ways(monkeypatch, run)


def _same_runs(got, batch, tag):
    old = got["0"]
    for ride in ("2", "1"):
        new = got[ride]
        print(f"{tag} ride {ride}: work {new[2][0]} sweeps {new[3]} (inline {old[3]}) inline launch groups {new[5]} ({old[5]})")
        for a, b in zip(new[1], old[1]):
            assert np.array_equal(a, b), (tag, ride)              # outer iterations per instance after every call
        for b in range(batch):
            for f in FIELDS:
                assert np.array_equal(new[0][b][f], old[0][b][f]), (tag, ride, b, f)
        assert new[2] == old[2], (tag, ride)


@pytest.mark.parametrize("quirks", [1, 0])
@pytest.mark.parametrize("batch", [12, 64])
def test_riding_transitions_give_the_bits_of_the_inline_launches(batch, quirks, monkeypatch):
    """IEEE-14 shape: 12 instances (one group of at least eight) and 64 (four groups of 16), both Hessian signs.  With riding
    only the first sweep of each of the four calls launches the transition kernels, in every group."""
    kw = dict(kkt_mode=2, max_iter=8, use_soc=1, literal_quirks=quirks, **SQP_KW)
    got = _batched(monkeypatch, "case14", batch, kw)
    groups = 4 if batch == 64 else 1
    assert got["0"][4] == got["2"][4] == got["1"][4] == groups
    _same_runs(got, batch, f"case14 batch {batch} quirks {quirks}")
    calls = 4
    assert got["2"][5] == got["1"][5] == calls * groups
    assert got["0"][5] > calls * groups


def test_riding_transitions_on_the_ieee118_shape(monkeypatch):
    """IEEE-118 shape, 12 instances with the reference's Hessian sign: second-order corrections, restoration sub-problems and
    refinement requests meet the rides (the entry-state dispatch sits beside the one that serves refinement solves)."""
    kw = dict(max_iter=8, use_soc=1, literal_quirks=1, **SQP_KW)
    got = _batched(monkeypatch, "case118", 12, kw)
    _same_runs(got, 12, "case118 batch 12")
    assert got["0"][4] == got["2"][4] == got["1"][4] == 1                 # one group: four calls, four inline launch groups
    assert got["2"][5] == got["1"][5] == 4 and got["0"][5] > 4
    for ride in RIDES:
        w = got[ride][2][0]
        assert w["n_solve"] > w["n_ipm_iter"], f"ride {ride}: no refinement solve in this run"


def _acopf_queue(nets, lays, M, slots, kw):
    q = _context(lays[0], kw, slots)
    q.acopf_attach(nets[0], lays[0])
    q.stream_begin(M)
    for s in range(M):
        q.stream_set(s, nets[s], lays[s])
    return q


def test_riding_transitions_through_the_scenario_queue(monkeypatch):
    """24 IEEE-14-shaped scenarios through 8 slots: a slot files its result, draws the next scenario and runs the prologue of
    run! inside a ride.  Every scenario filed once (the totals of sub-problems agree), with the same bits."""
    M, slots = 24, 8
    nets, lays = _nets("case14", M)
    kw = dict(kkt_mode=2, max_iter=8, use_soc=1, literal_quirks=1, **SQP_KW)

    def run():
        q = _acopf_queue(nets, lays, M, slots, kw)
        q.stream_run()
        res = [q.stream_get(s) for s in range(M)]
        assert q.sqp_status()[2].all()
        out = (res,) + _work(q)
        q.close()
        return out

    got = _three_ways(monkeypatch, run)
    for ride in RIDES:
        assert all(r["iter"] >= 1 for r in got[ride][0]), ride            # (a scenario nobody filed reports iter = -1)
    for ride in ("2", "1"):
        for s in range(M):
            for f in ("x", "obj_val", "status", "iter"):
                assert np.array_equal(got[ride][0][s][f], got["0"][0][s][f]), (ride, s, f)
        assert got[ride][1] == got["0"][1], ride
        assert got[ride][3] == got["0"][3] == 1                           # n_groups
        assert got[ride][4] == 1 and got["0"][4] > 1                      # one run of one group


def _qcqp_problem(problem, M):
    if problem == "synth":
        q0 = qcqp_synth(24, 14, seed=5)
        return q0, qcqp_layout(q0), [qcqp_scenario(q0, s, 5) for s in range(M)], 60
    # IEEE-14-shaped contingencies in rectangular coordinates, extracted as general QCQPs (tests/test_gpu_qcqp_stream.py)
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from oracle import oracle as O
    from qcqp_ref import extract
    from sqpsolver_jl_amd.acopf_synth import acr_layout
    nb, ng, nl, seed = CASES["case14"]
    base = acopf_synth(nb, ng, nl, seed)
    nets = [base] + [contingency(base, s, seed) for s in range(1, M)]
    lays = [acr_layout(nt) for nt in nets]
    qs = extract([O.problem_acopf(nt, ly) for nt, ly in zip(nets, lays)])
    return qs[0], lays[0], qs, 8


@pytest.mark.parametrize("problem", ["synth", "acr14"])
def test_riding_transitions_through_the_qcqp_queue(problem, monkeypatch):
    """16 scenarios through 8 slots of a QCQP context on the sparse solver, multipliers kept.  synth: the synthetic QCQP of
    tests/test_gpu_qcqp_stream.py -- its multifrontal plan has no streamed top, so the transitions stay in line whatever the
    switch says (the condition of ipm_sweep) and the case shows that the switch changes nothing there.  acr14: IEEE-14-shaped
    contingencies in rectangular coordinates as general QCQPs -- the slots are refilled with QCQP values inside a ride."""
    M, slots = 16, 8
    q0, lay, qs, max_iter = _qcqp_problem(problem, M)
    kw = dict(kkt_mode=2, max_iter=max_iter, use_soc=1, literal_quirks=0, **SQP_KW)

    def run():
        ctx = _context(lay, kw, slots)
        ctx.qcqp_attach(q0)
        ctx.qcqp_stream_begin(M, keep_multipliers=True)
        for s in range(M):
            ctx.qcqp_stream_set(s, qs[s])
        ctx.stream_run()
        res = [ctx.stream_get_full(s) for s in range(M)]
        assert ctx.sqp_status()[2].all()
        out = (res,) + _work(ctx)
        ctx.close()
        return out

    got = _three_ways(monkeypatch, run)
    assert any(np.abs(r["mult_g"]).max() > 0 for r in got["0"][0])        # (the comparison is not one of zeros)
    assert all(r["iter"] >= 1 for r in got["0"][0])
    for ride in ("2", "1"):
        print(f"qcqp {problem} ride {ride}: work {got[ride][1][0]} sweeps {got[ride][2]} ({got['0'][2]}) inline launch groups {got[ride][4]} ({got['0'][4]})")
        for s in range(M):
            for f in FIELDS:
                assert np.array_equal(got[ride][0][s][f], got["0"][0][s][f]), (ride, s, f)
        assert got[ride][1] == got["0"][1], ride
        assert got[ride][3] == got["0"][3] == 1                           # n_groups: one run of one group
        if problem == "acr14":
            assert got[ride][4] == 1 and got["0"][4] > 1
        else:
            assert got[ride][4] == got["0"][4] and got[ride][2] == got["0"][2]


def test_the_switch_changes_nothing_below_eight_instances(monkeypatch):
    """A group of three: no riding, whatever the switch says -- the same sweeps and inline launch groups too."""
    kw = dict(kkt_mode=2, max_iter=8, use_soc=1, literal_quirks=1, **SQP_KW)
    got = _batched(monkeypatch, "case14", 3, kw)
    _same_runs(got, 3, "case14 batch 3")
    for ride in ("2", "1"):
        assert got[ride][3] == got["0"][3] and got[ride][5] == got["0"][5]


def test_a_second_run_on_the_context_gives_the_inline_results(monkeypatch):
    """After a run has ended: sqp_reset and a second sqp_run on the same context, and a second stream_run over the same
    queue -- the first sweep of the new run carries the transitions in line, the rest rides."""
    nets, lays = _nets("case14", 12)
    kw = dict(kkt_mode=2, max_iter=8, use_soc=1, literal_quirks=1, **SQP_KW)

    def run():
        ctx = _context(lays[0], kw, 12)
        ctx.acopf_attach(nets[0], lays[0])
        for b in range(12):
            ctx.acopf_set_instance(b, nets[b], lays[b])
        ctx.sqp_reset(); ctx.sqp_run(0)
        first = [ctx.sqp_get(b) for b in range(12)]
        ctx.sqp_reset(); ctx.sqp_run(0)
        assert ctx.sqp_status()[2].all()
        second = [ctx.sqp_get(b) for b in range(12)]
        inline_b = ctx.trans_inline_groups()
        ctx.close()
        q = _acopf_queue(nets, lays, 12, 8, kw)
        q.stream_run()
        q.stream_run()
        assert q.sqp_status()[2].all()
        queue = [q.stream_get(s) for s in range(12)]
        inline_q = q.trans_inline_groups()
        q.close()
        return first, second, queue, inline_b, inline_q

    got = _three_ways(monkeypatch, run)
    for ride in ("2", "1"):
        for b in range(12):
            for f in FIELDS:
                assert np.array_equal(got[ride][1][b][f], got["0"][1][b][f]), (ride, b, f)
            for f in ("x", "obj_val", "status", "iter"):
                assert np.array_equal(got[ride][2][b][f], got["0"][2][b][f]), (ride, b, f)
        assert got[ride][3] == 2 and got[ride][4] == 2
