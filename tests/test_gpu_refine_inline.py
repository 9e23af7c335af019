"""Refinement solves in the sweep's own solve chain, and the sweep's counters from k_ipm_post (ipm.hip, ipm_sweep).

With the monotone barrier rule on the sparse path an instance that asks for a refinement step (PH_RESOLVE) is served by the
regular solve chain of a later sweep -- forward level launches gated to it, then the top launch, the backward levels and
k_ipm_post shared with everybody else -- instead of a second chain of eight gated launches; the "anyone left?" counts of a
sweep are formed by the workgroups of k_ipm_post instead of k_sqp_count.  SQPHIP_REFINE_SLOT=1 (read at context creation)
keeps the old sequence.  Which sweep serves an instance changes nothing it computes: every case here runs both ways and asks
for the same bits, the same work counters and the same number of outer iterations; only the number of sweeps may differ.
Every case also asserts that refinement solves happened (more solves than interior-point iterations)."""
import numpy as np
import pytest

import sqpsolver_jl_amd as pkg
from sqpsolver_jl_amd.acopf_synth import acopf_synth, acopf_layout, contingency, CASES

pytestmark = pytest.mark.gpu

FIELDS = ("x", "g", "mult_g", "mult_x_L", "mult_x_U", "obj_val", "status", "iter")
WORK = ("n_qp", "n_ipm_iter", "n_factor", "n_solve")


def _case118(count):
    nb, ng, nl, seed = CASES["case118"]
    base = acopf_synth(nb, ng, nl, seed)
    nets = [base] + [contingency(base, s, seed) for s in range(1, count)]
    return nets, [acopf_layout(nt) for nt in nets]


def _context(lay, kw, batch):
    return pkg.Context(lay.n, lay.m, lay.num_linear, lay.jrow, lay.jcol, lay.hrow, lay.hcol, lay.xL, lay.xU, lay.gL, lay.gU,
                       pkg.default_options(**kw), batch=batch)


def _work(ctx):
    c = ctx.counters()
    return {k: c[k] for k in WORK}, ctx.mode_counters(), ctx.termination_counters(), c["n_sweeps"]


def _both_ways(monkeypatch, run):
    """run() the new way and under SQPHIP_REFINE_SLOT=1"""
    out = {}
    for slot in ("0", "1"):
        monkeypatch.setenv("SQPHIP_REFINE_SLOT", slot)
        out[slot] = run()
    monkeypatch.delenv("SQPHIP_REFINE_SLOT")
    return out["0"], out["1"]


def _same_work(new, old, tag):
    print(f"{tag}: work {new[0]} sweeps new / slot {new[3]} / {old[3]}, refinement solves {new[0]['n_solve'] - new[0]['n_ipm_iter']}")
    assert new[0] == old[0] and new[1] == old[1] and new[2] == old[2], tag
    assert old[0]["n_solve"] > old[0]["n_ipm_iter"], f"{tag}: no refinement solve in this run"


@pytest.mark.parametrize("quirks", [1, 0])
@pytest.mark.parametrize("batch", [12, 128])
def test_refinement_in_the_solve_chain_gives_the_bits_of_the_second_slot(batch, quirks, monkeypatch):
    """Batched runs on the IEEE-118 shape: 12 instances (one group, the two-shift speculation active) and 128 (four groups),
    with the sign that produces refinement requests (literal_quirks = 1) and without.  The run is cut into calls of two outer
    iterations each, so the counters also end every call after the same number of outer iterations per instance."""
    nets, lays = _case118(batch)
    kw = dict(max_iter=8, tol_infeas=1e-6, tol_residual=1e-4, use_soc=1, literal_quirks=quirks)

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
        groups = ctx.counters()["n_groups"]
        work = _work(ctx)
        ctx.close()
        return res, its, work, groups

    new, old = _both_ways(monkeypatch, run)
    assert new[3] == old[3] == (4 if batch == 128 else 1)
    for a, b in zip(new[1], old[1]):
        assert np.array_equal(a, b)                      # outer iterations per instance after every call
    for b in range(batch):
        for f in FIELDS:
            assert np.array_equal(new[0][b][f], old[0][b][f]), (b, f)
    _same_work(new[2], old[2], f"batch {batch} quirks {quirks}")


def test_refinement_in_the_solve_chain_through_the_scenario_queue(monkeypatch):
    """12 IEEE-118-shaped scenarios through 4 slots: a slot is refilled on the device while others wait for a refinement."""
    M, slots = 12, 4
    nets, lays = _case118(M)
    kw = dict(max_iter=8, tol_infeas=1e-6, tol_residual=1e-4, use_soc=1, literal_quirks=1)

    def run():
        q = _context(lays[0], kw, slots)
        q.acopf_attach(nets[0], lays[0])
        q.stream_begin(M)
        for s in range(M):
            q.stream_set(s, nets[s], lays[s])
        q.stream_run()
        res = [q.stream_get(s) for s in range(M)]
        assert q.sqp_status()[2].all()
        work = _work(q)
        q.close()
        return res, work

    new, old = _both_ways(monkeypatch, run)
    for s in range(M):
        for f in ("x", "obj_val", "status", "iter"):
            assert np.array_equal(new[0][s][f], old[0][s][f]), (s, f)
    _same_work(new[1], old[1], "scenario queue")


def test_refinement_in_the_solve_chain_through_the_drop_in_seat(monkeypatch):
    """sqphip_qp_solve (no SQP-level kernels, every sweep serves, counters by k_count): the sub-problems of a batched run on
    the IEEE-118 shape -- the one each of 12 instances worked on last in each of 8 outer iterations, taken from the device --
    replayed through a one-instance context.  The batched run and the seat are one code path, so the replays hold the
    refinement steps of the run."""
    B, iters = 12, 8
    nets, lays = _case118(B)
    kw = dict(max_iter=3000, tol_infeas=1e-6, tol_residual=1e-4, use_soc=1, literal_quirks=1)
    ctx = _context(lays[0], kw, B)
    ctx.acopf_attach(nets[0], lays[0])
    for b in range(B):
        ctx.acopf_set_instance(b, nets[b], lays[b])
    ctx.sqp_reset()
    calls = []
    for _ in range(iters):
        ctx.sqp_run(1)
        for b in range(B):
            rq = ctx.sqp_last_request(b)
            calls.append((b, (rq["mode"], rq["x_k"], rq["delta"], rq["mu_pen"], rq["c"], rq["b"], rq["jac_coo"], rq["hess_coo"])))
    ctx.close()

    def run():
        seats = [_context(lays[b], kw, 1) for b in range(B)]
        res = [seats[b].qp_solve(*args) for b, args in calls]
        work = {k: sum(c.counters()[k] for c in seats) for k in WORK}
        for c in seats:
            c.close()
        return res, work

    new, old = _both_ways(monkeypatch, run)
    for k, (a, b) in enumerate(zip(new[0], old[0])):
        for f in a:
            assert np.array_equal(a[f], b[f]), (k, f)
    print(f"drop-in seat: {len(calls)} sub-problems, work {new[1]}, refinement solves {new[1]['n_solve'] - new[1]['n_ipm_iter']}")
    assert new[1] == old[1]
    assert old[1]["n_solve"] > old[1]["n_ipm_iter"], "drop-in seat: no refinement solve in these sub-problems"
