"""The item-parallel values kernel (k_mf_values: one thread per item, ordered sum through LDS) against the kernel it
replaces (one thread per destination, SQPHIP_MF_VALUES_SERIAL=1), bit for bit, through sqphip_mf_values_test: the IEEE-14
and IEEE-118 structures and the synthetic ones whose longest destination has 255 / 256 / 257 items (257: the plan has no
blocks and the context keeps the serial kernel).  Five instances, one idle, candidate 1 live on some (a shift > 0, a retry),
free rows in every instance.  Last: 12 IEEE-14 scenarios to termination under the four combinations of this switch and
SQPHIP_MF_F2_PACKED -- the same iterates, logs and work counters."""
import numpy as np
import pytest

import sqpsolver_jl_amd as pkg
from sqpsolver_jl_amd.acopf_synth import acopf_synth, acopf_layout, contingency, CASES
import mf_structures as MS
import mf_values_cases as VC

pytestmark = pytest.mark.gpu

STRUCTURES = {S.name: S for S in VC.structures()}
B, IDLE, SENTINEL = 5, 3, -7.5
DW = np.array([0.0, 1e-3, 0.0, 2e-3, 5e-3])
DW_LAST = np.array([0.0, 1e-4, 0.0, 0.0, 5e-3])
FAC_ATTEMPT = np.array([0, 0, 1, 0, 2])
SPEC = (FAC_ATTEMPT > 0) | (DW > 0)            # mf_speculates at spec_mode 1 (batches this small)


@pytest.mark.parametrize("name", list(STRUCTURES))
def test_item_parallel_values_equal_the_serial_kernel_bit_for_bit(name, monkeypatch):
    S = STRUCTURES[name]
    # the plan of this structure has blocks (the default run below is the item-parallel kernel) except where a destination
    # has 257 items (both runs are the serial kernel)
    nblocks = len(pkg.mf_values_blocks(S.n, S.m, S.jrow, S.jcol, S.hrow, S.hcol, S.gL, S.gU, 1)["blocks"])
    assert (nblocks == 0) if name == "items257" else (nblocks > 0), (name, nblocks)
    ctx = pkg.Context(S.n, S.m, 0, S.jrow, S.jcol, S.hrow, S.hcol, -np.ones(S.n), np.ones(S.n), S.gL, S.gU,
                      pkg.default_options(kkt_mode=2, kkt_condense=1), batch=B)
    vals = [VC.values(S, MS.VALUE_SETS[b % 3], 31 * b + 7) for b in range(B)]
    assert all((v[5] == 0).any() for v in vals)
    st = lambda k: np.stack([v[k] for v in vals])
    active = np.array([b != IDLE for b in range(B)], dtype=np.int32)
    got = {}
    for serial in (None, "1"):
        if serial is None:
            monkeypatch.delenv("SQPHIP_MF_VALUES_SERIAL", raising=False)
        else:
            monkeypatch.setenv("SQPHIP_MF_VALUES_SERIAL", serial)
        got[serial] = ctx.mf_values_test(active, st(0), st(1), st(2), st(3), st(4), st(5), np.array([v[6] for v in vals]),
                                         DW, DW_LAST, FAC_ATTEMPT, sentinel=SENTINEL)
    assert ctx.mf_census()["k_mf_values"] == 2          # one entry for whichever variant runs
    ctx.close()
    (a0, a1), (s0, s1) = got[None], got["1"]
    assert np.array_equal(a0, s0) and np.array_equal(a1, s1), name
    for b in range(B):
        if b == IDLE:
            assert (a0[b] == SENTINEL).all() and (a1[b] == SENTINEL).all()
            continue
        assert np.isfinite(a0[b]).all() and not (a0[b] == SENTINEL).any()
        if SPEC[b]:
            assert np.isfinite(a1[b]).all() and not (a1[b] == SENTINEL).any()
            assert not np.array_equal(a1[b], a0[b])      # (the next shift sits on the variables' diagonal)
        else:
            assert (a1[b] == SENTINEL).all()


def test_twelve_case14_scenarios_end_the_same_under_the_four_switch_combinations(monkeypatch):
    nb, ng, nl, seed = CASES["case14"]
    base = acopf_synth(nb, ng, nl, seed)
    nets = [base] + [contingency(base, 1 + s % 19, seed + s) for s in range(1, 12)]
    lays = [acopf_layout(nt) for nt in nets]
    kw = dict(max_iter=40, tol_infeas=1e-6, tol_residual=1e-4, use_soc=1, literal_quirks=1)
    got = {}
    for serial in ("0", "1"):
        for packed in ("1", "0"):
            monkeypatch.setenv("SQPHIP_MF_VALUES_SERIAL", serial)
            monkeypatch.setenv("SQPHIP_MF_F2_PACKED", packed)
            ctx = pkg.Context(lays[0].n, lays[0].m, lays[0].num_linear, lays[0].jrow, lays[0].jcol, lays[0].hrow, lays[0].hcol,
                              lays[0].xL, lays[0].xU, lays[0].gL, lays[0].gU, pkg.default_options(**kw), batch=len(nets))
            ctx.acopf_attach(nets[0], lays[0])
            for b in range(len(nets)):
                ctx.acopf_set_instance(b, nets[b], lays[b])
            ctx.sqp_reset(); ctx.sqp_run(0)
            c = ctx.counters()
            census = ctx.mf_census()
            assert c["sparse"] == 1 and census["k_mf_values"] > 0 and census["k_mf_factor2<1, 3, true>"] > 0
            got[serial, packed] = ([ctx.sqp_get(b)["x"] for b in range(len(nets))], [ctx.sqp_qp_log(b) for b in range(len(nets))],
                                   (c["n_qp"], c["n_ipm_iter"], c["n_factor"], c["n_solve"]))
            ctx.close()
    ref = got["0", "1"]
    for key, g in got.items():
        assert all(np.array_equal(a, b) for a, b in zip(g[0], ref[0])), key
        assert g[1] == ref[1] and g[2] == ref[2], key
