"""The working vector of the solves from entry-parallel terms in LDS (ipm.hip, solve_vector_terms)
against the column walk it replaces in build_rhs (solve_vector_at / load_solve_vector), bit for bit.

Kernel level (sqphip_solve_vector_test): five distinct instances per call, one of them inactive, on the sparse context and
on the dense one (kkt_mode = 1: another order of the factorised matrix, the same two routines).  Right-hand sides and
Jacobian values carry signed zeros: an entry that must be skipped and is added instead as + 0.0 turns a - 0.0 into + 0.0, which
only a comparison of the bits sees.  Row types per instance: from the bounds (equality rows stay in the matrix, every other
row is eliminated), the LP phase's (every nonlinear row free), a random mix, and -- a contingency's values -- the bounds
again.  The ACOPF layouts themselves have no free row (an outage zeroes admittances, the bounds stay): free rows come in as
the interior-point method sets them, through the row types.

Run level: contexts created with SQPHIP_XV_TERMS=0 and without must give the same bits and the same work.

No tolerance anywhere: every comparison is exact."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import sqpsolver_jl_amd as pkg                                                            # noqa: E402
from sqpsolver_jl_amd.acopf_synth import acopf_synth, acopf_layout, contingency, CASES    # noqa: E402

pytestmark = pytest.mark.gpu

B, IDLE = 5, 2
SENT = pkg.Context.SOLVE_VECTOR_SENTINEL
ROW_FREE, ROW_EQ, ROW_INEQ = 0, 1, 2
FIELDS = ("x", "g", "mult_g", "mult_x_L", "mult_x_U", "obj_val", "status", "iter")
WORK = ("n_qp", "n_ipm_iter", "n_factor", "n_solve")
SQP_KW = dict(tol_infeas=1e-6, tol_residual=1e-4)
_LAYOUTS = {}


def _layout(case):
    if case not in _LAYOUTS:
        nb, ng, nl, seed = CASES[case]
        base = acopf_synth(nb, ng, nl, seed)
        _LAYOUTS[case] = (base, acopf_layout(base), seed)
    return _LAYOUTS[case]


def _context(lay, batch, **kw):
    return pkg.Context(lay.n, lay.m, lay.num_linear, lay.jrow, lay.jcol, lay.hrow, lay.hcol, lay.xL, lay.xU, lay.gL, lay.gU,
                       pkg.default_options(**kw), batch=batch)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _with_signed_zeros(rng, a, frac):
    """a with a fraction of its entries replaced by + 0.0 and - 0.0 (half each)"""
    z = rng.random(a.shape)
    a = a.copy()
    a[z < frac / 2] = 0.0
    a[(z >= frac / 2) & (z < frac)] = -0.0
    return a


def _inputs(lay, seed):
    """Jacobian values, D, row types and right-hand sides of the five instances, and how many Jacobian entries of the
    active instances the condensed form adds / skips (rows that stay in the matrix -- gL == gU in the structure -- and
    free rows are skipped)."""
    rng = np.random.default_rng(seed)
    n, m, nnz = lay.n, lay.m, len(lay.jrow)
    kept = lay.gL == lay.gU
    from_bounds = np.where(kept, ROW_EQ, ROW_INEQ).astype(np.int32)
    lp_phase = from_bounds.copy(); lp_phase[lay.num_linear:] = ROW_FREE             # (b_ipm_start, LP phase)
    mixed = rng.integers(0, 3, size=m).astype(np.int32)
    rtype = np.stack([from_bounds, lp_phase, mixed, mixed[::-1].copy(), from_bounds])
    jval = _with_signed_zeros(rng, rng.normal(size=(B, nnz)), 0.1)
    # D at the scales the interior-point method produces, a few exact zeros (the regularisation is what is divided by)
    Dd = np.exp(rng.uniform(np.log(1e-9), np.log(1e9), size=(B, m)))
    Dd[rng.random((B, m)) < 0.02] = 0.0
    rhs = _with_signed_zeros(rng, rng.normal(size=(B, n + m)), 0.3)
    rhs[0, :n] = -0.0                 # every variable of instance 0 starts from - 0.0: a lost skip there cannot hide
    active = np.array([b != IDLE for b in range(B)], dtype=np.int32)
    rows = np.asarray(lay.jrow, dtype=np.int64) - 1                  # (the layouts count from one)
    added = skipped = 0
    for b in range(B):
        if active[b]:
            a = (rtype[b][rows] != ROW_FREE) & ~kept[rows]
            added += int(a.sum()); skipped += int((~a).sum())
    return active, jval, Dd, rtype, rhs, added, skipped


def _check(case, seed, **kw):
    base, lay, _ = _layout(case)
    ctx = _context(lay, B, **kw)
    active, jval, Dd, rtype, rhs, added, skipped = _inputs(lay, seed)
    assert added > 0 and skipped > 0, (case, added, skipped)
    plain, terms, mismatch = ctx.solve_vector_test(active, jval, Dd, rtype, rhs)
    ctx.close()
    print(f"[xv-terms] {case} {kw}: Fpad {plain.shape[1]}, entries added {added} skipped {skipped}, mismatch {mismatch}")
    assert mismatch == 0, (case, kw, mismatch)
    assert np.array_equal(plain, terms, equal_nan=True), (case, kw)
    assert np.array_equal(_bits(plain), _bits(terms)), (case, kw)
    assert (plain[IDLE] == SENT).all() and (terms[IDLE] == SENT).all(), (case, kw, "the inactive instance was written")
    for b in range(B):
        if b != IDLE:       # (written everywhere: padding positions hold 0.0)
            assert not (terms[b] == SENT).any() and np.abs(terms[b][np.isfinite(terms[b])]).max() > 0, (case, kw, b)
    return plain


MODES = {"sparse": dict(kkt_mode=2), "dense": dict(kkt_mode=1)}


@pytest.mark.parametrize("mode", list(MODES))
def test_ieee14_threads_without_position_or_entry(mode):
    """IEEE-14 polar: Fpad and the 651 entries both below one stride of 1 024 threads (threads with neither a position nor
    an entry), a 30-entry column, the last ballot word partial (651 = 10 x 64 + 11)."""
    _, lay, _ = _layout("case14")
    assert len(lay.jrow) == 651
    plain = _check("case14", 11, **MODES[mode])
    assert plain.shape[1] < 1024


@pytest.mark.parametrize("mode", list(MODES))
def test_ieee118_third_trip_ragged_stride_longest_column(mode):
    """IEEE-118 polar: Fpad above 2 x 1 024 (a third trip for some threads), 6 061 = 5 x 1 024 + 941 entries (the sixth
    stride ragged), the 42-entry column."""
    _, lay, _ = _layout("case118")
    assert len(lay.jrow) == 6061
    plain = _check("case118", 12, **MODES[mode])
    assert plain.shape[1] > 2048


@pytest.mark.parametrize("mode", list(MODES))
def test_contingency_values_with_free_and_kept_rows(mode):
    """The Jacobian of a contingency scenario near its start point (the outaged branch's entries are exact zeros) in every
    instance's values, free rows and kept equality rows beside eliminated ones."""
    base, lay, seed = _layout("case14")
    from oracle import oracle as O
    net = contingency(base, 3, seed)
    layc = acopf_layout(net)
    P = O.problem_acopf(net, layc)
    x = np.asarray(layc.x0, dtype=np.float64) + 0.05 * np.random.default_rng(5).normal(size=lay.n)
    jac = np.asarray(P.eval_jac_g(x), dtype=np.float64)
    assert jac.shape == (len(lay.jrow),) and (jac == 0.0).any() and (jac != 0.0).sum() > len(jac) // 2
    ctx = _context(lay, B, **MODES[mode])
    active, jval, Dd, rtype, rhs, added, skipped = _inputs(lay, 13)
    jval = np.stack([jac * (1.0 + 0.1 * b) for b in range(B)])
    jval[1][jac == 0.0] = -0.0
    assert added > 0 and skipped > 0
    plain, terms, mismatch = ctx.solve_vector_test(active, jval, Dd, rtype, rhs)
    ctx.close()
    assert mismatch == 0
    assert np.array_equal(plain, terms, equal_nan=True) and np.array_equal(_bits(plain), _bits(terms))
    assert (plain[IDLE] == SENT).all() and (terms[IDLE] == SENT).all()


@pytest.mark.parametrize("how", ["kkt_condense=0", "SQPHIP_NO_VSTAGE=1", "SQPHIP_XV_TERMS=0"])
def test_the_hook_reports_a_context_without_the_stage(how, monkeypatch):
    """Each of the three switches leaves the context without the stage: the hook says so (SQPHIP_ESTATE)."""
    _, lay, _ = _layout("case14")
    kw = dict(kkt_mode=2)
    if how == "kkt_condense=0":
        kw["kkt_condense"] = 0
    else:
        name, val = how.split("=")
        monkeypatch.setenv(name, val)
    ctx = _context(lay, B, **kw)
    active, jval, Dd, rtype, rhs, _, _ = _inputs(lay, 14)
    with pytest.raises(pkg.SqpHipError):
        ctx.solve_vector_test(active, jval, Dd, rtype, rhs)
    ctx.close()


def _run(case, batch, kw, outer):
    base, lay0, seed = _layout(case)
    nets = [base] + [contingency(base, s, seed) for s in range(1, batch)]
    lays = [lay0] + [acopf_layout(nt) for nt in nets[1:]]
    ctx = _context(lay0, batch, **kw)
    ctx.acopf_attach(base, lay0)
    for b in range(batch):
        ctx.acopf_set_instance(b, nets[b], lays[b])
    ctx.sqp_reset()
    ctx.sqp_run(outer)
    res = [ctx.sqp_get(b) for b in range(batch)]
    c = ctx.counters()
    work = ({k: c[k] for k in WORK}, ctx.mode_counters(), ctx.termination_counters())
    ctx.close()
    return res, work


def _same_with_and_without(monkeypatch, case, kw, tag):
    monkeypatch.setenv("SQPHIP_XV_TERMS", "0")
    old = _run(case, 8, kw, 3)
    monkeypatch.delenv("SQPHIP_XV_TERMS")
    new = _run(case, 8, kw, 3)
    print(f"[xv-terms] run {tag}: work {new[1][0]}")
    assert new[1][0]["n_ipm_iter"] > 0
    for b in range(8):
        for f in FIELDS:
            assert np.array_equal(new[0][b][f], old[0][b][f]), (tag, b, f)
            assert np.array_equal(_bits(new[0][b][f]), _bits(old[0][b][f])), (tag, b, f)
    assert new[1] == old[1], tag


@pytest.mark.parametrize("ride", [None, "0"], ids=["ride", "SQPHIP_TRANS_RIDE=0"])
@pytest.mark.parametrize("quirks", [1, 0])
@pytest.mark.parametrize("case", ["case14", "case118"])
def test_a_run_gives_the_same_bits_with_and_without_the_stage(case, quirks, ride, monkeypatch):
    """Eight scenarios, three outer iterations, both Hessian signs: results, multipliers, status, iterations, work, mode and
    termination counters of a context with the stage and of one created under SQPHIP_XV_TERMS=0.  Default launches
    (k_ipm_post_ride) and SQPHIP_TRANS_RIDE=0 (k_ipm_post<PH_SOLVE, true>, k_ipm_head)."""
    if ride is not None:
        monkeypatch.setenv("SQPHIP_TRANS_RIDE", ride)
    kw = dict(kkt_mode=2, max_iter=8, use_soc=1, literal_quirks=quirks, **SQP_KW)
    _same_with_and_without(monkeypatch, case, kw, f"{case} quirks {quirks} ride {ride}")


@pytest.mark.parametrize("quirks", [1, 0])
def test_a_predictor_corrector_run_gives_the_same_bits(quirks, monkeypatch):
    """options.ipm_corrector = 1 on the IEEE-14 shape: the corrector's right-hand side (b_mpc -> build_rhs)."""
    kw = dict(kkt_mode=2, max_iter=8, use_soc=1, literal_quirks=quirks, ipm_corrector=1, **SQP_KW)
    _same_with_and_without(monkeypatch, "case14", kw, f"case14 corrector quirks {quirks}")
