"""The merit and line-search seat (`sqphip_norm_violations`, `_kt_residuals`, `_norm_complementarity`, `_compute_phi`,
`_compute_qmodel`, `_compute_derivative`, `_compute_derivative_full`, `_compute_mu_rule_dev`, their `*_batch` forms and
`sqphip_acopf_armijo`) on the structures of tests/merit_cases.py: k_merit, k_merit_batch, the three k_armijo<KIND> of
csrc/sqp.hip and k_seat_stage of csrc/api.hip at sizes around one wave (64), one workgroup (1024 threads, the stride of every
loop of merit_body) and beyond two strides, with no rows, repeated COO entries, empty rows and columns, a completely dense
Hessian, a null Hval, equal / one-sided / infinite bounds, values exactly on a bound and a staged field longer than one
trip of k_seat_stage's grid.

The reference is tests/merit_ref.py: exact rational arithmetic over the float64 operands, rounded once.  The tolerance is
derived there, not measured: |got - r| <= 2 * depth * 2^-53 * mag per result, propagated through the quotients, and `==`
where a result is made of comparisons, differences of two operands and a max.  tests/test_merit_cases_cpu.py holds the
oracle and numpy to the same rule at every case, and the Armijo inputs to the margins that make the loop's decisions
independent of rounding."""
import math

import numpy as np
import pytest

import sqpsolver_jl_amd as pkg
from sqpsolver_jl_amd.host import SqpHipError
import merit_cases as MC
import merit_ref as MR

pytestmark = pytest.mark.gpu
PNORMS = MR.PNORMS

_ctxs: dict = {}
_refs: dict = {}


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for ctx in _ctxs.values():
        ctx.close()
    _ctxs.clear(); _refs.clear()


def _ctx(name):
    """One context of batch 1 per case: each shape is analysed once"""
    if name not in _ctxs:
        _ctxs[name] = pkg.Context(*MC.case(name).ctx_args())
    return _ctxs[name]


def _ref(name, oset):
    if (name, oset) not in _refs:
        c = MC.case(name)
        _refs[name, oset] = MR.reference_values(c.P, c.B, c.ops[oset])
    return _refs[name, oset]


def scalar_ops(ctx, o):
    """{key: call} of every scalar entry point on operands o, keyed as merit_ref.reference_values"""
    ops = {}
    for pn in PNORMS:
        ops["viol", pn] = lambda pn=pn: ctx.norm_violations(o.E, o.x, pn)
        ops["compl", pn] = lambda pn=pn: ctx.norm_complementarity(o.E, o.lam, pn)
    ops["kt"] = lambda: ctx.kt_residuals(o.df, o.lam, o.mult_x_U, o.mult_x_L, o.Jval)
    for fr in (0, 1):
        ops["phi", fr] = lambda fr=fr: ctx.compute_phi(o.f, o.E, o.x, o.mu, fr)
    ops["q", "step"] = lambda: ctx.compute_qmodel(o.x, o.p, o.df, o.E, o.Jval, o.Hval, o.mu, True)
    ops["q", "nohess"] = lambda: ctx.compute_qmodel(o.x, o.p, o.df, o.E, o.Jval, None, o.mu, True)
    ops["q", "nostep"] = lambda: ctx.compute_qmodel(o.x, o.p, o.df, o.E, o.Jval, o.Hval, o.mu, False)
    ops["D5"] = lambda: ctx.compute_derivative(o.df, o.p, o.E, o.mu)
    for vec in (False, True):
        for fr in (0, 1):
            ops["D", vec, fr] = lambda vec=vec, fr=fr: ctx.compute_derivative_full(
                o.df, o.p, o.E, o.mu, mu_vec=o.mu_vec if vec else None, feasibility_restoration=bool(fr), slack=o.slack)
    for rule in (1, 2, 3):
        for it in (1, 4):
            ops["mu", rule, it] = lambda rule=rule, it=it: ctx.compute_mu_rule(rule, it, o.rho, o.x, o.E, o.df, o.p, o.Hval, o.lam, o.mu_vec)
    return ops


def _bits(v):
    return v.tobytes() if isinstance(v, np.ndarray) else np.float64(v).tobytes()


# ------------------------------------------------------------------ 1. every op at every case
@pytest.mark.parametrize("name", MC.ALL_NAMES)
def test_every_op_at_every_case(name):
    c = MC.case(name); ctx = _ctx(name)
    for oset in (0, 1):
        got = {key: call() for key, call in scalar_ops(ctx, c.ops[oset]).items()}
        ref = _ref(name, oset)
        assert set(got) == set(ref)
        MR.check_against(ref, got, f"{name} set {oset}")
        assert ref["viol", math.inf].exact


# ------------------------------------------------------------------ 2. no op depends on the calls before it
@pytest.mark.parametrize("name", ["65x63-dups", "1025x1023", "hfull-65"])
def test_results_do_not_depend_on_the_calls_before(name):
    """The ops in two shuffled orders, a call on the OTHER operand set between any two: the same bits in both runs, and the
    reference's value.  An op that read a vector an earlier call left in instance 0's slots -- jcoo after
    compute_mu_rule_dev has cleared it, plam after a vector-penalty call -- would differ between the orders."""
    c = MC.case(name); ctx = _ctx(name)
    for oset in (0, 1):
        mine, other = scalar_ops(ctx, c.ops[oset]), list(scalar_ops(ctx, c.ops[1 - oset]).values())
        keys = list(mine)
        runs = []
        for seed in (1, 2):
            rng = np.random.default_rng([43, seed, oset])
            got = {}
            for k in rng.permutation(len(keys)):
                got[keys[k]] = mine[keys[k]]()
                other[int(rng.integers(len(other)))]()
            runs.append(got)
        for key in keys:
            assert _bits(runs[0][key]) == _bits(runs[1][key]), (name, oset, key)
        MR.check_against(_ref(name, oset), runs[1], f"{name} set {oset} shuffled")


# ------------------------------------------------------------------ 3. the batch forms
REQUESTS = ([4], [3, 0], [1, 4, 2, 0, 3])


def batch_ops(ctx, inst, os_):
    """{key: call} of every *_batch entry point for the requests `inst` with operands os_[k]: each returns [count] values"""
    col = lambda f: [getattr(o, f) for o in os_]
    ops = {}
    for pn in PNORMS:
        ops["viol", pn] = lambda pn=pn: ctx.norm_violations_batch(inst, col("E"), col("x"), pn)
        ops["compl", pn] = lambda pn=pn: ctx.norm_complementarity_batch(inst, col("E"), col("lam"), pn)
    ops["kt"] = lambda: ctx.kt_residuals_batch(inst, col("df"), col("lam"), col("mult_x_U"), col("mult_x_L"), col("Jval"))
    for fr in (0, 1):
        ops["phi", fr] = lambda fr=fr: ctx.compute_phi_batch(inst, col("f"), col("E"), col("x"), col("mu"), fr)
    ops["q", "step"] = lambda: ctx.compute_qmodel_batch(inst, col("x"), col("p"), col("df"), col("E"), col("Jval"), col("Hval"), col("mu"), True)
    ops["q", "nohess"] = lambda: ctx.compute_qmodel_batch(inst, col("x"), col("p"), col("df"), col("E"), col("Jval"), None, col("mu"), True)
    ops["q", "nostep"] = lambda: ctx.compute_qmodel_batch(inst, col("x"), col("p"), col("df"), col("E"), col("Jval"), col("Hval"), col("mu"), False)
    for vec in (False, True):
        for fr in (0, 1):
            ops["D", vec, fr] = lambda vec=vec, fr=fr: ctx.compute_derivative_full_batch(
                inst, col("df"), col("p"), col("E"), col("mu"), mu_vec=col("mu_vec") if vec else None, feasibility_restoration=bool(fr),
                slack=col("slack"))
    return ops


@pytest.mark.parametrize("name", ["long-row", "1025x1023"])
def test_batch_forms_on_odd_shapes_and_long_rows(name):
    """A context of batch 5, bounds per instance; every *_batch entry point on one, two and five requests in permuted
    order: each value meets the reference of its request's operands under its instance's bounds and is bit-equal to the
    scalar call on a batch-1 context with those bounds.  `seat_check` (api.hip) demands pairwise distinct instances of
    every batch call, merit calls included: [2, 2] is refused, and the context serves the next call."""
    c = MC.case(name); P = c.P
    Bs = [MC.bounds(P.n, P.m, bseed=10 + b) for b in range(5)]
    os_ = [MC.operands(P, Bs[b], oset=b % 2, oseed=10 + b) for b in range(5)]
    assert len({B.gL.tobytes() for B in Bs}) == len({B.xU.tobytes() for B in Bs}) == len({o.E.tobytes() for o in os_}) == 5
    if name == "long-row":
        assert c.longest_field() > MC.STAGE_PASS and c.row_doubles() > MC.STAGE_PASS and P.n % 2 == P.m % 2 == len(P.jrow) % 2 == len(P.hrow) % 2 == 1
    refs = [MR.reference_values(P, Bs[b], os_[b]) for b in range(5)]
    one = _ctx(name)                                             # the batch-1 context, its bounds set per instance below
    single = []
    try:
        for b in range(5):
            one.set_bounds(0, Bs[b])
            single.append({key: call() for key, call in scalar_ops(one, os_[b]).items() if key[0] not in ("mu", "D5")})
    finally:
        one.set_bounds(0, c.B)                                   # the cached context serves other tests with the case's bounds
    ctx = pkg.Context(*c.ctx_args(), batch=5)
    try:
        for b in range(5):
            ctx.set_bounds(b, Bs[b])
        for inst in REQUESTS:
            for key, call in batch_ops(ctx, inst, [os_[b] for b in inst]).items():
                out = call()
                assert out.shape == (len(inst),)
                for k, b in enumerate(inst):
                    MR.check_against({key: refs[b][key]}, {key: float(out[k])}, f"{name} request {k} of {inst} on instance {b}")
                    assert _bits(out[k]) == _bits(single[b][key]), (name, inst, k, key, out[k], single[b][key])
        for key, call in batch_ops(ctx, [2, 2], [os_[2], os_[2]]).items():
            with pytest.raises(SqpHipError, match="repeats"):
                call()
        out = ctx.norm_violations_batch([2], [os_[2].E], [os_[2].x], 1)
        assert _bits(out[0]) == _bits(single[2]["viol", 1])
    finally:
        ctx.close()


# ------------------------------------------------------------------ 4. Armijo beyond one stride
@pytest.mark.parametrize("name", MC.ARMIJO_NAMES)
def test_armijo_beyond_one_stride(name):
    """n, m > 1024 on a QCQP, a factorable-NLP and a polar ACOPF context of batch 2, probed in instance 1 (instance 0 holds
    other data): (alpha, is_valid, evaluations) is the triple of the reference loop over the Python evaluators, for inputs
    that leave at alpha = 1, backtrack, run below min_alpha, and return at once on a step below tol_direction."""
    pr = MC.armijo_problem(name)
    assert pr.n > MC.TPB and pr.m > MC.TPB
    ctx = pr.make_ctx()
    try:
        assert ctx.opts.tol_direction == MC.TOL_DIRECTION
        for mu, fr, step, phi0, D in pr.steps:
            alpha, valid, nev, margin = MR.compute_alpha(MC.armijo_phi(pr, mu, fr, step), phi0, D, float(np.abs(step).max()),
                                                         MC.TOL_DIRECTION, **pr.kw)
            got = ctx.acopf_armijo(1, pr.x, step, mu, phi0, D, pr.kw["eta"], pr.kw["tau"], pr.kw["min_alpha"], fr)
            print("armijo", name, (mu, fr), got, (alpha, valid, nev), "margin", margin)
            assert got == (alpha, valid, nev), (name, mu, fr)
    finally:
        ctx.close()


# ------------------------------------------------------------------ 5. no rows
def test_no_rows():
    c = MC.case("2500x0"); ctx = _ctx("2500x0")
    assert c.P.m == 0 and len(c.P.jrow) == 0
    for oset in (0, 1):
        o = c.ops[oset]; ref = _ref("2500x0", oset)
        got = {key: call() for key, call in scalar_ops(ctx, o).items()}
        MR.check_against(ref, got, f"no rows, set {oset}")
        for pn in PNORMS:
            assert got["compl", pn] == 0.0
        res = np.abs(o.df + o.mult_x_U - o.mult_x_L).max()
        sc = max(1.0, np.abs(o.df).max(), np.abs(o.mult_x_U).max(), np.abs(o.mult_x_L).max())
        # (the same two additions per entry in the same order, exact maxima, one division)
        assert abs(got["kt"] - res / sc) <= 2.0 * MR.U * (res / sc) and abs(ref["kt"].value - res / sc) <= ref["kt"].tol
        for rule in (1, 2, 3):
            assert got["mu", rule, 1].shape == (0,)
        assert got["D", True, 0] == got["D5"] and got["q", "nostep"] == o.mu * got["viol", 1]
