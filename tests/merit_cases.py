"""Structures and operands for the merit and line-search seat (`sqphip_norm_violations` .. `sqphip_compute_mu_rule_dev`,
their `*_batch` forms, `sqphip_acopf_armijo`), at the edges of the one-workgroup loops of csrc/sqp.hip / sqp_dev.hpp.

Every loop there is `for (i = threadIdx.x; i < n; i += TPB)` followed by `block_reduce`, with TPB = 1024 threads in waves
of 64 (csrc/dev_util.hpp; this module reads no constant of the library -- 64 and 1024 are the values its sizes were chosen
for).  The sizes sit around one wave, around one workgroup and beyond two strides; the structures add repeated COO
entries (`gather_csc` sums them), empty rows and columns, a completely dense Hessian (`hfull`, a branch of its own in
`qmodel_step`) and, in `long-row`, a staged field (Hval) of more than 32 x 256 x 2 = 16 384 doubles with odd n, m, nnzJ,
nnzH: `k_seat_stage` loops per field with a grid capped at 32 blocks of 256 threads moving 2 doubles each, so its threads
take a second trip only where ONE field is longer than that (the length of the whole row does not matter), and every other
instance sits on an 8-byte-aligned slot.

Merit ops need no attach: `Context(n, m, num_linear, jrow, jcol, hrow, hcol, xL, xU, gL, gU, batch=...)` is enough.  The
patterns are banded (a Jacobian row touches at most 4 columns near i n / m, the Hessian is its diagonal and a few
sub-diagonals), so the symbolic analysis at creation takes well under a second.

Bounds cycle through equality / range / lower only / upper only, in rows and in variables (infinite sides are +-np.inf;
no row is free on both sides: creation refuses that).  Operands put entries above the upper bound, below the lower,
strictly inside and EXACTLY ON a bound, every combination with the bound kinds within 16 consecutive indices; the largest
violation and the largest |lam_i| ||J_i|| (in both operand sets) sit at an index >= 1024 wherever the size has one, so a kernel that drops a
second trip or a wave's share of a reduction changes every result, the max-norms included.  Operand set 1 spreads the
magnitudes over 1e-6 .. 1e6: summation order matters there, and no missing term hides behind rounding.

The second half holds the inputs of the Armijo probe beyond one stride (n, m > 1024) on a QCQP, a factorable-NLP and a
polar ACOPF context; tests/test_merit_cases_cpu.py holds them to the conditions the GPU test relies on.

Pure numpy; the library, the oracle and the evaluators are imported only inside the Armijo builders."""
from __future__ import annotations

import dataclasses
import numpy as np

inf = np.inf
WAVE, TPB = 64, 1024                        # csrc/dev_util.hpp: the values the sizes below were chosen for
STAGE_PASS = 32 * 256 * 2                   # doubles of one field that one trip of k_seat_stage's grid moves (api.hip, SeatCall::grid)

SIZES = [(1, 1), (63, 65), (64, 64), (65, 63), (1023, 1025), (1024, 1024), (1025, 1023), (2049, 3), (3, 2049), (2500, 0)]
STRUCTURES = {                              # name: (n, m, options)
    "65x63-dups": (65, 63, dict(dups=True)), "1025x1023-dups": (1025, 1023, dict(dups=True)),
    "holes": (130, 70, dict(holes=True)), "hfull-65": (65, 33, dict(hfull=True)),
    "long-row": (2049, 2047, dict(row_width=4, hsub=tuple(range(1, 9)), odd=True)),     # nnzH = 18 405 > STAGE_PASS
}
SIZE_NAMES = [f"{n}x{m}" for n, m in SIZES]
ALL_NAMES = SIZE_NAMES + list(STRUCTURES)

# bound kinds (rows and variables), operand positions
K_EQ, K_RANGE, K_LOWER, K_UPPER = range(4)
P_ABOVE, P_BELOW, P_INSIDE, P_ON = range(4)


@dataclasses.dataclass
class Pattern:
    n: int
    m: int
    jrow: np.ndarray            # 1-based COO
    jcol: np.ndarray
    hrow: np.ndarray            # lower triangle
    hcol: np.ndarray
    empty_rows: np.ndarray      # rows without an entry
    empty_cols: np.ndarray      # variables in no row and in no Hessian entry
    num_linear: int = 0


def pattern(n, m, dups=False, holes=False, hfull=False, row_width=None, hsub=(1, 3), odd=False) -> Pattern:
    hole_col = np.zeros(n, dtype=bool); hole_row = np.zeros(m, dtype=bool)
    if holes:
        hole_col[4::9] = True; hole_row[3::7] = True
    jr, jc = [], []
    for i in range(m):
        if hole_row[i]: continue
        k = min(n, row_width if row_width else 2 + i % 3)
        lo = min(i * n // m, n - k)
        cols = [j for j in range(lo, lo + k) if not hole_col[j]]
        jr += [i] * len(cols); jc += cols
    if hfull:
        hr, hc = np.tril_indices(n)
    else:
        hr, hc = [np.arange(n)], [np.arange(n)]
        for s in hsub:
            if n > s: hr.append(np.arange(s, n)); hc.append(np.arange(n - s))
        hr, hc = np.concatenate(hr), np.concatenate(hc)
        keep = ~(hole_col[hr] | hole_col[hc]); hr, hc = hr[keep], hc[keep]
    jr, jc = np.asarray(jr, dtype=np.int64), np.asarray(jc, dtype=np.int64)
    hr, hc = np.asarray(hr, dtype=np.int64), np.asarray(hc, dtype=np.int64)
    if odd:                                                     # all four counts odd: drop one entry of a row that keeps others
        if len(jr) % 2 == 0: jr, jc = jr[1:], jc[1:]
        if len(hr) % 2 == 0: hr, hc = hr[:-1], hc[:-1]
    if dups:                                                    # every fifth / seventh entry twice, scattered through the lists
        rng = np.random.default_rng([31, n, m])
        jp, hp = rng.permutation(len(jr) + len(jr[::5])), rng.permutation(len(hr) + len(hr[::7]))
        jr, jc = np.concatenate([jr, jr[::5]])[jp], np.concatenate([jc, jc[::5]])[jp]
        hr, hc = np.concatenate([hr, hr[::7]])[hp], np.concatenate([hc, hc[::7]])[hp]
    return Pattern(n, m, jr + 1, jc + 1, hr + 1, hc + 1, np.nonzero(hole_row)[0], np.nonzero(hole_col)[0])


@dataclasses.dataclass
class Bounds:
    xL: np.ndarray
    xU: np.ndarray
    gL: np.ndarray
    gU: np.ndarray


def kinds(k):
    """range, lower, upper, equality, range, ...: index 1024 and index 2048 are no equalities"""
    return (np.arange(k) + 1) % 4


def _one_side(rng, k):
    """(lo, hi) of k entries cycling through the four bound kinds: equality, range, lower only, upper only"""
    mid, gap = rng.uniform(-1.0, 1.0, k), rng.uniform(0.5, 1.5, k)
    kd = kinds(k)
    lo = np.where(kd == K_UPPER, -inf, np.where(kd == K_EQ, mid, mid - gap))
    hi = np.where(kd == K_LOWER, inf, np.where(kd == K_EQ, mid, mid + gap))
    return lo, hi


def bounds(n, m, bseed=0) -> Bounds:
    """The kind of every row and variable follows from its index (`kinds`) whatever the seed (instances of one context share the kinds)."""
    rng = np.random.default_rng([37, n, m, bseed])
    xL, xU = _one_side(rng, n); gL, gU = _one_side(rng, m)
    return Bounds(xL, xU, gL, gU)


def positions(k):
    """Above / below / inside / on, turning once per four indices: with the kinds cycling per index, every (kind, position) couple
    within 16 consecutive indices."""
    i = np.arange(k)
    return (i // 4) % 4 if k >= 16 else (i + i // 4) % 4          # (fewer than 16 entries: as many couples as fit)


def _place(rng, lo, hi, pos, scale):
    """Values against [lo, hi] at the given positions.  Where a side is infinite the violation goes to the other side; an
    equality has no inside (the value is put on it).  Distances are scale * 10^u, u in [-1, 0] (scale 1) or [-6, 0]."""
    k = len(lo)
    dist = scale * 10.0 ** rng.uniform(-6.0 if scale > 1.0 else -1.0, 0.0, k)
    out = np.empty(k)
    for i in range(k):
        p, l, h = pos[i], lo[i], hi[i]
        if p == P_ABOVE: out[i] = h + dist[i] if np.isfinite(h) else l - dist[i]
        elif p == P_BELOW: out[i] = l - dist[i] if np.isfinite(l) else h + dist[i]
        elif p == P_ON or l == h: out[i] = h if (np.isfinite(h) and (i // 16) % 2 == 0) or not np.isfinite(l) else l     # (both sides in turn)
        elif np.isfinite(l) and np.isfinite(h): out[i] = l + (h - l) * rng.uniform(0.2, 0.8)
        else: out[i] = l + dist[i] if np.isfinite(l) else h - dist[i]
    return out


@dataclasses.dataclass
class Operands:
    E: np.ndarray
    x: np.ndarray
    df: np.ndarray
    p: np.ndarray
    lam: np.ndarray
    mult_x_U: np.ndarray
    mult_x_L: np.ndarray
    mu_vec: np.ndarray
    slack: np.ndarray
    Jval: np.ndarray
    Hval: np.ndarray
    f: float
    mu: float
    rho: float
    row_pos: np.ndarray
    var_pos: np.ndarray
    ibig: int                   # row of the largest violation and the largest |lam_i| ||J_i||, -1: m = 0
    jbig: int                   # variable of the largest variable violation and the largest |df_j|


def big_index(k):
    """The last index that is no equality: >= 1024 wherever k > 1024"""
    return -1 if k == 0 else (k - 1 if k % 4 != K_EQ or k == 1 else k - 2)


def operands(P: Pattern, B: Bounds, oset=0, oseed=0) -> Operands:
    n, m = P.n, P.m
    rng = np.random.default_rng([41, n, m, oset, oseed])
    S = 1.0 if oset == 0 else 1.0e6
    val = (lambda k: rng.standard_normal(k)) if oset == 0 else (lambda k: rng.choice([-1.0, 1.0], k) * 10.0 ** rng.uniform(-6.0, 6.0, k))
    rp, vp = positions(m), positions(n)
    ib, jb = big_index(m), big_index(n)
    if m: rp[ib] = P_ABOVE
    vp[jb] = P_ABOVE
    E, x = _place(rng, B.gL, B.gU, rp, S), _place(rng, B.xL, B.xU, vp, S)
    df, p, lam = val(n), val(n) * (0.05 if oset == 0 else 1.0), val(m)
    mxU, mxL = -np.abs(val(n)), np.abs(val(n))
    mu_vec, slack = np.abs(val(m)) * 10.0, np.abs(val(2 * m))
    jv, hv = val(len(P.jrow)), val(len(P.hrow))
    # the largest terms: 50 S on the row (20 S where only the variables reach beyond index 1024), 40 S on the variable,
    # |lam| = 100 S on the row, |df| = 30 S on the variable
    if m:
        big = (50.0 if m > TPB or n <= TPB else 20.0) * S
        E[ib] = B.gU[ib] + big if np.isfinite(B.gU[ib]) else B.gL[ib] - big
        lam[ib] = -100.0 * S
    x[jb] = B.xU[jb] + 40.0 * S if np.isfinite(B.xU[jb]) else B.xL[jb] - 40.0 * S
    df[jb] = 30.0 * S
    if m and oset == 1: jv[P.jrow - 1 == ib] = 1.0e6           # (set 1: other rows reach |lam_i| ||J_i|| of 1e12, this one 1e14)
    return Operands(E, x, df, p, lam, mxU, mxL, mu_vec, slack, jv, hv, 3.5 if oset == 0 else -2.5e3, 7.0 if oset == 0 else 4.0e2,
                    0.8, rp, vp, ib, jb)


@dataclasses.dataclass
class Case:
    name: str
    P: Pattern
    B: Bounds
    ops: tuple                  # the two operand sets

    def ctx_args(self, B: Bounds | None = None):
        P, B = self.P, B or self.B
        return (P.n, P.m, P.num_linear, P.jrow, P.jcol, P.hrow, P.hcol, B.xL, B.xU, B.gL, B.gU)

    def row_doubles(self):
        """The longest operand row of a batch call: x, p, df, E, Jval, Hval of compute_qmodel_batch"""
        return 3 * self.P.n + self.P.m + len(self.P.jrow) + len(self.P.hrow)

    def longest_field(self):
        """The longest single field a batch call stages: n, m, 2 m (the slacks), nnzJ or nnzH doubles"""
        return max(self.P.n, 2 * self.P.m, len(self.P.jrow), len(self.P.hrow))


_cache: dict = {}


def case(name) -> Case:
    """A committed case by name; generated once and shared: treat it as read-only."""
    if name not in _cache:
        if name in STRUCTURES: n, m, o = STRUCTURES[name]
        else: n, m = (int(v) for v in name.split("x")); o = {}
        P = pattern(n, m, **o); B = bounds(n, m)
        _cache[name] = Case(name, P, B, (operands(P, B, 0), operands(P, B, 1)))
    return _cache[name]


def hessian_is_dense(P: Pattern) -> bool:
    """The library's `hfull` rule (api.hip, sqphip_create): the mirrored pattern has n * n distinct entries, n > 1"""
    r, c = P.hrow, P.hcol
    keys = set((np.concatenate([r, c]) * (P.n + 1) + np.concatenate([c, r])).tolist())
    return P.n > 1 and len(keys) == P.n * P.n


# ------------------------------------------------------------------------------------------------ Armijo beyond one stride
ARMIJO_NAMES = ("qcqp", "nlp", "acopf")
ARMIJO_KW = dict(eta=0.4, tau=0.9, min_alpha=1e-6)            # the reference's defaults (parameters.jl)
ARMIJO_KW_NLP = dict(eta=0.4, tau=0.5, min_alpha=1e-3)        # the factorable NLP: fewer evaluations of its Python evaluator
TOL_DIRECTION = 1e-8                        # default_options().tol_direction
# (mu, feasibility restoration, step scale, claimed slope: None = the true slope of f along the step)
ARMIJO_INPUTS = ((0.0, False, 0.05, None),          # a short descent step of f: accepted at alpha = 1
                 (0.0, False, 40.0, None),          # a long one: backtracks
                 (5.0, False, 1.0, 1.0),            # a random step against a claimed slope of -(1 + |phi0|)
                 (1.0, True, 1.0, 1e6),             # no step length delivers this slope: alpha falls below min_alpha
                 (5.0, False, 1e-10, 1.0))          # ||p||_inf <= tol_direction: returns at once


@dataclasses.dataclass
class ArmijoProblem:
    name: str
    n: int
    m: int
    f: object                   # x -> f(x), g(x), grad f(x): the Python evaluators of instance 1
    g: object
    grad: object
    xL: np.ndarray
    xU: np.ndarray
    gL: np.ndarray
    gU: np.ndarray
    x: np.ndarray
    steps: list                 # per input: (mu, fr, step vector, phi0, D)
    make_ctx: object            # () -> a context of batch 2 whose instance 1 is this problem
    kw: dict = dataclasses.field(default_factory=lambda: dict(ARMIJO_KW))
    keep: object = None         # what the evaluators need alive (the oracle's problem)


def _steps(pr, box, seed):
    """The step of every input, kept inside `box` around x (the domain of every factor); D as tests/test_gpu_nlp.py forms it"""
    rng = np.random.default_rng(seed)
    out = []
    for mu, fr, scale, slope in ARMIJO_INPUTS:
        step = -scale * pr.grad(pr.x) if mu == 0.0 else scale * rng.standard_normal(pr.n)
        if box is not None: step = np.clip(step, box[0] - pr.x, box[1] - pr.x)
        out.append((mu, fr, step, slope))
    return out


def armijo_phi(pr, mu, fr, step):
    """alpha -> compute_phi (sqp.jl:170-183) over the Python evaluators, the 1-norm by the oracle"""
    from oracle import oracle as O

    def phi(a):
        xt = pr.x + a * step
        v = O.norm_violations(pr.g(xt), pr.gL, pr.gU, xt, pr.xL, pr.xU, 1)
        return v if fr else pr.f(xt) + mu * v
    return phi


def armijo_problem(name) -> ArmijoProblem:
    key = ("armijo", name)
    if key in _cache: return _cache[key]
    import sqpsolver_jl_amd as pkg
    if name == "qcqp":
        from sqpsolver_jl_amd.qcqp import qcqp_layout, qcqp_scenario, qcqp_synth
        from qcqp_ref import QcqpRef
        q0 = qcqp_synth(n=1100, m=1030); q = qcqp_scenario(q0, 1); lay = qcqp_layout(q0); R = QcqpRef(q)
        x = np.clip(q.x0 + 0.1 * np.random.default_rng(6).standard_normal(q.n), q.xL, q.xU)

        def make_ctx():
            ctx = pkg.Context(lay.n, lay.m, lay.num_linear, lay.jrow, lay.jcol, lay.hrow, lay.hcol, lay.xL, lay.xU, lay.gL, lay.gU, batch=2)
            ctx.qcqp_attach(q0); ctx.qcqp_set_instance(0, q0); ctx.qcqp_set_instance(1, q)
            return ctx
        pr = ArmijoProblem(name, q.n, q.m, R.f, R.g, R.grad, q.xL, q.xU, q.gL, q.gU, x, [], make_ctx); box = None
    elif name == "nlp":
        from sqpsolver_jl_amd.nlp_terms import nlp_general_synth, nlp_terms_layout, nlp_terms_scenario
        from nlp_general_ref import NlpGeneralRef
        p0 = nlp_general_synth(n=1100, m=1030); p = nlp_terms_scenario(p0, 1, 1, 0.05); lay = nlp_terms_layout(p0); R = NlpGeneralRef(p)
        x = np.clip(p.x0 + 0.1 * np.random.default_rng(6).standard_normal(p.n), 0.3, 2.8)

        def make_ctx():
            ctx = pkg.Context(lay.n, lay.m, lay.num_linear, lay.jrow, lay.jcol, lay.hrow, lay.hcol, lay.xL, lay.xU, lay.gL, lay.gU, batch=2)
            ctx.nlp_attach(p0, general=True); ctx.nlp_set_instance(0, p0); ctx.nlp_set_instance(1, p)
            return ctx
        pr = ArmijoProblem(name, p.n, p.m, R.f, R.g, R.grad, p.xL, p.xU, p.gL, p.gU, x, [], make_ctx, dict(ARMIJO_KW_NLP)); box = (0.25, 2.95)
    else:
        from sqpsolver_jl_amd.acopf_synth import acopf_layout, acopf_synth, contingency
        from oracle import oracle as O
        base = acopf_synth(300, 60, 450, 7); net = contingency(base, 1, 7)
        lay0, lay = acopf_layout(base), acopf_layout(net); Pb = O.problem_acopf(net, lay)
        x = np.clip(lay.x0 + 0.05 * np.random.default_rng(6).standard_normal(lay.n), lay.xL, lay.xU)

        def make_ctx():
            ctx = pkg.Context(lay0.n, lay0.m, lay0.num_linear, lay0.jrow, lay0.jcol, lay0.hrow, lay0.hcol, lay0.xL, lay0.xU, lay0.gL,
                              lay0.gU, batch=2)
            ctx.acopf_attach(base, lay0); ctx.acopf_set_instance(0, base, lay0); ctx.acopf_set_instance(1, net, lay)
            return ctx
        pr = ArmijoProblem(name, lay.n, lay.m, Pb.eval_f, Pb.eval_g, Pb.eval_grad_f, np.asarray(lay.xL, float), np.asarray(lay.xU, float),
                           np.asarray(lay.gL, float), np.asarray(lay.gU, float), x, [], make_ctx); box = None
        pr.keep = Pb
    steps = []
    for mu, fr, step, slope in _steps(pr, box, 8):
        phi0 = armijo_phi(pr, mu, fr, step)(0.0)
        D = float(pr.grad(pr.x) @ step) if slope is None else -slope * (1.0 + abs(phi0))
        steps.append((mu, fr, step, phi0, D))
    pr.steps = steps
    _cache[key] = pr
    return pr
