"""A sparse factorable NLP for the batched device run (sqphip_nlp_attach): sums of products of univariate functions,

    min  f0 + sum_{t: row(t) = 0} c_t prod_k phi_tk(x_{v_tk})
    s.t. gL_i <= g0_i + sum_{t: row(t) = i} c_t prod_k phi_tk(x_{v_tk}) <= gU_i   (i = 1..m),   xL <= x <= xU

Every factor is phi(x) = kappa(a x + b) with kappa one of POW (u^e, integer e, 1 <= |e| <= 32), SIN, COS, EXP, LOG.  A term
has 1 to 8 factors on distinct variables (x x is written x^2); rows 1..num_linear carry single plain factors (POW, e = 1,
a = 1, b = 0) only.  The structure (rows, variables, kinds, e, a, b) is shared by a batch; an instance has its own
f0, g0 and term coefficients.  Domain is the caller's business: LOG and negative powers need bounds that keep a x + b
positive.

A factor may also take an affine form of several variables (sqphip_nlp_attach_affine): kappa(sum_j a_j x_{v_j} + b), 1 to 8
arguments, the variables of a term distinct across all arguments of all its factors.  Such a problem carries the argument
arrays aptr / avar / acoef (None in the one-argument form above, where fvar / fscale say it all); in it fvar / fscale hold
the first argument of every factor.

A variable may also sit in several factors of one term and the menu may go beyond LOG (sqphip_nlp_attach_general): SQRT,
TANH, ATAN, SIGMOID 1 / (1 + e^-u), SOFTPLUS log(1 + e^u) and POWR u^p with a real exponent p (finite, not 0; fpar holds
it, and a float in the exponent's place of a POWR factor sets it).  x log x is [(i, POW), (i, LOG)], (x + y)(x - y) two
plain affine factors.  Twice inside one factor stays an error.  SQRT and POWR need a positive argument, as LOG does.

    NlpTerms             the data (terms, factors, values, bounds, start)
    make_nlp_terms       ... from a list of (row, coefficient, [(variable, kind, e, a, b), ...]); a factor may be
                         ([(variable, coefficient), ...], kind, e, b) instead
    nlp_terms_args       (aptr, avar, acoef) of a problem of either form
    nlp_terms_layout     the structures a Context is created with (1-based Jacobian COO, lower Hessian COO, bounds, start)
    nlp_terms_rows       g(x) in numpy
    nlp_terms_synth      a seeded test problem over the whole menu with a start that satisfies every row
    nlp_affine_synth     the same with affine arguments and least-squares residuals in the objective
    nlp_general_synth    the same with variables shared between the factors of a term and every kind up to POWR
    entropy_model, cobb_douglas_model, logistic_model     three small models with known answers
    needs_general        whether a problem is outside what sqphip_nlp_attach / _affine take (make_nlp_terms records it in
                         NlpTerms.general, and Context.nlp_attach goes by that record)
    nlp_terms_scenario   scenario s of a problem: the same structure, other coefficients, the same feasible start
    nlp_data_scenario    ... other shifts, argument coefficients and real exponents (sqphip_nlp_attach_data: the data of the
                         factors belongs to the instance), the same feasible start
    logistic_folds       the k training folds of a dataset as k logistic models of one structure
    NlpBlock             a dense data block of the objective, sum_i w_i kappa(A_i'x_cols + b_i) (sqphip_nlp_add_block): A, the
                         columns and the kind are shared by the batch, the weights and shifts belong to the instance
    NlpSoftmaxBlock      a multinomial (softmax) data block, sum_i w_i [log sum_k exp(u_ik) - u_{i, y_i}] with
                         u_ik = A_i'x_cols[k] + shift_ki (sqphip_nlp_add_softmax_block); it sits in NlpTerms.blocks beside NlpBlock
    NlpRowBlock          a dense data block with several outputs: one A, R <= 8 weight vectors with a target row each (row 0:
                         the objective), sum_i w_ri kappa(A_i'x_cols + b_i) added to row r (sqphip_nlp_add_row_block)
    NlpCoxBlock          a Cox partial-likelihood data block (survival data, Breslow ties), sum_i w_i event_i [log sum_{j < risk_i}
                         w_j exp(u_j) - u_i] over points sorted by non-increasing time (sqphip_nlp_add_cox_block)
    NlpLseBlock          a log-sum-exp row block: output r = log sum_{i in segment r} w_i exp(A_i'x_cols + b_i) added to row r, any
                         number of outputs over consecutive segments of the points (sqphip_nlp_add_lse_block)
    block_eval           value, gradient and dense Hessian of the blocks of a problem in numpy
    row_block_eval       ... of its blocks with several outputs: the rows' values and Jacobian rows too, the Hessian of the
                         Lagrangian with sigma and lam
    lse_block_eval       ... of its log-sum-exp row blocks, likewise
    NlpNormBlock         a Euclidean-norm row block: output r = sqrt(sum_{i in segment r} w_i (A_i'x_cols + b_i)^2) added to row r, any
                         number of outputs over consecutive segments of the points, any number of them on one row
                         (sqphip_nlp_add_norm_block)
    norm_block_eval      ... of its Euclidean-norm row blocks, likewise
    sum_of_norms_model, robust_lp_model, socp_synth, norm_scenario     Fermat-Weber location as norms on the objective; a robust
                         linear programme with second-order-cone rows; a seeded cone programme; its scenarios (other shifts)
    geometric_program_model, gp_synth, gp_scenario     a geometric programme in log variables as one log-sum-exp row block; a
                         seeded one; its scenarios (other log-coefficients)
    neyman_pearson_model, rate_constrained_logistic_model     constraints on the data the objective is fitted to, as row blocks
    multinomial_block_model  ridge-regularised K-class logistic regression as one softmax block plus terms
    cox_risk, cox_block_model  the risk sets of sorted times; ridge-regularised Cox regression as one Cox block plus terms
    logistic_block_model, poisson_block_model, least_squares_block_model     data fits of any size as one block plus terms
    fold_weights         the k training folds of N points as 0 / 1 weight vectors (logistic_fold_indices)
    from_qcqp            a Qcqp (qcqp.py) restated as terms
    from_polar_acopf     the polar ACOPF of acopf_layout restated as terms, on that layout's COO structures

Device evaluator: csrc/nlp_dev.hpp nlp_eval."""
from __future__ import annotations

import dataclasses

import numpy as np

POW, SIN, COS, EXP, LOG = 0, 1, 2, 3, 4
SQRT, TANH, ATAN, SIGMOID, SOFTPLUS, POWR = 5, 6, 7, 8, 9, 10
MAX_FACTORS = 8
MAX_ARGS = 8
MAX_BLOCKS = 4
MAX_BLOCK_COLS = 128
MAX_SOFTMAX_CLASSES = 64
MAX_BLOCK_ROWS = 8


@dataclasses.dataclass
class NlpBlock:
    """sum_{i < N} weight_i kappa(sum_j A[i, j] x_{cols[j]} + shift_i) in the objective: kind from the menu (exp for POW, par
    for POWR), cols d distinct 1-based variables in any order (d <= 128), A [N, d]; shift None: zeros, weight None: ones."""
    kind: int
    cols: np.ndarray
    A: np.ndarray
    shift: np.ndarray | None = None
    weight: np.ndarray | None = None
    exp: int = 1
    par: float = 0.0

    def __post_init__(self):
        self.cols = _i64(np.atleast_1d(self.cols))
        self.A = _f64(np.atleast_2d(self.A))
        N = self.A.shape[0]
        self.shift = np.zeros(N) if self.shift is None else _f64(self.shift)
        self.weight = np.ones(N) if self.weight is None else _f64(self.weight)


@dataclasses.dataclass
class NlpSoftmaxBlock:
    """sum_{i < N} weight_i [log sum_{k < K} exp(u_ik) - u_{i, labels_i}], u_ik = sum_j A[i, j] x_{cols[k, j]} + shift[k, i], in the
    objective: cols [Kf, d] distinct 1-based variables in any order (Kf d <= 128), A [N, d], labels [N] in 0..K-1, 2 <= K <= 64.
    pinned: the last class has no variables and u_{i, K-1} = 0, Kf = K - 1; else Kf = K.  shift [Kf, N] None: zeros, weight [N]
    None: ones."""
    cols: np.ndarray
    A: np.ndarray
    labels: np.ndarray
    K: int
    pinned: bool = True
    shift: np.ndarray | None = None
    weight: np.ndarray | None = None

    def __post_init__(self):
        self.A = _f64(np.atleast_2d(self.A))
        N, d = self.A.shape
        self.K, self.pinned = int(self.K), bool(self.pinned)
        if not 2 <= self.K <= MAX_SOFTMAX_CLASSES:
            raise ValueError(f"K = {self.K} classes (2..{MAX_SOFTMAX_CLASSES})")
        Kf = self.Kf
        if Kf * d > MAX_BLOCK_COLS:
            raise ValueError(f"Kf d = {Kf} x {d} columns (at most {MAX_BLOCK_COLS})")
        self.cols = _i64(self.cols)
        if self.cols.size != Kf * d:
            raise ValueError(f"cols holds {self.cols.size} variables, not Kf d = {Kf} x {d}")
        self.cols = self.cols.reshape(Kf, d)
        if len(np.unique(self.cols)) != Kf * d:
            raise ValueError("a variable sits in two columns of the block")
        self.labels = np.ascontiguousarray(self.labels, dtype=np.int32)
        if self.labels.shape != (N,) or (N and (self.labels.min() < 0 or self.labels.max() >= self.K)):
            raise ValueError(f"labels: {N} values in 0..{self.K - 1}")
        self.shift = np.zeros((Kf, N)) if self.shift is None else _f64(self.shift).reshape(Kf, N)
        self.weight = np.ones(N) if self.weight is None else _f64(self.weight)

    @property
    def Kf(self) -> int:
        return self.K - 1 if self.pinned else self.K


@dataclasses.dataclass
class NlpCoxBlock:
    """sum_{i < N} c_i [log sum_{j < risk_i} weight_j exp(u_j) - u_i], u_i = sum_j A[i, j] x_{cols[j]} + shift_i, c_i = weight_i event_i,
    in the objective: the Cox partial likelihood with Breslow ties.  The points are sorted by non-increasing time and the risk
    set of point i is the risk[i] leading points: i + 1 <= risk[i] <= N (i 0-based), non-decreasing, one value per tie group
    (cox_risk).  cols d distinct 1-based variables in any order (d <= 128), A [N, d], event [N] >= 0 (0: censored); shift None:
    zeros, weight None: ones (0 / 1 for folds, integers for resamples)."""
    cols: np.ndarray
    A: np.ndarray
    risk: np.ndarray
    event: np.ndarray
    shift: np.ndarray | None = None
    weight: np.ndarray | None = None

    def __post_init__(self):
        self.cols = _i64(np.atleast_1d(self.cols))
        self.A = _f64(np.atleast_2d(self.A))
        N, d = self.A.shape
        if not 1 <= d <= MAX_BLOCK_COLS:
            raise ValueError(f"d = {d} columns (1..{MAX_BLOCK_COLS})")
        if len(self.cols) != d or len(np.unique(self.cols)) != d:
            raise ValueError(f"cols: {d} distinct variables")
        self.risk = np.ascontiguousarray(np.atleast_1d(self.risk), dtype=np.int32)
        self.event = _f64(np.atleast_1d(self.event))
        if self.risk.shape != (N,) or self.event.shape != (N,):
            raise ValueError(f"risk and event: {N} values each")
        lo = np.arange(1, N + 1)
        if np.any(self.risk < lo) or np.any(self.risk > N):
            i = int(np.argmax((self.risk < lo) | (self.risk > N)))
            raise ValueError(f"point {i + 1}: risk {int(self.risk[i])} outside {i + 1}..{N}")
        if np.any(np.diff(self.risk) < 0):
            i = int(np.argmax(np.diff(self.risk) < 0)) + 1
            raise ValueError(f"point {i + 1}: risk {int(self.risk[i])} decreases from {int(self.risk[i - 1])}")
        if not np.all(np.isfinite(self.event)) or np.any(self.event < 0):
            i = int(np.argmax(~(np.isfinite(self.event) & (self.event >= 0))))
            raise ValueError(f"point {i + 1}: event {self.event[i]} (finite and not negative)")
        self.shift = np.zeros(N) if self.shift is None else _f64(self.shift)
        self.weight = np.ones(N) if self.weight is None else _f64(self.weight)
        if self.shift.shape != (N,) or self.weight.shape != (N,):
            raise ValueError(f"shift and weight: {N} values each")


@dataclasses.dataclass
class NlpLseBlock:
    """Output r adds log sum_{i in segment r} weight_i exp(u_i), u_i = sum_j A[i, j] x_{cols[j]} + shift_i, to row rows[r] (0: the
    objective, i: row i, a nonlinear one): the log-sum-exp of the consecutive points seg[r] .. seg[r + 1] - 1 (seg[0] = 0,
    seg[R] = N, every segment at least one point), R = len(rows) distinct target rows, 1 <= R <= N.  cols d distinct 1-based
    variables in any order (d <= 128), A [N, d]; shift [N] None: zeros (the log-coefficients of the monomials), weight [N] >= 0
    None: ones (0 removes a monomial)."""
    cols: np.ndarray
    A: np.ndarray
    rows: np.ndarray
    seg: np.ndarray
    shift: np.ndarray | None = None
    weight: np.ndarray | None = None

    def __post_init__(self):
        self.cols = _i64(np.atleast_1d(self.cols))
        self.A = _f64(np.atleast_2d(self.A))
        self.rows = _i64(np.atleast_1d(self.rows))
        self.seg = _i64(np.atleast_1d(self.seg))
        N, d = self.A.shape
        R = len(self.rows)
        if not 1 <= d <= MAX_BLOCK_COLS:
            raise ValueError(f"d = {d} columns (1..{MAX_BLOCK_COLS})")
        if N < 1:
            raise ValueError(f"N = {N} points (at least 1)")
        if len(self.cols) != d or len(np.unique(self.cols)) != d:
            raise ValueError(f"cols: {d} distinct variables")
        if not 1 <= R <= N:
            raise ValueError(f"R = {R} outputs (1..{N})")
        if self.seg.shape != (R + 1,):
            raise ValueError(f"seg: R + 1 = {R + 1} values")
        if self.seg[0] != 0:
            raise ValueError(f"output 1: seg[0] = {int(self.seg[0])} (the first segment starts at point 0)")
        if np.any(np.diff(self.seg) <= 0):
            r = int(np.argmax(np.diff(self.seg) <= 0))
            raise ValueError(f"output {r + 1}: the segment {int(self.seg[r])}..{int(self.seg[r + 1])} is "
                             + ("empty" if self.seg[r + 1] == self.seg[r] else "decreasing"))
        if self.seg[R] != N:
            raise ValueError(f"output {R}: seg[R] = {int(self.seg[R])} (the last segment ends at N = {N})")
        if len(np.unique(self.rows)) != R:
            raise ValueError("a row is the target of two outputs of the block")
        self.shift = np.zeros(N) if self.shift is None else _f64(self.shift)
        self.weight = np.ones(N) if self.weight is None else _f64(self.weight)
        if self.shift.shape != (N,) or self.weight.shape != (N,):
            raise ValueError(f"shift and weight: {N} values each")


@dataclasses.dataclass
class NlpNormBlock:
    """Output r adds sqrt(sum_{i in segment r} weight_i v_i^2), v_i = sum_j A[i, j] x_{cols[j]} + shift_i, to row rows[r] (0: the
    objective, i: row i, a nonlinear one): the Euclidean norm of the consecutive points seg[r] .. seg[r + 1] - 1 (seg[0] = 0,
    seg[R] = N, every segment at least one point), R = len(rows), 1 <= R <= N.  Rows may repeat: a sum of norms in the objective
    is several outputs on row 0.  cols d distinct 1-based variables in any order (d <= 128), A [N, d]; shift [N] None: zeros,
    weight [N] >= 0 None: ones (0 removes a point; a coefficient c > 0 on a norm is c^2 on its points).  An output whose value is
    0 contributes nothing to the derivatives (the apex); a point with a zero row of A and the shift delta smooths the norm."""
    cols: np.ndarray
    A: np.ndarray
    rows: np.ndarray
    seg: np.ndarray
    shift: np.ndarray | None = None
    weight: np.ndarray | None = None

    def __post_init__(self):
        self.cols = _i64(np.atleast_1d(self.cols))
        self.A = _f64(np.atleast_2d(self.A))
        self.rows = _i64(np.atleast_1d(self.rows))
        self.seg = _i64(np.atleast_1d(self.seg))
        N, d = self.A.shape
        R = len(self.rows)
        if not 1 <= d <= MAX_BLOCK_COLS:
            raise ValueError(f"d = {d} columns (1..{MAX_BLOCK_COLS})")
        if N < 1:
            raise ValueError(f"N = {N} points (at least 1)")
        if len(self.cols) != d or len(np.unique(self.cols)) != d:
            raise ValueError(f"cols: {d} distinct variables")
        if not 1 <= R <= N:
            raise ValueError(f"R = {R} outputs (1..{N})")
        if self.seg.shape != (R + 1,):
            raise ValueError(f"seg: R + 1 = {R + 1} values")
        if self.seg[0] != 0:
            raise ValueError(f"output 1: seg[0] = {int(self.seg[0])} (the first segment starts at point 0)")
        if np.any(np.diff(self.seg) <= 0):
            r = int(np.argmax(np.diff(self.seg) <= 0))
            raise ValueError(f"output {r + 1}: the segment {int(self.seg[r])}..{int(self.seg[r + 1])} is "
                             + ("empty" if self.seg[r + 1] == self.seg[r] else "decreasing"))
        if self.seg[R] != N:
            raise ValueError(f"output {R}: seg[R] = {int(self.seg[R])} (the last segment ends at N = {N})")
        self.shift = np.zeros(N) if self.shift is None else _f64(self.shift)
        self.weight = np.ones(N) if self.weight is None else _f64(self.weight)
        if self.shift.shape != (N,) or self.weight.shape != (N,):
            raise ValueError(f"shift and weight: {N} values each")


@dataclasses.dataclass
class NlpRowBlock:
    """Output r adds sum_{i < N} weight[r, i] kappa(sum_j A[i, j] x_{cols[j]} + shift_i) to row rows[r] (0: the objective, i: row
    i, a nonlinear one): one design matrix, R = len(rows) <= 8 distinct target rows.  kind, cols, A, exp, par as in NlpBlock;
    shift [N] None: zeros, weight [R, N] None: ones."""
    kind: int
    cols: np.ndarray
    A: np.ndarray
    rows: np.ndarray
    shift: np.ndarray | None = None
    weight: np.ndarray | None = None
    exp: int = 1
    par: float = 0.0

    def __post_init__(self):
        self.cols = _i64(np.atleast_1d(self.cols))
        self.A = _f64(np.atleast_2d(self.A))
        self.rows = _i64(np.atleast_1d(self.rows))
        N, R = self.A.shape[0], len(self.rows)
        if not 1 <= R <= MAX_BLOCK_ROWS:
            raise ValueError(f"R = {R} outputs (1..{MAX_BLOCK_ROWS})")
        if len(np.unique(self.rows)) != R:
            raise ValueError("a row is the target of two outputs of the block")
        self.shift = np.zeros(N) if self.shift is None else _f64(self.shift)
        self.weight = np.ones((R, N)) if self.weight is None else _f64(self.weight)
        if self.weight.size != R * N:
            raise ValueError(f"weight holds {self.weight.size} values, not R N = {R} x {N}")
        self.weight = self.weight.reshape(R, N)


@dataclasses.dataclass
class NlpTerms:
    n: int
    m: int
    num_linear: int
    trow: np.ndarray       # [nterms] 0: objective, i: row i (1-based)
    tcoef: np.ndarray      # [nterms]
    tptr: np.ndarray       # [nterms + 1] offsets into the factor arrays
    fvar: np.ndarray       # [nfac] variable (1-based)
    fkind: np.ndarray      # [nfac] POW .. LOG
    fexp: np.ndarray       # [nfac] exponent (POW only; 1 elsewhere)
    fscale: np.ndarray     # [nfac] a
    fshift: np.ndarray     # [nfac] b
    g0: np.ndarray         # [m]
    f0: float
    xL: np.ndarray
    xU: np.ndarray
    gL: np.ndarray
    gU: np.ndarray
    x0: np.ndarray
    aptr: np.ndarray | None = None     # [nfac + 1] offsets into the argument arrays; None: one argument per factor (fvar, fscale)
    avar: np.ndarray | None = None     # [nargs] variable (1-based)
    acoef: np.ndarray | None = None    # [nargs] coefficient
    fpar: np.ndarray | None = None     # [nfac] real exponent of a POWR factor (0 elsewhere); None: no POWR factor
    general: bool = False              # written for sqphip_nlp_attach_general (make_nlp_terms: needs_general); False: a model
                                       # of the older calls, which keep refusing what they refuse
    blocks: list = dataclasses.field(default_factory=list)     # NlpBlock, NlpSoftmaxBlock, NlpRowBlock, NlpCoxBlock, NlpLseBlock, NlpNormBlock: dense data blocks (at most 4)

    @property
    def affine(self) -> bool:
        return self.aptr is not None


def nlp_terms_args(p: NlpTerms):
    """(aptr, avar, acoef) of either form."""
    if p.aptr is not None:
        return p.aptr, p.avar, p.acoef
    return np.arange(len(p.fvar) + 1, dtype=np.int64), p.fvar, p.fscale


@dataclasses.dataclass
class NlpTermsLayout:
    """What SqpSolver.Model holds for this problem (1-based COO structures, bounds, start)."""
    n: int
    m: int
    num_linear: int
    jrow: np.ndarray
    jcol: np.ndarray
    hrow: np.ndarray
    hcol: np.ndarray
    xL: np.ndarray
    xU: np.ndarray
    gL: np.ndarray
    gU: np.ndarray
    x0: np.ndarray


def _i64(a):
    return np.ascontiguousarray(a, dtype=np.int64)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def make_nlp_terms(n, m, num_linear, terms, g0=None, f0=0.0, xL=None, xU=None, gL=None, gU=None, x0=None, blocks=None) -> NlpTerms:
    """terms: (row, coefficient, factors) with row 0 for the objective and factors (variable, kind[, e[, a[, b]]]), 1-based
    variables; a factor may be (args, kind[, e[, b]]) with args a list of (variable, coefficient) pairs, and one such factor
    makes the problem an affine one (aptr / avar / acoef set).  The e of a POWR factor is its real exponent (fpar set).
    Variables may repeat across the factors of a term.  Missing vectors are zeros, missing bounds infinite."""
    inf = np.inf
    full = lambda v, k, d: _f64(np.full(k, d) if v is None else v)
    trow, tcoef, tptr, fv, fk, fe, fa, fb, fp = [], [], [0], [], [], [], [], [], []
    aptr, avar, acoef, affine = [0], [], [], False
    for row, coef, factors in terms:
        trow.append(int(row)); tcoef.append(float(coef))
        for fac in factors:
            if isinstance(fac[0], (list, tuple)):
                affine = True
                args, kind, e, b = (tuple(fac) + (1, 0.0)[len(fac) - 2:])[:4]
                args = [(int(v), float(c)) for v, c in args]
            else:
                var, kind, e, a, b = (tuple(fac) + (1, 1.0, 0.0)[len(fac) - 2:])[:5]
                args = [(int(var), float(a))]
            fv.append(args[0][0] if args else 0); fa.append(args[0][1] if args else 1.0)
            real = int(kind) == POWR
            fk.append(int(kind)); fe.append(1 if real else int(e)); fp.append(float(e) if real else 0.0); fb.append(float(b))
            avar += [v for v, _ in args]; acoef += [c for _, c in args]; aptr.append(len(avar))
        tptr.append(len(fv))
    extra = (_i64(aptr), _i64(avar), _f64(acoef)) if affine else (None, None, None)
    extra += (_f64(fp) if POWR in fk else None,)
    p = NlpTerms(n, m, num_linear, _i64(trow), _f64(tcoef), _i64(tptr), _i64(fv), np.ascontiguousarray(fk, dtype=np.int32),
                 np.ascontiguousarray(fe, dtype=np.int32), _f64(fa), _f64(fb), full(g0, m, 0.0), float(f0),
                 full(xL, n, -inf), full(xU, n, inf), full(gL, m, -inf), full(gU, m, inf), full(x0, n, 0.0), *extra)
    p.general = needs_general(p)
    p.blocks = list(blocks or [])
    if len(p.blocks) > MAX_BLOCKS:
        raise ValueError(f"{len(p.blocks)} blocks (at most {MAX_BLOCKS})")
    for k, b in enumerate(p.blocks):
        if isinstance(b, (NlpSoftmaxBlock, NlpRowBlock, NlpCoxBlock, NlpLseBlock, NlpNormBlock)) and (b.cols.min() < 1 or b.cols.max() > n):
            raise ValueError(f"block {k + 1}: a column outside 1..{n}")
        if isinstance(b, (NlpRowBlock, NlpLseBlock, NlpNormBlock)):
            if b.rows.min() < 0 or b.rows.max() > m:
                raise ValueError(f"block {k + 1}: a row outside 0..{m}")
            if np.any((b.rows >= 1) & (b.rows <= num_linear)):
                raise ValueError(f"block {k + 1}: a row among the num_linear = {num_linear} linear rows")
    return p


def _term_of_factor(p: NlpTerms) -> np.ndarray:
    return np.repeat(np.arange(len(p.trow), dtype=np.int64), np.diff(p.tptr))


def nlp_terms_layout(p: NlpTerms) -> NlpTermsLayout:
    """Jacobian COO: (i, v) of every argument of every factor of a term of row i, row-major; Hessian COO: the lower entry
    (v, w) of every two distinct variables of one term -- except two arguments of one plain linear factor (POW, e = 1) --
    and (v, v) of every argument of a factor that is not plain linear, column-major; every pair of columns of a block,
    the diagonal included; (i, v) of every column v of a block with an output on row i >= 1.  Each once."""
    n = p.n
    aptr, avar, _ = nlp_terms_args(p)
    nargs = np.diff(aptr)
    fa = np.repeat(np.arange(len(p.fkind), dtype=np.int64), nargs)      # factor of an argument
    rows = p.trow[_term_of_factor(p)][fa]
    inrow = rows > 0
    jk = [(rows[inrow] - 1) * n + (avar[inrow] - 1)]
    for b in getattr(p, "blocks", []):
        if isinstance(b, (NlpRowBlock, NlpLseBlock, NlpNormBlock)):
            jk += [(i - 1) * n + (b.cols - 1) for i in b.rows.tolist() if i >= 1]
    jkey = np.unique(np.concatenate(jk))
    hk = []
    curved = ~((p.fkind == POW) & (p.fexp == 1))
    ca = curved[fa]
    hk.append((avar[ca] - 1) * n + (avar[ca] - 1))
    for t in range(len(p.trow)):
        j0, j1 = aptr[p.tptr[t]], aptr[p.tptr[t + 1]]
        v, f = avar[j0:j1], fa[j0:j1]
        if len(v) > 1:
            a, b = np.triu_indices(len(v), 1)
            keep = (f[a] != f[b]) | curved[f[a]]
            a, b = a[keep], b[keep]
            hk.append((np.minimum(v[a], v[b]) - 1) * n + np.maximum(v[a], v[b]) - 1)      # column-major key of the lower entry
    for b in getattr(p, "blocks", []):
        cols = np.ravel(b.cols)                       # (a softmax block: every pair of its Kf d columns)
        a, c = np.tril_indices(len(cols))
        hk.append((np.minimum(cols[a], cols[c]) - 1) * n + np.maximum(cols[a], cols[c]) - 1)
    hkey = np.unique(np.concatenate(hk)) if hk else np.zeros(0, np.int64)
    return NlpTermsLayout(n, p.m, p.num_linear, jkey // n + 1, jkey % n + 1, hkey % n + 1, hkey // n + 1,
                          p.xL.copy(), p.xU.copy(), p.gL.copy(), p.gU.copy(), p.x0.copy())


def factor_values(p: NlpTerms, x) -> np.ndarray:
    """phi of every factor at x."""
    if p.aptr is None:
        u = p.fscale * _f64(x)[p.fvar - 1] + p.fshift
    else:
        prod = p.acoef * _f64(x)[p.avar - 1]
        u = (np.add.reduceat(prod, p.aptr[:-1]) if len(prod) else np.zeros(0)) + p.fshift
    out = np.empty(len(u))
    with np.errstate(all="ignore"):
        for kind, fn in ((SIN, np.sin), (COS, np.cos), (EXP, np.exp), (LOG, np.log)):
            k = p.fkind == kind
            out[k] = fn(u[k])
        k = p.fkind == POW
        out[k] = u[k] ** p.fexp[k].astype(np.float64)
        for kind, fn in ((SQRT, np.sqrt), (TANH, np.tanh), (ATAN, np.arctan)):
            k = p.fkind == kind
            out[k] = fn(u[k])
        # the logistic pair without overflow: e = exp(-|u|) <= 1
        k = p.fkind == SIGMOID
        e = np.exp(-np.abs(u[k]))
        out[k] = np.where(u[k] < 0, e / (1.0 + e), 1.0 / (1.0 + e))
        k = p.fkind == SOFTPLUS
        out[k] = np.maximum(u[k], 0.0) + np.log1p(np.exp(-np.abs(u[k])))
        k = p.fkind == POWR
        if k.any():
            out[k] = u[k] ** p.fpar[k]
    return out


def needs_general(p: NlpTerms) -> bool:
    """A variable shared by two factors of a term, a kind above LOG or fpar set: sqphip_nlp_attach_general's class."""
    if getattr(p, "fpar", None) is not None or (len(p.fkind) and int(np.max(p.fkind)) > LOG):
        return True
    aptr, avar, _ = nlp_terms_args(p)
    term = _term_of_factor(p)[np.repeat(np.arange(len(p.fkind), dtype=np.int64), np.diff(aptr))]
    key = term * (p.n + 1) + avar
    return len(np.unique(key)) < len(key)


def _term_values(p: NlpTerms, x) -> np.ndarray:
    phi = factor_values(p, x)
    return p.tcoef * (np.multiply.reduceat(phi, p.tptr[:-1]) if len(phi) else np.zeros(0))


def nlp_terms_rows(p: NlpTerms, x) -> np.ndarray:
    """g(x) (used to place the bounds of generated problems)."""
    tv = _term_values(p, x)
    g = p.g0.copy()
    k = p.trow > 0
    np.add.at(g, p.trow[k] - 1, tv[k])
    return g


def nlp_terms_synth(n: int = 24, m: int = 14, seed: int = 1, terms_per_row: int = 3) -> NlpTerms:
    """Seeded problem over the whole menu: the objective sum w_j (x_j - a_j)^2 with a = x0 +- 0.3, two leading linear rows,
    then rows of terms_per_row terms with 1-4 factors on distinct variables, kinds uniform over the menu.  Bounds [0.2, 3]
    keep LOG and negative powers inside their domain; g0 and the row bounds are placed so that every row holds at the start
    x0 (uniform in [0.6, 1.4]): equalities at their value, one-sided and range rows with slack 0.2 - 1.  (A start that
    violates the linear rows sends the solver's feasibility phase to x = 0 and out of the domain.)"""
    rng = np.random.default_rng(seed)
    nlin = 2
    x0 = rng.uniform(0.6, 1.4, n)
    terms = []
    a = x0 + 0.3 * rng.choice([-1.0, 1.0], n)
    w = rng.uniform(0.5, 2.0, n)
    for j in range(n):
        terms.append((0, w[j], [(j + 1, POW, 2, 1.0, -a[j])]))
    kinds = []
    for i in range(1, m + 1):
        if i <= nlin:
            for j in rng.choice(n, terms_per_row, replace=False) + 1:
                terms.append((i, rng.uniform(-1, 1), [(int(j), POW, 1, 1.0, 0.0)]))
            kinds.append("eq" if i % 2 else "range")
            continue
        for _ in range(terms_per_row):
            facs = []
            for j in rng.choice(n, int(rng.integers(1, 5)), replace=False) + 1:
                kind = int(rng.integers(0, 5))
                e = int(rng.choice([-2, -1, 1, 2, 3])) if kind == POW else 1
                sc = float(rng.choice([1.0, -1.0, 0.5, 2.0])) if kind in (SIN, COS, EXP) else 1.0
                sh = float(rng.choice([0.0, 0.3])) if kind != POW else 0.0
                facs.append((int(j), kind, e, sc, sh))
            terms.append((i, rng.uniform(-1, 1), facs))
        kinds.append(("eq", "upper", "range")[(i - nlin - 1) % 3])
    p = make_nlp_terms(n, m, nlin, terms, g0=rng.uniform(-0.2, 0.2, m), f0=float(rng.standard_normal()),
                       xL=np.full(n, 0.2), xU=np.full(n, 3.0), x0=x0)
    g = nlp_terms_rows(p, x0)
    for i, kind in enumerate(kinds):
        s = rng.uniform(0.2, 1.0)
        if kind == "eq":
            p.gL[i] = p.gU[i] = g[i]
        elif kind == "upper":
            p.gL[i], p.gU[i] = -np.inf, g[i] + s
        else:
            p.gL[i], p.gU[i] = g[i] - s, g[i] + s
    return p


def nlp_affine_synth(n: int = 24, m: int = 14, seed: int = 1, terms_per_row: int = 3, max_args: int = 3) -> NlpTerms:
    """Seeded problem with affine arguments: the objective sum w_j (x_j - a_j)^2 with a = x0 +- 0.3 plus four least-squares
    residuals (sum_3 c_i x_i - r)^2 with r the value at x0 +- 0.3, two leading linear rows, then rows of terms_per_row terms
    of 1-3 factors, each with 1-max_args arguments, all variables of a term distinct, kinds uniform over the menu.  LOG and
    negative powers take positive coefficients (0.5, 1, 2) and shift 0 or 0.3, so their argument is positive on the whole
    box [0.2, 3]; the others take 1, -1, 0.5, 2, halved for EXP.  g0 and the row bounds are placed as nlp_terms_synth
    places them: every row holds at the start x0 (uniform in [0.6, 1.4])."""
    assert n >= 3 * max_args and 1 <= max_args <= MAX_ARGS
    rng = np.random.default_rng(seed)
    nlin = 2
    x0 = rng.uniform(0.6, 1.4, n)
    terms = []
    a = x0 + 0.3 * rng.choice([-1.0, 1.0], n)
    w = rng.uniform(0.5, 2.0, n)
    for j in range(n):
        terms.append((0, w[j], [(j + 1, POW, 2, 1.0, -a[j])]))
    for _ in range(4):
        js = rng.choice(n, 3, replace=False)
        c = rng.choice([1.0, -1.0, 0.5, 2.0], 3)
        r = float(c @ x0[js]) + 0.3 * float(rng.choice([-1.0, 1.0]))
        terms.append((0, 1.0, [([(int(j) + 1, float(cj)) for j, cj in zip(js, c)], POW, 2, -r)]))
    kinds = []
    for i in range(1, m + 1):
        if i <= nlin:
            for j in rng.choice(n, terms_per_row, replace=False) + 1:
                terms.append((i, rng.uniform(-1, 1), [(int(j), POW, 1, 1.0, 0.0)]))
            kinds.append("eq" if i % 2 else "range")
            continue
        for _ in range(terms_per_row):
            nargs = [int(rng.integers(1, max_args + 1)) for _ in range(int(rng.integers(1, 4)))]
            js = rng.choice(n, sum(nargs), replace=False) + 1
            facs, at = [], 0
            for na in nargs:
                kind = int(rng.integers(0, 5))
                e = int(rng.choice([-2, -1, 1, 2, 3])) if kind == POW else 1
                positive = kind == LOG or (kind == POW and e < 0)
                c = rng.choice([0.5, 1.0, 2.0] if positive else [1.0, -1.0, 0.5, 2.0], na)
                if kind == EXP:
                    c = 0.5 * c
                sh = float(rng.choice([0.0, 0.3]))
                facs.append(([(int(j), float(cj)) for j, cj in zip(js[at:at + na], c)], kind, e, sh))
                at += na
            terms.append((i, rng.uniform(-1, 1), facs))
        kinds.append(("eq", "upper", "range")[(i - nlin - 1) % 3])
    p = make_nlp_terms(n, m, nlin, terms, g0=rng.uniform(-0.2, 0.2, m), f0=float(rng.standard_normal()),
                       xL=np.full(n, 0.2), xU=np.full(n, 3.0), x0=x0)
    g = nlp_terms_rows(p, x0)
    for i, kind in enumerate(kinds):
        s = rng.uniform(0.2, 1.0)
        if kind == "eq":
            p.gL[i] = p.gU[i] = g[i]
        elif kind == "upper":
            p.gL[i], p.gU[i] = -np.inf, g[i] + s
        else:
            p.gL[i], p.gU[i] = g[i] - s, g[i] + s
    return p


_POSITIVE = (LOG, SQRT, POWR)


def nlp_general_synth(n: int = 24, m: int = 14, seed: int = 1, terms_per_row: int = 3, max_args: int = 3) -> NlpTerms:
    """Seeded problem of sqphip_nlp_attach_general's class: the objective sum w_j (x_j - a_j)^2 with a = x0 +- 0.3, four
    entropy terms x log x (two factors on one variable), four softplus residuals of three variables and two products
    (x_i + x_j)(x_i - x_j) of plain affine factors; two leading linear rows; then rows of terms_per_row terms of 1-3 factors,
    each with 1-max_args arguments drawn from a pool smaller than the argument count, so that factors of a term share
    variables (never twice inside a factor); the kinds cycle through the new ones first and are uniform over all eleven
    after.  LOG, SQRT, POWR and negative integer powers take positive coefficients (0.5, 1, 2) and shift 0 or 0.3, so their
    argument stays above 0.1 on the whole box [0.2, 3]; the others take 1, -1, 0.5, 2, halved for EXP.  Real exponents come
    from 0.5, 1.5, -0.7, 1.852.  g0 and the row bounds are placed as nlp_terms_synth places them: every row holds at x0."""
    assert n >= 3 * max_args and 1 <= max_args <= MAX_ARGS
    rng = np.random.default_rng(seed)
    nlin = 2
    x0 = rng.uniform(0.6, 1.4, n)
    terms = []
    a = x0 + 0.3 * rng.choice([-1.0, 1.0], n)
    w = rng.uniform(0.5, 2.0, n)
    for j in range(n):
        terms.append((0, w[j], [(j + 1, POW, 2, 1.0, -a[j])]))
    for j in rng.choice(n, 4, replace=False) + 1:
        terms.append((0, 0.5, [(int(j), POW), (int(j), LOG)]))
    for _ in range(4):
        js = rng.choice(n, 3, replace=False)
        c = rng.choice([1.0, -1.0, 0.5, 2.0], 3)
        terms.append((0, 1.0, [([(int(j) + 1, float(cj)) for j, cj in zip(js, c)], SOFTPLUS, 1, -float(c @ x0[js]))]))
    for _ in range(2):
        i, j = (int(v) + 1 for v in rng.choice(n, 2, replace=False))
        terms.append((0, 0.1, [([(i, 1.0), (j, 1.0)], POW, 1, 0.0), ([(i, 1.0), (j, -1.0)], POW, 1, 0.0)]))
    kinds, made = [], 0
    for i in range(1, m + 1):
        if i <= nlin:
            for j in rng.choice(n, terms_per_row, replace=False) + 1:
                terms.append((i, rng.uniform(-1, 1), [(int(j), POW, 1, 1.0, 0.0)]))
            kinds.append("eq" if i % 2 else "range")
            continue
        for _ in range(terms_per_row):
            nargs = [int(rng.integers(1, max_args + 1)) for _ in range(int(rng.integers(1, 4)))]
            pool = rng.choice(n, max(max(nargs), sum(nargs) - int(rng.integers(0, 3))), replace=False) + 1
            facs = []
            for na in nargs:
                kind = SQRT + made % 6 if made < 12 else int(rng.integers(0, POWR + 1))
                made += 1
                e = int(rng.choice([-2, -1, 1, 2, 3])) if kind == POW else 1
                if kind == POWR:
                    e = float(rng.choice([0.5, 1.5, -0.7, 1.852]))
                positive = kind in _POSITIVE or (kind == POW and e < 0)
                c = rng.choice([0.5, 1.0, 2.0] if positive else [1.0, -1.0, 0.5, 2.0], na)
                if kind == EXP:
                    c = 0.5 * c
                sh = float(rng.choice([0.0, 0.3]))
                facs.append(([(int(j), float(cj)) for j, cj in zip(rng.choice(pool, na, replace=False), c)], kind, e, sh))
            terms.append((i, rng.uniform(-1, 1), facs))
        kinds.append(("eq", "upper", "range")[(i - nlin - 1) % 3])
    p = make_nlp_terms(n, m, nlin, terms, g0=rng.uniform(-0.2, 0.2, m), f0=float(rng.standard_normal()),
                       xL=np.full(n, 0.2), xU=np.full(n, 3.0), x0=x0)
    g = nlp_terms_rows(p, x0)
    for i, kind in enumerate(kinds):
        s = rng.uniform(0.2, 1.0)
        if kind == "eq":
            p.gL[i] = p.gU[i] = g[i]
        elif kind == "upper":
            p.gL[i], p.gU[i] = -np.inf, g[i] + s
        else:
            p.gL[i], p.gU[i] = g[i] - s, g[i] + s
    return p


def entropy_model(c) -> NlpTerms:
    """min sum_i x_i log x_i + c'x  s.t.  sum_i x_i = 1 (a linear row), 1e-6 <= x <= 1, from the uniform point.  Optimum
    x_i = exp(-c_i) / sum_j exp(-c_j).  x log x is two factors on one variable."""
    c = _f64(c)
    n = len(c)
    terms = [(0, 1.0, [(j + 1, POW), (j + 1, LOG)]) for j in range(n)] + [(0, c[j], [(j + 1, POW)]) for j in range(n)]
    terms += [(1, 1.0, [(j + 1, POW)]) for j in range(n)]
    return make_nlp_terms(n, 1, 1, terms, xL=np.full(n, 1e-6), xU=np.ones(n), gL=[1.0], gU=[1.0], x0=np.full(n, 1.0 / n))


def cobb_douglas_model(alpha, prices, wealth) -> NlpTerms:
    """min -prod_i x_i^alpha_i  s.t.  prices'x <= wealth (a linear row), x >= 1e-3, from an equal split of half the wealth.
    With sum alpha <= 1 the utility is concave; optimum x_i = alpha_i wealth / (prices_i sum alpha).
    The structure depends on len(alpha) only -- alpha sits in fpar, the prices in tcoef, the wealth in gU --, so consumers
    with different elasticities are instances of one context of Context.nlp_attach(p, instance_data=True)."""
    alpha, prices = _f64(alpha), _f64(prices)
    n = len(alpha)
    terms = [(0, -1.0, [(j + 1, POWR, float(alpha[j])) for j in range(n)])]
    terms += [(1, prices[j], [(j + 1, POW)]) for j in range(n)]
    return make_nlp_terms(n, 1, 1, terms, xL=np.full(n, 1e-3), xU=np.full(n, wealth / prices.min()), gL=[-np.inf], gU=[float(wealth)],
                          x0=0.5 * wealth / (n * prices))


def logistic_model(X, y, reg) -> NlpTerms:
    """Ridge-regularised logistic regression, labels y in {0, 1}: min sum_i [softplus(X_i'w) - y_i X_i'w] + reg / 2 |w|^2
    over -50 <= w <= 50, no rows, from w = 0.  One SOFTPLUS factor of an affine form per point."""
    X, y = np.atleast_2d(_f64(X)), _f64(y)
    N, n = X.shape
    terms = [(0, 1.0, [([(j + 1, X[i, j]) for j in range(n)], SOFTPLUS, 1, 0.0)]) for i in range(N)]
    terms += [(0, -float(y @ X[:, j]), [(j + 1, POW)]) for j in range(n)]
    terms += [(0, 0.5 * float(reg), [(j + 1, POW, 2)]) for j in range(n)]
    return make_nlp_terms(n, 0, 0, terms, xL=np.full(n, -50.0), xU=np.full(n, 50.0), x0=np.zeros(n))


def _kappa3(kind, e, par, u):
    """kappa, kappa', kappa'' of one menu entry at the array u."""
    u = _f64(u)
    with np.errstate(all="ignore"):
        if kind == POW:
            e = int(e)
            return u ** e, e * u ** (e - 1), (e * (e - 1)) * u ** (e - 2) if e != 1 else np.zeros_like(u)
        if kind == POWR:
            return u ** par, par * u ** (par - 1.0), par * (par - 1.0) * u ** (par - 2.0)
        if kind == SIN:
            return np.sin(u), np.cos(u), -np.sin(u)
        if kind == COS:
            return np.cos(u), -np.sin(u), -np.cos(u)
        if kind == EXP:
            return np.exp(u), np.exp(u), np.exp(u)
        if kind == LOG:
            return np.log(u), 1.0 / u, -1.0 / (u * u)
        if kind == SQRT:
            r = np.sqrt(u)
            return r, 0.5 / r, -0.25 / (u * r)
        if kind == TANH:
            # sech^2 u = 4 e / (1 + e)^2, e = exp(-2 |u|): the device's form (1 - t t cancels, and is 0 from |u| = 19.07 on)
            t, e2 = np.tanh(u), np.exp(-2.0 * np.abs(u))
            d = 4.0 * e2 / ((1.0 + e2) * (1.0 + e2))
            return t, d, -2.0 * t * d
        if kind == ATAN:
            q = 1.0 / (1.0 + u * u)
            return np.arctan(u), q, -2.0 * (u * q) * q                 # (q q underflows from |u| = 1e77 on)
        e_ = np.exp(-np.abs(u))
        sg, sc = np.where(u < 0, e_ / (1.0 + e_), 1.0 / (1.0 + e_)), np.where(u < 0, 1.0 / (1.0 + e_), e_ / (1.0 + e_))
        if kind == SIGMOID:
            dm = np.expm1(-np.abs(u)) / (1.0 + e_)                          # (1 - s) - s = -+(1 - e) den without cancellation at 0
            return sg, sg * sc, sg * sc * np.where(u < 0, -dm, dm)
        if kind == SOFTPLUS:
            return np.maximum(u, 0.0) + np.log1p(e_), sg, sg * sc
    raise ValueError(f"unknown kind {kind}")


def _softmax_eval(b: NlpSoftmaxBlock, x):
    """(f, grad [Kf d], H [Kf d, Kf d]) of a softmax block over the flat index k d + j.  The logits are shifted by their
    maximum (the pinned class enters with 0), so any finite logits give finite results; the Hessian is formed as
    A'diag(w p_k) A on the class diagonal minus A'diag(w p_k p_l) A everywhere, as the device forms it."""
    Kf, d = b.cols.shape
    N = b.A.shape[0]
    u = np.stack([b.A @ x[b.cols[k] - 1] + b.shift[k] for k in range(Kf)])          # [Kf, N]
    if b.pinned:
        u = np.vstack([u, np.zeros(N)])
    m = u.max(axis=0)
    e = np.exp(u - m)
    s = e.sum(axis=0)
    P = (e / s)[:Kf]
    f = float(b.weight @ ((m + np.log(s)) - u[b.labels, np.arange(N)]))
    Y = (b.labels[None, :] == np.arange(Kf)[:, None]).astype(float)
    g = ((b.weight * (P - Y)) @ b.A).ravel()
    H = np.zeros((Kf * d, Kf * d))
    for k in range(Kf):
        wp = b.weight * P[k]
        for l in range(Kf):
            H[k * d:(k + 1) * d, l * d:(l + 1) * d] = -(b.A.T @ ((wp * P[l])[:, None] * b.A))
        H[k * d:(k + 1) * d, k * d:(k + 1) * d] += b.A.T @ (wp[:, None] * b.A)
    return f, g, H


def _cox_eval(b: NlpCoxBlock, x):
    """(f, grad [d], H [d, d]) of a Cox block in the block's own column order.  The logits are shifted by their maximum; T and Q
    are running sums from the front and from the back, as on the device; the Hessian is formed as A'diag(e Q) A minus
    M'diag(c) M with M_i = P[risk_i - 1] / T_i, P the running sums of e_j A_j: two separate sums, as the device forms it.  A
    point with c_i = 0 contributes exactly 0 and its logarithm is never formed."""
    N, d = b.A.shape
    u = b.A @ x[b.cols - 1] + b.shift
    m = u.max()
    e = b.weight * np.exp(u - m)
    c = b.weight * b.event
    on = c != 0.0
    T = np.cumsum(e)[b.risk - 1]
    with np.errstate(all="ignore"):
        lt = np.where(on, np.log(np.where(on, T, 1.0)), 0.0)
        q = np.where(on, c / np.where(on, T, 1.0), 0.0)
    f = float(np.sum(np.where(on, c * ((m + lt) - u), 0.0)))
    first = np.searchsorted(b.risk, np.arange(N), side="right")       # the first i with risk_i > j
    G = e * np.cumsum(q[::-1])[::-1][first]
    g = b.A.T @ (G - c)
    with np.errstate(all="ignore"):
        M = np.where(on[:, None], np.cumsum(e[:, None] * b.A, axis=0)[b.risk - 1] / np.where(on, T, 1.0)[:, None], 0.0)
    H = b.A.T @ (G[:, None] * b.A) - M.T @ (c[:, None] * M)
    return f, g, H


def block_eval(p: NlpTerms, x, blocks=None):
    """(f, grad [n], H [n, n]) of the blocks of p at x: sum_i w_i kappa(u_i), A'(w kappa'), A' diag(w kappa'') A scattered to
    the blocks' columns.  Blocks with several outputs (NlpRowBlock) are row_block_eval's and log-sum-exp row blocks (NlpLseBlock)
    lse_block_eval's, Euclidean-norm row blocks (NlpNormBlock) norm_block_eval's, not counted here."""
    x = _f64(x)
    f, g, H = 0.0, np.zeros(p.n), np.zeros((p.n, p.n))
    for b in (p.blocks if blocks is None else blocks):
        if isinstance(b, (NlpRowBlock, NlpLseBlock, NlpNormBlock)):
            continue
        if isinstance(b, NlpSoftmaxBlock):
            fb, gb, Hb = _softmax_eval(b, x)
            c = b.cols.ravel() - 1
            f += fb
            np.add.at(g, c, gb)
            H[np.ix_(c, c)] += Hb
            continue
        if isinstance(b, NlpCoxBlock):
            fb, gb, Hb = _cox_eval(b, x)
            c = b.cols - 1
            f += fb
            np.add.at(g, c, gb)
            H[np.ix_(c, c)] += Hb
            continue
        c = b.cols - 1
        k0, k1, k2 = _kappa3(b.kind, b.exp, b.par, b.A @ x[c] + b.shift)
        f += float(b.weight @ k0)
        np.add.at(g, c, b.A.T @ (b.weight * k1))
        H[np.ix_(c, c)] += b.A.T @ ((b.weight * k2)[:, None] * b.A)
    return f, g, H


def row_block_eval(p: NlpTerms, x, sigma=1.0, lam=None, blocks=None):
    """(f, grad [n], g [m], J [m, n], H [n, n]) of the blocks with several outputs of p at x: what they add to the objective,
    its gradient, the rows' values and Jacobian rows, and to the Hessian of the Lagrangian,
    A' diag(kappa'' (sum_r mu_r w_r)) A with mu_r = sigma for row 0 and lam[i - 1] for row i (lam None: zeros)."""
    x = _f64(x)
    lam = np.zeros(p.m) if lam is None else _f64(lam)
    f, g, gv, J, H = 0.0, np.zeros(p.n), np.zeros(p.m), np.zeros((p.m, p.n)), np.zeros((p.n, p.n))
    for b in (p.blocks if blocks is None else blocks):
        if not isinstance(b, NlpRowBlock):
            continue
        c = b.cols - 1
        k0, k1, k2 = _kappa3(b.kind, b.exp, b.par, b.A @ x[c] + b.shift)
        e = np.zeros(len(k0))
        for r, i in enumerate(b.rows.tolist()):
            if i == 0:
                f += float(b.weight[r] @ k0)
                np.add.at(g, c, b.A.T @ (b.weight[r] * k1))
            else:
                gv[i - 1] += float(b.weight[r] @ k0)
                np.add.at(J[i - 1], c, b.A.T @ (b.weight[r] * k1))
            e += (float(sigma) if i == 0 else lam[i - 1]) * b.weight[r]
        H[np.ix_(c, c)] += b.A.T @ ((e * k2)[:, None] * b.A)
    return f, g, gv, J, H


def lse_block_eval(p: NlpTerms, x, sigma=1.0, lam=None, blocks=None):
    """(f, grad [n], g [m], J [m, n], H [n, n]) of the log-sum-exp row blocks of p at x: what they add to the objective, its
    gradient, the rows' values and Jacobian rows, and to the Hessian of the Lagrangian, sum_r mu_r (A_r' diag(p) A_r - G_r G_r')
    with mu_r = sigma for row 0 and lam[i - 1] for row i (lam None: zeros).  The logits of a segment are shifted by the largest
    among its points of non-zero weight; a zero-weight point contributes exactly 0 and its exponential is never formed."""
    x = _f64(x)
    lam = np.zeros(p.m) if lam is None else _f64(lam)
    f, g, gv, J, H = 0.0, np.zeros(p.n), np.zeros(p.m), np.zeros((p.m, p.n)), np.zeros((p.n, p.n))
    for b in (p.blocks if blocks is None else blocks):
        if not isinstance(b, NlpLseBlock):
            continue
        c = b.cols - 1
        u = b.A @ x[c] + b.shift
        for r, i in enumerate(b.rows.tolist()):
            s0, s1 = int(b.seg[r]), int(b.seg[r + 1])
            on = b.weight[s0:s1] != 0.0
            Ar, ur, wr = b.A[s0:s1][on], u[s0:s1][on], b.weight[s0:s1][on]
            with np.errstate(all="ignore"):
                mr = ur.max() if len(ur) else -np.inf
                e = wr * np.exp(ur - mr)
                T = e.sum()
                pr = e / T
                val = float(mr + np.log(T))
            Gr = Ar.T @ pr
            mu = float(sigma) if i == 0 else lam[i - 1]
            if i == 0:
                f += val
                np.add.at(g, c, Gr)
            else:
                gv[i - 1] += val
                np.add.at(J[i - 1], c, Gr)
            H[np.ix_(c, c)] += mu * (Ar.T @ (pr[:, None] * Ar) - np.outer(Gr, Gr))
    return f, g, gv, J, H


def geometric_program_model(n, posynomials, monomial_rows=None, bounds=(-np.inf, np.inf), ridge=0.0, x0=None) -> NlpTerms:
    """A geometric programme in the log variables x = log y:
        min  log P_0(e^x) + ridge sum_j x_j^2   s.t.  log P_k(e^x) <= 0 (k >= 1),   a_l'x + log c_l = 0,   lo <= x <= hi.
    posynomials: [(coefs [k] > 0, exponents [k, n])], number 0 the objective, every other one a row log-sum-exp <= 0.  All
    of them are one NlpLseBlock on the variables in use: its points are the monomials, its shifts the log-coefficients, so the
    scenarios of one programme differ in the shifts only (gp_scenario).  monomial_rows: [(coef > 0, exponents [n])], the monomial
    equalities c prod y^a = 1, which are linear in x: they go to the num_linear leading rows of the terms.  bounds (lo, hi):
    scalars or [n].  From x0 (None: zeros)."""
    n = int(n)
    mono = list(monomial_rows or [])
    nl, K = len(mono), len(posynomials)
    if K < 1:
        raise ValueError("geometric_program_model: the objective posynomial is missing")
    A, S, seg = [], [], [0]
    for k, (c, E) in enumerate(posynomials):
        c, E = _f64(np.atleast_1d(c)), _f64(np.atleast_2d(E))
        if E.shape != (len(c), n) or len(c) < 1:
            raise ValueError(f"posynomial {k}: coefficients [k] and exponents [k, {n}]")
        if not np.all(c > 0) or not np.all(np.isfinite(c)):
            raise ValueError(f"posynomial {k}: a coefficient is not positive and finite")
        A.append(E); S.append(np.log(c)); seg.append(seg[-1] + len(c))
    A, S = np.vstack(A), np.concatenate(S)
    used = np.flatnonzero(np.any(A != 0.0, axis=0))
    if len(used) == 0:
        used = np.arange(1)
    rows = [0] + [nl + k for k in range(1, K)]
    blk = NlpLseBlock(used + 1, A[:, used], rows, seg, S)
    m = nl + K - 1
    terms, g0 = [], np.zeros(m)
    for l, (c, a) in enumerate(mono):
        a = _f64(np.atleast_1d(a))
        if a.shape != (n,) or not float(c) > 0:
            raise ValueError(f"monomial row {l + 1}: a positive coefficient and exponents [{n}]")
        terms += [(l + 1, float(a[j]), [(j + 1, POW)]) for j in np.flatnonzero(a)]
        g0[l] = np.log(float(c))
    if ridge:
        terms += [(0, float(ridge), [(j + 1, POW, 2)]) for j in range(n)]
    lo, hi = bounds
    gL = np.concatenate([np.zeros(nl), np.full(K - 1, -np.inf)])
    return make_nlp_terms(n, m, nl, terms, g0=g0, xL=np.broadcast_to(_f64(lo), (n,)).copy(), xU=np.broadcast_to(_f64(hi), (n,)).copy(),
                          gL=gL, gU=np.zeros(m), x0=np.zeros(n) if x0 is None else x0, blocks=[blk])


def gp_synth(n: int, lens, seed: int = 1) -> NlpTerms:
    """A seeded geometric programme on n log variables: lens[0] monomials in the objective, lens[k] in constraint k.  The
    exponents lie on the half-integer grid round(2 U(-2, 2)) / 2 with about 40 % non-zeros (a monomial left empty gets one);
    the coefficients are exp(0.5 N(0, 1)), normalised so that every constraint posynomial is 0.5 at x = 0 (x = 0 is strictly
    feasible) and the objective 1.  A ridge 1e-3 x_j^2 on every variable stays in the terms; -3 <= x <= 3, from x = 0."""
    rng = np.random.default_rng(int(seed))
    n = int(n)
    pos = []
    for k, K in enumerate(lens):
        E = np.round(2.0 * rng.uniform(-2.0, 2.0, (int(K), n))) / 2.0
        E *= rng.random((int(K), n)) < 0.4
        for i in np.flatnonzero(~np.any(E != 0.0, axis=1)):
            E[i, rng.integers(n)] = 1.0 if rng.random() < 0.5 else -1.0
        c = np.exp(0.5 * rng.standard_normal(int(K)))
        pos.append((c * ((1.0 if k == 0 else 0.5) / c.sum()), E))
    return geometric_program_model(n, pos, bounds=(-3.0, 3.0), ridge=1e-3)


def gp_scenario(p: NlpTerms, s: int, seed: int = 1, noise: float = 0.05) -> NlpTerms:
    """Scenario s of a geometric programme (s = 0 or noise = 0: p itself): every log-coefficient of its log-sum-exp row blocks
    moved by noise N(0, 1) -- prices, loads, process corners.  Structure, bounds and start stay."""
    if s == 0 or noise == 0:
        return p
    rng = np.random.default_rng(int(seed) * 1000 + int(s))
    out = dataclasses.replace(p)
    out.blocks = [dataclasses.replace(b, shift=b.shift + noise * rng.standard_normal(len(b.shift))) if isinstance(b, NlpLseBlock) else b
                  for b in p.blocks]
    return out


def norm_block_eval(p: NlpTerms, x, sigma=1.0, lam=None, blocks=None):
    """(f, grad [n], g [m], J [m, n], H [n, n]) of the Euclidean-norm row blocks of p at x: what they add to the objective, its
    gradient, the rows' values and Jacobian rows, and to the Hessian of the Lagrangian, sum_r mu_r (A_r' diag(w / f_r) A_r -
    G_r G_r' / f_r) with mu_r = sigma for row 0 and lam[i - 1] for row i (lam None: zeros).  The residuals of a segment are scaled
    by the largest magnitude among its points of non-zero weight; a zero-weight point is masked out (its residual may be
    anything); an output whose value is 0 (no weighted point, or all weighted residuals exactly zero) contributes the value 0
    and nothing to the derivatives."""
    x = _f64(x)
    lam = np.zeros(p.m) if lam is None else _f64(lam)
    f, g, gv, J, H = 0.0, np.zeros(p.n), np.zeros(p.m), np.zeros((p.m, p.n)), np.zeros((p.n, p.n))
    for b in (p.blocks if blocks is None else blocks):
        if not isinstance(b, NlpNormBlock):
            continue
        c = b.cols - 1
        for r, i in enumerate(b.rows.tolist()):
            s0, s1 = int(b.seg[r]), int(b.seg[r + 1])
            on = b.weight[s0:s1] != 0.0
            Ar, wr = b.A[s0:s1][on], b.weight[s0:s1][on]
            vr = Ar @ x[c] + b.shift[s0:s1][on]
            mr = np.abs(vr).max() if len(vr) else 0.0
            if mr == 0.0:
                continue                                # the apex: value 0, no derivative
            y = vr / mr
            sr = np.sqrt(np.sum(wr * y * y))
            val = float(mr * sr)
            Gr = Ar.T @ (wr * y / sr)
            mu = float(sigma) if i == 0 else lam[i - 1]
            if i == 0:
                f += val
                np.add.at(g, c, Gr)
            else:
                gv[i - 1] += val
                np.add.at(J[i - 1], c, Gr)
            H[np.ix_(c, c)] += Ar.T @ ((mu * wr / val)[:, None] * Ar) + (-mu / val) * np.outer(Gr, Gr)
    return f, g, gv, J, H


def sum_of_norms_model(anchors, weights=None, smooth=0.0, bounds=(-np.inf, np.inf), ridge=0.0, x0=None) -> NlpTerms:
    """Fermat-Weber location: min sum_k w_k sqrt(|x - a_k|^2 + smooth^2) + ridge sum_j x_j^2 over x in R^dim, anchors [K, dim], weights [K] > 0
    (None: ones).  One NlpNormBlock with K outputs on row 0: output k owns the dim points x_j - a_kj and, with smooth != 0, one
    more point with a zero row of A and the shift smooth; w_k enters as the weight w_k^2 of the points of output k.  No
    constraint rows.  From x0 (None: the weighted mean of the anchors)."""
    a = _f64(np.atleast_2d(anchors))
    K, dim = a.shape
    w = np.ones(K) if weights is None else _f64(weights)
    if w.shape != (K,) or not np.all(w > 0):
        raise ValueError(f"sum_of_norms_model: {K} positive weights")
    per = dim + (1 if smooth else 0)
    A, S = np.zeros((K * per, dim)), np.zeros(K * per)
    for k in range(K):
        A[k * per:k * per + dim] = np.eye(dim)
        S[k * per:k * per + dim] = -a[k]
        if smooth:
            S[k * per + dim] = float(smooth)
    blk = NlpNormBlock(np.arange(1, dim + 1), A, np.zeros(K, np.int64), np.arange(K + 1) * per, S, np.repeat(w * w, per))
    lo, hi = bounds
    start = (w @ a) / w.sum() if x0 is None else x0
    terms = [(0, float(ridge), [(j + 1, POW, 2)]) for j in range(dim)] if ridge else []
    return make_nlp_terms(dim, 0, 0, terms, xL=np.broadcast_to(_f64(lo), (dim,)).copy(), xU=np.broadcast_to(_f64(hi), (dim,)).copy(),
                          x0=start, blocks=[blk])


def robust_lp_model(c, a, P, kappa, b, bounds=(-np.inf, np.inf), smooth=0.0, ridge=0.0, x0=None) -> NlpTerms:
    """A robust linear programme: min c'x + ridge sum_j x_j^2  s.t.  a_k'x + kappa_k sqrt(|P_k x|^2 + smooth^2) <= b_k, lo <= x <= hi
    -- the worst case of a_k'x over an ellipsoid of coefficients.  c [n], a [K, n], P a list of K matrices [l_k, n], kappa [K] > 0,
    b [K].  The K rows are nonlinear rows 1..K: the linear part a_k'x is plain terms on the row, the norm is output k of one
    NlpNormBlock on the variables in use, kappa_k in the weights as kappa_k^2; with smooth != 0 every output gets a point with a
    zero row of A and the shift smooth.  From x0 (None: zeros)."""
    c, a, b_, kap = _f64(c), _f64(np.atleast_2d(a)), _f64(np.atleast_1d(b)), _f64(np.atleast_1d(kappa))
    n, K = len(c), len(a)
    if a.shape != (K, n) or len(P) != K or b_.shape != (K,) or kap.shape != (K,) or not np.all(kap > 0):
        raise ValueError(f"robust_lp_model: a [{K}, {n}], {K} matrices P, kappa > 0 and b [{K}]")
    A, W, S, seg = [], [], [], [0]
    for k in range(K):
        Pk = _f64(np.atleast_2d(P[k]))
        if Pk.shape[1] != n or len(Pk) < 1:
            raise ValueError(f"robust_lp_model: P[{k}] has {n} columns and at least one row")
        rows_k = len(Pk) + (1 if smooth else 0)
        A.append(Pk); S.append(np.zeros(len(Pk)))
        if smooth:
            A.append(np.zeros((1, n))); S.append(np.array([float(smooth)]))
        W.append(np.full(rows_k, kap[k] ** 2)); seg.append(seg[-1] + rows_k)
    A = np.vstack(A)
    used = np.flatnonzero(np.any(A != 0.0, axis=0))
    if len(used) == 0:
        used = np.arange(1)
    blk = NlpNormBlock(used + 1, A[:, used], np.arange(1, K + 1), seg, np.concatenate(S), np.concatenate(W))
    terms = [(0, float(c[j]), [(j + 1, POW)]) for j in np.flatnonzero(c)]
    terms += [(k + 1, float(a[k, j]), [(j + 1, POW)]) for k in range(K) for j in np.flatnonzero(a[k])]
    if ridge:
        terms += [(0, float(ridge), [(j + 1, POW, 2)]) for j in range(n)]
    lo, hi = bounds
    return make_nlp_terms(n, K, 0, terms, xL=np.broadcast_to(_f64(lo), (n,)).copy(), xU=np.broadcast_to(_f64(hi), (n,)).copy(),
                          gL=np.full(K, -np.inf), gU=b_, x0=np.zeros(n) if x0 is None else x0, blocks=[blk])


def socp_synth(n: int, lens, seed: int = 1) -> NlpTerms:
    """A seeded second-order-cone programme on n variables: min c'x + 1e-3 sum x_j^2 + sum of lens[0] norms of 2 points each on
    the objective (a group penalty |B_g x - t_g|), and a cone row a_k'x + |P_k x + s_k| <= b_k of lens[k] points for every k >= 1,
    smoothed by one more point with the shift 1e-2 each.  The entries of P, B are N(0, 1) / sqrt(n) with about half of them zero,
    s, t are 0.3 N(0, 1), and b_k puts x = 0 strictly inside (b_k = |s_k| + 0.5); -3 <= x <= 3, from x = 0."""
    rng = np.random.default_rng(int(seed))
    n = int(n)
    groups = int(lens[0])
    A, S, rows, seg = [], [], [], [0]
    for g in range(groups):
        B = rng.standard_normal((2, n)) / np.sqrt(n) * (rng.random((2, n)) < 0.5)
        A += [B, np.zeros((1, n))]; S += [0.3 * rng.standard_normal(2), [1e-2]]
        rows.append(0); seg.append(seg[-1] + 3)
    K = len(lens) - 1
    a = rng.standard_normal((K, n)) / np.sqrt(n)
    gU = np.zeros(K)
    for k in range(K):
        L = int(lens[k + 1])
        Pk = rng.standard_normal((L, n)) / np.sqrt(n) * (rng.random((L, n)) < 0.5)
        sk = 0.3 * rng.standard_normal(L)
        A += [Pk, np.zeros((1, n))]; S += [sk, [1e-2]]
        rows.append(k + 1); seg.append(seg[-1] + L + 1)
        gU[k] = np.sqrt(sk @ sk + 1e-4) + 0.5
    A, S = np.vstack(A), np.concatenate([np.atleast_1d(v) for v in S])
    used = np.flatnonzero(np.any(A != 0.0, axis=0))
    blk = NlpNormBlock(used + 1, A[:, used], rows, seg, S)
    c = rng.standard_normal(n)
    terms = [(0, float(c[j]), [(j + 1, POW)]) for j in range(n)] + [(0, 1e-3, [(j + 1, POW, 2)]) for j in range(n)]
    terms += [(k + 1, float(a[k, j]), [(j + 1, POW)]) for k in range(K) for j in range(n)]
    return make_nlp_terms(n, K, 0, terms, xL=np.full(n, -3.0), xU=np.full(n, 3.0), gL=np.full(K, -np.inf), gU=gU, x0=np.zeros(n), blocks=[blk])


def norm_scenario(p: NlpTerms, s: int, seed: int = 1, noise: float = 0.05) -> NlpTerms:
    """Scenario s of a model with Euclidean-norm row blocks (s = 0 or noise = 0: p itself): every shift of a point with a
    non-zero row of A moved by noise N(0, 1) -- other anchors, targets, nominal loads; the smoothing points stay.  Structure,
    bounds and start stay."""
    if s == 0 or noise == 0:
        return p
    rng = np.random.default_rng(int(seed) * 1000 + int(s))
    out = dataclasses.replace(p)
    out.blocks = [dataclasses.replace(b, shift=b.shift + noise * rng.standard_normal(len(b.shift)) * np.any(b.A != 0.0, axis=1))
                  if isinstance(b, NlpNormBlock) else b for b in p.blocks]
    return out


def fold_weights(N: int, k: int) -> np.ndarray:
    """[k, N] 0 / 1 weights: row f is 1 on the training rows of fold f of logistic_fold_indices(N, k), 0 on its validation
    rows and on the N % k rows that no fold uses."""
    W = np.zeros((int(k), int(N)))
    for f, (tr, _) in enumerate(logistic_fold_indices(N, k)):
        W[f, tr] = 1.0
    return W


def _ridge(n, reg):
    return [(0, 0.5 * float(reg), [(j + 1, POW, 2)]) for j in range(n)] if reg else []


def logistic_block_model(X, y, reg, weight=None) -> NlpTerms:
    """logistic_model as one SOFTPLUS block: softplus(u) - y u = softplus((1 - 2 y) u) for y in {0, 1}, so row i of X enters
    as (1 - 2 y_i) X_i and the model is sum_i w_i softplus(A_i'w) + reg / 2 |w|^2 -- no linear terms, and the folds or
    resamples of one dataset differ in the weights only (fold_weights).  -50 <= w <= 50, from w = 0."""
    X, y = np.atleast_2d(_f64(X)), _f64(y)
    N, n = X.shape
    blk = NlpBlock(SOFTPLUS, np.arange(1, n + 1), (1.0 - 2.0 * y)[:, None] * X, None, weight)
    return make_nlp_terms(n, 0, 0, _ridge(n, reg), xL=np.full(n, -50.0), xU=np.full(n, 50.0), x0=np.zeros(n), blocks=[blk])


def multinomial_block_model(X, y, K, reg, pinned=True, weight=None) -> NlpTerms:
    """Ridge-regularised K-class logistic regression, sum_i w_i [log sum_k exp(X_i'b_k) - X_i'b_{y_i}] + reg / 2 |b|^2, as one
    softmax block on the variables b_k = x[k d : (k + 1) d] (class-major) plus the ridge terms.  pinned: b_{K-1} = 0, the
    identifiable form.  The folds or resamples of one dataset differ in the weights only (fold_weights).  -50 <= b <= 50,
    from b = 0."""
    X = np.atleast_2d(_f64(X))
    N, d = X.shape
    Kf = int(K) - 1 if pinned else int(K)
    n = Kf * d
    blk = NlpSoftmaxBlock(np.arange(1, n + 1).reshape(Kf, d), X, y, K, pinned, None, weight)
    return make_nlp_terms(n, 0, 0, _ridge(n, reg), xL=np.full(n, -50.0), xU=np.full(n, 50.0), x0=np.zeros(n), blocks=[blk])


def cox_risk(time) -> np.ndarray:
    """risk [N] of times sorted in non-increasing order: risk[i] is the number of points with time >= time[i] (Breslow: a tie
    group shares one value)."""
    t = _f64(np.atleast_1d(time))
    if np.any(np.diff(t) > 0):
        raise ValueError("cox_risk: the times are not sorted in non-increasing order")
    return np.searchsorted(-t, -t, side="right").astype(np.int32)


def cox_block_model(A, time, event, ridge, weight=None, shift=None) -> NlpTerms:
    """Ridge-regularised Cox proportional-hazards regression with Breslow ties,
        sum_i w_i event_i [log sum_{j: time_j >= time_i} w_j exp(A_j'b) - A_i'b] + ridge / 2 |b|^2,
    as one Cox block plus the ridge terms, which keep the fit bounded.  The points are sorted here by decreasing time (a stable
    sort: tied points keep their order) and weight / shift, given in the caller's order, are sorted with them; NlpTerms.cox_order
    is that permutation, so that the weights of another fold or resample are w[p.cox_order] (fold_weights: the folds of the
    sorted points).  -50 <= b <= 50, from b = 0."""
    A, t, ev = np.atleast_2d(_f64(A)), _f64(time), _f64(event)
    N, n = A.shape
    if t.shape != (N,) or ev.shape != (N,):
        raise ValueError(f"time and event: {N} values each")
    order = np.argsort(-t, kind="stable")
    pick = lambda v: None if v is None else _f64(v)[order]
    blk = NlpCoxBlock(np.arange(1, n + 1), A[order], cox_risk(t[order]), ev[order], pick(shift), pick(weight))
    p = make_nlp_terms(n, 0, 0, _ridge(n, ridge), xL=np.full(n, -50.0), xU=np.full(n, 50.0), x0=np.zeros(n), blocks=[blk])
    p.cox_order = order
    return p


def neyman_pearson_model(X, y, alpha, reg, weight=None) -> NlpTerms:
    """Neyman-Pearson classification, labels y in {0, 1}: the logistic loss on the positives under a level on the mean loss of
    the negatives,
        min  sum_{y_i = 1} w_i [softplus(X_i'b) - X_i'b] + reg / 2 |b|^2   s.t.  sum_{y_i = 0} w_i softplus(X_i'b) / sum_{y_i = 0} w_i <= alpha
    as one SOFTPLUS block on X with rows = [0, 1] plus the linear and ridge terms.  weight None: ones; the folds or resamples
    of one dataset differ in the two weight vectors and the coefficients of the linear terms.  -50 <= b <= 50, from b = 0."""
    X, y = np.atleast_2d(_f64(X)), _f64(y)
    N, n = X.shape
    w = np.ones(N) if weight is None else _f64(weight)
    w1, w0 = w * (y == 1), w * (y == 0)
    blk = NlpRowBlock(SOFTPLUS, np.arange(1, n + 1), X, [0, 1], None, np.stack([w1, w0 / w0.sum()]))
    terms = [(0, -float(w1 @ X[:, j]), [(j + 1, POW)]) for j in range(n)] + _ridge(n, reg)
    return make_nlp_terms(n, 1, 0, terms, xL=np.full(n, -50.0), xU=np.full(n, 50.0), gL=[-np.inf], gU=[float(alpha)], x0=np.zeros(n),
                          blocks=[blk])


def rate_constrained_logistic_model(X, y, group, reg, tol) -> NlpTerms:
    """Logistic regression under a bound on the difference of the mean predicted rates of two groups (group in {0, 1}):
    logistic_block_model's block in the objective, and one row
        -tol <= mean_{group = 1} sigmoid(X_i'b) - mean_{group = 0} sigmoid(X_i'b) <= tol
    as a SIGMOID block with one output on row 1 (tol = 0: an equality).  Not convex.  -50 <= b <= 50, from b = 0."""
    X, y, gr = np.atleast_2d(_f64(X)), _f64(y), _f64(group)
    N, n = X.shape
    cols = np.arange(1, n + 1)
    w = (gr == 1) / (gr == 1).sum() - (gr == 0) / (gr == 0).sum()
    blocks = [NlpBlock(SOFTPLUS, cols, (1.0 - 2.0 * y)[:, None] * X), NlpRowBlock(SIGMOID, cols, X, [1], None, w[None, :])]
    return make_nlp_terms(n, 1, 0, _ridge(n, reg), xL=np.full(n, -50.0), xU=np.full(n, 50.0), gL=[-float(tol)], gU=[float(tol)],
                          x0=np.zeros(n), blocks=blocks)


def poisson_block_model(X, counts, reg, weight=None) -> NlpTerms:
    """Ridge-regularised Poisson regression, sum_i w_i [exp(X_i'b) - c_i X_i'b] + reg / 2 |b|^2: an EXP block and the linear
    terms -(sum_i w_i c_i X_ij) b_j, whose coefficients are the instance's as the weights are.  -50 <= b <= 50, from 0."""
    X, c = np.atleast_2d(_f64(X)), _f64(counts)
    N, n = X.shape
    w = np.ones(N) if weight is None else _f64(weight)
    terms = [(0, -float((w * c) @ X[:, j]), [(j + 1, POW)]) for j in range(n)] + _ridge(n, reg)
    blk = NlpBlock(EXP, np.arange(1, n + 1), X, None, w)
    return make_nlp_terms(n, 0, 0, terms, xL=np.full(n, -50.0), xU=np.full(n, 50.0), x0=np.zeros(n), blocks=[blk])


def least_squares_block_model(A, b, reg) -> NlpTerms:
    """sum_i (A_i'x - b_i)^2 + reg / 2 |x|^2: a POW 2 block with the shifts -b (measurements: one b per instance).  No
    bounds, from x = 0."""
    A, b = np.atleast_2d(_f64(A)), _f64(b)
    n = A.shape[1]
    return make_nlp_terms(n, 0, 0, _ridge(n, reg), x0=np.zeros(n), blocks=[NlpBlock(POW, np.arange(1, n + 1), A, -b, None, exp=2)])


def nlp_terms_scenario(p: NlpTerms, s: int, seed: int = 1, noise: float = 0.05) -> NlpTerms:
    """Scenario s of p (s = 0: p itself): every coefficient scaled by 1 + noise * N(0, 1) (5 % by default), g0 moved so
    that every row keeps its value at x0 -- the bounds (and the feasibility of x0) stay.  A larger noise spreads the
    iteration counts of the scenarios (the queue tests: slots that refill at different times)."""
    if s == 0:
        return p
    rng = np.random.default_rng(seed * 1000 + s)
    out = dataclasses.replace(p, tcoef=p.tcoef * (1.0 + noise * rng.standard_normal(len(p.tcoef))), f0=p.f0 + 0.1 * s)
    out.g0 = p.g0 + (nlp_terms_rows(p, p.x0) - nlp_terms_rows(out, p.x0))
    return out


def logistic_fold_indices(N: int, k: int):
    """[(training rows, validation rows)] of the k folds of N points: fold f validates on rows f * (N // k) .. and trains on
    the other (k - 1) * (N // k) of the first k * (N // k) rows; the remainder N % k is dropped."""
    sz = int(N) // int(k)
    assert k >= 2 and sz >= 1
    used = np.arange(k * sz)
    return [(np.concatenate([used[:f * sz], used[(f + 1) * sz:]]), used[f * sz:(f + 1) * sz]) for f in range(k)]


def logistic_folds(X, y, reg, k: int) -> list:
    """logistic_model on each of the k training folds of (X, y) (logistic_fold_indices: equal sizes, the remainder dropped).
    The k models have one structure -- a fold differs in acoef (its rows of X) and in the coefficients of its linear terms
    -- so they are the instances of one context of Context.nlp_attach(folds[0], instance_data=True)."""
    X, y = np.atleast_2d(_f64(X)), _f64(y)
    return [logistic_model(X[tr], y[tr], reg) for tr, _ in logistic_fold_indices(len(y), k)]


def _needs_positive(p: NlpTerms) -> np.ndarray:
    return np.isin(p.fkind, _POSITIVE) | ((p.fkind == POW) & (p.fexp < 0))


def nlp_data_scenario(p: NlpTerms, s: int, seed: int = 1, noise: float = 0.05) -> NlpTerms:
    """Scenario s of p (s = 0: p itself) in the data of its factors: every argument coefficient scaled by 1 + noise z, every
    shift moved by noise z, every real exponent scaled by max(1 + noise z, 0.1), z standard normal cut at +-2; the terms'
    coefficients stay (nlp_terms_scenario moves those).  The single factors of the terms of rows 1..num_linear stay as
    they are.  g0 moves so that every row keeps its value at x0: the bounds and the feasibility of x0 stay.
    A factor that needs a positive argument (LOG, SQRT, POWR, a negative power) gets its perturbation shrunk, coefficients
    and shift together, until the argument at x0 -- and its minimum over the box [xL, xU] where that was positive in p --
    keeps at least half of what it was in p.  The structure (trow, tptr, aptr, avar, fkind, fexp) is p's."""
    if s == 0:
        return p
    rng = np.random.default_rng([int(seed), int(s), 77])
    aptr, avar, acoef = nlp_terms_args(p)
    nfac = len(p.fkind)
    fa = np.repeat(np.arange(nfac, dtype=np.int64), np.diff(aptr))          # factor of an argument
    z = lambda k: np.clip(rng.standard_normal(k), -2.0, 2.0)
    da, db = acoef * noise * z(len(acoef)), noise * z(nfac)
    fixed = np.isin(p.trow[_term_of_factor(p)], np.arange(1, p.num_linear + 1))
    da[fixed[fa]] = 0.0; db[fixed] = 0.0

    def at(x, a, b):
        return np.bincount(fa, a * x[avar - 1], nfac) + b

    def box_min(a, b):
        with np.errstate(invalid="ignore"):
            lo = np.where(a >= 0, a * p.xL[avar - 1], a * p.xU[avar - 1])
        return np.bincount(fa, np.where(a == 0, 0.0, lo), nfac) + b

    theta = np.ones(nfac)
    pos = _needs_positive(p)
    for u0, u1 in ((at(p.x0, acoef, p.fshift), at(p.x0, acoef + da, p.fshift + db)),
                   (box_min(acoef, p.fshift), box_min(acoef + da, p.fshift + db))):
        # the margin is concave in theta: at theta it keeps at least (1 - theta) u0 + theta u1
        k = pos & np.isfinite(u0) & (u0 > 0) & ~(u1 >= 0.5 * u0)
        with np.errstate(all="ignore"):
            theta[k] = np.minimum(theta[k], np.where(np.isfinite(u1[k]), 0.5 * u0[k] / (u0[k] - u1[k]), 0.0))
    a1, b1 = acoef + theta[fa] * da, p.fshift + theta * db
    out = dataclasses.replace(p, fshift=b1)
    if p.aptr is None:
        out.fscale = a1
    else:
        out.acoef = a1
        out.fscale = np.where(np.diff(aptr) > 0, a1[np.minimum(aptr[:-1], len(a1) - 1)], p.fscale) if len(a1) else p.fscale.copy()
    if p.fpar is not None:
        out.fpar = np.where(p.fkind == POWR, p.fpar * np.maximum(1.0 + noise * z(nfac), 0.1), p.fpar)
    out.g0 = p.g0 + (nlp_terms_rows(p, p.x0) - nlp_terms_rows(out, p.x0))
    return out


def from_qcqp(q) -> NlpTerms:
    """The Qcqp q as terms: c_j x_j for every variable, an off-diagonal Q entry v as v x_r x_c, a diagonal one as
    (v / 2) x_r^2, A entries as single plain factors.  The term structure depends on q's structure only."""
    terms = [(0, q.c[j], [(j + 1, POW)]) for j in range(q.n)]
    quad = lambda row, r, c, v: (row, v, [(int(r), POW), (int(c), POW)]) if r != c else (row, 0.5 * v, [(int(r), POW, 2)])
    terms += [quad(0, r, c, v) for r, c, v in zip(q.q0r, q.q0c, q.q0v)]
    terms += [(int(i), v, [(int(j), POW)]) for i, j, v in zip(q.ar, q.ac, q.av)]
    terms += [quad(int(i), r, c, v) for i, r, c, v in zip(q.qi, q.qr, q.qc, q.qv)]
    return make_nlp_terms(q.n, q.m, q.num_linear, terms, g0=q.g0, f0=q.f0, xL=q.xL, xU=q.xU, gL=q.gL, gU=q.gU, x0=q.x0)


def from_polar_acopf(net, lay, joint: bool = False) -> NlpTerms:
    """The polar model of acopf_layout(net) as terms, for a Context created with lay's own COO structures (duplicates
    included).  Flow k of a branch, F = A v_self^2 + v_f v_t (Bc cos(th_f - th_t) + Bs sin(th_f - th_t)), becomes
    A v_self^2 and four four-factor terms through cos(th_f - th_t) = cos th_f cos th_t + sin th_f sin th_t and
    sin(th_f - th_t) = sin th_f cos th_t - cos th_f sin th_t; the twelve coefficients per branch are net.branch_coeffs().
    With joint = True the angle difference is the argument of one factor (affine form): two three-factor terms per flow,
    -Bc v_f v_t cos(th_f - th_t) and -Bs v_f v_t sin(th_f - th_t).
    The structure depends on the topology only: contingency scenarios differ in their coefficients."""
    nb, ng, nl, ndc = net.nb, net.ng, net.nl, net.ndc
    VA, VM, PG = 1, nb + 1, 2 * nb + 1                     # 1-based first variables
    PF = 2 * nb + 2 * ng + 1
    own = [PF, PF + 2 * nl, PF + nl, PF + 3 * nl]          # p_f, q_f, p_t, q_t
    DC = PF + 4 * nl
    T0 = 2 * nl + 1 + 2 * nb                               # rows before the thermal rows
    O0 = T0 + 2 * nl
    co = net.branch_coeffs()
    lin = lambda j: [(int(j), POW)]
    terms = []
    for g in range(ng):
        terms.append((0, net.c2[g], [(PG + g, POW, 2)]))
        terms.append((0, net.c1[g], lin(PG + g)))
    for l in range(nl):
        f, t = int(net.f_bus[l]), int(net.t_bus[l])
        for off in (0, nl):                                # angle <= and >= rows
            terms.append((off + l + 1, 1.0, lin(VA + f)))
            terms.append((off + l + 1, -1.0, lin(VA + t)))
    terms.append((2 * nl + 1, 1.0, lin(VA + net.ref_bus)))
    gs = np.zeros(nb); bs = np.zeros(nb)
    gs[lay.sh_bus] = lay.sh_gs; bs[lay.sh_bus] = lay.sh_bs
    shunted = np.zeros(nb, bool); shunted[lay.sh_bus] = True
    for i in range(nb):
        for k in range(lay.bal_ptr[i], lay.bal_ptr[i + 1]):
            terms.append((2 * nl + 2 + 2 * i, lay.bal_coef[k], lin(lay.bal_colP[k] + 1)))
            terms.append((2 * nl + 3 + 2 * i, lay.bal_coef[k], lin(lay.bal_colQ[k] + 1)))
        if shunted[i]:
            terms.append((2 * nl + 2 + 2 * i, gs[i], [(VM + i, POW, 2)]))
            terms.append((2 * nl + 3 + 2 * i, -bs[i], [(VM + i, POW, 2)]))
    for l in range(nl):
        terms.append((T0 + 2 * l + 1, 1.0, [(own[0] + l, POW, 2)])); terms.append((T0 + 2 * l + 1, 1.0, [(own[1] + l, POW, 2)]))
        terms.append((T0 + 2 * l + 2, 1.0, [(own[2] + l, POW, 2)])); terms.append((T0 + 2 * l + 2, 1.0, [(own[3] + l, POW, 2)]))
    for l in range(nl):
        f, t = int(net.f_bus[l]), int(net.t_bus[l])
        vf, vt = (VM + f, POW), (VM + t, POW)
        cf, sf, ct, st = (VA + f, COS), (VA + f, SIN), (VA + t, COS), (VA + t, SIN)
        for k in range(4):
            A, Bc, Bs = co[l, 3 * k:3 * k + 3]
            row = O0 + 4 * l + k + 1
            terms.append((row, 1.0, lin(own[k] + l)))
            terms.append((row, -A, [(VM + (t if k >= 2 else f), POW, 2)]))
            if joint:
                dth = [(VA + f, 1.0), (VA + t, -1.0)]
                terms.append((row, -Bc, [vf, vt, (dth, COS)]))
                terms.append((row, -Bs, [vf, vt, (dth, SIN)]))
                continue
            terms.append((row, -Bc, [vf, vt, cf, ct]))
            terms.append((row, -Bc, [vf, vt, sf, st]))
            terms.append((row, -Bs, [vf, vt, sf, ct]))
            terms.append((row, Bs, [vf, vt, cf, st]))
    for d in range(ndc):                                   # loss rows: (1 - loss1) p_dc_f + p_dc_t = loss0
        row = O0 + 4 * nl + d + 1
        terms.append((row, 1.0 - lay.dc_loss1[d], lin(DC + d)))
        terms.append((row, 1.0, lin(DC + ndc + d)))
    return make_nlp_terms(lay.n, lay.m, lay.num_linear, terms, xL=lay.xL, xU=lay.xU, gL=lay.gL, gU=lay.gU, x0=lay.x0)
