/*
 * sqphip.h -- C ABI of libsqphip.so, the MI355X (gfx950) hot path behind SqpSolver.Optimizer.
 *
 * What it replaces in /root/reference (exanauts/SqpSolver.jl):
 *   - the per-iteration QP sub-problem that `SqpTR` delegates to `external_optimizer` through
 *     `QpJuMP` (src/algorithms/subproblem_JuMP.jl:127-183 QP, :185-244 LP phase, :283-347 L1QP,
 *     :352-393 feasibility restoration, :398-429 INFEAS, :432-463 trust-region bounds,
 *     :514-563 collect_solution!), i.e. the `AbstractSubOptimizer` seat of
 *     src/algorithms/subproblem.jl:1-28 as dispatched by src/algorithms/sqp_trust_region.jl:314-331;
 *   - the merit / step-acceptance path of src/algorithms: common.jl:14-77, merit.jl:13-17,
 *     sqp.jl:170-213, sqp_trust_region.jl:370-380 and :487-579.
 * The Julia host (MOI_wrapper.jl, model.jl) stays; it reaches this library through `ccall`
 * (binding shown in INTEGRATION.md).  Plain pointers and sizes only; no C++ or torch types.
 *
 * Conventions
 *   - every function returns 0 on success, a negative SQPHIP_E* code on misuse / HIP failure;
 *     nothing throws across the ABI; sqphip_last_error() gives the message.
 *   - solver outcomes are MOI.TerminationStatusCode integers (sub-problem) and the Ipopt-style
 *     codes of src/status.jl:2-23 (whole solve).
 *   - all arrays are caller-owned HOST memory unless the name ends in _dev; indices are 1-based
 *     (Julia-native) at the boundary.
 *   - multipliers use the JuMP sign convention exactly as collect_solution! returns them
 *     (mult_x_U <= 0 <= mult_x_L; stationarity H p + c = J'lambda + mult_x_L + mult_x_U).
 *   - one HIP stream per context; a context is not thread-safe, distinct contexts are.
 */
#ifndef SQPHIP_H
#define SQPHIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sqphip_ctx sqphip_ctx;

enum { SQPHIP_OK = 0, SQPHIP_EINVAL = -1, SQPHIP_EHIP = -2, SQPHIP_ENOMEM = -3, SQPHIP_ESTATE = -4 };

/* sub-problem modes (subproblem_JuMP.jl line ranges above) */
enum { SQPHIP_MODE_QP = 0, SQPHIP_MODE_FR = 1, SQPHIP_MODE_SOC = 2, SQPHIP_MODE_LP = 3,
       SQPHIP_MODE_L1QP = 4, SQPHIP_MODE_INFEAS = 5 };

/* MOI.TerminationStatusCode values this library can return (MathOptInterface v1 enum order) */
enum { SQPHIP_MOI_LOCALLY_SOLVED = 4, SQPHIP_MOI_LOCALLY_INFEASIBLE = 5,
       SQPHIP_MOI_ITERATION_LIMIT = 11, SQPHIP_MOI_NUMERICAL_ERROR = 20 };

/* Mirror of src/parameters.jl:1-30 (fields the hot path reads) plus the sub-solver's own knobs */
typedef struct {
    double tol_direction, tol_residual, tol_infeas;   /* parameters.jl:17-19 */
    double init_mu, max_mu, tr_size;                   /* :22,:23,:28 */
    double rho, eta, tau, min_alpha;                   /* :24-27 (Armijo variant) */
    int32_t max_iter;                                  /* :20 */
    int32_t use_soc;                                   /* :29 */
    int32_t literal_quirks;  /* 1: reproduce SURVEY.md App. C #2/#3 (JuMP-sign Hessian/KT residual) */
    double ipm_tol;          /* interior-point optimality tolerance (scaled), default 1e-9 */
    int32_t ipm_max_iter;    /* default 200; a second-order correction (mode 2) gets half of it: a correction that has not
                              * converged by then is abandoned -- for run! that is the same as any other unsuccessful
                              * correction (no correction step, sqp_trust_region.jl:341-360), and no successful one of a
                              * 5082-sub-problem survey of the IEEE-118 workload needed more than 83 iterations */
    int32_t ipm_phase1;      /* 1: confirm infeasibility verdicts with a phase-1 run (default 0) */
    int32_t device;          /* HIP device ordinal */
    int32_t ipm_corrector;   /* 0 (default since round 4): monotone Fiacco-McCormick barrier rule throughout -- what Ipopt,
                              * the sub-solver of every test and example of the reference, does by default (mu_strategy =
                              * monotone; test/ext_solver.jl:2-6 and examples/acopf/opf.jl:59-64 leave it there): one solve
                              * per factorisation; 1: Mehrotra predictor-corrector iterations until the first inertia
                              * correction of a solve (4 % fewer factorisations on the IEEE-118 workload, a second solve per
                              * iteration: 15 - 25 % slower end to end) */
    int32_t kkt_condense;    /* 1: rows with gL != gU (diagonal block -D of the Newton matrix) are eliminated before
                              * the factorisation: dense LDL^T of order n + #(gL == gU) instead of n + m */
    int32_t kkt_tile_order;  /* 1 (needs kkt_condense): the variables are ordered so that the leading tile columns of
                              * the condensed matrix are mutually independent (sqphip_kkt_order, rows_last = 1) and
                              * the factorisation treats them as such: one launch per kernel for all of them, the
                              * dense chain only on the remainder */
    int32_t kkt_mode;        /* linear solver of the Newton systems.  1: batched dense LDL^T on the MFMA pipe (ldlt.hip);
                              * 2: multifrontal LDL^T of the sparse matrix (mfront.hip: symbolic analysis once per
                              * structure, dense fronts in LDS); 0 (default): the sparse one when it does at most a
                              * quarter of the dense flops and no front exceeds 512 rows, else the dense one */
    int32_t ipm_warm_start;  /* 1: the first interior-point run of a sub-problem starts from the step and the equality-row
                              * multipliers of the instance's previous solved sub-problem of the same mode -- what
                              * warm_start_init_point = "yes" asks of Ipopt (/root/reference/test/ext_solver.jl:5,
                              * examples/acopf/opf.jl:62; upstream the model is rebuilt every iteration, so the option has
                              * no effect there).  0 (default): centred cold start, fewer iterations on every workload
                              * measured */
} sqphip_options;

void sqphip_default_options(sqphip_options *o);

/* Create a context for `batch` NLP instances sharing dimensions and sparsity
 * (one instance = one SqpSolver.Model, src/model.jl:37-67).  COO structures as produced by
 * MOI_wrapper.jl:930-945 (Jacobian) and :1010-1025 (Hessian, triangular, duplicates allowed);
 * nnzH = 0 means no Hessian (LP / SLP).  Bounds may be +-Inf; they apply to every instance
 * until overridden with sqphip_set_bounds.  With options.kkt_condense = 1 the rows with gL == gU given HERE are the
 * ones that stay in the factorised matrix: sqphip_set_bounds may change their values per instance but returns
 * SQPHIP_EINVAL if it would turn one of the other rows into an equality. */
int sqphip_create(sqphip_ctx **ctx, int64_t n, int64_t m, int64_t num_linear,
                  int64_t nnzJ, const int64_t *jrow, const int64_t *jcol,
                  int64_t nnzH, const int64_t *hrow, const int64_t *hcol,
                  const double *xL, const double *xU, const double *gL, const double *gU,
                  const sqphip_options *opt, int32_t batch);
void sqphip_destroy(sqphip_ctx *ctx);
/* Host-only (no GPU): the ordering options.kkt_tile_order = 1 gives the condensed Newton matrix of this structure.
 * pos[u], u < n + #(gL == gU): position of variable u (u < n) or of the (u - n)-th row with gL == gU in the
 * factorised matrix; the first n_lead_tiles 64-column tiles are mutually independent (block-diagonal leading block,
 * identity padding inside the tiles), the positions from 64 * n_lead_tiles to order - 1 are the dense remainder.
 * rows_last = 1 is what the library uses: rows enter a leading tile only behind ALL the variables they couple to,
 * everything else goes to the remainder.  rows_last = 0 lets rows and variables compete freely for the tiles
 * (smaller remainder, but rows pivoted before their variables lose digits -- kept for experiments only).
 * Same COO conventions as sqphip_create. */
int sqphip_kkt_order(int64_t n, int64_t m, int64_t nnzJ, const int64_t *jrow, const int64_t *jcol,
                     int64_t nnzH, const int64_t *hrow, const int64_t *hcol, const double *gL, const double *gU,
                     int32_t rows_last, int32_t *pos, int32_t *n_lead_tiles, int32_t *order);
/* Host-only (no GPU): symbolic analysis of the sparse Newton matrix of this structure -- what the analysis phase of
 * Ipopt's linear solver does for the reference (/root/reference/examples/acopf/opf.jl:59-64).  condense = 1: rows with
 * gL != gU (and at most 32 entries) are eliminated first, as options.kkt_condense does.  rows_after_vars = 1 is what
 * the library uses: a row is ordered behind every variable it couples to.  small_front / zero_frac: amalgamation
 * thresholds (<= 0 / < 0: library defaults).  pos[u], u < order: position of variable u (u < n) or of the (u - n)-th
 * kept row in the elimination order; any output may be NULL. */
typedef struct {
    int64_t order;            /* unknowns of the factorised matrix */
    int64_t nnz_k_lower;      /* structural entries of its lower triangle, diagonal included */
    int64_t n_supernodes, n_levels, max_front, max_cols;
    int64_t nnz_l;            /* entries of L below the diagonal as the dense fronts hold them (explicit zeros included) */
    int64_t nnz_l_exact;      /* ... of the exact sparse factor under the same order */
    double flops, flops_exact;/* 2 x multiply-adds of one numeric factorisation: dense fronts / exact sparse */
    int64_t front_doubles;    /* doubles of front storage per instance */
} sqphip_symbolic_stats;
int sqphip_kkt_symbolic(int64_t n, int64_t m, int64_t nnzJ, const int64_t *jrow, const int64_t *jcol,
                        int64_t nnzH, const int64_t *hrow, const int64_t *hcol, const double *gL, const double *gU,
                        int32_t condense, int32_t rows_after_vars, int32_t small_front, double zero_frac,
                        int32_t *pos, sqphip_symbolic_stats *out);
const char *sqphip_last_error(const sqphip_ctx *ctx);
int sqphip_set_bounds(sqphip_ctx *ctx, int32_t inst, const double *xL, const double *xU,
                      const double *gL, const double *gU);

/* ---- the AbstractSubOptimizer seat ------------------------------------------------------------
 * Replaces sub_optimize! / sub_optimize_FR! / sub_optimize_lp / sub_optimize_L1QP! /
 * sub_optimize_infeas and sub_optimize_soc! (pass mode SOC with E = E_soc,
 * sqp_trust_region.jl:341-360).  Jval/Hval are in the COO order given to sqphip_create
 * (what eval_jac_g / eval_h fill, sqp.jl:93,112); Hval may be NULL.
 * Outputs: p[n], lambda[m], mult_x_U[n], mult_x_L[n] caller-allocated; slack may be NULL else [2m]
 * (t+ then t-).  For mode LP `p` receives the absolute point x (subproblem_JuMP.jl:212-218).
 * Infeasible-family statuses zero the outputs (subproblem_JuMP.jl:551-555). */
int sqphip_qp_solve(sqphip_ctx *ctx, int32_t mode, const double *x_k, double delta, double mu,
                    const double *df, const double *E, const double *Jval, const double *Hval,
                    double *p, double *lambda, double *mult_x_U, double *mult_x_L,
                    double *slack, int32_t *moi_status);
/* statistics of the last sqphip_qp_solve: interior-point iterations, KKT factorisations */
int sqphip_qp_stats(const sqphip_ctx *ctx, int32_t *ipm_iters, int32_t *n_factor);
/* ... how its last interior-point run ended: rule 0 = scaled optimality error <= options.ipm_tol, 1 / 2 / 3 = one of the
 * acceptable-termination rules (8 consecutive iterates within 100 x the tolerance, 15 within 1 000 x, 25 within 10^4 x:
 * what Ipopt's acceptable_tol / acceptable_iter do for the reference's sub-solver, test/ext_solver.jl:2-6), -1 = not
 * converged; scaled_error = that error at the final iterate.  A sub-problem reported LOCALLY_SOLVED under rule 3 is
 * accurate to 1e4 x ipm_tol only. */
int sqphip_qp_termination(const sqphip_ctx *ctx, int32_t *rule, double *scaled_error);

/* ---- the seat for many host models at once ---------------------------------------------------------
 * `count` sub-problems in one call, request k on instance inst[k] of the context -- the bounds sqphip_set_bounds gave that
 * instance -- with its own mode[k], delta[k], mu[k].  Arrays are stored back to back per request: x_k, df [count][n],
 * E [count][m], Jval [count][nnzJ], Hval [count][nnzH] or NULL; outputs p, mult_x_U, mult_x_L [count][n], lambda [count][m],
 * slack [count][2m] or NULL, moi_status [count].  count in 1 .. batch, inst[k] in range and pairwise distinct, modes in range,
 * else SQPHIP_EINVAL with sqphip_last_error naming the offending index; NULL rules as for sqphip_qp_solve (df and E may be
 * NULL only when every mode is LP).  Request k returns bit for bit what sqphip_qp_solve returns for it on a context whose
 * instance 0 carries the bounds of inst[k]: no instance's arithmetic depends on which others are active.  Instances not
 * listed keep their outputs, warm-start state and interior-point state (the start flags are cleared for all, as
 * sqphip_qp_solve does).  The call lasts as long as its slowest request.  Its HIP traffic does not grow with count: the
 * operands are packed into a pinned staging buffer (allocated at the first batch call, sized for the batch), moved by one
 * copy and spread over the instances by one kernel; results and the instances' states come back the same way.  The
 * counters of sqphip_get_counters advance by the sums over the batch; afterwards sqphip_qp_stats / _termination describe
 * request count - 1. */
int sqphip_qp_solve_batch(sqphip_ctx *ctx, int32_t count, const int32_t *inst, const int32_t *mode, const double *x_k,
                          const double *delta, const double *mu, const double *df, const double *E, const double *Jval,
                          const double *Hval, double *p, double *lambda, double *mult_x_U, double *mult_x_L, double *slack,
                          int32_t *moi_status);
/* sqphip_qp_stats and sqphip_qp_termination for the last sub-problem of each listed instance, read from the device
 * ([count] each, any may be NULL) */
int sqphip_qp_stats_batch(const sqphip_ctx *ctx, int32_t count, const int32_t *inst, int32_t *ipm_iters, int32_t *n_factor,
                          int32_t *rule, double *scaled_error);

/* ---- merit / acceptance path (device reductions over host-supplied vectors) -------------------- */
/* common.jl:54-77; pnorm 1, 2 or 0 (=Inf) */
int sqphip_norm_violations(sqphip_ctx *ctx, const double *E, const double *x, int32_t pnorm,
                           double *out);
/* common.jl:14-23 */
int sqphip_kt_residuals(sqphip_ctx *ctx, const double *df, const double *lambda,
                        const double *mult_x_U, const double *mult_x_L, const double *Jval,
                        double *out);
/* common.jl:30-47 */
int sqphip_norm_complementarity(sqphip_ctx *ctx, const double *E, const double *lambda,
                                int32_t pnorm, double *out);
/* sqp.jl:170-183 given f(x+ap), g(x+ap) from the host callbacks */
int sqphip_compute_phi(sqphip_ctx *ctx, double f_trial, const double *E_trial,
                       const double *x_trial, double mu, int32_t feasibility_restoration,
                       double *phi);
/* sqp_trust_region.jl:487-508: q(p) if with_step else q(0) */
int sqphip_compute_qmodel(sqphip_ctx *ctx, const double *x, const double *p, const double *df,
                          const double *E, const double *Jval, const double *Hval, double mu,
                          int32_t with_step, double *q);
/* merit.jl:13-17 + sqp.jl:190-213 (scalar-mu form): D = df'p - mu * sum(viol(E)) */
int sqphip_compute_derivative(sqphip_ctx *ctx, const double *df, const double *p,
                              const double *E, double mu, double *D);
/* The whole compute_derivative(sqp) of sqp.jl:190-213 over merit.jl:13-17.  mu_vec (may be NULL): the vector-penalty
 * forms D = dfp - mu_vec' cons_viol (merit.jl:14,17), else D = dfp - mu sum(cons_viol) (:15,:16).
 * feasibility_restoration = 1 (sqp.jl:194-203): dfp = sum of the slack values of the last sub-problem (slack[2m] as
 * sqphip_qp_solve returns them), cons_viol_i = violation of E_i - viol_i. */
int sqphip_compute_derivative_full(sqphip_ctx *ctx, const double *df, const double *p, const double *E, double mu,
                                   const double *mu_vec, int32_t feasibility_restoration, const double *slack,
                                   double *D);
/* Batch forms of the merit calls run! makes: `count, inst` in front as for sqphip_qp_solve_batch, every vector operand
 * [count][.] stored back to back, every scalar operand [count], flags (pnorm, feasibility_restoration, with_step) one value
 * per call, out [count].  Operands of request k are staged into the vectors of instance inst[k] and reduced with its bounds
 * by the arithmetic of the scalar call, in the same order: out[k] is bit for bit the scalar result. */
int sqphip_norm_violations_batch(sqphip_ctx *ctx, int32_t count, const int32_t *inst, const double *E, const double *x,
                                 int32_t pnorm, double *out);
int sqphip_kt_residuals_batch(sqphip_ctx *ctx, int32_t count, const int32_t *inst, const double *df, const double *lambda,
                              const double *mult_x_U, const double *mult_x_L, const double *Jval, double *out);
int sqphip_norm_complementarity_batch(sqphip_ctx *ctx, int32_t count, const int32_t *inst, const double *E,
                                      const double *lambda, int32_t pnorm, double *out);
int sqphip_compute_phi_batch(sqphip_ctx *ctx, int32_t count, const int32_t *inst, const double *f_trial,
                             const double *E_trial, const double *x_trial, const double *mu,
                             int32_t feasibility_restoration, double *phi);
int sqphip_compute_qmodel_batch(sqphip_ctx *ctx, int32_t count, const int32_t *inst, const double *x, const double *p,
                                const double *df, const double *E, const double *Jval, const double *Hval, const double *mu,
                                int32_t with_step, double *q);
/* mu_vec [count][m] or NULL for the whole call; slack [count][2m] under feasibility restoration */
int sqphip_compute_derivative_full_batch(sqphip_ctx *ctx, int32_t count, const int32_t *inst, const double *df,
                                         const double *p, const double *E, const double *mu, const double *mu_vec,
                                         int32_t feasibility_restoration, const double *slack, double *D);
/* sqp_trust_region.jl:529-538,:574-577: ratio test and radius update.
 * accept_out = 1 if ared > 0 and ared/pred > 0; delta_out the updated radius. */
int sqphip_tr_update(double ared, double pred, double delta, double pnorm_inf,
                     double delta_max, double tol_direction, int32_t *accept_out,
                     double *delta_out);

/* sqp_line_search.jl:303-334 (compute_alpha; the line-search algorithm is unreachable upstream, kept for
 * completeness of the merit path): backtracking Armijo search alpha <- tau * alpha while
 * phi(alpha) > phi0 + eta * alpha * D, starting from 1; stops with is_valid = 0 once alpha < min_alpha.
 * phi(alpha) is the caller's merit at x + alpha p (compute_phi needs eval_f / eval_g: host callbacks), so it
 * comes in as a C callback.  Returns at once with alpha = 1, is_valid = 1 when pnorm_inf <= tol_direction. */
typedef double (*sqphip_phi_fn)(double alpha, void *user);
int sqphip_armijo_alpha(double phi0, double D, double eta, double tau, double min_alpha, double pnorm_inf,
                        double tol_direction, sqphip_phi_fn phi, void *user, double *alpha, int32_t *is_valid);
/* sqp_line_search.jl:270-294 (compute_mu_rule1! / rule2! / rule3!), vector penalty mu[m]:
 *   t = (df'p + max(p'Hp/2, 0)) / max((1 - rho) * viol1, 1e-8)
 *   rule 1: mu_i = max(mu_i, t, |lambda_i|);  rule 2: iter == 1 ? mu_i = t : mu_i = max(mu_i, |lambda_i|);
 *   rule 3: mu_i = max(mu_i, |lambda_i|) */
int sqphip_compute_mu_rule(int32_t rule, int64_t iter, double rho, double viol1, double dfp, double half_pHp,
                           int64_t m, const double *lambda, double *mu);
/* The same rules with every reduction on the device (wave-level butterflies + LDS exchange): norm_violations(sqp, 1),
 * df'p and p'Hp/2 from the iterate (x, E, df, p, Hval in the COO order of the structure; Hval may be NULL), then the
 * element-wise update of mu[m] (in/out, host memory). */
int sqphip_compute_mu_rule_dev(sqphip_ctx *ctx, int32_t rule, int64_t iter, double rho, const double *x, const double *E,
                               const double *df, const double *p, const double *Hval, const double *lambda, double *mu);
/* compute_alpha (sqp_line_search.jl:303-334) for an instance of the built-in ACOPF evaluator, entirely on the device:
 * phi(alpha) = f(x + alpha p) + mu |viol(x + alpha p)|_1 (|viol|_1 alone under feasibility restoration,
 * sqp.jl:170-183) is evaluated by the device callbacks, the backtracking loop alpha <- tau alpha runs inside the kernel
 * and stops with is_valid = 0 once alpha < min_alpha.  n_eval = merit evaluations made. */
int sqphip_acopf_armijo(sqphip_ctx *ctx, int32_t inst, const double *x, const double *p, double mu, double phi0,
                        double D, double eta, double tau, double min_alpha, int32_t feasibility_restoration,
                        double *alpha, int32_t *is_valid, int32_t *n_eval);

/* ---- device-resident batched SQP-TR over the built-in ACOPF evaluator --------------------------
 * (sqp_trust_region.jl:98-223 for every instance of the batch; callbacks of
 * MOI_wrapper.jl:1115-1146 replaced by HIP kernels over PowerModels-ACP-shaped data,
 * test/opf.jl:5-9).  Topology is shared; electrical data, loads and bounds are per instance. */
int sqphip_acopf_attach(sqphip_ctx *ctx, int32_t nb, int32_t ng, int32_t nl,
                        const int32_t *f_bus, const int32_t *t_bus, const int32_t *gen_bus,
                        const int32_t *bal_ptr, const int32_t *bal_colP, const int32_t *bal_colQ,
                        const double *bal_coef, int32_t ref_bus);
/* The same evaluator in rectangular voltage coordinates: PowerModels' ACRPowerModel under the build_opf of
 * /root/reference/examples/acopf/opf.jl:12-43 -- the formulation run_sqp_opf instantiates (:46, :51).  Variables
 * (vi, vr, pg, qg, flows, dc lines), rows vi[ref] = 0; power balance; vmin^2 <= vr^2 + vi^2 and vr^2 + vi^2 <= vmax^2 per
 * bus (constraint_voltage_magnitude_bounds); thermal limits; Ohm's law with v_f v_t cos / sin written as
 * vr_f vr_t + vi_f vi_t and vi_f vr_t - vr_f vi_t (same twelve coefficients per branch); dc-line losses; no
 * angle-difference rows (opf.jl:33).  The context must have been created with the structure of
 * sqpsolver.jl_amd/acopf_synth.py acr_layout; everything after the attach (set_shunts: four Jacobian and two Hessian
 * entries per shunted bus, num_linear = 1; set_dclines; set_instance; eval; sqp_run) is shared with the polar form. */
int sqphip_acopf_attach_acr(sqphip_ctx *ctx, int32_t nb, int32_t ng, int32_t nl,
                            const int32_t *f_bus, const int32_t *t_bus, const int32_t *gen_bus,
                            const int32_t *bal_ptr, const int32_t *bal_colP, const int32_t *bal_colQ,
                            const double *bal_coef, int32_t ref_bus);
/* ... and in the W-space form of /root/reference/examples/acopf/acwr.jl:1-37 (ACWRPowerModel over PowerModels' build_opf;
 * defined by the reference, instantiated by none of its scripts): variables (vi, vr, w, wr, wi, pg, qg, flows, dc lines)
 * with w_i = |v_i|^2 and wr, wi per bus pair i < j; balance, angle-difference (wi <= tan(angmax) wr, wi >= tan(angmin) wr)
 * and Ohm rows linear in (w, wr, wi); constraint_model_voltage as nb + 2 nbp quadratic equalities; thermal limits.
 * Structure: sqpsolver.jl_amd/acopf_synth.py acwr_layout.  bp_i / bp_j: the buses of pair k; br_bp / br_sig: pair and
 * orientation (+1: from = i, -1: from = j) of branch l; bp_tmin / bp_tmax: tan of the pair's angle limits.  Shunts enter
 * the (linear) balance rows through w: sqphip_acopf_set_shunts supplies them without changing the structure. */
int sqphip_acopf_attach_acwr(sqphip_ctx *ctx, int32_t nb, int32_t ng, int32_t nl,
                             const int32_t *f_bus, const int32_t *t_bus, const int32_t *gen_bus,
                             const int32_t *bal_ptr, const int32_t *bal_colP, const int32_t *bal_colQ,
                             const double *bal_coef, int32_t ref_bus, int32_t nbp, const int32_t *bp_i,
                             const int32_t *bp_j, const int32_t *br_bp, const double *br_sig, const double *bp_tmin,
                             const double *bp_tmax);
/* Bus shunts (optional, after sqphip_acopf_attach): bus sh_bus[s] consumes gs[s] vm^2 of active and injects
 * bs[s] vm^2 of reactive power.  The context must have been created with the matching structure: two more Jacobian
 * COO entries (P row, Q row; column vm) and one more Hessian COO entry (vm, vm) per shunted bus at the END of the
 * lists, and num_linear = 2 nl + 1 (the balance rows are no longer linear) -- sqpsolver.jl_amd/acopf_synth.py,
 * acopf_layout.  Shared by every instance of the batch. */
int sqphip_acopf_set_shunts(sqphip_ctx *ctx, int32_t nsh, const int32_t *sh_bus, const double *gs, const double *bs);
/* HVDC lines (optional, after sqphip_acopf_attach; PowerModels variable_dcline_power +
 * constraint_dcline_power_losses, /root/reference/examples/acopf/opf.jl:16,40-42).  The structure given to
 * sqphip_create carries them already -- per line 4 variables (p_f, p_t, q_f, q_t of the line, blocks of ndc behind
 * all other variables, entering the balance rows of their buses through the incidence lists of sqphip_acopf_attach)
 * and one row  (1 - loss1) p_f + p_t = loss0  behind all other rows, its two Jacobian entries behind all others
 * (acopf_synth.py, acopf_layout); this call supplies loss1 per line (default 0).  ndc must match the structure. */
int sqphip_acopf_set_dclines(sqphip_ctx *ctx, int32_t ndc, const double *loss1);
/* ohm[nl][12]: per branch the coefficients (A, Bc, Bs) of the four flow equations p_f, q_f, p_t, q_t,
 *   F_k = A_k v_self^2 + v_f v_t (Bc_k cos(va_f - va_t) + Bs_k sin(va_f - va_t)),
 * i.e. the pi model with an ideal transformer (tap ratio, phase shift) at the from end folded into 12 numbers on the
 * host (sqpsolver.jl_amd/acopf_synth.py, Network.branch_coeffs); an outaged branch is 12 zeros. */
int sqphip_acopf_set_instance(sqphip_ctx *ctx, int32_t inst, const double *ohm, const double *c2, const double *c1,
                              const double *x0);
/* Evaluate the five callbacks on the device for instance `inst` at host point x (parity tests): the attached device
 * callbacks, whichever attach provided them (ACOPF, dense, QCQP, factorable NLP).  Any output may be NULL.
 * lambda/sigma only matter for hval. */
int sqphip_acopf_eval(sqphip_ctx *ctx, int32_t inst, const double *x, double sigma,
                      const double *lambda, double *f, double *grad, double *g, double *jval,
                      double *hval);
/* A synthetic NLP with a DENSE Lagrangian Hessian for the batched run (bench.py --workload dense; no reference counterpart:
 * the reference's examples are ACOPF models, whose Hessians are sparse):
 *     min  1/2 x'Qx + c'x + kappa / 4 sum_i x_i^4    s.t.  A x = b,  xL <= x <= xU
 * Q [n][n] symmetric and A [m][n] row-major are shared by the batch; an instance carries c [n], its start x0 and -- through
 * sqphip_set_bounds -- xL, xU and gL = gU = b.  The context must have been created with the matching structure
 * (sqpsolver.jl_amd/dense_synth.py): Jacobian COO = A row-major (m n entries), Hessian COO = lower triangle of Q
 * column-major (n (n + 1) / 2 entries), num_linear = m.  With options.kkt_mode = 1 every sub-problem factorises a dense
 * Newton matrix of order n + m on the MFMA path (ldlt.hip). */
int sqphip_dense_attach(sqphip_ctx *ctx, const double *Q, const double *A, double kappa);
int sqphip_dense_set_instance(sqphip_ctx *ctx, int32_t inst, const double *c, const double *x0);
/* A general sparse QCQP for the batched run -- any user model whose objective and rows are at most quadratic:
 *     min  f0 + c'x + 1/2 x'Q0 x    s.t.  gL_i <= g0_i + a_i'x + 1/2 x'Q_i x <= gU_i  (i = 1..m),   xL <= x <= xU
 * Terms are triplets with 1-based indices: Q0 as (q0r, q0c, q0v), A as (ar = row, ac = column, av), every Q_i as
 * (qi = row, qr, qc, qv).  A Q entry may sit in either triangle and duplicates are summed; it folds into the lower
 * triangle with the value convention of the Hessian COO: an off-diagonal v contributes v x_r x_c, a diagonal v
 * contributes 1/2 v x_r^2.  The context must have been created with a Jacobian COO that holds every entry the terms need
 * (A's, and (i, r), (i, c) of every Q_i term) and a Hessian COO that holds the lower entry of every Q0 / Q_i term (with
 * nnzH = 0 only the Jacobian is checked: the SLP path); rows 1..num_linear must carry no quadratic term.  The values
 * given here (c [n] and g0 [m] may be NULL: zeros) start every instance.  Once, on the host, the call builds gather
 * plans from the terms and the COO structures (per row, per variable, per Jacobian and per Hessian COO slot); the
 * device evaluates them per instance with fixed summation orders (bit-reproducible, independent of the slot).
 * Returns SQPHIP_EINVAL, sqphip_last_error naming the first offending term, on an index out of range, an entry the COO
 * structures lack or a quadratic term in a linear row; SQPHIP_ESTATE on a context attached before (any *_attach).
 * On a QCQP context sqphip_acopf_set_instance, _set_shunts, _set_dclines and sqphip_sqp_stream_begin / _set return
 * SQPHIP_EINVAL: their tables are those of the ACOPF evaluators.  The scenario queue of a QCQP context is begun and
 * filled with sqphip_qcqp_stream_begin / _set (below) and then run, shared and read with the sqphip_sqp_stream_* calls.
 * An instance's values are one block of doubles (f0 | c | Q0 | g0 | A | Q, padded to an even count).
 * sqphip_acopf_eval probes the attached device callbacks, the QCQP evaluator included. */
int sqphip_qcqp_attach(sqphip_ctx *ctx, int64_t nnzQ0, const int64_t *q0r, const int64_t *q0c, const double *q0v,
                       int64_t nnzA, const int64_t *ar, const int64_t *ac, const double *av,
                       int64_t nnzQ, const int64_t *qi, const int64_t *qr, const int64_t *qc, const double *qv,
                       const double *c, const double *g0, double f0);
/* Per-instance values, in the term order of the attach (f0 one value, c [n], q0v [nnzQ0], g0 [m], av [nnzA],
 * qv [nnzQ]) and the start x0 [n]; any pointer may be NULL: keep.  Same structure, other coefficients (zeros allowed):
 * contingency-style scenarios.  Bounds go through sqphip_set_bounds. */
int sqphip_qcqp_set_instance(sqphip_ctx *ctx, int32_t inst, const double *f0, const double *c, const double *q0v,
                             const double *g0, const double *av, const double *qv, const double *x0);
/* A sparse factorable NLP for the batched run -- any user model whose objective and rows are sums of products of
 * univariate functions:
 *     min  f0 + sum_{t: trow[t] = 0} c_t prod_k phi_tk(x_{v_tk})
 *     s.t. gL_i <= g0_i + sum_{t: trow[t] = i} c_t prod_k phi_tk(x_{v_tk}) <= gU_i  (i = 1..m),   xL <= x <= xU
 * Every factor is phi(x) = kappa(a x + b) with kappa = fkind: 0 POW u^e (integer e = fexp, 1 <= |e| <= 32; fexp is read
 * for POW only), 1 SIN, 2 COS, 3 EXP, 4 LOG; a = fscale, b = fshift.  Term t has the factors tptr[t] .. tptr[t + 1] - 1 of
 * the factor arrays, at least 1 and at most 8, on distinct variables (x x is written x^2); a constant belongs in f0 / g0.
 * The context must have been created with a Jacobian COO that holds (i, v) for every factor of a term of row i and --
 * unless nnzH = 0, the SLP path -- a Hessian COO that holds the lower entry (v, w) for every two factors of one term
 * and (v, v) for every factor that is not a plain linear POW with e = 1; a term of rows 1..num_linear is a single POW
 * factor with e = 1, a = 1, b = 0.  The structure (rows, variables, kinds, e, a, b) is shared by the batch; the values
 * given here (g0 [m] may be NULL: zeros) start every instance.  Once, on the host, the call builds gather plans from
 * the terms and the COO structures (per row, per variable, per Jacobian and per Hessian COO slot; the first COO copy
 * of a duplicated slot owns its plan, the other copies stay 0); the device evaluates per instance in two passes --
 * phi, phi', phi'' of every factor, then products over the plans -- with fixed summation orders (bit-reproducible,
 * independent of the slot).
 * Domain is the caller's business: LOG and negative powers need bounds that keep a x + b positive at every point the
 * solver visits.  Note that the linear-feasibility phase moves to x = 0 when the linear rows are infeasible inside the
 * first trust region (its outputs are zeroed on an infeasible LP), whatever the bounds say: start from a point that
 * satisfies the linear rows when a factor is undefined at 0.
 * Returns SQPHIP_EINVAL, sqphip_last_error naming the 1-based term (and factor), on an index out of range, an unknown
 * kind, an exponent of 0 or beyond +-32, a term with no or with more than 8 factors, a variable twice in one term, a
 * nonlinear term in a linear row, or an entry the COO structures lack; SQPHIP_ESTATE on a context attached before (any
 * *_attach).  On such a context sqphip_sqp_reset / _run / _get / _status / _trace / _work / _qp_log* / _last_request
 * and the counters work unchanged, sqphip_acopf_eval probes the evaluator and sqphip_acopf_armijo works;
 * sqphip_acopf_set_instance, _set_shunts, _set_dclines, sqphip_qcqp_set_instance and the ACOPF and QCQP queues'
 * _stream_begin / _set (sqphip_sqp_stream_begin, sqphip_qcqp_stream_begin) return SQPHIP_EINVAL: their tables are those
 * of the other evaluators.  The scenario queue of an NLP context is begun and filled with sqphip_nlp_stream_begin / _set
 * (below) and then run, shared and read with the sqphip_sqp_stream_* calls.
 * An instance's values are one block of doubles (f0 | g0 | c, padded to an even count). */
int sqphip_nlp_attach(sqphip_ctx *ctx, int64_t nterms, const int64_t *trow /* 0: objective, i: row i */,
                      const double *tcoef, const int64_t *tptr /* [nterms + 1], offsets into the factor arrays */,
                      const int64_t *fvar /* 1-based */, const int32_t *fkind, const int32_t *fexp,
                      const double *fscale, const double *fshift /* either may be NULL: 1 and 0 */,
                      const double *g0 /* [m] or NULL */, double f0);
/* The same model with factors of affine multi-variable arguments -- least-squares residuals (a'x - b)^2, exp(a'x),
 * log(a'x + b), 1 / (a'x + b), sin(th_f - th_t):
 *     factor k = kappa(u_k),   u_k = sum_{j = aptr[k] .. aptr[k + 1] - 1} acoef[j] x_{avar[j]} + fshift[k]
 * with kappa = fkind[k] from the menu above (fexp for POW, 1 <= |e| <= 32).  u is summed in argument order and the shift
 * is added last: u = 0, then u = fma(acoef[j], x, u) for every argument -- each step one fused multiply-add, so only the
 * first product is rounded on its own --, then u + fshift[k].  An evaluator that rounds every product separately follows
 * the same order and agrees to a few units in the last place of the largest partial sum (about 1e-13 relative in the
 * outputs), not bit for bit.  A factor of one argument is evaluated as sqphip_nlp_attach evaluates it, u = a x + b in one
 * fused expression.  Term t has the factors tptr[t] .. tptr[t + 1] - 1, at least 1 and at most 8; a factor
 * has at least 1 and at most 8 arguments; the variables of a term are distinct across all arguments of all its factors
 * (so every Hessian entry of a term is a single product).  A term of rows 1..num_linear is a single POW factor with
 * e = 1, one argument with coefficient 1 and shift 0.
 * The context must have been created with a Jacobian COO that holds (i, v) for every argument of every factor of a term
 * of row i and -- unless nnzH = 0 -- a Hessian COO that holds the lower entry (v, w) for every two distinct variables of
 * one term, except two arguments of the same plain linear factor (POW, e = 1: kappa'' = 0), and (v, v) for every argument
 * of a factor that is not plain linear.  With v in factor a and w in factor b the device files
 *     d/dx_v = c a_v kappa'_a prod_{k != a} kappa_k,    d2/dx_v dx_w = c a_v a_w kappa'_a kappa'_b prod_{others}  (a != b),
 *     d2/dx_v dx_w = c a_v a_w kappa''_a prod_{k != a} kappa_k  (a = b, v = w included),
 * products in factor order, one thread per output entry summing in term order, no atomics (bit-reproducible,
 * independent of the slot).  A model with one argument per factor files the bits it files through sqphip_nlp_attach.
 * The structure, acoef included, is shared by the batch (sqphip_nlp_attach_data below hands shifts, coefficients and real
 * exponents to the instance); an instance's values are f0 | g0 | c as above, so
 * sqphip_nlp_set_instance, sqphip_nlp_stream_begin / _set, sqphip_sqp_stream_* and everything sqphip_nlp_attach lists
 * work on such a context unchanged (it is an NLP context to every other entry point).
 * Domain is the caller's business, as above: LOG and negative powers need u > 0 at every point the solver visits.
 * Returns SQPHIP_EINVAL, sqphip_last_error naming the 1-based term and factor, on aptr[0] != 0 or a decreasing aptr, a
 * factor with no or with more than 8 arguments, a variable out of range, a variable twice in one factor or twice across
 * the factors of one term, an unknown kind, an exponent of 0 or beyond +-32, a term with no or with more than 8 factors,
 * a term in a linear row that is not the plain one above, or a Jacobian / Hessian entry (named) that the COO structures
 * lack; SQPHIP_ESTATE on a context attached before (any *_attach). */
int sqphip_nlp_attach_affine(sqphip_ctx *ctx, int64_t nterms, const int64_t *trow, const double *tcoef,
                             const int64_t *tptr /* [nterms + 1] factors of a term */,
                             const int64_t *aptr /* [nfac + 1] arguments of a factor */,
                             const int64_t *avar /* [nargs] 1-based */, const double *acoef /* [nargs] or NULL: ones */,
                             const int32_t *fkind, const int32_t *fexp, const double *fshift /* [nfac] or NULL: zeros */,
                             const double *g0 /* [m] or NULL */, double f0);
/* The same model once more, with two restrictions lifted.
 * (1) A variable may occur in several factors of one term: x log x (a POW and a LOG factor on x), x exp(-x), x / (1 + x),
 * (x + y)(x - y), sin x cos x, any product of affine forms with overlapping supports.  Twice inside one factor stays
 * refused (add the coefficients).  With F(v) the (factor, argument) couples of a term on variable v the device files
 *     d/dx_v       = c sum_{(a,j) in F(v)} a_j kappa'_a prod_{k != a} kappa_k
 *     d2/dx_v dx_w = c sum_{(a,j) in F(v)} sum_{(b,l) in F(w)} a_j a_l [a = b ? kappa''_a prod_{k != a} kappa_k
 *                                                                            : kappa'_a kappa'_b prod_{k != a, b} kappa_k],
 * every summand one plan entry: two different arguments on the same variable enter the slot (v, v) twice, once per order.
 * The context must have been created with a Jacobian COO that holds (i, v) for every argument of a term of row i and --
 * unless nnzH = 0 -- a Hessian COO that holds the lower entry (v, w) for every two arguments of a term that lie in
 * different factors, or in the same factor when it is not plain linear (POW, e = 1), and (v, v) for every argument of a
 * factor that is not plain linear and for every variable that sits in two factors of a term, plain linear or not.
 * (2) The menu goes on after LOG: 5 SQRT, 6 TANH, 7 ATAN, 8 SIGMOID 1 / (1 + e^-u), 9 SOFTPLUS log(1 + e^u), 10 POWR u^p with
 * the real exponent p = fpar[k], finite and not 0 (fpar is read for POWR only and may be NULL when there is none; a POWR
 * factor is never plain linear, p = 1 included).  SIGMOID and SOFTPLUS are evaluated through e = exp(-|u|) (e / (1 + e)
 * or 1 / (1 + e); max(u, 0) + log1p(e)) and stay finite with their derivatives for every finite u.  SQRT and POWR need
 * u > 0 at every point the solver visits: the caller's business, as for LOG.
 * Everything else is sqphip_nlp_attach_affine: the limits (8 factors, 8 arguments), the order of the sums, the rule for
 * rows 1..num_linear, the refusals and their 1-based messages (plus: POWR without fpar, a real exponent that is 0 or not
 * finite), SQPHIP_ESTATE on a context attached before, the block f0 | g0 | c of an instance, and the result is an NLP
 * context to every other entry point.  A model that sqphip_nlp_attach or sqphip_nlp_attach_affine takes files the same
 * bits through this call. */
int sqphip_nlp_attach_general(sqphip_ctx *ctx, int64_t nterms, const int64_t *trow, const double *tcoef,
                              const int64_t *tptr /* [nterms + 1] factors of a term */,
                              const int64_t *aptr /* [nfac + 1] arguments of a factor */,
                              const int64_t *avar /* [nargs] 1-based */, const double *acoef /* [nargs] or NULL: ones */,
                              const int32_t *fkind, const int32_t *fexp,
                              const double *fpar /* [nfac] or NULL: real exponent, read for POWR only */,
                              const double *fshift /* [nfac] or NULL: zeros */, const double *g0 /* [m] or NULL */, double f0);
/* The same model once more, with the data of the factors owned by the instance: shifts, coefficients and real exponents may
 * differ between the instances of a batch and between the scenarios of a queue -- one dataset per instance of
 * logistic_model-like fits (cross-validation folds, bootstrap resamples), measurements b_s in (a'x - b_s)^2 or
 * exp(a'x - b_s), one vector of elasticities per consumer, a phase-shifter angle per contingency.  The arguments, the class
 * of models, the checks, the messages and SQPHIP_ESTATE on a context attached before are those of sqphip_nlp_attach_general,
 * and the result is an NLP context to every other entry point.  What stays shared is the structure proper: rows, terms,
 * factors, arguments and their variables, kinds, integer exponents.
 * An instance's block of doubles becomes
 *     f0 | g0 [m] | c [nterms] | b [nfac] | a [nargs] | p [nfac]       (padded to an even count)
 * with b = fshift, a = acoef in argument order and p = fpar; the p segment exists only when the model has a POWR factor.
 * The call fills the data segments of every instance with the arrays given here (NULL acoef: ones, NULL fshift: zeros).
 * sqphip_nlp_set_instance keeps writing f0 | g0 | c and leaves the data alone; sqphip_nlp_stream_set writes a whole block,
 * the data of this call included.  The device reads b, a, p from the instance's block in pass 1 and the weights a_v of the
 * derivative plans from its a segment (a one-argument factor keeps a folded into phi', phi'' and the weight 1.0); orders
 * of summation, the absence of atomics and the factor workspace are unchanged.
 * Bit rule: a context attached through this call whose instances all carry the data of the attach files, in all five
 * callbacks and in sqphip_sqp_get, the bits of the same model attached through sqphip_nlp_attach_general, with equal work
 * counters.  Contexts of the three other calls are untouched by the switch. */
int sqphip_nlp_attach_data(sqphip_ctx *ctx, int64_t nterms, const int64_t *trow, const double *tcoef,
                           const int64_t *tptr /* [nterms + 1] factors of a term */,
                           const int64_t *aptr /* [nfac + 1] arguments of a factor */,
                           const int64_t *avar /* [nargs] 1-based */, const double *acoef /* [nargs] or NULL: ones */,
                           const int32_t *fkind, const int32_t *fexp,
                           const double *fpar /* [nfac] or NULL: real exponent, read for POWR only */,
                           const double *fshift /* [nfac] or NULL: zeros */, const double *g0 /* [m] or NULL */, double f0);
/* The data of one instance of such a context: fshift [nfac], acoef [nargs], fpar [nfac] in the order of the attach; any
 * pointer may be NULL: keep.  SQPHIP_EINVAL with a message in sqphip_last_error on a context without
 * sqphip_nlp_attach_data (the message names that call), inst out of range, fpar on a model without a POWR factor, a real
 * exponent of a POWR factor that is 0 or not finite (1-based term and factor named) and data that would leave the single
 * factor of a term of rows 1..num_linear with a coefficient other than 1 or a shift other than 0 (term named).  A zero
 * coefficient is allowed anywhere else: the structure, and with it every plan entry, stays.  Only the real exponents are
 * checked for finiteness: a NaN or infinite coefficient or shift is taken as given, as the attach calls take it.  Domain
 * stays the caller's business. */
int sqphip_nlp_set_instance_data(sqphip_ctx *ctx, int32_t inst, const double *fshift, const double *acoef,
                                 const double *fpar);
/* Dense data blocks of the objective of an NLP context: block k adds
 *     sum_{i < N} W[i] kappa(sum_{j < d} A[i][j] x_{cols[j]} + S[i])
 * to row 0, kappa of the menu of sqphip_nlp_attach_general (kind 0..10; exp for POW, par for POWR), A a dense row-major
 * N x d design matrix.  A, cols and the kind are shared by the batch; the weights W and shifts S belong to the instance
 * (folds: 0 / 1 weights, bootstrap resamples: integer weights, measurements: shifts).  Limits: 1 <= d <= 128 distinct
 * 1-based columns in any order, N >= 1, N d < 2^31, at most 4 blocks per context; a plain linear block (POW, e = 1) is
 * refused -- that is what terms are for.  Domain (LOG, SQRT, POWR, negative powers) is the caller's business.
 * Valid after any sqphip_nlp_attach* call and before the first sqphip_sqp_reset, sqphip_sqp_run or
 * sqphip_nlp_stream_begin of the context (SQPHIP_ESTATE after).  The call re-lays the instances' blocks of doubles and keeps
 * what they hold,
 *     f0 | g0 | c | [b | a | p] | W_0 [N_0] | S_0 [N_0] | W_1 | S_1 | ...        (padded to an even count)
 * fills W and S of every instance with weight and shift, uploads A once and maps every lower entry (r, c) of the block's
 * d x d Hessian to its COO slot (the first COO copy of an entry owns it, as for the plans).  Unless nnzH = 0 the Hessian
 * COO of sqphip_create must hold the lower entry of every pair of block columns, the diagonal included.
 * SQPHIP_EINVAL, with sqphip_last_error naming the block and the 1-based column or entry: a context without an NLP attach,
 * d outside 1..128, N < 1 or N d too large, a fifth block, a column out of range or twice, an unknown kind, POW with
 * e = 1, e = 0 or |e| > 32, POWR with par zero or not finite, a missing Hessian entry.
 * Evaluation, per block in block order, behind the plan passes of the terms (one workgroup per instance):
 *   points    u_i = 0, u_i = fma(A[i][j], x_cols[j], u_i) for j = 0 .. d - 1, u_i += S[i] (the rule of
 *             sqphip_nlp_attach_affine), then kappa, kappa', kappa'' by the code of the factors;
 *   f         thread t sums W[i] kappa_i over i = t, t + 1024, ..., a wave adds its 64 sums by the xor butterfly
 *             32, 16, .. 1, thread 0 adds the 16 wave sums in wave order, and the result is added to f;
 *   gradient  column j: lane l of its wave sums (W[i] kappa'_i) A[i][j] over i = l, l + 64, ..., the same butterfly, added
 *             to grad[cols[j]];
 *   Hessian   A' diag(W kappa'') A by lower 16 x 16 tiles on v_mfma_f64_16x16x4_f64, four points per instruction in
 *             rising order, operands (W[i] kappa''_i) A[i][r] (one rounding) and A[i][c], ragged edges as zeros; sigma
 *             times the entry is added to its COO slot by one thread.
 * No atomics: results are bit-reproducible and independent of slot, neighbours and instance groups.  They are not the
 * bits of the same model written as one term per point (the sums run in another order).  Every other entry point sees
 * an NLP context as before, and a context without a block files the bits it filed before this call existed. */
int sqphip_nlp_add_block(sqphip_ctx *ctx, int32_t kind, int32_t exp, double par, int64_t N, int32_t d,
                         const int64_t *cols /* [d] 1-based */, const double *A /* [N][d] row-major */,
                         const double *shift /* [N] or NULL: zeros */, const double *weight /* [N] or NULL: ones */,
                         int32_t *blk_out /* 0-based block number, or NULL */);
/* weight [N], shift [N] (a softmax block: [Kf][N]) of block blk of one instance; NULL: keep.  SQPHIP_EINVAL for inst or blk
 * out of range. */
int sqphip_nlp_set_instance_block(sqphip_ctx *ctx, int32_t inst, int32_t blk, const double *weight, const double *shift);
/* Multinomial (softmax) data blocks of the objective of an NLP context: the block adds
 *     sum_{i < N} W[i] [ log sum_{k < K} exp(u_ik) - u_{i, labels[i]} ],   u_ik = sum_{j < d} A[i][j] x_{cols[k][j]} + S[k][i]
 * to row 0: K-class logistic regression on a dense row-major N x d design matrix A.  A, cols, the labels (0-based, < K) and
 * K are shared by the batch; the weights W [N] (folds, resamples) and the per-class offsets S [Kf][N] (prior correction,
 * stage-wise fitting) belong to the instance.  pinned = 1: the last class has no variables and u_{i, K - 1} = 0 (the
 * identifiable form), Kf = K - 1; pinned = 0: Kf = K.  Limits: 2 <= K <= 64, d >= 1, Kf d <= 128, N >= 1, N d < 2^31; the Kf d
 * columns are distinct and 1-based, in any order.  Softmax blocks count among the four blocks of a context and are evaluated
 * in block order with the blocks of sqphip_nlp_add_block, behind the same barrier.  With q = k d + j and the softmax
 * probabilities p_ik: gradient g_q = sum_i W[i] (p_ik - [labels[i] = k]) A[i][j], Hessian
 * H_qq' = sum_i W[i] p_ik ([k = l] - p_il) A[i][j] A[i][j'] (q' = l d + j').
 * State rules and re-lay as for sqphip_nlp_add_block (SQPHIP_ESTATE once the layout is final); the instance's block grows by
 *     W [N] | S [Kf N]                                                            (padded to an even count)
 * sqphip_nlp_set_instance_block and sqphip_nlp_stream_set_block serve the block unchanged, with a shift array of Kf N entries.
 * Unless nnzH = 0 the Hessian COO of sqphip_create must hold the lower entry of every pair of the block's Kf d columns.
 * SQPHIP_EINVAL, with sqphip_last_error naming the block and the 1-based column, entry or point: a context without an NLP
 * attach, K outside 2..64, d < 1, Kf d > 128, N < 1 or N d too large, a fifth block, a column out of range or twice anywhere
 * in the block, a label outside 0..K-1, null cols, A or labels, a missing Hessian entry.
 * Evaluation (one workgroup per instance; every sum in an order that depends on N, d, K and pinned only, no atomics):
 *   points    u_ik = 0, u_ik = fma(A[i][j], x_cols[k][j], u_ik) for j = 0 .. d - 1, u_ik += S[k][i]; m = max_k u_ik (the pinned
 *             class enters with 0); e_k = exp(u_ik - m), s = sum of e_k for k = 0 .. Kf - 1 in that order, then exp(0 - m) of
 *             the pinned class; lse = m + log(s); p_ik = e_k / s.  u_ik - m <= 0 and s >= 1: logits of +-800 give finite
 *             results;
 *   f         thread t sums W[i] (lse_i - u_{i, labels[i]}) over i = t, t + 1024, ..., a wave adds its 64 sums by the xor
 *             butterfly 32, 16, .. 1, thread 0 adds the 16 wave sums in wave order, and the result is added to f;
 *   gradient  entry q: lane l of its wave sums (W[i] (p_ik - [labels[i] = k])) A[i][j] over i = l, l + 64, ..., the same
 *             butterfly, added to grad[cols[k][j]];
 *   Hessian   lower 16 x 16 tiles of the Kf d x Kf d matrix on v_mfma_f64_16x16x4_f64, four points per instruction in rising
 *             order, two accumulator chains with the shared operand (W[i] p_ik) A[i][j] (two roundings) against
 *             (-p_il) A[i][j'] (one rounding) and against A[i][j']; the second chain counts for the entries with k = l only
 *             and is skipped for a tile without any; ragged edges as zeros; sigma times (chain 1 + [k = l] chain 2) is added
 *             to the entry's COO slot by one thread.
 * Results are bit-reproducible and independent of slot, neighbours and instance groups.  A context without a softmax
 * block files the bits it filed before this call existed. */
int sqphip_nlp_add_softmax_block(sqphip_ctx *ctx, int64_t N, int32_t d, int32_t K, int32_t pinned,
                                 const int64_t *cols /* [Kf][d] 1-based */, const double *A /* [N][d] row-major */,
                                 const int32_t *labels /* [N] 0-based */, const double *shift /* [Kf][N] or NULL: zeros */,
                                 const double *weight /* [N] or NULL: ones */, int32_t *blk_out /* 0-based block number, or NULL */);
/* Cox partial-likelihood data blocks of the objective of an NLP context (survival data, Breslow ties): the block adds
 *     sum_{i < N} c_i [ log( sum_{j < risk[i]} W[j] exp(u_j) ) - u_i ],   u_i = sum_{j < d} A[i][j] x_{cols[j]} + S[i],   c_i = W[i] event[i]
 * to row 0.  The points are given sorted by non-increasing time, so the risk set of point i is the risk[i] leading points:
 * i + 1 <= risk[i] <= N (i 0-based), non-decreasing in i, one value per tie group.  event[i] >= 0 is the event indicator (0: a
 * censored point).  A, cols, risk and event are shared by the batch; the weights W [N] (0 / 1 for folds, integers for
 * resamples) and the offsets S [N] belong to the instance.  A point with c_i = 0 contributes exactly 0 and its logarithm is
 * never formed; W[j] = 0 removes point j from every risk set, so a fold is the Cox fit on the subset and an integer weight is a
 * replicated point.  W >= 0 is the caller's business.  Limits: 1 <= d <= 128 distinct 1-based columns in any order, N >= 1,
 * N d < 2^31.  Cox blocks count among the four blocks of a context and are evaluated in block order with the others, behind
 * the same barrier.  With m = max_i u_i, e_j = W[j] exp(u_j - m), T_i = sum_{j < risk[i]} e_j, q_i = c_i / T_i (0 where
 * c_i = 0) and Q_j = sum_{i : risk[i] > j} q_i:
 *     f = sum_i c_i (m + log T_i - u_i),   gradient A'(e o Q - c),
 *     Hessian A' diag(e o Q) A - sum_i (c_i / T_i^2) m_i m_i',   m_i = sum_{j < risk[i]} e_j A[j][.]
 * State rules and re-lay as for sqphip_nlp_add_block (SQPHIP_ESTATE once the layout is final); the instance's block grows by
 *     W [N] | S [N]                                                               (padded to an even count)
 * and its workspace by 6 N + N d doubles (u, e, the running sums of e, q, -q, 1 / T and the N x d running sums P of e_j A[j][.]).
 * sqphip_nlp_set_instance_block and sqphip_nlp_stream_set_block serve the block unchanged (weight [N], shift [N]);
 * sqphip_nlp_stream_set restores the data of this call.
 * Unless nnzH = 0 the Hessian COO of sqphip_create must hold the lower entry of every pair of block columns, the diagonal
 * included.
 * SQPHIP_EINVAL, with sqphip_last_error naming the block and the 1-based column, entry or point: a context without an NLP
 * attach, d outside 1..128, N < 1 or N d too large, a fifth block, null cols, A, risk or event, risk[i] outside i + 1 .. N,
 * risk decreasing, an event that is negative or not finite, a column out of range or twice, a missing Hessian entry.
 * Evaluation (one workgroup per instance; every sum in an order that depends on N, d and risk only, no atomics):
 *   points    u_i = 0, u_i = fma(A[i][j], x_cols[j], u_i) for j = 0 .. d - 1, u_i += S[i]; m by a maximum over the workgroup;
 *             e_i = W[i] exp(u_i - m);
 *   scans     one wave per scan, chunks of 64 points in rising order: within a chunk lane l adds the value of lane l - o for
 *             o = 1, 2, .. 32, then the carry of the chunks before, and lane 63's sum becomes the next carry.  The running sums
 *             of e give T_i = (sum up to point risk[i] - 1); those of e_k A[k][c] (one rounding) give column c of P; q is
 *             scanned from the last point down and Q_j is that sum at the first point i with risk[i] > j;
 *   f         thread t sums c_i ((m + log T_i) - u_i) over the i = t, t + 1024, ... with c_i != 0, a wave adds its 64 sums by
 *             the xor butterfly 32, 16, .. 1, thread 0 adds the 16 wave sums in wave order, and the result is added to f.  A
 *             call for f alone (the Armijo probe) forms u, m, e and T and nothing else;
 *   gradient  column j: lane l of its wave sums (e_i Q_i - c_i) A[i][j] over i = l, l + 64, ..., the same butterfly, added to
 *             grad[cols[j]];
 *   Hessian   lower 16 x 16 tiles on v_mfma_f64_16x16x4_f64, four points per instruction in rising order, two accumulator
 *             chains: (e_p Q_p) A[p][r] against A[p][c], and (-q_p) P[risk[p] - 1][r] against P[risk[p] - 1][c] (1 / T_p) -- the factor
 *             -c_p / T_p^2 split between the operands, since T^2 underflows for logits 350 below the maximum; ragged
 *             edges as zeros; sigma times (chain 1 + chain 2) is added to the entry's COO slot by one thread.  The two parts are
 *             separate sums; their difference is a covariance and cancels, and the error bound (tests/nlp_cox_ref.py) is that
 *             of their magnitudes added.
 * Domain: a point whose u_j lies more than about 700 below max u underflows to e_j = 0, and a risk set made of such points
 * alone has T = 0: the caller's business.  Results are bit-reproducible and independent of slot, neighbours and instance
 * groups.  A context without a Cox block files the bits it filed before this call existed. */
int sqphip_nlp_add_cox_block(sqphip_ctx *ctx, int64_t N, int32_t d, const int64_t *cols /* [d] 1-based */,
                             const double *A /* [N][d] row-major, points by non-increasing time */,
                             const int32_t *risk /* [N] leading points in the risk set */, const double *event /* [N] >= 0 */,
                             const double *shift /* [N] or NULL: zeros */, const double *weight /* [N] or NULL: ones */,
                             int32_t *blk_out /* 0-based block number, or NULL */);
/* Log-sum-exp row blocks of an NLP context (geometric programmes in convex form, smooth maxima of affine functions, entropic
 * risk): output r owns the consecutive points seg[r] .. seg[r + 1] - 1 (0-based; seg[0] = 0, seg[R] = N, every segment at
 * least one point) and adds
 *     lse_r = log( sum_{i in segment r} W[i] exp(u_i) ),   u_i = sum_{j < d} A[i][j] x_{cols[j]} + S[i]
 * to row rows[r]; row 0 is the objective (it may be absent), row i >= 1 a nonlinear constraint row (i > num_linear); the rows are
 * distinct.  A posynomial sum_k c_k prod_j y_j^{a_kj} in the variables x = log y is one output with A = (a_kj) and S = log c.
 * A, cols, seg and rows are shared by the batch; the weights W [N] >= 0 and the shifts S [N] (the log-coefficients of the
 * monomials) belong to the instance.  W[i] = 0 removes monomial i: it contributes exactly 0 whatever its logit, and its
 * exponential is never multiplied in.  W >= 0 is the caller's business.  Limits: 1 <= d <= 128 distinct 1-based columns in any
 * order, N >= 1, N d < 2^31, 1 <= R <= N, R d < 2^31 -- R is not capped otherwise: rows, seg, the output of every point and the
 * Jacobian slots live in uploaded arrays.  The block counts among the four blocks of a context and is evaluated in block order
 * with the others, behind the same barrier.  With m_r the largest u_i over the points of segment r with W[i] != 0,
 * e_i = W[i] exp(u_i - m_r), T_r = sum e_i, p_i = e_i / T_r and mu_r = sigma on row 0, lambda[row - 1] elsewhere:
 *     value m_r + log T_r,   Jacobian row G[r] = A_r' p,   Hessian of the Lagrangian sum_r mu_r (A_r' diag(p) A_r - G[r] G[r]').
 * State rules and re-lay as for sqphip_nlp_add_block (SQPHIP_ESTATE once the layout is final); the instance's block grows by
 *     W [N] | S [N]                                                               (padded to an even count)
 * and its workspace by 2 N + 2 R + R d doubles (u then p, e then z = mu p, m, T, G).
 * sqphip_nlp_set_instance_block and sqphip_nlp_stream_set_block serve the block unchanged (weight [N], shift [N]);
 * sqphip_nlp_stream_set restores the data of this call.
 * The Jacobian COO of sqphip_create must hold (rows[r], cols[j]) for every output on a row >= 1 and every column; unless
 * nnzH = 0 the Hessian COO must hold the lower entry of every pair of block columns, the diagonal included.  Where the COO
 * repeats an entry the first copy owns the slot and the others read 0.
 * SQPHIP_EINVAL, with sqphip_last_error naming the block and the 1-based output, column, entry or point: a context without an
 * NLP attach, d outside 1..128, N < 1 or N d too large, a fifth block, null cols or A, R outside 1..N or R d too large, null
 * rows or seg, seg[0] != 0, seg[R] != N, an empty or decreasing segment, a column out of range or twice, a missing Hessian
 * entry, a row outside 0..m, a row twice, a row among 1..num_linear, a missing Jacobian entry.
 * Evaluation (one workgroup per instance; every sum in an order that depends on N, d and seg only, no atomics):
 *   logits    u_i = 0, u_i = fma(A[i][j], x_cols[j], u_i) for j = 0 .. d - 1, u_i += S[i];
 *   maxima    wave w owns the outputs w, w + 16, ...: lane l takes the largest u_i over i = seg[r] + l, + 64, ... with W[i] != 0,
 *             then the xor butterfly 32, 16, .. 1;
 *   sums      e_i = W[i] exp(u_i - m_r), exactly 0 where W[i] = 0; the same wave sums e_i per lane in rising order, then the
 *             butterfly, and adds m_r + log T_r to f (row 0) or to g[row - 1].  A call for values alone (the Armijo probe) ends
 *             here;
 *   Jacobian  p_i = e_i / T_r; the pairs (r, j), numbered r d + j, are dealt to the sixteen waves: lane l sums p_i A[i][j] over
 *             i = seg[r] + l, + 64, ..., the butterfly, G[r][j] is kept and added to grad[cols[j]] (row 0) or to the Jacobian
 *             slot of (rows[r], cols[j]);
 *   Hessian   lower 16 x 16 tiles on v_mfma_f64_16x16x4_f64, two accumulator chains: four points per instruction in rising
 *             order, (mu_r p_i) A[i][r'] against A[i][c'] (z = mu p and the product: one rounding each), and four outputs per
 *             instruction in rising order, (-mu_r) G[r][r'] against G[r][c']; ragged edges as zeros; chain 1 + chain 2 is added
 *             to the entry's COO slot by one thread.  The two parts are separate sums; their difference is a covariance and
 *             cancels, and the error bound (tests/nlp_lse_ref.py) is that of their magnitudes added.
 * Domain: an output whose points all have weight 0, or whose weighted points all underflow, has T = 0: the caller's business.
 * Logits 300 either side of the middle of a segment give finite results.  Results are bit-reproducible and independent of slot,
 * neighbours and instance groups.  A context without such a block files the bits it filed before this call existed. */
int sqphip_nlp_add_lse_block(sqphip_ctx *ctx, int64_t N, int32_t d, const int64_t *cols /* [d] 1-based */,
                             const double *A /* [N][d] row-major */, int32_t R, const int64_t *rows /* [R] */,
                             const int64_t *seg /* [R + 1] */, const double *shift /* [N] or NULL: zeros */,
                             const double *weight /* [N] or NULL: ones */, int32_t *blk_out /* 0-based block number, or NULL */);
/* Euclidean-norm row blocks of an NLP context (second-order-cone rows a'x + kappa |P x| <= b, chance constraints, risk budgets;
 * sums of norms in the objective: Fermat-Weber location, group lasso, total variation, robust least squares): output r owns the
 * consecutive points seg[r] .. seg[r + 1] - 1 (0-based; seg[0] = 0, seg[R] = N, every segment at least one point) and adds
 *     f_r = sqrt( sum_{i in segment r} W[i] v_i^2 ),   v_i = sum_{j < d} A[i][j] x_{cols[j]} + S[i]
 * to row rows[r]; row 0 is the objective (it may be absent), row i >= 1 a nonlinear constraint row (i > num_linear).  Any number
 * of outputs may share a row, row 0 included: a sum of norms in the objective is several outputs on row 0.  The linear part of
 * a cone row stays in the terms of the same row.  A, cols, seg and rows are shared by the batch; the weights W [N] >= 0 and the
 * shifts S [N] belong to the instance.  A coefficient c_r > 0 on a norm goes into the weights of its points as c_r^2.  There is
 * no smoothing parameter: a point whose row of A is zero and whose shift is delta puts delta^2 under the root, per instance.
 * W[i] = 0 removes point i without a trace: its residual is never read into a maximum, a sum or a product and may be infinite or
 * NaN.  W >= 0 and finite residuals on weighted points are the caller's business.  Limits: 1 <= d <= 128 distinct 1-based
 * columns in any order, N >= 1, N d < 2^31, 1 <= R <= N, R d < 2^31.  The block counts among the four blocks of a context and
 * is evaluated in block order with the others, behind the same barrier.  With m_r the largest |v_i| over the points of segment r
 * with W[i] != 0, y_i = v_i / m_r, s_r = sum W[i] y_i^2 and mu_r = sigma on row 0, lambda[row - 1] elsewhere:
 *     value f_r = m_r sqrt(s_r),   q_i = W[i] y_i / sqrt(s_r),   Jacobian row G[r] = A_r' q,
 *     Hessian of the Lagrangian sum_r mu_r (A_r' diag(W / f_r) A_r - G[r] G[r]' / f_r).
 * Residuals of 1e+-200 give finite values and first derivatives.
 * The apex: an output with f_r = 0 -- all its weights zero, or all its weighted residuals exactly zero -- files the value 0,
 * which is exact for an unsmoothed norm, and contributes exactly nothing to gradient, Jacobian and Hessian (q = 0, z = 0, no
 * division by zero, no NaN).  That derivative is a choice of subgradient; a model that is to converge to an apex carries the
 * smoothing point.
 * State rules and re-lay as for sqphip_nlp_add_block (SQPHIP_ESTATE once the layout is final); the instance's block grows by
 *     W [N] | S [N]                                                               (padded to an even count)
 * and its workspace by 2 N + 2 R + R d doubles (v then q, z, m, F, G).
 * sqphip_nlp_set_instance_block and sqphip_nlp_stream_set_block serve the block unchanged (weight [N], shift [N]);
 * sqphip_nlp_stream_set restores the data of this call.
 * The Jacobian COO of sqphip_create must hold (rows[r], cols[j]) for every output on a row >= 1 and every column; unless
 * nnzH = 0 the Hessian COO must hold the lower entry of every pair of block columns, the diagonal included.  Where the COO
 * repeats an entry the first copy owns the slot and the others read 0.
 * SQPHIP_EINVAL, with sqphip_last_error naming the block and the 1-based output, column, entry or point: a context without an
 * NLP attach, d outside 1..128, N < 1 or N d too large, a fifth block, null cols or A, R outside 1..N or R d too large, null
 * rows or seg, seg[0] != 0, seg[R] != N, an empty or decreasing segment, a column out of range or twice, a missing Hessian
 * entry, a row outside 0..m, a row among 1..num_linear, a missing Jacobian entry.  A repeated row is accepted.
 * Evaluation (one workgroup per instance; every sum in an order that depends on N, d, seg and rows only, no atomics).  An output
 * of at most 64 points is short, any other long:
 *   residuals v_i = 0, v_i = fma(A[i][j], x_cols[j], v_i) for j = 0 .. d - 1, v_i += S[i];
 *   norms     a long output belongs to a wave: lane l takes the largest |v_i| over i = seg[r] + l, + 64, ... with W[i] != 0, the
 *             xor butterfly 32, 16, .. 1, then sums W[i] y_i^2 over the same points in rising order and the butterfly.  A short
 *             output belongs to one thread, which does both in rising i;
 *   values    one thread per distinct target row adds f_r over its outputs in rising r to f (row 0) or g[row - 1].  A call for
 *             values alone (the Armijo probe) ends here, with the bits of a full call;
 *   Jacobian  G[r][j] = sum q_i A[i][j]: for a long output by a wave per (r, j) as above, for a short one by one thread per
 *             (r, j) in rising i; then one thread per (target row, j) adds G[r][j] over the row's outputs in rising r to
 *             grad[cols[j]] (row 0) or to the Jacobian slot of (row, cols[j]);
 *   Hessian   lower 16 x 16 tiles on v_mfma_f64_16x16x4_f64, two accumulator chains: four points per instruction in rising
 *             order, (mu_r W[i] / f_r) A[i][r'] against A[i][c'], and four outputs per instruction in rising order,
 *             (-mu_r / f_r) G[r][r'] against G[r][c']; ragged edges as zeros; chain 1 + chain 2 is added to the entry's COO slot by
 *             one thread.  The two parts are separate sums; their difference cancels, and the error bound
 *             (tests/nlp_norm_ref.py) is that of their magnitudes added.
 * Results are bit-reproducible and independent of slot, neighbours and instance groups.  A context without such a block files
 * the bits it filed before this call existed. */
int sqphip_nlp_add_norm_block(sqphip_ctx *ctx, int64_t N, int32_t d, const int64_t *cols /* [d] 1-based */,
                              const double *A /* [N][d] row-major */, int32_t R, const int64_t *rows /* [R], may repeat */,
                              const int64_t *seg /* [R + 1] */, const double *shift /* [N] or NULL: zeros */,
                              const double *weight /* [N] or NULL: ones */, int32_t *blk_out /* 0-based block number, or NULL */);
/* Dense data blocks with several outputs: one design matrix, R weight vectors, a target row each.  Output r adds
 *     sum_{i < N} W[r][i] kappa(sum_{j < d} A[i][j] x_{cols[j]} + S[i])
 * to row rows[r]; row 0 is the objective, row i >= 1 a nonlinear constraint row (i > num_linear).  Constraints on the data the
 * objective is fitted to: a mean loss of one class below a level (Neyman-Pearson), a calibration or parity equality, an
 * entropic-risk budget, moment constraints.  Kinds, exp, par and the limits on d (1..128), N and N d are those of
 * sqphip_nlp_add_block; 1 <= R <= 8, the rows are distinct.  A, cols, the kind, rows and R are shared by the batch; W [R][N]
 * and S [N] belong to the instance.  The block counts among the four blocks of a context and is evaluated in block order with
 * the others, behind the same barrier.
 * State rules and re-lay as for sqphip_nlp_add_block (SQPHIP_ESTATE once the layout is final); the instance's block grows by
 *     W [R][N] | S [N]                                                            (padded to an even count)
 * sqphip_nlp_set_instance_block and sqphip_nlp_stream_set_block serve the block with a weight array of R N entries;
 * sqphip_nlp_stream_set restores the data of this call.
 * The Jacobian COO of sqphip_create must hold (i, cols[j]) for every target row i >= 1 and every column; unless nnzH = 0 the
 * Hessian COO must hold the lower entry of every pair of columns.  The first COO copy of a slot owns it.
 * SQPHIP_EINVAL, with sqphip_last_error naming the block and the 1-based output, column or entry: everything
 * sqphip_nlp_add_block refuses, R outside 1..8, null rows, a row outside 0..m, a row twice, a row in 1..num_linear, a missing
 * Jacobian entry (row and column named).
 * Evaluation (one workgroup per instance; every sum in an order that depends on N, d and R only, no atomics):
 *   points    u_i as in sqphip_nlp_add_block; kappa, kappa', kappa'' once per point;
 *   values    output r: thread t sums W[r][i] kappa_i over i = t, t + 1024, ..., the xor butterfly 32 .. 1 within a wave,
 *             thread 0 adds the 16 wave sums in wave order; the result is added to f (row 0) or g[row - 1];
 *   first derivatives  the pairs (r, j), numbered r d + j, are dealt to the waves; lane l sums (W[r][i] kappa'_i) A[i][j] over
 *             i = l, l + 64, ..., the same butterfly, added to grad[cols[j]] (row 0) or the Jacobian slot of (rows[r], cols[j]);
 *   Hessian   e_i = 0, e_i = fma(mu_r, W[r][i], e_i) for r = 0 .. R - 1, mu_r = sigma (row 0) or lambda[row - 1];
 *             z_i = e_i kappa''_i; then the lower 16 x 16 tiles of sqphip_nlp_add_block with the operand z_p A[p][r] (one
 *             rounding), and the sum is added as it is to the entry's COO slot: one MFMA pass whatever R is.
 * Results are bit-reproducible and independent of slot, neighbours and instance groups.  A context without such a block
 * files the bits it filed before this call existed; a block with R = 1 on row 0 need not file the bits of
 * sqphip_nlp_add_block (the Hessian weight enters in another place). */
int sqphip_nlp_add_row_block(sqphip_ctx *ctx, int32_t kind, int32_t exp, double par, int64_t N, int32_t d,
                             const int64_t *cols /* [d] 1-based */, const double *A /* [N][d] row-major */,
                             int32_t R, const int64_t *rows /* [R] 0: objective, i: row i */,
                             const double *shift /* [N] or NULL: zeros */,
                             const double *weight /* [R][N] or NULL: ones */, int32_t *blk_out);
/* Per-instance values (f0 one value, g0 [m], tcoef [nterms] in the term order of the attach) and the start x0 [n];
 * any pointer may be NULL: keep.  Bounds go through sqphip_set_bounds. */
int sqphip_nlp_set_instance(sqphip_ctx *ctx, int32_t inst, const double *f0, const double *g0,
                            const double *tcoef, const double *x0);   /* NULL: keep; bounds via sqphip_set_bounds */
/* Run SQP-TR for every instance until each has terminated or done `max_outer` more outer
 * iterations (0 = no cap beyond options.max_iter).  Restartable: state stays on the device. */
int sqphip_sqp_reset(sqphip_ctx *ctx);
int sqphip_sqp_run(sqphip_ctx *ctx, int32_t max_outer);
/* results per instance (src/model.jl result slots as written by sqp_trust_region.jl:215-222);
 * any pointer may be NULL */
/* Scenario queue: more scenarios than the context has slots (contingency screening).  A slot whose run has terminated
 * files its result under its scenario id, takes the next id from a device-wide counter, loads that scenario from tables
 * in HBM and starts over -- inside the kernels of the running sweep, without the host -- so the batch stays full until
 * the queue is empty and no slot waits for the slowest run of a batch (no reference counterpart; SURVEY.md section
 * 8f-4, load re-balancing of stragglers).  Which slot solves which scenario depends on timing, the result of a
 * scenario does not.  _begin allocates tables for n_scenarios; _set uploads one scenario (the arguments of
 * sqphip_set_bounds and sqphip_acopf_set_instance); _run solves them all; _get returns one result (final point,
 * objective, status as src/status.jl, iterations; iterations = -1: this context has filed no result for the scenario since
 * the last _stream_run / _stream_assign -- another rank solved it, or it is still waiting or in progress). */
int sqphip_sqp_stream_begin(sqphip_ctx *ctx, int32_t n_scenarios);
int sqphip_sqp_stream_set(sqphip_ctx *ctx, int32_t scenario, const double *xL, const double *xU, const double *gL,
                          const double *gU, const double *ohm, const double *c2, const double *c1, const double *x0);
int sqphip_sqp_stream_run(sqphip_ctx *ctx);
/* A queue shared between ranks (multi-GPU screening): every rank uploads the tables of ALL
 * scenarios (_begin with the total, _set for each) but hands out only the ids assigned to it (_assign: ids in hand-out
 * order).  _run_some lets every slot perform up to max_outer more outer iterations and reports how many ids of this
 * rank's queue nobody has drawn yet and how many slots have a run in progress; between such runs the host may take
 * unstarted ids off the tail of a rank's queue (_release) and hand them to a rank whose queue ran dry (_append) --
 * sqpsolver.jl_amd/shard.py run_shared_queue does that with one small host-side exchange per round.  No iterate crosses
 * ranks, and the result of a scenario does not depend on the rank or slot that solved it. */
int sqphip_sqp_stream_assign(sqphip_ctx *ctx, int32_t n, const int32_t *ids);
int sqphip_sqp_stream_append(sqphip_ctx *ctx, int32_t n, const int32_t *ids);
int sqphip_sqp_stream_release(sqphip_ctx *ctx, int32_t n, int32_t *ids_out, int32_t *n_out);
int sqphip_sqp_stream_run_some(sqphip_ctx *ctx, int32_t max_outer, int32_t *n_unstarted, int32_t *n_active);
int sqphip_sqp_stream_get(sqphip_ctx *ctx, int32_t scenario, double *x, double *obj_val, int32_t *status, int32_t *iter);
/* The queue of a QCQP context (sqphip_qcqp_attach): one structure, many coefficient sets, more scenarios than slots.
 * _run, _run_some, _assign, _append, _release and _get above work on it unchanged; a slot loads a scenario by one
 * streaming copy of its block of values into the slot's own (the layout of sqphip_qcqp_set_instance).
 * tables for n_scenarios on a QCQP context; keep_multipliers = 1 also allocates result tables for g, mult_g,
 * mult_x_L, mult_x_U.  SQPHIP_EINVAL on a context without sqphip_qcqp_attach. */
int sqphip_qcqp_stream_begin(sqphip_ctx *ctx, int32_t n_scenarios, int32_t keep_multipliers);
/* one scenario: bounds as sqphip_set_bounds, values in the term order of the attach as sqphip_qcqp_set_instance,
 * start x0.  A NULL value part means "the values given to sqphip_qcqp_attach" (not what an instance holds now); NULL
 * bounds mean the bounds given to sqphip_create; NULL x0 is refused.  SQPHIP_EINVAL, sqphip_last_error naming the row
 * (0-based), for a row unbounded on both sides and, with options.kkt_condense = 1, for an equality row that was not
 * one at sqphip_create. */
int sqphip_qcqp_stream_set(sqphip_ctx *ctx, int32_t scenario, const double *xL, const double *xU, const double *gL,
                           const double *gU, const double *f0, const double *c, const double *q0v, const double *g0,
                           const double *av, const double *qv, const double *x0);
/* The queue of a factorable-NLP context (sqphip_nlp_attach): the same, for any sparse factorable NLP.  _run, _run_some,
 * _assign, _append, _release and _get above work on it unchanged; a slot loads a scenario by one streaming copy of its
 * block of values (f0 | g0 | c, after sqphip_nlp_attach_data | b | a | p, padded to an even count) into the slot's own.
 * tables for n_scenarios on an NLP context; keep_multipliers = 1 also allocates result tables for g, mult_g, mult_x_L,
 * mult_x_U.  SQPHIP_EINVAL on a context without sqphip_nlp_attach (unattached, ACOPF, dense, QCQP) and for
 * n_scenarios <= 0. */
int sqphip_nlp_stream_begin(sqphip_ctx *ctx, int32_t n_scenarios, int32_t keep_multipliers);
/* one scenario: bounds as sqphip_set_bounds, values as sqphip_nlp_set_instance (f0 one value, g0 [m], tcoef [nterms] in
 * the term order of the attach), start x0.  A NULL value part means "the value given to sqphip_nlp_attach" (not what an
 * instance holds now); NULL bounds mean the bounds given to sqphip_create; NULL x0 is refused.  SQPHIP_EINVAL,
 * sqphip_last_error naming the scenario or the row (0-based), for a scenario outside the queue, a row unbounded on both
 * sides and, with options.kkt_condense = 1, an equality row that was not one at sqphip_create; before
 * sqphip_nlp_stream_begin the call is refused too. */
int sqphip_nlp_stream_set(sqphip_ctx *ctx, int32_t scenario, const double *xL, const double *xU, const double *gL,
                          const double *gU, const double *f0, const double *g0, const double *tcoef, const double *x0);
/* The data of one scenario of the queue of a context of sqphip_nlp_attach_data: overlays the b | a | p segments of the
 * scenario's block in the tables (the blocks there have the layout of that attach; every queue call works on the longer
 * block unchanged).  sqphip_nlp_stream_set writes the whole block, data of the attach included, so the order is
 * sqphip_nlp_stream_set, then this call; a later sqphip_nlp_stream_set restores the attach's data.  NULL: keep.  Refused
 * with SQPHIP_EINVAL and a message on a context without sqphip_nlp_attach_data, before sqphip_nlp_stream_begin, for a
 * scenario outside the queue and for the values sqphip_nlp_set_instance_data refuses. */
int sqphip_nlp_stream_set_data(sqphip_ctx *ctx, int32_t scenario, const double *fshift, const double *acoef,
                               const double *fpar);
/* weight / shift of block blk of one scenario of the queue (sqphip_nlp_add_block): overlays the table entry.
 * sqphip_nlp_stream_set writes the whole block with the add-call's weights and shifts, so the order is
 * sqphip_nlp_stream_set, then this call; a later sqphip_nlp_stream_set restores the add-call's.  NULL: keep.  SQPHIP_EINVAL
 * before sqphip_nlp_stream_begin, for a scenario outside the queue and for a blk the context does not have. */
int sqphip_nlp_stream_set_block(sqphip_ctx *ctx, int32_t scenario, int32_t blk, const double *weight, const double *shift);
/* everything sqphip_sqp_get returns, for a scenario of a queue begun with keep_multipliers = 1 (same signs as
 * sqphip_sqp_get: mult_g = -lambda, mult_x_U negated; any pointer may be NULL): the slot files them with the final
 * point before it draws its next scenario.  SQPHIP_ESTATE when the tables were not asked for (sqphip_qcqp_stream_begin
 * or sqphip_nlp_stream_begin with keep_multipliers = 0, or the ACOPF queue). */
int sqphip_sqp_stream_get_full(sqphip_ctx *ctx, int32_t scenario, double *x, double *g, double *mult_g,
                               double *mult_x_L, double *mult_x_U, double *obj_val, int32_t *status, int32_t *iter);
int sqphip_sqp_get(sqphip_ctx *ctx, int32_t inst, double *x, double *g, double *mult_g,
                   double *mult_x_L, double *mult_x_U, double *obj_val, int32_t *status,
                   int32_t *iter);
/* ret codes and iteration counts of the whole batch, device -> host (the arrays a host layer
 * all-gathers across ranks); done[i] = 1 once instance i has terminated */
int sqphip_sqp_status(sqphip_ctx *ctx, int32_t *ret_codes, int32_t *iters, int32_t *done);
/* ---- multi-GPU: the convergence-status gather --------------------------------------
 * Independent instances are cut into `world` contiguous blocks (sizes differing by at most one, rank r holding block r;
 * one process and one context per GPU, the context's batch = its block).  The only exchange between ranks is an
 * all-gather of int32 (ret, iter, done) per instance over RCCL on a communicator the library owns: rank 0 obtains the
 * 128-byte ncclUniqueId with sqphip_comm_unique_id and ships it to the other ranks by whatever channel the host has
 * (MPI, a file, torch.distributed, Julia's Distributed), every rank then calls sqphip_comm_init.  RCCL is loaded with
 * dlopen on the first of these calls; a context without a communicator returns the local table from
 * sqphip_gather_status, one with a communicator always runs the collective (also for world = 1).  `total` must be the
 * same on every rank of a call (the all-gather counts derive from it).  sqphip_comm_init is collective: call
 * sqphip_comm_available (1 = librccl loads in this process) on every rank and agree on the minimum before entering it.
 * Outputs: length `total`, ordered by global instance id; any may be NULL. */
int sqphip_comm_available(void);
int sqphip_comm_unique_id(void *id128);
int sqphip_comm_init(sqphip_ctx *ctx, const void *id128, int32_t world, int32_t rank);
int sqphip_gather_status(sqphip_ctx *ctx, int32_t total, int32_t *ret_codes, int32_t *iters, int32_t *done);
int sqphip_comm_destroy(sqphip_ctx *ctx);
/* per-instance trace rows (columns of the reference's log line, sqp_trust_region.jl:605-634):
 * rows[k*12 + {iter, accepted, fr, sub_status, ipm_iters, f, phi, mu, delta, |p|, inf_pr, inf_du}] */
int sqphip_sqp_trace(sqphip_ctx *ctx, int32_t inst, double *rows, int32_t cap, int32_t *len);

/* counters since create/reset: sub-problem solves, interior-point iterations, factorisations,
 * flops spent in LDL^T (N^3/3 each), seconds inside the factor kernels (HIP events) */
typedef struct {
    int64_t n_qp, n_ipm_iter, n_factor;
    double ldlt_flops, ldlt_seconds, trailing_seconds, solve_seconds, total_seconds;
    int64_t trailing_launches;
    int64_t kkt_order;       /* order of the matrices the LDL^T factorises (n + m, or the condensed order) */
    int64_t lead_tiles;      /* leading 64-column tiles treated as mutually independent (options.kkt_tile_order) */
    double trailing_flops_per_factor;   /* algorithmic flops of the k_trailing launches of one factorisation */
    /* sparse (multifrontal) solver; all zero when the dense one is in use */
    int64_t sparse;          /* 1: the Newton systems go through mfront.hip */
    int64_t nnz_k;           /* structural entries of the lower triangle of the factorised matrix, diagonal included */
    int64_t nnz_l;           /* entries of L below the diagonal as the fronts hold them (deterministic order of the library) */
    int64_t n_supernodes, n_levels, max_front;
    double factor_flops;     /* flops of one numeric factorisation of one instance (dense partial factorisations of the fronts) */
    int64_t front_doubles;   /* doubles of front storage per instance (L + contribution blocks + right-hand-side rows) */
    int64_t cb_doubles;      /* ... of which contribution blocks (written once by the child, read once by the parent) */
    int64_t factor_launches, solve_launches;   /* kernel launches of one factorisation / of one forward + backward solve */
    int64_t n_sweeps;        /* passes of the fixed kernel sequence (ipm_sweep) since create / reset: with continuous
                              * batching the slowest instance of the batch decides this number */
    int64_t n_solve;         /* forward + backward solves with the factors, summed over the instances (first solve of a
                              * factorisation, corrector, refinement steps) */
    int64_t n_groups;        /* instance groups of sqphip_sqp_run, each on its own HIP stream and host thread (1: none).
                              * n_sweeps and the kernel seconds are summed over the groups */
    int64_t nnz_l_top, nnz_k_top, cols_top;   /* the narrow top of the assembly tree (the fronts k_mf_solve_top2 streams): entries
                              * of L, structural entries of the matrix, columns -- the algorithmic bytes of the per-kernel records */
} sqphip_counters;
int sqphip_get_counters(sqphip_ctx *ctx, sqphip_counters *c);
/* The work of the batched run since sqphip_sqp_reset, split by sub-problem mode: out[3 k + 0..2] = sub-problems solved,
 * interior-point iterations, KKT factorisations of mode k = 0 QP (sub_optimize!, subproblem_JuMP.jl:127-183), 1 FR
 * (:352-393), 2 SOC (sqp_trust_region.jl:341-360), 3 linear phase (:264-304).  12 values. */
int sqphip_get_mode_counters(sqphip_ctx *ctx, int64_t *out12);
/* ... and per instance (arrays of length batch, any may be NULL): sub-problems, interior-point iterations and KKT
 * factorisations since sqphip_sqp_reset.  With continuous batching a call to sqphip_sqp_run lasts as long as its
 * busiest instance: max / mean of `factorisations` is the load imbalance of the batch. */
int sqphip_sqp_work(sqphip_ctx *ctx, int64_t *sub_problems, int64_t *ipm_iterations, int64_t *factorisations);
/* The last (up to 64) sub-problems of one instance in the order they finished: rows of four int32 (mode, MOI status,
 * interior-point iterations, factorisations); *n_rows receives the number written (cap: rows available in `rows`). */
int sqphip_sqp_qp_log(sqphip_ctx *ctx, int32_t inst, int32_t *rows, int32_t cap, int32_t *n_rows);
/* ... and for the same rows: the scaled optimality error each ended with and the rule that ended it (as
 * sqphip_qp_termination; either array may be NULL) */
int sqphip_sqp_qp_log_term(sqphip_ctx *ctx, int32_t inst, double *scaled_error, int32_t *rule, int32_t cap, int32_t *n_rows);
/* Sub-problems of the batched run since sqphip_sqp_reset by the way their interior-point run ended: out4[0] tolerance
 * reached, out4[1..3] acceptable-termination rule 1 / 2 / 3 (sqphip_qp_termination). */
int sqphip_get_termination_counters(sqphip_ctx *ctx, int64_t *out4);
/* Diagnostics: the sub-problem request instance `inst` of the batched run worked on last, in the argument convention of
 * sqphip_qp_solve (x_k[n], c[n], b[m], jac_coo[nnzJ], hess_coo[nnzH]; any pointer may be NULL), so that a sub-problem
 * seen on the device can be replayed through sqphip_qp_solve or another solver. */
int sqphip_sqp_last_request(sqphip_ctx *ctx, int32_t inst, int32_t *mode, double *delta, double *mu_pen, double *x_k,
                            double *c, double *b, double *jac_coo, double *hess_coo);
int sqphip_reset_counters(sqphip_ctx *ctx);
/* HIP-event timing of the factor / trailing-update / solve kernels (off by default); enabled = 2 additionally brackets every
 * launch group of a sweep by kernel class (about twenty more event records per sweep: meant for a short measurement leg) */
int sqphip_set_timing(sqphip_ctx *ctx, int32_t enabled);
/* ... the class timers (sparse path): seconds[c] of kernel time and groups[c] = launch groups timed, summed over the instance
 * groups, since sqphip_reset_counters; classes c = 0 values of the matrix entries (k_mf_values), 1 front kernels below the
 * narrow top of the assembly tree, 2 front kernels of the top (level launches, or k_mf_spine), 3 the top of the tree in
 * the solves (k_mf_solve_top2, with the inertia test), 4 level launches of the solves (k_mf_fwd2 / k_mf_bwd2), 5 the stage
 * kernel behind the solve (k_ipm_post: residual check, step, convergence test, next right-hand side), 6 transitions between
 * sub-problems (k_qp_finish, k_sqp_stage, k_ipm_head).  cap = length of both arrays (7 classes). */
int sqphip_get_kernel_times(sqphip_ctx *ctx, double *seconds, int64_t *groups, int32_t cap);

/* Test hooks and micro-benchmarks (host reference of the multifrontal plan, kernel-level twins, dense LDL^T probes) are
 * exported by the library but are not part of the drop-in boundary: include/sqphip_test_hooks.h. */

#ifdef __cplusplus
}
#endif
#endif
