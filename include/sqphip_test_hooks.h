/* sqphip_test_hooks.h -- entry points of libsqphip.so that exist for the parity tests and the micro-benchmarks only.
 * NOT part of the drop-in boundary (include/sqphip.h): no caller of the AbstractSubOptimizer seat needs them, and the
 * Julia shim binds none of them.  Kept in the shared library so that tests reach the kernels through the same C ABI. */
#ifndef SQPHIP_TEST_HOOKS_H
#define SQPHIP_TEST_HOOKS_H
#include "sqphip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Host-only test hook (no GPU, never on the product path): builds the multifrontal plan of the structure and runs a
 * plain host reference of its numeric phase -- assembly from the item lists, front-by-front partial LDL^T with the
 * right-hand side carried along, backward substitution -- on the Newton matrix
 *     [ hsc H + diag(hd + sigp + dw + 1e-8) + J_I' (D_I + 1e-8)^-1 J_I    J_K' ;  J_K   -(D_K + 1e-8) ]
 * (rows with rtype 0 are free: diagonal -1, no coupling).  Jval / Hval in the COO order of the structure; Dd, rtype
 * per row; sigp, hd per variable; rhs / sol / dinv_by_unknown in unknown order (variables, then kept rows);
 * npos = positive pivots.  CPU tests compare it with a dense solve to validate the plan the kernels run. */
int sqphip_mf_host_solve(int64_t n, int64_t m, int64_t nnzJ, const int64_t *jrow, const int64_t *jcol,
                         int64_t nnzH, const int64_t *hrow, const int64_t *hcol, const double *gL, const double *gU,
                         int32_t condense, const double *Jval, const double *Hval, const double *Dd,
                         const double *sigp, const double *hd, const int32_t *rtype, double hsc, double dw,
                         const double *rhs, double *sol, double *dinv_by_unknown, int32_t *npos);
/* After sqphip_mf_host_solve: relative error of the host replay of the streamed top-of-tree solve (k_mf_solve_top2) from
 * its own plan arrays against the plain recursion of the same call; -1 when the plan has no such top (a front of more than
 * 128 rows or 84 columns, or SQPHIP_MF_TOP2=0).  Not thread safe (one global). */
double sqphip_mf_host_top2_err(void);
/* ... and of the host replay of the spine kernel's front assembly (k_mf_spine: gather entries from the arena, the block the
 * previous front hands over through its row map, destination list) against the images the plain recursion assembled; -1
 * when the plan has no spine (a front of more than eight tiles near the top, or SQPHIP_MF_SPINE=0). */
double sqphip_mf_host_spine_err(void);
/* Device twin of sqphip_mf_host_solve (kernel-level parity tests): the same Newton matrix, assembled, factorised and
 * solved by the multifrontal kernels in instance `inst` of a context that uses the sparse solver (kkt_mode 2, or 0
 * where it selects it).  sol_fused: right-hand side carried through the factorisation; sol_standalone: the
 * stand-alone forward / backward kernels on the same factors.  Leaves the instance idle. */
int sqphip_mf_solve_test(sqphip_ctx *ctx, int32_t inst, const double *Jval, const double *Hval, const double *Dd,
                         const double *sigp, const double *hd, const int32_t *rtype, double hsc, double dw,
                         const double *rhs, double *sol_fused, double *sol_standalone, double *dinv_by_unknown);
/* Batched twin of sqphip_mf_solve_test: every instance with active[b] != 0 gets its own values and interior-point state
 * (Hessian scale, delta_w, last accepted delta_w, failed factorisations so far) and goes through one sweep's factorisation
 * (both candidate shifts, right-hand side fused in), inertia test (by the path the sweep takes) and backward solve; then the
 * stand-alone forward / backward solve of the same right-hand side.  Per-instance arrays back to back: Jval [B][nnzJ],
 * Hval [B][nnzH], Dd / rtype [B][m], sigp / hd [B][n], rhs and outputs [B][nu] in unknown order.  decision [B][5]: outcome
 * (0 idle, 1 another shift needed, 2 passed, 3 given up), sel, n_factor, fac_attempt and -- derived on the host from the
 * inputs by the rule of mf_speculates, not reported by the device -- whether the instance speculates; dw_out [B]: delta_w
 * after the decision.  dinv1: pivots of the second candidate (zero where the context keeps none).  Leaves every instance idle. */
int sqphip_mf_batch_test(sqphip_ctx *ctx, const int32_t *active, const double *Jval, const double *Hval, const double *Dd,
                         const double *sigp, const double *hd, const int32_t *rtype, const double *hsc, const double *dw,
                         const double *dw_last, const int32_t *fac_attempt, const double *rhs, double *sol_fused,
                         double *sol_standalone, double *dinv0, double *dinv1, int32_t *decision, double *dw_out);
/* The values launch of a sweep on its own (k_mf_values: the item-parallel kernel, or the one-thread-per-destination kernel
 * under SQPHIP_MF_VALUES_SERIAL=1 / for a plan without blocks): instances and interior-point states as in
 * sqphip_mf_batch_test.  vals0 / vals1 [B][nnzK]: the assembled values of the structural entries of both candidate shifts as
 * the device holds them after the launch; every slot is preset to `sentinel`, which is what an idle instance -- and candidate
 * 1 of an instance that does not speculate, or of a context without a second candidate -- comes back with.  *nnzK (may be
 * null): entries per instance; with vals0 and vals1 both null nothing else happens.  Leaves every instance idle. */
int sqphip_mf_values_test(sqphip_ctx *ctx, const int32_t *active, const double *Jval, const double *Hval, const double *Dd,
                          const double *sigp, const double *hd, const int32_t *rtype, const double *hsc, const double *dw,
                          const double *dw_last, const int32_t *fac_attempt, double sentinel, double *vals0, double *vals1,
                          int64_t *nnzK);
/* Host-only (no GPU): the blocks the item-parallel values kernel (k_mf_values) runs for the structure and condense option --
 * blocks[cap_blocks][4] = (first destination, first item, destinations, items); *n_blocks = 0: the plan has none (a
 * destination of more than 256 items) and the one-thread-per-destination kernel runs --, item_ptr[cap_dest + 1] (items of
 * destination e: [item_ptr[e], item_ptr[e + 1]); written when cap_dest >= *n_dest), and two host replays of the values
 * from the inputs of sqphip_mf_host_solve (vals_list / vals_block [*n_dest], written when not null and cap_dest >= *n_dest):
 * every destination summed in list order, and -- as the kernel does it -- block by block through a staging array of the
 * items' values, formed from the kernel's own item copy (vals_block is left alone when there are no blocks). */
int sqphip_mf_values_blocks(int64_t n, int64_t m, int64_t nnzJ, const int64_t *jrow, const int64_t *jcol, int64_t nnzH,
                            const int64_t *hrow, const int64_t *hcol, const double *gL, const double *gU, int32_t condense,
                            const double *Jval, const double *Hval, const double *Dd, const double *sigp, const double *hd,
                            const int32_t *rtype, double hsc, double dw, int32_t *blocks, int32_t cap_blocks,
                            int32_t *n_blocks, int32_t *item_ptr, int64_t cap_dest, int64_t *n_dest, int64_t *n_items,
                            double *vals_list, double *vals_block);
/* Host-only (no GPU): what sqphip_create sets up for the dense path (kkt_mode = 1, or 0 where it selects it) of the structure
 * under options.kkt_condense / kkt_tile_order, by the same functions (kkt_row_is_kept, kkt_order, kkt_pair_lists).  pos[nu]:
 * unknown (variable, or n + index among the rows that stay in the matrix) -> position in the factorised matrix; info[6] = nu,
 * Ts (independent leading tile columns), Tr (remainder tiles), Nf (positions in use), Fpad = 64 (Ts + Tr), and 1 when the
 * coupling mask is handed to the kernels (Ts > 0, Tr > 0, SQPHIP_NO_TILE_MASK unset).  tmask[Tr][max(Ts, 1)], pair_ptr[Tr (Tr + 1)
 * / 2 + 1], pair_k[*n_k]: the mask and the pair lists (all zero / empty where the kernels get none); each is written when
 * its capacity suffices (cap_mask, cap_ptr, cap_k entries). */
int sqphip_kkt_order_info(int64_t n, int64_t m, int64_t nnzJ, const int64_t *jrow, const int64_t *jcol, int64_t nnzH,
                          const int64_t *hrow, const int64_t *hcol, const double *gL, const double *gU, int32_t condense,
                          int32_t tile_order, int32_t *pos, int32_t *info, uint8_t *tmask, int32_t cap_mask, int32_t *pair_ptr,
                          int32_t cap_ptr, int32_t *pair_k, int32_t cap_k, int32_t *n_k);
/* Dense twin of sqphip_mf_batch_test, on a context that uses the dense solver (SQPHIP_ESTATE otherwise).  Inputs per instance,
 * back to back as there; rhs[B][n + m]: a full-length right-hand side [g; b].  Every instance's xv, vv and dinv are preset to
 * `sentinel`; the working vector of the solves is built twice from rhs -- by k_sp_load_xv (mode 0) and by load_solve_vector --
 * and *xv_mismatch counts the entries whose bits differ between the two; then k_kkt_assemble, and what a sweep does on the dense
 * path: ldlt_factor with the right-hand side fused in, the inertia test, the backward solve of the instances that passed.
 * Outputs (any may be null): K_assembled[B][Fpad * Fpad] (column-major in factorised order, as the device holds it behind the
 * assembly) and xv_loaded[B][Fpad]; sol / dinv[B][nu] in unknown order; dinv_pad[B][Fpad] as the device holds it; decision[B][4]
 * = outcome (0 idle, 1 another shift needed, 2 passed, 3 given up), sel, n_factor, fac_attempt; dw_out[B].  Leaves every
 * instance idle. */
int sqphip_kkt_dense_test(sqphip_ctx *ctx, const int32_t *active, const double *Jval, const double *Hval, const double *Dd,
                          const double *sigp, const double *hd, const int32_t *rtype, const double *hsc, const double *dw,
                          const double *dw_last, const int32_t *fac_attempt, const double *rhs, double sentinel,
                          double *K_assembled, double *xv_loaded, int32_t *xv_mismatch, double *sol, double *dinv,
                          double *dinv_pad, int32_t *decision, double *dw_out);
/* The working vector of the solves by the two routines of the one-workgroup stages, on a context of either solver: the column
 * walk (load_solve_vector) and the entry-parallel terms in LDS (solve_vector_terms, what build_rhs runs where the context has
 * the stage).  Inputs per instance, back to back: Jval [B][nnzJ], Dd / rtype [B][m], rhs [B][n + m] = [g; b].  Every instance
 * with active[b] != 0 is built by both; xv of every instance is preset to SQPHIP_SOLVE_VECTOR_SENTINEL before each, which is
 * what an inactive instance comes back with.  xv_plain / xv_terms [B][Fpad] (may be null); *mismatch: entries whose bits differ.
 * SQPHIP_ESTATE where the context runs without the stage (options.kkt_condense = 0, SQPHIP_NO_VSTAGE, SQPHIP_XV_TERMS=0, a
 * structure whose stage does not fit).  Leaves every instance idle. */
#define SQPHIP_SOLVE_VECTOR_SENTINEL (-7.5)
int sqphip_solve_vector_test(sqphip_ctx *ctx, const int32_t *active, const double *Jval, const double *Dd, const int32_t *rtype,
                             const double *rhs, double *xv_plain, double *xv_terms, int32_t *mismatch);
/* Launch census of the multifrontal path: launches enqueued per kernel instantiation (factor, solve, inertia test) since the
 * context was created.  counts[cap]; names (may be null): cap x 64 characters; *n_kernels = number of instantiations. */
int sqphip_mf_census(const sqphip_ctx *ctx, int64_t *counts, char *names, int32_t cap, int32_t *n_kernels);
/* Transition launch groups in line: how many sweeps, summed over the instance groups of the context, have launched the three
 * transition kernels (k_qp_finish, k_sqp_stage, k_ipm_head) themselves since the context was created.  With the transitions
 * riding in the post launch (SQPHIP_TRANS_RIDE) that is the first sweep of every run of every group and no other. */
int sqphip_trans_inline_groups(const sqphip_ctx *ctx, int64_t *count);
/* Host-only (no GPU): the shape of the multifrontal plan sqphip_create builds for the structure, condense option and batch
 * (and the SQPHIP_MF_SMALL_FRONT / _ZERO_FRAC / _ROWS_AFTER overrides it reads): fronts[cap_fronts][3] = (columns, rows,
 * level), launches[cap_launches][4] = factor launches (level, tiles of the kernel, fronts, tiles of the smallest front);
 * *top2_lds_bytes: LDS of the streamed top-of-tree solve (0: none); *spine_fronts: fronts of the spine kernel (0: none). */
int sqphip_mf_plan_info(int64_t n, int64_t m, int64_t nnzJ, const int64_t *jrow, const int64_t *jcol, int64_t nnzH,
                        const int64_t *hrow, const int64_t *hcol, const double *gL, const double *gU, int32_t condense,
                        int32_t batch, int32_t *fronts, int32_t cap_fronts, int32_t *n_fronts, int32_t *launches,
                        int32_t cap_launches, int32_t *n_launches, int64_t *top2_lds_bytes, int32_t *spine_fronts);
/* Host-only (no GPU): what the factorisation launches for the same plan under the current environment --
 * kernels[cap_launches][4], one row per row of `launches` above = (index in the census of sqphip_mf_census of the front kernel
 * chosen for the launch, 1 when its instantiation with the packed LDS image runs, 1 when the spine kernel takes the launch
 * instead, 1 when the launch held at most eight fronts before the deferral pass); big_lds: whether the device grants 160 KB of
 * dynamic LDS (every MI355X does). */
int sqphip_mf_factor_kernels(int64_t n, int64_t m, int64_t nnzJ, const int64_t *jrow, const int64_t *jcol, int64_t nnzH,
                             const int64_t *hrow, const int64_t *hcol, const double *gL, const double *gU, int32_t condense,
                             int32_t batch, int32_t big_lds, int32_t *kernels, int32_t cap_launches, int32_t *n_launches);
/* Host-only (no GPU): where the deferral pass of the plan (SQPHIP_MF_DEFER) put the fronts of the same plan --
 * fronts[cap_fronts][3] = (factor launch the front runs in: a row of `launches` above, its launch in the schedule before the
 * pass, numbered in that schedule -- the rows of `launches` under SQPHIP_MF_DEFER=0 --, parent front or -1 for a root). */
int sqphip_mf_front_launches(int64_t n, int64_t m, int64_t nnzJ, const int64_t *jrow, const int64_t *jcol, int64_t nnzH,
                             const int64_t *hrow, const int64_t *hcol, const double *gL, const double *gU, int32_t condense,
                             int32_t batch, int32_t *fronts, int32_t cap_fronts, int32_t *n_fronts);
/* ---- kernel-level entry points (parity tests, micro-benchmarks) -------------------------------
 * Batched dense LDL^T without pivoting of `batch` symmetric N x N matrices given as full
 * column-major host arrays A[batch][N*N] (lower triangle read).  On return L (unit lower) is in the
 * strict lower triangle, dinv[batch][N] = 1/D.  npos[batch] = number of positive pivots. */
int sqphip_ldlt_factor_host(int32_t device, int32_t batch, int64_t N, double *A, double *dinv,
                            int32_t *npos);
/* Factor + solve K x = rhs for each batch member; x overwrites rhs[batch][N]. */
int sqphip_ldlt_solve_host(int32_t device, int32_t batch, int64_t N, const double *A,
                           double *rhs);
/* time `reps` factorisations of resident random quasi-definite matrices; returns seconds per
 * factorisation of the whole batch and seconds spent in the trailing-update kernel */
int sqphip_ldlt_bench(int32_t device, int32_t batch, int64_t N, int32_t reps,
                      double *sec_per_factor, double *sec_trailing, int64_t *trailing_launches);
/* Host-only (no GPU): what sqphip_ldlt_case_test derives from the matrices when Ts > 0.  A[batch][N * N]: lower triangles in
 * full column-major storage; T = ceil(N / 64), Tr = T - Ts.  tmask[Tr][Ts]: the (remainder tile, leading tile) block has a
 * non-zero in some instance; pair_ptr[Tr (Tr + 1) / 2 + 1], pair_k[cap_k] (*n_k entries exist): the pair lists the product's
 * ordering builds from such a mask (order.hip, the same function).  SQPHIP_EINVAL and a message on stderr when some
 * instance has an entry between two different leading tiles. */
int sqphip_ldlt_tile_masks(int32_t batch, int64_t N, const double *A, int32_t Ts, uint8_t *tmask, int32_t *pair_ptr,
                           int32_t *pair_k, int32_t cap_k, int32_t *n_k);
/* One case of the dense path, everything at padded size Npad = 64 ceil(N / 64) so that the identity padding is visible.
 * A[batch][N * N]: lower triangles in full column-major storage (the strict upper triangle of the input is ignored); the
 * strict upper triangle of the device buffers is filled with quiet NaNs (nan_upper != 0) or zeros before the run.
 * rhs[batch][N] (may be null: factorisation only).  phase[batch] / want: the phase mask of the kernels (null: every instance).
 * Ts: independent leading tile columns (0: plain dense); the coupling mask and pair lists come from the zero blocks of A as in
 * sqphip_ldlt_tile_masks (SQPHIP_EINVAL when the leading block is not block diagonal); no_tile_mask != 0: Ts set, masks null
 * (the product under SQPHIP_NO_TILE_MASK).  The schedule switches (SQPHIP_KC, SQPHIP_OUTER, ...) are read from the environment
 * per call, as the product reads them.  Before the run dinv and v hold `sentinel` everywhere, b and both x the right-hand side
 * (zero padded): what an instance outside the mask must come back with.
 * Outputs (any may be null): factor[batch][Npad * Npad] (the device buffer after the factorisation: L strictly below the
 * diagonal), dinv[batch][Npad], npos[batch], b / v[batch][Npad] after the fused factorisation (y and D^-1 y), x_fused
 * (ldlt_factor with the right-hand side + backward steps), x_standalone (stand-alone forward and backward steps on the same
 * factors from a fresh right-hand side).  counts[cap] / names[cap][64] (may be null): launches per kernel instantiation of
 * ldlt.hip during the call; info[8] = number of instantiations counted, Npad, T, diagonal tiles factorised per instance,
 * launches enqueued on the auxiliary stream (counted where they are enqueued), 1 when the tile masks were in use, the longest
 * run of tiles per workgroup among the k_trailing launches and among the k_colupdate launches (SQPHIP_TPB; 0: no launch). */
int sqphip_ldlt_case_test(int32_t device, int32_t batch, int64_t N, const double *A, int32_t nan_upper, const double *rhs,
                          const int32_t *phase, int32_t want, int32_t Ts, int32_t no_tile_mask, double sentinel,
                          double *factor, double *dinv, int32_t *npos, double *b, double *v, double *x_fused,
                          double *x_standalone, int64_t *counts, char *names, int32_t cap, int64_t *info);

/* on-box fp64 MFMA issue-rate probe (register-resident v_mfma_f64_16x16x4_f64 loop), TFLOP/s */
/* test hook: factorise random batches with and without the look-ahead schedule and count repetitions whose
 * factors differ in any bit (must be 0) */
int sqphip_ldlt_stress(int32_t device, int32_t batch, int64_t N, int32_t reps, int32_t *mismatches);
int sqphip_mfma_f64_peak(int32_t device, double *tflops);

/* test hook of the batched seat: what instance `inst` holds on the device in the output slots of the sub-problem seat (the
 * results sqphip_qp_solve / _batch returned for it last) and the MOI status of its interior-point state -- an instance a batch
 * call does not list must come back unchanged.  Any output may be NULL. */
int sqphip_seat_peek(sqphip_ctx *ctx, int32_t inst, double *p, double *lambda, double *mult_x_U, double *mult_x_L,
                     double *slack, int32_t *moi_status);

#ifdef __cplusplus
}
#endif
#endif
