// sqp_dev.hpp -- the stage blocks of run! (sqp.hip has the reference lines) as device routines, for the two translation
// units whose kernels run them: sqp.hip (k_sqp_stage, k_sqp_begin, k_sqp_reset) and ipm.hip (k_ipm_post_ride, where the
// workgroup of an instance between two sub-problems runs its transition inside the post launch).  One workgroup of TPB
// threads owns one instance; every block keeps its own gate.
#pragma once
#include "ctx.hpp"
#include "dev_util.hpp"
#include "acopf_dev.hpp"
#include <cmath>

namespace sqphip {

// the sub-problem requested by this instance has reached a final MOI status
static __device__ __forceinline__ bool qp_final(const DV &d, int inst)
{
    const IpmState &I = d.ist[inst];
    return d.phase[inst] == PH_IDLE && I.start == 0 && I.status > 0;
}

#define SQP_PTRS                                                                                     \
    const long on = (long)inst * d.n, om = (long)inst * d.m;                                        \
    SqpState &S = d.sst[inst];                                                                       \
    IpmState &I = d.ist[inst];                                                                       \
    double *x = d.x + on, *lam = d.lambda + om, *mxL = d.mxL + on, *mxU = d.mxU + on;                \
    double *df = d.df + on, *E = d.E + om, *ps = d.pstep + on, *psoc = d.psoc + on;                  \
    double *plam = d.plam + om, *pmxL = d.pmxL + on, *pmxU = d.pmxU + on, *Esoc = d.Esoc + om;       \
    double *tmpx = d.tmpx + on, *tmpE = d.tmpE + om, *hlam = d.hlam + om;                            \
    const double *xL = d.xL + on, *xU = d.xU + on, *gL = d.gL + om, *gU = d.gU + om;                 \
    double *jcoo = d.jcoo + (long)inst * d.nnzj_coo, *hcoo = d.hcoo + (long)inst * d.nnzh_coo;       \
    double *jv = d.jv + (long)inst * d.nnzjc, *hv = d.hv + (long)inst * d.nnzhc;                     \
    (void)x; (void)lam; (void)mxL; (void)mxU; (void)df; (void)E; (void)ps; (void)psoc; (void)plam;   \
    (void)pmxL; (void)pmxU; (void)Esoc; (void)tmpx; (void)tmpE; (void)hlam; (void)xL; (void)xU;      \
    (void)gL; (void)gU; (void)jcoo; (void)hcoo; (void)jv; (void)hv; (void)I; (void)S;

// Julia isapprox(a,b): rtol = sqrt(eps), atol = 0 (sqp_trust_region.jl:146,:200,:535)
static __device__ __forceinline__ bool isapprox_d(double a, double b)
{
    if (a == b) return true;
    if (!fin(a) || !fin(b)) return false;
    return fabs(a - b) <= 1.4901161193847656e-08 * fmax(fabs(a), fabs(b));
}

// common.jl:54-77 with p = 1
static __device__ __forceinline__ double viol1(const DV &d, const double *E, const double *gL, const double *gU,
                               const double *x, const double *xL, const double *xU)
{
    double acc = 0.0;
    for (int i = threadIdx.x; i < d.m; i += TPB) {
        if (E[i] > gU[i]) acc += E[i] - gU[i];
        else if (E[i] < gL[i]) acc += gL[i] - E[i];
    }
    for (int j = threadIdx.x; j < d.n; j += TPB) {
        if (x[j] > xU[j]) acc += x[j] - xU[j];
        else if (x[j] < xL[j]) acc += xL[j] - x[j];
    }
    return block_reduce<OpSum>(acc);
}

static __device__ __forceinline__ double norm_inf(const double *v, int k)
{
    double a = 0.0;
    for (int i = threadIdx.x; i < k; i += TPB) a = fmax(a, fabs(v[i]));
    return block_reduce<OpMax>(a);
}

static __device__ __forceinline__ void gather_csc(const DV &d, const double *jcoo, const double *hcoo, double *jv, double *hv)
{
    for (int s = threadIdx.x; s < d.nnzjc; s += TPB) {
        double a = 0.0;
        for (int k = d.jg_ptr[s]; k < d.jg_ptr[s + 1]; ++k) a += jcoo[d.jg_src[k]];
        jv[s] = a;
    }
    if (hv)
        for (int s = threadIdx.x; s < d.nnzhc; s += TPB) {
            double a = 0.0;
            for (int k = d.hg_ptr[s]; k < d.hg_ptr[s + 1]; ++k) a += hcoo[d.hg_src[k]];
            hv[s] = a;
        }
}

// common.jl:14-23 on the CSC Jacobian; sgn = +1 literal, -1 textbook (lambda and mult_x_U negated)
static __device__ __forceinline__ double kt_residuals(const DV &d, const double *df, const double *lam, const double *mxU,
                                      const double *mxL, const double *jv, double sgn, double *rowsq)
{
    for (int i = threadIdx.x; i < d.m; i += TPB) {
        double a = 0.0;
        for (int k = d.jrowptr[i]; k < d.jrowptr[i + 1]; ++k) { const double v = jv[d.jrslot[k]]; a += v * v; }
        rowsq[i] = a;
    }
    double res = 0.0, sc = 1.0;
    for (int j = threadIdx.x; j < d.n; j += TPB) {
        double jtl = 0.0;
        for (int k = d.jcolptr[j]; k < d.jcolptr[j + 1]; ++k) jtl += jv[k] * lam[d.jrowval[k]];
        res = fmax(res, fabs(df[j] + sgn * jtl + sgn * mxU[j] - mxL[j]));
        sc = fmax(sc, fmax(fabs(df[j]), fmax(fabs(mxU[j]), fabs(mxL[j]))));
    }
    __syncthreads();
    for (int i = threadIdx.x; i < d.m; i += TPB) sc = fmax(sc, fabs(lam[i]) * sqrt(rowsq[i]));
    res = block_reduce<OpMax>(res);
    sc = block_reduce<OpMax>(sc);
    return res / sc;
}

static __device__ __forceinline__ void push_trace(const DV &d, int inst, SqpState &S, double pn)
{
    if (threadIdx.x == 0) {
        if (S.trace_len < SQPHIP_TRACE_CAP) {
            double *r = d.trace + ((long)inst * SQPHIP_TRACE_CAP + S.trace_len) * SQPHIP_TRACE_COLS;
            r[0] = S.iter; r[1] = S.step_acceptance; r[2] = S.fr; r[3] = S.sub_status; r[4] = S.it_ipm;
            r[5] = S.f; r[6] = S.phi; r[7] = S.mu; r[8] = S.Delta; r[9] = pn; r[10] = S.prim_infeas;
            r[11] = S.dual_infeas;
        }
        S.trace_len++;
    }
}

// work of a finished sub-problem, booked under its mode (sqphip_get_mode_counters)
static __device__ __forceinline__ void book_mode(SqpState &S, const IpmState &I)
{
    const int k = I.mode & 3;
    S.md_qp[k]++; S.md_ipm[k] += I.ipm_iters; S.md_fac[k] += I.n_factor;
    int *q = S.qlog + 4 * (S.qlog_n % SQPHIP_QLOG_CAP);
    q[0] = I.mode; q[1] = I.status; q[2] = I.ipm_iters; q[3] = I.n_factor;
    S.qerr[S.qlog_n % SQPHIP_QLOG_CAP] = (float)I.e0; S.qrule[S.qlog_n % SQPHIP_QLOG_CAP] = (signed char)(I.rc == 0 ? I.acc_rule : -1);
    if (I.rc == 0) S.term_rule[I.acc_rule & 3]++;
    S.qlog_n++;
}

static __device__ __forceinline__ void qp_request(IpmState &I, int mode, double delta, double mu_pen)
{
    I.mode = mode; I.delta = delta; I.mu_pen = mu_pen;
    I.stage = 0; I.rho_big = 1e4; I.start = 1; I.ipm_iters = 0; I.n_factor = 0; I.n_solve = 0; I.status = 0;
}

// sqp_trust_region.jl:215-222
static __device__ __forceinline__ void finalize(const DV &d, int inst, SqpState &S, const double *x)
{
    double f;
    __shared__ double fsh;
    acopf_eval(d, inst, x, 1.0, nullptr, &fsh, nullptr, nullptr, nullptr, nullptr);
    __syncthreads();
    f = fsh;
    if (threadIdx.x == 0) { S.obj_val = f; S.done = 1; S.stage = ST_DONE; }
}

// ---------------------------------------------------------------------------------------------
// state of a run about to start from x0; keep_totals: the cumulative work counters survive (a slot of the scenario queue)
static __device__ __forceinline__ void reset_instance(const DV &d, int inst, bool keep_totals)
{
    SQP_PTRS
    const double *x0 = d.x0 + on;
    for (int j = threadIdx.x; j < d.n; j += TPB) { x[j] = x0[j]; mxL[j] = 0; mxU[j] = 0; ps[j] = 0; psoc[j] = 0; }
    for (int i = threadIdx.x; i < d.m; i += TPB) { lam[i] = 0; E[i] = 0; }
    if (threadIdx.x == 0) {
        SqpState z = {};
        z.phi = 1e20; z.mu = d.init_mu; z.Delta = d.tr_size;
        z.prim_infeas = INFINITY; z.dual_infeas = INFINITY;
        z.step_acceptance = 1; z.fr = 0; z.iter = 1; z.ret = -5;
        if (keep_totals) {
            z.n_qp = S.n_qp; z.tot_ipm = S.tot_ipm; z.tot_fac = S.tot_fac; z.tot_sol = S.tot_sol; z.budget = S.budget;
            for (int k = 0; k < 4; ++k) { z.md_qp[k] = S.md_qp[k]; z.md_ipm[k] = S.md_ipm[k]; z.md_fac[k] = S.md_fac[k]; z.term_rule[k] = S.term_rule[k]; }
        }
        S = z;
        I.start = 0; I.dw_last = 0.0; I.prev_mode = 0;
        d.phase[inst] = PH_IDLE;
    }
}

// run! prologue: sqp_trust_region.jl:100-122
static __device__ __forceinline__ void b_sqp_begin(const DV &d)
{
    const int inst = blockIdx.x;
    SQP_PTRS
    const bool go = !(S.started || S.done);
    __syncthreads();                 // every thread has read the gate before any thread changes the state
    if (!go) return;
    __shared__ double fsh;
    acopf_eval(d, inst, x, 1.0, nullptr, &fsh, nullptr, E, nullptr, nullptr);
    __syncthreads();
    const double f = fsh;
    double lpv = 0.0;                                     // :244-253
    for (int i = threadIdx.x; i < d.nlin; i += TPB) { lpv += fmax(0.0, gL[i] - E[i]); lpv -= fmin(0.0, gU[i] - E[i]); }
    for (int j = threadIdx.x; j < d.n; j += TPB) { lpv += fmax(0.0, xL[j] - x[j]); lpv -= fmin(0.0, xU[j] - x[j]); }
    lpv = block_reduce<OpSum>(lpv);
    if (threadIdx.x == 0) { S.f = f; S.started = 1; S.it_ipm = 0; S.stage = ST_TOP; }
    if (isnan(f)) {                                       // :113-115
        if (threadIdx.x == 0) { S.ret = -13; S.done = 1; S.stage = ST_DONE; }
        return;
    }
    if (lpv > d.tol_infeas) {                             // :116-119 -> sub_optimize_lp! :264-304
        acopf_eval(d, inst, x, 1.0, nullptr, nullptr, df, nullptr, jcoo, nullptr);
        double *xk = d.xk + on;
        for (int j = threadIdx.x; j < d.n; j += TPB) xk[j] = x[j];
        if (threadIdx.x == 0) { qp_request(I, SQPHIP_MODE_LP, S.Delta, S.mu); S.stage = ST_LP; }
    }
}

static __device__ __forceinline__ void b_sqp_lp_finish(const DV &d)
{
    const int inst = blockIdx.x;
    SQP_PTRS
    const bool go = !(S.done || S.stage != ST_LP || !qp_final(d, inst));
    __syncthreads();                 // gate read by every thread before thread 0 moves the stage on
    if (!go) return;
    const double *op = d.op + on, *ol = d.olam + om, *oU = d.omxU + on, *oL = d.omxL + on;
    auto dz = [](double v) { return fabs(v) < 1e-10 ? 0.0 : v; };   // utils.jl:16-22
    for (int j = threadIdx.x; j < d.n; j += TPB) { x[j] = dz(op[j]); mxU[j] = dz(oU[j]); mxL[j] = dz(oL[j]); }
    for (int i = threadIdx.x; i < d.m; i += TPB) lam[i] = dz(ol[i]);
    if (threadIdx.x == 0) {
        S.sub_status = I.status; S.stage = ST_TOP; S.n_qp++; S.it_ipm = I.ipm_iters;
        S.tot_ipm += I.ipm_iters; S.tot_fac += I.n_factor; S.tot_sol += I.n_solve;
        book_mode(S, I);
    }
    __syncthreads();
    push_trace(d, inst, S, norm_inf(ps, d.n));            // print(sqp, "LP")
}

// top of the loop: iteration limit, eval_functions!, infeasibility measures, QP request
// (sqp_trust_region.jl:126-141)
static __device__ __forceinline__ void b_sqp_top(const DV &d)
{
    const int inst = blockIdx.x;
    SQP_PTRS
    const bool go = !(S.done || !S.started || S.stage != ST_TOP || S.budget <= 0);
    const int step_acceptance = S.step_acceptance, fr = S.fr;
    __syncthreads();                 // gate (and the flags used below) read by every thread before any write
    if (!go) return;
    if (threadIdx.x == 0) { S.stage = ST_QP; S.it_ipm = 0; }
    __syncthreads();
    if (S.iter > d.max_iter) {                            // sqp.jl:215-224
        if (threadIdx.x == 0) S.ret = S.prim_infeas <= d.tol_infeas ? 6 : -1;
        __syncthreads();
        finalize(d, inst, S, x);
        return;
    }
    if (step_acceptance) {                                // :134-138, sqp.jl:86-104
        const double hs = d.literal_quirks ? 1.0 : -1.0;
        for (int i = threadIdx.x; i < d.m; i += TPB) hlam[i] = hs * lam[i];
        __syncthreads();
        __shared__ double fsh;
        acopf_eval(d, inst, x, 1.0, hlam, &fsh, df, E, jcoo, d.nnzh_coo ? hcoo : nullptr);
        __syncthreads();
        gather_csc(d, jcoo, hcoo, jv, d.nnzh_coo ? hv : nullptr);
        __syncthreads();
        const double pr = viol1(d, E, gL, gU, x, xL, xU);
        const double du = kt_residuals(d, df, lam, mxU, mxL, jv, hs, tmpE);
        if (threadIdx.x == 0) { S.f = fsh; S.prim_infeas = pr; S.dual_infeas = du; }
    }
    // QP request: QpData(sqp) sqp.jl:66-79, dispatch :314-331
    double *xk = d.xk + on, *cin = d.cin + on, *bE = d.bE + om;
    for (int j = threadIdx.x; j < d.n; j += TPB) { xk[j] = x[j]; cin[j] = df[j]; }
    for (int i = threadIdx.x; i < d.m; i += TPB) bE[i] = E[i];
    if (threadIdx.x == 0) qp_request(I, fr ? SQPHIP_MODE_FR : SQPHIP_MODE_QP, S.Delta, S.mu);
}

// q(p) of sqp_trust_region.jl:487-508 (with_step = true); tmpx/tmpE are scratch
static __device__ __forceinline__ double qmodel_step(const DV &d, int inst, const SqpState &S, const double *p,
                                     const double *x, const double *df, const double *E, const double *jv,
                                     const double *hv, const double *gL, const double *gU, const double *xL,
                                     const double *xU, double *tmpx, double *tmpE)
{
    double acc = 0.0;
    for (int j = threadIdx.x; j < d.n; j += TPB) {
        double hp = 0.0;
        if (d.hfull) { const double *hj = hv + j; for (int k = 0; k < d.n; ++k) hp += hj[(long)k * d.n] * p[k]; }      // (dense Hessian: the mirrored entries, coalesced: ipm.hip hess_row)
        else for (int k = d.hcolptr[j]; k < d.hcolptr[j + 1]; ++k) hp += hv[k] * p[d.hrowval[k]];
        acc += df[j] * p[j] + 0.5 * p[j] * hp;
        tmpx[j] = x[j] + p[j];
    }
    for (int i = threadIdx.x; i < d.m; i += TPB) {
        double jp = 0.0;
        for (int k = d.jrowptr[i]; k < d.jrowptr[i + 1]; ++k) jp += jv[d.jrslot[k]] * p[d.jrcol[k]];
        tmpE[i] = E[i] + jp;
    }
    acc = block_reduce<OpSum>(acc);
    __syncthreads();
    return acc + S.mu * viol1(d, tmpE, gL, gU, tmpx, xL, xU);
}

static __device__ __forceinline__ void accept_step(const DV &d, double *x, double *lam, double *mxL, double *mxU,
                                   const double *step, const double *plam, const double *pmxL,
                                   const double *pmxU)
{
    for (int j = threadIdx.x; j < d.n; j += TPB) { x[j] += step[j]; mxL[j] += pmxL[j]; mxU[j] += pmxU[j]; }
    for (int i = threadIdx.x; i < d.m; i += TPB) lam[i] += plam[i];
}

// after the QP: compute_step!, status branches, phi, termination tests, do_step!
// (sqp_trust_region.jl:141-213, :370-380, :515-579)
static __device__ __forceinline__ void b_sqp_mid(const DV &d)
{
    const int inst = blockIdx.x;
    SQP_PTRS
    const bool go = !(S.done || S.stage != ST_QP || !qp_final(d, inst));
    // snapshot of the flags the branches below test: thread 0 changes S.fr / S.step_acceptance inside those
    // branches, and a wave that reads them late must not take a different path from the one that wrote them
    const int fr = S.fr, step_acceptance = S.step_acceptance;
    __syncthreads();
    if (!go) return;
    const double *op = d.op + on, *ol = d.olam + om, *oU = d.omxU + on, *oL = d.omxL + on;
    // compute_step! :373-378
    for (int j = threadIdx.x; j < d.n; j += TPB) { ps[j] = op[j]; pmxL[j] = oL[j] - mxL[j]; pmxU[j] = oU[j] - mxU[j]; }
    for (int i = threadIdx.x; i < d.m; i += TPB) plam[i] = ol[i] - lam[i];
    __syncthreads();
    const double nl_ = norm_inf(lam, d.m), nL = norm_inf(mxL, d.n), nU = norm_inf(mxU, d.n);
    const double pn = norm_inf(ps, d.n);
    const int st = I.status;
    if (threadIdx.x == 0) {
        S.mu = fmax(fmax(S.mu, nl_), fmax(nL, nU));
        S.sub_status = st; S.n_qp++; S.it_ipm += I.ipm_iters;
        S.tot_ipm += I.ipm_iters; S.tot_fac += I.n_factor; S.tot_sol += I.n_solve;
        book_mode(S, I);
    }
    __syncthreads();
    if (st == SQPHIP_MOI_LOCALLY_SOLVED) {
        if (S.Delta == 1e8 && isapprox_d(pn, S.Delta)) {            // :146-150
            if (threadIdx.x == 0) S.ret = 4;
            __syncthreads();
            finalize(d, inst, S, x);
            return;
        }
    } else if (st == SQPHIP_MOI_LOCALLY_INFEASIBLE) {
        if (fr) {                                                      // :152-159
            if (threadIdx.x == 0) S.ret = S.prim_infeas <= d.tol_infeas ? 6 : 2;
            __syncthreads();
            finalize(d, inst, S, x);
        } else {                                                       // :160-168
            if (threadIdx.x == 0) S.fr = 1;
            __syncthreads();
            push_trace(d, inst, S, pn);
            if (threadIdx.x == 0) { S.iter += 1; S.stage = ST_TOP; S.budget -= 1; }
        }
        return;
    } else {                                                           // :169-178 (quirk #1)
        if (threadIdx.x == 0 && S.prim_infeas <= d.tol_infeas * 10.0) S.ret = 6;
        __syncthreads();
        finalize(d, inst, S, x);
        return;
    }
    if (step_acceptance) {                                             // :180-182, sqp.jl:170-183 alpha = 0
        const double v = viol1(d, E, gL, gU, x, xL, xU);
        if (threadIdx.x == 0) S.phi = fr ? v : S.f + S.mu * v;
    }
    __syncthreads();
    push_trace(d, inst, S, pn);                                        // :184
    if (pn <= d.tol_direction) {                                       // :187-196
        if (fr) {
            if (threadIdx.x == 0) { S.fr = 0; S.iter += 1; S.stage = ST_TOP; S.budget -= 1; }
        } else {
            if (threadIdx.x == 0) S.ret = 0;
            __syncthreads();
            finalize(d, inst, S, x);
        }
        return;
    }
    if (S.prim_infeas <= d.tol_infeas && S.dual_infeas <= d.tol_residual && !isapprox_d(S.Delta, pn) &&
        !fr) {                                                       // :198-204
        if (threadIdx.x == 0) S.ret = 0;
        __syncthreads();
        finalize(d, inst, S, x);
        return;
    }
    // do_step! :515-579
    for (int j = threadIdx.x; j < d.n; j += TPB) tmpx[j] = x[j] + ps[j];
    __syncthreads();
    __shared__ double fsh;
    acopf_eval(d, inst, tmpx, 1.0, nullptr, &fsh, nullptr, tmpE, nullptr, nullptr);
    __syncthreads();
    const double c_k = viol1(d, tmpE, gL, gU, tmpx, xL, xU);
    const double phi_k = fr ? c_k : fsh + S.mu * c_k;
    double ared = S.phi - phi_k, pred = 1.0, q0 = 0.0;
    if (!fr) {
        q0 = S.mu * viol1(d, E, gL, gU, x, xL, xU);                    // compute_qmodel(sqp, false)
        const double qk = qmodel_step(d, inst, S, ps, x, df, E, jv, hv, gL, gU, xL, xU, tmpx, tmpE);
        pred = q0 - qk;
    }
    const double rho = ared / pred;
    if (ared > 0 && rho > 0) {                                         // :530-538
        accept_step(d, x, lam, mxL, mxU, ps, plam, pmxL, pmxU);
        if (threadIdx.x == 0) {
            if (isapprox_d(S.Delta, pn)) S.Delta = fmin(2 * S.Delta, 1e8);
            S.step_acceptance = 1;
        }
    } else {
        if (d.use_soc && c_k > 0 && !fr) {                           // :544-549 -> sub_optimize_soc! :341-360
            for (int j = threadIdx.x; j < d.n; j += TPB) tmpx[j] = x[j] + ps[j];
            __syncthreads();
            acopf_eval(d, inst, tmpx, 1.0, nullptr, nullptr, nullptr, Esoc, nullptr, nullptr);
            __syncthreads();
            double *bE = d.bE + om;
            for (int i = threadIdx.x; i < d.m; i += TPB) {
                double jp = 0.0;
                for (int k = d.jrowptr[i]; k < d.jrowptr[i + 1]; ++k) jp += jv[d.jrslot[k]] * ps[d.jrcol[k]];
                Esoc[i] -= jp;
                bE[i] = Esoc[i];
            }
            if (threadIdx.x == 0) {
                qp_request(I, SQPHIP_MODE_SOC, S.Delta, S.mu);
                S.q0 = q0; S.pnorm = pn; S.stage = ST_SOC;
            }
            return;
        }
        if (threadIdx.x == 0) {                                        // :574-577
            S.Delta = fmax(0.5 * fmin(S.Delta, pn), 0.1 * d.tol_direction);
            S.step_acceptance = 0;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (S.fr && S.step_acceptance) S.fr = 0;                       // :209-211
        S.iter += 1;                                                   // :213
        S.stage = ST_TOP; S.budget -= 1;
    }
}

// second half of do_step! for instances that requested a second-order correction (:551-572)
static __device__ __forceinline__ void b_sqp_soc_finish(const DV &d)
{
    const int inst = blockIdx.x;
    SQP_PTRS
    const bool go = !(S.done || S.stage != ST_SOC || !qp_final(d, inst));
    const int fr = S.fr;
    __syncthreads();
    if (!go) return;
    const double *op = d.op + on;
    for (int j = threadIdx.x; j < d.n; j += TPB) { psoc[j] = ps[j] + op[j]; tmpx[j] = x[j] + ps[j] + op[j]; }
    __syncthreads();
    __shared__ double fsh;
    acopf_eval(d, inst, tmpx, 1.0, nullptr, &fsh, nullptr, tmpE, nullptr, nullptr);
    __syncthreads();
    const double c_s = viol1(d, tmpE, gL, gU, tmpx, xL, xU);
    const double phi_soc = fr ? c_s : fsh + S.mu * c_s;
    const double ared = S.phi - phi_soc;
    const double qs = qmodel_step(d, inst, S, psoc, x, df, E, jv, hv, gL, gU, xL, xU, tmpx, tmpE);
    const double pred = S.q0 - qs;
    const double rho = ared / pred;
    if (threadIdx.x == 0) { S.n_qp++; S.it_ipm += I.ipm_iters; S.tot_ipm += I.ipm_iters; S.tot_fac += I.n_factor; S.tot_sol += I.n_solve; book_mode(S, I); }
    if (ared > 0 && rho > 0) {
        accept_step(d, x, lam, mxL, mxU, psoc, plam, pmxL, pmxU);
        if (threadIdx.x == 0) S.step_acceptance = 1;
    } else if (threadIdx.x == 0) {
        S.Delta = fmax(0.5 * fmin(S.Delta, S.pnorm), 0.1 * d.tol_direction);
        S.step_acceptance = 0;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (S.fr && S.step_acceptance) S.fr = 0;
        S.iter += 1;
        S.stage = ST_TOP; S.budget -= 1;
    }
}

// Scenario queue (ctx.hpp StreamDev): a slot whose run has terminated files its result under its scenario id, takes the
// next id, loads that scenario and runs the prologue of run! -- all inside the stage kernel of the sweep in which the
// run ended, so the slot never idles while scenarios are left.  On a QCQP or factorable-NLP context (sqphip_qcqp_stream_*,
// sqphip_nlp_stream_*) the scenario's data is its block of values; with keep_multipliers the row values and the multipliers
// are filed next to the point.

// The block copy of those two loaders: 2 nv2 doubles from a scenario's block of StreamDev::val into the slot's block of
// DV::qcv / DV::nlv.  The strides are even and both arrays come from the allocator, so every block is 16-byte aligned: two
// values per access, two accesses in flight per thread, every load of an iteration before its stores.
static __device__ __forceinline__ void stream_copy_block(double *dst, const double *src, int nv2)
{
    const double2 *sv = reinterpret_cast<const double2 *>(src);
    double2 *vw = reinterpret_cast<double2 *>(dst);
    for (int k = threadIdx.x; k < nv2; k += 2 * TPB) {
        const bool two = k + TPB < nv2;
        const double2 a = sv[k], b = two ? sv[k + TPB] : a;
        vw[k] = a;
        if (two) vw[k + TPB] = b;
    }
}

// ... and their copy of the scenario's bounds and start (one access in flight per table)
static __device__ __forceinline__ void stream_copy_bounds(const DV &d, const StreamDev &Q, int sc, long on, long om)
{
    double *xLw = d.xL + on, *xUw = d.xU + on, *gLw = d.gL + om, *gUw = d.gU + om, *x0w = d.x0 + on;
    const double *sxL = Q.xL + (long)sc * d.n, *sxU = Q.xU + (long)sc * d.n, *sx0 = Q.x0 + (long)sc * d.n;
    const double *sgL = Q.gL + (long)sc * d.m, *sgU = Q.gU + (long)sc * d.m;
    for (int j = threadIdx.x; j < d.n; j += TPB) { const double a = sxL[j], b = sxU[j], c = sx0[j]; xLw[j] = a; xUw[j] = b; x0w[j] = c; }
    for (int i = threadIdx.x; i < d.m; i += TPB) { const double a = sgL[i], b = sgU[i]; gLw[i] = a; gUw[i] = b; }
}

static __device__ __forceinline__ void b_sqp_stream(const DV &d)
{
    const int inst = blockIdx.x;
    SQP_PTRS
    const StreamDev &Q = d.stream;
    const int cur = Q.slot_scen[inst];
    const bool go = S.done && cur != -1;
    __syncthreads();                 // gate read by every thread before any write
    if (!go) return;
    if (cur >= 0) {
        double *rx = Q.rx + (long)cur * d.n;
        for (int j = threadIdx.x; j < d.n; j += TPB) rx[j] = x[j];
        if (Q.rE) {                  // sqphip_qcqp_stream_begin, keep_multipliers: what sqphip_sqp_get reads from the slot
            double *rE = Q.rE + (long)cur * d.m, *rl = Q.rlam + (long)cur * d.m;
            double *rmL = Q.rmxL + (long)cur * d.n, *rmU = Q.rmxU + (long)cur * d.n;
            for (int i = threadIdx.x; i < d.m; i += TPB) { const double a = E[i], b = lam[i]; rE[i] = a; rl[i] = b; }
            for (int j = threadIdx.x; j < d.n; j += TPB) { const double a = mxL[j], b = mxU[j]; rmL[j] = a; rmU[j] = b; }
        }
        if (threadIdx.x == 0) { Q.robj[cur] = S.obj_val; Q.rstat[cur] = S.ret; Q.riter[cur] = S.iter; }
    }
    __shared__ int nxt;
    if (threadIdx.x == 0) {
        const int k = atomicAdd(Q.next, 1);
        nxt = k < *Q.qend ? Q.qids[k] : -1;
    }
    __syncthreads();
    const int sc = nxt;
    if (sc < 0) {
        if (threadIdx.x == 0) Q.slot_scen[inst] = -1;
        return;
    }
    if (d.qc) {
        // A QCQP scenario is one block of qc->nv values in the layout of the slot's block of DV::qcv, next to its bounds and
        // start.
        const int nv2 = d.qc->nv >> 1;
        stream_copy_block(d.qcv + (long)inst * (2 * nv2), Q.val + (long)sc * (2 * nv2), nv2);
        stream_copy_bounds(d, Q, sc, on, om);
    } else if (d.nlp) {
        // The same for a factorable NLP: nlp->nv values (f0 | g0 | c, padded to even) into the slot's block of DV::nlv.  The
        // factor workspace DV::nlw needs no reset: every evaluation rewrites in its first pass what its second pass reads
        // (phi always, phi' / phi'' whenever a plan that reads them runs), behind the barrier at the entry of nlp_eval --
        // and the barrier below orders this copy before the first evaluation of the new scenario (b_sqp_begin).
        const int nv2 = d.nlp->nv >> 1;
        stream_copy_block(d.nlv + (long)inst * (2 * nv2), Q.val + (long)sc * (2 * nv2), nv2);
        stream_copy_bounds(d, Q, sc, on, om);
    } else {
        double *xLw = d.xL + on, *xUw = d.xU + on, *gLw = d.gL + om, *gUw = d.gU + om, *x0w = d.x0 + on;
        double *ohm = d.br_ohm + (long)inst * d.nl * 12, *c2 = d.c2 + (long)inst * d.ng, *c1 = d.c1 + (long)inst * d.ng;
        const double *sxL = Q.xL + (long)sc * d.n, *sxU = Q.xU + (long)sc * d.n, *sx0 = Q.x0 + (long)sc * d.n;
        const double *sgL = Q.gL + (long)sc * d.m, *sgU = Q.gU + (long)sc * d.m;
        const double *so = Q.ohm + (long)sc * d.nl * 12, *s2 = Q.c2 + (long)sc * d.ng, *s1 = Q.c1 + (long)sc * d.ng;
        for (int j = threadIdx.x; j < d.n; j += TPB) { xLw[j] = sxL[j]; xUw[j] = sxU[j]; x0w[j] = sx0[j]; }
        for (int i = threadIdx.x; i < d.m; i += TPB) { gLw[i] = sgL[i]; gUw[i] = sgU[i]; }
        for (int k = threadIdx.x; k < 12 * d.nl; k += TPB) ohm[k] = so[k];
        for (int g = threadIdx.x; g < d.ng; g += TPB) { c2[g] = s2[g]; c1[g] = s1[g]; }
    }
    __syncthreads();
    reset_instance(d, inst, true);
    if (threadIdx.x == 0) Q.slot_scen[inst] = sc;
    __syncthreads();
    b_sqp_begin(d);
}

// SQP-level stages of a sweep in dependency order (one workgroup owns one instance: its stages run one after the other,
// a barrier in between publishes the stage word thread 0 wrote; every stage keeps its own gate)
static __device__ __forceinline__ void b_sqp_stage(const DV &d)
{
    b_sqp_lp_finish(d);
    __syncthreads();
    b_sqp_mid(d);
    __syncthreads();
    if (d.use_soc) { b_sqp_soc_finish(d); __syncthreads(); }
    b_sqp_top(d);
    if (d.stream.M > 0) { __syncthreads(); b_sqp_stream(d); }
}

}  // namespace sqphip
