// nlp_dev.hpp -- device-side evaluator of a sparse factorable NLP (sqphip_nlp_attach): sums of products of univariate
// functions,
//     min  f0 + sum_{t: row(t) = 0} c_t prod_k phi_tk(x_{v_tk})
//     s.t. gL_i <= g0_i + sum_{t: row(t) = i} c_t prod_k phi_tk(x_{v_tk}) <= gU_i,   xL <= x <= xU
// with phi(x) = kappa(a x + b), kappa one of u^e (integer e), sin, cos, exp, log.  A term has at most 8 factors on distinct
// variables.  The structure of the batch (rows, variables, kinds, e, a, b) is fixed at attach; an instance carries its own
// values [f0 | g0 (m) | c (nterms)].  Two passes per evaluation, one workgroup per instance:
//   1. one thread per factor writes phi, phi', phi'' (chain factors a, a^2 included) into the instance's workspace in HBM
//      -- the only place that calls sincos / exp / log; integer powers by repeated multiplication, one reciprocal for a
//      negative exponent; only phi when just f / g are asked for (trial points, Armijo probes), phi'' only with the Hessian;
//   2. the gather plans of the host (CSR, indices only: per row, per variable, per Jacobian COO slot, per Hessian COO slot)
//      combine the stored values by multiplications only: c prod phi, c phi'_a prod_{k != a} phi_k,
//      c phi'_a phi'_b prod_{others}, c phi''_a prod_{k != a} phi_k, each times sigma or lambda_i.
// Every output entry is one thread's sum over its plan row in plan order: no atomics, bit-reproducible results that do not
// depend on the slot an instance sits in.
// sqphip_nlp_attach_affine: a factor may be kappa(u) of an affine form u = sum_j a_j x_{v_j} + b of up to 8 variables (summed
// in argument order, the shift added last).  Such a factor stores the plain kappa, kappa', kappa'' in pass 1 and the chain
// factors a_v (a_v a_w for a Hessian entry) reach pass 2 as the weights aw of its arguments, which the derivative plans name
// next to (term, factor).  A one-argument factor keeps the arithmetic above -- u = a x + b in one expression, a and a^2
// folded into phi', phi'' -- and its argument carries the weight 1.0: sqphip_nlp_attach builds such factors only, and
// c (prod 1.0) rounds as c prod does, so both entry points file the same bits for the same one-argument model.  A context
// without any multi-argument factor (NlpDev::multi = 0, uniform over the launch) skips the weight loads: the same bits, since
// the weights it skips are 1.0.
// sqphip_nlp_attach_general: a variable may sit in several factors of one term (x log x, (x + y)(x - y)), and the menu grows
// by sqrt, tanh, atan, the logistic pair 1 / (1 + e^-u), log(1 + e^u) in their overflow-free forms and u^p with a real p.
// Shared variables are the host's business alone: the plans file one entry per ordered pair of (factor, argument) couples
// and the sums above do the rest.  The six kinds sit behind one out-of-line function of scalars and the factor's place in
// the workspace (nlp_kappa_wide, one call site per nlp_eval): inlined, tanh / atan / log1p / pow cost the kernels that
// inline nlp_eval 120 - 130 B of scratch per lane each.
// sqphip_nlp_attach_data: shifts, coefficients and real exponents belong to the instance.  Its block goes on after c with
// b [nfac] | a [nargs] | p [nfac, only with a POWR factor] (NlpDev::ob, oa, op), and one switch, NlpDev::data, uniform over the
// launch as multi is, makes pass 1 read them there instead of fab / acoef / fpar.  Pass 2 takes its weights from a as well:
// the coefficient of an argument of a multi-argument factor, 1.0 for the argument of a one-argument factor (fvar >= 0),
// whose a is folded into phi', phi'' as above.  The arithmetic is the same expression on other operands, so a data context
// whose instances carry the attach's arrays files the bits of sqphip_nlp_attach_general; with the switch off no load moves.
// sqphip_nlp_add_block: dense data blocks sum_i W_i kappa(A_i'x + S_i) in the objective, W and S behind the other segments of
// the instance's block.  They are evaluated behind the plan passes by one out-of-line call per block (nlp_block_dev.hpp),
// inside a branch on NlpDev::nblk that is uniform over the launch: a context without a block runs the passes above and
// nothing else, on the workspace stride NlpDev::ws = 3 nfac it always had.
// sqphip_nlp_add_softmax_block: multinomial blocks sum_i W_i [log sum_k exp(u_ik) - u_{i, y_i}] count among the same four
// blocks; nlp_eval's one call for blocks is nlp_blocks_eval (below), which walks the blocks in block order and
// hands each to the evaluator of its family (NlpBlkDev::family).
// sqphip_nlp_add_row_block: a block with R <= 8 outputs, one weight vector and one target row each (row 0: the objective), on
// one design matrix: sum_i W_r[i] kappa(A_i'x + S_i) is added to row r's value, A'(W_r kappa') to its Jacobian row and
// A' diag(kappa'' sum_r mu_r W_r) A to the Hessian of the Lagrangian in one MFMA pass (nlp_rowblock_dev.hpp).  It counts among
// the same four blocks and adds to gv and jv behind the plan passes as the others add to f, grad and hv.
// sqphip_nlp_add_cox_block: Cox partial-likelihood blocks sum_i c_i [log sum_{j < risk[i]} W_j exp(u_j) - u_i] couple the points of
// a block through prefix and suffix scans (nlp_cox_dev.hpp); they count among the same four blocks and add to f, grad and hv.
// sqphip_nlp_add_lse_block: log-sum-exp row blocks, output r = log sum_{i in segment r} W_i exp(u_i) on the objective or a
// constraint row, any number of outputs over consecutive segments of the points (nlp_lse_dev.hpp); they count among the same
// four blocks and add to f, grad, gv, jv and hv.
// sqphip_nlp_add_norm_block: Euclidean-norm row blocks, output r = sqrt(sum_{i in segment r} W_i (A_i'x + S_i)^2) on the objective
// or a constraint row (second-order-cone rows, sums of norms), any number of outputs over consecutive segments of the points and
// any number of them on one target row (nlp_norm_dev.hpp); they count among the same four blocks and add to f, grad, gv, jv and hv.
#pragma once
#include "ctx.hpp"
#include "dev_util.hpp"
#include <cmath>

namespace sqphip {

// (the kinds NLP_POW .. NLP_POWR and NLP_KIND_BITS / _MASK: model_plans.hpp, shared with the host-side plan builder)
enum { NLP_NONE = -(1 << 30), NLP_ARG = (1 << 28) - 1 };     // no factor of a term; the argument bits of a plan entry (nargs <= 2^28)

// a dense data block (the sqphip_nlp_add_*_block calls; the shared steps, the evaluators and their dispatcher: included below)
enum { NLP_MAX_BLOCKS = 4, NLP_BLOCK_MAX_D = 128, NLP_SOFTMAX_MAX_K = 64, NLP_BLOCK_MAX_R = 8 };
// the family of a block, set by its add call and read by nlp_blocks_eval: sqphip_nlp_add_block, _row_block, _softmax_block,
// _cox_block, _lse_block, _norm_block
enum { NLP_BLK_SCALAR, NLP_BLK_ROWS, NLP_BLK_SOFTMAX, NLP_BLK_COX, NLP_BLK_LSE, NLP_BLK_NORM };

struct NlpBlkDev {
    int family;
    int ke, N, d;                         // kind + 16 * (exponent + 32) as NlpDev::fke (SCALAR, ROWS); points; columns
    int ow, os;                           // W [N] (ROWS: [R][N]), S [N] (SOFTMAX: [Kf][N]) in the instance's block of DV::nlv
    int wz;                               // the block's arrays in the instance's workspace (DV::nlw), laid out by the family's nlp_*_ws
    double par;                           // real exponent (POWR; SCALAR, ROWS)
    const double *A, *At;                 // [N][d] row-major (Hessian) and its transpose [d][N] (points, gradient)
    const int *col;                       // [d] variable of a column (0-based); SOFTMAX: [Kf d] over the flat index k d + j
    const int *hs;                        // [D (D + 1) / 2] COO slot of the lower entry (r, c) at r (r + 1) / 2 + c, D = d (SOFTMAX: Kf d); -1: no Hessian structure
    // SOFTMAX: K classes, of which Kf = K or K - 1 carry variables
    int K, Kf;
    const int *y;                         // [N] label of a point, 0 .. K - 1
    // ROWS, LSE: R outputs; their targets (0: the objective, i: row i, 1-based) in row for ROWS (inline, R <= 8) and in lrow for
    // LSE (uploaded, R not capped)
    int R;
    int row[NLP_BLOCK_MAX_R];
    const int *lrow;
    const int *js;                        // [R][d] Jacobian COO slot of (target of r, col[j]); unread for an output on row 0
    // COX
    const int *risk, *first;              // [N] leading points in the risk set of a point; [N] the first point whose risk set holds a point (0-based)
    const double *event;                  // [N] event indicator (0: censored)
    // LSE, NORM
    const int *seg, *outp;                // [R + 1] first point of an output; [N] output of a point
    // NORM: R outputs on T distinct targets (js: [T][d], by target); the outputs of at most NLP_NORM_SHORT points and the others
    const int *tgt, *trow;                // [R] target of an output, 0 .. T - 1; [T] row of a target (0: the objective, i: row i, 1-based)
    const int *tptr, *tout;               // [T + 1], [R] the outputs of a target in rising order (CSR)
    const int *shortl, *longl;            // [nshort], [nlong] outputs in rising order
    int T, nshort, nlong;
};

struct NlpDev {
    int n, m, nterms, nfac, nv, nobj;     // variables, rows, terms, factors, values per instance (even), objective terms
    int f_ptr, j_ptr, h_ptr;              // where the row pointers of the variable / Jacobian / Hessian plans start in ptr
    const int *ptr;                       // the four CSR row pointers back to back: rows [m + 1], variables [n + 1], slots
    const int *tptr;                      // [nterms + 1] factors of a term
    const int *fvar;                      // [nfac] variable of a one-argument factor (0-based); -1: the arguments aptr[k] .. aptr[k + 1] - 1
    const int *fke;                       // [nfac] kind + 16 * (exponent + 32)
    const double2 *fab;                   // [nfac] (a, b)
    const int *ot;                        // [nobj] the objective's terms
    const int *ge;                        // row i: g0_i + sum over terms t
    const int2 *fe;                       // variable j: sum over (term, argument + 2^28 its factor within the term) of objective terms
    const int2 *je;                       // Jacobian slot: sum over (term, argument + 2^28 its factor within the term)
    const int4 *he;                       // Hessian slot: sum over (term, the same for factor a, for factor b or a, row or -1) times
                                          // lambda[row] or sigma
    const int *aptr;                      // [nfac + 1] arguments of a factor
    const int *avar;                      // [nargs] variable of an argument (0-based)
    const double *acoef;                  // [nargs] its coefficient (pass 1)
    const double *aw;                     // [nargs] its weight in the derivative plans: the coefficient, 1.0 in a one-argument factor
    int multi;                            // some factor has several arguments; 0: every weight is 1.0 and the plans do not load aw
    const double *fpar;                   // [nfac] real exponent of a POWR factor (loaded for that kind only)
    int data;                             // sqphip_nlp_attach_data: b, a, p are the instance's, in its block of DV::nlv at ...
    int ob, oa, op;                       // ... ob [nfac], oa [nargs], op [nfac] (op: with a POWR factor only); fab, acoef, aw, fpar unread
    int ws;                               // doubles of workspace per instance (DV::nlw): 3 nfac, with blocks + TPB / 64 wave sums + 3 TPB kappa values + every block's own (the size of its family's nlp_*_ws)
    int nblk;                             // dense data blocks of any family (the sqphip_nlp_add_*_block calls); uniform over the launch
    NlpBlkDev blk[NLP_MAX_BLOCKS];
};

// pass 1 of a factor of the kinds SQRT .. POWR at u: kappa, a kappa', a^2 kappa'' to w[0], w[nf], w[2 nf] (nd: how many
// derivatives).  Out of line on purpose and never handed DV: scalars and the factor's workspace pointer only.
struct NlpK3 { double k0, k1, k2; };
static __device__ __noinline__ void nlp_kappa_wide(int kind, double a, double u, double pw, int nd, double *__restrict__ w, int nf)
{
    NlpK3 r;
    if (kind == NLP_SQRT) {
        const double s = sqrt(u);
        r.k0 = s; r.k1 = 0.5 / s; r.k2 = -0.25 / (u * s);
    } else if (kind == NLP_TANH) {
        // sech^2 u = 4 e / (1 + e)^2 with e = exp(-2 |u|) <= 1: no 1 - t t, which cancels from |u| = 2 on and is 0 from 19.07 on
        const double t = tanh(u), e = exp(-2.0 * fabs(u)), p = 1.0 + e, d = 4.0 * e / (p * p);
        r.k0 = t; r.k1 = d; r.k2 = -2.0 * t * d;
    } else if (kind == NLP_ATAN) {
        // -2 (u q) q: q q underflows from |u| = 1e77 on, where -2 u q q is still a normal number
        const double q = 1.0 / (1.0 + u * u);
        r.k0 = atan(u); r.k1 = q; r.k2 = -2.0 * (u * q) * q;
    } else if (kind == NLP_POWR) {
        const double v = pow(u, pw);
        r.k0 = v; r.k1 = pw * v / u; r.k2 = pw * (pw - 1.0) * v / (u * u);
    } else {
        // e = exp(-|u|) <= 1 never overflows; s and 1 - s both from e, none by cancellation; (1 - s) - s = -+(1 - e) den
        // through expm1, which does not cancel around u = 0 either
        const double e = exp(-fabs(u)), den = 1.0 / (1.0 + e);
        const double s = u < 0.0 ? e * den : den, sc = u < 0.0 ? den : e * den;
        if (kind == NLP_SIGMOID) {
            const double dm = expm1(-fabs(u)) * den;
            r.k0 = s; r.k1 = s * sc; r.k2 = s * sc * (u < 0.0 ? -dm : dm);
        }
        else { r.k0 = fmax(u, 0.0) + log1p(e); r.k1 = s; r.k2 = s * sc; }
    }
    w[0] = r.k0;
    if (nd >= 1) w[nf] = a * r.k1;
    if (nd >= 2) w[2 * nf] = a * a * r.k2;
}

// c-free product of term t with its factors a and b (counted within the term) differentiated (a == b: twice;
// NLP_NONE: not at all), in factor order
static __device__ __forceinline__ double nlp_prod(const int *__restrict__ tptr, const double *__restrict__ w, int nf, int t,
                                                  int a, int b)
{
    double p = 1.0;
    const int k0 = tptr[t];
    a += k0; b += k0;
    #pragma unroll 1
    for (int k = k0; k < tptr[t + 1]; ++k) p *= w[((k == a) + (k == b)) * nf + k];
    return p;
}

// the weight of the argument named by the plan entry ey (argument + 2^28 its factor within term t); aw: NlpDev::aw, or the
// a segment of the instance's block on a data context, where a one-argument factor keeps its weight 1.0
static __device__ __forceinline__ double nlp_weight(const NlpDev &q, const double *__restrict__ aw, bool data, int t, int ey)
{
    if (data && q.fvar[q.tptr[t] + (ey >> 28)] >= 0) return 1.0;
    return aw[ey & NLP_ARG];
}

// pass 1 for factor k at u = a x + b (pw: the exponent of a POWR factor)
static __device__ __forceinline__ void nlp_factor(int ke, double a, double u, double pw, bool d1, bool d2, double *__restrict__ w, int nf, int k)
{
    const int kind = ke & NLP_KIND_MASK;
    double p0, p1 = 0.0, p2 = 0.0;
    if (kind >= NLP_SQRT) {
        nlp_kappa_wide(kind, a, u, pw, (int)d1 + (int)d2, w + k, nf);
        return;
    } else if (kind == NLP_POW) {
        const int e = (ke >> NLP_KIND_BITS) - 32, ae = e < 0 ? -e : e;
        const double q = e < 0 ? 1.0 / u : u;
        // lo = q^(ae - 2) (e >= 2) or 1; then u^(e-2), u^(e-1), u^e upwards (e > 0) or q^ae, q^(ae+1), q^(ae+2) (e < 0)
        double lo = 1.0;
        #pragma unroll 1
        for (int i = (e < 0 ? 0 : 2); i < ae; ++i) lo *= q;
        if (e > 0) {
            const double m1 = e >= 2 ? lo * u : 1.0;
            p0 = m1 * u; p1 = e * m1 * a; p2 = (double)(e * (e - 1)) * lo * (a * a);
        } else {
            const double m1 = lo * q;
            p0 = lo; p1 = e * m1 * a; p2 = (double)(e * (e - 1)) * (m1 * q) * (a * a);
        }
    } else if (kind == NLP_EXP) {
        p0 = exp(u); p1 = a * p0; p2 = a * a * p0;
    } else if (kind == NLP_LOG) {
        const double r = 1.0 / u;
        p0 = log(u); p1 = a * r; p2 = -(a * a) * (r * r);
    } else {
        double s, c;
        sincos(u, &s, &c);
        if (kind == NLP_SIN) { p0 = s; p1 = a * c; p2 = -(a * a) * s; }
        else { p0 = c; p1 = -a * s; p2 = -(a * a) * c; }
    }
    w[k] = p0;
    if (d1) w[nf + k] = p1;
    if (d2) w[2 * nf + k] = p2;
}

}  // namespace sqphip
#include "nlp_blocks_dev.hpp"
#include "nlp_block_dev.hpp"
#include "nlp_rowblock_dev.hpp"
#include "nlp_softmax_dev.hpp"
#include "nlp_cox_dev.hpp"
#include "nlp_lse_dev.hpp"
#include "nlp_norm_dev.hpp"
namespace sqphip {

// every block of the context in block order; a barrier in front of each: the plan passes of nlp_eval and an earlier block wrote
// f, grad, gv, jv and hv entries that this block adds to from other threads.  Out of line, pointers and scalars only: the kernels
// that inline nlp_eval carry one call for all blocks of any family.
static __device__ __noinline__ void nlp_blocks_eval(const NlpBlkDev *blk_, int nblk_, const double *val_, double *wsp_, double *part_,
                                                    const double *x_, double sigma_, const double *lam_, double *f_out_, double *grad_,
                                                    double *gv_, double *jv_, double *hv_)
{
    // the arguments are the same in every lane: in scalar registers they cross the calls below without a frame of saved
    // vector registers (80 B per lane otherwise, which every kernel that inlines nlp_eval would carry)
    const NlpBlkDev *blk = nlp_uniform(blk_);
    const double *val = nlp_uniform(val_), *x = nlp_uniform(x_);
    double *wsp = nlp_uniform(wsp_), *part = nlp_uniform(part_), *f_out = nlp_uniform(f_out_), *grad = nlp_uniform(grad_), *hv = nlp_uniform(hv_);
    const double *lam = nlp_uniform(lam_);
    double *gv = nlp_uniform(gv_), *jv = nlp_uniform(jv_);      // (read and written by the families with target rows only)
    const int nblk = __builtin_amdgcn_readfirstlane(nblk_);
    const double sigma = nlp_uniform(sigma_);
    #pragma unroll 1
    for (int k = 0; k < nblk; ++k) {
        __syncthreads();
        switch (__builtin_amdgcn_readfirstlane(blk[k].family)) {      // uniform over the launch
        case NLP_BLK_SCALAR: nlp_block_eval(blk + k, val, wsp, part, x, sigma, f_out, grad, hv); break;
        case NLP_BLK_ROWS: nlp_rowblock_eval(blk + k, val, wsp, part, x, sigma, lam, f_out, grad, gv, jv, hv); break;
        case NLP_BLK_SOFTMAX: nlp_softmax_eval(blk + k, val, wsp, part, x, sigma, f_out, grad, hv); break;
        case NLP_BLK_COX: nlp_cox_eval(blk + k, val, wsp, part, x, sigma, f_out, grad, hv); break;
        case NLP_BLK_LSE: nlp_lse_eval(blk + k, val, wsp, part, x, sigma, lam, f_out, grad, gv, jv, hv); break;
        case NLP_BLK_NORM: nlp_norm_eval(blk + k, val, wsp, part, x, sigma, lam, f_out, grad, gv, jv, hv); break;
        }
    }
}


// the acopf_eval signature; any of f_out, grad, gv, jv, hv may be null.  Called by every thread of the workgroup.
static __device__ __forceinline__ void nlp_eval(const DV &d, int inst, const double *__restrict__ x, double sigma,
                                                const double *__restrict__ lam, double *f_out, double *grad, double *gv,
                                                double *jv, double *hv)
{
    const NlpDev &q = *d.nlp;
    const int nf = q.nfac;
    const double *__restrict__ val = d.nlv + (long)inst * q.nv;
    double *__restrict__ w = d.nlw + (long)inst * q.ws;
    const double *__restrict__ cf = val + 1 + q.m;
    const int *__restrict__ tptr = q.tptr;
    const bool d1 = grad || jv || hv, d2 = hv != nullptr;     // phi'' is read by the Hessian plan only
    const bool multi = q.multi != 0, data = q.data != 0;
    const double *__restrict__ aw = data ? val + q.oa : q.aw;
    __syncthreads();                        // x is complete; nobody still reads the workspace of an earlier evaluation
    #pragma unroll 1
    for (int k = threadIdx.x; k < nf; k += TPB) {
        const int v = q.fvar[k], ke = q.fke[k];
        double2 ab;
        double pw = 0.0;
        if (data) {
            ab = double2{v >= 0 ? aw[q.aptr[k]] : 1.0, val[q.ob + k]};
            if ((ke & NLP_KIND_MASK) == NLP_POWR) pw = val[q.op + k];
        } else {
            ab = q.fab[k];
            if ((ke & NLP_KIND_MASK) == NLP_POWR) pw = q.fpar[k];
        }
        const double *__restrict__ ac = data ? aw : q.acoef;
        double a = 1.0, u;
        if (v >= 0) { a = ab.x; u = ab.x * x[v] + ab.y; }
        else {
            u = 0.0;
            #pragma unroll 1
            for (int j = q.aptr[k]; j < q.aptr[k + 1]; ++j) u += ac[j] * x[q.avar[j]];
            u += ab.y;
        }
        nlp_factor(ke, a, u, pw, d1, d2, w, nf, k);
    }
    __syncthreads();
    if (f_out) {
        double f = 0.0;
        #pragma unroll 1
        for (int e = threadIdx.x; e < q.nobj; e += TPB) { const int t = q.ot[e]; f += cf[t] * nlp_prod(tptr, w, nf, t, NLP_NONE, NLP_NONE); }
        f = block_reduce<OpSum>(f);
        if (threadIdx.x == 0) *f_out = val[0] + f;
    }
    if (grad) {
        const int *ptr = q.ptr + q.f_ptr;
        #pragma unroll 1
        for (int j = threadIdx.x; j < q.n; j += TPB) {
            double s = 0.0;
            #pragma unroll 1
            for (int k = ptr[j]; k < ptr[j + 1]; ++k) {
                const int2 e = q.fe[k];
                s += cf[e.x] * (nlp_prod(tptr, w, nf, e.x, e.y >> 28, NLP_NONE) * (multi ? nlp_weight(q, aw, data, e.x, e.y) : 1.0));
            }
            grad[j] = s;
        }
    }
    if (gv)
        #pragma unroll 1
        for (int i = threadIdx.x; i < q.m; i += TPB) {
            double s = val[1 + i];
            #pragma unroll 1
            for (int k = q.ptr[i]; k < q.ptr[i + 1]; ++k) { const int t = q.ge[k]; s += cf[t] * nlp_prod(tptr, w, nf, t, NLP_NONE, NLP_NONE); }
            gv[i] = s;
        }
    if (jv) {
        const int *ptr = q.ptr + q.j_ptr;
        #pragma unroll 1
        for (int s_ = threadIdx.x; s_ < d.nnzj_coo; s_ += TPB) {
            double s = 0.0;
            #pragma unroll 1
            for (int k = ptr[s_]; k < ptr[s_ + 1]; ++k) {
                const int2 e = q.je[k];
                s += cf[e.x] * (nlp_prod(tptr, w, nf, e.x, e.y >> 28, NLP_NONE) * (multi ? nlp_weight(q, aw, data, e.x, e.y) : 1.0));
            }
            jv[s_] = s;
        }
    }
    if (hv) {
        const int *ptr = q.ptr + q.h_ptr;
        #pragma unroll 1
        for (int s_ = threadIdx.x; s_ < d.nnzh_coo; s_ += TPB) {
            double s = 0.0;
            #pragma unroll 1
            for (int k = ptr[s_]; k < ptr[s_ + 1]; ++k) {
                const int4 e = q.he[k];
                s += cf[e.x] * (nlp_prod(tptr, w, nf, e.x, e.y >> 28, e.z >> 28) * (multi ? nlp_weight(q, aw, data, e.x, e.y) * nlp_weight(q, aw, data, e.x, e.z) : 1.0)) *
                     (e.w < 0 ? sigma : lam[e.w]);
            }
            hv[s_] = s;
        }
    }
    // dense data blocks of any family, in block order behind a barrier each: one out-of-line call
    if (q.nblk != 0) nlp_blocks_eval(q.blk, q.nblk, val, w, w + 3 * nf, x, sigma, lam, f_out, grad, gv, jv, hv);
}

}  // namespace sqphip
