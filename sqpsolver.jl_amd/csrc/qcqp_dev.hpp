// qcqp_dev.hpp -- device-side evaluator of a general sparse QCQP (sqphip_qcqp_attach):
//     min  f0 + c'x + 1/2 x'Q0 x     s.t.  gL_i <= g0_i + a_i'x + 1/2 x'Q_i x <= gU_i,   xL <= x <= xU
// Every Q is given as triplets folded into the lower triangle: an off-diagonal v contributes v x_r x_c, a diagonal v
// contributes 1/2 v x_r^2 (the value convention of the Hessian COO).  The structure of the batch is fixed at attach; an
// instance carries its own values [f0 | c (n) | Q0 (nq0) | g0 (m) | A (na) | Q (nq)] in term order.  The host builds
// four gather plans once (CSR, indices only): per row (g), per variable (grad f), per Jacobian COO slot, per Hessian COO
// slot.  Every output entry is one thread's sum over its plan row in a fixed order: no atomics, bit-reproducible results
// that do not depend on the slot an instance sits in.
#pragma once
#include "ctx.hpp"
#include "dev_util.hpp"

namespace sqphip {

struct QcqpDev {
    int n, m, nv, nq0;                    // variables, rows, values per instance, Q0 terms
    int off_c, off_q0, off_g0;            // offsets of c, Q0 and g0 in an instance's values (f0 at 0)
    int f_ptr, j_ptr, h_ptr;              // where the row pointers of the variable / Jacobian / Hessian plans start in ptr
    const int *ptr;                       // the four CSR row pointers back to back: rows [m + 1], variables [n + 1], slots
    const int2 *q0;                       // Q0 terms (a, b), 0-based, folded (a >= b)
    const int4 *ge;                       // row i: g0_i + sum val[v] x[a] (b < 0) or val[v] x[a] x[b] (halved when a == b)
    const int2 *fe;                       // variable j: c_j + sum val[v] x[x]
    const int2 *je;                       // Jacobian slot: sum val[v] (x < 0: constant) or val[v] x[x]
    const int2 *he;                       // Hessian slot: sum val[v] times sigma (r < 0) or lambda[r]
};

// the acopf_eval signature; any of f_out, grad, gv, jv, hv may be null
static __device__ __forceinline__ void qcqp_eval(const DV &d, int inst, const double *__restrict__ x, double sigma,
                                                 const double *__restrict__ lam, double *f_out, double *grad, double *gv,
                                                 double *jv, double *hv)
{
    const QcqpDev &q = *d.qc;
    const double *__restrict__ val = d.qcv + (long)inst * q.nv;
    if (f_out) {
        double f = 0.0;
        #pragma unroll 1
        for (int j = threadIdx.x; j < q.n; j += TPB) f += val[q.off_c + j] * x[j];
        #pragma unroll 1
        for (int t = threadIdx.x; t < q.nq0; t += TPB) {
            const int2 e = q.q0[t];
            f += (e.x == e.y ? 0.5 : 1.0) * val[q.off_q0 + t] * x[e.x] * x[e.y];
        }
        f = block_reduce<OpSum>(f);
        if (threadIdx.x == 0) *f_out = val[0] + f;
    }
    if (grad) {
        const int *ptr = q.ptr + q.f_ptr;
        #pragma unroll 1
        for (int j = threadIdx.x; j < q.n; j += TPB) {
            double s = val[q.off_c + j];
            #pragma unroll 1
            for (int k = ptr[j]; k < ptr[j + 1]; ++k) {
                const int2 e = q.fe[k]; s += val[e.x] * x[e.y]; }
            grad[j] = s;
        }
    }
    if (gv)
        #pragma unroll 1
        for (int i = threadIdx.x; i < q.m; i += TPB) {
            double s = val[q.off_g0 + i];
            #pragma unroll 1
            for (int k = q.ptr[i]; k < q.ptr[i + 1]; ++k) {
                const int4 e = q.ge[k];
                const double t = val[e.x] * x[e.y];
                s += e.z < 0 ? t : (e.y == e.z ? 0.5 : 1.0) * t * x[e.z];
            }
            gv[i] = s;
        }
    if (jv) {
        const int *ptr = q.ptr + q.j_ptr;
        #pragma unroll 1
        for (int s_ = threadIdx.x; s_ < d.nnzj_coo; s_ += TPB) {
            double s = 0.0;
            #pragma unroll 1
            for (int k = ptr[s_]; k < ptr[s_ + 1]; ++k) { const int2 e = q.je[k]; s += e.y < 0 ? val[e.x] : val[e.x] * x[e.y]; }
            jv[s_] = s;
        }
    }
    if (hv) {
        const int *ptr = q.ptr + q.h_ptr;
        #pragma unroll 1
        for (int s_ = threadIdx.x; s_ < d.nnzh_coo; s_ += TPB) {
            double s = 0.0;
            #pragma unroll 1
            for (int k = ptr[s_]; k < ptr[s_ + 1]; ++k) { const int2 e = q.he[k]; s += val[e.x] * (e.y < 0 ? sigma : lam[e.y]); }
            hv[s_] = s;
        }
    }
}

}  // namespace sqphip
