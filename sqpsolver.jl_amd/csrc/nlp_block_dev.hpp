// nlp_block_dev.hpp -- dense data blocks of a factorable NLP (sqphip_nlp_add_block): the data-fitting objective
//     sum_{i < N} W_i kappa(sum_{j < d} A[i][j] x_{col_j} + S_i)
// with a dense N x d design matrix A shared by the batch (d <= 128, up to 4 blocks) and the weights W and shifts S of the
// instance, which sit behind the other segments of its block of values (NlpBlkDev::ow, os).  Gradient A'(W kappa'),
// Hessian A' diag(W kappa'') A: a dense fp64 rank-N update, done on the MFMA pipe (v_mfma_f64_16x16x4_f64).
// nlp_eval's one call for blocks (nlp_blocks_eval, nlp_dev.hpp; the shared steps named below: nlp_blocks_dev.hpp) calls
// nlp_block_eval for every block of the family NLP_BLK_SCALAR in block order, behind the plan passes and a barrier, with a
// barrier between two blocks (they may share gradient entries and Hessian slots).  One call, by every thread of the workgroup:
//   1. points: thread i % TPB computes the logit u_i, then kappa, kappa', kappa'' through nlp_factor -- the menu exists once --
//      and stores z1_i = W_i kappa'_i, z2_i = W_i kappa''_i in the instance's workspace (z1 with the gradient, z2 with the
//      Hessian; nothing is stored for f alone);
//   2. f: a thread sums W_i kappa_i over i = t, t + TPB, ... in rising order, then the workgroup's sum, and *f_out += that;
//   3. gradient: wave w owns the columns j = w, w + 16, ...; lane l sums z1_i At[j][i] over i = l, l + 64, ... in rising
//      order, the same butterfly, and lane 0 adds the sum to grad[col_j];
//   4. Hessian: the tile walk with d columns; a tile is accumulated by one MFMA per four points, p = 0, 4, 8, ... in rising order,
//      with the operands a = z2_p A[p][16 R + .] (one rounding) and b = A[p][16 C + .]; points >= N enter as zeros.  The lane
//      that holds the lower entry (r, c) adds sigma H[r][c] to its COO slot.
// Every sum has a fixed order that depends on N and d only: the results are bit-reproducible and do not depend on the
// slot, the neighbours or the instance groups.  They are not the bits of the same model written as per-point terms
// (another order of the sums); tests/nlp_block_ref.py states the forward error bound both meet.
#pragma once

namespace sqphip {

// the block's doubles in the instance's workspace (at NlpBlkDev::wz): z1 [N] | z2 [N]
struct NlpBlockWs { long z1, z2, size; };
static __host__ __device__ __forceinline__ NlpBlockWs nlp_block_ws(long N) { return {0, N, 2 * N}; }

// val: the instance's block of values; wsp: its workspace; part: [TPB / 64] wave sums of the instance, then [TPB][3] kappa, kappa', kappa'' of the point a thread is at
static __device__ __noinline__ void nlp_block_eval(const NlpBlkDev *bp_, const double *val_, double *wsp_, double *part_,
                                                   const double *x_, double sigma, double *f_out_, double *grad_, double *hv_)
{
    const NlpBlkDev *__restrict__ bp = nlp_uniform(bp_);
    const double *__restrict__ val = nlp_uniform(val_), *__restrict__ x = nlp_uniform(x_);
    double *__restrict__ wsp = nlp_uniform(wsp_), *__restrict__ part = nlp_uniform(part_);
    double *f_out = nlp_uniform(f_out_), *grad = nlp_uniform(grad_), *hv = nlp_uniform(hv_);
    const int N = bp->N, d = bp->d, ke = bp->ke;
    const double pw = bp->par;
    const double *__restrict__ A = bp->A, *__restrict__ At = bp->At;
    const int *__restrict__ col = bp->col;
    const double *__restrict__ W = val + bp->ow, *__restrict__ S = val + bp->os;
    const NlpBlockWs ws = nlp_block_ws(N);
    double *__restrict__ z1 = wsp + bp->wz + ws.z1, *__restrict__ z2 = wsp + bp->wz + ws.z2;
    const bool d1 = grad || hv, d2 = hv != nullptr;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    double f = 0.0;
    #pragma unroll 1
    for (int i = threadIdx.x; i < N; i += TPB) {
        const double u = nlp_block_logit(At, x, col, S, N, d, i);
        double *__restrict__ k3 = part + TPB / 64 + 3 * threadIdx.x;
        nlp_block_kappa(ke, u, pw, (int)d1 + (int)d2, k3);
        const double wi = W[i];
        f += wi * k3[0];
        if (grad) z1[i] = wi * k3[1];
        if (d2) z2[i] = wi * k3[2];
    }
    nlp_block_sum_out(f, part, wv, f_out);      // (its barrier: z1 and z2 are complete as well)
    if (grad) {
        #pragma unroll 1
        for (int j = wv; j < d; j += TPB / 64) {
            const double *__restrict__ a = At + (long)j * N;
            double s = 0.0;
            #pragma unroll 1
            for (int i = lane; i < N; i += 64) s += z1[i] * a[i];
            s = nlp_wave_sum(s);
            if (lane == 0) grad[col[j]] += s;
        }
    }
    if (hv) {
        nlp_d4 acc;
        nlp_block_hess_tiles(d, wv, bp->hs, hv,
            [&](const NlpTile &t) __attribute__((always_inline)) {
                const bool okr = t.okr, okc = t.okc;   // (copies: read through t inside the loops, the loads are formed another way)
                const int l4 = t.l4;
                // a lane past the edge reads column 0 of the last point and selects zero: every load is in bounds and none sits behind a branch
                const int jr = okr ? t.cr : 0, jc = okc ? t.cc : 0;
                acc = nlp_d4{0.0, 0.0, 0.0, 0.0};
                #pragma unroll 2
                for (int p0 = 0; p0 < N; p0 += 4) {
                    const bool okp = p0 + l4 < N;
                    const int p = okp ? p0 + l4 : N - 1;
                    const double av = z2[p] * A[(long)p * d + jr], bv = A[(long)p * d + jc];
                    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(okp && okr ? av : 0.0, okp && okc ? bv : 0.0, acc, 0, 0, 0);
                }
            },
            [&](int q, int) __attribute__((always_inline)) { return sigma * acc[q]; });
    }
}

}  // namespace sqphip
