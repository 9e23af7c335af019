// nlp_rowblock_dev.hpp -- dense data blocks with several outputs (sqphip_nlp_add_row_block): one design matrix A (N x d), one
// pass over the points, R <= 8 weight vectors with a target row each,
//     row_r  +=  sum_{i < N} W_r[i] kappa(sum_{j < d} A[i][j] x_{col_j} + S_i)          (row 0: the objective, i: constraint row i)
// A, the columns, the kind, the rows and R are shared by the batch; W [R][N] and S [N] are the instance's (NlpBlkDev::ow, os).
// Row r has the Jacobian row A'(W_r kappa'), and the Hessian of the Lagrangian of all R outputs is one rank-N update
//     A' diag(kappa'' (sum_r mu_r W_r)) A,      mu_r = sigma for row 0, lambda_i for row i,
// which costs one pass on the MFMA pipe (v_mfma_f64_16x16x4_f64) whatever R is.
// nlp_blocks_eval (nlp_dev.hpp; the shared steps named below: nlp_blocks_dev.hpp) hands a block of the family NLP_BLK_ROWS
// to nlp_rowblock_eval, behind a barrier as any block.
// One call, by every thread of the workgroup, computes what the non-null pointers ask for:
//   1. points: thread i % TPB computes the logit u_i, then kappa, kappa', kappa'' once through nlp_block_kappa, and stores
//      kappa_i, kappa'_i (with any derivative) and z2_i = e_i kappa''_i (with the Hessian) in the instance's workspace, where
//      e_i = 0, e_i = fma(mu_r, W_r[i], e_i) for r = 0 .. R - 1 in that order;
//   2. values: for output r, thread t sums W_r[i] kappa_i over i = t, t + TPB, ... in rising order, then the workgroup's sum
//      (one barrier for all outputs), and that is added to *f_out (row 0, with f_out) or gv[row - 1] (with gv);
//   3. first derivatives: the pairs (r, j), numbered r d + j, are dealt to the waves (wave, wave + 16, ...); lane l sums
//      (W_r[i] kappa'_i) At[j][i] over i = l, l + 64, ... in rising order, the same butterfly, and lane 0 adds the sum to
//      grad[col_j] (row 0, with grad) or jv[js[r][j]] (with jv);
//   4. Hessian: the tile walk with d columns, one MFMA per four points in rising order, a = z2_p A[p][16 R + .] with one
//      rounding, b = A[p][16 C + .], points >= N as zeros; the lane that holds the lower entry (r, c) adds the accumulator,
//      with no further factor, to its COO slot.
// Every sum has a fixed order that depends on (N, d, R) only: bit-reproducible, independent of slot, neighbours and instance
// groups.  No atomics.  Pointers and scalars only, never DV; out of line.
#pragma once

namespace sqphip {

// the block's doubles in the instance's workspace (at NlpBlkDev::wz): kappa [N] | kappa' [N] | z2 [N]
struct NlpRowblockWs { long k0, k1, z2, size; };
static __host__ __device__ __forceinline__ NlpRowblockWs nlp_rowblock_ws(long N) { return {0, N, 2 * N, 3 * N}; }

// val: the instance's block of values; wsp: its workspace; part: [TPB / 64] wave sums of the instance, then [TPB][3] kappa,
// kappa', kappa'' of the point a thread is at.  Behind the barrier that ends the points the wave sums of output r sit at
// part[16 r ..]: the places of the threads' kappa values are free by then.
static __device__ __noinline__ void nlp_rowblock_eval(const NlpBlkDev *bp_, const double *val_, double *wsp_, double *part_,
                                                      const double *x_, double sigma_, const double *lam_, double *f_out_,
                                                      double *grad_, double *gv_, double *jv_, double *hv_)
{
    const NlpBlkDev *__restrict__ bp = nlp_uniform(bp_);
    const double *__restrict__ val = nlp_uniform(val_), *__restrict__ x = nlp_uniform(x_);
    const double *lam = nlp_uniform(lam_);
    double *wsp = nlp_uniform(wsp_), *part = nlp_uniform(part_);
    double *f_out = nlp_uniform(f_out_), *grad = nlp_uniform(grad_), *gv = nlp_uniform(gv_), *jv = nlp_uniform(jv_), *hv = nlp_uniform(hv_);
    const double sigma = nlp_uniform(sigma_);
    const int N = __builtin_amdgcn_readfirstlane(bp->N), d = __builtin_amdgcn_readfirstlane(bp->d);
    const int R = __builtin_amdgcn_readfirstlane(bp->R), ke = __builtin_amdgcn_readfirstlane(bp->ke);
    const double pw = nlp_uniform(bp->par);
    const double *__restrict__ A = nlp_uniform(bp->A), *__restrict__ At = nlp_uniform(bp->At);
    const int *__restrict__ col = nlp_uniform(bp->col), *__restrict__ js = nlp_uniform(bp->js);
    const double *__restrict__ W = val + __builtin_amdgcn_readfirstlane(bp->ow), *__restrict__ S = val + __builtin_amdgcn_readfirstlane(bp->os);
    const NlpRowblockWs ws = nlp_rowblock_ws(N);
    double *base = wsp + __builtin_amdgcn_readfirstlane(bp->wz), *k0 = base + ws.k0, *k1 = base + ws.k1, *z2 = base + ws.z2;
    const bool d1 = grad || jv || hv, d2 = hv != nullptr;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int wu = __builtin_amdgcn_readfirstlane(wv);
    #pragma unroll 1
    for (int i = threadIdx.x; i < N; i += TPB) {
        const double u = nlp_block_logit(At, x, col, S, N, d, i);
        double *__restrict__ k3 = part + TPB / 64 + 3 * threadIdx.x;
        nlp_block_kappa(ke, u, pw, (int)d1 + (int)d2, k3);
        k0[i] = k3[0];
        if (d1) k1[i] = k3[1];
        if (d2) {
            double e = 0.0;
            #pragma unroll 1
            for (int r = 0; r < R; ++r) {
                const int row = __builtin_amdgcn_readfirstlane(bp->row[r]);
                e = fma(row == 0 ? sigma : lam[row - 1], W[(long)r * N + i], e);
            }
            z2[i] = e * k3[2];
        }
    }
    __syncthreads();                        // kappa, kappa', z2 are complete; nobody is at its kappa values in part any more
    #pragma unroll 1
    for (int r = 0; r < R; ++r) {
        const int row = __builtin_amdgcn_readfirstlane(bp->row[r]);
        if (!(row == 0 ? f_out : gv)) continue;
        const double *__restrict__ Wr = W + (long)r * N;
        double f = 0.0;
        #pragma unroll 1
        for (int i = threadIdx.x; i < N; i += TPB) f += Wr[i] * k0[i];
        nlp_block_sum_put(f, part + r * (TPB / 64), wu);
    }
    __syncthreads();                        // the wave sums are complete
    if (threadIdx.x == 0) {
        #pragma unroll 1
        for (int r = 0; r < R; ++r) {
            const int row = __builtin_amdgcn_readfirstlane(bp->row[r]);
            double *out = row == 0 ? f_out : gv;
            if (!out) continue;
            const double s = nlp_block_sum_get(part + r * (TPB / 64));
            if (row == 0) *out += s;
            else out[row - 1] += s;
        }
    }
    if (grad || jv) {
        #pragma unroll 1
        for (int q = wu; q < R * d; q += TPB / 64) {
            const int r = q / d, j = q - r * d;
            const int row = __builtin_amdgcn_readfirstlane(bp->row[r]);
            double *out = row == 0 ? grad : jv;
            if (!out) continue;
            const double *__restrict__ a = At + (long)j * N, *__restrict__ Wr = W + (long)r * N;
            double s = 0.0;
            #pragma unroll 1
            for (int i = lane; i < N; i += 64) s += (Wr[i] * k1[i]) * a[i];
            s = nlp_wave_sum(s);
            if (lane == 0) out[row == 0 ? col[j] : js[q]] += s;
        }
    }
    if (hv) {
        nlp_d4 acc;
        nlp_block_hess_tiles(d, wu, nlp_uniform(bp->hs), hv,
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
            [&](int q, int) __attribute__((always_inline)) { return acc[q]; });
    }
}

}  // namespace sqphip
