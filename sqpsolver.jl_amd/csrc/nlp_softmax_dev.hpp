// nlp_softmax_dev.hpp -- multinomial (softmax) data blocks of a factorable NLP (sqphip_nlp_add_softmax_block): the objective
//     sum_{i < N} W_i [ log sum_{k < K} exp(u_ik) - u_{i, y_i} ],   u_ik = sum_{j < d} A[i][j] x_{col[k][j]} + S[k][i]
// with the design matrix A (N x d), the columns and the labels y shared by the batch and the weights W [N] and per-class
// offsets S [Kf][N] of the instance (NlpBlkDev::ow, os).  Kf = K - 1 classes carry variables when the last class is pinned
// (u_{i, K - 1} = 0), Kf = K otherwise; Kf d <= 128.  With the flat index q = k d + j and the softmax probabilities p_ik,
//     gradient  g_q    = sum_i W_i (p_ik - [y_i = k]) A_ij
//     Hessian   H_qq'  = sum_i W_i p_ik ([k = l] - p_il) A_ij A_ij'           (q' = l d + j')
// nlp_blocks_eval (nlp_dev.hpp; the shared steps named below: nlp_blocks_dev.hpp) hands a block of the family
// NLP_BLK_SOFTMAX to nlp_softmax_eval, behind a barrier as any block.  One call, by every thread of the workgroup:
//   1. points: thread i % TPB computes the logits u_ik (columns col[k][.], shifts S[k][.]) for k = 0 .. Kf - 1 and the maximum m
//      of the logits (the pinned class enters with 0, last); then, with the same logits computed again, e_k = exp(u_k - m) and
//      their sum s in class order (the pinned class adds exp(0 - m) last), lse = m + log(s) and the point's value
//      W_i (lse - u_{i, y_i}).  No thread keeps an array over the classes: with a gradient or Hessian asked for, e_k goes to
//      P[k][i] in the instance's workspace (consecutive doubles across lanes) and a second sweep leaves p_k = e_k / s there;
//      for f alone nothing is stored.  u_k - m <= 0 and s >= 1, so any finite logits give finite results;
//   2. f: per-thread sums over i = t, t + TPB, ... in rising order, then the workgroup's sum, *f_out += that;
//   3. gradient: wave w owns q = w, w + 16, ...; lane l sums (W_i (P[k][i] - [y_i = k])) At[j][i] over i = l, l + 64, ... in
//      rising order, the same butterfly, and lane 0 adds the sum to grad[col[q]];
//   4. Hessian: the tile walk over the Kf d x Kf d matrix, two accumulator chains of one v_mfma_f64_16x16x4_f64 per four points
//      each, p = 0, 4, 8, ... in rising order.  Both take a = (W_p P[k(r)][p]) A[p][j(r)]; chain 1 takes
//      b1 = (-P[k(c)][p]) A[p][j(c)], chain 2 takes b2 = A[p][j(c)].  The class of a row or column is the lane's own (k = q / d):
//      a tile may straddle class boundaries anywhere.  Chain 2 is skipped for a tile whose rows and columns share no class
//      (uniform over the wave).  Points >= N enter as zeros.  The lane that holds the lower entry (r, c) adds
//      sigma (acc1 + [k(r) = k(c)] acc2) to its COO slot; distinct columns make every slot single-writer within a block.
// Every sum has a fixed order that depends on (N, d, K, pinned) only.  No atomics.  Pointers and scalars only, never DV.
#pragma once

namespace sqphip {

// the block's doubles in the instance's workspace (at NlpBlkDev::wz): P [Kf][N]
struct NlpSoftmaxWs { long P, size; };
static __host__ __device__ __forceinline__ NlpSoftmaxWs nlp_softmax_ws(long N, long Kf) { return {0, Kf * N}; }

// u_ik of point i
static __device__ __forceinline__ double nlp_softmax_logit(const double *__restrict__ At, const double *__restrict__ x,
                                                           const int *__restrict__ col, const double *__restrict__ S, int N, int d,
                                                           int k, int i)
{
    return nlp_block_logit(At, x, col + k * d, S + (long)k * N, N, d, i);
}

// val: the instance's block of values; wsp: its workspace; part: [TPB / 64] wave sums of the instance
static __device__ __noinline__ void nlp_softmax_eval(const NlpBlkDev *bp_, const double *val_, double *wsp_, double *part_,
                                                     const double *x_, double sigma, double *f_out_, double *grad_, double *hv_)
{
    const NlpBlkDev *__restrict__ bp = nlp_uniform(bp_);
    const double *__restrict__ val = nlp_uniform(val_), *__restrict__ x = nlp_uniform(x_);
    double *wsp = nlp_uniform(wsp_), *__restrict__ part = nlp_uniform(part_);
    double *f_out = nlp_uniform(f_out_), *grad = nlp_uniform(grad_), *hv = nlp_uniform(hv_);
    // the block's fields arrive through vector loads: moved to scalar registers, the loop bounds and the tile bookkeeping below
    // are uniform to the compiler as they are in fact
    const int N = __builtin_amdgcn_readfirstlane(bp->N), d = __builtin_amdgcn_readfirstlane(bp->d);
    const int K = __builtin_amdgcn_readfirstlane(bp->K), Kf = __builtin_amdgcn_readfirstlane(bp->Kf), D = Kf * d;
    const double *__restrict__ A = nlp_uniform(bp->A), *__restrict__ At = nlp_uniform(bp->At);
    const int *__restrict__ col = nlp_uniform(bp->col), *__restrict__ y = nlp_uniform(bp->y);
    const double *__restrict__ W = val + __builtin_amdgcn_readfirstlane(bp->ow), *__restrict__ S = val + __builtin_amdgcn_readfirstlane(bp->os);
    double *P = wsp + __builtin_amdgcn_readfirstlane(bp->wz) + nlp_softmax_ws(N, Kf).P;
    const bool d1 = grad || hv, pinned = Kf < K;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    double f = 0.0;
    #pragma unroll 1
    for (int i = threadIdx.x; i < N; i += TPB) {
        const int yi = y[i];
        double m = -INFINITY, uy = 0.0;
        #pragma unroll 1
        for (int k = 0; k < Kf; ++k) {
            const double u = nlp_softmax_logit(At, x, col, S, N, d, k, i);
            m = fmax(m, u);
            if (k == yi) uy = u;
        }
        if (pinned) m = fmax(m, 0.0);
        double s = 0.0;
        #pragma unroll 1
        for (int k = 0; k < Kf; ++k) {
            const double e = nlp_block_exp(nlp_softmax_logit(At, x, col, S, N, d, k, i) - m);
            s += e;
            if (d1) P[(long)k * N + i] = e;
        }
        if (pinned) s += nlp_block_exp(0.0 - m);
        f += W[i] * ((m + nlp_block_log(s)) - uy);
        if (d1)
            #pragma unroll 1
            for (int k = 0; k < Kf; ++k) P[(long)k * N + i] = P[(long)k * N + i] / s;
    }
    nlp_block_sum_out(f, part, wv, f_out);      // (its barrier: P is complete as well)
    if (grad) {
        #pragma unroll 1
        for (int q = wv; q < D; q += TPB / 64) {
            const int k = q / d, j = q - k * d;
            const double *__restrict__ a = At + (long)j * N, *__restrict__ pk = P + (long)k * N;
            double s = 0.0;
            #pragma unroll 1
            for (int i = lane; i < N; i += 64) s += (W[i] * (pk[i] - (y[i] == k ? 1.0 : 0.0))) * a[i];
            s = nlp_wave_sum(s);
            if (lane == 0) grad[col[q]] += s;
        }
    }
    if (hv) {
        // The tile walk of nlp_block_hess_tiles, written out: through the shared walker the compiler forms the loads of the
        // chains another way and the larger benchmark shape loses 4 %; a change of the walk is made here as well.
        const int *__restrict__ hs = nlp_uniform(bp->hs);
        const int nt = (D + 15) >> 4, T = nt * (nt + 1) / 2;
        const int l15 = lane & 15, l4 = lane >> 4;
        const int wu = __builtin_amdgcn_readfirstlane(wv);      // the tile, its class range and the choice of chains: scalar registers
        #pragma unroll 1
        for (int t = wu; t < T; t += TPB / 64) {
            int R = 0;
            while ((R + 1) * (R + 2) / 2 <= t) ++R;
            const int Cc = t - R * (R + 1) / 2;
            const int cr = 16 * R + l15, cc = 16 * Cc + l15;
            const bool okr = cr < D, okc = cc < D;
            // class and feature of this lane's row (a operand) and column (b operands, and the column of its outputs); a lane
            // past the edge reads entry 0 and selects zero: every load is in bounds and none sits behind a branch
            const int kr = okr ? cr / d : 0, jr = okr ? cr - kr * d : 0, kc = okc ? cc / d : 0, jc = okc ? cc - kc * d : 0;
            const double *__restrict__ pr = P + (long)kr * N, *__restrict__ pc = P + (long)kc * N;
            // the classes of the tile's rows [16 R / d, rhi] and columns [16 C / d, chi]; C <= R
            const int rhi = (min(16 * R + 15, D - 1)) / d, chi = (min(16 * Cc + 15, D - 1)) / d;
            const bool two = (16 * R) / d <= chi && (16 * Cc) / d <= rhi;
            nlp_d4 acc1 = {0.0, 0.0, 0.0, 0.0}, acc2 = {0.0, 0.0, 0.0, 0.0};
            // four points: both chains, or chain 1 alone (second: a constant at either call)
            auto step = [&](int p0, bool second) __attribute__((always_inline)) {
                const bool okp = p0 + l4 < N;
                const int p = okp ? p0 + l4 : N - 1;
                const double av = (W[p] * pr[p]) * A[(long)p * d + jr], bv = A[(long)p * d + jc], pv = pc[p];
                const double a = okp && okr ? av : 0.0;
                const double b2 = okp && okc ? bv : 0.0;
                const double b1 = -pv * b2;
                acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b1, acc1, 0, 0, 0);
                if (second) acc2 = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b2, acc2, 0, 0, 0);
            };
            if (two) {
                #pragma unroll 2
                for (int p0 = 0; p0 < N; p0 += 4) step(p0, true);
            } else {
                #pragma unroll 2
                for (int p0 = 0; p0 < N; p0 += 4) step(p0, false);
            }
            #pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int r = 16 * R + l4 + 4 * q;
                if (r < D && cc <= r) {
                    const int s = hs[r * (r + 1) / 2 + cc];
                    if (s >= 0) hv[s] += sigma * (r / d == kc ? acc1[q] + acc2[q] : acc1[q]);
                }
            }
        }
    }
}

}  // namespace sqphip
