// nlp_lse_dev.hpp -- log-sum-exp row blocks of a factorable NLP (sqphip_nlp_add_lse_block): output r owns the consecutive
// points seg[r] .. seg[r + 1] - 1 of one design matrix A (N x d) and adds
//     lse_r = log sum_{i in segment r} W_i exp(u_i),   u_i = sum_{j < d} A[i][j] x_{col[j]} + S_i
// to row row[r] (0: the objective, i: constraint row i): the convex form of a posynomial, a smooth maximum of affine functions.
// A, the columns, seg, the rows and the output of every point are shared by the batch and live in uploaded arrays
// (NlpBlkDev::lrow, seg, outp, js), so R is not capped; W [N] >= 0 and S [N] are the instance's (NlpBlkDev::ow, os).  With m_r the
// largest u_i over the points of segment r with W_i != 0,
//     e_i = W_i exp(u_i - m_r),  T_r = sum e_i,  p_i = e_i / T_r,  value m_r + log T_r,  Jacobian row G_r = A_r' p,
//     Hessian of the Lagrangian  sum_r mu_r (A_r' diag(p) A_r - G_r G_r'),   mu_r = sigma on row 0, lam[row - 1] elsewhere.
// nlp_blocks_eval (nlp_dev.hpp; the shared steps named below: nlp_blocks_dev.hpp) hands a block of the family NLP_BLK_LSE
// to nlp_lse_eval, behind a barrier as any block.  One call, by every thread of the workgroup (the arrays: nlp_lse_ws below):
//   1. logits: thread i % TPB computes the logit u_i;
//   2. maxima: wave w owns the outputs r = w, w + 16, ...; lane l visits i = seg[r] + l, + 64, ... and keeps the largest u_i
//      among the visited points with W_i != 0; the xor butterfly 32 .. 1 (a maximum does not depend on its order);
//   3. exponentials, by all threads over all points: e_i = W_i exp(u_i - m_{out(i)}) where W_i != 0 and exactly 0 elsewhere.  The
//      exponential of a zero-weight point is never multiplied in: it may lie far above m_r and overflow, and 0 inf is a NaN;
//   4. sums: the wave of output r sums e_i per lane in rising order, then the butterfly; T_r is kept and lane 0 adds
//      m_r + log T_r to *f_out (row 0, with f_out) or gv[row - 1] (with gv).  A call for values alone (the Armijo probe) ends here;
//   5. probabilities: p_i = e_i / T_{out(i)} over all points and, with the Hessian, z_i = mu_{out(i)} p_i (one rounding);
//   6. first derivatives: the pairs (r, j), numbered r d + j, are dealt to the waves (wave, wave + 16, ...); lane l sums
//      p_i At[j][i] over i = seg[r] + l, + 64, ... in rising order, the butterfly, and lane 0 stores G[r][j] and adds it to
//      grad[col[j]] (row 0, with grad) or jv[js[r][j]] (with jv).  With the Hessian asked for G is formed for every output,
//      whatever pointers are null;
//   7. Hessian: the tile walk with d columns, two accumulator chains of v_mfma_f64_16x16x4_f64: chain 1 one instruction per four points p = 0, 4, ... in rising order, a = z_p A[p][16 R + .]
//      (one rounding) against b = A[p][16 C + .]; chain 2 one instruction per four outputs r = 0, 4, ... in rising order,
//      a = (-mu_r) G[r][16 R + .] (one rounding) against b = G[r][16 C + .].  Ragged edges in points, outputs and columns
//      enter as zeros.  The lane that holds the lower entry (r, c) adds acc1 + acc2, with no further factor, to its COO slot.
//      The two parts are separate sums: their difference is a covariance and cancels, and
//      tests/nlp_lse_ref.py bounds the error by their magnitudes added.
// Every sum has a fixed order that depends on (N, d, seg) only.  No atomics.  Pointers and scalars only, never DV; out of line.
// Domain: an output whose points all have weight 0, or whose weighted points all underflow, has T = 0 and files infinities or
// NaNs -- the caller's business, as W >= 0 is.  Logits 300 either side of the middle of one segment give finite results.
#pragma once

namespace sqphip {

// the block's doubles in the instance's workspace (at NlpBlkDev::wz): u [N] (from step 5 on p) | e [N] (from step 5 on z = mu p) |
// m [R] | T [R] | G [R][d]
struct NlpLseWs { long u, e, m, T, G, size; };
static __host__ __device__ __forceinline__ NlpLseWs nlp_lse_ws(long N, long R, long d)
{
    return {0, N, 2 * N, 2 * N + R, 2 * N + 2 * R, 2 * N + 2 * R + R * d};
}

// val: the instance's block of values; wsp: its workspace; part: unused (the sums of this block never leave a wave)
static __device__ __noinline__ void nlp_lse_eval(const NlpBlkDev *bp_, const double *val_, double *wsp_, double *part_,
                                                 const double *x_, double sigma_, const double *lam_, double *f_out_,
                                                 double *grad_, double *gv_, double *jv_, double *hv_)
{
    (void)part_;
    const NlpBlkDev *__restrict__ bp = nlp_uniform(bp_);
    const double *__restrict__ val = nlp_uniform(val_), *__restrict__ x = nlp_uniform(x_);
    const double *lam = nlp_uniform(lam_);
    double *wsp = nlp_uniform(wsp_);
    double *f_out = nlp_uniform(f_out_), *grad = nlp_uniform(grad_), *gv = nlp_uniform(gv_), *jv = nlp_uniform(jv_), *hv = nlp_uniform(hv_);
    const double sigma = nlp_uniform(sigma_);
    const int N = __builtin_amdgcn_readfirstlane(bp->N), d = __builtin_amdgcn_readfirstlane(bp->d);
    const int R = __builtin_amdgcn_readfirstlane(bp->R);
    const double *__restrict__ A = nlp_uniform(bp->A), *__restrict__ At = nlp_uniform(bp->At);
    const int *__restrict__ col = nlp_uniform(bp->col), *__restrict__ js = nlp_uniform(bp->js);
    const int *__restrict__ lrow = nlp_uniform(bp->lrow), *__restrict__ seg = nlp_uniform(bp->seg), *__restrict__ outp = nlp_uniform(bp->outp);
    const double *__restrict__ W = val + __builtin_amdgcn_readfirstlane(bp->ow), *__restrict__ S = val + __builtin_amdgcn_readfirstlane(bp->os);
    const NlpLseWs ws = nlp_lse_ws(N, R, d);
    double *base = wsp + __builtin_amdgcn_readfirstlane(bp->wz), *up = base + ws.u;        // u [N], from step 5 on p [N]
    double *ez = base + ws.e, *mm = base + ws.m, *Ts = base + ws.T, *G = base + ws.G;     // e [N], from step 5 on z [N]; m [R]; T [R]; G [R][d]
    const bool d1 = grad || jv || hv;
    const int lane = threadIdx.x & 63;
    const int wu = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // 1. logits
    #pragma unroll 1
    for (int i = threadIdx.x; i < N; i += TPB) up[i] = nlp_block_logit(At, x, col, S, N, d, i);
    __syncthreads();                        // u is complete
    // 2. maxima over the weighted points of a segment
    #pragma unroll 1
    for (int r = wu; r < R; r += TPB / 64) {
        const int i1 = __builtin_amdgcn_readfirstlane(seg[r + 1]);
        double m = -INFINITY;
        #pragma unroll 1
        for (int i = __builtin_amdgcn_readfirstlane(seg[r]) + lane; i < i1; i += 64)
            if (W[i] != 0.0) m = fmax(m, up[i]);
        #pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o));
        if (lane == 0) mm[r] = m;
    }
    __syncthreads();                        // m is complete
    // 3. exponentials; a zero-weight point is exactly 0 whatever its logit
    #pragma unroll 1
    for (int i = threadIdx.x; i < N; i += TPB) {
        const double w = W[i];
        double e = 0.0;
        if (w != 0.0) e = w * nlp_block_exp(up[i] - mm[outp[i]]);
        ez[i] = e;
    }
    __syncthreads();                        // e is complete
    // 4. sums and values
    #pragma unroll 1
    for (int r = wu; r < R; r += TPB / 64) {
        const int i1 = __builtin_amdgcn_readfirstlane(seg[r + 1]);
        double s = 0.0;
        #pragma unroll 1
        for (int i = __builtin_amdgcn_readfirstlane(seg[r]) + lane; i < i1; i += 64) s += ez[i];
        s = nlp_wave_sum(s);
        const int row = __builtin_amdgcn_readfirstlane(lrow[r]);
        double *out = row == 0 ? f_out : gv;
        if (out) {
            const double v = mm[r] + nlp_block_log(s);
            if (lane == 0) out[row == 0 ? 0 : row - 1] += v;
        }
        if (lane == 0) Ts[r] = s;
    }
    if (!d1) return;                        // (uniform over the workgroup)
    __syncthreads();                        // T is complete
    // 5. probabilities and, with the Hessian, z = mu p
    #pragma unroll 1
    for (int i = threadIdx.x; i < N; i += TPB) {
        const int r = outp[i];
        const double p = ez[i] / Ts[r];
        up[i] = p;
        if (hv) {
            const int row = lrow[r];
            ez[i] = (row == 0 ? sigma : lam[row - 1]) * p;
        }
    }
    __syncthreads();                        // p and z are complete
    // 6. first derivatives
    {
        const long RD = (long)R * d;        // (R d < 2^31: sqphip_nlp_add_lse_block)
        #pragma unroll 1
        for (int q = wu; q < RD; q += TPB / 64) {
            const int r = q / d, j = q - r * d;
            const int row = __builtin_amdgcn_readfirstlane(lrow[r]);
            double *out = row == 0 ? grad : jv;
            if (!out && !hv) continue;
            const int i1 = __builtin_amdgcn_readfirstlane(seg[r + 1]);
            const double *__restrict__ a = At + (long)j * N;
            double s = 0.0;
            #pragma unroll 1
            for (int i = __builtin_amdgcn_readfirstlane(seg[r]) + lane; i < i1; i += 64) s += up[i] * a[i];
            s = nlp_wave_sum(s);
            if (lane == 0) {
                G[q] = s;
                if (out) out[row == 0 ? col[j] : js[q]] += s;
            }
        }
    }
    // 7. Hessian
    if (hv) {
        __syncthreads();                    // G is complete
        nlp_d4 acc1, acc2;
        nlp_block_hess_tiles(d, wu, nlp_uniform(bp->hs), hv,
            [&](const NlpTile &t) __attribute__((always_inline)) {
                const bool okr = t.okr, okc = t.okc;   // (copies: read through t inside the loops, the loads are formed another way)
                const int l4 = t.l4;
                // a lane past the edge reads column 0 of the last point or output and selects zero: every load is in bounds
                const int jr = okr ? t.cr : 0, jc = okc ? t.cc : 0;
                acc1 = nlp_d4{0.0, 0.0, 0.0, 0.0};
                acc2 = nlp_d4{0.0, 0.0, 0.0, 0.0};
                #pragma unroll 2
                for (int p0 = 0; p0 < N; p0 += 4) {
                    const bool okp = p0 + l4 < N;
                    const int p = okp ? p0 + l4 : N - 1;
                    const double av = ez[p] * A[(long)p * d + jr], bv = A[(long)p * d + jc];
                    acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(okp && okr ? av : 0.0, okp && okc ? bv : 0.0, acc1, 0, 0, 0);
                }
                #pragma unroll 1
                for (int r0 = 0; r0 < R; r0 += 4) {
                    const bool oko = r0 + l4 < R;
                    const int r = oko ? r0 + l4 : R - 1;
                    const int row = lrow[r];
                    const double mu = row == 0 ? sigma : lam[row - 1];
                    const double av = (-mu) * G[(long)r * d + jr], bv = G[(long)r * d + jc];
                    acc2 = __builtin_amdgcn_mfma_f64_16x16x4f64(oko && okr ? av : 0.0, oko && okc ? bv : 0.0, acc2, 0, 0, 0);
                }
            },
            [&](int q, int) __attribute__((always_inline)) { return acc1[q] + acc2[q]; });
    }
}

}  // namespace sqphip
