// nlp_norm_dev.hpp -- Euclidean-norm row blocks of a factorable NLP (sqphip_nlp_add_norm_block): output r owns the consecutive
// points seg[r] .. seg[r + 1] - 1 of one design matrix A (N x d) and adds
//     f_r = sqrt( sum_{i in segment r} W_i v_i^2 ),   v_i = sum_{j < d} A[i][j] x_{col[j]} + S_i
// to row row[r] (0: the objective, i: constraint row i): second-order-cone rows a'x + kappa |P x| <= b (the linear part stays in the
// terms), sums of norms in the objective.  Any number of outputs may share a target row, row 0 included.  A, the columns, seg, the
// target of every output and the output of every point are shared by the batch and live in uploaded arrays (NlpBlkDev::tgt, seg,
// outp; the distinct targets: trow [T], their outputs in rising order: tptr [T + 1] / tout [R], their Jacobian slots: js [T][d]; the
// outputs of at most NLP_NORM_SHORT points: shortl [nshort], the others: longl [nlong], both rising); W [N] >= 0 and S [N] are the
// instance's (NlpBlkDev::ow, os).  A coefficient c_r > 0 on a norm goes into the weights as c_r^2; a smoothing delta is a point
// with a zero row of A and the shift delta -- there is no parameter for either.  With m_r the largest |v_i| over the points of
// segment r with W_i != 0,
//     y_i = v_i / m_r,  s_r = sum W_i y_i^2,  f_r = m_r sqrt(s_r),  q_i = W_i y_i / sqrt(s_r),  Jacobian row G_r = A_r' q,
//     Hessian of the Lagrangian  sum_r mu_r (A_r' diag(W / f_r) A_r - G_r G_r' / f_r),   mu_r = sigma on row 0, lam[row - 1] elsewhere.
// nlp_blocks_eval (nlp_dev.hpp; the shared steps named below: nlp_blocks_dev.hpp) hands a block of the family NLP_BLK_NORM to
// nlp_norm_eval, behind a barrier as any block.  One call, by every thread of the workgroup (the arrays: nlp_norm_ws below):
//   1. residuals: thread i % TPB computes v_i by the logit rule;
//   2. maxima, 3. sums and 4. norms, by the owner of an output.  A long output k of longl belongs to wave k % 16: lane l visits
//      i = seg[r] + l, + 64, ..., keeps the largest |v_i| among the visited points with W_i != 0, the xor butterfly 32 .. 1 (a maximum
//      does not depend on its order), then sums W_i y_i^2 over the same points in rising order and the butterfly.  A short output k
//      of shortl belongs to thread k % TPB, which takes the maximum and then the sum over i = seg[r], + 1, ... in rising order.  A
//      zero-weight point is never read into either.  m_r = 0 (no weighted point, or all weighted residuals exactly zero) gives
//      s_r = 0 without a division.  F[r] = m_r sqrt(s_r); sqrt(s_r) waits in G[r][0] for step 6;
//   5. values: thread t % TPB of target t adds F[r] over the target's outputs in rising r, one sum, to *f_out (row 0, with f_out) or
//      gv[row - 1] (with gv).  A call for values alone (the Armijo probe) ends here, with the bits of the full call;
//   6. by all threads over all points: q_i = W_i y_i / sqrt(s_r), exactly 0 where W_i = 0 or f_r = 0, and, with the Hessian,
//      z_i = mu_r W_i / f_r, likewise 0 there; then, behind a barrier and with the Hessian, m[r] becomes the coefficient of chain 2,
//      -mu_r / f_r, 0 where f_r = 0;
//   7. G[r][j]: the pairs (k, j) of the long outputs, numbered k d + j, are dealt to the waves (wave, wave + 16, ...); lane l sums
//      q_i At[j][i] over i = seg[r] + l, + 64, ... in rising order, then the butterfly.  The pairs (k, j) of the short outputs, numbered
//      k d + j, are dealt to the threads (thread, thread + TPB, ...), so consecutive threads hold consecutive j: the thread sums
//      q_i A[i][j] over i = seg[r], + 1, ... in rising order from row-major A, whose loads coalesce.  With the Hessian asked for G is
//      formed for every output, whatever pointers are null; without it the pairs of an output whose target has no pointer
//      (grad for row 0, jv elsewhere) are skipped and G[r][0] keeps sqrt(s_r), which nobody reads: step 8 skips the same targets;
//   8. first derivatives: thread (t d + j) % TPB adds G[r][j] over the outputs of target t in rising r, one sum, to grad[col[j]]
//      (row 0, with grad) or jv[js[t][j]] (with jv): one thread per entry, so outputs that share a row do not race;
//   9. Hessian: the tile walk with d columns, two accumulator chains of v_mfma_f64_16x16x4_f64: chain 1 one instruction per four
//      points p = 0, 4, ... in rising order, a = z_p A[p][16 R + .] (one rounding) against b = A[p][16 C + .]; chain 2 one
//      instruction per four outputs r = 0, 4, ... in rising order, a = m[r] G[r][16 R + .] (one rounding) against b = G[r][16 C + .].
//      Ragged edges in points, outputs and columns enter as zeros: loads are clamped, then selected.  The lane that holds the lower
//      entry (r, c) adds acc1 + acc2 to its COO slot.  The two parts are separate sums: their difference cancels (along v the
//      Hessian of a norm vanishes), and tests/nlp_norm_ref.py bounds the error by their magnitudes added.
// Every sum has a fixed order that depends on (N, d, seg, rows) only.  No atomics.  Pointers and scalars only, never DV; out of line.
// NLP_NORM_SHORT = 64 rests on a count of latencies, not on a measurement made before it was chosen: up to 64 points the wave form
// gives a lane one product and then six dependent shuffle-adds, for 16 pairs at a time; the thread form runs up to 64 dependent
// multiply-adds for 1 024 pairs at a time.  scripts/nlp_norm_bench.py measures both forms.
// Scaling: the squares are those of y, |y| <= 1, so residuals of 1e+-200 give finite values and first derivatives of the size of the
// data.  The apex: an output with f_r = 0 (all weights zero, or all weighted residuals exactly zero) files the value 0 -- exact
// for an unsmoothed norm -- and contributes exactly nothing to gradient, Jacobian and Hessian: q = 0, z = 0, coefficient 0 in chain
// 2, no division by zero, no NaN.  That derivative is one choice of subgradient (0 lies in the unit ball); a solver that is to
// converge to an apex wants the smoothing point.  A zero-weight point may hold an infinite or NaN residual: it is never read into
// a maximum, a sum or a product.  W >= 0 and finite residuals on weighted points are the caller's business.
#pragma once

#ifndef NLP_NORM_SHORT
#define NLP_NORM_SHORT 64               // an output of at most this many points is short (unmeasured when chosen: see above)
#endif

namespace sqphip {

// the block's doubles in the instance's workspace (at NlpBlkDev::wz): v [N] (from step 6 on q) | z [N] | m [R] (from step 6 on
// the coefficient of chain 2) | F [R] | G [R][d] (G[r][0]: sqrt(s_r) between steps 4 and 6)
struct NlpNormWs { long v, z, m, F, G, size; };
static __host__ __device__ __forceinline__ NlpNormWs nlp_norm_ws(long N, long R, long d)
{
    return {0, N, 2 * N, 2 * N + R, 2 * N + 2 * R, 2 * N + 2 * R + R * d};
}

// val: the instance's block of values; wsp: its workspace; part: unused (the sums of this block never leave a wave)
static __device__ __noinline__ void nlp_norm_eval(const NlpBlkDev *bp_, const double *val_, double *wsp_, double *part_,
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
    const int R = __builtin_amdgcn_readfirstlane(bp->R), T = __builtin_amdgcn_readfirstlane(bp->T);
    const int nshort = __builtin_amdgcn_readfirstlane(bp->nshort), nlong = __builtin_amdgcn_readfirstlane(bp->nlong);
    const double *__restrict__ A = nlp_uniform(bp->A), *__restrict__ At = nlp_uniform(bp->At);
    const int *__restrict__ col = nlp_uniform(bp->col), *__restrict__ js = nlp_uniform(bp->js);
    const int *__restrict__ tgt = nlp_uniform(bp->tgt), *__restrict__ seg = nlp_uniform(bp->seg), *__restrict__ outp = nlp_uniform(bp->outp);
    const int *__restrict__ trow = nlp_uniform(bp->trow), *__restrict__ tptr = nlp_uniform(bp->tptr), *__restrict__ tout = nlp_uniform(bp->tout);
    const int *__restrict__ shortl = nlp_uniform(bp->shortl), *__restrict__ longl = nlp_uniform(bp->longl);
    const double *__restrict__ W = val + __builtin_amdgcn_readfirstlane(bp->ow), *__restrict__ S = val + __builtin_amdgcn_readfirstlane(bp->os);
    const NlpNormWs ws = nlp_norm_ws(N, R, d);
    double *base = wsp + __builtin_amdgcn_readfirstlane(bp->wz), *vq = base + ws.v;       // v [N], from step 6 on q [N]
    double *zz = base + ws.z, *mm = base + ws.m, *F = base + ws.F, *G = base + ws.G;      // z [N]; m [R]; F [R]; G [R][d]
    const bool d1 = grad || jv || hv;
    const int lane = threadIdx.x & 63;
    const int wu = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // 1. residuals
    #pragma unroll 1
    for (int i = threadIdx.x; i < N; i += TPB) vq[i] = nlp_block_logit(At, x, col, S, N, d, i);
    __syncthreads();                        // v is complete
    // 2. - 4. long outputs: a wave each
    #pragma unroll 1
    for (int k = wu; k < nlong; k += TPB / 64) {
        const int r = __builtin_amdgcn_readfirstlane(longl[k]);
        const int i0 = __builtin_amdgcn_readfirstlane(seg[r]), i1 = __builtin_amdgcn_readfirstlane(seg[r + 1]);
        double m = 0.0;
        #pragma unroll 1
        for (int i = i0 + lane; i < i1; i += 64)
            if (W[i] != 0.0) m = fmax(m, fabs(vq[i]));
        #pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o));
        double s = 0.0;
        if (m != 0.0) {                     // (uniform over the wave)
            #pragma unroll 1
            for (int i = i0 + lane; i < i1; i += 64) {
                const double w = W[i];
                if (w != 0.0) { const double y = vq[i] / m; s += w * (y * y); }
            }
            s = nlp_wave_sum(s);
        }
        if (lane == 0) {
            const double sr = sqrt(s);
            mm[r] = m; F[r] = m * sr; G[(long)r * d] = sr;
        }
    }
    // 2. - 4. short outputs: a thread each
    #pragma unroll 1
    for (int k = threadIdx.x; k < nshort; k += TPB) {
        const int r = shortl[k];
        const int i0 = seg[r], i1 = seg[r + 1];
        double m = 0.0;
        #pragma unroll 1
        for (int i = i0; i < i1; ++i)
            if (W[i] != 0.0) m = fmax(m, fabs(vq[i]));
        double s = 0.0;
        if (m != 0.0) {
            #pragma unroll 1
            for (int i = i0; i < i1; ++i) {
                const double w = W[i];
                if (w != 0.0) { const double y = vq[i] / m; s += w * (y * y); }
            }
        }
        const double sr = sqrt(s);
        mm[r] = m; F[r] = m * sr; G[(long)r * d] = sr;
    }
    __syncthreads();                        // m, F and sqrt(s) are complete
    // 5. values: a thread per distinct target
    #pragma unroll 1
    for (int t = threadIdx.x; t < T; t += TPB) {
        const int row = trow[t];
        double *out = row == 0 ? f_out : gv;
        if (!out) continue;
        const int k1 = tptr[t + 1];
        int k = tptr[t];
        double s = F[tout[k]];
        #pragma unroll 1
        for (++k; k < k1; ++k) s += F[tout[k]];
        out[row == 0 ? 0 : row - 1] += s;
    }
    if (!d1) return;                        // (uniform over the workgroup)
    // 6. q and, with the Hessian, z; exactly 0 at a zero weight and at the apex
    #pragma unroll 1
    for (int i = threadIdx.x; i < N; i += TPB) {
        const int r = outp[i];
        const double w = W[i], f = F[r];
        const bool on = w != 0.0 && f != 0.0;
        double q = 0.0;
        if (on) q = w * (vq[i] / mm[r]) / G[(long)r * d];
        vq[i] = q;
        if (hv) {
            double z = 0.0;
            if (on) {
                const int row = trow[tgt[r]];
                z = (row == 0 ? sigma : lam[row - 1]) * w / f;
            }
            zz[i] = z;
        }
    }
    __syncthreads();                        // q and z are complete; nobody still reads m or sqrt(s)
    if (hv) {
        #pragma unroll 1
        for (int r = threadIdx.x; r < R; r += TPB) {
            const int row = trow[tgt[r]];
            const double f = F[r];
            mm[r] = f != 0.0 ? -(row == 0 ? sigma : lam[row - 1]) / f : 0.0;
        }
    }
    // 7. G of the long outputs: a wave per pair
    {
        const long LD = (long)nlong * d;    // (R d < 2^31: sqphip_nlp_add_norm_block)
        #pragma unroll 1
        for (int p = wu; p < LD; p += TPB / 64) {
            const int k = p / d, j = p - k * d;
            const int r = __builtin_amdgcn_readfirstlane(longl[k]);
            if (!hv && !(__builtin_amdgcn_readfirstlane(trow[tgt[r]]) == 0 ? grad : jv)) continue;
            const int i1 = __builtin_amdgcn_readfirstlane(seg[r + 1]);
            const double *__restrict__ a = At + (long)j * N;
            double s = 0.0;
            #pragma unroll 1
            for (int i = __builtin_amdgcn_readfirstlane(seg[r]) + lane; i < i1; i += 64) s += vq[i] * a[i];
            s = nlp_wave_sum(s);
            if (lane == 0) G[(long)r * d + j] = s;
        }
    }
    // 7. G of the short outputs: a thread per pair, consecutive threads on consecutive columns of row-major A
    {
        const long SD = (long)nshort * d;
        #pragma unroll 1
        for (int p = threadIdx.x; p < SD; p += TPB) {
            const int k = p / d, j = p - k * d;
            const int r = shortl[k];
            if (!hv && !(trow[tgt[r]] == 0 ? grad : jv)) continue;
            const int i1 = seg[r + 1];
            double s = 0.0;
            #pragma unroll 1
            for (int i = seg[r]; i < i1; ++i) s += vq[i] * A[(long)i * d + j];
            G[(long)r * d + j] = s;
        }
    }
    __syncthreads();                        // G and the coefficients of chain 2 are complete
    // 8. first derivatives: a thread per (target, column)
    {
        const long TD = (long)T * d;
        #pragma unroll 1
        for (int p = threadIdx.x; p < TD; p += TPB) {
            const int t = p / d, j = p - t * d;
            const int row = trow[t];
            double *out = row == 0 ? grad : jv;
            if (!out) continue;
            const int k1 = tptr[t + 1];
            int k = tptr[t];
            double s = G[(long)tout[k] * d + j];
            #pragma unroll 1
            for (++k; k < k1; ++k) s += G[(long)tout[k] * d + j];
            out[row == 0 ? col[j] : js[p]] += s;
        }
    }
    // 9. Hessian
    if (hv) {
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
                    const double av = zz[p] * A[(long)p * d + jr], bv = A[(long)p * d + jc];
                    acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(okp && okr ? av : 0.0, okp && okc ? bv : 0.0, acc1, 0, 0, 0);
                }
                #pragma unroll 1
                for (int r0 = 0; r0 < R; r0 += 4) {
                    const bool oko = r0 + l4 < R;
                    const int r = oko ? r0 + l4 : R - 1;
                    const double av = mm[r] * G[(long)r * d + jr], bv = G[(long)r * d + jc];
                    acc2 = __builtin_amdgcn_mfma_f64_16x16x4f64(oko && okr ? av : 0.0, oko && okc ? bv : 0.0, acc2, 0, 0, 0);
                }
            },
            [&](int q, int) __attribute__((always_inline)) { return acc1[q] + acc2[q]; });
    }
}

}  // namespace sqphip
