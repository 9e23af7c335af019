// nlp_cox_dev.hpp -- Cox partial-likelihood data blocks of a factorable NLP (sqphip_nlp_add_cox_block): the objective
//     sum_{i < N} c_i [ log sum_{j < risk[i]} W_j exp(u_j) - u_i ],   u_i = sum_{j < d} A[i][j] x_{col[j]} + S_i,   c_i = W_i event_i
// over points sorted by non-increasing time, so that the risk set of point i is the risk[i] leading points (Breslow ties: a tie
// group shares one value; i + 1 <= risk[i] <= N, non-decreasing).  The design matrix A (N x d), the columns, risk, first and
// event are shared by the batch, the weights W [N] and offsets S [N] are the instance's (NlpBlkDev::ow, os).  With
//     m = max_i u_i,  e_j = W_j exp(u_j - m),  T_i = sum_{j < risk[i]} e_j,  q_i = c_i / T_i (0 where c_i = 0),
//     Q_j = sum_{i >= first[j]} q_i      (first[j]: the first point whose risk set holds j; built by the host)
//     f = sum_i c_i (m + log T_i - u_i),   grad = A'(e o Q - c),
//     H = A' diag(e o Q) A - M' diag(c / T^2) M,   M_i = P[risk[i] - 1],   P[j] = sum_{k <= j} e_k A[k][.]
// nlp_blocks_eval (nlp_dev.hpp; the shared steps named below: nlp_blocks_dev.hpp) hands a block of the family NLP_BLK_COX
// to nlp_cox_eval, behind a barrier as any block.  One call, by every thread of the workgroup (the arrays: nlp_cox_ws below):
//   1. logits: thread i % TPB computes the logit u_i and keeps the largest of its own; the workgroup's maximum m (xor butterfly,
//      then the sixteen wave maxima: a maximum does not depend on its order); e_i = W_i exp(u_i - m);
//   2. scans, each by one wave alone in chunks of 64 points in rising order: within a chunk lane l adds the value of lane l - o
//      for o = 1, 2, 4, .. 32 (Hillis-Steele), then the carry of the chunks before is added and the sum of lane 63 becomes the
//      next carry.  Wave 0 scans e into cs; with a gradient or Hessian asked for, wave c % 16 scans the products
//      e_k At[c][k] (one rounding) into column c of P;
//   3. T_i = cs[risk[i] - 1]; f: thread t sums c_i ((m + log T_i) - u_i) over i = t, t + TPB, ... in rising order, skipping the
//      points with c_i = 0 (their logarithm is never formed), then the workgroup's sum, *f_out += that.  For f alone the call
//      ends here and P, q, 1 / T and G are never written;
//   4. q_i = c_i / T_i and 1 / T_i, both 0 where c_i = 0; wave 0 scans q from the last point down (the same chunked
//      scan on the index N - 1 - k), in place; G_j = e_j q[first[j]];
//   5. gradient: wave w owns the columns j = w, w + 16, ...; lane l sums (G_i - c_i) At[j][i] over i = l, l + 64, ... in rising
//      order, the butterfly, and lane 0 adds the sum to grad[col[j]];
//   6. Hessian: the tile walk with d columns, two accumulator chains of one v_mfma_f64_16x16x4_f64 per four points each,
//      p = 0, 4, 8, ... in rising order: chain 1 takes G_p A[p][r] against A[p][c], chain 2 takes (-q_p) P[risk[p] - 1][r] against
//      P[risk[p] - 1][c] (1 / T_p): the factor -c_p / T_p^2 is split between the two operands and never formed, since T^2
//      underflows once the logits of a risk set lie 350 below m.  Points >= N enter as zeros.  The lane that holds the lower
//      entry (r, c) adds sigma (acc1 + acc2) to its COO slot.  The two parts are separate sums: their difference is a
//      covariance and cancels, and tests/nlp_cox_ref.py bounds the error by their magnitudes added.
// Every sum has a fixed order that depends on (N, d, risk) only.  No atomics.  Pointers and scalars only, never DV.
// Domain: a point whose u_j lies more than about 700 below m underflows to e_j = 0; a risk set made of such points alone has
// T = 0 and files infinities -- the caller's business, as W >= 0 is.
#pragma once

namespace sqphip {

// the block's doubles in the instance's workspace (at NlpBlkDev::wz): u [N] (from step 4 on G = e o Q) | e [N] | cs [N] | q [N] |
// -q [N] | 1 / T [N] | P [N][d]
struct NlpCoxWs { long u, e, cs, q, nq, rT, P, size; };
static __host__ __device__ __forceinline__ NlpCoxWs nlp_cox_ws(long N, long d)
{
    return {0, N, 2 * N, 3 * N, 4 * N, 5 * N, 6 * N, 6 * N + N * d};
}

// the running sum of one chunk of 64 values by one wave: Hillis-Steele within the chunk, then the carry of the chunks before;
// the carry becomes the chunk's last sum
static __device__ __forceinline__ double nlp_cox_chunk_scan(double v, double &carry, int lane)
{
    #pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const double t = __shfl_up(v, o);
        if (lane >= o) v += t;
    }
    v += carry;
    carry = __shfl(v, 63);
    return v;
}

// val: the instance's block of values; wsp: its workspace; part: [TPB / 64] wave maxima, then wave sums of the instance
static __device__ __noinline__ void nlp_cox_eval(const NlpBlkDev *bp_, const double *val_, double *wsp_, double *part_,
                                                 const double *x_, double sigma, double *f_out_, double *grad_, double *hv_)
{
    const NlpBlkDev *__restrict__ bp = nlp_uniform(bp_);
    const double *__restrict__ val = nlp_uniform(val_), *__restrict__ x = nlp_uniform(x_);
    double *wsp = nlp_uniform(wsp_), *part = nlp_uniform(part_);
    double *f_out = nlp_uniform(f_out_), *grad = nlp_uniform(grad_), *hv = nlp_uniform(hv_);
    const int N = __builtin_amdgcn_readfirstlane(bp->N), d = __builtin_amdgcn_readfirstlane(bp->d);
    const double *__restrict__ A = nlp_uniform(bp->A), *__restrict__ At = nlp_uniform(bp->At);
    const int *__restrict__ col = nlp_uniform(bp->col), *__restrict__ risk = nlp_uniform(bp->risk), *__restrict__ first = nlp_uniform(bp->first);
    const double *__restrict__ ev = nlp_uniform(bp->event);
    const double *__restrict__ W = val + __builtin_amdgcn_readfirstlane(bp->ow), *__restrict__ S = val + __builtin_amdgcn_readfirstlane(bp->os);
    const NlpCoxWs ws = nlp_cox_ws(N, d);
    double *base = wsp + __builtin_amdgcn_readfirstlane(bp->wz), *ug = base + ws.u;        // u [N], from step 4 on G [N]
    double *e = base + ws.e, *cs = base + ws.cs, *qs = base + ws.q, *nq = base + ws.nq, *rT = base + ws.rT, *P = base + ws.P;
    const bool d1 = grad || hv;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int wu = __builtin_amdgcn_readfirstlane(wv);
    // 1. logits and their maximum
    double m = -INFINITY;
    #pragma unroll 1
    for (int i = threadIdx.x; i < N; i += TPB) {
        const double u = nlp_block_logit(At, x, col, S, N, d, i);
        ug[i] = u;
        m = fmax(m, u);
    }
    #pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o));
    if (lane == 0) part[wv] = m;
    __syncthreads();
    m = part[0];
    #pragma unroll 1
    for (int w = 1; w < TPB / 64; ++w) m = fmax(m, part[w]);
    #pragma unroll 1
    for (int i = threadIdx.x; i < N; i += TPB) e[i] = W[i] * nlp_block_exp(ug[i] - m);
    __syncthreads();                        // e is complete; every thread has read the wave maxima
    // 2. the scans: cs by wave 0, the columns of P dealt to the waves
    if (wu == 0) {
        double carry = 0.0;
        #pragma unroll 1
        for (int k0 = 0; k0 < N; k0 += 64) {
            const int k = k0 + lane;
            const double s = nlp_cox_chunk_scan(k < N ? e[k] : 0.0, carry, lane);
            if (k < N) cs[k] = s;
        }
    }
    if (d1) {
        #pragma unroll 1
        for (int c = wu; c < d; c += TPB / 64) {
            const double *__restrict__ a = At + (long)c * N;
            double carry = 0.0;
            #pragma unroll 1
            for (int k0 = 0; k0 < N; k0 += 64) {
                const int k = k0 + lane;
                const double s = nlp_cox_chunk_scan(k < N ? e[k] * a[k] : 0.0, carry, lane);
                if (k < N) P[(long)k * d + c] = s;
            }
        }
    }
    __syncthreads();                        // cs and P are complete
    // 3. T and f; 4. q and 1 / T
    double f = 0.0;
    #pragma unroll 1
    for (int i = threadIdx.x; i < N; i += TPB) {
        const double c = W[i] * ev[i];
        double q = 0.0, r = 0.0;
        if (c != 0.0) {
            const double T = cs[risk[i] - 1];
            if (f_out) f += c * ((m + nlp_block_log(T)) - ug[i]);
            q = c / T;
            r = 1.0 / T;
        }
        if (d1) { qs[i] = q; nq[i] = -q; rT[i] = r; }
    }
    nlp_block_sum_out(f, part, wv, f_out);  // (its barrier: q and 1 / T are complete as well; nobody reads u any more)
    if (!d1) return;                        // (uniform over the workgroup)
    if (wu == 0) {
        double carry = 0.0;
        #pragma unroll 1
        for (int k0 = 0; k0 < N; k0 += 64) {
            const int k = k0 + lane, i = N - 1 - k;
            const double s = nlp_cox_chunk_scan(k < N ? qs[i] : 0.0, carry, lane);
            if (k < N) qs[i] = s;
        }
    }
    __syncthreads();                        // q holds its sums from the last point down
    #pragma unroll 1
    for (int i = threadIdx.x; i < N; i += TPB) ug[i] = e[i] * qs[first[i]];
    __syncthreads();                        // G is complete
    // 5. gradient
    if (grad) {
        #pragma unroll 1
        for (int j = wu; j < d; j += TPB / 64) {
            const double *__restrict__ a = At + (long)j * N;
            double s = 0.0;
            #pragma unroll 1
            for (int i = lane; i < N; i += 64) s += (ug[i] - W[i] * ev[i]) * a[i];
            s = nlp_wave_sum(s);
            if (lane == 0) grad[col[j]] += s;
        }
    }
    // 6. Hessian
    if (hv) {
        nlp_d4 acc1, acc2;
        nlp_block_hess_tiles(d, wu, nlp_uniform(bp->hs), hv,
            [&](const NlpTile &t) __attribute__((always_inline)) {
                const bool okr = t.okr, okc = t.okc;   // (copies: read through t inside the loops, the loads are formed another way)
                const int l4 = t.l4;
                // a lane past the edge reads column 0 and selects zero: every load is in bounds and none sits behind a branch
                const int jr = okr ? t.cr : 0, jc = okc ? t.cc : 0;
                acc1 = nlp_d4{0.0, 0.0, 0.0, 0.0};
                acc2 = nlp_d4{0.0, 0.0, 0.0, 0.0};
                #pragma unroll 2
                for (int p0 = 0; p0 < N; p0 += 4) {
                    const bool okp = p0 + l4 < N;
                    const int p = okp ? p0 + l4 : N - 1;
                    const long rp = (long)(risk[p] - 1) * d;
                    const double av = ug[p] * A[(long)p * d + jr], bv = A[(long)p * d + jc];
                    const double mv = nq[p] * P[rp + jr], nv = P[rp + jc] * rT[p];
                    const double a1 = okp && okr ? av : 0.0, b1 = okp && okc ? bv : 0.0;
                    const double a2 = okp && okr ? mv : 0.0, b2 = okp && okc ? nv : 0.0;
                    acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc1, 0, 0, 0);
                    acc2 = __builtin_amdgcn_mfma_f64_16x16x4f64(a2, b2, acc2, 0, 0, 0);
                }
            },
            [&](int q, int) __attribute__((always_inline)) { return sigma * (acc1[q] + acc2[q]); });
    }
}

}  // namespace sqphip
