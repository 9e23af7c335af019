// nlp_block_dev.hpp -- dense data blocks of a factorable NLP (sqphip_nlp_add_block): the data-fitting objective
//     sum_{i < N} W_i kappa(sum_{j < d} A[i][j] x_{col_j} + S_i)
// with a dense N x d design matrix A shared by the batch (d <= 128, up to 4 blocks) and the weights W and shifts S of the
// instance, which sit behind the other segments of its block of values (NlpBlkDev::ow, os).  Gradient A'(W kappa'),
// Hessian A' diag(W kappa'') A: a dense fp64 rank-N update, done on the MFMA pipe (v_mfma_f64_16x16x4_f64).
// nlp_eval's one call for blocks (nlp_blocks_eval, nlp_softmax_dev.hpp) calls nlp_block_eval for every such block in block
// order, behind the plan passes and a barrier, with a barrier between two blocks (they may share gradient entries and
// Hessian slots).  One call, by every thread of the workgroup:
//   1. points: thread i % TPB computes u_i = 0, u_i = fma(A[i][j], x_{col_j}, u_i) for j = 0 .. d - 1 in that order, u_i += S_i
//      (the rule of sqphip_nlp_attach_affine; A is read through its transpose At [d][N], so the lanes of a wave read
//      consecutive doubles), then kappa, kappa', kappa'' through nlp_factor -- the menu exists once -- and stores
//      z1_i = W_i kappa'_i, z2_i = W_i kappa''_i in the instance's workspace (z1 with the gradient, z2 with the Hessian;
//      nothing is stored for f alone);
//   2. f: a thread sums W_i kappa_i over i = t, t + TPB, ... in rising order, then the pattern of block_reduce: the xor
//      butterfly 32, 16, .. 1 within a wave, the sixteen wave sums added by thread 0 in wave order, and *f_out += that;
//   3. gradient: wave w owns the columns j = w, w + 16, ...; lane l sums z1_i At[j][i] over i = l, l + 64, ... in rising
//      order, the same butterfly, and lane 0 adds the sum to grad[col_j];
//   4. Hessian: the lower 16 x 16 tiles (R, C), C <= R, numbered R (R + 1) / 2 + C, tile t on wave t % 16; a tile is
//      accumulated by one MFMA per four points, p = 0, 4, 8, ... in rising order, with the operands
//      a = z2_p A[p][16 R + .] (one rounding) and b = A[p][16 C + .]; columns >= d and points >= N enter as zeros.  The
//      lane that holds the lower entry (r, c) then adds sigma H[r][c] to its COO slot (NlpBlkDev::hs).
// Every sum has a fixed order that depends on N and d only: the results are bit-reproducible and do not depend on the
// slot, the neighbours or the instance groups.  They are not the bits of the same model written as per-point terms
// (another order of the sums); tests/nlp_block_ref.py states the forward error bound both meet.
// The function takes pointers and scalars only, never DV, and is out of line: the kernels that inline nlp_eval (k_sqp_begin,
// k_sqp_stage, k_ipm_post_ride, k_armijo<ARMIJO_NLP>, k_acopf_eval_point) get one call behind a branch uniform over the launch.
#pragma once
// (NlpBlkDev: nlp_dev.hpp, in front of NlpDev, which holds the blocks)

namespace sqphip {

static __device__ __forceinline__ double nlp_wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// kappa, kappa', kappa'' at u to w[0], w[1], w[2] (nd: how many derivatives) by the code of the factors.  Out of line: inlined
// into nlp_block_eval, the menu costs that function 128 registers and 300 B of scratch per lane, which every kernel that
// calls it would carry; w is the thread's own place in the instance's workspace in HBM, not a private array.
static __device__ __noinline__ void nlp_block_kappa(int ke, double u, double pw, int nd, double *__restrict__ w)
{
    nlp_factor(ke, 1.0, u, pw, nd >= 1, nd >= 2, w, 1, 0);
}

// An argument of an out-of-line function arrives in vector registers.  These are the same in every lane: moved to scalar
// registers they stay out of the vector registers that live across the call of nlp_block_kappa and would be saved to scratch.
template <class T> static __device__ __forceinline__ T *nlp_uniform(T *p)
{
    const unsigned long v = (unsigned long)p;
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
    return (T *)(((unsigned long)hi << 32) | lo);
}

// val: the instance's block of values; wsp: its workspace; part: [TPB / 64] wave sums of the instance, then [TPB][3] kappa, kappa', kappa'' of the point a thread is at
static __device__ __noinline__ void nlp_block_eval(const NlpBlkDev *bp_, const double *val_, double *wsp_, double *part_,
                                                   const double *x_, double sigma, double *f_out_, double *grad_, double *hv_)
{
    const NlpBlkDev *__restrict__ bp = nlp_uniform(bp_);
    const double *__restrict__ val = nlp_uniform(val_), *__restrict__ x = nlp_uniform(x_);
    double *__restrict__ wsp = nlp_uniform(wsp_), *__restrict__ part = nlp_uniform(part_);
    double *f_out = nlp_uniform(f_out_), *grad = nlp_uniform(grad_), *hv = nlp_uniform(hv_);
    typedef double d4 __attribute__((ext_vector_type(4)));
    const int N = bp->N, d = bp->d, ke = bp->ke;
    const double pw = bp->par;
    const double *__restrict__ A = bp->A, *__restrict__ At = bp->At;
    const int *__restrict__ col = bp->col;
    const double *__restrict__ W = val + bp->ow, *__restrict__ S = val + bp->os;
    double *__restrict__ z1 = wsp + bp->wz, *__restrict__ z2 = z1 + N;
    const bool d1 = grad || hv, d2 = hv != nullptr;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    double f = 0.0;
    #pragma unroll 1
    for (int i = threadIdx.x; i < N; i += TPB) {
        double u = 0.0;
        #pragma unroll 1
        for (int j = 0; j < d; ++j) u = fma(At[(long)j * N + i], x[col[j]], u);
        u += S[i];
        double *__restrict__ k3 = part + TPB / 64 + 3 * threadIdx.x;
        nlp_block_kappa(ke, u, pw, (int)d1 + (int)d2, k3);
        const double wi = W[i];
        f += wi * k3[0];
        if (grad) z1[i] = wi * k3[1];
        if (d2) z2[i] = wi * k3[2];
    }
    if (f_out) {
        f = nlp_wave_sum(f);
        if (lane == 0) part[wv] = f;
    }
    __syncthreads();                        // z1, z2 and the wave sums are complete
    if (f_out && threadIdx.x == 0) {
        double r = part[0];
        #pragma unroll 1
        for (int w = 1; w < TPB / 64; ++w) r += part[w];
        *f_out += r;
    }
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
        const int *__restrict__ hs = bp->hs;
        const int nt = (d + 15) >> 4, T = nt * (nt + 1) / 2;
        const int l15 = lane & 15, l4 = lane >> 4;
        #pragma unroll 1
        for (int t = wv; t < T; t += TPB / 64) {
            int R = 0;
            while ((R + 1) * (R + 2) / 2 <= t) ++R;
            const int Cc = t - R * (R + 1) / 2;
            const int cr = 16 * R + l15, cc = 16 * Cc + l15;
            const bool okr = cr < d, okc = cc < d;
            d4 acc = {0.0, 0.0, 0.0, 0.0};
            #pragma unroll 2
            for (int p0 = 0; p0 < N; p0 += 4) {
                const int p = p0 + l4;
                const bool okp = p < N;
                const double a = okp && okr ? z2[p] * A[(long)p * d + cr] : 0.0;
                const double b = okp && okc ? A[(long)p * d + cc] : 0.0;
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
            }
            // D[i][j] = sum_k a[i][k] b[k][j]: this lane holds the rows l4 + 4 q, q = 0 .. 3, of column l15
            #pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int r = 16 * R + l4 + 4 * q;
                if (r < d && cc <= r) {
                    const int s = hs[r * (r + 1) / 2 + cc];
                    if (s >= 0) hv[s] += sigma * acc[q];
                }
            }
        }
    }
}

}  // namespace sqphip
