// nlp_blocks_dev.hpp -- what the dense data blocks of a factorable NLP share.  Six families, one evaluator each in a header of
// its own; nlp_dev.hpp includes this header, then the six, and holds their dispatcher nlp_blocks_eval behind them:
//     NLP_BLK_SCALAR   nlp_block_eval      nlp_block_dev.hpp       sum_i W_i kappa(u_i) in the objective
//     NLP_BLK_ROWS     nlp_rowblock_eval   nlp_rowblock_dev.hpp    R <= 8 weight vectors on one pass, a target row each
//     NLP_BLK_SOFTMAX  nlp_softmax_eval    nlp_softmax_dev.hpp     multinomial log-likelihood
//     NLP_BLK_COX      nlp_cox_eval        nlp_cox_dev.hpp         Cox partial likelihood
//     NLP_BLK_LSE      nlp_lse_eval        nlp_lse_dev.hpp         log-sum-exp rows over segments of the points
//     NLP_BLK_NORM     nlp_norm_eval       nlp_norm_dev.hpp        Euclidean norms over segments of the points, several per row
// A family header keeps its mathematics, its order-of-summation contract and the layout of its workspace (nlp_*_ws, read by the
// evaluator and by the add call of api_models.hip alike); the steps below are described here once.
//   logit      u_i = 0, u_i = fma(At[j][i], x_{col_j}, u_i) for j = 0 .. d - 1 in that order, u_i += S_i: the rule of
//              sqphip_nlp_attach_affine.  A is read through its transpose At [d][N], so the lanes of a wave read consecutive doubles.
//   sum        a workgroup's sum of one double per thread, the pattern of block_reduce: the xor butterfly 32, 16, .. 1 within a
//              wave, lane 0 stores the wave's sum in part[wave], a barrier, thread 0 adds the sixteen wave sums in wave order.
//   Hessian    the lower 16 x 16 tiles (R, C), C <= R, of a D x D matrix, numbered R (R + 1) / 2 + C, tile t on wave t % 16.  A tile
//              is accumulated by chains of v_mfma_f64_16x16x4_f64 (D[i][j] = sum_k a[i][k] b[k][j], four k per instruction); lane l
//              feeds row 16 R + l % 16 (a operand) and column 16 C + l % 16 (b operand) of k = l / 16 and ends up holding rows
//              16 R + l / 16 + 4 q, q = 0 .. 3, of column 16 C + l % 16.  Rows and columns >= D enter as zeros.  The lane that
//              holds a lower entry (r, c) adds the family's combination of its accumulators to the entry's COO slot (NlpBlkDev::hs).
// Every function takes pointers and scalars only, never DV.  The evaluators and the dispatcher are out of line: the kernels that
// inline nlp_eval (k_sqp_begin, k_sqp_stage, k_ipm_post_ride, k_armijo<ARMIJO_NLP>, k_acopf_eval_point) get one call behind a
// branch uniform over the launch.
#pragma once
// (NlpBlkDev, nlp_factor: nlp_dev.hpp, which includes this header behind them)

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

static __device__ __forceinline__ double nlp_uniform(double v)
{
    const unsigned long b = (unsigned long)__double_as_longlong(v);
    return __longlong_as_double((long long)(((unsigned long)(unsigned)__builtin_amdgcn_readfirstlane((unsigned)(b >> 32)) << 32) |
                                            (unsigned)__builtin_amdgcn_readfirstlane((unsigned)b)));
}

// exp and log out of line: inlined, the constants of their polynomials stay in vector registers across the loop over the points
// (36 of them), nlp_softmax_eval needs callee-saved registers and every kernel that inlines nlp_eval carries a 108 B frame for it
static __device__ __noinline__ double nlp_block_exp(double v) { return exp(v); }
static __device__ __noinline__ double nlp_block_log(double v) { return log(v); }

// the logit of point i (col: the d variables of the columns, S: the N shifts)
static __device__ __forceinline__ double nlp_block_logit(const double *__restrict__ At, const double *__restrict__ x,
                                                         const int *__restrict__ col, const double *__restrict__ S, int N, int d, int i)
{
    double u = 0.0;
    #pragma unroll 1
    for (int j = 0; j < d; ++j) u = fma(At[(long)j * N + i], x[col[j]], u);
    return u + S[i];
}

// the sum in two halves, for a caller whose barrier between them publishes more than one sum: a thread's f into its wave's place ...
static __device__ __forceinline__ void nlp_block_sum_put(double f, double *part, int wave)
{
    f = nlp_wave_sum(f);
    if ((threadIdx.x & 63) == 0) part[wave] = f;
}

// ... and, behind a barrier, the wave sums in wave order (thread 0's business)
static __device__ __forceinline__ double nlp_block_sum_get(const double *part)
{
    double r = part[0];
    #pragma unroll 1
    for (int w = 1; w < TPB / 64; ++w) r += part[w];
    return r;
}

// the sum of every thread's f added to *out (null: nothing is summed).  The barrier is met by every thread either way, and the
// caller may rely on it for arrays of its own.
static __device__ __forceinline__ void nlp_block_sum_out(double f, double *part, int wave, double *out)
{
    if (out) nlp_block_sum_put(f, part, wave);
    __syncthreads();
    if (out && threadIdx.x == 0) *out += nlp_block_sum_get(part);
}

// where a lane stands in a tile of the Hessian walk: the tile, the lane's l % 16 and l / 16, the row of its a operand and the
// column of its b operands and of its outputs, and whether these lie inside the matrix
struct NlpTile {
    int R, C, l15, l4, cr, cc;
    bool okr, okc;
};
typedef double nlp_d4 __attribute__((ext_vector_type(4)));

// The walk over the lower tiles of a D x D Hessian by wave `wave` of the workgroup.  body(tile) runs the family's accumulator
// chain(s) for one tile; combine(q, r) then gives what the lane adds to the slot of the lower entry (r = 16 R + l / 16 + 4 q,
// tile.cc) from element q of its accumulators.  Both are the caller's closures over its own accumulators, so a family may keep
// whatever it needs of a tile between the two (the softmax: the class of the lane's column).
template <class Body, class Combine>
static __device__ __forceinline__ void nlp_block_hess_tiles(int D, int wave, const int *__restrict__ hs, double *hv, Body body, Combine combine)
{
    const int lane = threadIdx.x & 63;
    const int nt = (D + 15) >> 4, T = nt * (nt + 1) / 2;
    const int l15 = lane & 15, l4 = lane >> 4;
    #pragma unroll 1
    for (int t = wave; t < T; t += TPB / 64) {
        int R = 0;
        while ((R + 1) * (R + 2) / 2 <= t) ++R;
        const int Cc = t - R * (R + 1) / 2;
        const int cr = 16 * R + l15, cc = 16 * Cc + l15;
        const NlpTile tile = {R, Cc, l15, l4, cr, cc, cr < D, cc < D};
        body(tile);
        #pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int r = 16 * R + l4 + 4 * q;
            if (r < D && cc <= r) {
                const int s = hs[r * (r + 1) / 2 + cc];
                if (s >= 0) hv[s] += combine(q, r);
            }
        }
    }
}

}  // namespace sqphip
