// api.hip -- the extern "C" boundary of libsqphip.so (declared in include/sqphip.h).
// Builds the shared sparsity structure once on the host (what `sparse(I,J,V)` does in
// /root/reference/src/algorithms/sqp_trust_region.jl:47-48,56-57 plus the symmetric mirroring of
// sqp.jl:96-101), lays the batch out in HBM and forwards to the kernels.
#include "api_util.hpp"
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <tuple>

using namespace sqphip;

Ctx::~Ctx()
{
    lanes.clear();              // before the arenas they point into
    tm.flush();
    comm_release(*this);
    plan.destroy_lookahead();
    for (void *p : allocs) hipFree(p);
    if (h_counters) hipHostFree(h_counters);
    if (stg_h) hipHostFree(stg_h);
    if (side) { hipStreamDestroy(side); for (auto &e : evS) if (e) hipEventDestroy(e); for (auto &e : evC) if (e) hipEventDestroy(e); }
    if (stream && owns_stream) hipStreamDestroy(stream);
}

namespace {

struct Pattern {
    std::vector<int> colptr, rowval, g_ptr, g_src;     // CSC + per-slot gather lists over COO indices
};

Pattern build_pattern(int64_t ncols, int64_t nnz, const int64_t *row, const int64_t *col, bool sym)
{
    std::vector<std::tuple<int64_t, int64_t, int64_t>> e;   // (col, row, coo index)
    e.reserve(sym ? 2 * nnz : nnz);
    for (int64_t k = 0; k < nnz; ++k) {
        e.emplace_back(col[k] - 1, row[k] - 1, k);
        if (sym && row[k] != col[k]) e.emplace_back(row[k] - 1, col[k] - 1, k);
    }
    std::sort(e.begin(), e.end());
    Pattern P;
    P.colptr.assign(ncols + 1, 0);
    P.g_ptr.push_back(0);
    for (size_t i = 0; i < e.size(); ++i) {
        const bool fresh = i == 0 || std::get<0>(e[i]) != std::get<0>(e[i - 1]) ||
                           std::get<1>(e[i]) != std::get<1>(e[i - 1]);
        if (fresh) {
            if (i) P.g_ptr.push_back((int)P.g_src.size());
            P.rowval.push_back((int)std::get<1>(e[i]));
            P.colptr[std::get<0>(e[i]) + 1]++;
        }
        P.g_src.push_back((int)std::get<2>(e[i]));
    }
    P.g_ptr.push_back((int)P.g_src.size());
    if (e.empty()) P.g_ptr.assign(1, 0);
    for (int64_t j = 0; j < ncols; ++j) P.colptr[j + 1] += P.colptr[j];
    return P;
}

// the device view of instances [i0, i0 + Bg): every per-instance array advanced to the group's first instance, so that
// the kernels see an ordinary (smaller) batch.  Shared structure arrays stay as they are.
DV group_view(const DV &d, int i0, int Bg, int g)
{
    DV v = d;
    v.B = Bg;
    const long n = d.n, m = d.m, o = i0;
    double **nv[] = { &v.xL, &v.xU, &v.xk, &v.cin, &v.c, &v.hd, &v.lb, &v.ub, &v.p, &v.zl, &v.zu, &v.dp, &v.dzl, &v.dzu, &v.rd,
                      &v.sigp, &v.wn, &v.op, &v.omxU, &v.omxL, &v.x, &v.mxL, &v.mxU, &v.df, &v.pstep, &v.psoc, &v.pmxL,
                      &v.pmxU, &v.tmpx, &v.x0, &v.socZL, &v.socZU };
    for (auto pp : nv) *pp += o * n;
    double **mv[] = { &v.gL, &v.gU, &v.bE, &v.lo, &v.hi, &v.wp, &v.wm, &v.s, &v.tp, &v.tm, &v.y, &v.vl, &v.vu, &v.ds, &v.dtp,
                      &v.dtm, &v.dy, &v.dvl, &v.dvu, &v.rp, &v.Dd, &v.olam, &v.lambda, &v.E, &v.plam, &v.Esoc, &v.tmpE,
                      &v.hlam, &v.zp, &v.zm, &v.rdir, &v.socZP, &v.socZM, &v.socVL, &v.socVU };
    for (auto pp : mv) *pp += o * m;
    v.oslack += 2 * o * m;
    v.rtype += o * m; v.rbase += o * m; v.hard += o * m;
    v.jcoo += o * d.nnzj_coo; v.hcoo += o * d.nnzh_coo; v.jv += o * d.nnzjc; v.hv += o * d.nnzhc;
    v.rhs += o * d.Npad; v.sol += o * d.Npad; v.wN += o * d.Npad;
    if (v.flat) { v.fH += o * n; v.fJt += o * n; v.fJ += o * m; v.fX += o * m; }
    v.xv += o * d.Fpad; v.vv += o * d.Fpad; v.dinv += o * d.Fpad;
    v.ist += o; v.sst += o; v.phase += o;
    if (v.stream.slot_scen) v.stream.slot_scen += o;
    v.trace += o * SQPHIP_TRACE_CAP * SQPHIP_TRACE_COLS;
    v.counters = d.counters + 8 * (g + 1);
    if (v.br_ohm) { v.br_ohm += o * d.nl * 12; v.c2 += o * d.ng; v.c1 += o * d.ng; }
    if (v.dnc) v.dnc += o * n;
    v.mf.fronts += o * d.mf.stride; v.mf.vals += o * (long)d.mf.nnzK;
    if (v.mf.fronts1) { v.mf.fronts1 += o * d.mf.stride; v.mf.vals1 += o * (long)d.mf.nnzK; v.dinv1 += o * d.Fpad; v.vv1 += o * d.Fpad; }
    return v;
}

}  // namespace

// (re)build the lanes from the owner's current device view (after sqphip_create and after every *_attach)
void sqphip::make_lanes(Ctx &C)
{
    for (const auto &L : C.lanes)           // (the launch census of the groups being replaced stays with the context)
        for (int k = 0; k < MFK_COUNT; ++k) C.mf_census[k] += L->mf_census[k];
    for (const auto &L : C.lanes) C.n_trans_inline += L->n_trans_inline;
    C.lanes.clear();
    int G = 1;
    // (round 3, with the shorter solve kernels: four groups from 64 instances on -- 64 resident scenarios 1 955 -> 2 015 QP/s;
    //  SQPHIP_GROUP_RULE=<g32>,<g16>: groups for batches of 32 .. 63 and 16 .. 31, experiment)
    if (C.d.sparse) {
        int g32 = 4, g16 = 2;           // (32 resident scenarios: 1 034 / 1 074 / 1 119 QP/s with one / two / four groups)
        if (const char *e = getenv("SQPHIP_GROUP_RULE")) sscanf(e, "%d,%d", &g32, &g16);
        G = C.d.B >= 64 ? 4 : (C.d.B >= 32 ? g32 : (C.d.B >= 16 ? g16 : 1));
    }
    if (const char *e = getenv("SQPHIP_GROUPS")) G = atoi(e);
    if (G > C.d.B) G = C.d.B;
    if (G > 7) G = 7;                       // counter slots
    if (!C.d.sparse || G < 2) return;
    for (int g = 0; g < G; ++g) {
        const int lo = (int)((long)C.d.B * g / G), hi = (int)((long)C.d.B * (g + 1) / G);
        std::unique_ptr<Ctx> L(new Ctx());
        L->is_lane = true;
        L->opt = C.opt; L->n = C.n; L->m = C.m; L->evaluator_attached = C.evaluator_attached;
        L->mfp_ = C.mfp_;
        L->trans_period = C.trans_period; L->trans_ride = C.trans_ride; L->refine_slot = C.refine_slot; L->refine_period = C.refine_period; L->mf_big_lds = C.mf_big_lds; L->post_split = C.post_split; L->side_mode = C.side_mode; L->spec_tail = C.spec_tail; L->spec_mode0 = C.spec_mode0;
        L->d = group_view(C.d, lo, hi - lo, g);
        if (L->d.qcv) L->d.qcv += (long)lo * C.qc.nv;
        if (L->d.nlv) { L->d.nlv += (long)lo * C.nl.nv; L->d.nlw += (long)lo * C.nl.ws; }
        // the first group runs on the owner's stream (idle during sqphip_sqp_run): HIP maps streams onto four hardware
        // queues by default, and a fifth stream would share one -- measured: 3131 QP/s with five streams against 5216
        // with four (or with GPU_MAX_HW_QUEUES=8)
        // (experiment, SQPHIP_CU_PARTITION = 1 | 2: every group on a stream restricted to a quarter of the CUs -- 1: a contiguous
        //  quarter of the mask bits, 2: every G-th bit -- so that one group's throughput-bound launches cannot slow another group's
        //  latency-bound ones; measured: profiles/r04_ab_experiments.txt)
        static const int cu_part = getenv("SQPHIP_CU_PARTITION") ? atoi(getenv("SQPHIP_CU_PARTITION")) : 0;
        if (cu_part != 0) {
            hipDeviceProp_t prop; SQPHIP_HIP_OK(hipGetDeviceProperties(&prop, C.opt.device));
            const int ncu = prop.multiProcessorCount, words = (ncu + 31) / 32;
            std::vector<uint32_t> mask(words, 0u);
            for (int c = 0; c < ncu; ++c) {
                const bool mine = cu_part == 1 ? (c * G / ncu == g) : (c % G == g);
                if (mine) mask[c / 32] |= 1u << (c % 32);
            }
            SQPHIP_HIP_OK(hipExtStreamCreateWithCUMask(&L->stream, (uint32_t)words, mask.data()));
        } else
        if (g == 0) { L->stream = C.stream; L->owns_stream = false; }
        else SQPHIP_HIP_OK(hipStreamCreateWithFlags(&L->stream, getenv("SQPHIP_STREAM_BLOCKING") ? hipStreamDefault : hipStreamNonBlocking));
        SQPHIP_HIP_OK(hipHostMalloc((void **)&L->h_counters, 8 * sizeof(int)));
        L->tm.enabled = C.tm.enabled;
        C.lanes.push_back(std::move(L));
    }
}

namespace {

__global__ void k_qp_request(DV d, int inst, int mode, double delta, double mu_pen)
{
    for (int i = threadIdx.x; i < d.B; i += blockDim.x) d.ist[i].start = 0;
    __syncthreads();
    if (threadIdx.x == 0) {
        IpmState &I = d.ist[inst];
        I.mode = mode; I.delta = delta; I.mu_pen = mu_pen;
        I.stage = 0; I.rho_big = 1e4; I.start = 1; I.ipm_iters = 0; I.n_factor = 0; I.n_solve = 0; I.status = 0;
    }
}

// the same for the requests of sqphip_qp_solve_batch: instances inst[0 .. count) (pairwise distinct, checked on the host) with
// their own mode, radius and penalty; every other instance loses its start flag and keeps everything else.  One workgroup,
// strided over the batch and over the requests (either may exceed the workgroup).
__global__ __launch_bounds__(256) void k_qp_request_batch(DV d, int count, const int *inst, const int *mode, const double *delta,
                                                          const double *mu_pen)
{
    for (int i = threadIdx.x; i < d.B; i += blockDim.x) d.ist[i].start = 0;
    __syncthreads();
    for (int k = threadIdx.x; k < count; k += blockDim.x) {
        IpmState &I = d.ist[inst[k]];
        I.mode = mode[k]; I.delta = delta[k]; I.mu_pen = mu_pen[k];
        I.stage = 0; I.rho_big = 1e4; I.start = 1; I.ipm_iters = 0; I.n_factor = 0; I.n_solve = 0; I.status = 0;
    }
}

// Staging of the batched seat.  A call packs its operands on the host into one pinned buffer, request
// after request: row k holds the fields of request k back to back, every field padded to an even number of doubles, so that
// rows and fields start on 16-byte boundaries.  One copy moves the buffer, then k_seat_stage<true> spreads row k over the
// slots of instance inst[k] (field f -> base[f] + inst[k] * stride[f]); k_seat_stage<false> collects results the other way,
// and the IpmState of every listed instance behind the rows.  Streaming copies: 16-byte loads from / stores to staging, and
// to / from a slot where the slot is aligned (n, m or the nnz odd: every other instance is not), two 8-byte ones otherwise.
#define SQPHIP_SEAT_FIELDS 8
struct StageMap {
    int nf, row;                                  // fields in use; doubles per row (even)
    int len[SQPHIP_SEAT_FIELDS], off[SQPHIP_SEAT_FIELDS], stride[SQPHIP_SEAT_FIELDS];   // off < 0 (to the slots only): zeros
    double *base[SQPHIP_SEAT_FIELDS];
    const IpmState *ist;                          // from the slots only, may be null: the states go to stg + ist_off,
    long ist_off;                                 // sizeof(IpmState) / 8 doubles each
};

template <bool TO_SLOTS>
__global__ __launch_bounds__(256) void k_seat_stage(StageMap M, double *stg, const int *inst)
{
    const int k = blockIdx.y, b = inst[k];
    double *row = stg + (long)k * M.row;
#pragma unroll
    for (int f = 0; f < SQPHIP_SEAT_FIELDS; ++f) {
        if (f >= M.nf) break;
        const int len = M.len[f];
        double *slot = M.base[f] + (long)b * M.stride[f];
        const bool al = ((unsigned long)slot & 15ul) == 0;
        for (int q = blockIdx.x * 256 + threadIdx.x; 2 * q < len; q += gridDim.x * 256) {
            const bool two = 2 * q + 1 < len;
            if (TO_SLOTS) {
                const double2 v = M.off[f] < 0 ? make_double2(0.0, 0.0) : *(const double2 *)(row + M.off[f] + 2 * q);
                if (two && al) *(double2 *)(slot + 2 * q) = v;
                else { slot[2 * q] = v.x; if (two) slot[2 * q + 1] = v.y; }
            } else {
                double2 v;
                if (two && al) v = *(const double2 *)(slot + 2 * q);
                else { v.x = slot[2 * q]; v.y = two ? slot[2 * q + 1] : 0.0; }
                *(double2 *)(row + M.off[f] + 2 * q) = v;
            }
        }
    }
    if (!TO_SLOTS && M.ist && blockIdx.x == 0) {
        constexpr int W = (int)(sizeof(IpmState) / 8);
        const unsigned long long *src = (const unsigned long long *)(M.ist + b);    // (bit copies)
        unsigned long long *dst = (unsigned long long *)(stg + M.ist_off) + (long)k * W;
        for (int w = threadIdx.x; w < W; w += 256) dst[w] = src[w];
    }
}
static_assert(sizeof(IpmState) % 8 == 0, "k_seat_stage copies IpmState in 8-byte words");

// test hook (sqphip_mf_solve_test): instance `inst` alone enters phase `ph` with the given Hessian scale / delta_w
__global__ void k_mf_test_setup(DV d, int inst, double hsc, double dw, int ph)
{
    for (int i = threadIdx.x; i < d.B; i += blockDim.x) { d.phase[i] = PH_IDLE; d.ist[i].start = 0; }
    __syncthreads();
    if (threadIdx.x == 0) { d.ist[inst].hsc = hsc; d.ist[inst].dw = dw; d.ist[inst].stage = 0; d.ist[inst].sel = 0; d.ist[inst].fac_attempt = 0; d.phase[inst] = ph; }
}

// test hook (sqphip_mf_batch_test): instance `inst` on its own -- a start request (start = 1: k_qp_gather converts its COO
// values) or the interior-point state a sweep factorises with: phase `ph`, Hessian scale, delta_w, the last accepted delta_w
// and the failed factorisations so far
__global__ void k_mf_inst_set(DV d, int inst, int start, int ph, double hsc, double dw, double dw_last, int fac_attempt)
{
    if (threadIdx.x != 0) return;
    IpmState &I = d.ist[inst];
    I.start = start;
    if (start) { I.mode = 0; I.delta = 1.0; I.mu_pen = 1.0; I.rho_big = 1e4; I.ipm_iters = 0; I.n_solve = 0; I.status = 0; }
    I.stage = 0; I.hsc = hsc; I.dw = dw; I.dw_last = dw_last; I.sel = 0; I.fac_attempt = fac_attempt; I.n_factor = 0; I.rc = 0;
    d.phase[inst] = ph;
}

}  // namespace

extern "C" void sqphip_default_options(sqphip_options *o)
{
    // /root/reference/src/parameters.jl:17-29
    o->tol_direction = 1e-8; o->tol_residual = 1e-8; o->tol_infeas = 1e-8;
    o->init_mu = 1.0; o->max_mu = 1e10; o->tr_size = 10.0;
    o->rho = 0.8; o->eta = 0.4; o->tau = 0.9; o->min_alpha = 1e-6;
    o->max_iter = 3000; o->use_soc = 0; o->literal_quirks = 1;
    o->ipm_tol = 1e-9; o->ipm_max_iter = 200; o->ipm_phase1 = 0; o->device = 0; o->ipm_corrector = 0; o->kkt_condense = 1; o->kkt_tile_order = 1;
    o->kkt_mode = 0; o->ipm_warm_start = 0;
}

extern "C" int sqphip_create(sqphip_ctx **out, int64_t n, int64_t m, int64_t num_linear, int64_t nnzJ,
                             const int64_t *jrow, const int64_t *jcol, int64_t nnzH, const int64_t *hrow,
                             const int64_t *hcol, const double *xL, const double *xU, const double *gL,
                             const double *gU, const sqphip_options *opt, int32_t batch)
{
    if (!out || n <= 0 || m < 0 || batch <= 0 || !opt || num_linear < 0 || num_linear > m) return SQPHIP_EINVAL;
    if (nnzJ < 0 || nnzH < 0 || (nnzJ > 0 && (!jrow || !jcol)) || (nnzH > 0 && (!hrow || !hcol))) return SQPHIP_EINVAL;
    if (!xL || !xU || (m > 0 && (!gL || !gU))) return SQPHIP_EINVAL;
    for (int64_t k = 0; k < nnzJ; ++k)
        if (jrow[k] < 1 || jrow[k] > m || jcol[k] < 1 || jcol[k] > n) return SQPHIP_EINVAL;
    for (int64_t k = 0; k < nnzH; ++k)
        if (hrow[k] < 1 || hrow[k] > n || hcol[k] < 1 || hcol[k] > n) return SQPHIP_EINVAL;
    // rows unbounded on both sides create no constraint upstream and shift its indexing
    // (SURVEY.md App. C #15): rejected
    for (int64_t i = 0; i < m; ++i)
        if (gL[i] == -INFINITY && gU[i] == INFINITY) return SQPHIP_EINVAL;
    sqphip_ctx *h = new (std::nothrow) sqphip_ctx();
    if (!h) return SQPHIP_ENOMEM;
    h->c.opt = *opt;
    int rc = guarded(h, [&](Ctx &C) {
        SQPHIP_HIP_OK(hipStreamCreate(&C.stream));
        SQPHIP_HIP_OK(hipHostMalloc((void **)&C.h_counters, 8 * sizeof(int)));
        DV &d = C.d;
        std::memset(&d, 0, sizeof(d));
        C.n = n; C.m = m;
        C.h_jrow.assign(jrow, jrow + nnzJ); C.h_jcol.assign(jcol, jcol + nnzJ);
        C.h_hrow.assign(hrow, hrow + nnzH); C.h_hcol.assign(hcol, hcol + nnzH);
        C.h_xL.assign(xL, xL + n); C.h_xU.assign(xU, xU + n);
        if (m > 0) { C.h_gL.assign(gL, gL + m); C.h_gU.assign(gU, gU + m); }
        const int B = batch;
        d.n = (int)n; d.m = (int)m; d.nlin = (int)num_linear; d.N = (int)(n + m);
        d.Npad = (d.N + 63) / 64 * 64; d.B = B;
        d.nnzj_coo = (int)nnzJ; d.nnzh_coo = (int)nnzH;
        Pattern PJ = build_pattern(n, nnzJ, jrow, jcol, false);
        Pattern PH = build_pattern(n, nnzH, hrow, hcol, true);
        d.nnzjc = (int)PJ.rowval.size(); d.nnzhc = (int)PH.rowval.size();
        d.hfull = n > 1 && (long)d.nnzhc == (long)n * n;
        // CSR view of J
        std::vector<int> rptr(m + 1, 0), rcol(d.nnzjc), rslot(d.nnzjc);
        for (int s = 0; s < d.nnzjc; ++s) rptr[PJ.rowval[s] + 1]++;
        for (int64_t i = 0; i < m; ++i) rptr[i + 1] += rptr[i];
        {
            std::vector<int> fill(rptr.begin(), rptr.end() - 1);
            for (int j = 0; j < (int)n; ++j)
                for (int s = PJ.colptr[j]; s < PJ.colptr[j + 1]; ++s) {
                    const int i = PJ.rowval[s];
                    rcol[fill[i]] = j; rslot[fill[i]] = s; fill[i]++;
                }
        }
        d.jcolptr = C.upload(PJ.colptr); d.jrowval = C.upload(PJ.rowval);
        d.jrowptr = C.upload(rptr); d.jrcol = C.upload(rcol); d.jrslot = C.upload(rslot);
        {   // condensed form: the equality rows (and rows too long to eliminate, sparse.hpp) stay in the factorised
            // matrix, all others are eliminated
            std::vector<int> kpos(m > 0 ? m : 1, -1), krow;
            for (int64_t i = 0; i < m; ++i)
                if (kkt_row_is_kept(gL[i], gU[i], rptr[i + 1] - rptr[i])) { kpos[i] = (int)krow.size(); krow.push_back((int)i); }
            d.condense = opt->kkt_condense != 0; d.mk = (int)krow.size();
            if (krow.empty()) krow.push_back(0);
            d.kpos = C.upload(kpos); d.krow = C.upload(krow);
            C.h_kpos = kpos;
        }
        {   // linear solver and order of the factorised matrix
            const std::vector<int> &kpos = C.h_kpos;
            const int nu = d.condense ? d.n + d.mk : d.N;       // unknowns of the factorised system
            std::vector<int> upos(nu);
            d.Ts = 0; d.Nf = nu; d.sparse = 0;
            if (opt->kkt_mode != 1) {
                // multifrontal plan of the sparse matrix (full form: every row is its own unknown)
                std::vector<int> kp(kpos);
                if (!d.condense) for (int64_t i = 0; i < m; ++i) kp[i] = (int)i;
                const SymOptions so = mf_sym_options(B);   // (small batches: one launch per level of small fronts, mfplan.hip)
                C.mfp_ = std::make_shared<MfPlan>(mf_build_plan(d.n, (int)m, kp, d.condense ? d.mk : (int)m, PH.colptr, PH.rowval, rptr, rcol, rslot, so));
                const SparseSym &S = C.mfp().S;
                // auto: the sparse factorisation when it does a quarter of the dense work or less and no front
                // outgrows what one workgroup eliminates in reasonable time; a dense Hessian goes to the MFMA path
                const double dense_flops = (double)nu * nu * nu / 3.0;
                const bool fits = S.max_front <= 1024;
                if (opt->kkt_mode == 2 && !fits) throw std::string("kkt_mode = 2: a front of " + std::to_string(S.max_front) + " rows exceeds the multifrontal kernels' limit (1024)");
                d.sparse = opt->kkt_mode == 2 || (fits && S.max_front <= 512 && S.flops <= 0.25 * dense_flops);
            }
            if (d.sparse) {
                const MfPlan &P = C.mfp();
                const SparseSym &S = P.S;
                upos = S.pos;
                MfDev &M = d.mf;
                M.ns = S.ns; M.stride = P.stride;
                M.first = C.upload(S.sn_first); M.nc = C.upload(S.sn_nc); M.nr = C.upload(S.sn_nr);
                M.rowptr = C.upload(S.sn_rowptr); M.rows = C.upload(S.sn_rows.empty() ? std::vector<int>(1, 0) : S.sn_rows);
                M.rel = C.upload(S.rel.empty() ? std::vector<int>(1, 0) : S.rel);
                M.child_ptr = C.upload(S.child_ptr); M.child = C.upload(S.child.empty() ? std::vector<int>(1, 0) : S.child);
                M.off = C.upload(P.off);
                M.asm_ptr = C.upload(P.asm_ptr); M.dest_loc = C.upload(P.dest_loc); M.item_ptr = C.upload(P.item_ptr);
                M.items = C.upload(P.items); M.sched = C.upload(P.sched);
                M.nvblk = (int)P.vblk.size();
                if (M.nvblk > 0) { M.vitems = C.upload(P.vitems); M.vblk = C.upload(P.vblk); }
                auto nz = [](const std::vector<int> &v) { return v.empty() ? std::vector<int>(1, 0) : v; };
                M.dest_rc = C.upload(P.dest_rc);
                M.ea_ptr = C.upload(P.ea_ptr); M.ea_rc = C.upload(nz(P.ea_rc));
                M.ea_src_ptr = C.upload(P.ea_src_ptr); M.ea_src = C.upload(nz(P.ea_src));
                M.ev_ptr = C.upload(P.ev_ptr); M.ev_idx = C.upload(nz(P.ev_idx));
                M.ev_src_ptr = C.upload(P.ev_src_ptr); M.ev_src = C.upload(nz(P.ev_src));
                M.level_ptr = C.upload(S.level_ptr); M.level_sn = C.upload(S.level_sn);
                M.nlevels = S.nlevels; M.max_front = S.max_front;
                M.sol_items = C.upload(nz(P.sol_items));
                M.desc = C.upload(P.desc);
                M.ea_ent = C.upload(P.ea_ent.empty() ? std::vector<MfGather>(1) : P.ea_ent);
                M.ev_ent = C.upload(P.ev_ent.empty() ? std::vector<MfGather>(1) : P.ev_ent);
                int lds_max = 0;                 // LDS a workgroup may have on this device (gfx950: 160 KB)
                if (hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, C.opt.device) != hipSuccess) lds_max = 0;
                M.top_n = P.top2_lds_bytes > 0 && P.top2_lds_bytes <= lds_max ? (int)P.top_fr.size() : 0;
                if (M.top_n > 0) {
                    M.top_fr = C.upload(P.top_fr); M.top_gptr = C.upload(P.top_gptr); M.top_gsrc = C.upload(nz(P.top_gsrc));
                    M.top_rows = C.upload(nz(P.top_rows)); M.top_ext = C.upload(nz(P.top_ext));
                    M.top_next = (int)P.top_ext.size(); M.top_utotal = P.top_utotal; M.top_xtotal = P.top_xtotal;
                    M.top_buf0 = P.top_buf0; M.top_buf1 = P.top_buf1;
                }
                M.sp_n = P.spine_lds_bytes > 0 && P.spine_lds_bytes <= lds_max ? (int)P.sp_fr.size() : 0;
                if (M.sp_n > 0) {
                    M.sp_fr = C.upload(P.sp_fr); M.sp_ent = C.upload(P.sp_ent.empty() ? std::vector<MfGather>(1) : P.sp_ent);
                    M.sp_src = C.upload(nz(P.sp_src)); M.sp_rel = C.upload(nz(P.sp_rel)); M.sp_T = P.spine_T; M.sp_stage = P.spine_stage;
                }
                M.nnzK = (int)P.nnzK;
                M.vals = C.dalloc<double>((size_t)B * P.nnzK);
                M.fronts = C.dalloc<double>((size_t)B * P.stride);
                // Second candidate of a sweep (the speculative next shift, k_inertia / dev_util.hpp): a failed first shift then
                // costs no extra sweep.  It pays while a sweep is bound by the latency of its kernel chain -- up to ~256
                // resident instances (+15 % QP/s at 64, +8 % at 128, +6.5 % at 256) -- and costs once the front kernels are
                // throughput-bound (-5 % at 512).  SQPHIP_MF_SPEC: 0 off, 1 shrink attempts and retries, 2 retries only.
                // Large matrices (1354 / 9241 buses) rarely fail a shrink attempt and gain nothing (measured): the second
                // arena is only spent where it is small (<= 1 GB).
                const bool small_arena = (double)B * (double)P.stride * 8.0 <= 1e9;
                // (round 4, monotone sweeps -- shorter, so a saved sweep is worth less against the doubled front work: 256
                //  resident scenarios 6 541 QP/s with it, 6 627 without; 128: 4 307 / 4 110; on up to 192 instances)
                d.spec_mode = getenv("SQPHIP_MF_SPEC") ? atoi(getenv("SQPHIP_MF_SPEC")) : (B <= (opt->ipm_corrector ? 256 : 192) && small_arena ? 1 : 0);
                // ... and for larger batches in the TAIL of a run: once most instances of a group have used up their outer iterations
                // the sweeps are latency-bound again and the stragglers' failed shifts are the critical path (sqp_run_lane switches
                // it on while at most spec_tail instances of the group have work left; SQPHIP_MF_SPEC_TAIL, 0 = never).  Measured,
                // driver's command: threshold 0 / 16 / 32 / 48 / 64 / 96 -> 8 992 / 9 036 / 9 052 / 9 031 / 9 049 / 9 016 QP/s at 512 resident
                // scenarios (1.4 % fewer sweeps, identical work counters), 6 614 / 6 682 / 6 708 / 6 692 / 6 552 / 6 561 at 256
                C.spec_tail = d.spec_mode == 0 && small_arena ? (getenv("SQPHIP_MF_SPEC_TAIL") ? atoi(getenv("SQPHIP_MF_SPEC_TAIL")) : (getenv("SQPHIP_MF_SPEC") ? 0 : 32)) : 0;
                C.spec_mode0 = d.spec_mode;
                // (the arenas of the second candidate are allocated below, once the way the values are assembled is known)
            } else if (d.condense && opt->kkt_tile_order) {
                KktOrder o = kkt_order(d.n, (int)m, kpos, d.mk, PH.colptr, PH.rowval, rptr, rcol, /*rows_last=*/true);
                upos = o.pos; d.Ts = o.Ts; d.Nf = o.Nf;
                if (o.Ts > 0 && o.Tr > 0 && !getenv("SQPHIP_NO_TILE_MASK")) {
                    C.plan.tmask = C.upload(o.tmask);
                    d.tmask = C.plan.tmask;
                    C.plan.pair_ptr = C.upload(o.pair_ptr);
                    C.plan.pair_k = C.upload(o.pair_k.empty() ? std::vector<int>(1, 0) : o.pair_k);
                    // per tile pair: (entries of the lower triangle in the tile) x 2 x 64 x (sub-panels in its list)
                    double fl = 0.0;
                    for (int ti = 0, pi = 0; ti < o.Tr; ++ti)
                        for (int tj = 0; tj <= ti; ++tj, ++pi)
                            fl += (ti == tj ? 64.0 * 65.0 / 2.0 : 64.0 * 64.0) * 2.0 * 64.0 * (o.pair_ptr[pi + 1] - o.pair_ptr[pi]);
                    C.plan.lead_update_flops = fl;
                }
            } else {
                for (int u = 0; u < nu; ++u) upos[u] = u;
            }
            d.Fpad = (d.Nf + 63) / 64 * 64; d.ld = d.Fpad;
            std::vector<int> uinv(d.Fpad, -1);
            for (int u = 0; u < nu; ++u) uinv[upos[u]] = u;
            d.upos = C.upload(upos); d.uinv = C.upload(uinv);
        }
        d.hcolptr = C.upload(PH.colptr); d.hrowval = C.upload(PH.rowval);
        d.jg_ptr = C.upload(PJ.g_ptr); d.jg_src = C.upload(PJ.g_src);
        d.hg_ptr = C.upload(PH.g_ptr); d.hg_src = C.upload(PH.g_src);
        const size_t Bn = (size_t)B * n, Bm = (size_t)B * m, BN = (size_t)B * d.Npad;
        d.xL = C.dalloc<double>(Bn); d.xU = C.dalloc<double>(Bn);
        d.gL = C.dalloc<double>(Bm); d.gU = C.dalloc<double>(Bm);
        for (int b = 0; b < B; ++b) {
            h2d(C, d.xL + (size_t)b * n, xL, n); h2d(C, d.xU + (size_t)b * n, xU, n);
            h2d(C, d.gL + (size_t)b * m, gL, m); h2d(C, d.gU + (size_t)b * m, gU, m);
        }
        d.xk = C.dalloc<double>(Bn); d.cin = C.dalloc<double>(Bn); d.bE = C.dalloc<double>(Bm);
        d.jcoo = C.dalloc<double>((size_t)B * nnzJ); d.hcoo = C.dalloc<double>((size_t)B * nnzH);
        d.jv = C.dalloc<double>((size_t)B * d.nnzjc); d.hv = C.dalloc<double>((size_t)B * d.nnzhc);
        double **nvec[] = { &d.c, &d.hd, &d.lb, &d.ub, &d.p, &d.zl, &d.zu, &d.dp, &d.dzl, &d.dzu, &d.rd,
                            &d.sigp, &d.wn, &d.op, &d.omxU, &d.omxL, &d.x, &d.mxL, &d.mxU, &d.df, &d.pstep,
                            &d.psoc, &d.pmxL, &d.pmxU, &d.tmpx, &d.x0, &d.socZL, &d.socZU };
        for (auto pp : nvec) *pp = C.dalloc<double>(Bn);
        double **mvec[] = { &d.lo, &d.hi, &d.wp, &d.wm, &d.s, &d.tp, &d.tm, &d.y, &d.vl, &d.vu, &d.ds,
                            &d.dtp, &d.dtm, &d.dy, &d.dvl, &d.dvu, &d.rp, &d.Dd, &d.olam, &d.lambda, &d.E,
                            &d.plam, &d.Esoc, &d.tmpE, &d.hlam, &d.zp, &d.zm, &d.rdir,
                            &d.socZP, &d.socZM, &d.socVL, &d.socVU };
        for (auto pp : mvec) *pp = C.dalloc<double>(Bm);
        d.oslack = C.dalloc<double>(2 * Bm);
        d.rtype = C.dalloc<int>(Bm); d.rbase = C.dalloc<int>(Bm); d.hard = C.dalloc<int>(Bm);
        d.rhs = C.dalloc<double>(BN); d.sol = C.dalloc<double>(BN); d.wN = C.dalloc<double>(BN);
        const size_t BF = (size_t)B * d.Fpad;          // solve vectors and pivots live in the factorised order
        d.xv = C.dalloc<double>(BF); d.vv = C.dalloc<double>(BF); d.dinv = C.dalloc<double>(BF);
        d.K = C.dalloc<double>(d.sparse ? 1 : (size_t)B * d.ld * d.Fpad);
        d.ist = C.dalloc<IpmState>(B); d.sst = C.dalloc<SqpState>(B);
        d.phase = C.dalloc<int>(B); d.counters = C.dalloc<int>(64);
        d.trace = C.dalloc<double>((size_t)B * SQPHIP_TRACE_CAP * SQPHIP_TRACE_COLS);
        d.ipm_tol = opt->ipm_tol; d.ipm_max_iter = opt->ipm_max_iter; d.ipm_phase1 = opt->ipm_phase1; d.ipm_corrector = opt->ipm_corrector; d.ipm_warm = opt->ipm_warm_start;
        d.refine_tol = getenv("SQPHIP_REFINE_TOL") ? atof(getenv("SQPHIP_REFINE_TOL")) : 1e-11;
        d.vstage = (d.n + d.N <= 7000 && !getenv("SQPHIP_NO_VSTAGE")) ? d.n + d.N : 0;      // up to 56 KB of LDS per workgroup
        // large instances (the vectors do not fit the LDS of one workgroup): the sparse products of the vector stages by flat
        // kernels over the whole batch (ipm.hip, k_sp_products); SQPHIP_VEC_FLAT=1 / 0 forces / forbids it (tests, A / B runs)
        d.flat = getenv("SQPHIP_VEC_FLAT") ? (atoi(getenv("SQPHIP_VEC_FLAT")) != 0) : (d.vstage == 0 && d.n + d.N > 7000);
        // (measured, round 4: the stage kernel assembling the values of its instance -- eight destinations per thread, each a
        //  chain item list -> items -> operands -- takes longer than the flat k_mf_values launch it saves: 7 528 against 7 706
        //  QP/s at 512 x IEEE-118, 1 880 against 2 002 at 64, +2 % on IEEE-14; on request only)
        d.vals_inline = d.sparse && !d.flat && getenv("SQPHIP_MF_VALS_INLINE") && atoi(getenv("SQPHIP_MF_VALS_INLINE")) == 1;
        // the stage kernel assembles the values of sweep k + 1 during sweep k, under that sweep's spec_mode: a second candidate
        // switched on between the two (spec_tail) would be factorised from values1 never written for it
        if (d.vals_inline) C.spec_tail = 0;
        if (d.sparse && (d.spec_mode != 0 || C.spec_tail > 0)) {
            d.mf.vals1 = C.dalloc<double>((size_t)B * C.mfp().nnzK);
            d.mf.fronts1 = C.dalloc<double>((size_t)B * C.mfp().stride);
            d.vv1 = C.dalloc<double>(BF); d.dinv1 = C.dalloc<double>(BF);
        }
        if (d.flat) {
            d.vstage = 0;
            d.fH = C.dalloc<double>(Bn); d.fJt = C.dalloc<double>(Bn); d.fJ = C.dalloc<double>(Bm); d.fX = C.dalloc<double>(Bm);
        }
        // the working vector of the condensed form from entry-parallel terms in LDS (ipm.hip, solve_vector_terms): where the
        // vector stages are on and its stage fits the 160 KB of a workgroup beside the static LDS of the reductions (8 KB kept
        // back); SQPHIP_XV_TERMS=0 leaves the column walk of load_solve_vector (cross-check, A / B runs; read once, here)
        d.xstage = 0;
        if (d.vstage && d.condense && !(getenv("SQPHIP_XV_TERMS") && atoi(getenv("SQPHIP_XV_TERMS")) == 0)) {
            const size_t xs = xv_terms_doubles(d);
            if (8 * xs <= 152 * 1024 && (8 * xs <= 64 * 1024 || ipm_device_setup(C))) d.xstage = (int)xs;
        }
        d.tol_direction = opt->tol_direction; d.tol_residual = opt->tol_residual;
        d.tol_infeas = opt->tol_infeas; d.init_mu = opt->init_mu; d.tr_size = opt->tr_size;
        d.max_iter = opt->max_iter; d.use_soc = opt->use_soc; d.literal_quirks = opt->literal_quirks;
        C.plan.N = d.Nf; C.plan.Npad = d.Fpad; C.plan.T = d.Fpad / 64; C.plan.ld = d.ld; C.plan.B = B;
        C.plan.Ts = d.Ts;
        C.plan.stream = C.stream;
        if (opt->kkt_tile_order && !d.condense && !d.sparse)
            C.err = "note: options.kkt_tile_order needs options.kkt_condense = 1 and was ignored";
        if (!d.sparse) {
            C.plan.Wbuf = C.dalloc<double>((size_t)std::max(2 * LdltPlan::MAX_R, d.Ts) * B * d.Fpad * 64);
            C.plan.init_lookahead();
        }
        SQPHIP_HIP_OK(hipStreamSynchronize(C.stream));
        if (const char *e = getenv("SQPHIP_TRANS_PERIOD")) C.trans_period = atoi(e);      // experiment switch, read once per context
        if (const char *e = getenv("SQPHIP_TRANS_RIDE")) C.trans_ride = atoi(e);      // transitions inside the post launch (ctx.hpp): 0 off, 1 one ride, 2 two
        C.refine_slot = getenv("SQPHIP_REFINE_SLOT") && atoi(getenv("SQPHIP_REFINE_SLOT")) == 1;      // the second solve chain of a sweep (ipm_sweep)
        if (const char *e = getenv("SQPHIP_REFINE_PERIOD")) C.refine_period = atoi(e);      // experiment switch
        if (d.sparse) mf_device_setup(C);
        C.post_split = getenv("SQPHIP_POST_SPLIT") && atoi(getenv("SQPHIP_POST_SPLIT")) == 1;
        C.side_mode = getenv("SQPHIP_SIDE_TRANS") && atoi(getenv("SQPHIP_SIDE_TRANS")) == 1;      // transitions on a side stream (ctx.hpp)
        make_lanes(C);
        return SQPHIP_OK;
    });
    if (rc != SQPHIP_OK) {
        fprintf(stderr, "sqphip_create: %s\n", h->c.err.c_str());
        delete h;
        return rc;
    }
    *out = h;
    return SQPHIP_OK;
}

extern "C" void sqphip_destroy(sqphip_ctx *h)
{
    if (!h) return;
    hipSetDevice(h->c.opt.device);
    delete h;
}

extern "C" const char *sqphip_last_error(const sqphip_ctx *h) { return h ? h->c.err.c_str() : "null context"; }

extern "C" int sqphip_set_bounds(sqphip_ctx *h, int32_t inst, const double *xL, const double *xU,
                                 const double *gL, const double *gU)
{
    if (!h || inst < 0 || inst >= h->c.d.B || !xL || !xU || (h->c.d.m > 0 && (!gL || !gU))) return SQPHIP_EINVAL;
    for (int i = 0; i < h->c.d.m; ++i)          // as sqphip_create: a row unbounded on both sides is no constraint upstream
        if (gL[i] == -INFINITY && gU[i] == INFINITY) { h->c.err = "sqphip_set_bounds: row " + std::to_string(i) + " is unbounded on both sides"; return SQPHIP_EINVAL; }
    return guarded(h, [&](Ctx &C) {
        DV &d = C.d;
        // condensed form: the kept-row set was fixed at creation; an instance may not turn an eliminated row into
        // an equality (its D would sit at the regularisation and 1/D in the condensed matrix at 1e8)
        if (d.condense)
            for (int i = 0; i < d.m; ++i)
                if (gL[i] == gU[i] && C.h_kpos[i] < 0) {
                    C.err = "sqphip_set_bounds: row " + std::to_string(i) + " is an equality for this instance but was "
                            "not one when the context was created (options.kkt_condense = 1 fixes the kept rows)";
                    return SQPHIP_EINVAL;
                }
        h2d(C, d.xL + (size_t)inst * d.n, xL, d.n); h2d(C, d.xU + (size_t)inst * d.n, xU, d.n);
        h2d(C, d.gL + (size_t)inst * d.m, gL, d.m); h2d(C, d.gU + (size_t)inst * d.m, gU, d.m);
        SQPHIP_HIP_OK(hipStreamSynchronize(C.stream));
        return SQPHIP_OK;
    });
}

extern "C" int sqphip_qp_solve(sqphip_ctx *h, int32_t mode, const double *x_k, double delta, double mu,
                               const double *df, const double *E, const double *Jval, const double *Hval,
                               double *p, double *lambda, double *mult_x_U, double *mult_x_L, double *slack,
                               int32_t *moi_status)
{
    if (!h || !x_k || !Jval || !p || !lambda || !mult_x_U || !mult_x_L || !moi_status) return SQPHIP_EINVAL;
    if (mode < 0 || mode > SQPHIP_MODE_INFEAS) return SQPHIP_EINVAL;
    if (mode != SQPHIP_MODE_LP && (!df || !E)) return SQPHIP_EINVAL;
    return guarded(h, [&](Ctx &C) {
        DV &d = C.d;
        auto t0 = std::chrono::steady_clock::now();
        h2d(C, d.xk, x_k, d.n);
        h2d(C, d.cin, df, d.n);
        h2d(C, d.bE, E, d.m);
        h2d(C, d.jcoo, Jval, d.nnzj_coo);
        if (Hval) h2d(C, d.hcoo, Hval, d.nnzh_coo);
        else SQPHIP_HIP_OK(hipMemsetAsync(d.hcoo, 0, sizeof(double) * (size_t)d.nnzh_coo, C.stream));
        hipLaunchKernelGGL(k_qp_request, dim3(1), dim3(64), 0, C.stream, d, 0, (int)mode, delta, mu);
        launch_qp_gather(C);
        ipm_run_all(C);
        IpmState st;
        SQPHIP_HIP_OK(hipMemcpyAsync(&st, d.ist, sizeof(IpmState), hipMemcpyDeviceToHost, C.stream));
        d2h(C, p, d.op, d.n); d2h(C, lambda, d.olam, d.m);
        d2h(C, mult_x_U, d.omxU, d.n); d2h(C, mult_x_L, d.omxL, d.n);
        d2h(C, slack, d.oslack, 2 * (size_t)d.m);
        SQPHIP_HIP_OK(hipStreamSynchronize(C.stream));
        *moi_status = st.status;
        C.last_ipm_iters = st.ipm_iters; C.last_n_factor = st.n_factor;
        C.last_rule = st.rc == 0 ? st.acc_rule : -1; C.last_e0 = st.e0;
        C.n_qp += 1; C.n_ipm_iter += st.ipm_iters; C.n_factor += st.n_factor; C.n_solve += st.n_solve;
        C.total_seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        return SQPHIP_OK;
    });
}

// Kernel-level test hook of the multifrontal path (mfront.hip) -- the device twin of sqphip_mf_host_solve: Newton
// matrix from the given values in instance `inst` of a context created with the sparse solver, factorised with the
// right-hand side fused in (sol_fused), then solved again through the stand-alone forward / backward kernels
// (sol_standalone).  Vectors in unknown order (variables, then kept rows).
extern "C" int sqphip_mf_solve_test(sqphip_ctx *h, int32_t inst, const double *Jval, const double *Hval,
                                    const double *Dd, const double *sigp, const double *hd, const int32_t *rtype,
                                    double hsc, double dw, const double *rhs, double *sol_fused,
                                    double *sol_standalone, double *dinv_by_unknown)
{
    if (!h || inst < 0 || inst >= h->c.d.B || !Jval || !Dd || !sigp || !hd || !rtype || !rhs) return SQPHIP_EINVAL;
    if (!h->c.d.sparse) { h->c.err = "sqphip_mf_solve_test: the context does not use the sparse solver"; return SQPHIP_ESTATE; }
    return guarded(h, [&](Ctx &C) {
        DV &d = C.d;
        const SparseSym &S = C.mfp().S;
        const size_t on = (size_t)inst * d.n, om = (size_t)inst * d.m;
        h2d(C, d.jcoo + (size_t)inst * d.nnzj_coo, Jval, d.nnzj_coo);
        if (Hval) h2d(C, d.hcoo + (size_t)inst * d.nnzh_coo, Hval, d.nnzh_coo);
        else SQPHIP_HIP_OK(hipMemsetAsync(d.hcoo + (size_t)inst * d.nnzh_coo, 0, sizeof(double) * (size_t)d.nnzh_coo, C.stream));
        hipLaunchKernelGGL(k_qp_request, dim3(1), dim3(64), 0, C.stream, d, (int)inst, 0, 1.0, 1.0);
        launch_qp_gather(C);                       // COO -> CSC values of the instance (start flag set, stage 0)
        hipLaunchKernelGGL(k_mf_test_setup, dim3(1), dim3(64), 0, C.stream, d, (int)inst, hsc, dw, (int)PH_FACTOR);
        h2d(C, d.Dd + om, Dd, d.m); h2d(C, d.sigp + on, sigp, d.n); h2d(C, d.hd + on, hd, d.n);
        SQPHIP_HIP_OK(hipMemcpyAsync(d.rtype + om, rtype, sizeof(int) * (size_t)d.m, hipMemcpyHostToDevice, C.stream));
        std::vector<double> xp(d.Fpad, 0.0), out(d.Fpad), dv(d.Fpad);
        for (int u = 0; u < S.nu; ++u) xp[S.pos[u]] = rhs[u];
        double *xv = d.xv + (size_t)inst * d.Fpad;
        h2d(C, xv, xp.data(), d.Fpad);
        mf_factor(C, PH_FACTOR, true);
        mf_solve(C, PH_FACTOR, true);
        d2h(C, out.data(), xv, d.Fpad); d2h(C, dv.data(), d.dinv + (size_t)inst * d.Fpad, d.Fpad);
        SQPHIP_HIP_OK(hipStreamSynchronize(C.stream));
        for (int u = 0; u < S.nu; ++u) {
            if (sol_fused) sol_fused[u] = out[S.pos[u]];
            if (dinv_by_unknown) dinv_by_unknown[u] = dv[S.pos[u]];
        }
        h2d(C, xv, xp.data(), d.Fpad);
        mf_solve(C, PH_FACTOR, false);
        d2h(C, out.data(), xv, d.Fpad);
        hipLaunchKernelGGL(k_mf_test_setup, dim3(1), dim3(64), 0, C.stream, d, (int)inst, 0.0, 0.0, (int)PH_IDLE);
        SQPHIP_HIP_OK(hipStreamSynchronize(C.stream));
        SQPHIP_HIP_OK(hipGetLastError());
        if (sol_standalone) for (int u = 0; u < S.nu; ++u) sol_standalone[u] = out[S.pos[u]];
        return SQPHIP_OK;
    });
}

// Batched twin of sqphip_mf_solve_test: every instance with active[b] != 0 gets its own values and interior-point state
// and goes through what one sweep does to it (ipm.hip, ipm_sweep): factorisation of both candidate shifts with the
// right-hand side fused in, the inertia test by the path the sweep takes (in k_mf_solve_top2, or k_inertia), the backward
// solve of the instances that passed; then the stand-alone forward / backward solve of the same right-hand side.  Arrays
// per instance, back to back: Jval [B][nnzJ], Hval [B][nnzH], Dd / rtype [B][m], sigp / hd [B][n], rhs / outputs [B][nu]
// (unknown order); hsc, dw, dw_last, fac_attempt [B].  decision [B][5]: outcome (0 idle, 1 another shift needed, 2 passed,
// 3 given up), sel, n_factor, fac_attempt, and 1 if the instance speculates -- derived here from the inputs by the rule of
// mf_speculates, not reported by the device; dw_out [B]: delta_w after the decision.  dinv1
// (may be null): the pivots of candidate 1, zero where the context keeps no second candidate.  Leaves every instance idle.
extern "C" int sqphip_mf_batch_test(sqphip_ctx *h, const int32_t *active, const double *Jval, const double *Hval,
                                    const double *Dd, const double *sigp, const double *hd, const int32_t *rtype,
                                    const double *hsc, const double *dw, const double *dw_last, const int32_t *fac_attempt,
                                    const double *rhs, double *sol_fused, double *sol_standalone, double *dinv0,
                                    double *dinv1, int32_t *decision, double *dw_out)
{
    if (!h || !active || !Jval || !Dd || !sigp || !hd || !rtype || !hsc || !dw || !dw_last || !fac_attempt || !rhs)
        return SQPHIP_EINVAL;
    if (!h->c.d.sparse) { h->c.err = "sqphip_mf_batch_test: the context does not use the sparse solver"; return SQPHIP_ESTATE; }
    return guarded(h, [&](Ctx &C) {
        DV &d = C.d;
        const SparseSym &S = C.mfp().S;
        const int B = d.B, nu = S.nu;
        std::vector<double> xp((size_t)B * d.Fpad, 0.0), out((size_t)B * d.Fpad), dv((size_t)B * d.Fpad), dv1((size_t)B * d.Fpad, 0.0);
        for (int b = 0; b < B; ++b) {
            const size_t on = (size_t)b * d.n, om = (size_t)b * d.m;
            h2d(C, d.jcoo + (size_t)b * d.nnzj_coo, Jval + (size_t)b * d.nnzj_coo, d.nnzj_coo);
            if (Hval) h2d(C, d.hcoo + (size_t)b * d.nnzh_coo, Hval + (size_t)b * d.nnzh_coo, d.nnzh_coo);
            else SQPHIP_HIP_OK(hipMemsetAsync(d.hcoo + (size_t)b * d.nnzh_coo, 0, sizeof(double) * (size_t)d.nnzh_coo, C.stream));
            h2d(C, d.Dd + om, Dd + om, d.m); h2d(C, d.sigp + on, sigp + on, d.n); h2d(C, d.hd + on, hd + on, d.n);
            SQPHIP_HIP_OK(hipMemcpyAsync(d.rtype + om, rtype + om, sizeof(int) * (size_t)d.m, hipMemcpyHostToDevice, C.stream));
            for (int u = 0; u < nu; ++u) xp[(size_t)b * d.Fpad + S.pos[u]] = rhs[(size_t)b * nu + u];
            hipLaunchKernelGGL(k_mf_inst_set, dim3(1), dim3(64), 0, C.stream, d, b, active[b] ? 1 : 0, (int)PH_IDLE, 0.0, 0.0, 0.0, 0);
        }
        h2d(C, d.xv, xp.data(), xp.size());
        launch_qp_gather(C);                       // COO -> CSC values of the active instances (start flag set, stage 0)
        for (int b = 0; b < B; ++b)
            hipLaunchKernelGGL(k_mf_inst_set, dim3(1), dim3(64), 0, C.stream, d, b, 0, active[b] ? (int)PH_FACTOR : (int)PH_IDLE,
                               hsc[b], dw[b], dw_last[b], (int)fac_attempt[b]);
        // what the sweep does (ipm_sweep): factorise, test the inertia, solve the instances that passed
        const bool top_inertia = mf_solve_tests_inertia(C);
        mf_factor(C, PH_FACTOR, true);
        if (!top_inertia) launch_inertia(C);
        mf_solve(C, PH_SOLVE, true, top_inertia);
        d2h(C, out.data(), d.xv, out.size()); d2h(C, dv.data(), d.dinv, dv.size());
        if (d.dinv1) d2h(C, dv1.data(), d.dinv1, dv1.size());
        std::vector<IpmState> st(B);
        std::vector<int> ph(B);
        SQPHIP_HIP_OK(hipMemcpyAsync(st.data(), d.ist, sizeof(IpmState) * (size_t)B, hipMemcpyDeviceToHost, C.stream));
        SQPHIP_HIP_OK(hipMemcpyAsync(ph.data(), d.phase, sizeof(int) * (size_t)B, hipMemcpyDeviceToHost, C.stream));
        SQPHIP_HIP_OK(hipStreamSynchronize(C.stream));
        for (int b = 0; b < B; ++b) {
            const size_t f = (size_t)b * d.Fpad, o = (size_t)b * nu;
            for (int u = 0; u < nu; ++u) {
                if (sol_fused) sol_fused[o + u] = out[f + S.pos[u]];
                if (dinv0) dinv0[o + u] = dv[f + S.pos[u]];
                if (dinv1) dinv1[o + u] = dv1[f + S.pos[u]];
            }
            const IpmState &I = st[b];
            const bool spec = d.mf.fronts1 != nullptr && d.spec_mode != 0 && (fac_attempt[b] > 0 || (d.spec_mode == 1 && dw[b] > 0.0));
            if (decision) {
                int32_t *r = decision + 5 * (size_t)b;
                r[0] = !active[b] ? 0 : ph[b] == PH_FACTOR ? 1 : ph[b] == PH_SOLVE ? 2 : 3;
                r[1] = I.sel; r[2] = I.n_factor; r[3] = I.fac_attempt; r[4] = active[b] && spec ? 1 : 0;
            }
            if (dw_out) dw_out[b] = I.dw;
        }
        // the stand-alone forward and backward solves on the factors the decision selected
        h2d(C, d.xv, xp.data(), xp.size());
        mf_solve(C, PH_SOLVE, false);
        d2h(C, out.data(), d.xv, out.size());
        for (int b = 0; b < B; ++b)
            hipLaunchKernelGGL(k_mf_inst_set, dim3(1), dim3(64), 0, C.stream, d, b, 0, (int)PH_IDLE, 0.0, 0.0, 0.0, 0);
        SQPHIP_HIP_OK(hipStreamSynchronize(C.stream));
        SQPHIP_HIP_OK(hipGetLastError());
        if (sol_standalone)
            for (int b = 0; b < B; ++b)
                for (int u = 0; u < nu; ++u) sol_standalone[(size_t)b * nu + u] = out[(size_t)b * d.Fpad + S.pos[u]];
        return SQPHIP_OK;
    });
}

// The values launch of a sweep on its own (k_mf_values, whichever variant the switches select): instances and
// interior-point states as in sqphip_mf_batch_test; vals0 / vals1 [B][nnzK] come back as the device holds them after the
// launch, every slot preset to `sentinel` (vals1: where the context keeps a second candidate, else the sentinel throughout).
// Null outputs: *nnzK only.  Leaves every instance idle.
extern "C" int sqphip_mf_values_test(sqphip_ctx *h, const int32_t *active, const double *Jval, const double *Hval,
                                     const double *Dd, const double *sigp, const double *hd, const int32_t *rtype,
                                     const double *hsc, const double *dw, const double *dw_last, const int32_t *fac_attempt,
                                     double sentinel, double *vals0, double *vals1, int64_t *nnzK)
{
    if (!h) return SQPHIP_EINVAL;
    if (!h->c.d.sparse) { h->c.err = "sqphip_mf_values_test: the context does not use the sparse solver"; return SQPHIP_ESTATE; }
    if (nnzK) *nnzK = h->c.d.mf.nnzK;
    if (!vals0 && !vals1) return SQPHIP_OK;
    if (!active || !Jval || !Dd || !sigp || !hd || !rtype || !hsc || !dw || !dw_last || !fac_attempt) return SQPHIP_EINVAL;
    return guarded(h, [&](Ctx &C) {
        DV &d = C.d;
        const int B = d.B;
        const size_t nv = (size_t)B * d.mf.nnzK;
        for (int b = 0; b < B; ++b) {
            const size_t on = (size_t)b * d.n, om = (size_t)b * d.m;
            h2d(C, d.jcoo + (size_t)b * d.nnzj_coo, Jval + (size_t)b * d.nnzj_coo, d.nnzj_coo);
            if (Hval) h2d(C, d.hcoo + (size_t)b * d.nnzh_coo, Hval + (size_t)b * d.nnzh_coo, d.nnzh_coo);
            else SQPHIP_HIP_OK(hipMemsetAsync(d.hcoo + (size_t)b * d.nnzh_coo, 0, sizeof(double) * (size_t)d.nnzh_coo, C.stream));
            h2d(C, d.Dd + om, Dd + om, d.m); h2d(C, d.sigp + on, sigp + on, d.n); h2d(C, d.hd + on, hd + on, d.n);
            SQPHIP_HIP_OK(hipMemcpyAsync(d.rtype + om, rtype + om, sizeof(int) * (size_t)d.m, hipMemcpyHostToDevice, C.stream));
            hipLaunchKernelGGL(k_mf_inst_set, dim3(1), dim3(64), 0, C.stream, d, b, active[b] ? 1 : 0, (int)PH_IDLE, 0.0, 0.0, 0.0, 0);
        }
        launch_qp_gather(C);                       // COO -> CSC values of the active instances (start flag set, stage 0)
        for (int b = 0; b < B; ++b)
            hipLaunchKernelGGL(k_mf_inst_set, dim3(1), dim3(64), 0, C.stream, d, b, 0, active[b] ? (int)PH_FACTOR : (int)PH_IDLE,
                               hsc[b], dw[b], dw_last[b], (int)fac_attempt[b]);
        std::vector<double> fill(nv, sentinel), out1(nv, sentinel);
        h2d(C, d.mf.vals, fill.data(), nv);
        if (d.mf.vals1) h2d(C, d.mf.vals1, fill.data(), nv);
        mf_values(C, PH_FACTOR);
        if (vals0) d2h(C, vals0, d.mf.vals, nv);
        if (d.mf.vals1) d2h(C, out1.data(), d.mf.vals1, nv);
        for (int b = 0; b < B; ++b)
            hipLaunchKernelGGL(k_mf_inst_set, dim3(1), dim3(64), 0, C.stream, d, b, 0, (int)PH_IDLE, 0.0, 0.0, 0.0, 0);
        SQPHIP_HIP_OK(hipStreamSynchronize(C.stream));
        SQPHIP_HIP_OK(hipGetLastError());
        if (vals1) std::copy(out1.begin(), out1.end(), vals1);
        return SQPHIP_OK;
    });
}

// Dense twin of sqphip_mf_batch_test: every instance with active[b] != 0 gets its own values and interior-point state; the
// working vector of the solves is built from the full-length right-hand side by both routines (k_sp_load_xv and
// load_solve_vector: *xv_mismatch counts entries whose bits differ), the Newton matrix is assembled (k_kkt_assemble) and read
// back, and the instance goes through what one sweep does on the dense path (ipm.hip, ipm_sweep): ldlt_factor with the
// right-hand side fused in, k_inertia, the backward solve of the instances that passed.  xv, vv and dinv of every instance
// are preset to `sentinel`: what an inactive instance must come back with.  Leaves every instance idle.
extern "C" int sqphip_kkt_dense_test(sqphip_ctx *h, const int32_t *active, const double *Jval, const double *Hval,
                                     const double *Dd, const double *sigp, const double *hd, const int32_t *rtype,
                                     const double *hsc, const double *dw, const double *dw_last, const int32_t *fac_attempt,
                                     const double *rhs, double sentinel, double *K_assembled, double *xv_loaded,
                                     int32_t *xv_mismatch, double *sol, double *dinv, double *dinv_pad, int32_t *decision,
                                     double *dw_out)
{
    if (!h || !active || !Jval || !Dd || !sigp || !hd || !rtype || !hsc || !dw || !dw_last || !fac_attempt || !rhs)
        return SQPHIP_EINVAL;
    if (h->c.d.sparse) { h->c.err = "sqphip_kkt_dense_test: the context uses the sparse solver"; return SQPHIP_ESTATE; }
    return guarded(h, [&](Ctx &C) {
        DV &d = C.d;
        const int B = d.B, nu = d.condense ? d.n + d.mk : d.N;
        const size_t BF = (size_t)B * d.Fpad;
        for (int b = 0; b < B; ++b) {
            const size_t on = (size_t)b * d.n, om = (size_t)b * d.m;
            h2d(C, d.jcoo + (size_t)b * d.nnzj_coo, Jval + (size_t)b * d.nnzj_coo, d.nnzj_coo);
            if (Hval) h2d(C, d.hcoo + (size_t)b * d.nnzh_coo, Hval + (size_t)b * d.nnzh_coo, d.nnzh_coo);
            else SQPHIP_HIP_OK(hipMemsetAsync(d.hcoo + (size_t)b * d.nnzh_coo, 0, sizeof(double) * (size_t)d.nnzh_coo, C.stream));
            h2d(C, d.Dd + om, Dd + om, d.m); h2d(C, d.sigp + on, sigp + on, d.n); h2d(C, d.hd + on, hd + on, d.n);
            SQPHIP_HIP_OK(hipMemcpyAsync(d.rtype + om, rtype + om, sizeof(int) * (size_t)d.m, hipMemcpyHostToDevice, C.stream));
            h2d(C, d.rhs + (size_t)b * d.Npad, rhs + (size_t)b * d.N, d.N);
            hipLaunchKernelGGL(k_mf_inst_set, dim3(1), dim3(64), 0, C.stream, d, b, active[b] ? 1 : 0, (int)PH_IDLE, 0.0, 0.0, 0.0, 0);
        }
        launch_qp_gather(C);                       // COO -> CSC values of the active instances (start flag set, stage 0)
        for (int b = 0; b < B; ++b)
            hipLaunchKernelGGL(k_mf_inst_set, dim3(1), dim3(64), 0, C.stream, d, b, 0, active[b] ? (int)PH_FACTOR : (int)PH_IDLE,
                               hsc[b], dw[b], dw_last[b], (int)fac_attempt[b]);
        const std::vector<double> fill(BF, sentinel);
        std::vector<double> xa(BF), xb(BF), out(BF), dv(BF);
        std::vector<int> upos(nu);
        SQPHIP_HIP_OK(hipMemcpyAsync(upos.data(), d.upos, sizeof(int) * (size_t)nu, hipMemcpyDeviceToHost, C.stream));
        h2d(C, d.vv, fill.data(), BF); h2d(C, d.dinv, fill.data(), BF);
        // the working vector twice: the flat kernel, then (last, so that it is what the factorisation consumes) the routine of
        // the one-workgroup stages
        h2d(C, d.xv, fill.data(), BF);
        launch_load_xv_test(C, true);
        d2h(C, xa.data(), d.xv, BF);
        h2d(C, d.xv, fill.data(), BF);
        launch_load_xv_test(C, false);
        d2h(C, xb.data(), d.xv, BF);
        launch_kkt_assemble(C);
        if (K_assembled) d2h(C, K_assembled, d.K, (size_t)B * d.ld * d.Fpad);
        // what the sweep does on the dense path (ipm_sweep): factorise with xv / vv fused in, test the inertia, solve backward
        ldlt_factor(C.plan, d.K, d.dinv, d.phase, PH_FACTOR, &C.tm, d.xv, d.vv);
        launch_inertia(C);
        ldlt_solve(C.plan, d.K, d.dinv, d.xv, d.vv, d.phase, PH_SOLVE, true);
        d2h(C, out.data(), d.xv, BF); d2h(C, dv.data(), d.dinv, BF);
        std::vector<IpmState> st(B);
        std::vector<int> ph(B);
        SQPHIP_HIP_OK(hipMemcpyAsync(st.data(), d.ist, sizeof(IpmState) * (size_t)B, hipMemcpyDeviceToHost, C.stream));
        SQPHIP_HIP_OK(hipMemcpyAsync(ph.data(), d.phase, sizeof(int) * (size_t)B, hipMemcpyDeviceToHost, C.stream));
        for (int b = 0; b < B; ++b)
            hipLaunchKernelGGL(k_mf_inst_set, dim3(1), dim3(64), 0, C.stream, d, b, 0, (int)PH_IDLE, 0.0, 0.0, 0.0, 0);
        SQPHIP_HIP_OK(hipStreamSynchronize(C.stream));
        SQPHIP_HIP_OK(hipGetLastError());
        if (xv_mismatch) {
            int bad = 0;
            for (size_t k = 0; k < BF; ++k) bad += std::memcmp(&xa[k], &xb[k], sizeof(double)) != 0;
            *xv_mismatch = bad;
        }
        if (xv_loaded) std::copy(xb.begin(), xb.end(), xv_loaded);
        if (dinv_pad) std::copy(dv.begin(), dv.end(), dinv_pad);
        for (int b = 0; b < B; ++b) {
            const size_t f = (size_t)b * d.Fpad, o = (size_t)b * nu;
            for (int u = 0; u < nu; ++u) {
                if (sol) sol[o + u] = out[f + upos[u]];
                if (dinv) dinv[o + u] = dv[f + upos[u]];
            }
            if (decision) {
                int32_t *r = decision + 4 * (size_t)b;
                r[0] = !active[b] ? 0 : ph[b] == PH_FACTOR ? 1 : ph[b] == PH_SOLVE ? 2 : 3;
                r[1] = st[b].sel; r[2] = st[b].n_factor; r[3] = st[b].fac_attempt;
            }
            if (dw_out) dw_out[b] = st[b].dw;
        }
        return SQPHIP_OK;
    });
}

// The working vector of the solves by both routines of the one-workgroup stages, on a sparse or a dense context: every instance
// with active[b] != 0 gets its Jacobian values, D, row types and full-length right-hand side and goes to PH_FACTOR; xv is preset
// to SQPHIP_SOLVE_VECTOR_SENTINEL, built by load_solve_vector (k_load_solve_vector_test) and copied out, preset again, built by solve_vector_terms
// behind a stage filled from the same arrays (k_solve_vector_terms_test) and copied out.  *mismatch: entries whose bits differ.
// SQPHIP_ESTATE where the context runs without the stage (DV::xstage == 0).  Leaves every instance idle.
extern "C" int sqphip_solve_vector_test(sqphip_ctx *h, const int32_t *active, const double *Jval, const double *Dd,
                                        const int32_t *rtype, const double *rhs, double *xv_plain, double *xv_terms,
                                        int32_t *mismatch)
{
    if (!h || !active || !Jval || !Dd || !rtype || !rhs) return SQPHIP_EINVAL;
    if (h->c.d.xstage == 0) { h->c.err = "sqphip_solve_vector_test: the context builds the working vector without the LDS stage (xstage = 0)"; return SQPHIP_ESTATE; }
    return guarded(h, [&](Ctx &C) {
        DV &d = C.d;
        const int B = d.B;
        const size_t BF = (size_t)B * d.Fpad;
        for (int b = 0; b < B; ++b) {
            const size_t om = (size_t)b * d.m;
            h2d(C, d.jcoo + (size_t)b * d.nnzj_coo, Jval + (size_t)b * d.nnzj_coo, d.nnzj_coo);
            SQPHIP_HIP_OK(hipMemsetAsync(d.hcoo + (size_t)b * d.nnzh_coo, 0, sizeof(double) * (size_t)d.nnzh_coo, C.stream));
            h2d(C, d.Dd + om, Dd + om, d.m);
            SQPHIP_HIP_OK(hipMemcpyAsync(d.rtype + om, rtype + om, sizeof(int) * (size_t)d.m, hipMemcpyHostToDevice, C.stream));
            h2d(C, d.rhs + (size_t)b * d.Npad, rhs + (size_t)b * d.N, d.N);
            hipLaunchKernelGGL(k_mf_inst_set, dim3(1), dim3(64), 0, C.stream, d, b, active[b] ? 1 : 0, (int)PH_IDLE, 0.0, 0.0, 0.0, 0);
        }
        launch_qp_gather(C);                       // COO -> CSC values of the active instances (start flag set, stage 0)
        for (int b = 0; b < B; ++b)
            hipLaunchKernelGGL(k_mf_inst_set, dim3(1), dim3(64), 0, C.stream, d, b, 0, active[b] ? (int)PH_FACTOR : (int)PH_IDLE,
                               0.0, 0.0, 0.0, 0);
        const std::vector<double> fill(BF, SQPHIP_SOLVE_VECTOR_SENTINEL);
        std::vector<double> xa(BF), xb(BF);
        h2d(C, d.xv, fill.data(), BF);
        launch_load_xv_test(C, false);
        d2h(C, xa.data(), d.xv, BF);
        h2d(C, d.xv, fill.data(), BF);
        launch_xv_terms_test(C);
        d2h(C, xb.data(), d.xv, BF);
        for (int b = 0; b < B; ++b)
            hipLaunchKernelGGL(k_mf_inst_set, dim3(1), dim3(64), 0, C.stream, d, b, 0, (int)PH_IDLE, 0.0, 0.0, 0.0, 0);
        SQPHIP_HIP_OK(hipStreamSynchronize(C.stream));
        SQPHIP_HIP_OK(hipGetLastError());
        if (mismatch) {
            int bad = 0;
            for (size_t k = 0; k < BF; ++k) bad += std::memcmp(&xa[k], &xb[k], sizeof(double)) != 0;
            *mismatch = bad;
        }
        if (xv_plain) std::copy(xa.begin(), xa.end(), xv_plain);
        if (xv_terms) std::copy(xb.begin(), xb.end(), xv_terms);
        return SQPHIP_OK;
    });
}

// Launch census of the multifrontal path: launches enqueued per kernel instantiation since the context was created, summed
// over its instance groups.  counts[cap]; names (may be null): cap x 64 characters, NUL-terminated; *n_kernels = how many
// there are (fewer than cap: the first cap).
extern "C" int sqphip_mf_census(const sqphip_ctx *h, int64_t *counts, char *names, int32_t cap, int32_t *n_kernels)
{
    if (!h || cap < 0 || (cap > 0 && !counts)) return SQPHIP_EINVAL;
    if (n_kernels) *n_kernels = MFK_COUNT;
    for (int k = 0; k < MFK_COUNT && k < cap; ++k) {
        long c = h->c.mf_census[k];
        for (const auto &L : h->c.lanes) c += L->mf_census[k];
        counts[k] = c;
        if (names) { std::strncpy(names + 64 * (size_t)k, mf_kernel_names[k], 63); names[64 * (size_t)k + 63] = 0; }
    }
    return SQPHIP_OK;
}

// Sweeps that launched the three transition kernels in line since the context was created, summed over its instance groups.
extern "C" int sqphip_trans_inline_groups(const sqphip_ctx *h, int64_t *count)
{
    if (!h || !count) return SQPHIP_EINVAL;
    long c = h->c.n_trans_inline;
    for (const auto &L : h->c.lanes) c += L->n_trans_inline;
    *count = c;
    return SQPHIP_OK;
}

extern "C" int sqphip_qp_stats(const sqphip_ctx *h, int32_t *ipm_iters, int32_t *n_factor)
{
    if (!h) return SQPHIP_EINVAL;
    if (ipm_iters) *ipm_iters = h->c.last_ipm_iters;
    if (n_factor) *n_factor = h->c.last_n_factor;
    return SQPHIP_OK;
}

extern "C" int sqphip_qp_termination(const sqphip_ctx *h, int32_t *rule, double *scaled_error)
{
    if (!h) return SQPHIP_EINVAL;
    if (rule) *rule = h->c.last_rule;
    if (scaled_error) *scaled_error = h->c.last_e0;
    return SQPHIP_OK;
}

// ---- the batched seat ---------------------------------------------------------------------------
namespace {

inline long ev(long k) { return (k + 1) & ~1L; }       // doubles of a staged field: padded to 16 bytes

// count in 1 .. batch, inst[k] in range and pairwise distinct; the message names the offending index
int seat_check(sqphip_ctx *h, const char *fn, int32_t count, const int32_t *inst)
{
    Ctx &C = h->c;
    if (count < 1 || count > C.d.B) { C.err = std::string(fn) + ": count " + std::to_string(count) + " is outside 1 .. batch = " + std::to_string(C.d.B); return SQPHIP_EINVAL; }
    if (!inst) { C.err = std::string(fn) + ": inst is NULL"; return SQPHIP_EINVAL; }
    std::vector<int> seen((size_t)C.d.B, -1);
    for (int k = 0; k < count; ++k) {
        if (inst[k] < 0 || inst[k] >= C.d.B) { C.err = std::string(fn) + ": inst[" + std::to_string(k) + "] = " + std::to_string(inst[k]) + " is outside 0 .. batch - 1 = " + std::to_string(C.d.B - 1); return SQPHIP_EINVAL; }
        if (seen[inst[k]] >= 0) { C.err = std::string(fn) + ": inst[" + std::to_string(k) + "] = " + std::to_string(inst[k]) + " repeats inst[" + std::to_string(seen[inst[k]]) + "]"; return SQPHIP_EINVAL; }
        seen[inst[k]] = k;
    }
    return SQPHIP_OK;
}

// One call of the batched seat in staging: header (per request: two scalars, the instance, the mode), then the rows.
//   doubles [0, cp) a0, [cp, 2 cp) a1, then cp int32 inst and cp int32 mode (cp = count padded to even), rows from 3 cp
struct SeatCall {
    Ctx &C;
    int count; long cp, rows0;
    StageMap in{}, out{};
    const double *src[SQPHIP_SEAT_FIELDS] = {};
    SeatCall(Ctx &C_, int count_) : C(C_), count(count_), cp(ev(count_)), rows0(3 * ev(count_))
    {
        // pinned and device staging, once per context, sized for its batch: the header, then per request the longest row of
        // any entry point (operands of compute_qmodel / results of the sub-problem) and its IpmState
        if (!C.stg_h) {
            const DV &d = C.d;
            const long row = 3 * ev(d.n) + 4 * ev(d.m) + ev(d.nnzj_coo) + ev(d.nnzh_coo) + (long)(sizeof(IpmState) / 8) + 2;
            C.stg_doubles = 3 * ev(d.B) + (long)d.B * row;
            SQPHIP_HIP_OK(hipHostMalloc((void **)&C.stg_h, sizeof(double) * (size_t)C.stg_doubles));
            C.stg_d = C.dalloc<double>((size_t)C.stg_doubles);
        }
    }
    double *a0() { return C.stg_h; }
    double *a1() { return C.stg_h + cp; }
    int *inst() { return (int *)(C.stg_h + 2 * cp); }
    int *mode() { return (int *)(C.stg_h + 2 * cp) + cp; }
    const double *a0_dev() const { return C.stg_d; }
    const double *a1_dev() const { return C.stg_d + cp; }
    const int *inst_dev() const { return (const int *)(C.stg_d + 2 * cp); }
    const int *mode_dev() const { return (const int *)(C.stg_d + 2 * cp) + cp; }
    // an operand: [count][len] on the host (null with zero: the slots are cleared; null without: the field is left out)
    void operand(const double *host, double *base, int len, bool zero = false)
    {
        if ((!host && !zero) || len == 0) return;
        const int f = in.nf++;
        in.len[f] = len; in.stride[f] = len; in.base[f] = base; src[f] = host;
        in.off[f] = host ? in.row : -1;
        if (host) in.row += (int)ev(len);
    }
    void result(double *base, int len)
    {
        if (len == 0) return;
        const int f = out.nf++;
        out.len[f] = len; out.stride[f] = len; out.base[f] = base; out.off[f] = out.row;
        out.row += (int)ev(len);
    }
    static dim3 grid(const StageMap &M, int count) { return dim3((unsigned)std::min(32L, std::max(1L, (M.row / 2 + 255L) / 256)), (unsigned)count); }
    // header and rows: packed on the host, one copy, one scatter kernel
    void send(const int32_t *inst_host, const int32_t *mode_host, const double *a0_host, const double *a1_host)
    {
        for (int k = 0; k < count; ++k) {
            a0()[k] = a0_host ? a0_host[k] : 0.0; a1()[k] = a1_host ? a1_host[k] : 0.0;
            inst()[k] = inst_host[k]; mode()[k] = mode_host ? mode_host[k] : 0;
        }
        for (int k = 0; k < count; ++k)
            for (int f = 0; f < in.nf; ++f)
                if (src[f]) std::memcpy(C.stg_h + rows0 + (long)k * in.row + in.off[f], src[f] + (size_t)k * in.len[f], sizeof(double) * (size_t)in.len[f]);
        SQPHIP_HIP_OK(hipMemcpyAsync(C.stg_d, C.stg_h, sizeof(double) * (size_t)(rows0 + (long)count * in.row), hipMemcpyHostToDevice, C.stream));
        if (in.nf) hipLaunchKernelGGL(k_seat_stage<true>, grid(in, count), dim3(256), 0, C.stream, in, C.stg_d + rows0, inst_dev());
    }
    // results (and, with_states, the IpmState of the listed instances): one gather kernel, one copy back, then the host waits
    long fetch(bool with_states, long extra = 0)
    {
        const long body = (long)count * out.row;
        out.ist = with_states ? C.d.ist : nullptr; out.ist_off = body;
        if (out.nf || with_states) hipLaunchKernelGGL(k_seat_stage<false>, grid(out, count), dim3(256), 0, C.stream, out, C.stg_d + rows0, inst_dev());
        const long total = body + (with_states ? (long)count * (long)(sizeof(IpmState) / 8) : 0) + extra;
        SQPHIP_HIP_OK(hipMemcpyAsync(C.stg_h + rows0, C.stg_d + rows0, sizeof(double) * (size_t)total, hipMemcpyDeviceToHost, C.stream));
        SQPHIP_HIP_OK(hipStreamSynchronize(C.stream));
        SQPHIP_HIP_OK(hipGetLastError());
        return body;
    }
    void unpack(int f, double *host) const
    {
        if (!host) return;
        for (int k = 0; k < count; ++k)
            std::memcpy(host + (size_t)k * out.len[f], C.stg_h + rows0 + (long)k * out.row + out.off[f], sizeof(double) * (size_t)out.len[f]);
    }
    IpmState state(int k, long body) const
    {
        IpmState st;
        std::memcpy(&st, (const char *)(C.stg_h + rows0 + body) + sizeof(IpmState) * (size_t)k, sizeof(IpmState));
        return st;
    }
};

}  // namespace

extern "C" int sqphip_qp_solve_batch(sqphip_ctx *h, int32_t count, const int32_t *inst, const int32_t *mode, const double *x_k,
                                     const double *delta, const double *mu, const double *df, const double *E,
                                     const double *Jval, const double *Hval, double *p, double *lambda, double *mult_x_U,
                                     double *mult_x_L, double *slack, int32_t *moi_status)
{
    if (!h || !mode || !x_k || !delta || !mu || !Jval || !p || !lambda || !mult_x_U || !mult_x_L || !moi_status) return SQPHIP_EINVAL;
    if (int rc = seat_check(h, "sqphip_qp_solve_batch", count, inst)) return rc;
    for (int k = 0; k < count; ++k) {
        if (mode[k] < 0 || mode[k] > SQPHIP_MODE_INFEAS) { h->c.err = "sqphip_qp_solve_batch: mode[" + std::to_string(k) + "] = " + std::to_string(mode[k]) + " is no sub-problem mode"; return SQPHIP_EINVAL; }
        if (mode[k] != SQPHIP_MODE_LP && (!df || !E)) { h->c.err = "sqphip_qp_solve_batch: mode[" + std::to_string(k) + "] needs df and E"; return SQPHIP_EINVAL; }
    }
    return guarded(h, [&](Ctx &C) {
        DV &d = C.d;
        auto t0 = std::chrono::steady_clock::now();
        SeatCall S(C, count);
        S.operand(x_k, d.xk, d.n); S.operand(df, d.cin, d.n); S.operand(E, d.bE, d.m);
        S.operand(Jval, d.jcoo, d.nnzj_coo); S.operand(Hval, d.hcoo, d.nnzh_coo, true);
        S.send(inst, mode, delta, mu);
        hipLaunchKernelGGL(k_qp_request_batch, dim3(1), dim3(256), 0, C.stream, d, (int)count, S.inst_dev(), S.mode_dev(), S.a0_dev(), S.a1_dev());
        launch_qp_gather(C);
        ipm_run_all(C);
        S.result(d.op, d.n); S.result(d.olam, d.m); S.result(d.omxU, d.n); S.result(d.omxL, d.n); S.result(d.oslack, 2 * d.m);
        const long body = S.fetch(true);
        int f = 0;
        S.unpack(f++, p);
        if (d.m) S.unpack(f++, lambda);
        S.unpack(f++, mult_x_U); S.unpack(f++, mult_x_L);
        if (d.m) S.unpack(f++, slack);
        for (int k = 0; k < count; ++k) {
            const IpmState st = S.state(k, body);
            moi_status[k] = st.status;
            C.last_ipm_iters = st.ipm_iters; C.last_n_factor = st.n_factor;
            C.last_rule = st.rc == 0 ? st.acc_rule : -1; C.last_e0 = st.e0;
            C.n_qp += 1; C.n_ipm_iter += st.ipm_iters; C.n_factor += st.n_factor; C.n_solve += st.n_solve;
        }
        C.total_seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        return SQPHIP_OK;
    });
}

extern "C" int sqphip_qp_stats_batch(const sqphip_ctx *hc, int32_t count, const int32_t *inst, int32_t *ipm_iters,
                                     int32_t *n_factor, int32_t *rule, double *scaled_error)
{
    sqphip_ctx *h = const_cast<sqphip_ctx *>(hc);       // (reads the states from the device: the stream and the staging are used)
    if (!h) return SQPHIP_EINVAL;
    if (int rc = seat_check(h, "sqphip_qp_stats_batch", count, inst)) return rc;
    return guarded(h, [&](Ctx &C) {
        SeatCall S(C, count);
        S.send(inst, nullptr, nullptr, nullptr);
        const long body = S.fetch(true);
        for (int k = 0; k < count; ++k) {
            const IpmState st = S.state(k, body);
            if (ipm_iters) ipm_iters[k] = st.ipm_iters;
            if (n_factor) n_factor[k] = st.n_factor;
            if (rule) rule[k] = st.rc == 0 ? st.acc_rule : -1;
            if (scaled_error) scaled_error[k] = st.e0;
        }
        return SQPHIP_OK;
    });
}

// test hook: the sub-problem outputs instance `inst` holds on the device (what the seat returned for it last)
extern "C" int sqphip_seat_peek(sqphip_ctx *h, int32_t inst, double *p, double *lambda, double *mult_x_U, double *mult_x_L,
                                double *slack, int32_t *moi_status)
{
    if (!h || inst < 0 || inst >= h->c.d.B) return SQPHIP_EINVAL;
    return guarded(h, [&](Ctx &C) {
        DV &d = C.d;
        d2h(C, p, d.op + (size_t)inst * d.n, d.n); d2h(C, lambda, d.olam + (size_t)inst * d.m, d.m);
        d2h(C, mult_x_U, d.omxU + (size_t)inst * d.n, d.n); d2h(C, mult_x_L, d.omxL + (size_t)inst * d.n, d.n);
        d2h(C, slack, d.oslack + 2 * (size_t)inst * d.m, 2 * (size_t)d.m);
        IpmState st;
        SQPHIP_HIP_OK(hipMemcpyAsync(&st, d.ist + inst, sizeof(IpmState), hipMemcpyDeviceToHost, C.stream));
        SQPHIP_HIP_OK(hipStreamSynchronize(C.stream));
        if (moi_status) *moi_status = st.status;
        return SQPHIP_OK;
    });
}

// ---- merit path -------------------------------------------------------------------------------
extern "C" int sqphip_norm_violations(sqphip_ctx *h, const double *E, const double *x, int32_t pnorm, double *out)
{
    if (!h || !E || !x || !out || pnorm < 0 || pnorm > 2) return SQPHIP_EINVAL;
    return guarded(h, [&](Ctx &C) {
        h2d(C, C.d.E, E, C.d.m); h2d(C, C.d.x, x, C.d.n);
        merit_eval(C, 0, 0.0, 0.0, pnorm, out);
        return SQPHIP_OK;
    });
}

extern "C" int sqphip_kt_residuals(sqphip_ctx *h, const double *df, const double *lambda, const double *mult_x_U,
                                   const double *mult_x_L, const double *Jval, double *out)
{
    if (!h || !df || !lambda || !mult_x_U || !mult_x_L || !Jval || !out) return SQPHIP_EINVAL;
    return guarded(h, [&](Ctx &C) {
        DV &d = C.d;
        h2d(C, d.df, df, d.n); h2d(C, d.lambda, lambda, d.m); h2d(C, d.mxU, mult_x_U, d.n);
        h2d(C, d.mxL, mult_x_L, d.n); h2d(C, d.jcoo, Jval, d.nnzj_coo);
        merit_eval(C, 1, 0.0, 0.0, 0, out);
        return SQPHIP_OK;
    });
}

extern "C" int sqphip_norm_complementarity(sqphip_ctx *h, const double *E, const double *lambda, int32_t pnorm,
                                           double *out)
{
    if (!h || !E || !lambda || !out || pnorm < 0 || pnorm > 2) return SQPHIP_EINVAL;
    return guarded(h, [&](Ctx &C) {
        h2d(C, C.d.E, E, C.d.m); h2d(C, C.d.lambda, lambda, C.d.m);
        merit_eval(C, 2, 0.0, 0.0, pnorm, out);
        return SQPHIP_OK;
    });
}

extern "C" int sqphip_compute_phi(sqphip_ctx *h, double f_trial, const double *E_trial, const double *x_trial,
                                  double mu, int32_t feasibility_restoration, double *phi)
{
    if (!h || !E_trial || !x_trial || !phi) return SQPHIP_EINVAL;
    return guarded(h, [&](Ctx &C) {
        h2d(C, C.d.E, E_trial, C.d.m); h2d(C, C.d.x, x_trial, C.d.n);
        merit_eval(C, 3, f_trial, mu, feasibility_restoration, phi);
        return SQPHIP_OK;
    });
}

extern "C" int sqphip_compute_qmodel(sqphip_ctx *h, const double *x, const double *p, const double *df,
                                     const double *E, const double *Jval, const double *Hval, double mu,
                                     int32_t with_step, double *q)
{
    if (!h || !x || !E || !q) return SQPHIP_EINVAL;
    if (with_step && (!p || !df || !Jval)) return SQPHIP_EINVAL;
    return guarded(h, [&](Ctx &C) {
        DV &d = C.d;
        h2d(C, d.x, x, d.n); h2d(C, d.E, E, d.m);
        if (with_step) {
            h2d(C, d.pstep, p, d.n); h2d(C, d.df, df, d.n); h2d(C, d.jcoo, Jval, d.nnzj_coo);
            if (Hval) h2d(C, d.hcoo, Hval, d.nnzh_coo);
            else SQPHIP_HIP_OK(hipMemsetAsync(d.hcoo, 0, sizeof(double) * (size_t)d.nnzh_coo, C.stream));
        }
        merit_eval(C, 4, 0.0, mu, with_step, q);
        return SQPHIP_OK;
    });
}

extern "C" int sqphip_compute_derivative(sqphip_ctx *h, const double *df, const double *p, const double *E,
                                         double mu, double *D)
{
    if (!h || !df || !p || !E || !D) return SQPHIP_EINVAL;
    return guarded(h, [&](Ctx &C) {
        h2d(C, C.d.df, df, C.d.n); h2d(C, C.d.pstep, p, C.d.n); h2d(C, C.d.E, E, C.d.m);
        merit_eval(C, 5, 0.0, mu, 0, D);
        return SQPHIP_OK;
    });
}

extern "C" int sqphip_compute_derivative_full(sqphip_ctx *h, const double *df, const double *p, const double *E, double mu,
                                              const double *mu_vec, int32_t feasibility_restoration, const double *slack,
                                              double *D)
{
    if (!h || !E || !D) return SQPHIP_EINVAL;
    if (feasibility_restoration ? !slack : (!df || !p)) return SQPHIP_EINVAL;
    return guarded(h, [&](Ctx &C) {
        DV &d = C.d;
        h2d(C, d.E, E, d.m);
        if (feasibility_restoration) h2d(C, d.oslack, slack, 2 * (size_t)d.m);
        else { h2d(C, d.df, df, d.n); h2d(C, d.pstep, p, d.n); }
        if (mu_vec) h2d(C, d.plam, mu_vec, d.m);
        merit_eval(C, 6, 0.0, mu, (feasibility_restoration ? 1 : 0) | (mu_vec ? 2 : 0), D);
        return SQPHIP_OK;
    });
}

// ---- merit path of the batched seat: operands of request k staged into the vectors of instance inst[k], one workgroup
// of k_merit_batch per request with the arithmetic of k_merit (sqp.hip, merit_body), out[count]
namespace {
template <class Stage>
int merit_batch(sqphip_ctx *h, const char *fn, int32_t count, const int32_t *inst, int op, const double *a0, const double *a1,
                int flag, double *out, Stage &&stage)
{
    if (int rc = seat_check(h, fn, count, inst)) return rc;
    return guarded(h, [&](Ctx &C) {
        SeatCall S(C, count);
        stage(S, C.d);
        S.send(inst, nullptr, a0, a1);
        double *o = C.stg_d + S.rows0;                    // (the rows have been spread by then: same stream)
        merit_eval_batch(C, count, S.inst_dev(), op, S.a0_dev(), S.a1_dev(), flag, o);
        S.fetch(false, count);
        std::memcpy(out, C.stg_h + S.rows0, sizeof(double) * (size_t)count);
        return SQPHIP_OK;
    });
}
}  // namespace

extern "C" int sqphip_norm_violations_batch(sqphip_ctx *h, int32_t count, const int32_t *inst, const double *E, const double *x,
                                            int32_t pnorm, double *out)
{
    if (!h || !E || !x || !out || pnorm < 0 || pnorm > 2) return SQPHIP_EINVAL;
    return merit_batch(h, "sqphip_norm_violations_batch", count, inst, 0, nullptr, nullptr, pnorm, out,
                       [&](SeatCall &S, DV &d) { S.operand(E, d.E, d.m); S.operand(x, d.x, d.n); });
}

extern "C" int sqphip_kt_residuals_batch(sqphip_ctx *h, int32_t count, const int32_t *inst, const double *df,
                                         const double *lambda, const double *mult_x_U, const double *mult_x_L,
                                         const double *Jval, double *out)
{
    if (!h || !df || !lambda || !mult_x_U || !mult_x_L || !Jval || !out) return SQPHIP_EINVAL;
    return merit_batch(h, "sqphip_kt_residuals_batch", count, inst, 1, nullptr, nullptr, 0, out, [&](SeatCall &S, DV &d) {
        S.operand(df, d.df, d.n); S.operand(lambda, d.lambda, d.m); S.operand(mult_x_U, d.mxU, d.n);
        S.operand(mult_x_L, d.mxL, d.n); S.operand(Jval, d.jcoo, d.nnzj_coo);
    });
}

extern "C" int sqphip_norm_complementarity_batch(sqphip_ctx *h, int32_t count, const int32_t *inst, const double *E,
                                                 const double *lambda, int32_t pnorm, double *out)
{
    if (!h || !E || !lambda || !out || pnorm < 0 || pnorm > 2) return SQPHIP_EINVAL;
    return merit_batch(h, "sqphip_norm_complementarity_batch", count, inst, 2, nullptr, nullptr, pnorm, out,
                       [&](SeatCall &S, DV &d) { S.operand(E, d.E, d.m); S.operand(lambda, d.lambda, d.m); });
}

extern "C" int sqphip_compute_phi_batch(sqphip_ctx *h, int32_t count, const int32_t *inst, const double *f_trial,
                                        const double *E_trial, const double *x_trial, const double *mu,
                                        int32_t feasibility_restoration, double *phi)
{
    if (!h || !f_trial || !E_trial || !x_trial || !mu || !phi) return SQPHIP_EINVAL;
    return merit_batch(h, "sqphip_compute_phi_batch", count, inst, 3, f_trial, mu, feasibility_restoration, phi,
                       [&](SeatCall &S, DV &d) { S.operand(E_trial, d.E, d.m); S.operand(x_trial, d.x, d.n); });
}

extern "C" int sqphip_compute_qmodel_batch(sqphip_ctx *h, int32_t count, const int32_t *inst, const double *x, const double *p,
                                           const double *df, const double *E, const double *Jval, const double *Hval,
                                           const double *mu, int32_t with_step, double *q)
{
    if (!h || !x || !E || !mu || !q) return SQPHIP_EINVAL;
    if (with_step && (!p || !df || !Jval)) return SQPHIP_EINVAL;
    return merit_batch(h, "sqphip_compute_qmodel_batch", count, inst, 4, nullptr, mu, with_step, q, [&](SeatCall &S, DV &d) {
        S.operand(x, d.x, d.n); S.operand(E, d.E, d.m);
        if (with_step) {
            S.operand(p, d.pstep, d.n); S.operand(df, d.df, d.n); S.operand(Jval, d.jcoo, d.nnzj_coo);
            S.operand(Hval, d.hcoo, d.nnzh_coo, true);
        }
    });
}

extern "C" int sqphip_compute_derivative_full_batch(sqphip_ctx *h, int32_t count, const int32_t *inst, const double *df,
                                                    const double *p, const double *E, const double *mu, const double *mu_vec,
                                                    int32_t feasibility_restoration, const double *slack, double *D)
{
    if (!h || !E || !mu || !D) return SQPHIP_EINVAL;
    if (feasibility_restoration ? !slack : (!df || !p)) return SQPHIP_EINVAL;
    return merit_batch(h, "sqphip_compute_derivative_full_batch", count, inst, 6, nullptr, mu,
                       (feasibility_restoration ? 1 : 0) | (mu_vec ? 2 : 0), D, [&](SeatCall &S, DV &d) {
        S.operand(E, d.E, d.m);
        if (feasibility_restoration) S.operand(slack, d.oslack, 2 * d.m);
        else { S.operand(df, d.df, d.n); S.operand(p, d.pstep, d.n); }
        S.operand(mu_vec, d.plam, d.m);
    });
}

extern "C" int sqphip_compute_mu_rule_dev(sqphip_ctx *h, int32_t rule, int64_t iter, double rho, const double *x,
                                          const double *E, const double *df, const double *p, const double *Hval,
                                          const double *lambda, double *mu)
{
    if (!h || rule < 1 || rule > 3 || !x || !E || !df || !p || !lambda || !mu) return SQPHIP_EINVAL;
    return guarded(h, [&](Ctx &C) {
        DV &d = C.d;
        h2d(C, d.x, x, d.n); h2d(C, d.E, E, d.m); h2d(C, d.df, df, d.n); h2d(C, d.pstep, p, d.n);
        h2d(C, d.lambda, lambda, d.m); h2d(C, d.plam, mu, d.m);
        SQPHIP_HIP_OK(hipMemsetAsync(d.jcoo, 0, sizeof(double) * (size_t)d.nnzj_coo, C.stream));
        if (Hval) h2d(C, d.hcoo, Hval, d.nnzh_coo);
        else SQPHIP_HIP_OK(hipMemsetAsync(d.hcoo, 0, sizeof(double) * (size_t)d.nnzh_coo, C.stream));
        double t = 0.0;
        merit_eval(C, 7, rho, 0.0, rule | ((iter == 1 ? 1 : 0) << 4), &t);
        d2h(C, mu, d.plam, d.m);
        SQPHIP_HIP_OK(hipStreamSynchronize(C.stream));
        return SQPHIP_OK;
    });
}

extern "C" int sqphip_acopf_armijo(sqphip_ctx *h, int32_t inst, const double *x, const double *p, double mu, double phi0,
                                   double D, double eta, double tau, double min_alpha, int32_t feasibility_restoration,
                                   double *alpha, int32_t *is_valid, int32_t *n_eval)
{
    if (!h || !h->c.evaluator_attached || inst < 0 || inst >= h->c.d.B || !x || !p || !alpha || !is_valid) return SQPHIP_EINVAL;
    if (!(tau > 0.0 && tau < 1.0)) return SQPHIP_EINVAL;        // the loop must terminate
    return guarded(h, [&](Ctx &C) {
        DV &d = C.d;
        h2d(C, d.x + (size_t)inst * d.n, x, d.n); h2d(C, d.pstep + (size_t)inst * d.n, p, d.n);
        double out[3];
        armijo_eval(C, inst, mu, phi0, D, eta, tau, min_alpha, feasibility_restoration, out);
        *alpha = out[0]; *is_valid = (int32_t)out[1];
        if (n_eval) *n_eval = (int32_t)out[2];
        return SQPHIP_OK;
    });
}

extern "C" int sqphip_tr_update(double ared, double pred, double delta, double pnorm_inf, double delta_max,
                                double tol_direction, int32_t *accept_out, double *delta_out)
{
    if (!accept_out || !delta_out) return SQPHIP_EINVAL;
    // sqp_trust_region.jl:529-538, :574-577; isapprox with rtol = sqrt(eps)
    const double rho = ared / pred;
    const bool acc = ared > 0 && rho > 0;
    double dn = delta;
    if (acc) {
        const bool approx = delta == pnorm_inf ||
                            (std::isfinite(delta) && std::isfinite(pnorm_inf) &&
                             std::fabs(delta - pnorm_inf) <=
                                 1.4901161193847656e-08 * std::fmax(std::fabs(delta), std::fabs(pnorm_inf)));
        if (approx) dn = std::fmin(2 * delta, delta_max);
    } else {
        dn = std::fmax(0.5 * std::fmin(delta, pnorm_inf), 0.1 * tol_direction);
    }
    *accept_out = acc ? 1 : 0;
    *delta_out = dn;
    return SQPHIP_OK;
}

// sqp_line_search.jl:303-334
extern "C" int sqphip_armijo_alpha(double phi0, double D, double eta, double tau, double min_alpha, double pnorm_inf,
                                   double tol_direction, sqphip_phi_fn phi, void *user, double *alpha,
                                   int32_t *is_valid)
{
    if (!phi || !alpha || !is_valid) return SQPHIP_EINVAL;
    double a = 1.0;
    int ok = 1;
    if (!(pnorm_inf <= tol_direction)) {
        double phi_x_p = phi(a, user);
        while (phi_x_p > phi0 + eta * a * D) {
            if (a < min_alpha) { ok = 0; break; }        // the step size can become too small
            a *= tau;
            phi_x_p = phi(a, user);
        }
    }
    *alpha = a;
    *is_valid = ok;
    return SQPHIP_OK;
}

// sqp_line_search.jl:270-294
extern "C" int sqphip_compute_mu_rule(int32_t rule, int64_t iter, double rho, double viol1, double dfp,
                                      double half_pHp, int64_t m, const double *lambda, double *mu)
{
    if (rule < 1 || rule > 3 || m < 0 || (m > 0 && (!lambda || !mu))) return SQPHIP_EINVAL;
    const double denom = std::fmax((1.0 - rho) * viol1, 1.0e-8);
    const double t = (dfp + std::fmax(half_pHp, 0.0)) / denom;
    for (int64_t i = 0; i < m; ++i) {
        if (rule == 1) { mu[i] = std::fmax(mu[i], t); mu[i] = std::fmax(mu[i], std::fabs(lambda[i])); }
        else if (rule == 2) mu[i] = iter == 1 ? t : std::fmax(mu[i], std::fabs(lambda[i]));
        else mu[i] = std::fmax(mu[i], std::fabs(lambda[i]));
    }
    return SQPHIP_OK;
}

extern "C" int sqphip_acopf_eval(sqphip_ctx *h, int32_t inst, const double *x, double sigma, const double *lambda,
                                 double *f, double *grad, double *g, double *jval, double *hval)
{
    if (!h || !h->c.evaluator_attached || inst < 0 || inst >= h->c.d.B || !x) return SQPHIP_EINVAL;
    if (hval && !lambda) return SQPHIP_EINVAL;
    return guarded(h, [&](Ctx &C) {
        DV &d = C.d;
        // staging in instance-`inst` scratch vectors
        double *xd = d.tmpx + (size_t)inst * d.n, *ld = d.hlam + (size_t)inst * d.m;
        double *gd = d.tmpE + (size_t)inst * d.m, *grd = d.wn + (size_t)inst * d.n;
        double *jd = d.jcoo + (size_t)inst * d.nnzj_coo, *hd = d.hcoo + (size_t)inst * d.nnzh_coo;
        double *fd = d.wN + (size_t)inst * d.Npad;
        h2d(C, xd, x, d.n);
        if (lambda) h2d(C, ld, lambda, d.m);
        launch_acopf_eval_point(C, inst, xd, sigma, lambda ? ld : nullptr, f ? fd : nullptr, grad ? grd : nullptr,
                                g ? gd : nullptr, jval ? jd : nullptr, hval ? hd : nullptr);
        d2h(C, f, fd, 1); d2h(C, grad, grd, d.n); d2h(C, g, gd, d.m);
        d2h(C, jval, jd, d.nnzj_coo); d2h(C, hval, hd, d.nnzh_coo);
        SQPHIP_HIP_OK(hipStreamSynchronize(C.stream));
        return SQPHIP_OK;
    });
}

extern "C" int sqphip_sqp_reset(sqphip_ctx *h)
{
    if (!h || !h->c.evaluator_attached) return SQPHIP_ESTATE;
    h->c.nl.started = true;
    return guarded(h, [&](Ctx &C) { sqp_reset(C); return SQPHIP_OK; });
}

extern "C" int sqphip_sqp_run(sqphip_ctx *h, int32_t max_outer)
{
    if (!h || !h->c.evaluator_attached) return SQPHIP_ESTATE;
    h->c.nl.started = true;
    return guarded(h, [&](Ctx &C) {
        auto t0 = std::chrono::steady_clock::now();
        sqp_run(C, max_outer);
        C.total_seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        return SQPHIP_OK;
    });
}

extern "C" int sqphip_sqp_get(sqphip_ctx *h, int32_t inst, double *x, double *g, double *mult_g, double *mult_x_L,
                              double *mult_x_U, double *obj_val, int32_t *status, int32_t *iter)
{
    if (!h || inst < 0 || inst >= h->c.d.B) return SQPHIP_EINVAL;
    return guarded(h, [&](Ctx &C) {
        DV &d = C.d;
        SqpState S;
        SQPHIP_HIP_OK(hipMemcpyAsync(&S, d.sst + inst, sizeof(SqpState), hipMemcpyDeviceToHost, C.stream));
        d2h(C, x, d.x + (size_t)inst * d.n, d.n); d2h(C, g, d.E + (size_t)inst * d.m, d.m);
        d2h(C, mult_g, d.lambda + (size_t)inst * d.m, d.m);
        d2h(C, mult_x_L, d.mxL + (size_t)inst * d.n, d.n); d2h(C, mult_x_U, d.mxU + (size_t)inst * d.n, d.n);
        SQPHIP_HIP_OK(hipStreamSynchronize(C.stream));
        // sqp_trust_region.jl:219-220: mult_g = -lambda, mult_x_U = -mult_x_U
        if (mult_g) for (int i = 0; i < d.m; ++i) mult_g[i] = -mult_g[i];
        if (mult_x_U) for (int j = 0; j < d.n; ++j) mult_x_U[j] = -mult_x_U[j];
        if (obj_val) *obj_val = S.obj_val;
        if (status) *status = S.ret;
        if (iter) *iter = S.iter;
        return SQPHIP_OK;
    });
}

extern "C" int sqphip_sqp_status(sqphip_ctx *h, int32_t *ret_codes, int32_t *iters, int32_t *done)
{
    if (!h) return SQPHIP_EINVAL;
    return guarded(h, [&](Ctx &C) {
        std::vector<SqpState> S(C.d.B);
        SQPHIP_HIP_OK(hipMemcpyAsync(S.data(), C.d.sst, sizeof(SqpState) * C.d.B, hipMemcpyDeviceToHost, C.stream));
        SQPHIP_HIP_OK(hipStreamSynchronize(C.stream));
        for (int b = 0; b < C.d.B; ++b) {
            if (ret_codes) ret_codes[b] = S[b].ret;
            if (iters) iters[b] = S[b].iter;
            if (done) done[b] = S[b].done;
        }
        return SQPHIP_OK;
    });
}

extern "C" int sqphip_sqp_trace(sqphip_ctx *h, int32_t inst, double *rows, int32_t cap, int32_t *len)
{
    if (!h || inst < 0 || inst >= h->c.d.B || !len) return SQPHIP_EINVAL;
    return guarded(h, [&](Ctx &C) {
        SqpState S;
        SQPHIP_HIP_OK(hipMemcpyAsync(&S, C.d.sst + inst, sizeof(SqpState), hipMemcpyDeviceToHost, C.stream));
        SQPHIP_HIP_OK(hipStreamSynchronize(C.stream));
        *len = S.trace_len;
        const int k = std::min<int>({cap, S.trace_len, SQPHIP_TRACE_CAP});
        if (rows && k > 0)
            d2h(C, rows, C.d.trace + (size_t)inst * SQPHIP_TRACE_CAP * SQPHIP_TRACE_COLS,
                (size_t)k * SQPHIP_TRACE_COLS);
        SQPHIP_HIP_OK(hipStreamSynchronize(C.stream));
        return SQPHIP_OK;
    });
}

extern "C" int sqphip_get_counters(sqphip_ctx *h, sqphip_counters *c)
{
    if (!h || !c) return SQPHIP_EINVAL;
    return guarded(h, [&](Ctx &C) {
        std::vector<SqpState> S(C.d.B);
        SQPHIP_HIP_OK(hipMemcpyAsync(S.data(), C.d.sst, sizeof(SqpState) * C.d.B, hipMemcpyDeviceToHost, C.stream));
        SQPHIP_HIP_OK(hipStreamSynchronize(C.stream));
        C.tm.flush();
        double lane_factor = 0, lane_trailing = 0, lane_solve = 0;
        long lane_sweeps = 0;
        for (auto &L : C.lanes) {
            L->tm.flush();
            lane_factor += L->tm.factor_seconds; lane_trailing += L->tm.trailing_seconds; lane_solve += L->tm.solve_seconds;
            lane_sweeps += L->n_sweeps;
        }
        int64_t nqp = C.n_qp, nip = C.n_ipm_iter, nf = C.n_factor, nsol = C.n_solve;
        for (auto &s : S) { nqp += s.n_qp; nip += s.tot_ipm; nf += s.tot_fac; nsol += s.tot_sol; }
        c->n_qp = nqp; c->n_ipm_iter = nip; c->n_factor = nf;
        const double N = (double)C.d.Nf;
        c->kkt_order = C.d.Nf;
        c->lead_tiles = C.d.Ts;
        c->trailing_flops_per_factor = ldlt_trailing_flops(C.plan);
        c->ldlt_flops = (double)nf * N * N * N / 3.0;
        c->ldlt_seconds = C.tm.factor_seconds + lane_factor; c->trailing_seconds = C.tm.trailing_seconds + lane_trailing;
        c->solve_seconds = C.tm.solve_seconds + lane_solve; c->total_seconds = C.total_seconds;
        c->trailing_launches = C.tm.trailing_launches;
        c->n_sweeps = C.n_sweeps + lane_sweeps; c->n_solve = nsol; c->n_groups = C.lanes.empty() ? 1 : (int64_t)C.lanes.size();
        c->sparse = C.d.sparse; c->nnz_k = 0; c->nnz_l = 0; c->n_supernodes = 0; c->n_levels = 0; c->max_front = 0;
        c->factor_flops = 0; c->front_doubles = 0; c->cb_doubles = 0; c->factor_launches = 0; c->solve_launches = 0;
        c->nnz_l_top = 0; c->nnz_k_top = 0; c->cols_top = 0;
        if (C.d.sparse) {
            const SparseSym &Y = C.mfp().S;
            c->nnz_k = C.mfp().nnzK; c->nnz_l = Y.nnzL; c->n_supernodes = Y.ns; c->n_levels = Y.nlevels;
            c->max_front = Y.max_front; c->factor_flops = Y.flops; c->front_doubles = C.mfp().stride;
            long cb = 0;
            for (int q = 0; q < Y.ns; ++q) cb += (long)(Y.sn_nr[q] + 1) * Y.sn_nr[q] - (long)Y.sn_nr[q] * (Y.sn_nr[q] - 1) / 2;
            c->cb_doubles = cb;
            long lt = 0, kt = 0, nct = 0;
            for (int q = 0; q < Y.ns; ++q)
                if (C.mfp().fac[C.mfp().launch_of[q]].level >= C.mfp().narrow_level) {      // (by the launch the front runs in: the timers open per launch level)
                    const long nc = Y.sn_nc[q], nr = Y.sn_nr[q];
                    lt += nc * (nc - 1) / 2 + nc * nr; kt += C.mfp().asm_ptr[q + 1] - C.mfp().asm_ptr[q]; nct += nc;
                }
            c->nnz_l_top = lt; c->nnz_k_top = kt; c->cols_top = nct;
            c->factor_launches = (int64_t)(C.d.mf.sp_n > 0 ? C.mfp().fac_below + 1 : (int)C.mfp().fac.size());   // (+ k_mf_values)
            c->solve_launches = (int64_t)(C.mfp().fwd.size() + C.mfp().bwd.size() + (C.mfp().top.count > 0 ? 1 : 0));
            c->ldlt_flops = (double)nf * Y.flops;
        }
        return SQPHIP_OK;
    });
}

extern "C" int sqphip_get_mode_counters(sqphip_ctx *h, int64_t *out)
{
    if (!h || !out) return SQPHIP_EINVAL;
    return guarded(h, [&](Ctx &C) -> int {
        for (int k = 0; k < 12; ++k) out[k] = 0;
        if (!C.d.sst) return SQPHIP_OK;
        std::vector<SqpState> S((size_t)C.d.B);
        SQPHIP_HIP_OK(hipMemcpyAsync(S.data(), C.d.sst, sizeof(SqpState) * C.d.B, hipMemcpyDeviceToHost, C.stream));
        SQPHIP_HIP_OK(hipStreamSynchronize(C.stream));
        for (auto &s : S)
            for (int k = 0; k < 4; ++k) { out[3 * k] += s.md_qp[k]; out[3 * k + 1] += s.md_ipm[k]; out[3 * k + 2] += s.md_fac[k]; }
        return SQPHIP_OK;
    });
}

extern "C" int sqphip_sqp_work(sqphip_ctx *h, int64_t *qp, int64_t *ipm, int64_t *fac)
{
    if (!h) return SQPHIP_EINVAL;
    return guarded(h, [&](Ctx &C) -> int {
        if (!C.d.sst) return SQPHIP_EINVAL;
        std::vector<SqpState> S((size_t)C.d.B);
        SQPHIP_HIP_OK(hipMemcpyAsync(S.data(), C.d.sst, sizeof(SqpState) * C.d.B, hipMemcpyDeviceToHost, C.stream));
        SQPHIP_HIP_OK(hipStreamSynchronize(C.stream));
        for (int b = 0; b < C.d.B; ++b) {
            if (qp) qp[b] = S[b].n_qp;
            if (ipm) ipm[b] = S[b].tot_ipm;
            if (fac) fac[b] = S[b].tot_fac;
        }
        return SQPHIP_OK;
    });
}

extern "C" int sqphip_sqp_qp_log(sqphip_ctx *h, int32_t inst, int32_t *rows, int32_t cap, int32_t *n_rows)
{
    if (!h || !rows || !n_rows || cap < 0) return SQPHIP_EINVAL;
    return guarded(h, [&](Ctx &C) -> int {
        if (!C.d.sst || inst < 0 || inst >= C.d.B) return SQPHIP_EINVAL;
        SqpState S;
        SQPHIP_HIP_OK(hipMemcpyAsync(&S, C.d.sst + inst, sizeof(SqpState), hipMemcpyDeviceToHost, C.stream));
        SQPHIP_HIP_OK(hipStreamSynchronize(C.stream));
        const int have = S.qlog_n < SQPHIP_QLOG_CAP ? S.qlog_n : SQPHIP_QLOG_CAP, n = have < cap ? have : cap;
        for (int k = 0; k < n; ++k) {
            const int src = (S.qlog_n - n + k) % SQPHIP_QLOG_CAP;
            for (int c = 0; c < 4; ++c) rows[4 * k + c] = S.qlog[4 * src + c];
        }
        *n_rows = n;
        return SQPHIP_OK;
    });
}

extern "C" int sqphip_sqp_qp_log_term(sqphip_ctx *h, int32_t inst, double *scaled_error, int32_t *rule, int32_t cap, int32_t *n_rows)
{
    if (!h || !n_rows || cap < 0) return SQPHIP_EINVAL;
    return guarded(h, [&](Ctx &C) -> int {
        if (!C.d.sst || inst < 0 || inst >= C.d.B) return SQPHIP_EINVAL;
        SqpState S;
        SQPHIP_HIP_OK(hipMemcpyAsync(&S, C.d.sst + inst, sizeof(SqpState), hipMemcpyDeviceToHost, C.stream));
        SQPHIP_HIP_OK(hipStreamSynchronize(C.stream));
        const int have = S.qlog_n < SQPHIP_QLOG_CAP ? S.qlog_n : SQPHIP_QLOG_CAP, n = have < cap ? have : cap;
        for (int k = 0; k < n; ++k) {
            const int src = (S.qlog_n - n + k) % SQPHIP_QLOG_CAP;
            if (scaled_error) scaled_error[k] = (double)S.qerr[src];
            if (rule) rule[k] = (int32_t)S.qrule[src];
        }
        *n_rows = n;
        return SQPHIP_OK;
    });
}

extern "C" int sqphip_get_termination_counters(sqphip_ctx *h, int64_t *out)
{
    if (!h || !out) return SQPHIP_EINVAL;
    return guarded(h, [&](Ctx &C) -> int {
        for (int k = 0; k < 4; ++k) out[k] = 0;
        if (!C.d.sst) return SQPHIP_OK;
        std::vector<SqpState> S((size_t)C.d.B);
        SQPHIP_HIP_OK(hipMemcpyAsync(S.data(), C.d.sst, sizeof(SqpState) * C.d.B, hipMemcpyDeviceToHost, C.stream));
        SQPHIP_HIP_OK(hipStreamSynchronize(C.stream));
        for (auto &s : S) for (int k = 0; k < 4; ++k) out[k] += s.term_rule[k];
        return SQPHIP_OK;
    });
}

extern "C" int sqphip_sqp_last_request(sqphip_ctx *h, int32_t inst, int32_t *mode, double *delta, double *mu_pen,
                                       double *x_k, double *c, double *b, double *jac_coo, double *hess_coo)
{
    if (!h) return SQPHIP_EINVAL;
    return guarded(h, [&](Ctx &C) -> int {
        const DV &d = C.d;
        if (!d.ist || inst < 0 || inst >= d.B) return SQPHIP_EINVAL;
        IpmState I;
        SQPHIP_HIP_OK(hipMemcpyAsync(&I, d.ist + inst, sizeof(IpmState), hipMemcpyDeviceToHost, C.stream));
        auto get = [&](double *dst, const double *src, long stride) {
            if (dst && stride > 0)
                SQPHIP_HIP_OK(hipMemcpyAsync(dst, src + inst * stride, sizeof(double) * stride, hipMemcpyDeviceToHost, C.stream));
        };
        get(x_k, d.xk, d.n); get(c, d.cin, d.n); get(b, d.bE, d.m);
        get(jac_coo, d.jcoo, d.nnzj_coo); get(hess_coo, d.hcoo, d.nnzh_coo);
        SQPHIP_HIP_OK(hipStreamSynchronize(C.stream));
        if (mode) *mode = I.mode;
        if (delta) *delta = I.delta;
        if (mu_pen) *mu_pen = I.mu_pen;
        return SQPHIP_OK;
    });
}

// ---- scenario queue: more scenarios than slots ----------------------------------------------------------------
extern "C" int sqphip_sqp_stream_begin(sqphip_ctx *h, int32_t n_scenarios)
{
    if (acopf_only(h, "sqphip_sqp_stream_begin")) return SQPHIP_EINVAL;
    if (!h || !h->c.evaluator_attached || n_scenarios <= 0) return SQPHIP_EINVAL;
    return stream_begin(h, n_scenarios, 0, -1);      // (api_models.hip: the tables of the three kinds of queue)
}

extern "C" int sqphip_sqp_stream_set(sqphip_ctx *h, int32_t scen, const double *xL, const double *xU, const double *gL,
                                     const double *gU, const double *ohm, const double *c2, const double *c1,
                                     const double *x0)
{
    if (acopf_only(h, "sqphip_sqp_stream_set")) return SQPHIP_EINVAL;
    if (!h || scen < 0 || scen >= h->c.d.stream.M || !xL || !xU || !gL || !gU || !ohm || !c2 || !c1 || !x0) return SQPHIP_EINVAL;
    for (int i = 0; i < h->c.d.m; ++i) {
        if (gL[i] == -INFINITY && gU[i] == INFINITY) return SQPHIP_EINVAL;
        if (h->c.d.condense && gL[i] == gU[i] && h->c.h_kpos[i] < 0) {
            h->c.err = "sqphip_sqp_stream_set: row " + std::to_string(i) + " is an equality for this scenario but was not one when "
                       "the context was created (options.kkt_condense = 1 fixes the kept rows)";
            return SQPHIP_EINVAL;
        }
    }
    return guarded(h, [&](Ctx &C) {
        DV &d = C.d;
        const StreamDev &Q = d.stream;
        const size_t s = (size_t)scen;
        h2d(C, const_cast<double *>(Q.xL) + s * d.n, xL, d.n); h2d(C, const_cast<double *>(Q.xU) + s * d.n, xU, d.n);
        h2d(C, const_cast<double *>(Q.x0) + s * d.n, x0, d.n);
        h2d(C, const_cast<double *>(Q.gL) + s * d.m, gL, d.m); h2d(C, const_cast<double *>(Q.gU) + s * d.m, gU, d.m);
        h2d(C, const_cast<double *>(Q.ohm) + s * d.nl * 12, ohm, (size_t)d.nl * 12);
        h2d(C, const_cast<double *>(Q.c2) + s * d.ng, c2, d.ng); h2d(C, const_cast<double *>(Q.c1) + s * d.ng, c1, d.ng);
        SQPHIP_HIP_OK(hipStreamSynchronize(C.stream));
        return SQPHIP_OK;
    });
}

extern "C" int sqphip_sqp_stream_run(sqphip_ctx *h)
{
    if (!h || !h->c.evaluator_attached || h->c.d.stream.M <= 0) return SQPHIP_ESTATE;
    return guarded(h, [&](Ctx &C) {
        auto t0 = std::chrono::steady_clock::now();
        SQPHIP_HIP_OK(hipMemsetAsync(C.d.stream.next, 0, sizeof(int), C.stream));
        SQPHIP_HIP_OK(hipMemsetAsync(C.d.stream.riter, 0xff, sizeof(int) * (size_t)C.d.stream.M, C.stream));   // results of an earlier pass are not this pass's
        sqp_stream_arm(C);
        C.stream_started = true;
        sqp_run(C, 0);
        C.total_seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        return SQPHIP_OK;
    });
}

// ---- a queue shared between ranks (SURVEY.md section 8f-4 remainder): every rank holds the tables of ALL scenarios
// (sqphip_sqp_stream_set) but hands out only the ids assigned to it; between budgeted runs the host moves unstarted ids
// from a rank that still has many to one whose queue ran dry (sqpsolver.jl_amd/shard.py, run_shared_queue).  No iterate
// crosses ranks: a scenario is solved from start to end by the rank that drew it, and its result does not depend on
// which rank or slot that was.
static int stream_state(Ctx &C, int &next, int &end)
{
    SQPHIP_HIP_OK(hipMemcpyAsync(&next, C.d.stream.next, sizeof(int), hipMemcpyDeviceToHost, C.stream));
    SQPHIP_HIP_OK(hipMemcpyAsync(&end, C.d.stream.qend, sizeof(int), hipMemcpyDeviceToHost, C.stream));
    SQPHIP_HIP_OK(hipStreamSynchronize(C.stream));
    if (next > end) next = end;                     // slots that found the queue empty overshoot by one each
    return SQPHIP_OK;
}

extern "C" int sqphip_sqp_stream_assign(sqphip_ctx *h, int32_t n, const int32_t *ids)
{
    if (!h || h->c.d.stream.M <= 0 || n < 0 || n > h->c.d.stream.M || (n > 0 && !ids)) return SQPHIP_EINVAL;
    for (int k = 0; k < n; ++k) if (ids[k] < 0 || ids[k] >= h->c.d.stream.M) return SQPHIP_EINVAL;
    return guarded(h, [&](Ctx &C) {
        const int zero = 0;
        if (n > 0) SQPHIP_HIP_OK(hipMemcpyAsync(C.d.stream.qids, ids, sizeof(int) * (size_t)n, hipMemcpyHostToDevice, C.stream));
        SQPHIP_HIP_OK(hipMemcpyAsync(C.d.stream.qend, &n, sizeof(int), hipMemcpyHostToDevice, C.stream));
        SQPHIP_HIP_OK(hipMemcpyAsync(C.d.stream.next, &zero, sizeof(int), hipMemcpyHostToDevice, C.stream));
        SQPHIP_HIP_OK(hipMemsetAsync(C.d.stream.riter, 0xff, sizeof(int) * (size_t)C.d.stream.M, C.stream));   // nothing filed yet under the new assignment
        SQPHIP_HIP_OK(hipStreamSynchronize(C.stream));
        C.stream_started = false;
        return SQPHIP_OK;
    });
}

extern "C" int sqphip_sqp_stream_append(sqphip_ctx *h, int32_t n, const int32_t *ids)
{
    if (!h || h->c.d.stream.M <= 0 || n < 0 || (n > 0 && !ids)) return SQPHIP_EINVAL;
    for (int k = 0; k < n; ++k) if (ids[k] < 0 || ids[k] >= h->c.d.stream.M) return SQPHIP_EINVAL;
    return guarded(h, [&](Ctx &C) {
        int next, end;
        stream_state(C, next, end);
        if (end + n > C.d.stream.M) { C.err = "sqphip_sqp_stream_append: more ids than scenario tables"; return SQPHIP_EINVAL; }
        if (n > 0) SQPHIP_HIP_OK(hipMemcpyAsync(C.d.stream.qids + end, ids, sizeof(int) * (size_t)n, hipMemcpyHostToDevice, C.stream));
        const int ne = end + n;
        SQPHIP_HIP_OK(hipMemcpyAsync(C.d.stream.qend, &ne, sizeof(int), hipMemcpyHostToDevice, C.stream));
        SQPHIP_HIP_OK(hipMemcpyAsync(C.d.stream.next, &next, sizeof(int), hipMemcpyHostToDevice, C.stream));   // undo the overshoot
        SQPHIP_HIP_OK(hipStreamSynchronize(C.stream));
        return SQPHIP_OK;
    });
}

extern "C" int sqphip_sqp_stream_release(sqphip_ctx *h, int32_t n, int32_t *ids_out, int32_t *n_out)
{
    if (!h || h->c.d.stream.M <= 0 || n < 0 || !n_out || (n > 0 && !ids_out)) return SQPHIP_EINVAL;
    return guarded(h, [&](Ctx &C) {
        int next, end;
        stream_state(C, next, end);
        const int k = std::min(n, end - next), ne = end - k;
        if (k > 0) SQPHIP_HIP_OK(hipMemcpyAsync(ids_out, C.d.stream.qids + ne, sizeof(int) * (size_t)k, hipMemcpyDeviceToHost, C.stream));
        SQPHIP_HIP_OK(hipMemcpyAsync(C.d.stream.qend, &ne, sizeof(int), hipMemcpyHostToDevice, C.stream));
        SQPHIP_HIP_OK(hipMemcpyAsync(C.d.stream.next, &next, sizeof(int), hipMemcpyHostToDevice, C.stream));
        SQPHIP_HIP_OK(hipStreamSynchronize(C.stream));
        *n_out = k;
        return SQPHIP_OK;
    });
}

// every slot performs up to `max_outer` more outer iterations (of whatever scenarios it holds or draws); afterwards
// n_unstarted = ids of this rank's queue nobody has drawn yet, n_active = slots with a run in progress
extern "C" int sqphip_sqp_stream_run_some(sqphip_ctx *h, int32_t max_outer, int32_t *n_unstarted, int32_t *n_active)
{
    if (!h || !h->c.evaluator_attached || h->c.d.stream.M <= 0 || max_outer < 1) return SQPHIP_ESTATE;
    return guarded(h, [&](Ctx &C) {
        auto t0 = std::chrono::steady_clock::now();
        if (!C.stream_started) { sqp_stream_arm(C); C.stream_started = true; }
        else sqp_stream_rearm(C);
        sqp_run(C, max_outer);
        C.total_seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        int next, end;
        stream_state(C, next, end);
        if (n_unstarted) *n_unstarted = end - next;
        if (n_active) {
            std::vector<int> slot(C.d.B);
            std::vector<SqpState> S(C.d.B);
            SQPHIP_HIP_OK(hipMemcpyAsync(slot.data(), C.d.stream.slot_scen, sizeof(int) * C.d.B, hipMemcpyDeviceToHost, C.stream));
            SQPHIP_HIP_OK(hipMemcpyAsync(S.data(), C.d.sst, sizeof(SqpState) * C.d.B, hipMemcpyDeviceToHost, C.stream));
            SQPHIP_HIP_OK(hipStreamSynchronize(C.stream));
            int a = 0;
            for (int b = 0; b < C.d.B; ++b) a += slot[b] >= 0 && !S[b].done;
            *n_active = a;
        }
        return SQPHIP_OK;
    });
}

extern "C" int sqphip_sqp_stream_get(sqphip_ctx *h, int32_t scen, double *x, double *obj_val, int32_t *status, int32_t *iter)
{
    if (!h || scen < 0 || scen >= h->c.d.stream.M) return SQPHIP_EINVAL;
    return guarded(h, [&](Ctx &C) {
        const DV &d = C.d;
        const StreamDev &Q = d.stream;
        d2h(C, x, Q.rx + (size_t)scen * d.n, d.n);
        d2h(C, obj_val, Q.robj + scen, 1);
        int st = 0, it = 0;
        SQPHIP_HIP_OK(hipMemcpyAsync(&st, Q.rstat + scen, sizeof(int), hipMemcpyDeviceToHost, C.stream));
        SQPHIP_HIP_OK(hipMemcpyAsync(&it, Q.riter + scen, sizeof(int), hipMemcpyDeviceToHost, C.stream));
        SQPHIP_HIP_OK(hipStreamSynchronize(C.stream));
        if (status) *status = st;
        if (iter) *iter = it;
        return SQPHIP_OK;
    });
}

extern "C" int sqphip_sqp_stream_get_full(sqphip_ctx *h, int32_t scen, double *x, double *g, double *mult_g, double *mult_x_L,
                                          double *mult_x_U, double *obj_val, int32_t *status, int32_t *iter)
{
    if (!h || scen < 0 || scen >= h->c.d.stream.M) return SQPHIP_EINVAL;
    if (!h->c.d.stream.rE) {
        h->c.err = "sqphip_sqp_stream_get_full: the queue keeps no multipliers (sqphip_qcqp_stream_begin / sqphip_nlp_stream_begin with keep_multipliers = 1)";
        return SQPHIP_ESTATE;
    }
    return guarded(h, [&](Ctx &C) {
        const DV &d = C.d;
        const StreamDev &Q = d.stream;
        const size_t s = (size_t)scen;
        d2h(C, x, Q.rx + s * d.n, d.n); d2h(C, g, Q.rE + s * d.m, d.m); d2h(C, mult_g, Q.rlam + s * d.m, d.m);
        d2h(C, mult_x_L, Q.rmxL + s * d.n, d.n); d2h(C, mult_x_U, Q.rmxU + s * d.n, d.n);
        d2h(C, obj_val, Q.robj + s, 1);
        int st = 0, it = 0;
        SQPHIP_HIP_OK(hipMemcpyAsync(&st, Q.rstat + s, sizeof(int), hipMemcpyDeviceToHost, C.stream));
        SQPHIP_HIP_OK(hipMemcpyAsync(&it, Q.riter + s, sizeof(int), hipMemcpyDeviceToHost, C.stream));
        SQPHIP_HIP_OK(hipStreamSynchronize(C.stream));
        // as sqphip_sqp_get (sqp_trust_region.jl:219-220): mult_g = -lambda, mult_x_U = -mult_x_U
        if (mult_g) for (int i = 0; i < d.m; ++i) mult_g[i] = -mult_g[i];
        if (mult_x_U) for (int j = 0; j < d.n; ++j) mult_x_U[j] = -mult_x_U[j];
        if (status) *status = st;
        if (iter) *iter = it;
        return SQPHIP_OK;
    });
}

// seconds of kernel time by class (sqphip.h: sqphip_get_kernel_times), summed over the instance groups, and launch groups timed
extern "C" int sqphip_get_kernel_times(sqphip_ctx *h, double *seconds, int64_t *groups, int32_t cap)
{
    if (!h || !seconds || !groups || cap < 0) return SQPHIP_EINVAL;
    return guarded(h, [&](Ctx &C) -> int {
        C.tm.flush();
        for (auto &L : C.lanes) L->tm.flush();
        for (int c = 0; c < cap; ++c) {
            seconds[c] = 0.0; groups[c] = 0;
            if (c >= KC_COUNT) continue;
            seconds[c] = C.tm.class_seconds[c]; groups[c] = C.tm.class_groups[c];
            for (auto &L : C.lanes) { seconds[c] += L->tm.class_seconds[c]; groups[c] += L->tm.class_groups[c]; }
        }
        return SQPHIP_OK;
    });
}

extern "C" int sqphip_reset_counters(sqphip_ctx *h)
{
    if (!h) return SQPHIP_EINVAL;
    Ctx &C = h->c;
    C.tm.flush();
    C.tm.trailing_seconds = C.tm.factor_seconds = C.tm.solve_seconds = 0;
    C.tm.trailing_launches = 0; C.tm.n_factor = 0;
    for (int c = 0; c < KC_COUNT; ++c) { C.tm.class_seconds[c] = 0; C.tm.class_groups[c] = 0; }
    C.n_qp = C.n_ipm_iter = C.n_factor = C.n_solve = 0; C.total_seconds = 0; C.n_sweeps = 0;
    for (auto &L : C.lanes) {
        L->tm.flush();
        L->tm.trailing_seconds = L->tm.factor_seconds = L->tm.solve_seconds = 0; L->tm.trailing_launches = 0; L->tm.n_factor = 0;
        for (int c = 0; c < KC_COUNT; ++c) { L->tm.class_seconds[c] = 0; L->tm.class_groups[c] = 0; }
        L->n_sweeps = 0;
    }
    return SQPHIP_OK;
}

// enable / disable HIP-event timing of the factor, trailing-update and solve kernels
extern "C" int sqphip_set_timing(sqphip_ctx *h, int32_t enabled)
{
    if (!h) return SQPHIP_EINVAL;
    h->c.tm.flush();
    h->c.tm.enabled = enabled != 0; h->c.tm.detail = enabled == 2;
    for (auto &L : h->c.lanes) { L->tm.flush(); L->tm.enabled = enabled != 0; L->tm.detail = enabled == 2; }
    return SQPHIP_OK;
}
