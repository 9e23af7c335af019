// sqp.hip -- device-resident SQP-TR outer loop for a batch of instances, and the merit kernels.
//
// Restates, per instance and entirely in HBM, what `run!(sqp::AbstractSqpTrOptimizer)` does
// (/root/reference/src/algorithms/sqp_trust_region.jl:98-223) with the state of
// sqp_trust_region.jl:26-91, plus
//   violation_of_linear_constraints :237-254,  sub_optimize_lp! :264-304 (dropzeros! utils.jl:16-22),
//   compute_step! :370-380,  sub_optimize_soc! :341-360,  compute_qmodel :487-508,  do_step! :515-579,
//   eval_functions! sqp.jl:86-104,  compute_phi sqp.jl:170-183,  terminate_by_iterlimit sqp.jl:215-224,
//   norm_violations / KT_residuals common.jl:54-77 / :14-23.
// The quirks of the reference are reproduced; `literal_quirks = 0` switches
// #2/#3 to the textbook signs.  The callbacks are the device ACOPF evaluator (acopf_dev.hpp).
// One 256-thread workgroup per instance; the host only sequences the kernels and the sub-solves.
#include "ctx.hpp"
#include "dev_util.hpp"
#include "sqp_dev.hpp"
#include <cmath>
#include <chrono>
#include <thread>

namespace sqphip {

__global__ __launch_bounds__(TPB) void k_sqp_reset(DV d) { reset_instance(d, blockIdx.x, false); }

__global__ __launch_bounds__(TPB) void k_sqp_begin(DV d) { b_sqp_begin(d); }

__global__ void k_sqp_budget(DV d, int budget)
{
    for (int i = threadIdx.x; i < d.B; i += blockDim.x) d.sst[i].budget = budget;
}

__global__ void k_sqp_count(DV d, int *host_slot)
{
    // counters[2] = instances that still have work in this run, [3] = pending sub-problem starts; host_slot: the same
    // two words in pinned host memory (written from here: one launch per sweep less than a device-to-host copy behind it)
    // host_slot[1] (round 4): instances waiting for a refinement solve (PH_RESOLVE) -- with the monotone rule the second solve
    // slot of a sweep is launched only when the host has seen one (ipm_sweep, Ctx::want_resolve)
    // (Where k_ipm_post is the last kernel of the sweep it forms the same three counts itself -- b_sweep_count, ipm.hip -- and this
    //  kernel is not launched; it remains for the other paths and for the side-stream mode, whose hand-over lives here.)
    int nb = 0, ns = 0, nr = 0;
    for (int i = threadIdx.x; i < d.B; i += blockDim.x) {
        // transitions on a side stream: the hand-over between the two sides (ctx.hpp, the PH_ enum); both streams are
        // quiet here -- this launch is behind the event of the side job, the next side job is behind this launch's
        if (d.side == 2) {
            const int ph = d.phase[i];
            if (ph == PH_DONE2) d.phase[i] = PH_DONE;
            else if (ph == PH_PEND) d.phase[i] = PH_FACTOR;
        }
        const SqpState &S = d.sst[i];
        if (!S.done && (S.budget > 0 || S.stage != ST_TOP)) ++nb;
        if (d.ist[i].start) ++ns;
        if (d.phase[i] == PH_RESOLVE) ++nr;
    }
    __shared__ int a[64], b[64], c[64];
    a[threadIdx.x] = nb; b[threadIdx.x] = ns; c[threadIdx.x] = nr;
    __syncthreads();
    if (threadIdx.x == 0) {
        int s0 = 0, s1 = 0, s2 = 0;
        for (int k = 0; k < (int)blockDim.x; ++k) { s0 += a[k]; s1 += b[k]; s2 += c[k]; }
        d.counters[2] = s0; d.counters[3] = s1;
        if (host_slot) { host_slot[0] = s0; host_slot[1] = s2; __threadfence_system(); }
    }
}

// scenario queue: every slot starts "terminated, nothing to file" and draws its first scenario in the first sweep
__global__ void k_sqp_stream_arm(DV d)
{
    for (int i = threadIdx.x; i < d.B; i += blockDim.x) {
        d.sst[i].done = 1; d.sst[i].stage = ST_DONE; d.stream.slot_scen[i] = -2;
    }
}

void sqp_stream_arm(Ctx &C)
{
    hipLaunchKernelGGL(k_sqp_reset, dim3(C.d.B), dim3(TPB), 0, C.stream, C.d);
    hipLaunchKernelGGL(k_sqp_stream_arm, dim3(1), dim3(256), 0, C.stream, C.d);
    SQPHIP_HIP_OK(hipStreamSynchronize(C.stream));
}

// slots that found the queue empty (-1) look again: ids may have been appended since (sqphip_sqp_stream_append)
__global__ void k_sqp_stream_rearm(DV d)
{
    for (int i = threadIdx.x; i < d.B; i += blockDim.x)
        if (d.stream.slot_scen[i] == -1) d.stream.slot_scen[i] = -2;
}

void sqp_stream_rearm(Ctx &C)
{
    hipLaunchKernelGGL(k_sqp_stream_rearm, dim3(1), dim3(256), 0, C.stream, C.d);
    SQPHIP_HIP_OK(hipStreamSynchronize(C.stream));
}

void sqp_reset(Ctx &C)
{
    hipLaunchKernelGGL(k_sqp_reset, dim3(C.d.B), dim3(TPB), 0, C.stream, C.d);
    SQPHIP_HIP_OK(hipStreamSynchronize(C.stream));
}

// Every instance performs up to `max_outer` more outer iterations of run! (0 = until it terminates).
// Continuous batching: one fixed kernel sequence per sweep; every kernel is gated on the per-instance
// stage / phase, so an instance whose sub-problem has converged goes through its merit step and into
// its next sub-problem while the others are still iterating -- no instance waits for the slowest.
static void sqp_run_lane(Ctx &C, int max_outer);

// With instance groups (Ctx::lanes) every group runs the same loop on its own stream from its own host thread;
// instances never interact, so the results do not depend on the grouping.
void sqp_run(Ctx &C, int max_outer)
{
    if (C.lanes.empty()) { sqp_run_lane(C, max_outer); return; }
    std::vector<std::thread> th;
    std::vector<std::string> errs(C.lanes.size());
    // nothing may leave a lane thread as an exception (std::terminate would take the host application down), and a
    // failure to start thread k must not destroy the joinable threads 0..k-1
    try {
        for (size_t g = 0; g < C.lanes.size(); ++g)
            th.emplace_back([&, g] {
                try {
                    SQPHIP_HIP_OK(hipSetDevice(C.opt.device));
                    sqp_run_lane(*C.lanes[g], max_outer);
                } catch (const std::string &e) { errs[g] = e; }
                catch (const std::bad_alloc &) { errs[g] = "sqphip: out of host memory in an instance group"; }
                catch (const std::exception &e) { errs[g] = std::string("sqphip: instance group: ") + e.what(); }
                catch (...) { errs[g] = "sqphip: unknown exception in an instance group"; }
            });
    } catch (...) {
        for (auto &t : th) t.join();
        throw std::string("sqphip: could not start the instance-group threads");
    }
    for (auto &t : th) t.join();
    for (auto &e : errs) if (!e.empty()) throw e;
}

static void sqp_run_lane(Ctx &C, int max_outer)
{
    DV &d = C.d;
    hipStream_t s = C.stream;
    const dim3 gB(d.B), bT(TPB);
    C.run_sweep = 0;                     // (the first sweep of a run always carries the transitions: ipm_sweep)
    C.want_resolve = true;               // (... and the refinement slot, until the first counter has come back)
    C.resolve_served = -1;
    // transitions on a side stream (ctx.hpp, the PH_ enum; ipm_sweep): monotone rule, sparse path, one-workgroup vector stages
    C.side_on = C.side_mode && d.sparse && !d.flat && d.ipm_corrector == 0 && d.B >= 8;
    if (C.side_on && !C.side) {
        SQPHIP_HIP_OK(hipStreamCreateWithFlags(&C.side, hipStreamNonBlocking));
        for (auto &e : C.evS) SQPHIP_HIP_OK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        for (auto &e : C.evC) SQPHIP_HIP_OK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    d.side = C.side_on ? 2 : 0;
    struct SideOff { Ctx &C; ~SideOff() { C.d.side = 0; C.side_on = false; C.d.spec_mode = C.spec_mode0; } } side_off{C};     // (other entry points run in line)
    hipLaunchKernelGGL(k_sqp_budget, dim3(1), dim3(64), 0, s, d, max_outer > 0 ? max_outer : 0x3fffffff);
    hipLaunchKernelGGL(k_sqp_begin, gB, bT, 0, s, d);
    SQPHIP_HIP_OK(hipMemsetAsync(d.counters + 4, 0, 4 * sizeof(int), s));      // accumulators and ticket of b_sweep_count (a run that failed may have left them)
    // The "anyone left?" counter of sweep k is read while sweep k + 1 is already queued: the stream never runs dry
    // behind a host round trip.  The price is one sweep of gated-off kernels after the last instance has finished.
    static const bool sweep_log = getenv("SQPHIP_SWEEP_LOG") != nullptr;    // instances with work left, per sweep
    static const bool lockstep = getenv("SQPHIP_SWEEP_LOCKSTEP") != nullptr; // experiment switch: read before queueing
    hipEvent_t ev[2];
    for (auto &e : ev) SQPHIP_HIP_OK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    // experiment aid (SQPHIP_HOST_STATS): where the host thread of this group spends its time -- queueing a sweep, or waiting for
    // the counter of the sweep before last; a wait that returns at once means the stream may have run dry behind the host
    static const bool host_stats = getenv("SQPHIP_HOST_STATS") != nullptr;
    double hs_queue = 0.0, hs_wait = 0.0; long hs_sweeps = 0, hs_nowait = 0;
    auto left_after = [&](long k) {          // instances with work left after sweep k
        const auto w0 = std::chrono::steady_clock::now();
        SQPHIP_HIP_OK(hipEventSynchronize(ev[k & 1]));
        if (host_stats) {
            const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - w0).count();
            hs_wait += us; if (us < 5.0) ++hs_nowait;
        }
        SQPHIP_HIP_OK(hipGetLastError());   // a failed launch anywhere in the sweep surfaces here
        const int left = C.h_counters[2 + 2 * (k & 1)];
        // refinement solves pending after sweep k: the next sweep queued serves them -- unless a sweep behind k has been queued
        // with them already (the counter is one sweep late: sweep k + 1 is in the queue): its solve chain serves every instance
        // that waited when sweep k ended, and what asks inside it shows in its own counter
        C.want_resolve = C.h_counters[3 + 2 * (k & 1)] > 0 && C.resolve_served <= k;
        if (C.spec_tail > 0) d.spec_mode = left <= C.spec_tail ? 1 : 0;     // second shift per sweep in the tail of the run (api.hip)
        if (sweep_log) fprintf(stderr, "%d%c", left, (k % 32) == 31 ? '\n' : ' ');
        return left;
    };
    try {
        for (long sweep = 0; sweep < 100000000L; ++sweep) {
            const auto q0 = std::chrono::steady_clock::now();
            int *slot = nullptr;                 // device view of the pinned words this sweep reports into
            SQPHIP_HIP_OK(hipHostGetDevicePointer((void **)&slot, C.h_counters + 2 + 2 * (sweep & 1), 0));
            // (the last kernel of the sweep forms the counts itself where it can -- b_sweep_count, ipm.hip --, k_sqp_count otherwise)
            const bool counted = ipm_sweep(C, /*sqp_level=*/true, C.side_on ? nullptr : slot);
            if (C.side_on && sweep > 0) SQPHIP_HIP_OK(hipStreamWaitEvent(s, C.evS[sweep & 3], 0));     // the side job of this sweep
            if (!counted) hipLaunchKernelGGL(k_sqp_count, dim3(1), dim3(64), 0, s, d, slot);
            if (C.side_on) SQPHIP_HIP_OK(hipEventRecord(C.evC[sweep & 3], s));
            SQPHIP_HIP_OK(hipEventRecord(ev[sweep & 1], s));
            if (host_stats) { hs_queue += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - q0).count(); ++hs_sweeps; }
            if (C.tm.pending_trailing.size() > 4096) C.tm.flush();
            if (lockstep) { if (left_after(sweep) == 0) break; continue; }
            if (sweep >= 1 && left_after(sweep - 1) == 0) break;
        }
        SQPHIP_HIP_OK(hipStreamSynchronize(s));
        if (C.side_on) SQPHIP_HIP_OK(hipStreamSynchronize(C.side));
        if (host_stats && hs_sweeps > 0)
            fprintf(stderr, "sqphip: group of %d: %ld sweeps, host queues a sweep in %.1f us, waits %.1f us per sweep, %ld waits returned at once\n",
                    d.B, hs_sweeps, hs_queue / hs_sweeps, hs_wait / hs_sweeps, hs_nowait);
    } catch (...) {
        for (auto &e : ev) hipEventDestroy(e);
        throw;
    }
    for (auto &e : ev) hipEventDestroy(e);
    if (const char *e = getenv("SQPHIP_EMPTY_SWEEPS")) {      // experiment: wall time of a sweep with every kernel gated off
        const int n = atoi(e);
        C.side_on = false; d.side = 0;       // (the experiment's sweeps run in line)
        const auto t0 = std::chrono::steady_clock::now();
        for (int k = 0; k < n; ++k) ipm_sweep(C, true);
        SQPHIP_HIP_OK(hipStreamSynchronize(s));
        const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
        fprintf(stderr, "sqphip: %d gated-off sweeps of %d instances: %.1f us each\n", n, d.B, us / (n > 0 ? n : 1));
        C.n_sweeps -= n;
    }
}

// SQP-level stages of a sweep, one kernel (b_sqp_stage, sqp_dev.hpp)
__global__ __launch_bounds__(TPB, SQPHIP_VEC_WAVES_PER_EU) void k_sqp_stage(DV d) { b_sqp_stage(d); }

void sqp_stage_kernels(Ctx &C, hipStream_t s, const DV &d)          // called from ipm_sweep
{
    hipLaunchKernelGGL(k_sqp_stage, dim3(d.B), dim3(TPB), 0, s, d);
}

// ---------------------------------------------------------------------------------------------
// Merit / acceptance reductions for the drop-in path: operands are staged in instance 0's vectors
// (x, E, df, lambda, mult_x_U, mult_x_L, pstep, jcoo, hcoo) by the host wrapper.
//   op 0 norm_violations (common.jl:54-77)      op 1 KT_residuals (common.jl:14-23)
//   op 2 norm_complementarity (common.jl:30-47) op 3 compute_phi (sqp.jl:170-183)
//   op 4 compute_qmodel (sqp_trust_region.jl:487-508)  op 5 compute_derivative (merit.jl:15, sqp.jl:203-212)
// The operands are those of instance `inst` (0 for the scalar entry points, inst[k] for request k of the batch forms): one
// body for both kernels, so that a batched result is the scalar one bit for bit.
static __device__ __forceinline__ double merit_body(const DV &d, const int inst, int op, double a0, double a1, int flag)
{
    SQP_PTRS
    double r = 0.0;
    if (op == 0 || op == 2) {
        double acc = 0.0, den = 0.0;
        if (op == 0) {
            for (int i = threadIdx.x; i < d.m; i += TPB) {
                double v = 0.0;
                if (E[i] > gU[i]) v = E[i] - gU[i]; else if (E[i] < gL[i]) v = gL[i] - E[i];
                acc = flag == 1 ? acc + v : (flag == 2 ? acc + v * v : fmax(acc, v));
            }
            for (int j = threadIdx.x; j < d.n; j += TPB) {
                double v = 0.0;
                if (x[j] > xU[j]) v = x[j] - xU[j]; else if (x[j] < xL[j]) v = xL[j] - x[j];
                acc = flag == 1 ? acc + v : (flag == 2 ? acc + v * v : fmax(acc, v));
            }
        } else {
            for (int i = threadIdx.x; i < d.m; i += TPB) {
                double c = 0.0;
                if (gL[i] != gU[i]) { c = fmin(E[i] - gL[i], gU[i] - E[i]) * lam[i]; den += lam[i] * lam[i]; }
                c = fabs(c);
                acc = flag == 1 ? acc + c : (flag == 2 ? acc + c * c : fmax(acc, c));
            }
        }
        acc = flag == 0 ? block_reduce<OpMax>(acc) : block_reduce<OpSum>(acc);
        if (flag == 2) acc = sqrt(acc);
        if (op == 2) { den = block_reduce<OpSum>(den); acc = acc / (1.0 + sqrt(den)); }
        r = acc;
    } else if (op == 1) {
        gather_csc(d, jcoo, hcoo, jv, nullptr);
        __syncthreads();
        r = kt_residuals(d, df, lam, mxU, mxL, jv, 1.0, tmpE);
    } else if (op == 3) {
        const double v = viol1(d, E, gL, gU, x, xL, xU);
        r = flag ? v : a0 + a1 * v;          // a0 = f(x + alpha p), a1 = mu, flag = feasibility restoration
    } else if (op == 4) {
        SqpState tmp = S;
        tmp.mu = a1;
        if (flag) {
            gather_csc(d, jcoo, hcoo, jv, d.nnzh_coo ? hv : nullptr);
            __syncthreads();
            r = qmodel_step(d, inst, tmp, ps, x, df, E, jv, hv, gL, gU, xL, xU, tmpx, tmpE);
        } else {
            r = a1 * viol1(d, E, gL, gU, x, xL, xU);
        }
    } else if (op == 5) {
        double dfp = 0.0, cv = 0.0;
        for (int j = threadIdx.x; j < d.n; j += TPB) dfp += df[j] * ps[j];
        for (int i = threadIdx.x; i < d.m; i += TPB) cv += fmax(0.0, fmax(E[i] - gU[i], gL[i] - E[i]));
        dfp = block_reduce<OpSum>(dfp); cv = block_reduce<OpSum>(cv);
        r = dfp - a1 * cv;
    } else if (op == 6) {
        // compute_derivative(sqp), sqp.jl:190-213 over merit.jl:13-17.  flag bit 0: feasibility restoration (dfp =
        // sum of the slacks staged in oslack), bit 1: vector penalty staged in plam
        const bool fr = flag & 1, vec = flag & 2;
        const double *slack = d.oslack + 2 * om;
        double dfp = 0.0, cv = 0.0;
        if (fr) { for (int k = threadIdx.x; k < 2 * d.m; k += TPB) dfp += slack[k]; }
        else for (int j = threadIdx.x; j < d.n; j += TPB) dfp += df[j] * ps[j];
        for (int i = threadIdx.x; i < d.m; i += TPB) {
            double v = fmax(0.0, fmax(E[i] - gU[i], gL[i] - E[i]));
            if (fr) { const double lhs = E[i] - v; v = fmax(0.0, fmax(lhs - gU[i], gL[i] - lhs)); }
            cv += vec ? plam[i] * v : v;
        }
        dfp = block_reduce<OpSum>(dfp); cv = block_reduce<OpSum>(cv);
        r = vec ? dfp - cv : dfp - a1 * cv;
    } else if (op == 7) {
        // compute_mu_rule1! / 2! / 3! (sqp_line_search.jl:270-294): a0 = rho, flag = rule | (iter == 1) << 4;
        // mu[m] staged in plam (updated in place), lambda in lam
        const int rule = flag & 15, first = flag >> 4;
        double dfp = 0.0, php = 0.0;
        gather_csc(d, jcoo, hcoo, jv, d.nnzh_coo ? hv : nullptr);
        __syncthreads();
        for (int j = threadIdx.x; j < d.n; j += TPB) {
            double hp = 0.0;
            for (int k = d.hcolptr[j]; k < d.hcolptr[j + 1]; ++k) hp += hv[k] * ps[d.hrowval[k]];
            dfp += df[j] * ps[j]; php += 0.5 * ps[j] * hp;
        }
        dfp = block_reduce<OpSum>(dfp); php = block_reduce<OpSum>(php);
        const double v1 = viol1(d, E, gL, gU, x, xL, xU);
        const double t = (dfp + fmax(php, 0.0)) / fmax((1.0 - a0) * v1, 1.0e-8);
        for (int i = threadIdx.x; i < d.m; i += TPB) {
            double mu = plam[i];
            if (rule == 1) { mu = fmax(mu, t); mu = fmax(mu, fabs(lam[i])); }
            else if (rule == 2) mu = first ? t : fmax(mu, fabs(lam[i]));
            else mu = fmax(mu, fabs(lam[i]));
            plam[i] = mu;
        }
        r = t;
    }
    return r;
}

__global__ __launch_bounds__(TPB) void k_merit(DV d, int op, double a0, double a1, int flag, double *out)
{
    const double r = merit_body(d, 0, op, a0, a1, flag);
    if (threadIdx.x == 0) *out = r;
}

// one workgroup per request of a batch call (sqphip_*_batch): instance table, per-request scalars (null: 0), out[count]
__global__ __launch_bounds__(TPB) void k_merit_batch(DV d, const int *inst, int op, const double *a0, const double *a1, int flag,
                                                     double *out)
{
    const int k = blockIdx.x;
    const double r = merit_body(d, inst[k], op, a0 ? a0[k] : 0.0, a1 ? a1[k] : 0.0, flag);
    if (threadIdx.x == 0) out[k] = r;
}

// compute_alpha (sqp_line_search.jl:303-334) on the device: x and p of instance `inst` are staged in d.x / d.pstep;
// out[0] = alpha, out[1] = is_valid, out[2] = merit evaluations.  One workgroup; the merit function is
// compute_phi (sqp.jl:170-183) over the device callbacks, its norms reduced by wave butterflies + an LDS exchange.
// (One body, three instantiations by evaluator: k_armijo<ARMIJO_DEDICATED> sits at the VGPR cap -- with the QCQP branch of
// acopf_eval inlined it spilled more --, so it evaluates through the dedicated dispatch, and k_armijo<ARMIJO_QCQP> /
// k_armijo<ARMIJO_NLP> serve QCQP (sqphip_qcqp_attach) and factorable-NLP (sqphip_nlp_attach) contexts)
enum { ARMIJO_DEDICATED = 0, ARMIJO_QCQP = 1, ARMIJO_NLP = 2 };
template <int KIND>
__global__ __launch_bounds__(TPB) void k_armijo(DV d, int inst, double mu, double phi0, double D, double eta, double tau,
                                                double min_alpha, int fr, double *out)
{
    SQP_PTRS
    const double pn = norm_inf(ps, d.n);
    double alpha = 1.0;
    int valid = 1, nev = 0;
    if (!(pn <= d.tol_direction)) {
        __shared__ double fsh;
        for (;;) {
            for (int j = threadIdx.x; j < d.n; j += TPB) tmpx[j] = x[j] + alpha * ps[j];
            __syncthreads();
            if constexpr (KIND == ARMIJO_NLP) nlp_eval(d, inst, tmpx, 1.0, nullptr, &fsh, nullptr, tmpE, nullptr, nullptr);
            else if constexpr (KIND == ARMIJO_QCQP) qcqp_eval(d, inst, tmpx, 1.0, nullptr, &fsh, nullptr, tmpE, nullptr, nullptr);
            else acopf_eval_dedicated(d, inst, tmpx, 1.0, nullptr, &fsh, nullptr, tmpE, nullptr, nullptr);
            __syncthreads();
            const double v = viol1(d, tmpE, gL, gU, tmpx, xL, xU);
            const double phi = fr ? v : fsh + mu * v;
            ++nev;
            if (!(phi > phi0 + eta * alpha * D)) break;
            if (alpha < min_alpha) { valid = 0; break; }     // the step size can become too small
            alpha *= tau;
            __syncthreads();
        }
    }
    if (threadIdx.x == 0) { out[0] = alpha; out[1] = valid; out[2] = nev; }
}

void armijo_eval(Ctx &C, int inst, double mu, double phi0, double D, double eta, double tau, double min_alpha, int fr,
                 double *out3_host)
{
    double *o = C.d.wN + (size_t)inst * C.d.Npad;     // scratch slots
    hipLaunchKernelGGL(C.d.nlp ? k_armijo<ARMIJO_NLP> : C.d.qc ? k_armijo<ARMIJO_QCQP> : k_armijo<ARMIJO_DEDICATED>, dim3(1), dim3(TPB), 0, C.stream, C.d, inst, mu, phi0, D, eta, tau,
                       min_alpha, fr, o);
    SQPHIP_HIP_OK(hipMemcpyAsync(out3_host, o, 3 * sizeof(double), hipMemcpyDeviceToHost, C.stream));
    SQPHIP_HIP_OK(hipStreamSynchronize(C.stream));
}

void merit_eval(Ctx &C, int op, double a0, double a1, int flag, double *out_host)
{
    double *o = C.d.wN;     // scratch scalar slot
    hipLaunchKernelGGL(k_merit, dim3(1), dim3(TPB), 0, C.stream, C.d, op, a0, a1, flag, o);
    SQPHIP_HIP_OK(hipMemcpyAsync(out_host, o, sizeof(double), hipMemcpyDeviceToHost, C.stream));
    SQPHIP_HIP_OK(hipStreamSynchronize(C.stream));
}

void merit_eval_batch(Ctx &C, int count, const int *inst_dev, int op, const double *a0_dev, const double *a1_dev, int flag,
                      double *out_dev)
{
    hipLaunchKernelGGL(k_merit_batch, dim3(count), dim3(TPB), 0, C.stream, C.d, inst_dev, op, a0_dev, a1_dev, flag, out_dev);
}

}  // namespace sqphip
