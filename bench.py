#!/usr/bin/env python3
"""Headline benchmark: QP sub-problems per second of the batched SQP-TR hot path on MI355X.

    python bench.py --gpus N --steps K --warmup W          (N > 1 without a launcher: the parent, which never touches a GPU,
                                                            starts N rank processes itself and relays rank 0's line)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \\
           bench.py --gpus N --steps K --warmup W          (one rank per GPU; --gpus must equal WORLD_SIZE)

One "step" = one SQP-TR outer iteration of every instance of the job: device ACOPF evaluation, the trust-region QP
(or feasibility-restoration / second-order-correction) sub-problem solved by the on-device interior-point method,
merit + ratio test.  Workload: BASELINE.json configs[3] -- 512 IEEE-118-shaped ACOPF contingency scenarios, ALL of
them on one GPU at N = 1 and 512 / N per rank at N > 1 (strong scaling; --scaling weak: 512 per GPU, N x 512 in the job);
Newton matrix of order 2813 condensed to 2069,
factorised by the multifrontal path (options.kkt_mode = 0 picks it), fp64, synthetic data of that shape, SQP options
of /root/reference/examples/acopf/opf.jl:76-79.  Inputs are resident in HBM before the timed region.  Ranks never
exchange iterates; the timed region ends with one all-gather of (ret, iter, done) per instance over RCCL
(sqphip_gather_status).  Prints ONE JSON line on rank 0.

Besides the contract's fields every line carries (rank 0, from the counters and HIP events of the timed steps):
  roofline       the multifrontal factor + solve kernels against the HBM roof (B_sparse)
A plain run stops there.  With --full it also runs, outside the timed region, the records that take runs of their own:
  kernels        per-kernel-class records over three more outer iterations; roofline.onbox_mfma_probe_tflops
  dense_ldlt     the dense MFMA LDL^T of round 1 on its own (N = 2813, 64 instances): ms and TFLOP/s of N^3/3 vs 78.6
  scaling_prediction   the same timed steps over 1/2, 1/4 and 1/8 of the scenarios
  termination    the same 512 scenarios run until every instance has terminated (at most 60 outer iterations), with
                 the reference's Hessian sign (literal_quirks = 1: the sub-problems are non-convex and most runs hit
                 the limit) and with the textbook sign (literal_quirks = 0: nearly all converge)
  screening      the scenario queue run to termination
  cpu_baseline   the CPU restatement (oracle/, its own sparse LDL^T), instances spread over the host cores
(--quick and the --no-* switches drop legs of --full.)

--dump-outputs DIR writes, after the timed steps, what a caller of the timed path receives after its last step, as
float64 .npy files (rank 0's block at N > 1): per instance the iterate x, the constraint values g, the multipliers
mult_g / mult_x_L / mult_x_U, obj_val, status and iter (sqphip_sqp_get), with the global scenario id in `instance`;
and the gathered (ret, iter, done) table of the whole job.  Past 56 MB the instances are a fixed, seeded sample.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

_ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, _ROOT)

FP64_MFMA_PEAK_TFLOPS = 78.6   # MI355X datasheet fp64 matrix peak; MI355X_MICROARCH.md has no fp64 row.  The on-box
                               # register-resident MFMA probe (printed next to it) sustains 77.6 of it.
HBM_PEAK_GBS = 8000.0          # MI355X_MICROARCH.md: HBM3E ~ 8 TB/s
DEFAULT_BATCH = {"case14": 512, "case118": 512, "case1354": 512, "case9241": 256, "dense": 64}    # (9241: 40 GB of fronts; 128 leave half of the CUs without a vector stage)


def host_cores():
    try:
        return max(1, min(16, len(os.sched_getaffinity(0))))   # the GPU box grants 16 host cores per GPU
    except AttributeError:
        return max(1, min(16, os.cpu_count() or 1))


def self_launch(n):
    """Start n rank processes of this script (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT as
    torch.distributed.run sets them), let their stdout / stderr through, return the largest exit code."""
    import socket
    import subprocess
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env))
    rc = 0
    try:
        for p in procs:
            rc = max(rc, abs(p.wait()))
    except KeyboardInterrupt:
        for p in procs:
            p.terminate()
        rc = 130
    if rc != 0:                    # a rank that died leaves the others waiting in a collective: end exactly the processes started here
        for p in procs:
            if p.poll() is None:
                p.terminate()
    return rc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=None)
    ap.add_argument("--workload", default="case118", choices=["case14", "case118", "case1354", "case9241", "dense"],
                    help="case*: ACOPF shapes of BASELINE.json; dense: a synthetic NLP with a dense Lagrangian Hessian (n = 2688, 128 linear rows: Newton matrices of order 2816 = 44 tiles; "
                         "sqpsolver.jl_amd/dense_synth.py) through the dense MFMA LDL^T (kkt_mode 1 unless given): 64 scenarios, --steps 4 --warmup 1 unless given")
    ap.add_argument("--formulation", default="polar", choices=["polar", "acr", "acwr"],
                    help="ACOPF evaluator: polar (ACP, default), rectangular (ACR, the one examples/acopf/opf.jl:46 runs) "
                         "or the W-space model of examples/acopf/acwr.jl")
    ap.add_argument("--topology", default=None, choices=["chain", "geo"],
                    help="synthetic network recipe: chain = SURVEY.md section 8d (default for case14 / case118), geo = lattice strip "
                         "with local generation (default for case1354 / case9241: the chain recipe gives no convergent NLP there)")
    ap.add_argument("--dense-n", type=int, default=2688, help="--workload dense: variables (the Newton matrix has order n + 128)")
    ap.add_argument("--batch", type=int, default=None, help="instances of the whole job (default 512 for case118); with --scaling weak: per GPU")
    ap.add_argument("--scaling", default="strong", choices=["strong", "weak"],
                    help="strong (default, BASELINE configs[3]): the job's scenarios are split over the GPUs; weak: every GPU "
                         "holds --batch scenarios (ids rank * batch ...), the job grows with N")
    ap.add_argument("--full", action="store_true",
                    help="also run the records that take runs of their own (kernels, dense_ldlt, scaling_prediction, termination, "
                         "screening, cpu_baseline, the MFMA probe); a plain run times the steps and prints the headline line only")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps, write what the timed path computed in its last step as DIR/<name>.npy (float64)")
    ap.add_argument("--quick", action="store_true", help="with --full: timed steps only (implies --no-cpu-baseline --no-termination --no-dense-ldlt --no-screening)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-termination", action="store_true", help="skip the run-to-termination legs")
    ap.add_argument("--no-dense-ldlt", action="store_true", help="skip the dense LDL^T record")
    ap.add_argument("--no-screening", action="store_true", help="skip the scenario-queue record")
    ap.add_argument("--no-batch-curve", action="store_true", help="skip the 64 / 128 / 256-scenario runs behind `scaling_prediction`")
    ap.add_argument("--screening-factor", type=int, default=4, help="scenario-queue record: scenarios = factor x slots")
    ap.add_argument("--literal-quirks", type=int, default=1)
    ap.add_argument("--kkt-mode", type=int, default=None, help="options.kkt_mode: 0 auto (sparse for the ACOPF shapes; default), 1 dense MFMA (default for --workload dense), 2 sparse")
    ap.add_argument("--kkt-tile-order", type=int, default=None)
    ap.add_argument("--kkt-condense", type=int, default=None)
    ap.add_argument("--ipm-corrector", type=int, default=0, help="0 (default): monotone barrier rule, Ipopt's default; 1: Mehrotra predictor-corrector")
    ap.add_argument("--no-kernel-timing", action="store_true", help="skip the HIP-event timing of the factor / solve kernels")
    ap.add_argument("--sqp-options", default="example", choices=["example", "defaults"],
                    help="example: tol_infeas 1e-6, tol_residual 1e-4, use_soc (examples/acopf/opf.jl:76-79, the headline); "
                         "defaults: the reference's Parameters defaults (parameters.jl:17-29: tol_direction = tol_residual = tol_infeas = 1e-8, no SOC)")
    ap.add_argument("--backend", default="nccl", choices=["nccl", "gloo"],
                    help="torch.distributed backend for N > 1 (nccl = RCCL; gloo only to rehearse the multi-rank flow "
                         "on a box with fewer GPUs than ranks, together with --one-device)")
    ap.add_argument("--one-device", action="store_true", help="rehearsal: every rank uses cuda:0")
    ap.add_argument("--shared-queue", type=int, default=0, metavar="M",
                    help="instead of the timed steps: M scenarios through a queue shared between the ranks (every rank holds all "
                         "tables, --batch slots per rank, --queue-split of the ids start on rank 0; run to termination, "
                         "literal_quirks as given); prints one JSON line, --dump-status gets the per-scenario results")
    ap.add_argument("--queue-split", type=float, default=None, help="fraction of the M ids assigned to rank 0 at the start (default: even)")
    ap.add_argument("--dump-status", default=None, help="rank 0 writes the gathered (ret, iter, done) table to this JSON file")
    args = ap.parse_args()
    dense_wl = args.workload == "dense"
    if args.steps is None: args.steps = 4 if dense_wl else 6          # (the dense NLP converges in six or seven outer iterations)
    if args.warmup is None: args.warmup = 1
    if args.kkt_mode is None: args.kkt_mode = 1 if dense_wl else 0
    if args.steps < 1:
        ap.error("--steps must be at least 1 (sqphip_sqp_run(0) would run to termination)")
    if args.quick or not args.full:
        args.no_cpu_baseline = args.no_termination = args.no_dense_ldlt = args.no_screening = args.no_batch_curve = True

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        # Typed without a launcher: this process -- which has made no GPU call and imported no GPU library -- starts one fresh
        # rank process per GPU (the environment torch.distributed.run would give them), relays their output and leaves with
        # their worst exit code.  Never an exec of a process that touched the GPU.
        sys.exit(self_launch(args.gpus))
    if world != args.gpus:
        if rank == 0:
            print(f"[bench] --gpus {args.gpus} but WORLD_SIZE is {world}: launch N > 1 as\n"
                  f"  python bench.py --gpus {args.gpus} ...   (starts the ranks itself), or\n"
                  f"  python -m torch.distributed.run --nnodes=1 --nproc-per-node {args.gpus} --master-addr 127.0.0.1 "
                  f"--master-port 29500 bench.py --gpus {args.gpus} ...", file=sys.stderr)
        sys.exit(2)

    if os.environ.get("SQPHIP_BENCH_RANK_ECHO"):      # test aid (tests/test_abi.py): what a rank process was started with; no GPU touched
        print(json.dumps({"rank": rank, "world": world, "local_rank": local_rank, "master": os.environ.get("MASTER_ADDR"),
                          "port": os.environ.get("MASTER_PORT")}), flush=True)
        return

    import numpy as np
    import torch
    import torch.distributed as dist

    if args.one_device:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    if world > 1:
        if args.backend == "nccl":
            dist.init_process_group(backend="nccl", device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(backend="gloo")
    dev = torch.device("cuda", local_rank) if args.backend == "nccl" else torch.device("cpu")   # collective buffers

    import sqpsolver_jl_amd as pkg
    from sqpsolver_jl_amd.acopf_synth import synth_case, acopf_layout, acr_layout, acwr_layout, contingency, CASES
    if args.formulation != "polar":
        acopf_layout = {"acr": acr_layout, "acwr": acwr_layout}[args.formulation]
    from sqpsolver_jl_amd.shard import shard_range, gather_status
    from sqpsolver_jl_amd import _lib

    nb, ng, nl, seed = CASES[args.workload] if not dense_wl else (0, 0, 0, 7)
    total = args.batch or DEFAULT_BATCH[args.workload]
    if args.scaling == "weak":          # every GPU holds --batch scenarios: rank r solves the ids r * batch .. (r + 1) * batch - 1
        per = total
        total = per * world
        lo, hi = rank * per, (rank + 1) * per
    else:
        lo, hi = shard_range(total, world, rank)
    B = hi - lo
    if dense_wl:
        from sqpsolver_jl_amd.dense_synth import dense_synth, dense_scenario, dense_layout
        base = dense_synth(args.dense_n, 128, seed)
        topology = "dense"
        lay0 = dense_layout(base)
    else:
        base = synth_case(args.workload, args.topology)
        topology = args.topology or ("chain" if nb <= 118 else "geo")
        lay0 = acopf_layout(base)
    use_soc = 1 if args.sqp_options == "example" else 0
    sqp_kw = dict(tol_infeas=1e-6, tol_residual=1e-4, use_soc=1) if use_soc else {}
    lin_kw = {"kkt_mode": args.kkt_mode}
    if args.kkt_condense is not None:
        lin_kw["kkt_condense"] = args.kkt_condense
    if args.kkt_tile_order is not None:
        lin_kw["kkt_tile_order"] = args.kkt_tile_order

    scen = {}

    def scenario(s_id):
        if s_id not in scen:
            if dense_wl:
                net = dense_scenario(base, s_id)
                scen[s_id] = (net, dense_layout(net))
            else:
                net = base if s_id == 0 else contingency(base, s_id, seed)
                scen[s_id] = (net, acopf_layout(net))
        return scen[s_id]

    def make_ctx(literal_quirks, max_iter=3000, first=None, corrector=None):
        """context over this rank's block of scenarios, or (first = k) over the scenarios 0..k-1"""
        ids = range(lo, hi) if first is None else range(first)
        opts = pkg.default_options(max_iter=max_iter, literal_quirks=literal_quirks, device=local_rank,
                                   ipm_corrector=args.ipm_corrector if corrector is None else corrector, **lin_kw, **sqp_kw)
        ctx = pkg.Context(lay0.n, lay0.m, lay0.num_linear, lay0.jrow, lay0.jcol, lay0.hrow, lay0.hcol,
                          lay0.xL, lay0.xU, lay0.gL, lay0.gU, opts, batch=len(ids))
        if dense_wl:
            ctx.dense_attach(base)
            for b, s_id in enumerate(ids):
                ctx.dense_set_instance(b, *scenario(s_id))
        else:
            ctx.acopf_attach(base, lay0)
            for b, s_id in enumerate(ids):
                ctx.acopf_set_instance(b, *scenario(s_id))
        ctx.sqp_reset()
        return ctx, opts

    def sync():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    if args.shared_queue > 0:
        # ---- a screening job over a queue shared between the ranks (no timed steps, no roofline: a functional mode)
        from sqpsolver_jl_amd.shard import run_shared_queue
        M, slots = args.shared_queue, (args.batch or 8)
        qopts = pkg.default_options(max_iter=60, literal_quirks=args.literal_quirks, device=local_rank,
                                    ipm_corrector=args.ipm_corrector, **lin_kw, **sqp_kw)
        qctx = pkg.Context(lay0.n, lay0.m, lay0.num_linear, lay0.jrow, lay0.jcol, lay0.hrow, lay0.hcol,
                           lay0.xL, lay0.xU, lay0.gL, lay0.gU, qopts, batch=slots)
        qctx.acopf_attach(base, lay0)
        qctx.stream_begin(M)
        for s_id in range(M):
            qctx.stream_set(s_id, *scenario(s_id))
        if world == 1:
            mine = list(range(M))
        else:
            cut0 = int(round(M * args.queue_split)) if args.queue_split is not None else shard_range(M, world, 0)[1]
            rest = [cut0 + shard_range(M - cut0, world - 1, r)[0] for r in range(world - 1)] + [M]
            mine = list(range(0, cut0)) if rank == 0 else list(range(rest[rank - 1], rest[rank]))
        qctx.stream_assign(mine)
        sync()
        ta = time.perf_counter()
        rounds = run_shared_queue(qctx, rank, world, slots, chunk=5)
        sync()
        tb = time.perf_counter()
        # every scenario was solved by exactly one rank: merge the per-scenario tables (the unsolved entries are -99)
        qc = qctx.counters()
        st = np.full(M, -99, dtype=np.int64); it = np.zeros(M, dtype=np.int64); obj = np.zeros(M)
        solved_here = 0
        for s_id in range(M):
            r_ = qctx.stream_get(s_id)
            if r_["iter"] >= 0:          # (-1: not filed by this rank since the ids were assigned, sqphip.h)
                st[s_id], it[s_id], obj[s_id] = r_["status"], r_["iter"], r_["obj_val"]; solved_here += 1
        tabs = [(st, it, obj, solved_here, int(qc["n_qp"]))]
        if world > 1:
            tabs = [None] * world
            dist.all_gather_object(tabs, (st, it, obj, solved_here, int(qc["n_qp"])))
        if rank == 0:
            owner = np.full(M, -1)
            for r_, (s_, i_, o_, _, _) in enumerate(tabs):
                sel = s_ != -99
                assert not np.any(owner[sel] >= 0), "a scenario was solved twice"
                owner[sel] = r_; st[sel] = s_[sel]; it[sel] = i_[sel]; obj[sel] = o_[sel]
            assert np.all(owner >= 0), "a scenario was not solved"
            if args.dump_status:
                with open(args.dump_status, "w") as fh:
                    json.dump({"status": st.tolist(), "iter": it.tolist(), "obj_hex": [float(v).hex() for v in obj]}, fh)
            print(json.dumps({"mode": "shared_queue", "scenarios": M, "n_gpus": world, "slots_per_rank": slots, "rounds": rounds,
                              "seconds": tb - ta, "scenarios_per_s": M / (tb - ta), "initial_ids_by_rank": [len(mine)] if world == 1 else None,
                              "solved_by_rank": [t[3] for t in tabs], "qp_by_rank": [t[4] for t in tabs],
                              "converged": int(np.sum(st == 0))}))
        qctx.close()
        if world > 1:
            dist.destroy_process_group()
        return

    ctx, opts = make_ctx(args.literal_quirks)

    # the status gather: RCCL inside the library (sqphip_gather_status); torch.distributed only carries the unique id
    use_lib_comm = False
    if world > 1 and args.backend == "nccl" and not args.one_device:
        # sqphip_comm_init is collective: agree that every rank can load RCCL before any rank enters it
        can = torch.tensor([1 if pkg.Context.comm_available() else 0], dtype=torch.int32, device=dev)
        dist.all_reduce(can, op=dist.ReduceOp.MIN)
        if not bool(can.item()):
            print(f"[bench] rank {rank}: RCCL not loadable on every rank; status gather through torch.distributed", file=sys.stderr)
    if world > 1 and args.backend == "nccl" and not args.one_device and bool(can.item()):
        try:
            idt = torch.zeros(128, dtype=torch.uint8, device=dev)
            if rank == 0:
                idt.copy_(torch.frombuffer(bytearray(pkg.Context.comm_unique_id()), dtype=torch.uint8))
            dist.broadcast(idt, src=0)
            ctx.comm_init(bytes(idt.cpu().numpy().tobytes()), world, rank)
            use_lib_comm = True
        except Exception as e:          # never lose the measurement to the gather: fall back to torch.distributed
            print(f"[bench] rank {rank}: sqphip_comm_init failed ({e}); status gather through torch.distributed", file=sys.stderr)
        ok = torch.tensor([1 if use_lib_comm else 0], dtype=torch.int32, device=dev)
        dist.all_reduce(ok, op=dist.ReduceOp.MIN)
        use_lib_comm = bool(ok.item())

    def sync():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    def run_steps(k):
        """k outer SQP-TR iterations of every instance of the block (continuous batching inside the library: an
        instance never waits for the slowest sub-problem of the batch), then the status all-gather across ranks."""
        ctx.sqp_run(k)
        if use_lib_comm:
            return ctx.gather_status(total)
        return gather_status(*ctx.sqp_status(), total, device=dev)

    if args.warmup > 0:
        run_steps(args.warmup)
    c0 = ctx.counters()
    m0 = ctx.mode_counters()
    w0 = ctx.sqp_work()[2].copy()
    ctx.set_timing(not args.no_kernel_timing)
    sync()
    t0 = time.perf_counter()
    g_ret, g_it, g_done = run_steps(args.steps)
    sync()
    t1 = time.perf_counter()
    ctx.set_timing(False)
    c1 = ctx.counters()
    m1 = ctx.mode_counters()
    term_rules = ctx.termination_counters()      # sub-problems since the reset by the way their interior-point run ended
    wfac = ctx.sqp_work()[2] - w0            # factorisations per instance over the timed steps (= sweeps it was active in)
    # rank-local table of the timed steps by sub-problem mode (sub-problems, IPM iterations and factorisations per solve)
    by_mode = {}
    for k in m1:
        q, i, f = (m1[k][j] - m0[k][j] for j in range(3))
        if q > 0:
            by_mode[k] = {"solved": int(q), "ipm_iterations_per_solve": i / q, "factorisations_per_solve": f / q,
                          "share_of_factorisations": f / max(1, c1["n_factor"] - c0["n_factor"])}

    elapsed = torch.tensor([t1 - t0], dtype=torch.float64, device=dev)
    stats = torch.tensor([c1["n_qp"] - c0["n_qp"], c1["n_ipm_iter"] - c0["n_ipm_iter"],
                          c1["n_factor"] - c0["n_factor"]], dtype=torch.float64, device=dev)
    if world > 1:
        dist.all_reduce(elapsed, op=dist.ReduceOp.MAX)
        dist.all_reduce(stats, op=dist.ReduceOp.SUM)
    elapsed = float(elapsed.item())
    n_qp, n_ipm, n_fac = (float(v) for v in stats.tolist())

    # ---- what the timed path computed in its last step (before any record below runs the context further)
    if rank == 0 and args.dump_outputs:
        os.makedirs(args.dump_outputs, exist_ok=True)
        per_instance = 8 * (3 * lay0.n + 2 * lay0.m)
        k = min(B, max(1, (56 << 20) // per_instance))
        ids = np.arange(B) if k == B else np.sort(np.random.default_rng(0).choice(B, k, replace=False))
        rows = [ctx.sqp_get(int(b)) for b in ids]
        dump = {"instance": lo + ids}
        for key in ("x", "g", "mult_g", "mult_x_L", "mult_x_U"):
            dump[key] = np.stack([r[key] for r in rows])
        for key in ("obj_val", "status", "iter"):
            dump[key] = np.array([r[key] for r in rows])
        dump.update(gathered_ret=g_ret, gathered_iter=g_it, gathered_done=g_done)
        for key, a in dump.items():
            np.save(os.path.join(args.dump_outputs, key + ".npy"), np.asarray(a, dtype=np.float64))

    # ---- roofline of the dominant kernels, rank-0 local measurement (HIP events on the library's stream)
    N_full = lay0.n + lay0.m
    N = int(c1["kkt_order"])
    loc_fac = c1["n_factor"] - c0["n_factor"]
    fac_sec = c1["ldlt_seconds"] - c0["ldlt_seconds"]
    sol_sec = c1["solve_seconds"] - c0["solve_seconds"]
    probe = None
    if rank == 0 and args.full:
        import ctypes as C
        v = C.c_double()
        if _lib.lib().sqphip_mfma_f64_peak(local_rank, C.byref(v)) == 0:
            probe = v.value
    if c1["sparse"]:
        # B_sparse = 12 nnz(K_lower) [values + indices read] + 8 nnz(L) [written] + 2 x 8 nnz(L)
        # [forward + backward reads] + 4 x 8 N [vectors] per factorisation with its solve, per instance.  The
        # refinement / corrector solves of an iteration add time but no bytes here: the fraction is a lower bound.
        b_sparse = 12.0 * c1["nnz_k"] + 24.0 * c1["nnz_l"] + 32.0 * N
        # the library runs the batch as n_groups instance groups on concurrent streams; the HIP events of a group time its
        # own stream (other groups' kernels share the chip meanwhile), so the seconds summed over the groups count the
        # same wall time n_groups times: the family's time is their average per stream
        n_groups = max(1, int(c1["n_groups"]))
        fac_sec /= n_groups; sol_sec /= n_groups
        ksec = fac_sec + sol_sec
        achieved = loc_fac * b_sparse / ksec / 1e9 if ksec > 0 else 0.0
        # the same with every solve counted (corrector and refinement solves read L again: 16 nnz(L) + 16 N each)
        loc_sol = c1["n_solve"] - c0["n_solve"]
        b_all = loc_fac * (12.0 * c1["nnz_k"] + 8.0 * c1["nnz_l"] + 16.0 * N) + loc_sol * (16.0 * c1["nnz_l"] + 16.0 * N)
        # HBM bytes per instance-factorisation from the PMC passes (profiles/mf_traffic_<workload>.json, written by
        # scripts/make_traffic_profile.py from rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE runs of THIS workload and build);
        # null when none was collected for this workload -- never another workload's constant
        traffic, traffic_src = None, None
        tpath = os.path.join(_ROOT, "profiles", f"mf_traffic_{args.workload}.json")
        if os.path.exists(tpath) and args.formulation == "polar" and args.kkt_mode in (0, 2):
            try:
                tj = json.load(open(tpath))
                if int(tj.get("nnz_l", -1)) == int(c1["nnz_l"]):          # same plan as the one measured
                    traffic = tj.get("hbm_bytes_per_instance_factorisation")
                    traffic_src = os.path.relpath(tpath, _ROOT)
            except Exception:
                traffic = None
        roofline = {"bound": "hbm", "kernel": "k_mf_values + k_mf_front<*> / k_mf_factor2<*> (factor, v_mfma_f64_16x16x4_f64 rank-4 blocks) + "
                                              "k_mf_fwd2 / k_mf_bwd2 / k_mf_solve_top2 (solves; k_mf_fwd / k_mf_bwd / k_mf_solve_top where a front "
                                              "exceeds the LDS-staged kernels)",
                    "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS,
                    "traffic": traffic, "traffic_static": True, "traffic_source": traffic_src,
                    "bytes_per_instance_factorisation": b_sparse, "nnz_k_lower": int(c1["nnz_k"]), "nnz_l": int(c1["nnz_l"]),
                    "instance_factorisations": int(loc_fac), "instance_solves": int(loc_sol),
                    "achieved_counting_all_solves": b_all / ksec / 1e9 if ksec > 0 else 0.0,
                    "factor_seconds": fac_sec, "solve_seconds": sol_sec,
                    "share_of_wall": ksec / (t1 - t0) if t1 > t0 else None,
                    "whole_factor_mfma_frac": (loc_fac * c1["factor_flops"] / fac_sec / 1e12 / FP64_MFMA_PEAK_TFLOPS) if fac_sec > 0 else None,
                    "instance_groups": n_groups,
                    "supernodes": int(c1["n_supernodes"]), "levels": int(c1["n_levels"]), "max_front": int(c1["max_front"]),
                    "onbox_mfma_probe_tflops": probe}
    else:
        tr_sec = c1["trailing_seconds"] - c0["trailing_seconds"]
        tr_launch = c1["trailing_launches"] - c0["trailing_launches"]
        achieved = loc_fac * float(c1["trailing_flops_per_factor"]) / tr_sec / 1e12 if tr_sec > 0 else 0.0
        roofline = {"bound": "mfma", "kernel": "k_trailing + k_trailing_list (v_mfma_f64_16x16x4_f64)",
                    "achieved": achieved, "peak": FP64_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
                    "frac": achieved / FP64_MFMA_PEAK_TFLOPS, "traffic": None,
                    "launches": int(tr_launch), "avg_launch_ms": 1e3 * tr_sec / tr_launch if tr_launch else None,
                    "share_of_wall": tr_sec / (t1 - t0) if t1 > t0 else None,
                    "onbox_mfma_probe_tflops": probe}
    # ---- per-kernel records (rank 0, sparse path): three more outer iterations with an event pair around every launch group
    # of a sweep by kernel class (sqphip_set_timing(ctx, 2) -- outside the timed region: about twenty event records per
    # sweep).  achieved = ALGORITHMIC bytes of what the class touches x the units it processed / its time on the stream
    # (averaged over the instance groups, which overlap), against the HBM peak; DESIGN.md section 6 has the byte counts.
    kernels = None
    if rank == 0 and args.full and c1["sparse"] and not args.no_kernel_timing:
        try:
            kt0, cc0 = ctx.kernel_times(), ctx.counters()
            ctx.set_timing(2)
            ctx.sqp_run(3)
            torch.cuda.synchronize()
            ctx.set_timing(False)
            kt1, cc1 = ctx.kernel_times(), ctx.counters()
            dfac, dsol, dit = (cc1[k] - cc0[k] for k in ("n_factor", "n_solve", "n_ipm_iter"))
            ng_ = max(1, int(cc1["n_groups"]))
            nK, nL, nKt, nLt, ct = (int(cc1[k]) for k in ("nnz_k", "nnz_l", "nnz_k_top", "nnz_l_top", "cols_top"))
            nj, nh = len(lay0.jrow), 2 * len(lay0.hrow)
            dres = max(0, dsol - dit)                      # refinement / corrector solves: forward + backward
            no_top = nLt == 0 or kt1["solve_top"][1] == kt0["solve_top"][1]     # no streamed top in this plan: its fronts are level launches of the solves
            sLt, sct = (0, 0) if no_top else (nLt, ct)
            per_unit = {
                "values": ("k_mf_values", "instance-factorisation", dfac, 20.0 * nK, "12 B read (value + index) + 8 B written per structural entry"),
                "fronts_low": ("k_mf_factor2<*> / k_mf_front<*> below the narrow top of the tree", "instance-factorisation", dfac,
                               8.0 * (nL - nLt) + 8.0 * (nK - nKt), "8 B per entry of L written + 8 B per assembled value read"),
                "fronts_top": ("k_mf_front<*> of the narrow top (17 fronts of IEEE-118)", "instance-factorisation", dfac,
                               8.0 * nLt + 8.0 * nKt, "8 B per entry of L written + 8 B per assembled value read"),
                "solve_top": ("k_mf_solve_top2 (with the inertia test)", "instance-solve", dit + dres,
                              (dit * (8.0 * nLt + 16.0 * ct) + dres * (16.0 * nLt + 16.0 * ct)) / max(1, dit + dres),
                              "backward pass: 8 B per entry of L of the top + 16 B per column; forward + backward: twice the L"),
                "solve_levels": ("k_mf_fwd2 / k_mf_bwd2", "instance-solve", dit + dres,
                                 (dit * (8.0 * (nL - sLt) + 16.0 * (N - sct)) + dres * (16.0 * (nL - sLt) + 16.0 * (N - sct))) / max(1, dit + dres),
                                 "as solve_top, the fronts below the top"),
                "post": ("k_ipm_post (residual check, step, convergence test, next right-hand side)", "instance-iteration", dit,
                         8.0 * (36 * lay0.n + 52 * lay0.m) + 12.0 * (2 * nh + 6 * nj),
                         "36 vector passes over n + 52 over m (8 B each) + 2 Hessian and 6 Jacobian products (12 B per entry)"),
            }
            kernels = {}
            if no_top:
                per_unit.pop("solve_top", None)
            for cls, (name, unit, units, bpu, what) in per_unit.items():
                sec, grp = kt1[cls][0] - kt0[cls][0], kt1[cls][1] - kt0[cls][1]
                if sec <= 0 or grp <= 0:
                    continue
                ach = units * bpu / (sec / ng_) / 1e9
                kernels[cls] = {"kernel": name, "unit": unit, "units": int(units), "algorithmic_bytes_per_unit": bpu, "bytes": what,
                                "launch_groups": int(grp), "avg_us_per_launch_group": 1e6 * sec / grp,
                                "achieved": ach, "peak": HBM_PEAK_GBS, "frac": ach / HBM_PEAK_GBS, "bound": "hbm"}
            tr = kt1["transitions"][0] - kt0["transitions"][0]
            if tr > 0:
                kernels["transitions"] = {"kernel": "k_qp_finish + k_sqp_stage + k_ipm_head", "launch_groups": int(kt1["transitions"][1] - kt0["transitions"][1]),
                                          "avg_us_per_launch_group": 1e6 * tr / max(1, kt1["transitions"][1] - kt0["transitions"][1])}
            tot = sum(kt1[k][0] - kt0[k][0] for k in kt1)
            for cls in kernels:
                kernels[cls]["share_of_timed_kernel_seconds"] = (kt1[cls][0] - kt0[cls][0]) / tot if tot > 0 else None
        except Exception as e:
            print(f"[bench] optional record 'kernels' failed: {e!r}", file=sys.stderr)
            kernels = {"error": repr(e)}
    ctx.close()

    # ---- rank 0, single-GPU only: the dense MFMA LDL^T on its own, the run-to-termination legs, the CPU baseline
    dense = None
    small = args.workload in ("case14", "case118")      # the extra legs belong to the headline workload
    if rank == 0 and not args.no_dense_ldlt and small:
        try:
            import ctypes as C
            sec, trs, nl_ = C.c_double(), C.c_double(), C.c_int64()
            if _lib.lib().sqphip_ldlt_bench(local_rank, 64, 2813, 3, C.byref(sec), C.byref(trs), C.byref(nl_)) == 0 and sec.value > 0:
                tf = 64 * 2813.0 ** 3 / 3.0 / sec.value / 1e12
                dense = {"what": "batched dense LDL^T (ldlt.hip), 64 matrices of order 2813 (IEEE-118 full Newton matrix)",
                         "ms_per_batch": 1e3 * sec.value, "tflops_n3_over_3": tf, "peak": FP64_MFMA_PEAK_TFLOPS,
                         "frac": tf / FP64_MFMA_PEAK_TFLOPS, "k_trailing_ms": 1e3 * trs.value, "k_trailing_launches": int(nl_.value)}
        except Exception as e:       # an optional leg must never cost the headline line
            print(f"[bench] optional record 'dense' failed: {e!r}", file=sys.stderr)
            dense = {"error": repr(e)}

    # Batch curve on this one GPU: the same K timed steps over the first 64 / 128 / 256 scenarios.  A rank of an N-GPU job
    # of the 512-scenario workload holds 512 / N scenarios, so these figures predict the strong-scaling curve the driver
    # measures on a whole node (no data crosses ranks; the status gather is a few KB): speedup(N) = N x QP/s(512 / N) / QP/s(512).
    scaling_prediction = None
    if rank == 0 and world == 1 and not args.no_batch_curve and small and args.workload == "case118":
        try:
            curve = {str(total): n_qp / elapsed}
            for bk in (total // 2, total // 4, total // 8):
                kctx, _ = make_ctx(args.literal_quirks, first=bk)
                if args.warmup > 0:
                    kctx.sqp_run(args.warmup)
                k0 = kctx.counters()
                torch.cuda.synchronize()
                ta = time.perf_counter()
                kctx.sqp_run(args.steps)
                torch.cuda.synchronize()
                tb = time.perf_counter()
                curve[str(bk)] = (kctx.counters()["n_qp"] - k0["n_qp"]) / (tb - ta)
                kctx.close()
            scaling_prediction = {
                "qp_per_s_by_resident_scenarios": curve,
                "predicted_strong_scaling_speedup": {str(g): g * curve[str(total // g)] / curve[str(total)] for g in (2, 4, 8)},
                "note": "one GPU, same steps / warm-up; a prediction from the batch curve, not a multi-GPU measurement"}
        except Exception as e:
            print(f"[bench] optional record 'scaling_prediction' failed: {e!r}", file=sys.stderr)
            scaling_prediction = {"error": repr(e)}

    termination = None
    if rank == 0 and world == 1 and not args.no_termination and (small or topology == "geo"):
        try:
            termination = {}
            # (the large shapes: textbook sign only -- they converge in ~15 iterations.  Third leg of the small shapes: the textbook
            #  sign with the OTHER barrier rule -- its sub-problems are convex, where Mehrotra's predictor-corrector halves the
            #  factorisations per sub-problem and the monotone rule's cheaper sweeps do not; the options of the headline stay the
            #  library defaults)
            legs = [(1, args.ipm_corrector), (0, args.ipm_corrector), (0, 1 - args.ipm_corrector)] if small else [(0, args.ipm_corrector)]
            for lq, corr in legs:
                tctx, _ = make_ctx(lq, max_iter=60, corrector=corr)
                torch.cuda.synchronize()
                ta = time.perf_counter()
                tctx.sqp_run(0)
                torch.cuda.synchronize()
                tb = time.perf_counter()
                tc = tctx.counters()
                tm = tctx.mode_counters()
                ret, it, done = tctx.sqp_status()
                termination[f"literal_quirks_{lq}" + ("" if corr == args.ipm_corrector else f"_ipm_corrector_{corr}")] = {
                    "ipm_corrector": corr, "seconds": tb - ta, "qp_solved": int(tc["n_qp"]), "qp_per_s": tc["n_qp"] / (tb - ta),
                    "instances_done": int(np.sum(done)), "converged_ret0": int(np.sum(ret == 0)),
                    "iteration_limit": int(np.sum(ret == -1)), "other": int(np.sum((ret != 0) & (ret != -1))),
                    "outer_iterations_median": float(np.median(it)), "ipm_iterations_per_qp": tc["n_ipm_iter"] / max(1, tc["n_qp"]),
                    "factorisations_per_qp": tc["n_factor"] / max(1, tc["n_qp"]), "sweeps": int(tc["n_sweeps"]),
                    "by_mode": {k: {"solved": int(v[0]), "ipm_iterations_per_solve": v[1] / v[0],
                                    "factorisations_per_solve": v[2] / v[0]} for k, v in tm.items() if v[0] > 0}}
                tctx.close()
        except Exception as e:       # an optional leg must never cost the headline line
            print(f"[bench] optional record 'termination' failed: {e!r}", file=sys.stderr)
            termination = {"error": repr(e)}

    # scenario queue (sqphip_sqp_stream_*): FACTOR x as many scenarios as slots, each run to termination, slots refilled on
    # the device as runs end -- the throughput of a screening job, free of the wait for the busiest instance of a batch
    screening = None
    if rank == 0 and world == 1 and not args.no_screening and small:
        try:
            screening = {}
            M = args.screening_factor * total
            for lq, mi in ((1, 20), (0, 60)):
                opts_q = pkg.default_options(max_iter=mi, literal_quirks=lq, device=local_rank, ipm_corrector=args.ipm_corrector,
                                             **lin_kw, **sqp_kw)
                qctx = pkg.Context(lay0.n, lay0.m, lay0.num_linear, lay0.jrow, lay0.jcol, lay0.hrow, lay0.hcol,
                                   lay0.xL, lay0.xU, lay0.gL, lay0.gU, opts_q, batch=B)
                qctx.acopf_attach(base, lay0)
                qctx.stream_begin(M)
                for s_id in range(M):
                    net = base if s_id == 0 else contingency(base, s_id, seed)
                    qctx.stream_set(s_id, net, acopf_layout(net))
                torch.cuda.synchronize()
                ta = time.perf_counter()
                qctx.stream_run()
                torch.cuda.synchronize()
                tb = time.perf_counter()
                qc = qctx.counters()
                st = np.array([qctx.stream_get(s_id)["status"] for s_id in range(0, M, max(1, M // 256))])
                screening[f"literal_quirks_{lq}"] = {
                    "scenarios": M, "slots": B, "max_outer_iterations": mi, "seconds": tb - ta,
                    "qp_solved": int(qc["n_qp"]), "qp_per_s": qc["n_qp"] / (tb - ta), "scenarios_per_s": M / (tb - ta),
                    "factorisations_per_qp": qc["n_factor"] / max(1, qc["n_qp"]),
                    "converged_fraction_of_sample": float(np.mean(st == 0))}
                qctx.close()
        except Exception as e:       # an optional leg must never cost the headline line
            print(f"[bench] optional record 'screening' failed: {e!r}", file=sys.stderr)
            screening = {"error": repr(e)}

    cpu = None
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        try:
            # CPU restatement (NOT Julia/Ipopt): a bounded sample of the same workload, one scenario per host thread
            from concurrent.futures import ThreadPoolExecutor
            from oracle import oracle as O
            cores = host_cores()
            n_s = min(total, {"case14": 512, "case118": 512, "case1354": 32, "case9241": 2, "dense": 2}[args.workload])
            k_it = args.steps + args.warmup
            probs = [(O.problem_dense if dense_wl else O.problem_acopf)(*scenario(s)) for s in range(n_s)]

            def cpu_run(iters):
                if dense_wl:        # the dense LDL^T of the oracle on all host threads, one scenario after the other
                    oo = O.default_options(max_iter=iters, literal_quirks=args.literal_quirks, num_threads=cores, kkt_mode=1,
                                           ipm_corrector=args.ipm_corrector, **sqp_kw)
                    ta = time.perf_counter()
                    res = [O.sqp_solve(p, oo) for p in probs]
                    return time.perf_counter() - ta, sum(r["n_qp"] for r in res), sum(r["n_factor"] for r in res)
                oo = O.default_options(max_iter=iters, literal_quirks=args.literal_quirks, num_threads=1, kkt_mode=2,
                                       ipm_corrector=args.ipm_corrector, **sqp_kw)
                ta = time.perf_counter()
                with ThreadPoolExecutor(max_workers=cores) as ex:          # ctypes releases the GIL inside ora_sqp_tr_solve
                    res = list(ex.map(lambda p: O.sqp_solve(p, oo), probs))
                return time.perf_counter() - ta, sum(r["n_qp"] for r in res), sum(r["n_factor"] for r in res)
            # The timed GPU steps are outer iterations W + 1 .. W + K of every scenario (the warm-up iterations are the cheap
            # ones: fewer interior-point iterations per sub-problem).  The oracle has no resumable state, so the same window is
            # taken by difference: a run of W iterations and a run of W + K iterations, both from the start.
            sec_all, nq_all, nf_all = cpu_run(k_it)
            sec_w, nq_w, nf_w = cpu_run(args.warmup) if args.warmup > 0 else (0.0, 0, 0)
            aligned = (nq_all - nq_w) / (sec_all - sec_w) if sec_all > sec_w and nq_all > nq_w else None
            cpu = {"value": aligned if aligned is not None else nq_all / sec_all, "unit": "QP subproblems/s", "cores": cores, "kind": "port",
                   "window": f"outer iterations {args.warmup + 1}..{k_it} (the timed steps), by difference of two runs from the start",
                   "value_from_the_first_iteration": nq_all / sec_all,
                   "sample": f"{args.workload} scenarios 0..{n_s - 1}: {nq_all - nq_w} sub-problems / {nf_all - nf_w} "
                             + (f"dense LDL^T of order {N} (oracle/qp_ipm.c, blocked, {cores} OpenMP threads, one scenario after the other) "
                                if dense_wl else f"sparse LDL^T of order {N} ") +
                             f"in the window ({nq_all} / {nf_all} from the first iteration" + ("" if dense_wl else "; oracle/sparse_ldlt.c, its own minimum-degree "
                             f"order), one scenario per thread on {cores} host threads") + f", {sec_all:.1f} + {sec_w:.1f} s; CPU "
                             f"restatement (oracle/), not Julia/Ipopt"}
        except Exception as e:       # an optional leg must never cost the headline line
            print(f"[bench] optional record 'cpu' failed: {e!r}", file=sys.stderr)
            cpu = {"error": repr(e)}

    if rank == 0 and args.dump_status:
        with open(args.dump_status, "w") as fh:
            json.dump({"ret": g_ret.tolist(), "iter": g_it.tolist(), "done": g_done.tolist()}, fh)
    if rank == 0:
        out = {
            "metric": "QP subproblems/sec on batched ACOPF; fp64 KKT LDL^T TFLOPS vs MFMA peak",
            "value": n_qp / elapsed if elapsed > 0 else 0.0,
            "unit": "QP subproblems/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": 1e3 * elapsed / max(1, args.steps),
            "higher_is_better": True,
            "scaling": args.scaling,
            "vs_baseline": None,
            "dtype": "f64",
            "data": "synthetic",
            "config": {"workload": (f"{total} scenarios of a synthetic NLP with a dense Lagrangian Hessian (n = {lay0.n}, {lay0.m} linear rows; "
                                    f"BASELINE.json north_star: dense LDL^T on MFMA where the Hessian is dense), {B} per GPU, " if dense_wl else
                                    f"{total} x IEEE-{nb}-bus-shaped ACOPF contingency scenarios (BASELINE.json configs[3]"
                                    f"{'' if args.workload == 'case118' else ' shape: ' + args.workload}), {B} per GPU, ") +
                                   f"Newton matrix of order {N_full}" + (f" condensed to {N}" if int(opts.kkt_condense) and N != N_full else "")
                                   + (", multifrontal LDL^T" if c1["sparse"] else ", dense MFMA LDL^T")
                                   + ", fp64, SQP-TR outer iterations",
                       "instances_total": total, "instances_per_gpu": B, "kkt_order": N, "kkt_order_full": N_full,
                       "formulation": args.formulation, "topology": topology, "use_soc": use_soc, "sqp_options": args.sqp_options,
                       "literal_quirks": args.literal_quirks, "ipm_corrector": args.ipm_corrector,
                       "kkt_mode": args.kkt_mode, "sparse_solver": int(c1["sparse"]), "kkt_condense": int(opts.kkt_condense),
                       "status_gather": "sqphip_gather_status (RCCL)" if use_lib_comm else
                                        ("local" if world == 1 else "torch.distributed " + args.backend),
                       "qp_solved": n_qp, "ipm_iterations": n_ipm, "kkt_factorisations": n_fac,
                       "sweeps": int(c1["n_sweeps"] - c0["n_sweeps"]),
                       "ipm_iterations_per_qp": n_ipm / max(1.0, n_qp), "factorisations_per_qp": n_fac / max(1.0, n_qp),
                       "by_mode": by_mode,
                       "qp_termination": {"what": "sub-problems of this rank since the start of the run (warm-up included) by the way their interior-point run "
                                                  "ended: scaled optimality error <= ipm_tol (1e-9), or the acceptable-termination rules 1 / 2 / 3 "
                                                  "(8 iterates within 1e-7, 15 within 1e-6, 25 within 1e-5)",
                                          "tolerance": term_rules[0], "rule1": term_rules[1], "rule2": term_rules[2], "rule3": term_rules[3]},
                       "busiest_instance_over_mean": float(wfac.max() / max(1.0, wfac.mean())),
                       "instances_done_in_timed_steps": int(np.sum(g_done)),
                       "parity_note": ("this configuration is compared with the oracle's committed fixture of scenario 1 (tests/golden/geo9241_s1.npz: "
                                       "decisions, statuses and interior-point counts of the first seven outer iterations; the converged point at 1e-8 "
                                       "with the textbook sign).  The trust-region QPs of the first three outer iterations end by the third "
                                       "acceptable-termination rule at a scaled error of 2e-6 ... 4e-6 -- on the device and in the oracle alike -- i.e. they "
                                       "are accurate to ~1e-6, not 1e-9 (qp_termination.rule3 counts them); DESIGN.md section 3"
                                       if args.workload == "case9241" else
                                       "this configuration (literal_quirks = 1) is compared with the oracle by exact decisions and "
                                       "per-sub-problem replays (tests/test_gpu_parity_depth.py); iterates at 1e-8 are "
                                       "asserted on converging runs (literal_quirks = 0), DESIGN.md section 8"),
                       "note": "with literal_quirks = 1 (the reference's JuMP-sign Hessian, SURVEY.md App. C #2) the "
                               "sub-problems are non-convex and most scenarios never meet the termination test; see "
                               "`termination` (--full) for both sign conventions run to the end"},
            "roofline": roofline,
            "kernels": kernels,
            "dense_ldlt": dense,
            "termination": termination,
            "screening": screening,
            "scaling_prediction": scaling_prediction,
            "cpu_baseline": cpu,
        }
        print(json.dumps(out))
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
