"""The numbers of the multinomial (softmax) data blocks (sqphip_nlp_add_softmax_block, csrc/nlp_softmax_dev.hpp) on one GPU.
Prints one JSON line.

Two shapes, K = 3, d = 8, N = 512 and K = 10, d = 12, N = 4096, pinned (Kf d = 16 and 108 columns), 64 fold-like weight vectors
each: QP/s of a run to termination, seconds per evaluator call with and without the Hessian (sqphip_acopf_eval: one launch
of k_acopf_eval_point and its copies), and the share of the fp64 MFMA peak of one CU (the probe sqphip_mfma_f64_peak over the
CU count; one workgroup per instance runs on one CU) that the Hessian phase reaches: 2 N 256 flops per executed chain per
lower 16 x 16 tile -- chain 1 on every tile, chain 2 on the tiles whose rows and columns share a class -- over the difference
of the two call times.  The yardstick is the scalar block's share in profiles/nlp_block_bench.json.

Every timed section is preceded by an untimed call of the same kind and ends on a device synchronisation.

    python scripts/nlp_softmax_bench.py [--runs 3] [--calls 20] [--batch 64]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np                                                     # noqa: E402
import torch                                                           # noqa: E402

import sqpsolver_jl_amd as pkg                                         # noqa: E402
from sqpsolver_jl_amd import _lib                                      # noqa: E402
from sqpsolver_jl_amd.nlp_terms import multinomial_block_model, nlp_terms_layout   # noqa: E402

OPTS = dict(max_iter=60, literal_quirks=0, tol_infeas=1e-8, tol_residual=1e-8)
SHAPES = [(3, 8, 512), (10, 12, 4096)]                                 # (K, d, N)


def dataset(N, d, K, seed):
    rng = np.random.default_rng(seed)
    X = np.column_stack([np.ones(N), rng.standard_normal((N, d - 1))])
    B = rng.standard_normal((d, K)) / np.sqrt(d)
    return X, np.argmax(X @ B + 0.8 * rng.gumbel(size=(N, K)), axis=1).astype(np.int32)


def context(lay, batch):
    return pkg.Context(lay.n, lay.m, lay.num_linear, lay.jrow, lay.jcol, lay.hrow, lay.hcol, lay.xL, lay.xU, lay.gL, lay.gU,
                       pkg.default_options(**OPTS), batch=batch)


def solve(ctx):
    ctx.sqp_reset()
    torch.cuda.synchronize()
    c0 = ctx.counters()
    t0 = time.perf_counter()
    ctx.sqp_run(0)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    c1 = ctx.counters()
    st, it = ctx.sqp_status()[:2]
    return {"qp_per_s": (c1["n_qp"] - c0["n_qp"]) / (t1 - t0), "seconds": t1 - t0, "n_qp": int(c1["n_qp"] - c0["n_qp"]),
            "converged": int(np.sum(np.asarray(st) == 0)), "iterations": int(np.sum(it))}


def eval_seconds(ctx, x, calls, hessian=True):
    lam = np.zeros(ctx.m) if hessian else None
    ctx.acopf_eval(0, x, 1.0, lam)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(calls):
        ctx.acopf_eval(k % ctx.batch, x, 1.0, lam)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls


def executed_chains(Kf, d):
    """(lower tiles, chains executed over them): chain 2 runs on a tile whose rows and columns share a class"""
    D = Kf * d
    nt = (D + 15) // 16
    tiles = chains = 0
    for R in range(nt):
        for Cc in range(R + 1):
            rlo, rhi = 16 * R // d, min(16 * R + 15, D - 1) // d
            clo, chi = 16 * Cc // d, min(16 * Cc + 15, D - 1) // d
            tiles += 1
            chains += 2 if (rlo <= chi and clo <= rhi) else 1
    return tiles, chains


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--batch", type=int, default=64)
    args = ap.parse_args()
    B = args.batch
    out = {"what": "multinomial (softmax) data blocks: scripts/nlp_softmax_bench.py", "batch": B, "runs": args.runs, "calls": args.calls}
    v = C.c_double()
    peak = v.value if _lib.lib().sqphip_mfma_f64_peak(0, C.byref(v)) == 0 else None
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    out["mfma_f64_peak_tflops"], out["compute_units"] = peak, cus
    out["scalar_block_share_of_one_cu_mfma_peak"] = "12.7 - 15.4 % (profiles/nlp_block_bench.json)"
    out["shapes"] = []
    for K, d, N in SHAPES:
        X, y = dataset(N, d, K, 3)
        rng = np.random.default_rng(4)
        W = [(rng.uniform(0, 1, N) > 0.25).astype(float) for _ in range(B)]
        p = multinomial_block_model(X, y, K, 0.5, True, W[0])
        ctx = context(nlp_terms_layout(p), B)
        ctx.nlp_attach(p)
        for b in range(B):
            ctx.nlp_set_instance(b, p, weight=W[b])
        x = 0.05 * rng.standard_normal(p.n)
        solve(ctx)                                                     # untimed
        runs = [solve(ctx) for _ in range(args.runs)]
        full, nohess = eval_seconds(ctx, x, args.calls, True), eval_seconds(ctx, x, args.calls, False)
        tiles, chains = executed_chains(K - 1, d)
        flops = 2.0 * N * 256 * chains
        rec = {"K": K, "d": d, "N": N, "pinned": 1, "columns": (K - 1) * d, "runs": runs,
               "median_qp_per_s": float(np.median([r["qp_per_s"] for r in runs])), "evaluator_seconds_per_call": full,
               "evaluator_seconds_per_call_without_hessian": nohess, "lower_tiles": tiles, "executed_chains": chains,
               "hessian_chain_flops": flops}
        if peak and full > nohess:
            rec["hessian_tflops"] = flops / (full - nohess) / 1e12
            rec["share_of_one_cu_mfma_peak"] = rec["hessian_tflops"] / (peak / cus)
        ctx.close()
        out["shapes"].append(rec)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
