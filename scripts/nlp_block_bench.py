"""The numbers of the dense data blocks (sqphip_nlp_add_block, csrc/nlp_block_dev.hpp) on one GPU.  Prints one JSON line.

  small   d = 8, N = 512, 64 bootstrap resamples of one logistic fit: the block (logistic_block_model, weights per instance)
          against the same models as per-point terms through sqphip_nlp_attach_data (logistic_model on the resampled rows):
          QP/s of a run to termination and seconds per full evaluator call (f, grad, g, J, H through sqphip_acopf_eval: one
          launch of k_acopf_eval_point and its copies).
  large   d = 64 and d = 128 at N = 4096, 64 fold-like weight vectors: QP/s, seconds per evaluator call with and without the
          Hessian, and the share of the fp64 MFMA peak of one CU (the probe sqphip_mfma_f64_peak over the CU count; one
          workgroup per instance runs on one CU) that the Hessian phase reaches: 2 N 256 flops per lower 16 x 16 tile over
          the difference of the two call times.

Every timed section is preceded by an untimed call of the same kind and ends on a device synchronisation.

    python scripts/nlp_block_bench.py [--runs 3] [--calls 20] [--batch 64] [--skip-large]"""
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
from sqpsolver_jl_amd.nlp_terms import logistic_block_model, logistic_model, nlp_terms_layout   # noqa: E402

OPTS = dict(max_iter=60, literal_quirks=0, tol_infeas=1e-8, tol_residual=1e-8)


def dataset(N, d, seed):
    rng = np.random.default_rng(seed)
    X = np.column_stack([np.ones(N), rng.standard_normal((N, d - 1))])
    w = rng.standard_normal(d)
    y = (X @ (w / np.linalg.norm(w)) + 0.8 * rng.standard_normal(N) > 0).astype(float)
    return X, y


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


def median_run(fn, runs):
    out = [fn() for _ in range(runs)]
    return out, float(np.median([r["qp_per_s"] for r in out]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--skip-large", action="store_true")
    args = ap.parse_args()
    B = args.batch
    out = {"what": "dense data blocks: scripts/nlp_block_bench.py", "batch": B, "runs": args.runs, "calls": args.calls}
    v = C.c_double()
    peak = v.value if _lib.lib().sqphip_mfma_f64_peak(0, C.byref(v)) == 0 else None
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    out["mfma_f64_peak_tflops"], out["compute_units"] = peak, cus

    # small: the block against per-point terms
    N, d = 512, 8
    X, y = dataset(N, d, 1)
    rng = np.random.default_rng(2)
    idx = [rng.integers(0, N, N) for _ in range(B)]                    # bootstrap resamples: rows with repetition
    W = [np.bincount(i, minlength=N).astype(float) for i in idx]
    x = 0.1 * rng.standard_normal(d)
    pb = logistic_block_model(X, y, 0.5, W[0])
    cb = context(nlp_terms_layout(pb), B)
    cb.nlp_attach(pb)
    for b in range(B):
        cb.nlp_set_instance(b, pb, weight=W[b])
    pts = [logistic_model(X[i], y[i], 0.5) for i in idx]
    ct = context(nlp_terms_layout(pts[0]), B)
    ct.nlp_attach(pts[0], instance_data=True)
    for b in range(B):
        ct.nlp_set_instance(b, pts[b])
    small = {"N": N, "d": d}
    for name, ctx in (("block", cb), ("per_point_terms", ct)):
        solve(ctx)                                                     # untimed
        runs, med = median_run(lambda: solve(ctx), args.runs)
        small[name] = {"runs": runs, "median_qp_per_s": med, "evaluator_seconds_per_call": eval_seconds(ctx, x, args.calls)}
    xb, xt = cb.sqp_get(0)["x"], ct.sqp_get(0)["x"]
    small["max_abs_difference_of_the_optima"] = float(np.abs(xb - xt).max())
    small["qp_per_s_ratio_block_over_terms"] = small["block"]["median_qp_per_s"] / small["per_point_terms"]["median_qp_per_s"]
    small["evaluator_ratio_terms_over_block"] = small["per_point_terms"]["evaluator_seconds_per_call"] / small["block"]["evaluator_seconds_per_call"]
    cb.close(); ct.close()
    out["small"] = small

    out["large"] = []
    for N, d in ([] if args.skip_large else [(4096, 64), (4096, 128)]):
        X, y = dataset(N, d, 3)
        rng = np.random.default_rng(4)
        W = [(rng.uniform(0, 1, N) > 0.25).astype(float) for _ in range(B)]
        p = logistic_block_model(X, y, 0.5, W[0])
        ctx = context(nlp_terms_layout(p), B)
        ctx.nlp_attach(p)
        for b in range(B):
            ctx.nlp_set_instance(b, p, weight=W[b])
        x = 0.05 * rng.standard_normal(d)
        solve(ctx)
        runs, med = median_run(lambda: solve(ctx), args.runs)
        full, nohess = eval_seconds(ctx, x, args.calls, True), eval_seconds(ctx, x, args.calls, False)
        nt = (d + 15) // 16
        flops = 2.0 * N * 256 * (nt * (nt + 1) // 2)
        rec = {"N": N, "d": d, "runs": runs, "median_qp_per_s": med, "evaluator_seconds_per_call": full,
               "evaluator_seconds_per_call_without_hessian": nohess, "hessian_tile_flops": flops}
        if peak and full > nohess:
            rec["hessian_tflops"] = flops / (full - nohess) / 1e12
            rec["share_of_one_cu_mfma_peak"] = rec["hessian_tflops"] / (peak / cus)
        ctx.close()
        out["large"].append(rec)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
