"""The numbers of the Cox partial-likelihood data blocks (sqphip_nlp_add_cox_block, csrc/nlp_cox_dev.hpp) on one GPU.  Prints
one JSON line and, with --out, writes it to a file.

One shape, N = 2048 points with tied times, d = 32 features, ridge 0.5, and 256 bootstrap resamples (integer weights) as the
instances of one context: QP/s of a run to termination, and seconds per evaluator call (sqphip_acopf_eval: one launch of
k_acopf_eval_point and its copies, one workgroup on one CU) asked for f alone, for f and the gradient, and for everything.  The
three calls nest, so their differences split a full evaluation into
    logits, maximum, exp and the scan of T                     (the call for f alone: the Armijo probe's path),
    the d scans of P, the scan of Q and the gradient           (f and gradient minus f alone),
    the two MFMA chains of the Hessian                         (everything minus f and gradient),
each with the launch and the copies of its call in it; the call on a context without any block gives that floor.  The Hessian
phase is also stated as a share of the fp64 MFMA peak of one CU (the probe sqphip_mfma_f64_peak over the CU count): 2 N 256
flops per chain and lower 16 x 16 tile, two chains on every tile.

Every timed section is preceded by an untimed call of the same kind and ends on a device synchronisation.

    python scripts/nlp_cox_bench.py [--runs 3] [--calls 20] [--batch 256] [--points 2048] [--features 32] [--out FILE]"""
import argparse
import ctypes as C
import dataclasses
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
from sqpsolver_jl_amd.nlp_terms import cox_block_model, nlp_terms_layout   # noqa: E402

OPTS = dict(max_iter=60, literal_quirks=0, tol_infeas=1e-8, tol_residual=1e-8)
_dp = C.POINTER(C.c_double)


def dataset(N, d, seed):
    """exponential survival times with hazard exp(A beta), rounded to two decimals (ties), about a quarter censored"""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((N, d))
    t = rng.exponential(np.exp(-(A @ (rng.standard_normal(d) / np.sqrt(d)))))
    cens = rng.exponential(2.5, N)
    return A, np.round(np.minimum(t, cens), 2), (t <= cens).astype(float)


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


def eval_seconds(ctx, x, calls, what):
    """seconds per call asked for "f", "fg" (f and the gradient) or "all" """
    x = np.ascontiguousarray(x, dtype=np.float64)
    f = C.c_double()
    g, lam = np.zeros(ctx.m), np.zeros(ctx.m)
    grad = np.zeros(ctx.n) if what != "f" else None
    hv = np.zeros(ctx.nnzh) if what == "all" else None
    ptr = lambda a: None if a is None else a.ctypes.data_as(_dp)

    def call(inst):
        ctx._ck(ctx.L.sqphip_acopf_eval(ctx.h, inst, ptr(x), 1.0, ptr(lam), C.byref(f), ptr(grad), ptr(g), None, ptr(hv)))

    call(0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(calls):
        call(k % ctx.batch)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--points", type=int, default=2048)
    ap.add_argument("--features", type=int, default=32)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    B, N, d = args.batch, args.points, args.features
    out = {"what": "Cox partial-likelihood data blocks: scripts/nlp_cox_bench.py", "batch": B, "runs": args.runs, "calls": args.calls}
    v = C.c_double()
    peak = v.value if _lib.lib().sqphip_mfma_f64_peak(0, C.byref(v)) == 0 else None
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    out["mfma_f64_peak_tflops"], out["compute_units"] = peak, cus
    A, t, ev = dataset(N, d, 3)
    rng = np.random.default_rng(4)
    p = cox_block_model(A, t, ev, 0.5)
    W = [np.bincount(rng.integers(0, N, N), minlength=N).astype(float) for _ in range(B)]      # resamples, in the block's order
    lay = nlp_terms_layout(p)
    ctx = context(lay, B)
    ctx.nlp_attach(p)
    for b in range(B):
        ctx.nlp_set_instance(b, p, weight=W[b])
    x = 0.05 * rng.standard_normal(p.n)
    solve(ctx)                                                         # untimed
    runs = [solve(ctx) for _ in range(args.runs)]
    sec = {k: eval_seconds(ctx, x, args.calls, k) for k in ("f", "fg", "all")}
    ctx.close()
    bare = context(lay, B)                                             # the same terms without the block: launch and copies
    bare.nlp_attach(dataclasses.replace(p, blocks=[]))
    for b in range(B):
        bare.nlp_set_instance(b, dataclasses.replace(p, blocks=[]))
    floor = {k: eval_seconds(bare, x, args.calls, k) for k in ("f", "fg", "all")}
    bare.close()
    nt = (d + 15) // 16
    tiles = nt * (nt + 1) // 2
    flops = 2.0 * N * 256 * 2 * tiles
    rec = {"N": N, "d": d, "distinct_risk_sets": int(len(set(p.blocks[0].risk.tolist()))), "events": int(ev.sum()), "runs": runs,
           "median_qp_per_s": float(np.median([r["qp_per_s"] for r in runs])),
           "evaluator_seconds_per_call": sec, "evaluator_seconds_per_call_without_the_block": floor,
           "share_of_a_full_evaluation": {"logits_exp_and_the_scan_of_T (the call for f alone)": sec["f"] / sec["all"],
                                          "scans_of_P_and_Q_and_the_gradient": (sec["fg"] - sec["f"]) / sec["all"],
                                          "the_two_mfma_chains": (sec["all"] - sec["fg"]) / sec["all"]},
           "lower_tiles": tiles, "hessian_chain_flops": flops}
    if peak and sec["all"] > sec["fg"]:
        rec["hessian_tflops"] = flops / (sec["all"] - sec["fg"]) / 1e12
        rec["share_of_one_cu_mfma_peak"] = rec["hessian_tflops"] / (peak / cus)
    out["shape"] = rec
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
