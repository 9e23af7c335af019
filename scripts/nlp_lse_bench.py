"""The numbers of the log-sum-exp row blocks (sqphip_nlp_add_lse_block, csrc/nlp_lse_dev.hpp) on one GPU.  Prints one JSON line
and, with --out, writes it to a file.

One shape: a seeded geometric programme (nlp_terms.gp_synth) of R = 64 posynomials -- the objective and 63 constraints -- with
N = 2048 monomials in all on d = 64 log variables, and a batch of gp_scenario instances (other log-coefficients) as the
instances of one context: QP/s of a run to termination, and seconds per evaluator call (sqphip_acopf_eval: one launch of
k_acopf_eval_point and its copies, one workgroup on one CU) asked for the values alone, for values, gradient and Jacobian, and
for everything.  The three calls nest, so their differences split a full evaluation into
    steps 1 - 4: logits, maxima, exponentials, sums and values      (the call for values alone: the Armijo probe's path),
    steps 5 - 6: probabilities and the R d first derivatives         (with first derivatives minus values alone),
    step 7: the two MFMA chains of the Hessian (and z, G for all)    (everything minus with first derivatives),
each with the launch and the copies of its call in it; the call on a context without the block gives that floor.  Inside a
launch the seven steps are not timed apart: a workgroup has no clock that is worth more than these differences.  The Hessian
phase is also stated as a share of the fp64 MFMA peak of one CU (the probe sqphip_mfma_f64_peak over the CU count):
2 (N + R) 256 flops per lower 16 x 16 tile.

Every timed section is preceded by an untimed call of the same kind and ends on a device synchronisation.

    python scripts/nlp_lse_bench.py [--runs 3] [--calls 20] [--batch 256] [--points 2048] [--columns 64] [--outputs 64] [--out FILE]"""
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
from sqpsolver_jl_amd.nlp_terms import gp_scenario, gp_synth, nlp_terms_layout   # noqa: E402

OPTS = dict(max_iter=60, literal_quirks=0, tol_infeas=1e-8, tol_residual=1e-8)
_dp = C.POINTER(C.c_double)


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
    """seconds per call asked for "values", "first" (values, gradient and Jacobian) or "all" """
    x = np.ascontiguousarray(x, dtype=np.float64)
    f = C.c_double()
    g, lam = np.zeros(ctx.m), np.full(ctx.m, 0.5)
    grad = np.zeros(ctx.n) if what != "values" else None
    jv = np.zeros(ctx.nnzj) if what != "values" else None
    hv = np.zeros(ctx.nnzh) if what == "all" else None
    ptr = lambda a: None if a is None else a.ctypes.data_as(_dp)

    def call(inst):
        ctx._ck(ctx.L.sqphip_acopf_eval(ctx.h, inst, ptr(x), 1.0, ptr(lam), C.byref(f), ptr(grad), ptr(g), ptr(jv), ptr(hv)))

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
    ap.add_argument("--columns", type=int, default=64)
    ap.add_argument("--outputs", type=int, default=64)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    B, N, d, R = args.batch, args.points, args.columns, args.outputs
    out = {"what": "log-sum-exp row blocks: scripts/nlp_lse_bench.py", "batch": B, "runs": args.runs, "calls": args.calls}
    v = C.c_double()
    peak = v.value if _lib.lib().sqphip_mfma_f64_peak(0, C.byref(v)) == 0 else None
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    out["mfma_f64_peak_tflops"], out["compute_units"] = peak, cus
    lens = [N // R + (1 if k < N % R else 0) for k in range(R)]
    p = gp_synth(d, lens, 3)
    lay = nlp_terms_layout(p)
    ctx = context(lay, B)
    ctx.nlp_attach(p)
    for b in range(B):
        ctx.nlp_set_instance(b, gp_scenario(p, b, 3, 0.1))
    x = 0.05 * np.random.default_rng(4).standard_normal(p.n)
    solve(ctx)                                                         # untimed
    runs = [solve(ctx) for _ in range(args.runs)]
    sec = {k: eval_seconds(ctx, x, args.calls, k) for k in ("values", "first", "all")}
    ctx.close()
    bare_p = dataclasses.replace(p, blocks=[])
    bare = context(lay, B)                                             # the same terms without the block: launch and copies
    bare.nlp_attach(bare_p)
    for b in range(B):
        bare.nlp_set_instance(b, bare_p)
    floor = {k: eval_seconds(bare, x, args.calls, k) for k in ("values", "first", "all")}
    bare.close()
    nt = (d + 15) // 16
    tiles = nt * (nt + 1) // 2
    flops = 2.0 * (N + R) * 256 * tiles
    rec = {"N": N, "d": d, "R": R, "columns_in_use": int(p.blocks[0].A.shape[1]), "runs": runs,
           "median_qp_per_s": float(np.median([r["qp_per_s"] for r in runs])),
           "evaluator_seconds_per_call": sec, "evaluator_seconds_per_call_without_the_block": floor,
           "share_of_a_full_evaluation": {"steps_1_to_4_logits_maxima_exponentials_sums (the call for values alone)": sec["values"] / sec["all"],
                                          "steps_5_and_6_probabilities_and_first_derivatives": (sec["first"] - sec["values"]) / sec["all"],
                                          "step_7_the_two_mfma_chains": (sec["all"] - sec["first"]) / sec["all"]},
           "lower_tiles": tiles, "hessian_chain_flops": flops}
    if peak and sec["all"] > sec["first"]:
        rec["hessian_tflops"] = flops / (sec["all"] - sec["first"]) / 1e12
        rec["share_of_one_cu_mfma_peak"] = rec["hessian_tflops"] / (peak / cus)
    out["shape"] = rec
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
