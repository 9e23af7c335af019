"""The factorable-NLP path against the dedicated polar evaluator on the bench workload of `bench.py`: 512 IEEE-118-shaped
polar contingency scenarios, restated as sums of products of univariate functions (nlp_terms.from_polar_acopf), run through
sqphip_nlp_attach and through sqphip_acopf_attach with the same structure, options, steps and warmup.  Prints one JSON line:
QP/s of both paths, their work counters and the share of the transition kernels -- the stage kernels that hold the
evaluator -- in the kernel time (sqphip_get_kernel_times).

    python scripts/nlp_bench.py [--batch 512] [--steps 20] [--warmup 5]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np                                                     # noqa: E402
import torch                                                           # noqa: E402

import sqpsolver_jl_amd as pkg                                         # noqa: E402
from sqpsolver_jl_amd.acopf_synth import synth_case, acopf_layout, contingency, CASES   # noqa: E402
from sqpsolver_jl_amd.nlp_terms import from_polar_acopf              # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--literal-quirks", type=int, default=1)
    args = ap.parse_args()
    nb, ng, nl, seed = CASES["case118"]
    base = synth_case("case118", None)
    nets = [base if s == 0 else contingency(base, s, seed) for s in range(args.batch)]
    lays = [acopf_layout(nt) for nt in nets]
    t0 = time.perf_counter()
    ps = [from_polar_acopf(nt, ly) for nt, ly in zip(nets, lays)]
    t_restate = time.perf_counter() - t0
    lay0 = lays[0]
    opts = dict(max_iter=3000, literal_quirks=args.literal_quirks, use_soc=1, tol_infeas=1e-6, tol_residual=1e-4)

    def make(kind):
        ctx = pkg.Context(lay0.n, lay0.m, lay0.num_linear, lay0.jrow, lay0.jcol, lay0.hrow, lay0.hcol, lay0.xL, lay0.xU,
                          lay0.gL, lay0.gU, pkg.default_options(**opts), batch=args.batch)
        if kind == "nlp":
            ctx.nlp_attach(ps[0])
            for b in range(args.batch):
                ctx.nlp_set_instance(b, ps[b])
        else:
            ctx.acopf_attach(nets[0], lay0)
            for b in range(args.batch):
                ctx.acopf_set_instance(b, nets[b], lays[b])
        ctx.sqp_reset()
        return ctx

    out = {"workload": f"{args.batch} x IEEE-118-shaped polar contingency scenarios", "steps": args.steps,
           "warmup": args.warmup, "literal_quirks": args.literal_quirks,
           "nlp_terms": {"terms": int(len(ps[0].trow)), "factors": int(len(ps[0].fvar))}, "restate_seconds": t_restate}
    for kind in ("polar", "nlp"):
        ctx = make(kind)
        if args.warmup:
            ctx.sqp_run(args.warmup)
        c0 = ctx.counters()
        torch.cuda.synchronize()
        ctx.L.sqphip_set_timing(ctx.h, 2)           # 2: per-class kernel times (sqphip_get_kernel_times)
        ta = time.perf_counter()
        ctx.sqp_run(args.steps)
        torch.cuda.synchronize()
        tb = time.perf_counter()
        ctx.set_timing(False)
        c1 = ctx.counters()
        kt = ctx.kernel_times()
        ksum = sum(v[0] for v in kt.values())
        st, it = ctx.sqp_status()[:2]
        out[kind] = {"qp_per_s": (c1["n_qp"] - c0["n_qp"]) / (tb - ta), "seconds": tb - ta,
                     "n_qp": int(c1["n_qp"] - c0["n_qp"]), "n_ipm_iter": int(c1["n_ipm_iter"] - c0["n_ipm_iter"]),
                     "n_factor": int(c1["n_factor"] - c0["n_factor"]),
                     "transition_kernel_share": kt["transitions"][0] / ksum if ksum > 0 else None,
                     "kernel_seconds": {k: v[0] for k, v in kt.items()},
                     "status_hash": int(np.sum(np.asarray(st, dtype=np.int64) * 31 + np.asarray(it, dtype=np.int64)))}
        ctx.close()
    out["ratio_nlp_over_polar"] = out["nlp"]["qp_per_s"] / out["polar"]["qp_per_s"]
    out["same_work"] = all(out["nlp"][k] == out["polar"][k] for k in ("n_qp", "n_ipm_iter", "n_factor", "status_hash"))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
