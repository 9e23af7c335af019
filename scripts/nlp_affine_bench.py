"""What affine multi-variable arguments buy the generic path on the bench workload of `bench.py`: 512 IEEE-118-shaped polar
contingency scenarios through the dedicated polar evaluator (sqphip_acopf_attach), through the expanded restatement (four
four-factor terms per flow row, sqphip_nlp_attach) and through the joint restatement (v_f v_t cos(th_f - th_t) and
v_f v_t sin(th_f - th_t), sqphip_nlp_attach_affine), with the same structure, options, steps and warmup.  The three legs
alternate, `--runs` runs each.  Prints one JSON line: every run (QP/s, work counters, per-class kernel seconds), the medians
and the ratios to the dedicated path.  `--legs expanded` runs that leg alone: with SQPHIP_SO naming another build of the
library (one without sqphip_nlp_attach_affine will do) it measures what a change costs the existing entry point.

    python scripts/nlp_affine_bench.py [--batch 512] [--steps 20] [--warmup 5] [--runs 3] [--legs polar,expanded,joint]"""
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
from sqpsolver_jl_amd.nlp_terms import from_polar_acopf, nlp_terms_args   # noqa: E402

LEGS = ("polar", "expanded", "joint")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--literal-quirks", type=int, default=1)
    ap.add_argument("--legs", default=",".join(LEGS))
    args = ap.parse_args()
    legs = tuple(k for k in LEGS if k in args.legs.split(","))
    nb, ng, nl, seed = CASES["case118"]
    base = synth_case("case118", None)
    nets = [base if s == 0 else contingency(base, s, seed) for s in range(args.batch)]
    lays = [acopf_layout(nt) for nt in nets]
    ps = {k: [from_polar_acopf(nt, ly, joint=k == "joint") for nt, ly in zip(nets, lays)] for k in legs if k != "polar"}
    lay0 = lays[0]
    opts = dict(max_iter=3000, literal_quirks=args.literal_quirks, use_soc=1, tol_infeas=1e-6, tol_residual=1e-4)

    def make(kind):
        ctx = pkg.Context(lay0.n, lay0.m, lay0.num_linear, lay0.jrow, lay0.jcol, lay0.hrow, lay0.hcol, lay0.xL, lay0.xU,
                          lay0.gL, lay0.gU, pkg.default_options(**opts), batch=args.batch)
        if kind == "polar":
            ctx.acopf_attach(nets[0], lay0)
            for b in range(args.batch):
                ctx.acopf_set_instance(b, nets[b], lays[b])
        else:
            ctx.nlp_attach(ps[kind][0])
            for b in range(args.batch):
                ctx.nlp_set_instance(b, ps[kind][b])
        ctx.sqp_reset()
        return ctx

    def one(kind):
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
        st, it = ctx.sqp_status()[:2]
        ctx.close()
        return {"qp_per_s": (c1["n_qp"] - c0["n_qp"]) / (tb - ta), "seconds": tb - ta,
                "n_qp": int(c1["n_qp"] - c0["n_qp"]), "n_ipm_iter": int(c1["n_ipm_iter"] - c0["n_ipm_iter"]),
                "n_factor": int(c1["n_factor"] - c0["n_factor"]), "kernel_seconds": {k: v[0] for k, v in kt.items()},
                "status_hash": int(np.sum(np.asarray(st, dtype=np.int64) * 31 + np.asarray(it, dtype=np.int64)))}

    size = lambda p: {"terms": int(len(p.trow)), "factors": int(len(p.fkind)), "arguments": int(len(nlp_terms_args(p)[1]))}
    out = {"workload": f"{args.batch} x IEEE-118-shaped polar contingency scenarios", "steps": args.steps, "warmup": args.warmup,
           "literal_quirks": args.literal_quirks, "order": ", ".join(legs) + f" x {args.runs}",
           "nlp_terms": {k: size(v[0]) for k, v in ps.items()}, "runs": {k: [] for k in legs}}
    for _ in range(args.runs):
        for kind in legs:
            out["runs"][kind].append(one(kind))
    med = {k: float(np.median([r["qp_per_s"] for r in out["runs"][k]])) for k in legs}
    out["median_qp_per_s"] = med
    if legs != LEGS:
        print(json.dumps(out))
        return
    out["expanded_min_qp_per_s"] = min(r["qp_per_s"] for r in out["runs"]["expanded"])
    out["ratio_expanded_over_polar"] = med["expanded"] / med["polar"]
    out["ratio_joint_over_polar"] = med["joint"] / med["polar"]
    out["joint_median_not_below_expanded_min"] = med["joint"] >= out["expanded_min_qp_per_s"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
