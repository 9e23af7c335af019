"""What per-instance data costs the generic path on the bench workload of `bench.py`: 512 IEEE-118-shaped polar contingency
scenarios in the joint restatement (v_f v_t cos(th_f - th_t) and v_f v_t sin(th_f - th_t), an affine argument per angle
difference) through sqphip_nlp_attach_general -- shifts and coefficients shared by the batch, read by all instances from
the same lines of L2 -- and through sqphip_nlp_attach_data with identical data in every instance's own block, with the
same structure, options, steps and warmup.  The two legs alternate, `--runs` runs each.  Prints one JSON line: every run
(QP/s, work counters, per-class kernel seconds), the medians, their ratio, whether the work counters and the final
points are equal (the bit rule of the header says they are) and the doubles per instance of both layouts.

    python scripts/nlp_data_bench.py [--batch 512] [--steps 20] [--warmup 5] [--runs 3]"""
import argparse
import hashlib
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

LEGS = ("general", "data")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--literal-quirks", type=int, default=1)
    args = ap.parse_args()
    nb, ng, nl, seed = CASES["case118"]
    base = synth_case("case118", None)
    nets = [base if s == 0 else contingency(base, s, seed) for s in range(args.batch)]
    lays = [acopf_layout(nt) for nt in nets]
    ps = [from_polar_acopf(nt, ly, joint=True) for nt, ly in zip(nets, lays)]
    lay0 = lays[0]
    opts = dict(max_iter=3000, literal_quirks=args.literal_quirks, use_soc=1, tol_infeas=1e-6, tol_residual=1e-4)

    def make(kind):
        ctx = pkg.Context(lay0.n, lay0.m, lay0.num_linear, lay0.jrow, lay0.jcol, lay0.hrow, lay0.hcol, lay0.xL, lay0.xU,
                          lay0.gL, lay0.gU, pkg.default_options(**opts), batch=args.batch)
        if kind == "data":
            ctx.nlp_attach(ps[0], instance_data=True)
        else:
            ctx.nlp_attach(ps[0], general=True)
        for b in range(args.batch):
            ctx.nlp_set_instance(b, ps[b])          # (on the data leg this also sends the instance's -- identical -- data)
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
        x = np.concatenate([ctx.sqp_get(b)["x"] for b in range(0, args.batch, max(1, args.batch // 16))])
        ctx.close()
        return {"qp_per_s": (c1["n_qp"] - c0["n_qp"]) / (tb - ta), "seconds": tb - ta,
                "n_qp": int(c1["n_qp"] - c0["n_qp"]), "n_ipm_iter": int(c1["n_ipm_iter"] - c0["n_ipm_iter"]),
                "n_factor": int(c1["n_factor"] - c0["n_factor"]), "kernel_seconds": {k: v[0] for k, v in kt.items()},
                "status_hash": int(np.sum(np.asarray(st, dtype=np.int64) * 31 + np.asarray(it, dtype=np.int64))),
                "x_sha1": hashlib.sha1(x.tobytes()).hexdigest()[:16]}

    p0 = ps[0]
    nfac, nargs = len(p0.fkind), len(nlp_terms_args(p0)[1])
    shared = 1 + p0.m + len(p0.trow)
    own = shared + nfac + nargs + (nfac if p0.fpar is not None else 0)
    out = {"workload": f"{args.batch} x IEEE-118-shaped polar contingency scenarios, joint restatement", "steps": args.steps,
           "warmup": args.warmup, "literal_quirks": args.literal_quirks, "order": ", ".join(LEGS) + f" x {args.runs}",
           "nlp_terms": {"terms": int(len(p0.trow)), "factors": int(nfac), "arguments": int(nargs)},
           "doubles_per_instance": {"general": shared + shared % 2, "data": own + own % 2}, "runs": {k: [] for k in LEGS}}
    for _ in range(args.runs):
        for kind in LEGS:
            out["runs"][kind].append(one(kind))
    med = {k: float(np.median([r["qp_per_s"] for r in out["runs"][k]])) for k in LEGS}
    out["median_qp_per_s"] = med
    out["ratio_data_over_general"] = med["data"] / med["general"]
    work = lambda r: (r["n_qp"], r["n_ipm_iter"], r["n_factor"], r["status_hash"])
    out["work_counters_equal"] = len({work(r) for k in LEGS for r in out["runs"][k]}) == 1
    out["final_points_equal"] = len({r["x_sha1"] for k in LEGS for r in out["runs"][k]}) == 1
    print(json.dumps(out))


if __name__ == "__main__":
    main()
