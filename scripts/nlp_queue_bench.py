"""The scenario queue of a factorable-NLP context against the dedicated polar ACOPF queue on the bench workload of
`bench.py`: the 512 IEEE-118-shaped polar contingencies, restated as sums of products of univariate functions
(nlp_terms.from_polar_acopf), queued as 2 048 scenarios (scenario s is contingency s mod 512) and run to termination
through 512 slots -- once through sqphip_nlp_stream_begin / _set, once through sqphip_sqp_stream_begin / _set, with the same
structure and options.  Prints one JSON line: scenarios/s and QP/s of both queues, their work counters and the ratio.

    python scripts/nlp_queue_bench.py [--slots 512] [--scenarios 2048] [--literal-quirks 1] [--max-iter 20] [--out FILE]"""
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
    ap.add_argument("--slots", type=int, default=512)
    ap.add_argument("--scenarios", type=int, default=2048)
    ap.add_argument("--distinct", type=int, default=512, help="contingencies behind the scenarios (scenario s is contingency s mod this)")
    ap.add_argument("--literal-quirks", type=int, default=1)
    ap.add_argument("--max-iter", type=int, default=20, help="outer iterations per scenario (bench.py's screening record: 20 with literal_quirks 1, 60 with 0)")
    ap.add_argument("--out", default=None, help="also write the JSON to this file")
    args = ap.parse_args()
    nb, ng, nl, seed = CASES["case118"]
    base = synth_case("case118", None)
    D, M = min(args.distinct, args.scenarios), args.scenarios
    nets = [base if s == 0 else contingency(base, s, seed) for s in range(D)]
    lays = [acopf_layout(nt) for nt in nets]
    t0 = time.perf_counter()
    ps = [from_polar_acopf(nt, ly) for nt, ly in zip(nets, lays)]
    t_restate = time.perf_counter() - t0
    lay0 = lays[0]
    opts = dict(max_iter=args.max_iter, literal_quirks=args.literal_quirks, use_soc=1, tol_infeas=1e-6, tol_residual=1e-4)
    out = {"workload": f"{M} scenarios ({D} IEEE-118-shaped polar contingencies, scenario s = contingency s mod {D}) through {args.slots} slots",
           "scenarios": M, "slots": args.slots, "max_outer_iterations": args.max_iter, "literal_quirks": args.literal_quirks,
           "nlp_terms": {"terms": int(len(ps[0].trow)), "factors": int(len(ps[0].fvar))}, "restate_seconds": t_restate}
    for kind in ("polar", "nlp"):
        ctx = pkg.Context(lay0.n, lay0.m, lay0.num_linear, lay0.jrow, lay0.jcol, lay0.hrow, lay0.hcol, lay0.xL, lay0.xU,
                          lay0.gL, lay0.gU, pkg.default_options(**opts), batch=args.slots)
        t0 = time.perf_counter()
        if kind == "nlp":
            ctx.nlp_attach(ps[0])
            ctx.nlp_stream_begin(M)
            for s in range(M):
                ctx.nlp_stream_set(s, ps[s % D])
        else:
            ctx.acopf_attach(nets[0], lay0)
            ctx.stream_begin(M)
            for s in range(M):
                ctx.stream_set(s, nets[s % D], lays[s % D])
        t_fill = time.perf_counter() - t0
        torch.cuda.synchronize()
        ta = time.perf_counter()
        ctx.stream_run()
        torch.cuda.synchronize()
        tb = time.perf_counter()
        c = ctx.counters()
        res = [ctx.stream_get(s) for s in range(M)]
        st = np.array([r["status"] for r in res], dtype=np.int64); it = np.array([r["iter"] for r in res], dtype=np.int64)
        # a scenario's result does not depend on the slot: the copies of one contingency must have filed the same bits
        same = all(np.array_equal(res[s]["x"], res[s % D]["x"]) and res[s]["iter"] == res[s % D]["iter"] for s in range(D, M))
        out[kind] = {"seconds": tb - ta, "fill_seconds": t_fill, "scenarios_per_s": M / (tb - ta), "qp_per_s": c["n_qp"] / (tb - ta),
                     "n_qp": int(c["n_qp"]), "n_ipm_iter": int(c["n_ipm_iter"]), "n_factor": int(c["n_factor"]),
                     "converged_fraction": float(np.mean(st == 0)), "all_filed": bool((it >= 0).all()),
                     "copies_bit_identical": bool(same), "status_hash": int(np.sum(st * 31 + it))}
        ctx.close()
    out["ratio_nlp_over_polar_scenarios_per_s"] = out["nlp"]["scenarios_per_s"] / out["polar"]["scenarios_per_s"]
    out["ratio_nlp_over_polar_qp_per_s"] = out["nlp"]["qp_per_s"] / out["polar"]["qp_per_s"]
    out["same_work"] = all(out["nlp"][k] == out["polar"][k] for k in ("n_qp", "n_ipm_iter", "n_factor", "status_hash"))
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
