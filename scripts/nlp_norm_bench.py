"""The numbers of the Euclidean-norm row blocks (sqphip_nlp_add_norm_block, csrc/nlp_norm_dev.hpp) on one GPU.  Prints one JSON
line and, with --out, writes it to a file.  A first measurement, no threshold.

1. A seeded second-order-cone programme (nlp_terms.socp_synth: 16 variables, 16 group norms on the objective, cone rows of 3,
   70, 1, 64, 8 and 8 points) and a batch of norm_scenario instances as the instances of one context: QP/s of a run to
   termination, and seconds per evaluator call (sqphip_acopf_eval: one launch of k_acopf_eval_point and its copies, one workgroup
   on one CU) asked for the values alone (steps 1 - 5, the Armijo probe's path), with the first derivatives (steps 6 - 8 more) and
   for everything (the coefficients of chain 2 and step 9 more).
2. The segment-length sweep: one block of N points on d columns cut into outputs of L points, L = 2, 8, 32, 64, 65, 128 (the last
   output takes what is left of N), the targets cycling over the objective and three rows; the same three evaluator calls.  An
   output of at most NLP_NORM_SHORT = 64 points runs through the thread form (a thread per output, a thread per (output,
   column)), a longer one through the wave form.  A library built with -DNLP_NORM_SHORT=0 sends every output through the wave
   form: give it through SQPHIP_SO and say --form wave, and the two records side by side are the measurement the constant
   stands on.

Every timed section is preceded by an untimed call of the same kind and ends on a device synchronisation.

    python scripts/nlp_norm_bench.py [--runs 3] [--calls 20] [--batch 256] [--points 2048] [--columns 32] [--form thread]
                                     [--sweep-only] [--out FILE]"""
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
from sqpsolver_jl_amd.nlp_terms import POW, NlpNormBlock, make_nlp_terms, nlp_terms_layout, norm_scenario, socp_synth   # noqa: E402

OPTS = dict(max_iter=60, literal_quirks=0, tol_infeas=1e-8, tol_residual=1e-8)
SOCP_N, SOCP_LENS = 16, [16, 3, 70, 1, 64, 8, 8]
SWEEP = (2, 8, 32, 64, 65, 128)
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


def sweep_model(N, d, L, seed=5):
    """N points on d columns in outputs of L points (the last: what is left), targets cycling over rows 0, 1, 2, 3; a ridge"""
    rng = np.random.default_rng([seed, N, d])
    lens = [L] * (N // L) + ([N % L] if N % L else [])
    seg = np.concatenate([[0], np.cumsum(lens)])
    rows = [r % 4 for r in range(len(lens))]
    blk = NlpNormBlock(np.arange(1, d + 1), rng.standard_normal((N, d)) / np.sqrt(d), rows, seg, 1.0 + 0.3 * rng.standard_normal(N))
    terms = [(0, 0.5, [(j + 1, POW, 2)]) for j in range(d)]
    return make_nlp_terms(d, 3, 0, terms, xL=np.full(d, -3.0), xU=np.full(d, 3.0), gL=np.full(3, -np.inf), gU=np.full(3, 1e3),
                          x0=np.zeros(d), blocks=[blk]), lens


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--points", type=int, default=2048)
    ap.add_argument("--columns", type=int, default=32)
    ap.add_argument("--form", default="thread", help="what the library does with short outputs: thread (NLP_NORM_SHORT = 64) or wave (a build with 0)")
    ap.add_argument("--sweep-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    B, N, d = args.batch, args.points, args.columns
    out = {"what": "Euclidean-norm row blocks: scripts/nlp_norm_bench.py", "form_of_short_outputs": args.form, "batch": B, "runs": args.runs,
           "calls": args.calls}
    if not args.sweep_only:
        p = socp_synth(SOCP_N, SOCP_LENS, 3)
        lay = nlp_terms_layout(p)
        ctx = context(lay, B)
        ctx.nlp_attach(p)
        for b in range(B):
            ctx.nlp_set_instance(b, norm_scenario(p, b, 3, 0.1))
        x = 0.05 * np.random.default_rng(4).standard_normal(p.n)
        solve(ctx)                                                     # untimed
        runs = [solve(ctx) for _ in range(args.runs)]
        sec = {k: eval_seconds(ctx, x, args.calls, k) for k in ("values", "first", "all")}
        ctx.close()
        b0 = p.blocks[0]
        out["socp"] = {"n": SOCP_N, "segment_lengths": np.diff(b0.seg).tolist(), "rows": b0.rows.tolist(), "N": int(b0.A.shape[0]),
                       "d": int(b0.A.shape[1]), "runs": runs, "median_qp_per_s": float(np.median([r["qp_per_s"] for r in runs])),
                       "evaluator_seconds_per_call": sec}
    sweep = []
    for L in SWEEP:
        p, lens = sweep_model(N, d, L)
        lay = nlp_terms_layout(p)
        ctx = context(lay, 4)
        ctx.nlp_attach(p)
        x = 0.05 * np.random.default_rng(4).standard_normal(p.n)
        for k in ("values", "first", "all"):
            eval_seconds(ctx, x, 2, k)                                 # untimed
        best = {k: min(eval_seconds(ctx, x, args.calls, k) for _ in range(args.runs)) for k in ("values", "first", "all")}
        ctx.close()
        sweep.append({"segment_length": L, "outputs": len(lens), "last_output": lens[-1], "N": N, "d": d,
                      "evaluator_seconds_per_call_best_of_runs": best})
    out["sweep"] = sweep
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
