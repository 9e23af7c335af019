"""The numbers of the dense data blocks with several outputs (sqphip_nlp_add_row_block, csrc/nlp_rowblock_dev.hpp) on one GPU.
Prints one JSON line.

(a) The Neyman-Pearson model (nlp_terms.neyman_pearson_model: a SOFTPLUS block with outputs on the objective and on one
    row) on N = 8192 points with d = 64 features, `batch` bootstrap-like weight vectors: QP/s of a run to termination and
    seconds per evaluator call with and without the Hessian (sqphip_acopf_eval: one launch of k_acopf_eval_point and its copies).
(b) The Hessian pass against the number of outputs: the same design matrix with R = 1 (the objective alone) and R = 8 (the
    objective and seven rows); the difference of the two call times is the Hessian pass, which is one MFMA pass whatever R is.

Every timed section is preceded by an untimed call of the same kind and ends on a device synchronisation.

    python scripts/nlp_rowblock_bench.py [--runs 3] [--calls 20] [--batch 16] [--points 8192] [--features 64]"""
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
from sqpsolver_jl_amd.nlp_terms import POW, SOFTPLUS, NlpRowBlock, make_nlp_terms, neyman_pearson_model, nlp_terms_layout   # noqa: E402

OPTS = dict(max_iter=60, literal_quirks=0, tol_infeas=1e-8, tol_residual=1e-8, init_mu=1000.0)


def dataset(N, d, seed):
    rng = np.random.default_rng(seed)
    X = np.column_stack([np.ones(N), rng.standard_normal((N, d - 1))])
    w = rng.standard_normal(d)
    return X, (X @ (w / np.linalg.norm(w)) + 0.8 * rng.standard_normal(N) > 0).astype(float)


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
    lam = np.full(ctx.m, 0.5) if hessian else None
    ctx.acopf_eval(0, x, 1.0, lam)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(calls):
        ctx.acopf_eval(k % ctx.batch, x, 1.0, lam)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls


def outputs_model(X, R):
    """the design matrix under R outputs: the objective and rows 1 .. R - 1"""
    N, n = X.shape
    rng = np.random.default_rng(R)
    blk = NlpRowBlock(SOFTPLUS, np.arange(1, n + 1), X, list(range(R)), None, rng.uniform(0.0, 1.0, (R, N)) / N)
    terms = [(0, 0.25, [(j + 1, POW, 2)]) for j in range(n)]
    return make_nlp_terms(n, R - 1, 0, terms, xL=np.full(n, -50.0), xU=np.full(n, 50.0), gL=np.full(R - 1, -np.inf), gU=np.full(R - 1, 10.0),
                          x0=np.zeros(n), blocks=[blk])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--points", type=int, default=8192)
    ap.add_argument("--features", type=int, default=64)
    args = ap.parse_args()
    B, N, d = args.batch, args.points, args.features
    out = {"what": "dense data blocks with several outputs: scripts/nlp_rowblock_bench.py", "batch": B, "runs": args.runs,
           "calls": args.calls, "N": N, "d": d}
    X, y = dataset(N, d, 3)
    rng = np.random.default_rng(4)
    ps = [neyman_pearson_model(X, y, 0.3, 0.5, rng.integers(0, 3, N).astype(float)) for _ in range(B)]
    ctx = context(nlp_terms_layout(ps[0]), B)
    ctx.nlp_attach(ps[0])
    for b in range(B):
        ctx.nlp_set_instance(b, ps[b])
    x = 0.05 * rng.standard_normal(d)
    solve(ctx)                                                         # untimed
    runs = [solve(ctx) for _ in range(args.runs)]
    full, nohess = eval_seconds(ctx, x, args.calls, True), eval_seconds(ctx, x, args.calls, False)
    ctx.close()
    out["neyman_pearson"] = {"runs": runs, "median_qp_per_s": float(np.median([r["qp_per_s"] for r in runs])),
                             "evaluator_seconds_per_call": full, "evaluator_seconds_per_call_without_hessian": nohess}
    out["hessian_pass_by_outputs"] = []
    for R in (1, 8):
        p = outputs_model(X, R)
        ctx = context(nlp_terms_layout(p), B)
        ctx.nlp_attach(p)
        reps = [(eval_seconds(ctx, x, args.calls, True), eval_seconds(ctx, x, args.calls, False)) for _ in range(args.runs)]
        ctx.close()
        out["hessian_pass_by_outputs"].append({"R": R, "evaluator_seconds_per_call": [r[0] for r in reps],
                                               "evaluator_seconds_per_call_without_hessian": [r[1] for r in reps],
                                               "median_hessian_pass_seconds": float(np.median([r[0] - r[1] for r in reps]))})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
