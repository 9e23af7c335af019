#!/usr/bin/env python3
"""Serial seat against batched seat on one structure: 64 host models, one QP each.

The requests are the first sub-problem of run! for `count` contingency scenarios of a synthetic network (QP mode at the
scenario's start point, zero multipliers, the default radius), evaluated once by the device callbacks.  Two legs:

    scalar   `count` calls of sqphip_qp_solve, scenario k on a one-instance context that carries its bounds
    batch    one call of sqphip_qp_solve_batch on a context of `count` instances (instance k: the bounds of scenario k)

Each leg is a process of its own under `timeout -k 10` (the parent never opens the GPU and stops at the first leg that
fails); it warms up, then times five windows with a host clock around calls that end in a stream synchronise, and
reports the median as one JSON line: QP/s, seconds per window, interior-point iterations (equal work on both legs).
Both legs call the C ABI directly, with every pointer prepared before the clock starts.

    python scripts/seat_batch_timing.py --out seat_batch.json                    # both legs, this build
    python scripts/seat_batch_timing.py --legs scalar --so /path/to/libsqphip.so --label parent --out seat_batch.json

--so runs a leg against another build of the library (the serial leg at the parent commit); lines are appended to --out.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIMITS = {"scalar": 420, "batch": 240}          # seconds per leg (context creation included)


def scenarios(case, count):
    from sqpsolver_jl_amd.acopf_synth import acopf_synth, acopf_layout, contingency, CASES
    nb, ng, nl, seed = CASES[case]
    net = acopf_synth(nb, ng, nl, seed)
    nets = [contingency(net, s + 1, 11) for s in range(count)]
    return net, acopf_layout(net), nets, [acopf_layout(nk) for nk in nets]


def requests(pkg, net, lay, nets, lays):
    """(x_k, df, E, jval, hval) per scenario at its start point, from the device callbacks"""
    import numpy as np
    ev = pkg.Context(lay.n, lay.m, lay.num_linear, lay.jrow, lay.jcol, lay.hrow, lay.hcol, lay.xL, lay.xU, lay.gL, lay.gU,
                     pkg.default_options(), batch=len(nets))
    ev.acopf_attach(net, lay)
    out = []
    for k, (nk, lk) in enumerate(zip(nets, lays)):
        ev.acopf_set_instance(k, nk, lk)
        r = ev.acopf_eval(k, lk.x0, 1.0, np.zeros(lay.m))
        out.append((np.ascontiguousarray(lk.x0, dtype=np.float64), r["grad"], r["g"], r["jval"], r["hval"]))
    ev.close()
    return out


def leg(args):
    import numpy as np
    import sqpsolver_jl_amd as pkg
    from sqpsolver_jl_amd import _lib
    from sqpsolver_jl_amd.host import _d, _i
    net, lay, nets, lays = scenarios(args.case, args.count)
    reqs = requests(pkg, net, lay, nets, lays)
    cnt, n, m = args.count, lay.n, lay.m
    delta, mu = float(pkg.default_options().tr_size), 1.0
    L = _lib.lib()
    mk = lambda bounds, batch: pkg.Context(lay.n, lay.m, lay.num_linear, lay.jrow, lay.jcol, lay.hrow, lay.hcol, bounds.xL,
                                           bounds.xU, bounds.gL, bounds.gU, pkg.default_options(), batch=batch)
    p = np.zeros((cnt, n)); lam = np.zeros((cnt, m)); mu_u = np.zeros((cnt, n)); mu_l = np.zeros((cnt, n))
    slack = np.zeros((cnt, 2 * m)); st = np.zeros(cnt, dtype=np.int32)
    if args.leg == "scalar":
        ctxs = [mk(lk, 1) for lk in lays]
        it = C.c_int32(); nf = C.c_int32()
        calls = [(c.h, 0, _d(r[0]), delta, mu, _d(r[1]), _d(r[2]), _d(r[3]), _d(r[4]), _d(p[k]), _d(lam[k]), _d(mu_u[k]),
                  _d(mu_l[k]), _d(slack[k]), _i(st[k:k + 1])) for k, (c, r) in enumerate(zip(ctxs, reqs))]

        def window():
            for a in calls:
                if L.sqphip_qp_solve(*a) != 0:
                    raise RuntimeError("sqphip_qp_solve failed")
        inner, iters = 1, 0
        window()
        for c in ctxs:
            L.sqphip_qp_stats(c.h, C.byref(it), C.byref(nf)); iters += it.value
    else:
        ctx = mk(lay, cnt)
        for k, lk in enumerate(lays):
            ctx.set_bounds(k, lk)
        col = lambda j: np.ascontiguousarray(np.stack([r[j] for r in reqs]))
        xk, df, E, jv, hv = (col(j) for j in range(5))
        inst = np.arange(cnt, dtype=np.int32); mode = np.zeros(cnt, dtype=np.int32)
        dl = np.full(cnt, delta); pen = np.full(cnt, mu)
        a = (ctx.h, cnt, _i(inst), _i(mode), _d(xk), _d(dl), _d(pen), _d(df), _d(E), _d(jv), _d(hv), _d(p), _d(lam), _d(mu_u),
             _d(mu_l), _d(slack), _i(st))

        def window():
            for _ in range(inner):
                if L.sqphip_qp_solve_batch(*a) != 0:
                    raise RuntimeError("sqphip_qp_solve_batch failed")
        inner = args.inner
        window()
        iters = sum(s["ipm_iters"] for s in ctx.qp_stats_batch(inst))
    window()                                     # second warm-up pass: every shape of the timed windows has run
    secs = []
    for _ in range(5):
        t0 = time.perf_counter(); window(); secs.append(time.perf_counter() - t0)
    med = statistics.median(secs)
    print(json.dumps(dict(leg=args.leg, label=args.label, case=args.case, count=cnt, n=n, m=m, calls_per_window=inner * (cnt if args.leg == "scalar" else 1),
                          qps_per_window=inner * cnt, seconds_median=med, seconds=secs, qp_per_s=inner * cnt / med,
                          ms_per_qp=1e3 * med / (inner * cnt), ipm_iters_total=int(iters), solved=int((st == 4).sum()))),
          flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--case", default="case118")
    ap.add_argument("--count", type=int, default=64)
    ap.add_argument("--inner", type=int, default=10, help="batch calls per timed window")
    ap.add_argument("--legs", default="scalar,batch")
    ap.add_argument("--label", default="this build")
    ap.add_argument("--so", default=None, help="another build of libsqphip.so for the legs (SQPHIP_SO)")
    ap.add_argument("--out", default=None, help="append the result lines to this file")
    ap.add_argument("--leg", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.leg:
        return leg(args)
    env = dict(os.environ)
    if args.so:
        env["SQPHIP_SO"] = os.path.abspath(args.so)
    for name in args.legs.split(","):
        cmd = ["timeout", "-k", "10", str(LIMITS[name]), sys.executable, os.path.abspath(__file__), "--leg", name, "--case", args.case,
               "--count", str(args.count), "--inner", str(args.inner), "--label", args.label]
        r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(r.stdout)
        if r.returncode != 0:
            print(f"leg {name} ended with status {r.returncode}: nothing more is started", file=sys.stderr)
            return r.returncode
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(r.stdout.strip().splitlines()[-1] + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
