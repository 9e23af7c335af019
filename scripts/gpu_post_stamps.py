"""Stamps of the post path (traced build, SQPHIP_TRACE_SO): python scripts/gpu_post_stamps.py CASE BATCH STEPS
Sums over every pass of workgroup 0 / thread 0 (one instance group: SQPHIP_GROUPS=1).  The traced library is every source of
_lib.SOURCES compiled with -DSQPHIP_MF_TRACE into one shared object, as scripts/gpu_mf_trace.py does it.  Segments named "entry"
run from the last stamp of one kernel or stage to the first of the next (other launches, other clocks): not durations."""
import ctypes as C, os, sys
import numpy as np
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
from sqpsolver_jl_amd import _lib
_lib.SO_PATH = os.path.abspath(os.environ["SQPHIP_TRACE_SO"])
import sqpsolver_jl_amd as pkg
from sqpsolver_jl_amd.acopf_synth import acopf_synth, acopf_layout, contingency, CASES
case, B, steps = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
nb, ng, nl, seed = CASES[case]
base = acopf_synth(nb, ng, nl, seed); lay0 = acopf_layout(base)
ctx = pkg.Context(lay0.n, lay0.m, lay0.num_linear, lay0.jrow, lay0.jcol, lay0.hrow, lay0.hcol, lay0.xL, lay0.xU, lay0.gL,
                  lay0.gU, pkg.default_options(kkt_mode=2, max_iter=3000, tol_infeas=1e-6, tol_residual=1e-4, use_soc=1), batch=B)
ctx.acopf_attach(base, lay0)
for b in range(B):
    net = base if b == 0 else contingency(base, b, seed)
    ctx.acopf_set_instance(b, net, acopf_layout(net))
ctx.sqp_reset(); ctx.sqp_run(steps)
c = ctx.counters()
L = _lib.lib()
buf = np.zeros(193, dtype=np.int64)
L.sqphip_vec_trace_sums.argtypes = [C.POINTER(C.c_longlong)]
assert L.sqphip_vec_trace_sums(buf.ctypes.data_as(C.POINTER(C.c_longlong))) == 0
s, n = buf[64:128], buf[128:192]
names = {1: "refine: accumulate (32|0 -> 1)", 2: "refine: stage/barrier (1 -> 2)", 3: "refine: residual loops + reduce (2 -> 3)",
         4: "refine: rare reload (3 -> 4)", 33: "refine[first]: accumulate", 34: "refine[first]: barrier", 35: "refine[first]: residual + reduce",
         36: "refine[first]: rare reload", 8: "step: entry (4|36 -> 8)", 9: "step: expand directions (8 -> 9)", 10: "step: 2 reductions (9 -> 10)",
         11: "step: update (10 -> 11)", 16: "prepare: entry (11 -> 16)", 17: "prepare: stage p, y (16 -> 17)", 19: "prepare: (17 -> 19)",
         20: "prepare: residual loops H p, J p, J'y (19 -> 20)", 21: "prepare: 7 reductions (20 -> 21)", 22: "prepare: rest (21 -> 22)",
         40: "rhs: entry (22 -> 40)", 41: "rhs: two element loops (40 -> 41)", 42: "rhs: block_reduce (41 -> 42)",
         43: "rhs: sol = 0 (42 -> 43)", 46: "rhs: terms, phase 1 (43 -> 46)", 47: "rhs: terms, barrier (46 -> 47)",
         44: "rhs: solve vector, thread 0 (43|47 -> 44)", 45: "rhs: to the closing barrier, whole workgroup (44 -> 45)"}
print(f"{case} B={B} steps={steps} XV_TERMS={os.environ.get('SQPHIP_XV_TERMS', 'default')}: n_qp {c['n_qp']} ipm {c['n_ipm_iter']} fac {c['n_factor']} sweeps {c['n_sweeps']}")
print("segment                                                      passes   cycles/pass")
for i in sorted(names):
    if n[i]:
        print(f"  {names[i]:58s} {int(n[i]):7d} {s[i] / n[i]:11.0f}")
sv = sum(s[i] / max(1, n[i]) for i in (46, 47, 44, 45))
print(f"  solve vector to the barrier (43 -> 45), cycles/pass: {sv:.0f}")
ctx.close()
