"""Average duration of every launch position of a sweep (kernel trace of rocprofv3): which level launches are slow.
usage: trace_by_position.py <dir with *_kernel_trace.csv> [first cycle] [last cycle] [kernel a cycle starts with] [forms shown]
A cycle starts at every launch of the given kernel: k_qp_finish by default (one transition period of a run with the transition
kernels in line), k_mf_values for one sweep (with the transitions in line the three kernels then close every fourth sweep).
Cycles are told apart by their sequence of kernels -- a sweep that serves a refinement request carries three forward launches --
and the most frequent forms are printed, one table each (default: the most frequent one only)."""
import csv, glob, sys, collections
f = glob.glob(sys.argv[1] + "/**/*_kernel_trace.csv", recursive=True)[0]
lo = int(sys.argv[2]) if len(sys.argv) > 2 else 60
hi = int(sys.argv[3]) if len(sys.argv) > 3 else 160
first = sys.argv[4] if len(sys.argv) > 4 else "k_qp_finish"
forms = int(sys.argv[5]) if len(sys.argv) > 5 else 1


def short(r):
    return r["Kernel_Name"].replace("sqphip::", "").replace("void ", "").split("(")[0][:30]


def us(r):
    return (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3


rows = list(csv.DictReader(open(f)))
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
idx = [i for i, r in enumerate(rows) if first in r["Kernel_Name"]]
cycles = [rows[a:b] for a, b in zip(idx[lo:hi], idx[lo + 1:hi + 1])]
by_form = collections.defaultdict(list)
for seq in cycles:
    by_form[tuple(short(r) for r in seq)].append(seq)
print(f"{len(cycles)} cycles from {first}: {sum(len(s) for s in cycles) / max(1, len(cycles)):.2f} launches and "
      f"{sum(us(r) for s in cycles for r in s) / max(1, len(cycles)):.1f} us of kernel time per cycle, {len(by_form)} forms")
for form, seqs in sorted(by_form.items(), key=lambda kv: -len(kv[1]))[:forms]:
    print(f"{len(seqs)} cycles of {len(form)} launches")
    tot = 0
    for k, name in enumerate(form):
        d = [us(s[k]) for s in seqs]; r = seqs[0][k]; tot += sum(d) / len(d)
        print(f"{k:3d} {sum(d) / len(d):7.1f} us  (max {max(d):7.1f})  {name:32s} {r['Grid_Size_X']}x{r['Grid_Size_Y']}/{r['Workgroup_Size_X']}")
    print("sum", round(tot, 1), "us")
