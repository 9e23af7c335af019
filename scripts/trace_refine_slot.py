"""Share of the refinement slot's launches and of k_sqp_count in the chain of every hardware queue (kernel trace of rocprofv3).
usage: trace_refine_slot.py <dir with *_kernel_trace.csv>"""
import csv, glob, sys, collections
f = glob.glob(sys.argv[1] + "/**/*_kernel_trace.csv", recursive=True)[0]
rows = [r for r in csv.DictReader(open(f)) if "sqphip" in r["Kernel_Name"]]
byq = collections.defaultdict(list)
for r in rows:
    byq[r["Queue_Id"]].append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
tot = collections.Counter()
for q, seq in sorted(byq.items()):
    seq.sort()
    if len(seq) < 1000:
        continue
    span = seq[-1][1] - seq[0][0]
    busy = sum(e - s for s, e, _ in seq)
    cnt = sum(e - s for s, e, n in seq if "k_sqp_count" in n); ncnt = sum(1 for _, _, n in seq if "k_sqp_count" in n)
    gap_cnt = 0
    slot = 0; nslot = 0; slot_l = 0; in_slot = False; slot_wall = 0; t_in = 0
    nsweep = sum(1 for _, _, n in seq if "k_mf_values" in n)
    for i, (s, e, n) in enumerate(seq):
        if "k_ipm_post<3" in n or "k_ipm_post<(int)3" in n:
            in_slot = True; t_in = e; continue
        if "k_mf_values" in n or "k_qp_finish" in n: in_slot = False        # (the next sweep has begun: no slot, no counter launch)
        if "k_sqp_count" in n:
            if in_slot and seq[i - 1][2] != n and "k_ipm_post<6" in seq[i - 1][2].replace("(int)", ""):
                slot_wall += s - t_in; nslot += 1
            in_slot = False
            if i + 1 < len(seq): gap_cnt += max(0, seq[i + 1][0] - s)       # wall time from its start to the next kernel's start
            continue
        if in_slot:
            slot += e - s; slot_l += 1
    print(f"queue {q}: {len(seq)} launches, {nsweep} sweeps, span {span / 1e6:.1f} ms, busy {busy / 1e6:.1f} ms; "
          f"k_sqp_count {ncnt} x {cnt / max(1, ncnt) / 1e3:.1f} us = {100 * cnt / span:.2f} % of the span "
          f"({100 * gap_cnt / span:.2f} % with the boundary behind it); refinement slot in {nslot} sweeps ({100 * nslot / max(1, nsweep):.1f} %), "
          f"{slot_l} launches, {slot / 1e6:.2f} ms of kernel time = {100 * slot / span:.2f} %, {slot_wall / 1e6:.2f} ms of wall time = {100 * slot_wall / span:.2f} % of the span")
names = collections.defaultdict(lambda: [0, 0])
for r in rows:
    k = r["Kernel_Name"].split("(")[0].replace("void ", "").replace("sqphip::", "")
    names[k][0] += 1; names[k][1] += int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
T = sum(v[1] for v in names.values())
print("kernel, launches, total ms, avg us, % of kernel time")
for k, v in sorted(names.items(), key=lambda kv: -kv[1][1])[:45]:
    print(f"{k:44s} {v[0]:8d} {v[1] / 1e6:9.2f} {v[1] / v[0] / 1e3:8.1f} {100 * v[1] / T:6.2f}")
