"""What a rocprofv3 --kernel-trace of `python bench.py --steps 100 --warmup 10` says about the end of a C2 sweep:
python profiles/dev/early_count_trace.py <dir with *kernel_trace.csv> -> one JSON line: calls and average duration of the sweep's
kernels, and the idle time between one sweep's k_slot_emit and the next sweep's k_fx_acc<1> (end -> start), over the timed sweeps."""
import csv, glob, json, os, statistics, sys

f = sorted(glob.glob(os.path.join(sys.argv[1], "**", "*kernel_trace.csv"), recursive=True))[0]
rows = [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(open(f))]
rows.sort()


def short(n):
    for k in ("k_fx_acc<1", "k_fx_acc<(int)1", "k_fx_nodes<1", "k_fx_nodes<(int)1", "k_slot_emit", "k_ex_ticket"):
        if k in n:
            return k.replace("(int)", "")
    return None


dur, gaps, period, last_emit_end, last_acc_start = {}, [], [], None, None
for s, e, n in rows:
    k = short(n)
    if k is None:
        continue
    dur.setdefault(k, []).append(e - s)
    if k == "k_slot_emit":
        last_emit_end = e
    if k == "k_fx_acc<1":
        if last_emit_end is not None:
            gaps.append(s - last_emit_end)
        if last_acc_start is not None:
            period.append(s - last_acc_start)
        last_acc_start, last_emit_end = s, None
skip = 12  # the warm-up sweeps (and the first timed ones)
out = {"kernels": {k: dict(calls=len(v), avg_us=round(statistics.mean(v[skip:] or v) / 1e3, 2)) for k, v in sorted(dur.items())},
       "idle_slot_emit_to_next_fx_acc_us": dict(n=len(gaps[skip:]), median=round(statistics.median(gaps[skip:]) / 1e3, 2),
                                                mean=round(statistics.mean(gaps[skip:]) / 1e3, 2), min=round(min(gaps[skip:]) / 1e3, 2)),
       "period_fx_acc_to_fx_acc_us": dict(median=round(statistics.median(period[skip:]) / 1e3, 2))}
print(json.dumps(out))
