#!/usr/bin/env python3
"""What a straddling swap pair costs the fused step with two chain groups, from a kernel trace.

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python3 bench.py --headline-only
    python3 tools/straddle_trace.py DIR/**/*kernel_trace.csv [--events-csv OUT.csv] [--json OUT.json]

The timed region of bench.py is one run() call: the longest run of k_step launches between two closing launches (commit workgroups
alone, a tiny grid).  Inside it a launch is ordinary (one chain group of the nominal size, on its group's queue), wide (more chains:
the joint launch over all chains, or a window's first launch, which carries one chain of the other group) or narrow (a window's second
launch).  An EVENT is a maximal run of launches of the first group's queue that are not ordinary.  For each event and each queue the
span from the end of the queue's last ordinary launch before it to the start of its first ordinary launch after it is set beside what
the same number of ordinary iterations take on that queue (the median start-to-start period, plus the median gap between two
consecutive launches); the event's overhead is the larger of the two queues'."""
import argparse
import csv
import json
import statistics as st
import sys


def col(row, *names):
    for n in names:
        if n in row and row[n] != "":
            return row[n]
    raise KeyError(names)


def load(path):
    out = []
    for r in csv.DictReader(open(path)):
        name = r["Kernel_Name"]
        name = name.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
        out.append({"name": name, "q": col(r, "Queue_Id"), "t0": int(col(r, "Start_Timestamp")), "t1": int(col(r, "End_Timestamp")),
                    "grid": int(col(r, "Grid_Size_X", "Grid_Size")), "vgpr": r.get("VGPR_Count", r.get("Arch_VGPR_Count", ""))})
    out.sort(key=lambda k: k["t0"])
    return out


def pct(v, p):
    v = sorted(v)
    return v[min(len(v) - 1, max(0, int(round(p * (len(v) - 1)))))]


def summary(v):
    return {"n": len(v), "mean": sum(v) / len(v), "median": st.median(v), "p10": pct(v, 0.1), "p90": pct(v, 0.9), "min": min(v), "max": max(v)} if v else {"n": 0}


def analyse(path):
    ks = load(path)
    res = {"kernel_averages_ns": {}}
    by = {}
    for k in ks:
        by.setdefault(k["name"], []).append(k["t1"] - k["t0"])
    for n, v in sorted(by.items(), key=lambda e: -sum(e[1])):
        res["kernel_averages_ns"][n] = {"calls": len(v), "average": sum(v) / len(v)}
    steps = [k for k in ks if "k_step<" in k["name"]]
    if not steps:
        raise SystemExit("no k_step launches in the trace")
    gmax = max(k["grid"] for k in steps)
    # segments between closing launches
    segs, cur = [], []
    for k in steps:
        if k["grid"] < 0.1 * gmax:
            if cur:
                segs.append(cur)
            cur = []
        else:
            cur.append(k)
    if cur:
        segs.append(cur)
    seg = max(segs, key=len)
    # the nominal group launch: the most frequent grid size (the swap pair's extra roles add 32 workgroups to one of the two groups)
    counts = {}
    for k in seg:
        counts[k["grid"]] = counts.get(k["grid"], 0) + 1
    nominal = max(counts, key=counts.get)
    kind = lambda k: 1 if k["grid"] > 1.03 * nominal else (-1 if k["grid"] < 0.97 * nominal else 0)  # wide | narrow | ordinary
    wide = lambda k: kind(k) > 0
    queues = sorted({k["q"] for k in seg}, key=lambda q: -sum(1 for k in seg if k["q"] == q))[:2]
    q1 = max(queues, key=lambda q: sum(1 for k in seg if k["q"] == q and wide(k)))  # the first group's queue: it carries the wide launches
    queues = [q1] + [q for q in queues if q != q1]
    res["grid_sizes"] = {str(g): n for g, n in sorted(counts.items())}
    res["launches_in_region"] = len(seg)
    res["region_us"] = (max(k["t1"] for k in seg) - seg[0]["t0"]) / 1e3
    res["wide_launches"] = sum(1 for k in seg if wide(k))
    res["narrow_launches"] = sum(1 for k in seg if kind(k) < 0)
    res["joint_launches"] = sum(1 for k in seg if k["grid"] > 1.6 * nominal)
    perq = {q: [k for k in seg if k["q"] == q] for q in queues}
    period, gap, dur = {}, {}, {}
    for q, v in perq.items():
        pp, gg = [], []
        for a, b in zip(v, v[1:]):
            if kind(a) == 0 and kind(b) == 0:
                pp.append(b["t0"] - a["t0"])
                gg.append(b["t0"] - a["t1"])
        dd = [k["t1"] - k["t0"] for k in v if kind(k) == 0]
        period[q], gap[q], dur[q] = st.median(pp), st.median(gg), st.median(dd)
    res["ordinary"] = {q: {"period_us": period[q] / 1e3, "gap_us": gap[q] / 1e3, "duration_us": dur[q] / 1e3, "launches": len(perq[q])} for q in queues}

    def runs(v):  # maximal runs of launches that are not ordinary, as (first index, last index)
        out, i = [], 0
        while i < len(v):
            if kind(v[i]) == 0:
                i += 1
                continue
            j = i
            while j + 1 < len(v) and kind(v[j + 1]) != 0:
                j += 1
            out.append((i, j))
            i = j + 1
        return out

    q2 = queues[1] if len(queues) > 1 else None
    runs2 = runs(perq[q2]) if q2 else []
    events = []
    for i, j in runs(perq[q1]):
        v = perq[q1]
        if i == 0 or j + 1 >= len(v):
            continue
        w = v[i:j + 1]
        n_it = len(w)
        ev = {"t_us": (w[0]["t0"] - seg[0]["t0"]) / 1e3, "iterations": n_it, "launch_us": [(k["t1"] - k["t0"]) / 1e3 for k in w],
              "between_us": [(y["t0"] - x["t1"]) / 1e3 for x, y in zip(w, w[1:])]}

        def fill(q, before, first, last, after):
            ev[f"gap_in_{q}_us"] = (first["t0"] - before["t1"]) / 1e3
            ev[f"gap_out_{q}_us"] = (after["t0"] - last["t1"]) / 1e3
            ev[f"span_{q}_us"] = (after["t0"] - before["t1"]) / 1e3
            ev[f"ordinary_{q}_us"] = (n_it * period[q] + gap[q]) / 1e3
            ev[f"overhead_{q}_us"] = ev[f"span_{q}_us"] - ev[f"ordinary_{q}_us"]
        fill(q1, v[i - 1], w[0], w[-1], v[j + 1])
        ok = True
        if q2:
            u = perq[q2]
            lo, hi = v[i - 1]["t0"] - 1.5 * period[q1], v[j + 1]["t1"] + 1.5 * period[q1]
            mine = [(x, y) for x, y in runs2 if u[x]["t0"] >= lo and u[y]["t1"] <= hi]
            if mine and mine[0][0] > 0 and mine[-1][1] + 1 < len(u):  # the second group's own (narrow) launches of this event
                x, y = mine[0][0], mine[-1][1]
                ev["launch2_us"] = [(k["t1"] - k["t0"]) / 1e3 for k in u[x:y + 1] if kind(k) != 0]
                fill(q2, u[x - 1], u[x], u[y], u[y + 1])
            else:  # it has none: the joint launches stand in its stream's way
                before = [k for k in u if k["t0"] < w[0]["t0"]]
                after = [k for k in u if k["t0"] > w[-1]["t0"]]
                if before and after:
                    fill(q2, before[-1], w[0], w[-1], after[0])
                else:
                    ok = False
        if ok:
            ev["overhead_us"] = max(ev[f"overhead_{q}_us"] for q in queues)
            events.append(ev)
    res["events"] = len(events)
    res["queues"] = queues
    keys = ["overhead_us"] + [f"{k}_{q}_us" for q in queues for k in ("span", "ordinary", "overhead", "gap_in", "gap_out")]
    res["per_event"] = {k: summary([e[k] for e in events]) for k in keys}
    res["per_event"]["launch_us"] = summary([d for e in events for d in e["launch_us"]])
    res["per_event"]["launch2_us"] = summary([d for e in events for d in e.get("launch2_us", [])])
    res["per_event"]["between_us"] = summary([d for e in events for d in e["between_us"]])
    res["per_event"]["iterations"] = summary([e["iterations"] for e in events])
    res["total_overhead_us"] = sum(e["overhead_us"] for e in events)
    # (every iteration has a launch on the first group's queue: its group's, a window's or the joint one)
    iters = max(len(perq[q]) for q in queues)
    res["iterations_seen"] = iters
    res["launches_per_iteration"] = len(seg) / iters
    res["region_minus_ordinary_us"] = res["region_us"] - iters * max(period.values()) / 1e3
    return res, events


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("trace")
    ap.add_argument("--events-csv", default="")
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    res, events = analyse(a.trace)
    if a.events_csv and events:
        keys = [k for k in events[0] if not isinstance(events[0][k], list)]
        with open(a.events_csv, "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(keys + ["launch_us", "launch2_us", "between_us"])
            for e in events:
                w.writerow([f"{e[k]:.3f}" if isinstance(e[k], float) else e[k] for k in keys] +
                           [" ".join(f"{d:.2f}" for d in e.get(c, [])) for c in ("launch_us", "launch2_us", "between_us")])
    if a.json:
        json.dump(res, open(a.json, "w"), indent=1)
    json.dump(res, sys.stdout, indent=1)
    print()


if __name__ == "__main__":
    main()
