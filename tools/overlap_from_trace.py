#!/usr/bin/env python3
"""Where the timed region of a benched run spends its time, from a kernel trace.

Input: the kernel-trace CSV of the benched command, collected in a run of its own
(no counters with it):

    rocprofv3 --kernel-trace --output-format csv -d DIR -o NAME -- python bench.py --steps 64
    python tools/overlap_from_trace.py DIR/.../NAME_kernel_trace.csv --steps 64 --batch 8

Only three columns are read: Kernel_Name, Start_Timestamp, End_Timestamp (ns), and
Stream_Id or Queue_Id to tell the render streams apart.

A pass of the generation pipeline starts with wf_frame_init on its stream and holds
every dispatch of that stream up to the next wf_frame_init. A pass whose fused
launches count their work (wf_trace_fused's TALLY argument, the fourth) is a counted
frame, not a timed one. The timed region of a plain `python bench.py` is its last
steps / batch uncounted passes (--skip-last N leaves out N uncounted passes that follow
the timed region, as the serialized pass of a --full run).

Output, per frame of the timed region (the region's time / steps), over the window
from the region's first dispatch to its last:
  fused        at least one wf_trace_fused running (with or without a combine)
  combine_alone  a wf_combine_parents running and no wf_trace_fused
  both         a wf_combine_parents and a wf_trace_fused running (part of `fused`)
  other_only   only other kernels (wf_frame_init, the caller's own)
  idle         nothing running
and the share of the combine dispatches' own time (the sum of their durations) during
which a fused kernel runs. A dispatch's interval is what the trace records: from its
first wave's start to its last wave's end, so a launch that waits for room between
its blocks is `running` throughout.
"""
import argparse
import csv
import json
import re
import sys

FUSED, COMBINE, INIT, OTHER = "fused", "combine", "init", "other"


def classify(name):
    if "wf_trace_fused" in name:
        return FUSED
    if "wf_combine_parents" in name:
        return COMBINE
    if "wf_frame_init" in name:
        return INIT
    return OTHER


def is_counted(name):
    """wf_trace_fused<PRIMARY, QUADS, LANE, TALLY, ...>: TALLY set."""
    m = re.search(r"wf_trace_fused<([^>]*)>", name)
    if not m:
        return False
    args = [x.strip() for x in m.group(1).split(",")]
    return len(args) > 3 and args[3] in ("true", "1")


def read_trace(path):
    """[(stream key, class, counted, start, end)] in start order."""
    rows = []
    with open(path, newline="") as f:
        rd = csv.DictReader(f)
        cols = rd.fieldnames or []
        for need in ("Kernel_Name", "Start_Timestamp", "End_Timestamp"):
            if need not in cols:
                raise SystemExit(f"{path}: no {need} column (a rocprofv3 --kernel-trace CSV is expected)")
        recs = list(rd)
    # the render streams: Stream_Id where the trace has one that varies, else the hardware queue
    key = "Queue_Id" if "Queue_Id" in cols else None
    if "Stream_Id" in cols and len({r["Stream_Id"] for r in recs}) > 1:
        key = "Stream_Id"
    for r in recs:
        s, e = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
        if e < s:
            raise SystemExit(f"{path}: a dispatch ends before it starts")
        name = r["Kernel_Name"]
        rows.append((r[key] if key else "0", classify(name), is_counted(name), s, e))
    rows.sort(key=lambda t: (t[3], t[4]))
    return rows


def passes_of(rows):
    """The passes in order of their first dispatch: lists of rows, each from a wf_frame_init
    of its stream up to the next one of that stream."""
    open_pass, out = {}, []
    for r in rows:
        k = r[0]
        if r[1] == INIT:
            open_pass[k] = []
            out.append(open_pass[k])
        if k in open_pass:
            open_pass[k].append(r)
    return out


def sweep(intervals, t0, t1):
    """intervals: [(class, start, end)]. ns inside [t0, t1] by what runs."""
    ev = []
    for c, s, e in intervals:
        s, e = max(s, t0), min(e, t1)
        if e > s:
            ev.append((s, 1, c))
            ev.append((e, -1, c))
    ev.sort(key=lambda x: (x[0], x[1]))  # at one instant ends come before starts
    live = {FUSED: 0, COMBINE: 0, INIT: 0, OTHER: 0}
    acc = {"fused": 0, "combine_alone": 0, "both": 0, "other_only": 0, "idle": 0}
    t = t0
    for at, d, c in ev:
        dt = at - t
        if dt > 0:
            if live[FUSED]:
                acc["fused"] += dt
                if live[COMBINE]:
                    acc["both"] += dt
            elif live[COMBINE]:
                acc["combine_alone"] += dt
            elif live[INIT] or live[OTHER]:
                acc["other_only"] += dt
            else:
                acc["idle"] += dt
        t = at
        live[c] += d
    acc["idle"] += t1 - t
    return acc


def union(spans):
    out = []
    for s, e in sorted(spans):
        if out and s <= out[-1][1]:
            out[-1][1] = max(out[-1][1], e)
        else:
            out.append([s, e])
    return out


def covered(s, e, merged):
    """ns of [s, e] inside the merged (disjoint, sorted) spans."""
    return sum(max(0, min(e, b) - max(s, a)) for a, b in merged if a < e and b > s)


def analyse(rows, steps, batch, skip_last=0):
    timed = [p for p in passes_of(rows) if any(r[1] == FUSED for r in p) and not any(r[2] for r in p)]
    if skip_last:
        timed = timed[:-skip_last]
    n_pass = (steps + batch - 1) // batch
    if len(timed) < n_pass:
        raise SystemExit(f"the trace holds {len(timed)} uncounted passes, the timed region needs {n_pass}")
    timed = timed[-n_pass:]
    t0 = min(r[3] for p in timed for r in p)
    t1 = max(r[4] for p in timed for r in p)
    # everything that runs inside the window counts, whichever pass it belongs to
    inside = [(r[1], r[3], r[4]) for r in rows if r[4] > t0 and r[3] < t1]
    acc = sweep(inside, t0, t1)
    fused_u = union([(s, e) for c, s, e in inside if c == FUSED])
    comb = [(s, e) for p in timed for (_, c, _, s, e) in p if c == COMBINE]
    comb_ns = sum(e - s for s, e in comb)
    comb_over = sum(covered(s, e, fused_u) for s, e in comb)
    fused_ns = sum(e - s for p in timed for (_, c, _, s, e) in p if c == FUSED)
    per = lambda ns: ns / steps / 1e6  # noqa: E731  (ms per frame)
    return {
        "steps": steps, "batch": batch, "passes": n_pass,
        "streams": len({p[0][0] for p in timed}),
        "window_ms_per_frame": per(t1 - t0),
        "fused_ms_per_frame": per(acc["fused"]),
        "combine_alone_ms_per_frame": per(acc["combine_alone"]),
        "both_ms_per_frame": per(acc["both"]),
        "other_only_ms_per_frame": per(acc["other_only"]),
        "idle_ms_per_frame": per(acc["idle"]),
        "fused_dispatch_ms_per_frame": per(fused_ns),
        "combine_dispatch_ms_per_frame": per(comb_ns),
        "combine_overlapped_share": (comb_over / comb_ns) if comb_ns else 0.0,
    }


def report(r):
    lines = [
        f"timed region: {r['steps']} frames in {r['passes']} passes of {r['batch']} on {r['streams']} streams",
        f"  window                         {r['window_ms_per_frame']:.4f} ms/frame",
        f"  fused running                  {r['fused_ms_per_frame']:.4f}",
        f"    of it with a combine         {r['both_ms_per_frame']:.4f}",
        f"  combine running alone          {r['combine_alone_ms_per_frame']:.4f}",
        f"  other kernels only             {r['other_only_ms_per_frame']:.4f}",
        f"  nothing running                {r['idle_ms_per_frame']:.4f}",
        f"  sum of fused dispatches        {r['fused_dispatch_ms_per_frame']:.4f} ms/frame (overlapping launches add up)",
        f"  sum of combine dispatches      {r['combine_dispatch_ms_per_frame']:.4f}",
        f"  combine time under a fused kernel  {100.0 * r['combine_overlapped_share']:.1f} %",
    ]
    return "\n".join(lines)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("csv")
    ap.add_argument("--steps", type=int, default=64, help="frames of the timed region (bench.py --steps)")
    ap.add_argument("--batch", type=int, default=8, help="frames per pass (bench.py --batch)")
    ap.add_argument("--skip-last", type=int, default=0, help="uncounted passes after the timed region")
    ap.add_argument("--json", action="store_true", help="print the figures as one JSON line")
    a = ap.parse_args(argv)
    if a.steps < 1 or a.batch < 1:
        ap.error("--steps and --batch are positive")
    r = analyse(read_trace(a.csv), a.steps, a.batch, a.skip_last)
    print(json.dumps(r) if a.json else report(r))
    return 0


if __name__ == "__main__":
    sys.exit(main())
