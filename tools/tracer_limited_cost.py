#!/usr/bin/env python3
"""What the two tracer schemes (beom_set_tracer_scheme) cost on one GPU, at 4096 x 4096 x 4 (tools/tracer_cost.py's headline):

  python tools/tracer_limited_cost.py [--reps 3] [--steps 40] [--parent ab/prev.so]      the alternated table
  python tools/tracer_limited_cost.py --one N --scheme S [--steps 40]                     one process: a JSON line
  rocprofv3 --kernel-trace --stats -d DIR -- python tools/tracer_limited_cost.py --one N --scheme S --trace
                                                                                          a few steps, for the launches' own times

The table alternates fresh processes on one box (tools/tracer_cost.py's way): the step without tracers on this tree's library
and, with --parent, on an older one (BEOM_HIP_LIB); 1 and 4 tracers under scheme 1; 1 and 4 tracers under scheme 2.  Per
configuration: the median step time (wall clock over --steps steps, stream synced on both sides, three blocks per process) and,
from HIP events around the launches of sampled steps (beom_profile_steps), the tracer sweep and update_h per launch.  Compulsory
traffic of either sweep: 3 + 5 * ntrc words per cell-layer."""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--one", type=int, default=None)
ap.add_argument("--scheme", type=int, default=1, choices=(1, 2))
ap.add_argument("--steps", type=int, default=40)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--parent", default=None)
ap.add_argument("--trace", action="store_true")
ap.add_argument("--size", type=int, nargs=3, default=(4096, 4096, 4), metavar=("LM", "MM", "NLAY"))
a = ap.parse_args()


def one():
    import numpy as np
    from beom_amd import capi, inputs as I
    from beom_amd.grid import read_input_data
    p, files = I.case_headline(*a.size)
    f = read_input_data(p, files=files)
    e = capi.Engine(f)
    out = {"lm": p.lm, "mm": p.mm, "nlay": p.nlay, "ntrc": a.one, "scheme": a.scheme, "lib": os.environ.get("BEOM_HIP_LIB", "in-tree")}
    if a.one > 0:
        e.set_tracer_scheme(a.scheme)
        e.set_tracers(a.one)
        i, j = f.subc[0].astype(np.float64), f.subc[1].astype(np.float64)
        wave = 1.0 + 0.3 * np.sin(0.9 * i) * np.cos(0.7 * j)             # (not flat: the limiter has work to do)
        c = np.linspace(0.5, 1.5, a.one)[:, None, None] * wave[None, None, :] * np.ones((1,) + f.hlay.shape)
        e.set_concentration(c)
    e.step(1, 10)
    if a.trace:
        e.step(11, 8)
        e.sync()
        print(json.dumps(out)); e.close(); return
    tstp, blocks = 11, []
    for _ in range(3):
        e.sync()
        t = time.perf_counter(); e.step(tstp, a.steps); blocks.append((time.perf_counter() - t) / a.steps * 1e6)
        tstp += a.steps
    out["step_us"] = round(statistics.median(blocks), 1)
    out["step_us_blocks"] = [round(b, 1) for b in blocks]
    ms, nl = e.profile_steps(tstp, 20)
    names = ("h", "mont", "visc", "u", "v", "mont+visc", "u+v", "tracers")
    out["per_launch_us"] = {names[k]: round(ms[k] / nl[k] * 1e3, 1) for k in range(len(nl)) if nl[k]}
    out["compulsory_MB"] = round(p.ndeg * p.nlay * (3 + 5 * a.one) * 8 / 1e6, 1) if a.one else 0.0
    if a.one > 0:
        out["finite"] = bool(np.isfinite(e.download_tracers()["q"]).all())
    print(json.dumps(out))
    e.close()


def traced(ntrc, scheme):
    """[ns, ...] of the tracer launches of a --trace process under rocprofv3 --kernel-trace --stats, or an error text."""
    d = tempfile.mkdtemp(prefix="tracer_trace_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
           "--one", str(ntrc), "--scheme", str(scheme), "--trace", "--size"] + [str(x) for x in a.size]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    except FileNotFoundError:
        return "rocprofv3 not found"
    except subprocess.TimeoutExpired:
        return "rocprofv3 run timed out"
    if r.returncode != 0:
        return "rocprofv3 failed (rc %d): %s" % (r.returncode, (r.stderr or r.stdout)[-400:].replace("\n", " | "))
    ns = []
    for fn in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        with open(fn) as fh:
            for row in csv.DictReader(fh):
                if "k_tracers" in row.get("Kernel_Name", ""):
                    ns.append(int(row["End_Timestamp"]) - int(row["Start_Timestamp"]))
    return ns or "no k_tracers launch in the trace"


def table():
    configs = [("tree", 0, 1), ("tree", 1, 1), ("tree", 4, 1), ("tree", 1, 2), ("tree", 4, 2)]
    if a.parent:
        configs.insert(0, ("parent", 0, 1))
    rows = {c: [] for c in configs}
    for rep in range(a.reps):
        for c in configs:
            env = dict(os.environ)
            env.pop("BEOM_HIP_LIB", None)
            if c[0] == "parent":
                env["BEOM_HIP_LIB"] = os.path.abspath(a.parent)
            cmd = [sys.executable, os.path.abspath(__file__), "--one", str(c[1]), "--scheme", str(c[2]), "--steps", str(a.steps),
                   "--size"] + [str(x) for x in a.size]
            r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                sys.exit("configuration %s failed (rc %d):\n%s\n%s" % (c, r.returncode, r.stdout[-2000:], r.stderr[-2000:]))
            rec = json.loads(r.stdout.strip().splitlines()[-1])
            rows[c].append(rec)
            print("# rep %d %-6s ntrc %d scheme %d: %s" % (rep, c[0], c[1], c[2], json.dumps(rec)), flush=True)
    base = statistics.median(x["step_us"] for x in rows[("tree", 0, 1)])
    print("%d x %d x %d: %d repetitions alternated, %d steps per block" % (tuple(a.size) + (a.reps, a.steps)))
    print("%-8s %4s %6s %12s %10s %14s %14s %12s" % ("library", "ntrc", "scheme", "step us", "vs 0", "sweep us", "update_h us", "sweep MB"))
    for c in configs:
        st = statistics.median(x["step_us"] for x in rows[c])
        sw = [x["per_launch_us"].get("tracers") for x in rows[c] if x["per_launch_us"].get("tracers") is not None]
        uh = statistics.median(x["per_launch_us"]["h"] for x in rows[c])
        print("%-8s %4d %6s %12.1f %+9.2f%% %14s %14.1f %12.1f" % (c[0], c[1], c[2] if c[1] else "-", st, (st / base - 1) * 100,
                                                                  "%.1f" % statistics.median(sw) if sw else "-", uh,
                                                                  rows[c][0]["compulsory_MB"]))
    print("The tracer launch under rocprofv3 --kernel-trace --stats (a process of its own per row; median of the launches of 18 steps):")
    for c in configs:
        if c[1] == 0:
            continue
        ns = traced(c[1], c[2])
        if isinstance(ns, str):                  # a child that failed may have faulted the card: nothing more is started on it
            sys.exit("  ntrc %d scheme %d: %s\nstopped: no further process is started after a failed one" % (c[1], c[2], ns))
        us, mb = statistics.median(ns) / 1e3, rows[c][0]["compulsory_MB"]
        print("  ntrc %d scheme %d: %8.1f us per launch (%d launches, min %.1f), %.1f MB compulsory = %.2f TB/s"
              % (c[1], c[2], us, len(ns), min(ns) / 1e3, mb, mb / us), flush=True)      # MB / us = TB/s


if a.one is not None:
    one()
else:
    table()
