#!/usr/bin/env python3
"""What passive tracers (beom_set_tracers) cost on one GPU, on the frames of tools/bench_case.py:

  python tools/tracer_cost.py headline|soliton [--reps 3] [--steps 40] [--parent ab/prev.so]      the alternated table
  python tools/tracer_cost.py CASE --one N [--steps 40]                                          one process, N tracers: a JSON line
  python tools/tracer_cost.py CASE --one 1 --pmc                                                 under rocprofv3 --pmc: a few steps

The table alternates fresh processes on one box (tools/ab.sh's way): the step with 0, 1, 2 and 4 tracers, and with --parent
the step without tracers of an older library (BEOM_HIP_LIB) next to this tree's.  Per configuration: the median step time
(wall clock over --steps steps, stream synced on both sides, three blocks per process) and, from HIP events around the
launches of sampled steps (beom_profile_steps), the tracer sweep and update_h per launch.  Compulsory traffic of the sweep:
3 + 5 * ntrc words per cell-layer (hlay, h_u, h_v; per tracer q and the two tendency levels read, q and the new tendency
written).  HBM bytes per launch come from a counter run of their own (--pmc, then tools/pmc_traffic.py)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ("headline", "soliton")
ap = argparse.ArgumentParser()
ap.add_argument("case", choices=CASES)
ap.add_argument("--one", type=int, default=None)
ap.add_argument("--steps", type=int, default=40)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--parent", default=None)
ap.add_argument("--pmc", action="store_true")
a = ap.parse_args()


def one():
    import numpy as np
    from beom_amd import capi, inputs as I
    from beom_amd.grid import read_input_data
    p, files = I.case_headline(4096, 4096, 4) if a.case == "headline" else I.case_soliton(lm=2048, mm=256, dt_s=60.0)
    f = read_input_data(p, files=files)
    e = capi.Engine(f)
    out = {"case": a.case, "lm": p.lm, "mm": p.mm, "nlay": p.nlay, "ntrc": a.one, "lib": os.environ.get("BEOM_HIP_LIB", "in-tree")}
    if a.one > 0:
        e.set_tracers(a.one)
        c = np.linspace(0.5, 1.5, a.one)[:, None, None] * np.ones((1,) + f.hlay.shape)
        e.set_concentration(c)
    e.step(1, 10)
    if a.pmc:
        e.step(11, 8)
        print(json.dumps(out)); return
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
    cl = p.ndeg * p.nlay
    out["compulsory_MB"] = {"update_h": round(cl * 7 * 8 / 1e6, 1), "tracers": round(cl * (3 + 5 * a.one) * 8 / 1e6, 1) if a.one else 0.0}
    if a.one > 0:
        q = e.download_tracers()["q"]
        out["finite"] = bool(np.isfinite(q).all())
    print(json.dumps(out))
    e.close()


def table():
    configs = [("tree", n) for n in (0, 1, 2, 4)]
    if a.parent:
        configs.insert(0, ("parent", 0))
    rows = {c: [] for c in configs}
    for rep in range(a.reps):
        for c in configs:
            env = dict(os.environ)
            env.pop("BEOM_HIP_LIB", None)
            if c[0] == "parent":
                env["BEOM_HIP_LIB"] = os.path.abspath(a.parent)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), a.case, "--one", str(c[1]), "--steps", str(a.steps)],
                               env=env, capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                sys.exit("configuration %s failed (rc %d):\n%s\n%s" % (c, r.returncode, r.stdout[-2000:], r.stderr[-2000:]))
            rec = json.loads(r.stdout.strip().splitlines()[-1])
            rows[c].append(rec)
            print("# rep %d %-6s ntrc %d: %s" % (rep, c[0], c[1], json.dumps(rec)), flush=True)
    base = statistics.median(x["step_us"] for x in rows[("tree", 0)])
    print("%s: %d repetitions alternated, %d steps per block" % (a.case, a.reps, a.steps))
    print("%-8s %4s %12s %10s %14s %14s %12s" % ("library", "ntrc", "step us", "vs 0", "sweep us", "update_h us", "sweep MB"))
    for c in configs:
        st = statistics.median(x["step_us"] for x in rows[c])
        sw = [x["per_launch_us"].get("tracers") for x in rows[c] if x["per_launch_us"].get("tracers") is not None]
        uh = statistics.median(x["per_launch_us"]["h"] for x in rows[c])
        print("%-8s %4d %12.1f %+9.2f%% %14s %14.1f %12.1f" % (c[0], c[1], st, (st / base - 1) * 100,
                                                             "%.1f" % statistics.median(sw) if sw else "-", uh,
                                                             rows[c][0]["compulsory_MB"]["tracers"]))


if a.one is not None:
    one()
else:
    table()
