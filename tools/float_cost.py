#!/usr/bin/env python3
"""What Lagrangian floats (beom_set_floats) cost on one GPU, at 4096 x 4096 x 4 (the headline frame of tools/bench_case.py):

  python tools/float_cost.py [--reps 3] [--steps 40] --parent ab/prev.so [--out profiles/float_cost.txt]      the alternated table
  python tools/float_cost.py --one [--steps 40]                                                              one process: a JSON line

The table alternates fresh processes on one box (tools/ab.sh's way): the parent commit's library (BEOM_HIP_LIB) and this
tree's, each stepping WITHOUT floats; the tree's process then carries 2^20 and 2^24 floats, seeded in row order (float k next
to float k+1 in the frame: the gathers of a wavefront fall into few cache lines) and in shuffled order (the same floats,
permuted: every lane somewhere else).  Per configuration: the median step time (wall clock over --steps steps per call, stream
synced on both sides, three blocks), and the time of one float launch (stage 1 and stage 2 alone through beom_update_floats,
20 launches each between two syncs).  The step time of a run drifts with the step number (the state evolves), so every
configuration with floats is timed between two blocks without floats in the same process and compared with their mean.
A call of K steps makes K + 1 float launches, each stage 2 + stage 1 but the two ends.
With 0 floats the tree's step has to lie within the parent's own max - min over the alternations; the float figures are
reported as they come."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--one", action="store_true")
ap.add_argument("--steps", type=int, default=40)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--parent", default=None)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "float_cost.txt"))
ap.add_argument("--frame", type=int, nargs=3, default=(4096, 4096, 4), metavar=("LM", "MM", "NLAY"))
a = ap.parse_args()
COUNTS = (1 << 20, 1 << 24)


def lattice(n, lm, mm, nlay):
    """n floats on a regular lattice of cell centres in row order (x fastest), the layer changing from row to row."""
    import numpy as np
    nx = 1
    while nx * nx < n:
        nx *= 2
    ny = n // nx
    k = np.arange(n, dtype=np.int64)
    x = (k % nx) * (lm / nx) + 0.5
    y = (k // nx) * (mm / ny) + 0.5
    return x, y, (1 + (k // nx) % nlay).astype(np.int32)


def one():
    import numpy as np
    from beom_amd import capi, inputs as I
    from beom_amd.grid import read_input_data
    lm, mm, nlay = a.frame
    p, files = I.case_headline(lm, mm, nlay)
    e = capi.Engine(read_input_data(p, files=files))
    has_floats = hasattr(e.lib, "beom_set_floats")
    out = {"lm": lm, "mm": mm, "nlay": nlay, "lib": "BEOM_HIP_LIB" if os.environ.get("BEOM_HIP_LIB") else "in-tree", "configs": {}}
    tstp = [1]

    def steps():
        e.step(tstp[0], 10); tstp[0] += 10
        blocks = []
        for _ in range(3):
            e.sync()
            t = time.perf_counter(); e.step(tstp[0], a.steps); blocks.append((time.perf_counter() - t) / a.steps * 1e6)
            tstp[0] += a.steps
        return {"step_us": round(statistics.median(blocks), 1), "step_us_blocks": [round(b, 1) for b in blocks], "last_step": tstp[0] - 1}

    before = out["configs"]["0"] = steps()
    if has_floats:
        rng = np.random.default_rng(3)
        for n in COUNTS:
            x, y, layer = lattice(n, lm, mm, nlay)
            perm = rng.permutation(n)
            for order, idx in (("rows", None), ("shuffled", perm)):
                xs, ys, ls = (x, y, layer) if idx is None else (x[idx], y[idx], layer[idx])
                e.set_floats(xs, ys, ls)
                rec = steps()
                rec["step_us_without_before"] = before["step_us"]
                for stage in (1, 2):
                    e.update_floats(stage); e.sync()
                    t = time.perf_counter()
                    for _ in range(20):
                        e.update_floats(stage)
                    e.sync()
                    rec["stage%d_us" % stage] = round((time.perf_counter() - t) / 20 * 1e6, 1)
                fl = e.download_floats()
                rec["finite"] = bool(np.isfinite(fl["x"]).all() and np.isfinite(fl["y"]).all())
                rec["rejected_steps"] = int(fl["rejected"].sum())
                rec["mean_displacement_cells"] = float(np.mean(np.hypot(fl["x"] - xs, fl["y"] - ys)))
                e.set_floats([], [], [])
                before = steps()
                rec["step_us_without_after"] = before["step_us"]
                out["configs"]["%d %s" % (n, order)] = rec
        out["configs"]["0 again"] = before
    print(json.dumps(out))
    e.close()


def table():
    if not a.parent:
        sys.exit("--parent LIB: the parent commit's libbeom_hip.so is needed for the alternation")
    runs = {"parent": [], "tree": []}
    log = []
    for rep in range(a.reps):
        for who in (("parent", "tree") if rep % 2 == 0 else ("tree", "parent")):      # (ABBA: neither library always runs second)
            env = dict(os.environ)
            env.pop("BEOM_HIP_LIB", None)
            if who == "parent":
                env["BEOM_HIP_LIB"] = os.path.abspath(a.parent)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", "--steps", str(a.steps), "--frame"] + [str(v) for v in a.frame],
                               env=env, capture_output=True, text=True, timeout=1500)
            if r.returncode != 0:
                sys.exit("%s failed (rc %d):\n%s\n%s" % (who, r.returncode, r.stdout[-2000:], r.stderr[-2000:]))
            rec = json.loads(r.stdout.strip().splitlines()[-1])
            runs[who].append(rec)
            log.append("# rep %d %-6s %s" % (rep, who, json.dumps(rec)))
            print(log[-1], flush=True)
    lm, mm, nlay = a.frame
    L = ["Lagrangian floats (k_floats, beom_floats.h): cost at %d x %d x %d            tools/float_cost.py" % (lm, mm, nlay), "",
         "%d alternations of two fresh processes (parent's library through BEOM_HIP_LIB and this tree's, the order swapped every time), %d steps per timed call,"
         % (a.reps, a.steps), "three calls per configuration, the median of the three; us per step (wall clock, stream synced).", ""]
    par = [r["configs"]["0"]["step_us"] for r in runs["parent"]]
    tre = [r["configs"]["0"]["step_us"] for r in runs["tree"]]
    L.append("0 floats   parent per alternation: %s   max - min %.1f" % (par, max(par) - min(par)))
    L.append("0 floats   tree   per alternation: %s   median %.1f against the parent's median %.1f (%+.2f %%)"
             % (tre, statistics.median(tre), statistics.median(par), (statistics.median(tre) / statistics.median(par) - 1) * 100))
    spread = max(par) - min(par)
    ok = abs(statistics.median(tre) - statistics.median(par)) <= spread
    L.append("condition (the tree's step with 0 floats within the parent's own max - min): %s" % ("met" if ok else "NOT met"))
    again = [r["configs"]["0 again"]["step_us"] for r in runs["tree"]]
    L.append("0 floats   tree, at the end of the process (step %d; the first figure ends at step %d): %s"
             % (runs["tree"][0]["configs"]["0 again"]["last_step"], runs["tree"][0]["configs"]["0"]["last_step"], again))
    L.append("")
    L.append("%-18s %12s %12s %12s %14s %14s %12s" % ("floats, seeding", "step us", "without us", "vs 0 us", "stage 1 us", "stage 2 us", "ns / float"))
    for n in COUNTS:
        for order in ("rows", "shuffled"):
            k = "%d %s" % (n, order)
            st = statistics.median(r["configs"][k]["step_us"] for r in runs["tree"])
            base = statistics.median(0.5 * (r["configs"][k]["step_us_without_before"] + r["configs"][k]["step_us_without_after"]) for r in runs["tree"])
            s1 = statistics.median(r["configs"][k]["stage1_us"] for r in runs["tree"])
            s2 = statistics.median(r["configs"][k]["stage2_us"] for r in runs["tree"])
            L.append("%-18s %12.1f %12.1f %+12.1f %14.1f %14.1f %12.3f" % ("2^%d %s" % (n.bit_length() - 1, order), st, base, st - base, s1, s2, (st - base) * 1e3 / n))
    L.append("")
    L.append("(without: the mean of the two blocks without floats timed around the configuration in the same process;")
    L.append(" vs 0: the step with floats minus that, i.e. one fused float launch, stage 2 + stage 1, per step;")
    L.append(" stage 1 / stage 2: one launch of that stage alone through beom_update_floats, 20 launches between two syncs.)")
    L.append("")
    L += log
    text = "\n".join(L) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)
    print(text)


if a.one:
    one()
else:
    table()
