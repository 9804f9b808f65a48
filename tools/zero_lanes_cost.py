#!/usr/bin/env python3
"""What the zero-lane shortcut of uv_core (DevView::vel_targets_zero: exact-zero lanes take their +0 velocity target as a
literal instead of fetching it) changes on one GPU, frame by frame, against the parent commit's library:

  python tools/zero_lanes_cost.py [--reps 3] [--steps 40] --parent ab/prev.so [--out profiles/zero_lanes_cost.txt]    the alternated table
  python tools/zero_lanes_cost.py --one FRAME [--steps 40]                                                            one process: a JSON line

Frames:
  headline   4096 x 4096 x 4 as bench.py steps it: a third of the cell-layers are exact-zero lanes, the targets are +0
  wide       control: the same frame with the mound widened to radius lm / 3 — no lane is an exact zero       (expected: no change)
  jet        guard: 2048 x 2048 x 2, the targets hold the jet (flag 0), exact zeros are rare                  (expected: no change)
  sill       guard: 4096 x 512 x 4, general form with sponges                                                 (expected: no change)

The table alternates fresh processes on one box (tools/ab.sh's way, the order swapped every time): the parent's library
(BEOM_HIP_LIB) and this tree's.  Every process runs under its own `timeout`, and the first one that fails ends the script.
Per process: 10 steps, then three timed calls of --steps steps (wall clock, stream synced on both sides), the median of
the three; at the end the census (u == 0 & v == 0).mean() over the cell-layers of the downloaded state — no oracle."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FRAMES = ("headline", "wide", "jet", "sill")

ap = argparse.ArgumentParser()
ap.add_argument("--one", choices=FRAMES)
ap.add_argument("--steps", type=int, default=40)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--parent", default=None)
ap.add_argument("--limit", type=int, default=300, help="seconds a process may take (timeout -k 10)")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "zero_lanes_cost.txt"))
a = ap.parse_args()


def case(frame):
    import numpy as np
    from beom_amd import inputs as I
    if frame == "jet":
        return I.case_unstable_jet(lm=2048, mm=2048, nlay=2, dt_s=50.0)
    if frame == "sill":
        return I.case_sill_exchange3d(lm=4096, mm=512, nlay=4, dt_s=30.0, npts=15, sill_halfwidth=50.0)
    p, files = I.recipe_headline(4096, 4096, 4).whole()
    if frame == "wide":      # the recipe's mound, radius lm / 3 instead of lm / 12: it is nowhere lost in the rounding of the layers
        lm, mm, nlay = p.lm, p.mm, p.nlay
        x = (np.arange(lm + 2, dtype=np.float64) - 0.5 * (lm + 1))[:, None]
        y = (np.arange(mm + 2, dtype=np.float64) - 0.5 * (mm + 1))[None, :]
        mound = np.exp(-(x * x + y * y) / (lm / 3.0) ** 2).astype(np.float32)
        init = np.zeros_like(files["init"])
        for k in range(nlay):
            init[:, :, k, 0] = mound * np.float32(1.0 - k / nlay)
        files = dict(files, init=init)
    return p, files


def one(frame):
    import numpy as np
    from beom_amd import capi
    from beom_amd.grid import read_input_data
    p, files = case(frame)
    e = capi.Engine(read_input_data(p, files=files))
    del files
    try:
        flag = e.info("vel_targets_zero")
    except capi.BeomError:                  # (the parent's library named by BEOM_HIP_LIB)
        flag = None
    e.step(1, 10)
    t, blocks = 11, []
    for _ in range(3):
        e.sync()
        t0 = time.perf_counter(); e.step(t, a.steps); blocks.append((time.perf_counter() - t0) / a.steps * 1e6)
        t += a.steps
    st = e.download(("u", "v"))
    u, v = st["u"][:, 1:], st["v"][:, 1:]
    print(json.dumps({"frame": frame, "lm": p.lm, "mm": p.mm, "nlay": p.nlay, "lib": "BEOM_HIP_LIB" if os.environ.get("BEOM_HIP_LIB") else "in-tree",
                      "vel_targets_zero": flag, "plain_sweeps": e.info("plain_sweeps"), "step_us": round(statistics.median(blocks), 1),
                      "step_us_blocks": [round(b, 1) for b in blocks], "last_step": t - 1,
                      "zero_lanes": round(float(((u == 0.0) & (v == 0.0)).mean()), 4), "finite": bool(np.isfinite(u).all() and np.isfinite(v).all())}))
    e.close()


def table():
    if not a.parent:
        sys.exit("--parent LIB: the parent commit's libbeom_hip.so is needed for the alternation")
    runs = {(f, w): [] for f in FRAMES for w in ("parent", "tree")}
    log = []
    for frame in FRAMES:
        for rep in range(a.reps):
            for who in (("parent", "tree") if rep % 2 == 0 else ("tree", "parent")):      # (ABBA: neither library always runs second)
                env = dict(os.environ)
                env.pop("BEOM_HIP_LIB", None)
                if who == "parent":
                    env["BEOM_HIP_LIB"] = os.path.abspath(a.parent)
                r = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--one", frame, "--steps", str(a.steps)],
                                   env=env, capture_output=True, text=True)
                if r.returncode != 0:       # nothing more is started on the GPU
                    sys.exit("%s %s failed (rc %d):\n%s\n%s" % (frame, who, r.returncode, r.stdout[-2000:], r.stderr[-2000:]))
                rec = json.loads(r.stdout.strip().splitlines()[-1])
                runs[(frame, who)].append(rec)
                log.append("# %-8s rep %d %-6s %s" % (frame, rep, who, json.dumps(rec)))
                print(log[-1], flush=True)
    L = ["Zero-lane shortcut of uv_core: step times against the parent's library            tools/zero_lanes_cost.py", "",
         "%d alternations per frame of two fresh processes (the parent's library through BEOM_HIP_LIB and this tree's, the order swapped every time)," % a.reps,
         "10 steps, then three timed calls of %d steps, the median of the three; us per step (wall clock, stream synced)." % a.steps,
         "zero lanes: (u == 0 & v == 0).mean() over the cell-layers of the state downloaded at the end (step %d)." % (10 + 3 * a.steps), "",
         "%-9s %-14s %5s %6s %11s %10s %10s %8s %9s  %s" % ("frame", "size", "flag", "plain", "zero lanes", "parent us", "tree us", "change", "spread us", "within the parent's max - min")]
    for frame in FRAMES:
        par = [r["step_us"] for r in runs[(frame, "parent")]]
        tre = [r["step_us"] for r in runs[(frame, "tree")]]
        r0 = runs[(frame, "tree")][0]
        mp, mt, spread = statistics.median(par), statistics.median(tre), max(par) - min(par)
        L.append("%-9s %-14s %5s %6s %11.4f %10.1f %10.1f %+7.2f%% %9.1f  %s"
                 % (frame, "%dx%dx%d" % (r0["lm"], r0["mm"], r0["nlay"]), r0["vel_targets_zero"], r0["plain_sweeps"], r0["zero_lanes"], mp, mt,
                    (mt / mp - 1) * 100, spread, "yes" if abs(mt - mp) <= spread else "no"))
        same = {r["zero_lanes"] for w in ("parent", "tree") for r in runs[(frame, w)]}
        if len(same) != 1:
            L.append("          (the census differs between the processes: %s)" % sorted(same))
    L += ["", "(frames wide, jet and sill are expected within the parent's spread; the headline frame is the one the change is for)", ""] + log
    text = "\n".join(L) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)
    print(text)


if a.one:
    one(a.one)
else:
    table()
