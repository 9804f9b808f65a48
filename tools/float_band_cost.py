#!/usr/bin/env python3
"""What Lagrangian floats on bands (beom_multi_set_floats) cost, at 4096 x 4096 x 4 cut into 2 and 8 bands on ONE device:

  python tools/float_band_cost.py [--reps 2] [--steps 20] --parent ab/prev.so [--out profiles/float_bands_cost.txt]   the table
  python tools/float_band_cost.py --one --bands 2 [--steps 20]                                              one process: a JSON line
  python tools/float_band_cost.py --trace --bands 2                 (what the table starts under rocprofv3 --kernel-trace)

The table alternates fresh processes on one box: the parent commit's library (BEOM_HIP_LIB) and this tree's, each stepping
WITHOUT floats; the tree's process then carries 2^20 floats, and 2^24 floats in row order (sorted by y, then x) and shuffled.
Per configuration: the median step time (wall clock over --steps steps per call, streams synced on both sides, three calls).
Without floats the tree's step has to lie within the parent's own max - min over the alternations; the other figures are
reported as they come.  One more process per band count runs under rocprofv3 --kernel-trace and gives the float launch's and
the ingest's own times.  Every band scans all N slots: the launch's time against N / bands says what that costs.  `make asm`
figures (beom_amd/csrc/resource_usage.txt) are appended if the file is there, and compared with --parent-usage FILE (the
parent's resource_usage.txt) kernel by kernel."""
import argparse
import csv
import glob
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--one", action="store_true")
ap.add_argument("--trace", action="store_true")
ap.add_argument("--bands", type=int, default=2)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--reps", type=int, default=2)
ap.add_argument("--parent", default=None)
ap.add_argument("--parent-usage", default=None)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "float_bands_cost.txt"))
ap.add_argument("--frame", type=int, nargs=3, default=(4096, 4096, 4), metavar=("LM", "MM", "NLAY"))
ap.add_argument("--counts", type=int, nargs="+", default=(1 << 20, 1 << 24))
a = ap.parse_args()


def engine():
    from beom_amd import capi, inputs as I
    from beom_amd.grid import read_input_data
    lm, mm, nlay = a.frame
    p, files = I.case_headline(lm, mm, nlay)
    return capi.MultiEngine(read_input_data(p, files=files), devices=[0] * a.bands)


def floats(n, shuffled):
    """n floats spread evenly over the interior of the closed frame (every interior cell is wet), in row order or shuffled"""
    import numpy as np
    lm, mm, nlay = a.frame
    r = np.random.default_rng(n)
    x, y = r.uniform(1.0, lm - 1.0, n), r.uniform(1.0, mm - 1.0, n)
    if not shuffled:
        o = np.lexsort((x, np.floor(y)))
        x, y = x[o], y[o]
    return x, y, (np.arange(n) % nlay + 1).astype(np.int32)


def one():
    e = engine()
    lm, mm, nlay = a.frame
    out = {"bands": a.bands, "lib": "BEOM_HIP_LIB" if os.environ.get("BEOM_HIP_LIB") else "in-tree", "configs": {}}
    tstp = [1]

    def steps():
        e.step(tstp[0], 10); tstp[0] += 10
        blocks = []
        for _ in range(3):
            e.sync()
            t = time.perf_counter(); e.step(tstp[0], a.steps); blocks.append((time.perf_counter() - t) / a.steps * 1e6)
            tstp[0] += a.steps
        return {"step_us": round(statistics.median(blocks), 1), "step_us_blocks": [round(b, 1) for b in blocks]}

    before = out["configs"]["0"] = steps()
    if hasattr(e.lib, "beom_multi_set_floats"):
        for n in a.counts:
            for shuffled in ((False,) if n < max(a.counts) else (False, True)):
                x, y, layer = floats(n, shuffled)
                e.set_floats(x, y, layer)
                rec = steps()
                rec["step_us_without_before"] = before["step_us"]
                got = e.download_floats()
                rec["handovers"] = e.info("float_handovers")
                rec["moved"] = int((got["y"] != y).sum())
                rec["capacity"] = max(4096, n // 8)
                rec["outbox_copy_bytes_per_step"] = 64 * (rec["capacity"] + 1) * 2 * (a.bands - 1)
                e.set_floats([], [], [])
                before = steps()
                rec["step_us_without_after"] = before["step_us"]
                out["configs"]["%d %s" % (n, "shuffled" if shuffled else "row order")] = rec
    print(json.dumps(out))
    e.close()


def trace():
    e = engine()
    for n in a.counts:
        x, y, layer = floats(n, False)
        e.set_floats(x, y, layer)
        e.step(1, 6)
        e.sync()
    e.close()


def traced(bands):
    """{kernel: [ns, ...]} of the float kernels of a --trace process under rocprofv3, in launch order"""
    d = tempfile.mkdtemp(prefix="float_bands_trace_")
    cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
           "--trace", "--bands", str(bands), "--frame"] + [str(v) for v in a.frame] + ["--counts"] + [str(n) for n in a.counts]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=1500)
    if r.returncode != 0:
        return None, "rocprofv3 failed (rc %d): %s" % (r.returncode, (r.stderr or r.stdout)[-400:].replace("\n", " | "))
    rows = []
    for fn in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        with open(fn) as fh:
            for row in csv.DictReader(fh):
                m = re.search(r"(k_floats_band<\d>|k_floats_ingest)", row.get("Kernel_Name", ""))
                if m:
                    rows.append((int(row["Start_Timestamp"]), m.group(1), int(row["End_Timestamp"]) - int(row["Start_Timestamp"]),
                                 int(row.get("Grid_Size", row.get("Grid_Size_X", 0)) or 0)))
    out = {}
    for _, k, ns, grid in sorted(rows):
        out.setdefault((k, grid), []).append(ns)
    return out, None


def usage(fn):
    if not fn or not os.path.exists(fn):
        return None
    out = {}
    for blk in re.split(r"(?=remark: [^\n]*Function Name:)", open(fn).read()):
        m = re.search(r"Function Name: (\S+)", blk)
        if m:
            g = lambda k: (re.search(k + r": (\d+)", blk) or [None, "?"])[1]
            out[m.group(1)] = (g("VGPRs"), g("AGPRs"), g("TotalSGPRs"), g("VGPRs Spill"), g("SGPRs Spill"), g(r"ScratchSize \[bytes/lane\]"),
                               g(r"Occupancy \[waves/SIMD\]"))
    return out


def resource_lines():
    new = usage(os.path.join(ROOT, "beom_amd", "csrc", "resource_usage.txt"))
    if new is None:
        return ["(no beom_amd/csrc/resource_usage.txt: run `make asm` for the register figures)"]
    L = []
    for k, v in new.items():
        if "k_floats_band" in k or "k_floats_ingest" in k or "k_floats_check_band" in k:
            L.append("  %-62s VGPRs %s  AGPRs %s  SGPRs %s  spills V/S %s/%s  scratch %s B/lane  occupancy %s" % ((k,) + v))
    old = usage(a.parent_usage)
    if old is None:
        L.append("(no --parent-usage file: the earlier kernels were not compared)")
    else:
        diff = [k for k in old if new.get(k) != old[k]]
        L.append("earlier kernels: %d in the parent's resource_usage.txt, %d of them here with other VGPR / AGPR / SGPR / spill / scratch / "
                 "occupancy figures%s; %d new kernels" % (len(old), len(diff), (": " + ", ".join(diff)) if diff else "", len(set(new) - set(old))))
    return L


def table():
    if not a.parent:
        sys.exit("--parent LIB: the parent commit's libbeom_hip.so is needed for the alternation")
    lm, mm, nlay = a.frame
    L = ["Floats on bands (k_floats_band, k_floats_ingest; beom_floats.h): cost at %d x %d x %d on one device      tools/float_band_cost.py" % (lm, mm, nlay), "",
         "%d alternations of two fresh processes per band count (the parent's library through BEOM_HIP_LIB and this tree's, the order swapped every"
         % a.reps, "time), %d steps per timed call, three calls per configuration, the median of the three; us per step (wall clock, streams synced)." % a.steps, ""]
    log = []
    for bands in (2, 8):
        runs = {"parent": [], "tree": []}
        for rep in range(a.reps):
            for who in (("parent", "tree") if rep % 2 == 0 else ("tree", "parent")):
                env = dict(os.environ)
                env.pop("BEOM_HIP_LIB", None)
                if who == "parent":
                    env["BEOM_HIP_LIB"] = os.path.abspath(a.parent)
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", "--bands", str(bands), "--steps", str(a.steps), "--frame"]
                                   + [str(v) for v in a.frame] + ["--counts"] + [str(n) for n in a.counts], env=env, capture_output=True, text=True, timeout=1500)
                if r.returncode != 0:
                    sys.exit("%s failed (rc %d):\n%s\n%s" % (who, r.returncode, r.stdout[-2000:], r.stderr[-2000:]))
                rec = json.loads(r.stdout.strip().splitlines()[-1])
                runs[who].append(rec)
                log.append("# bands %d rep %d %-6s %s" % (bands, rep, who, json.dumps(rec)))
                print(log[-1], flush=True)
        par = [r["configs"]["0"]["step_us"] for r in runs["parent"]]
        tre = [r["configs"]["0"]["step_us"] for r in runs["tree"]]
        L.append("%d bands" % bands)
        L.append("  no floats   parent per alternation: %s   max - min %.1f" % (par, max(par) - min(par)))
        L.append("  no floats   tree   per alternation: %s   median %.1f against the parent's median %.1f (%+.2f %%)"
                 % (tre, statistics.median(tre), statistics.median(par), (statistics.median(tre) / statistics.median(par) - 1) * 100))
        ok = abs(statistics.median(tre) - statistics.median(par)) <= max(par) - min(par)
        L.append("  condition (the tree's step without floats within the parent's own max - min): %s" % ("met" if ok else "NOT met"))
        L.append("  %-22s %10s %12s %12s %12s %12s %22s" % ("floats", "step us", "without us", "vs none us", "hand-overs", "moved", "outbox copies B/step"))
        for k in runs["tree"][0]["configs"]:
            if k == "0":
                continue
            st = statistics.median(r["configs"][k]["step_us"] for r in runs["tree"])
            base = statistics.median(0.5 * (r["configs"][k]["step_us_without_before"] + r["configs"][k]["step_us_without_after"]) for r in runs["tree"])
            c = runs["tree"][0]["configs"][k]
            L.append("  %-22s %10.1f %12.1f %+12.1f %12d %12d %22d" % (k, st, base, st - base, c["handovers"], c["moved"], c["outbox_copy_bytes_per_step"]))
        tr, err = traced(bands)
        L.append("  under rocprofv3 --kernel-trace (a process of its own, floats in row order; median of the launches per kernel and grid size):")
        if tr is None:
            L.append("    not measured: " + err)
        else:
            for (k, grid), ns in sorted(tr.items(), key=lambda kv: (kv[0][1], kv[0][0])):
                L.append("    %-20s grid %10d  %3d launches  median %9.1f us" % (k, grid, len(ns), statistics.median(ns) / 1e3))
        L.append("")
    L.append("(without: the mean of the two blocks without floats timed around the configuration in the same process; outbox copies: 64 B x")
    L.append(" (capacity + 1) per neighbour side at the default capacity max(4096, n / 8), whatever the number of records in them.)")
    L.append("")
    L.append("`make asm` figures of the new kernels:")
    L += resource_lines()
    L.append("")
    L += log
    text = "\n".join(L) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)
    print(text)


if a.one:
    one()
elif a.trace:
    trace()
else:
    table()
