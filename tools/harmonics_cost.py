#!/usr/bin/env python3
"""What the harmonics (beom_set_harmonics) cost on one GPU, at 4096 x 4096 x 4 (the headline frame of tools/bench_case.py):

  python tools/harmonics_cost.py [--reps 3] [--steps 40] --parent ab/prev.so [--out profiles/harmonics_cost.txt]    the alternated table
  python tools/harmonics_cost.py --one [--steps 40]                                                                one process: a JSON line
  python tools/harmonics_cost.py --trace                            (what the table starts under rocprofv3 --kernel-trace --stats)

The table alternates fresh processes on one box (tools/moments_cost.py's way): the parent commit's library (BEOM_HIP_LIB) and
this tree's, each stepping WITHOUT harmonics; the tree's process then keeps level 1 with one frequency at stride 1 and 10 and
level 2 with four frequencies at stride 10.  Per configuration: the median step time (wall clock over --steps steps per call,
stream synced on both sides, three blocks); the step time of a run drifts with the step number, so every configuration with
harmonics is timed between two blocks without them in the same process and compared with their mean.  One more process runs
under rocprofv3 --kernel-trace --stats and gives the sample launches' own time per K (first sample and later ones), from
which the bandwidth on the compulsory 4 + 4K words per element and field follows (2 + 2K written by a first sample), beside
the stream-count ceiling of profiles/README.md for that number of arrays.  Without harmonics the tree's step has to lie
within the parent's own max - min over the alternations; the other figures are reported as they come.  `make asm` figures
(resource_usage.txt) are appended if the file is there."""
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
ap.add_argument("--steps", type=int, default=40)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--parent", default=None)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "harmonics_cost.txt"))
ap.add_argument("--frame", type=int, nargs=3, default=(4096, 4096, 4), metavar=("LM", "MM", "NLAY"))
a = ap.parse_args()
M2 = 12.1408331767                                   # rad/day
CONFIGS = ((1, 1, 1), (1, 1, 10), (2, 4, 10))        # (level, K, stride)
# K: the stream-count row of profiles/r01_stream_count_microbench.txt nearest to a later sample's 2 + (1+2K) reads and 1+2K writes
CEILING = {1: ("reads 5 writes 2", 6021), 2: ("reads 8 writes 3", 5818), 3: ("reads 8 writes 3", 5818), 4: ("reads 14 writes 6", 5597)}


def omegas(K):
    return [M2 * (k + 1) for k in range(K)]


def engine():
    from beom_amd import capi, inputs as I
    from beom_amd.grid import read_input_data
    lm, mm, nlay = a.frame
    p, files = I.case_headline(lm, mm, nlay)
    return capi.Engine(read_input_data(p, files=files))


def one():
    import numpy as np
    e = engine()
    lm, mm, nlay = a.frame
    has = hasattr(e.lib, "beom_set_harmonics")
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
    if has:
        for level, K, stride in CONFIGS:
            e.set_harmonics(omegas(K), level, stride)
            rec = steps()
            rec["step_us_without_before"] = before["step_us"]
            e.sample_harmonics(0.1); e.sync()
            t = time.perf_counter()
            for n in range(20):
                e.sample_harmonics(0.1 + 0.01 * n)
            e.sync()
            rec["sample_us"] = round((time.perf_counter() - t) / 20 * 1e6, 1)
            rec["count"] = e.info("harmonic_samples")
            rec["launches"] = e.info("harmonic_launches")
            if K == 1 and stride == 1:                # (the large configurations are not downloaded: 50 arrays of 0.5 GB)
                m = e.download_harmonics()
                rec["finite"] = bool(np.isfinite(m["sum"]).all())
                rec["cond_gram"] = float(np.linalg.cond(m["gram"]))
                del m
            e.set_harmonics(())
            before = steps()
            rec["step_us_without_after"] = before["step_us"]
            out["configs"]["%d/%d/%d" % (level, K, stride)] = rec
        out["configs"]["0 again"] = before
    import ctypes as C
    ptr, sl, sr, r0 = C.c_void_p(), C.c_int64(0), C.c_int64(0), C.c_int64(0)
    e.lib.beom_device_field(e.h, b"hlay", C.byref(ptr), C.byref(sl), C.byref(sr), C.byref(r0))
    out["elements"] = nlay * int(sl.value)          # of every array's padded storage: what one launch covers
    print(json.dumps(out))
    e.close()


def trace():
    """A few steps and samples per K: the kernel trace holds the launches' own times."""
    e = engine()
    for K in (1, 2, 4):
        e.set_harmonics(omegas(K), 1, 1)
        for k in range(3):                   # three first samples and 3 x 6 later ones, three launches each
            e.reset_harmonics()
            e.step(1 + 7 * k, 7)
        e.sync()
        e.set_harmonics(())
    e.close()


def traced():
    """{(K, first): [ns, ...]} of the k_harmonics launches of a --trace process under rocprofv3."""
    d = tempfile.mkdtemp(prefix="harmonics_trace_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
           "--trace", "--frame"] + [str(v) for v in a.frame]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=1500)
    if r.returncode != 0:
        return None, "rocprofv3 failed (rc %d): %s" % (r.returncode, (r.stderr or r.stdout)[-400:].replace("\n", " | "))
    out = {}
    for fn in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        with open(fn) as fh:
            for row in csv.DictReader(fh):
                m = re.search(r"k_harmonics<(\d), (true|false)>", row.get("Kernel_Name", ""))
                if m:
                    out.setdefault((int(m.group(1)), m.group(2) == "true"), []).append(int(row["End_Timestamp"]) - int(row["Start_Timestamp"]))
    return out, None


def resource_lines():
    fn = os.path.join(ROOT, "beom_amd", "csrc", "resource_usage.txt")
    if not os.path.exists(fn):
        return ["(no beom_amd/csrc/resource_usage.txt: run `make asm` for the register figures)"]
    txt = open(fn).read()
    L = []
    for blk in re.split(r"(?=remark: [^\n]*Function Name:)", txt):
        m = re.search(r"Function Name: (\S+)", blk)
        if not m or "k_harmonics" not in m.group(1):
            continue
        g = lambda k: (re.search(k + r": (\d+)", blk) or [None, "?"])[1]
        L.append("  %-40s VGPRs %s  AGPRs %s  SGPRs %s  spills V/S %s/%s  scratch %s B/lane  LDS %s B  occupancy %s waves/SIMD"
                 % (m.group(1), g("VGPRs"), g("AGPRs"), g("SGPRs"), g("VGPRs Spill"), g("SGPRs Spill"), g(r"ScratchSize \[bytes/lane\]"),
                    g(r"LDS Size \[bytes/block\]"), g(r"Occupancy \[waves/SIMD\]")))
    return L or ["(resource_usage.txt names no k_harmonics)"]


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
    L = ["Harmonics (k_harmonics, beom_harmonics.h): cost at %d x %d x %d            tools/harmonics_cost.py" % (lm, mm, nlay), "",
         "%d alternations of two fresh processes (parent's library through BEOM_HIP_LIB and this tree's, the order swapped every time), %d steps per timed call,"
         % (a.reps, a.steps), "three calls per configuration, the median of the three; us per step (wall clock, stream synced).",
         "order of the processes: " + " ".join(l.split()[3] for l in log), ""]
    par = [r["configs"]["0"]["step_us"] for r in runs["parent"]]
    tre = [r["configs"]["0"]["step_us"] for r in runs["tree"]]
    L.append("no harmonics   parent per alternation: %s   max - min %.1f" % (par, max(par) - min(par)))
    L.append("no harmonics   tree   per alternation: %s   median %.1f against the parent's median %.1f (%+.2f %%)"
             % (tre, statistics.median(tre), statistics.median(par), (statistics.median(tre) / statistics.median(par) - 1) * 100))
    spread = max(par) - min(par)
    ok = abs(statistics.median(tre) - statistics.median(par)) <= spread
    L.append("condition (the tree's step without harmonics within the parent's own max - min): %s" % ("met" if ok else "NOT met"))
    again = [r["configs"]["0 again"]["step_us"] for r in runs["tree"]]
    L.append("no harmonics   tree, at the end of the process (step %d; the first figure ends at step %d): %s"
             % (runs["tree"][0]["configs"]["0 again"]["last_step"], runs["tree"][0]["configs"]["0"]["last_step"], again))
    L.append("")
    L.append("%-20s %12s %12s %12s %16s" % ("level / K / stride", "step us", "without us", "vs none us", "one sample us"))
    for level, K, stride in CONFIGS:
        k = "%d/%d/%d" % (level, K, stride)
        st = statistics.median(r["configs"][k]["step_us"] for r in runs["tree"])
        base = statistics.median(0.5 * (r["configs"][k]["step_us_without_before"] + r["configs"][k]["step_us_without_after"]) for r in runs["tree"])
        su = statistics.median(r["configs"][k]["sample_us"] for r in runs["tree"])
        L.append("%-20s %12.1f %12.1f %+12.1f %16.1f" % (k, st, base, st - base, su))
    L.append("")
    L.append("(without: the mean of the two blocks without harmonics timed around the configuration in the same process;")
    L.append(" vs none: the step with harmonics minus that; one sample: beom_sample_harmonics alone, all its fields' launches, 20 samples")
    L.append(" between two syncs, wall clock.)")
    L.append("")
    tr, err = traced()
    L.append("One field's sample launch under rocprofv3 --kernel-trace --stats (a process of its own; median of the launches):")
    if tr is None:
        L.append("  not measured: " + err)
    else:
        n = runs["tree"][0]["elements"]
        cl = nlay * lm * mm
        L.append("  %d elements per array (padded storage), %d wet cell-layers" % (n, cl))
        for (K, first), ns in sorted(tr.items()):
            w = 2 + 2 * K if first else 4 + 4 * K
            t = statistics.median(ns)
            row, gbs = CEILING[K]
            L.append("  k_harmonics<%d, %-5s>  %3d launches  median %8.1f us  %3d B per element  %6.1f B per wet cell-layer  %.2f TB/s%s"
                     % (K, "true" if first else "false", len(ns), t / 1e3, 8 * w, 8.0 * w * n / cl, 8.0 * w * n / t / 1e3,
                        "" if first else "   (ceiling of the '%s' row: %.2f TB/s)" % (row, gbs / 1e3)))
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
