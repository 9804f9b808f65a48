#!/usr/bin/env python3
"""What forcing in time (beom_set_forcing) costs on one GPU, at 4096 x 4096 x 4 (the headline frame of tools/bench_case.py):

  python tools/forcing_cost.py [--reps 2] [--steps 40] --parent ab/prev.so [--parent-asm ab/prev_resource_usage.txt]    the alternated table
  python tools/forcing_cost.py --one [--steps 40]                                                                       one process: a JSON line
  python tools/forcing_cost.py --trace                                (what the table starts under rocprofv3 --kernel-trace --stats)

The table alternates fresh processes on one box (tools/moments_cost.py's way): the parent commit's library (BEOM_HIP_LIB) and
this tree's, each stepping WITHOUT frames; the tree's process then steps with two taus frames, with two hdot frames and with
both, the frames so far apart that every step has a weight of its own and launches.  Per configuration: the median step time
(wall clock over --steps steps per call, stream synced on both sides, three blocks); the step time of a run drifts with the
step number, so every configuration with frames is timed between two blocks without them in the same process and compared
with their mean.  The headline case has neither wind nor hdot of its own: a handle that is given frames GAINS the term, so
its step also pays for the stress (folded into the momentum sweep, no longer the plain form) resp. for hdot in update_h; the
table says what the step costs, the trace what the launch alone costs.  One more process runs under rocprofv3
--kernel-trace --stats and gives k_forcing_lerp's own time, from which the bandwidth on the compulsory words follows (taus:
2 read + 2 written, hdot: 2 + 1 per element), beside the stream-count ceiling of profiles/README.md.  Without frames the
tree's step is stated against the parent's own max - min over the alternations; nothing is fixed here.  `make asm` figures
(resource_usage.txt) are appended if the file is there, compared with the parent's listing if --parent-asm names it."""
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
ap.add_argument("--reps", type=int, default=2)
ap.add_argument("--parent", default=None)
ap.add_argument("--parent-asm", default=None)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "forcing_cost.txt"))
ap.add_argument("--frame", type=int, nargs=3, default=(4096, 4096, 4), metavar=("LM", "MM", "NLAY"))
a = ap.parse_args()
CONFIGS = (("taus",), ("hdot",), ("taus", "hdot"))
# the stream-count row of profiles/r01_stream_count_microbench.txt nearest to 2 reads and 1 | 2 writes (the file has no row of
# exactly these counts: the copy, 1 + 1, stands above both; 3 + 4 at 5961 GB/s below)
CEILING = ("reads 1 writes 1", 6112)
WORDS = {"taus": 4, "hdot": 3}


def engine():
    from beom_amd import capi, inputs as I
    from beom_amd.grid import read_input_data
    lm, mm, nlay = a.frame
    p, files = I.case_headline(lm, mm, nlay)
    f = read_input_data(p, files=files)
    return capi.Engine(f), f


def frames_of(f, field):
    """Two frames over the real cells: a smooth pattern and 1.5 times it, 0.05 N/m2 resp. 1e-5 of the top layer per step."""
    import numpy as np
    shape = (2 if field == "taus" else f.p.nlay, f.p.ndeg + 1)
    amp = 0.05 if field == "taus" else 1.e-5 * float(np.mean(f.hlay[0, 1:])) / float(f.p.dt)
    base = np.zeros(shape)
    base[:, 1:] = amp * np.sin(1.e-3 * np.arange(1, shape[1]))[None, :]
    return np.stack([base, 1.5 * base])


def give(e, f, fields):
    import numpy as np
    times = np.array([0.0, 1.e6 * float(f.p.dtd8)])          # (every step of the run lies between the two: a weight of its own)
    for field in fields:
        e.set_forcing(field, times, frames_of(f, field))


def one():
    e, f = engine()
    lm, mm, nlay = a.frame
    has = hasattr(e.lib, "beom_set_forcing")
    out = {"lm": lm, "mm": mm, "nlay": nlay, "lib": "BEOM_HIP_LIB" if os.environ.get("BEOM_HIP_LIB") else "in-tree", "configs": {}}
    tstp = [1]

    def steps():
        e.step(tstp[0], 10); tstp[0] += 10
        blocks = []
        for _ in range(3):
            e.sync()
            t = time.perf_counter(); e.step(tstp[0], a.steps); blocks.append((time.perf_counter() - t) / a.steps * 1e6)
            tstp[0] += a.steps
        return {"step_us": round(statistics.median(blocks), 1), "step_us_blocks": [round(b, 1) for b in blocks], "last_step": tstp[0] - 1,
                "stress_folded": e.info("stress_folded"), "plain_sweeps": e.info("plain_sweeps")}

    before = out["configs"]["none"] = steps()
    if has:
        for fields in CONFIGS:
            give(e, f, fields)
            n0 = e.info("forcing_launches")
            rec = steps()
            rec["launches_per_step"] = (e.info("forcing_launches") - n0) / float(10 + 3 * a.steps)
            rec["step_us_without_before"] = before["step_us"]
            for field in fields:
                e.set_forcing(field, None)
            before = steps()
            rec["step_us_without_after"] = before["step_us"]
            out["configs"]["+".join(fields)] = rec
        out["configs"]["none again"] = before
    import ctypes as C
    ptr, sl, sr, r0 = C.c_void_p(), C.c_int64(0), C.c_int64(0), C.c_int64(0)
    e.lib.beom_device_field(e.h, b"hlay", C.byref(ptr), C.byref(sl), C.byref(sr), C.byref(r0))
    out["elements_per_slice"] = int(sl.value)         # of every array's padded storage: what one slice of a launch covers
    print(json.dumps(out))
    e.close()


def trace():
    """A few steps with both sets: the kernel trace holds the launches' own times."""
    e, f = engine()
    give(e, f, ("taus", "hdot"))
    e.step(1, 12)
    e.sync()
    e.close()


def traced():
    """{"taus" | "hdot": [ns, ...]} of the k_forcing_lerp launches of a --trace process under rocprofv3."""
    d = tempfile.mkdtemp(prefix="forcing_trace_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
           "--trace", "--frame"] + [str(v) for v in a.frame]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=1500)
    if r.returncode != 0:
        return None, "rocprofv3 failed (rc %d): %s" % (r.returncode, (r.stderr or r.stdout)[-400:].replace("\n", " | "))
    out = {}
    for fn in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        with open(fn) as fh:
            for row in csv.DictReader(fh):
                m = re.search(r"k_forcing_lerp<(true|false|1|0), ", row.get("Kernel_Name", ""))
                if m:
                    out.setdefault("taus" if m.group(1) in ("true", "1") else "hdot", []).append(int(row["End_Timestamp"]) - int(row["Start_Timestamp"]))
    return out, None


FIGURES = ("SGPRs", "VGPRs", "AGPRs", "SGPRs Spill", "VGPRs Spill", r"ScratchSize \[bytes/lane\]", r"LDS Size \[bytes/block\]", r"Occupancy \[waves/SIMD\]")


def listing(fn):
    """{function: (figures...)} of a `make asm` listing (-Rpass-analysis=kernel-resource-usage)."""
    out = {}
    for blk in re.split(r"(?=remark: [^\n]*Function Name:)", open(fn).read()):
        m = re.search(r"Function Name: (\S+)", blk)
        if m:
            out[m.group(1)] = tuple((re.search(k + r": (\d+)", blk) or [None, "?"])[1] for k in FIGURES)
    return out


def resource_lines():
    fn = os.path.join(ROOT, "beom_amd", "csrc", "resource_usage.txt")
    if not os.path.exists(fn):
        return ["(no beom_amd/csrc/resource_usage.txt: run `make asm` for the register figures)"]
    new = listing(fn)
    L = ["`make asm` figures of the new kernel's instantiations (gfx950, -O3 -ffp-contract=off):"]
    for name, g in sorted(new.items()):
        if "k_forcing_lerp" in name:
            L.append("  %-44s SGPRs %s  VGPRs %s  AGPRs %s  spills S/V %s/%s  scratch %s B/lane  LDS %s B  occupancy %s waves/SIMD" % ((name,) + g))
    if a.parent_asm and os.path.exists(a.parent_asm):
        old = listing(a.parent_asm)
        same = [k for k in old if new.get(k) == old[k]]
        diff = [k for k in old if new.get(k) != old[k]]
        L.append("Every earlier kernel: %d of the %d functions of the parent's `make asm` listing report identical SGPR, VGPR, AGPR, spill, scratch,"
                 % (len(same), len(old)))
        L.append("LDS and occupancy figures in this build%s  DevView is unchanged." % ("." if not diff else "; NOT identical: " + ", ".join(diff) + "."))
    else:
        L.append("(no parent listing given: --parent-asm)")
    return L


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
    L = ["Forcing in time (k_forcing_lerp, beom_forcing.h): cost at %d x %d x %d            tools/forcing_cost.py" % (lm, mm, nlay), "",
         "%d alternations of two fresh processes (parent's library through BEOM_HIP_LIB and this tree's, the order swapped every time), %d steps per timed call,"
         % (a.reps, a.steps), "three calls per configuration, the median of the three; us per step (wall clock, stream synced).",
         "order of the processes: " + " ".join(l.split()[3] for l in log), ""]
    par = [r["configs"]["none"]["step_us"] for r in runs["parent"]]
    tre = [r["configs"]["none"]["step_us"] for r in runs["tree"]]
    L.append("no frames   parent per alternation: %s   max - min %.1f" % (par, max(par) - min(par)))
    L.append("no frames   tree   per alternation: %s   median %.1f against the parent's median %.1f (%+.2f %%)"
             % (tre, statistics.median(tre), statistics.median(par), (statistics.median(tre) / statistics.median(par) - 1) * 100))
    L.append("the tree's median minus the parent's: %+.1f us; the parent's own max - min over the alternations: %.1f us"
             % (statistics.median(tre) - statistics.median(par), max(par) - min(par)))
    again = [r["configs"]["none again"]["step_us"] for r in runs["tree"]]
    L.append("no frames   tree, at the end of the process (step %d; the first figure ends at step %d): %s"
             % (runs["tree"][0]["configs"]["none again"]["last_step"], runs["tree"][0]["configs"]["none"]["last_step"], again))
    L.append("")
    L.append("%-12s %10s %12s %12s %10s %8s %8s" % ("frames of", "step us", "without us", "vs none us", "launches", "folded", "plain"))
    for fields in CONFIGS:
        k = "+".join(fields)
        st = statistics.median(r["configs"][k]["step_us"] for r in runs["tree"])
        base = statistics.median(0.5 * (r["configs"][k]["step_us_without_before"] + r["configs"][k]["step_us_without_after"]) for r in runs["tree"])
        c = runs["tree"][0]["configs"][k]
        L.append("%-12s %10.1f %12.1f %+12.1f %10.2f %8d %8d" % (k, st, base, st - base, c["launches_per_step"], c["stress_folded"], c["plain_sweeps"]))
    c = runs["tree"][0]["configs"]["none"]
    L.append("%-12s %10s %12s %12s %10s %8d %8d" % ("none", "", "", "", "", c["stress_folded"], c["plain_sweeps"]))
    L.append("")
    L.append("(without: the mean of the two blocks without frames timed around the configuration in the same process; vs none: the step with")
    L.append(" frames minus that; launches: k_forcing_lerp launches per step; folded, plain: beom_info \"stress_folded\", \"plain_sweeps\" of the")
    L.append(" last step.  The case has no wind and no hdot: with frames the handle gains the term, and the step pays for it besides the launch.)")
    L.append("")
    tr, err = traced()
    L.append("The launch under rocprofv3 --kernel-trace --stats (a process of its own, both sets, 12 steps; median of the launches):")
    if tr is None:
        L.append("  not measured: " + err)
    else:
        n = runs["tree"][0]["elements_per_slice"]
        for field, ns in sorted(tr.items()):
            outer = 2 if field == "taus" else nlay
            t = statistics.median(ns)
            unit = lm * mm * outer
            L.append("  k_forcing_lerp %-4s  %3d launches  median %8.1f us  %d slices of %d elements (padded storage)  %2d B per element  %.2f TB/s"
                     "   floor at the '%s' row's %.2f TB/s: %.1f us   (%.1f B per cell and %s)"
                     % (field, len(ns), t / 1e3, outer, n, 8 * WORDS[field], 8.0 * WORDS[field] * n * outer / t / 1e3, CEILING[0], CEILING[1] / 1e3,
                        8.0 * WORDS[field] * n * outer / CEILING[1] / 1e3, 8.0 * WORDS[field] * n * outer / unit,
                        "direction" if field == "taus" else "layer"))
    L.append("")
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
