#!/usr/bin/env python3
"""What the tracer moments (beom_set_tracer_moments) cost on one GPU, at 4096 x 4096 x 4 (the headline frame of
tools/bench_case.py); modelled on tools/moments_cost.py:

  python tools/tracer_moments_cost.py [--reps 3] [--steps 40] --parent ab/prev.so [--parent-asm FILE] [--out profiles/tracer_moments_cost.txt]
  python tools/tracer_moments_cost.py --one [--steps 40]                                                      one process: a JSON line
  python tools/tracer_moments_cost.py --trace                       (what the table starts under rocprofv3 --kernel-trace --stats)

The table alternates fresh processes on one box (tools/ab.sh's way): the parent commit's library (BEOM_HIP_LIB) and this
tree's, each stepping with 1 and with 4 tracers and WITHOUT tracer moments; the tree's process then keeps level 1, 2, 3 at
stride 1 and level 3 at stride 10 on its 4 tracers.  Per configuration: the median step time (wall clock over --steps steps
per call, stream synced on both sides, three blocks); every configuration with tracer moments is timed between two blocks
without them in the same process and compared with their mean.  One more process runs under rocprofv3 --kernel-trace --stats
and gives the sample launch's own time per level and tracer count (first sample and later ones), next to the floor of the
compulsory words (DESIGN.md section 4 "Tracer moments") at the streaming rate of profiles/README.md.  Without tracer moments
the tree's step has to lie within the parent's own max - min over the alternations; the other figures are reported as they
come.  `make asm` figures (resource_usage.txt) of the new kernel are appended, and with --parent-asm (the parent's
resource_usage.txt) the comparison of every earlier kernel's figures."""
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
ap.add_argument("--parent-asm", default=None)
ap.add_argument("--asm-only", action="store_true", help="print the make asm comparison alone (no GPU)")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tracer_moments_cost.txt"))
ap.add_argument("--frame", type=int, nargs=3, default=(4096, 4096, 4), metavar=("LM", "MM", "NLAY"))
a = ap.parse_args()
TRACERS = (1, 4)
CONFIGS = ((1, 1), (2, 1), (3, 1), (3, 10))          # (level, stride), on 4 tracers
RATE_TBS = 5.6                                       # the 14+6-stream row of profiles/r01_stream_count_microbench.txt


def words(level, first, ntrc):
    """Compulsory 8-byte words per cell-layer: the thicknesses and transports once, then per tracer q, the references read (a
    first sample writes them), the sums (and Q) read and written (written)."""
    shared = 1 if level == 1 else 3
    nq = 2 if level == 1 else 4
    per = 1 + nq + (1 if first else 2) * (nq + (1 if level == 3 else 0))
    return shared + per * ntrc


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
    has = hasattr(e.lib, "beom_set_tracer_moments")
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

    for n in TRACERS:
        e.set_tracers(n)
        e.set_concentration(np.linspace(0.25, 1.0, n)[:, None, None])
        before = out["configs"]["trc%d" % n] = steps()
    if has:
        for level, stride in CONFIGS:
            e.set_tracer_moments(level, stride)
            rec = steps()
            rec["step_us_without_before"] = before["step_us"]
            e.sample_tracer_moments(); e.sync()
            t = time.perf_counter()
            for _ in range(20):
                e.sample_tracer_moments()
            e.sync()
            rec["sample_us"] = round((time.perf_counter() - t) / 20 * 1e6, 1)
            rec["count"] = e.info("tracer_moment_samples")
            if level == 3 and stride == 10:
                m = e.download_tracer_moments()
                rec["finite"] = bool(np.isfinite(m["sum"]).all() and np.isfinite(m["sq"]).all())
                rec["max_var_c"] = float(m["var_c"].max())
                del m
            e.set_tracer_moments(0)
            before = steps()
            rec["step_us_without_after"] = before["step_us"]
            out["configs"]["%d/%d" % (level, stride)] = rec
        out["configs"]["trc4 again"] = before
    print(json.dumps(out))
    e.close()


def trace():
    """A few steps and samples per tracer count and level: the kernel trace holds the launches' own times, in this order."""
    import numpy as np
    e = engine()
    for n in TRACERS:
        e.set_tracers(n)
        e.set_concentration(np.linspace(0.25, 1.0, n)[:, None, None])
        for level in (1, 2, 3):
            e.set_tracer_moments(level, 1)
            for k in range(2):                   # two first samples and 2 x 4 later ones
                e.reset_tracer_moments()
                e.step(1 + 5 * k, 5)
            e.sync()
    e.close()


def traced():
    """{(ntrc, level, first): [ns, ...]} of the k_tracer_moments launches of a --trace process under rocprofv3: the launches
    come in the order of trace(), 10 per (ntrc, level)."""
    d = tempfile.mkdtemp(prefix="tracer_moments_trace_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
           "--trace", "--frame"] + [str(v) for v in a.frame]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        return None, "rocprofv3 failed (rc %d): %s" % (r.returncode, (r.stderr or r.stdout)[-400:].replace("\n", " | "))
    rows = []
    for fn in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        with open(fn) as fh:
            for row in csv.DictReader(fh):
                m = re.search(r"k_tracer_moments<.*?(\d), (true|false)>", row.get("Kernel_Name", ""))
                if m:
                    rows.append((int(row["Start_Timestamp"]), int(m.group(1)), m.group(2) == "true", int(row["End_Timestamp"]) - int(row["Start_Timestamp"])))
    rows.sort()
    out = {}
    per = 10 * 3                                  # launches per tracer count
    for k, (_, level, first, ns) in enumerate(rows):
        out.setdefault((TRACERS[min(k // per, len(TRACERS) - 1)], level, first), []).append(ns)
    return out, None


def _usage(fn):
    """{function name: the figures of its remark block} of a `make asm` listing."""
    keys = ("TotalSGPRs", "VGPRs", "AGPRs", r"ScratchSize \[bytes/lane\]", r"Occupancy \[waves/SIMD\]", "SGPRs Spill", "VGPRs Spill", r"LDS Size \[bytes/block\]")
    out = {}
    for blk in re.split(r"(?=remark: [^\n]*Function Name:)", open(fn).read()):
        m = re.search(r"Function Name: (\S+)", blk)
        if m:
            out[m.group(1)] = tuple((re.search(r"remark: [^\n]*\b" + k + r": (\d+)", blk) or [None, "?"])[1] for k in keys)
    return out


def resource_lines():
    fn = os.path.join(ROOT, "beom_amd", "csrc", "resource_usage.txt")
    if not os.path.exists(fn):
        return ["(no beom_amd/csrc/resource_usage.txt: run `make asm` for the register figures)"]
    mine = _usage(fn)
    L = ["`make asm` figures of the new kernel (gfx950, -O3 -ffp-contract=off; <context, level, first sample>):"]
    for name, v in sorted(mine.items()):
        if "k_tracer_moments" in name:
            short = re.sub(r"^_Z\d+k_tracer_momentsI\d+(Cell(?:Dense|Gather))T?(ILb0EE)?Li(\d)ELb([01])E.*$", r"k_tracer_moments<\1, \3, \4>", name)
            L.append("  %-42s SGPRs %3s  VGPRs %3s  AGPRs %s  spills S/V %s/%s  scratch %s B/lane  LDS %s B  occupancy %s waves/SIMD"
                     % (short, v[0], v[1], v[2], v[5], v[6], v[3], v[7], v[4]))
    if a.parent_asm and os.path.exists(a.parent_asm):
        par = _usage(a.parent_asm)
        moved = [n for n in par if par[n] != mine.get(n)]
        new = [n for n in mine if n not in par]
        L.append("")
        L.append("Every earlier kernel: %d of the %d functions of the parent's `make asm` listing report identical SGPR, VGPR, AGPR, spill,"
                 % (len(par) - len(moved), len(par)))
        L.append("scratch, LDS and occupancy figures in this tree's listing (compared function by function); %d functions are new, all of them"
                 % len(new))
        L.append("k_tracer_moments: %s." % ("yes" if all("k_tracer_moments" in n for n in new) else "NO: " + ", ".join(n for n in new if "k_tracer_moments" not in n)))
        for n in moved:
            L.append("  MOVED %s: parent %s, tree %s" % (n, par[n], mine.get(n)))
    else:
        L.append("(no --parent-asm listing: the earlier kernels' figures were not compared)")
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
                               env=env, capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                sys.exit("%s failed (rc %d):\n%s\n%s" % (who, r.returncode, r.stdout[-2000:], r.stderr[-2000:]))
            rec = json.loads(r.stdout.strip().splitlines()[-1])
            runs[who].append(rec)
            log.append("# rep %d %-6s %s" % (rep, who, json.dumps(rec)))
            print(log[-1], flush=True)
    lm, mm, nlay = a.frame
    cl = nlay * (lm + 1) * (mm + 1)
    L = ["Tracer moments (k_tracer_moments, beom_tracer_moments.h): cost at %d x %d x %d            tools/tracer_moments_cost.py" % (lm, mm, nlay), "",
         "%d alternations of two fresh processes (parent's library through BEOM_HIP_LIB and this tree's, the order swapped every time), %d steps per timed call,"
         % (a.reps, a.steps), "three calls per configuration, the median of the three; us per step (wall clock, stream synced).",
         "order of the processes: " + " ".join(l.split()[3] for l in log), ""]
    ok = True
    for n in TRACERS:
        k = "trc%d" % n
        par = [r["configs"][k]["step_us"] for r in runs["parent"]]
        tre = [r["configs"][k]["step_us"] for r in runs["tree"]]
        spread = max(par) - min(par)
        L.append("%d tracer(s), no tracer moments   parent per alternation: %s   max - min %.1f" % (n, par, spread))
        L.append("%d tracer(s), no tracer moments   tree   per alternation: %s   median %.1f against the parent's median %.1f (%+.2f %%)"
                 % (n, tre, statistics.median(tre), statistics.median(par), (statistics.median(tre) / statistics.median(par) - 1) * 100))
        met = abs(statistics.median(tre) - statistics.median(par)) <= spread
        ok = ok and met
        L.append("   condition (the tree's step within the parent's own max - min): %s" % ("met" if met else "NOT met"))
    again = [r["configs"]["trc4 again"]["step_us"] for r in runs["tree"]]
    L.append("4 tracers, no tracer moments, tree, at the end of the process (step %d; the first figure ends at step %d): %s"
             % (runs["tree"][0]["configs"]["trc4 again"]["last_step"], runs["tree"][0]["configs"]["trc4"]["last_step"], again))
    L.append("")
    L.append("4 tracers:")
    L.append("%-16s %12s %12s %12s %16s" % ("level / stride", "step us", "without us", "vs none us", "one sample us"))
    for level, stride in CONFIGS:
        k = "%d/%d" % (level, stride)
        st = statistics.median(r["configs"][k]["step_us"] for r in runs["tree"])
        base = statistics.median(0.5 * (r["configs"][k]["step_us_without_before"] + r["configs"][k]["step_us_without_after"]) for r in runs["tree"])
        su = statistics.median(r["configs"][k]["sample_us"] for r in runs["tree"])
        L.append("%-16s %12.1f %12.1f %+12.1f %16.1f" % (k, st, base, st - base, su))
    L.append("")
    L.append("(without: the mean of the two blocks without tracer moments timed around the configuration in the same process;")
    L.append(" vs none: the step with tracer moments minus that; one sample: beom_sample_tracer_moments alone, 20 launches between two syncs, wall clock.)")
    L.append("")
    tr, err = traced()
    L.append("The sample launch under rocprofv3 --kernel-trace --stats (a process of its own; median of the launches), next to the floor:")
    L.append("the compulsory words of a cell-layer (hlay, and from level 2 h_u, h_v, once; per tracer q, the references, the sums and Q read")
    L.append("and written, or written only by a first sample) over %d cell-layers at %.1f TB/s (profiles/README.md, the 14+6-stream row)." % (cl, RATE_TBS))
    if tr is None:
        L.append("  not measured: " + err)
    else:
        for (n, level, first), ns in sorted(tr.items()):
            w = words(level, first, n)
            t = statistics.median(ns)
            floor_us = 8.0 * w * cl / (RATE_TBS * 1e12) * 1e6
            L.append("  %d tracer(s)  k_tracer_moments<%d, %-5s>  %3d launches  median %8.1f us  %3d words = %4d B per cell-layer  floor %7.1f us  x%.2f  %.2f TB/s"
                     % (n, level, "true" if first else "false", len(ns), t / 1e3, w, 8 * w, floor_us, t / 1e3 / floor_us, 8.0 * w * cl / t / 1e3))
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
elif a.asm_only:
    print("\n".join(resource_lines()))
else:
    table()
