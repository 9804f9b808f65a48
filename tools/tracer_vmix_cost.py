#!/usr/bin/env python3
"""What the tracers' vertical mixing launch (beom_set_tracer_vmixing) costs on one GPU, at 4096 x 4096 x 4 (the headline
frame of tools/bench_case.py); modelled on tools/tracer_mix_cost.py:

  python tools/tracer_vmix_cost.py [--reps 2] [--steps 40] --parent ab/prev.so [--parent-asm FILE] [--out profiles/tracer_vmix_cost.txt]
  python tools/tracer_vmix_cost.py --one [--steps 40]                                                      one process: a JSON line
  python tools/tracer_vmix_cost.py --trace                           (what the table starts under rocprofv3 --kernel-trace --stats)
  python tools/tracer_vmix_cost.py --launch-only                                        the rocprofv3 section alone: one process
  python tools/tracer_vmix_cost.py --asm-only [--parent-asm FILE]                                          the listing comparison

The table alternates fresh processes on one box (tools/ab.sh's way): the parent commit's library (BEOM_HIP_LIB) and this
tree's, each stepping with 1 and with 4 tracers and WITHOUT vertical mixing (and without lateral mixing); the tree's process
then switches the vertical mixing on (kappa_v = 1e-4 m2/s on every tracer and interface), times the step, switches it off
and times the step again.
Per configuration: the median step time (wall clock over --steps steps per call, stream synced on both sides, three blocks).
One more process runs under rocprofv3 --kernel-trace --stats and gives the launch's own time per tracer count, next to the
floor of the compulsory words, (1 + 2 ntrc) x 8 B per cell-layer, at the streaming rates of profiles/README.md.  Without
mixing the tree's step has to lie within the parent's own max - min over the alternations; the other figures are reported
as they come.  `python bench.py` runs once per library (no handle of it carries tracers).  `make asm` figures
(resource_usage.txt) of the new kernel are appended, and with --parent-asm (the parent's resource_usage.txt) the comparison
of every earlier kernel's figures."""
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
ap.add_argument("--asm-only", action="store_true", help="print the make asm comparison alone (no GPU)")
ap.add_argument("--launch-only", action="store_true", help="the rocprofv3 section alone: one process")
ap.add_argument("--no-bench", action="store_true", help="leave out the two runs of bench.py")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tracer_vmix_cost.txt"))
ap.add_argument("--frame", type=int, nargs=3, default=(4096, 4096, 4), metavar=("LM", "MM", "NLAY"))
a = ap.parse_args()
TRACERS = (1, 4)
RATES_TBS = (5.4, 6.0)                               # the streaming rates of profiles/README.md


def engine():
    from beom_amd import capi, inputs as I
    from beom_amd.grid import read_input_data
    lm, mm, nlay = a.frame
    p, files = I.case_headline(lm, mm, nlay)
    return capi.Engine(read_input_data(p, files=files))


def mixing_on(e):
    e.set_tracer_vertical_mixing(1.0e-4)


def one():
    import numpy as np
    e = engine()
    lm, mm, nlay = a.frame
    has = hasattr(e.lib, "beom_set_tracer_vmixing")
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
        out["configs"]["trc%d off" % n] = steps()
        if has:
            mixing_on(e)
            rec = out["configs"]["trc%d on" % n] = steps()
            e.sync()
            t = time.perf_counter()
            for _ in range(20):
                e.update_tracer_vertical_mixing()
            e.sync()
            rec["launch_us"] = round((time.perf_counter() - t) / 20 * 1e6, 1)
            rec["launches"] = e.info("tracer_vmix_launches")
            rec["finite"] = bool(np.isfinite(e.download_tracers()["q"]).all())
            e.set_tracer_vertical_mixing(None)
            assert e.info("tracer_vmixing") == 0
            out["configs"]["trc%d off again" % n] = steps()
    print(json.dumps(out))
    e.close()


def trace():
    """Ten steps with mixing per tracer count: the kernel trace holds the launches' own times, in this order."""
    import numpy as np
    e = engine()
    for n in TRACERS:
        e.set_tracers(n)
        e.set_concentration(np.linspace(0.25, 1.0, n)[:, None, None])
        mixing_on(e)
        e.step(1, 10)
        e.sync()
    e.close()


def traced():
    """{ntrc: [ns, ...]} of the k_tracer_vmix launches of a --trace process under rocprofv3: 10 per tracer count, in order."""
    d = tempfile.mkdtemp(prefix="tracer_vmix_trace_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
           "--trace", "--frame"] + [str(v) for v in a.frame]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        return None, "rocprofv3 failed (rc %d): %s" % (r.returncode, (r.stderr or r.stdout)[-400:].replace("\n", " | "))
    rows = []
    for fn in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        with open(fn) as fh:
            for row in csv.DictReader(fh):
                if "k_tracer_vmix" in row.get("Kernel_Name", ""):
                    rows.append((int(row["Start_Timestamp"]), int(row["End_Timestamp"]) - int(row["Start_Timestamp"])))
    rows.sort()
    out = {}
    for k, (_, ns) in enumerate(rows):
        out.setdefault(TRACERS[min(k // 10, len(TRACERS) - 1)], []).append(ns)
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
    L = ["`make asm` figures of the new kernel's instantiations (gfx950, -O3 -ffp-contract=off):"]
    for name, v in sorted(mine.items(), key=lambda kv: ("CellGather" in kv[0], int((re.search(r"Li(\d+)EE", kv[0]) or [0, 0])[1]))):
        if "k_tracer_vmix" in name:
            short = "k_tracer_vmix<%s, %s>" % ("CellGather" if "CellGather" in name else "CellDense", re.search(r"Li(\d+)EE", name).group(1))
            L.append("  %-30s SGPRs %3s  VGPRs %3s  AGPRs %s  spills S/V %s/%s  scratch %s B/lane  LDS %s B  occupancy %s waves/SIMD"
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
        L.append("k_tracer_vmix: %s." % ("yes" if all("k_tracer_vmix" in n for n in new) else "NO: " + ", ".join(n for n in new if "k_tracer_vmix" not in n)))
        for n in moved:
            L.append("  MOVED %s: parent %s, tree %s" % (n, par[n], mine.get(n)))
    else:
        L.append("(no --parent-asm listing: the earlier kernels' figures were not compared)")
    return L


def bench_lines():
    """python bench.py once per library: the JSON line of each."""
    L = ["python bench.py --gpus 1 --steps 50 --warmup 10 (no handle of it carries tracers), the parent's library, then this tree's:"]
    for who in ("parent", "tree"):
        env = dict(os.environ)
        env.pop("BEOM_HIP_LIB", None)
        if who == "parent":
            env["BEOM_HIP_LIB"] = os.path.abspath(a.parent)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "50", "--warmup", "10"],
                           env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
        if r.returncode != 0:
            sys.exit("bench.py (%s) failed (rc %d):\n%s\n%s" % (who, r.returncode, r.stdout[-2000:], r.stderr[-2000:]))
        line = [l for l in r.stdout.strip().splitlines() if l.startswith("{")][-1]
        L.append("  %-6s %s" % (who, line))
        print(L[-1], flush=True)
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
    L = ["Vertical tracer mixing (k_tracer_vmix, beom_tracer_vmix.h): cost at %d x %d x %d            tools/tracer_vmix_cost.py" % (lm, mm, nlay), "",
         "%d alternations of two fresh processes (parent's library through BEOM_HIP_LIB and this tree's, the order swapped every time), %d steps per timed call,"
         % (a.reps, a.steps), "three calls per configuration, the median of the three; us per step (wall clock, stream synced).",
         "order of the processes: " + " ".join(l.split()[3] for l in log), ""]
    for n in TRACERS:
        k = "trc%d off" % n
        par = [r["configs"][k]["step_us"] for r in runs["parent"]]
        tre = [r["configs"][k]["step_us"] for r in runs["tree"]]
        spread = max(par) - min(par)
        L.append("%d tracer(s), no vmix   parent per alternation: %s   max - min %.1f" % (n, par, spread))
        L.append("%d tracer(s), no vmix   tree   per alternation: %s   median %.1f against the parent's median %.1f (%+.2f %%)"
                 % (n, tre, statistics.median(tre), statistics.median(par), (statistics.median(tre) / statistics.median(par) - 1) * 100))
        met = abs(statistics.median(tre) - statistics.median(par)) <= spread
        L.append("   condition (the tree's step within the parent's own max - min): %s" % ("met" if met else "NOT met"))
    L.append("")
    L.append("%-10s %12s %12s %12s %12s %16s" % ("tracers", "off us", "on us", "off again us", "on - off us", "one launch us"))
    for n in TRACERS:
        off = statistics.median(r["configs"]["trc%d off" % n]["step_us"] for r in runs["tree"])
        on = statistics.median(r["configs"]["trc%d on" % n]["step_us"] for r in runs["tree"])
        again = statistics.median(r["configs"]["trc%d off again" % n]["step_us"] for r in runs["tree"])
        lu = statistics.median(r["configs"]["trc%d on" % n]["launch_us"] for r in runs["tree"])
        L.append("%-10d %12.1f %12.1f %12.1f %+12.1f %16.1f" % (n, off, on, again, on - 0.5 * (off + again), lu))
    L.append("")
    L.append("(off / off again: the step without vertical mixing before and after, in the same process; on - off: against their mean; one launch:")
    L.append(" beom_update_tracer_vmixing alone, 20 launches between two syncs, wall clock.)")
    L.append("")
    tr, err = traced()
    L.append("The launch under rocprofv3 --kernel-trace --stats (a process of its own; median of the launches), next to the floor: the")
    L.append("compulsory words of a cell-layer (hlay once; per tracer q read and written in place: 1 + 2 ntrc) over %d cell-layers at" % cl)
    L.append("%.1f and %.1f TB/s (profiles/README.md)." % RATES_TBS)
    if tr is None:
        L.append("  not measured: " + err)
    else:
        for n, ns in sorted(tr.items()):
            w = 1 + 2 * n
            t = statistics.median(ns)
            lo, hi = (8.0 * w * cl / (r * 1e12) * 1e6 for r in reversed(RATES_TBS))
            L.append("  %d tracer(s)  k_tracer_vmix  %3d launches  median %8.1f us  %2d words = %3d B per cell-layer  floor %6.1f-%6.1f us  x%.2f of the upper floor  %.2f TB/s"
                     % (n, len(ns), t / 1e3, w, 8 * w, lo, hi, t / 1e3 / hi, 8.0 * w * cl / t / 1e3))
    L.append("")
    if not a.no_bench:
        L += bench_lines()
        L.append("")
    L += resource_lines()
    L.append("")
    L += log
    text = "\n".join(L) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)
    print(text)


if a.launch_only:
    tr, err = traced()
    print(err if tr is None else "\n".join("%d tracer(s): k_tracer_vmix median %.1f us over %d launches" % (n, statistics.median(ns) / 1e3, len(ns))
                                           for n, ns in sorted(tr.items())))
elif a.one:
    one()
elif a.trace:
    trace()
elif a.asm_only:
    print("\n".join(resource_lines()))
else:
    table()
