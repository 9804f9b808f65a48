#!/usr/bin/env python3
"""What the maps (beom_set_maps) cost on one GPU, at 4096 x 4096 x 4 (the headline frame):

  python tools/maps_cost.py [--reps 2] [--steps 40] --parent ab/prev.so [--out profiles/maps_cost.txt]   the alternated table
  python tools/maps_cost.py --one [--steps 40]                          one process: a JSON line
  python tools/maps_cost.py --trace                                     (what the table starts under rocprofv3 --kernel-trace --stats)
  python tools/maps_cost.py --asm-only                                  the `make asm` figures alone (needs no GPU)

(a) The table alternates fresh processes on one box (tools/column_series_cost.py's way): the parent commit's library
(BEOM_HIP_LIB) and this tree's, each stepping WITHOUT maps.  (b) The tree's process then keeps maps at level 1 and 2 for B = 8
and B = 64 at stride 1, and at stride 10 for B = 8; then, with 4 tracers on the handle, at level 3; every configuration is
timed between two blocks without maps in the same process and compared with their mean.  It also times the use case the maps
replace: download(("hlay", "u", "v")) and a numpy block sum.  (c) One more process runs under rocprofv3 --kernel-trace --stats
(no counters in that run) and gives the map launch's own time next to the time its compulsory words (3, 5, 5 + ntrc per
cell-layer) would take at the stream-count ceiling of profiles/r01_stream_count_microbench.txt (its 5-read row, 6.0 TB/s).
Every process that uses the GPU runs under its own `timeout -k 10`, and the first one that fails ends the run.  Without maps
the tree's step has to lie within the parent's own max - min over the alternations; the other figures are reported as they
come."""
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
ap.add_argument("--asm-only", action="store_true")
ap.add_argument("--steps", type=int, default=40)
ap.add_argument("--reps", type=int, default=2)
ap.add_argument("--parent", default=None)
ap.add_argument("--limit", type=int, default=300, help="seconds a process of the table may take (timeout -k 10)")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "maps_cost.txt"))
ap.add_argument("--frame", type=int, nargs=3, default=(4096, 4096, 4), metavar=("LM", "MM", "NLAY"))
a = ap.parse_args()
NTRC = 4
CONFIGS = ((1, 8, 1), (1, 64, 1), (2, 8, 1), (2, 64, 1), (2, 8, 10))      # (level, block, stride), without tracers
CONFIGS3 = ((3, 8, 1), (3, 64, 1))                                         # with NTRC tracers
WORDS = {1: 3, 2: 5, 3: 5 + NTRC}                    # compulsory words read per cell-layer
STREAM_TBS = 6.0                                     # profiles/r01_stream_count_microbench.txt, reads 5 writes 2
TRACE_RECORDS = 5
TRACE_ORDER = [(lv, B) for lv in (1, 2, 3) for B in (8, 64)]


def engine():
    from beom_amd import capi, inputs as I
    from beom_amd.grid import read_input_data
    lm, mm, nlay = a.frame
    p, files = I.case_headline(lm, mm, nlay)
    return capi.Engine(read_input_data(p, files=files))


def tracers(e):
    import numpy as np
    h = np.asarray(e.f.hlay, dtype=np.float64)
    e.set_tracers(NTRC)
    e.upload_tracers(q=np.ascontiguousarray(np.stack([h * (0.5 + 0.1 * t) for t in range(NTRC)])))


def one():
    import numpy as np
    e = engine()
    lm, mm, nlay = a.frame
    has = hasattr(e.lib, "beom_set_maps") and not os.environ.get("BEOM_HIP_LIB")
    out = {"lm": lm, "mm": mm, "nlay": nlay, "lib": "BEOM_HIP_LIB" if os.environ.get("BEOM_HIP_LIB") else "in-tree", "configs": {}}
    tstp = [1]
    maps = [False]

    def steps():
        e.step(tstp[0], 10); tstp[0] += 10
        if maps[0]:
            e.download_maps()
        blocks = []
        for _ in range(3):
            e.sync()
            t = time.perf_counter(); e.step(tstp[0], a.steps); e.sync(); blocks.append((time.perf_counter() - t) / a.steps * 1e6)
            tstp[0] += a.steps
            if maps[0]:
                e.download_maps()                      # (outside the timed part: the recorder holds one call)
        return {"step_us": round(statistics.median(blocks), 1), "step_us_blocks": [round(b, 1) for b in blocks], "last_step": tstp[0] - 1}

    def config(level, B, stride, before):
        e.set_maps(level, B, stride, max(a.steps, 20)); maps[0] = True
        rec = steps()
        rec["step_us_without_before"] = before["step_us"]
        e.sample_maps(); e.sync()
        t = time.perf_counter()
        for _ in range(19):
            e.sample_maps()
        e.sync()
        rec["sample_us"] = round((time.perf_counter() - t) / 19 * 1e6, 1)
        s = e.download_maps()
        rec["count"] = s["count"]
        rec["finite"] = bool(np.isfinite(s["raw"]).all())
        rec["cells"] = float(s["n"][-1].sum())
        del s
        e.set_maps(0); maps[0] = False
        after = steps()
        rec["step_us_without_after"] = after["step_us"]
        out["configs"]["%d/%d/%d" % (level, B, stride)] = rec
        return after

    before = out["configs"]["0"] = steps()
    if has:
        for c in CONFIGS:
            before = config(*c, before)
        out["configs"]["0 again"] = before
        # the use case the maps replace: three fields to the host, block sums there
        e.sync()
        t = time.perf_counter(); st = e.download(("hlay", "u", "v")); out["download_ms"] = round((time.perf_counter() - t) * 1e3, 1)
        f = e.f
        t = time.perf_counter()
        for k in ("hlay", "u", "v"):
            r = np.zeros((nlay, mm + 1, lm + 1))
            r[:, f.subc[1, 1:] - 1, f.subc[0, 1:] - 1] = st[k][:, 1:]
            r = r[:, :(mm + 1) // 8 * 8, :(lm + 1) // 8 * 8].reshape(nlay, (mm + 1) // 8, 8, (lm + 1) // 8, 8).sum(axis=(2, 4))
        out["numpy_block_sum_ms"] = round((time.perf_counter() - t) * 1e3, 1)
        del st, r
        tracers(e)
        before = out["configs"]["0 tracers"] = steps()
        for c in CONFIGS3:
            before = config(*c, before)
    print(json.dumps(out))
    e.close()


def trace():
    """TRACE_RECORDS records per (level, B) of TRACE_ORDER by hand, level 3 with NTRC tracers."""
    e = engine()
    e.step(1, 3)
    for lv, B in TRACE_ORDER:
        if lv == 3 and not e.ntrc:
            tracers(e)
        e.set_maps(lv, B, 1, TRACE_RECORDS)
        for _ in range(TRACE_RECORDS):
            e.sample_maps()
        e.sync()
        e.download_maps()
    e.close()


def traced():
    """{(level, B): [ns, ...]} of the map launches of a --trace process under rocprofv3, in launch order."""
    d = tempfile.mkdtemp(prefix="maps_trace_")
    cmd = ["timeout", "-k", "10", str(a.limit), "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--",
           sys.executable, os.path.abspath(__file__), "--trace", "--frame"] + [str(v) for v in a.frame]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        return None, "rocprofv3 failed (rc %d): %s" % (r.returncode, (r.stderr or r.stdout)[-400:].replace("\n", " | "))
    rows = []
    for fn in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        with open(fn) as fh:
            for row in csv.DictReader(fh):
                if "k_map_blocks" in row.get("Kernel_Name", ""):
                    rows.append((int(row["Start_Timestamp"]), int(row["End_Timestamp"]) - int(row["Start_Timestamp"])))
    rows.sort()
    if len(rows) != TRACE_RECORDS * len(TRACE_ORDER):
        return None, "%d map launches in the trace, %d expected" % (len(rows), TRACE_RECORDS * len(TRACE_ORDER))
    return {c: [ns for _, ns in rows[k * TRACE_RECORDS:(k + 1) * TRACE_RECORDS]] for k, c in enumerate(TRACE_ORDER)}, None


def resource_lines():
    fn = os.path.join(ROOT, "beom_amd", "csrc", "resource_usage.txt")
    if not os.path.exists(fn):
        return ["(no beom_amd/csrc/resource_usage.txt: run `make asm` for the register figures)"]
    txt = open(fn).read()
    L = []
    for blk in re.split(r"(?=remark: [^\n]*Function Name:)", txt):
        m = re.search(r"Function Name: (\S+)", blk)
        if not m or not re.search(r"k_map_blocks|k_column_blocks", m.group(1)):
            continue
        g = lambda k: (re.search(k + r": (\d+)", blk) or [None, "?"])[1]
        L.append("  %-44s VGPRs %s  AGPRs %s  SGPRs %s  spills V/S %s/%s  scratch %s B/lane  LDS %s B  occupancy %s waves/SIMD"
                 % (m.group(1), g("VGPRs"), g("AGPRs"), g("TotalSGPRs"), g("VGPRs Spill"), g("SGPRs Spill"), g(r"ScratchSize \[bytes/lane\]"),
                    g(r"LDS Size \[bytes/block\]"), g(r"Occupancy \[waves/SIMD\]")))
    return L or ["(resource_usage.txt names no k_map_blocks)"]


def asm_section():
    return ["`make asm` figures (gfx950) of the new kernels k_map_blocks<DENSE, LEVEL> next to k_column_blocks<DENSE, LEVEL>, whose",
            "ColumnTree they share (unchanged from the parent commit).  -Rpass-analysis=kernel-resource-usage:"] + resource_lines()


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
            r = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--one", "--steps", str(a.steps),
                                "--frame"] + [str(v) for v in a.frame], env=env, capture_output=True, text=True)
            if r.returncode != 0:                      # nothing more is started on the GPU
                sys.exit("%s failed (rc %d):\n%s\n%s" % (who, r.returncode, r.stdout[-2000:], r.stderr[-2000:]))
            rec = json.loads(r.stdout.strip().splitlines()[-1])
            runs[who].append(rec)
            log.append("# rep %d %-6s %s" % (rep, who, json.dumps(rec)))
            print(log[-1], flush=True)
    lm, mm, nlay = a.frame
    L = ["Maps (beom_set_maps, beom_maps.h): cost at %d x %d x %d            tools/maps_cost.py" % (lm, mm, nlay), "",
         "%d alternations of two fresh processes (parent's library through BEOM_HIP_LIB and this tree's, the order swapped every time), %d steps per timed call,"
         % (a.reps, a.steps), "three calls per configuration, the median of the three; us per step (wall clock, stream synced).",
         "order of the processes: " + " ".join(l.split()[3] for l in log), ""]
    par = [r["configs"]["0"]["step_us"] for r in runs["parent"]]
    tre = [r["configs"]["0"]["step_us"] for r in runs["tree"]]
    L.append("(a) no maps parent per alternation: %s   max - min %.1f" % (par, max(par) - min(par)))
    L.append("(a) no maps tree   per alternation: %s   median %.1f against the parent's median %.1f (%+.2f %%)"
             % (tre, statistics.median(tre), statistics.median(par), (statistics.median(tre) / statistics.median(par) - 1) * 100))
    ok = abs(statistics.median(tre) - statistics.median(par)) <= max(par) - min(par)
    L.append("condition (the tree's step without maps within the parent's own max - min): %s" % ("met" if ok else "NOT met"))
    L.append("")
    L.append("(b) %-22s %12s %12s %12s %16s" % ("level / block / stride", "step us", "without us", "vs none us", "one sample us"))
    for c in CONFIGS + CONFIGS3:
        k = "%d/%d/%d" % c
        st = statistics.median(r["configs"][k]["step_us"] for r in runs["tree"])
        base = statistics.median(0.5 * (r["configs"][k]["step_us_without_before"] + r["configs"][k]["step_us_without_after"]) for r in runs["tree"])
        su = statistics.median(r["configs"][k]["sample_us"] for r in runs["tree"])
        L.append("    %-22s %12.1f %12.1f %+12.1f %16.1f%s" % (k, st, base, st - base, su, "   (%d tracers on the handle)" % NTRC if c[0] == 3 else ""))
    L.append("")
    L.append("(without: the mean of the two blocks without maps timed around the configuration in the same process; vs none: the step")
    L.append(" with maps minus that; one sample: beom_sample_maps alone, 19 launches between two syncs, wall clock.)")
    L.append("the use case without maps: download((\"hlay\", \"u\", \"v\")) %s ms, then a numpy block sum at B = 8 of the three fields %s ms"
             % ([r["download_ms"] for r in runs["tree"]], [r["numpy_block_sum_ms"] for r in runs["tree"]]))
    L.append("")
    tr, err = traced()
    L.append("(c) The launch of one record under rocprofv3 --kernel-trace --stats (a process of its own, no counters; %d records each)," % TRACE_RECORDS)
    L.append("    and its compulsory words at %.1f TB/s:" % STREAM_TBS)
    if tr is None:
        L.append("  not measured: " + err)
    else:
        cl = nlay * (lm + 1) * (mm + 1)
        for (lv, B), ns in tr.items():
            t = statistics.median(ns)
            byts = 8.0 * WORDS[lv] * cl
            L.append("  level %d B %2d  k_map_blocks median %8.1f us  min %8.1f   %d words = %.0f MB compulsory   %.2f TB/s   floor at %.1f TB/s %7.1f us   x%.2f"
                     % (lv, B, t / 1e3, min(ns) / 1e3, WORDS[lv], byts / 1e6, byts / t / 1e3, STREAM_TBS, byts / STREAM_TBS / 1e6,
                        t / 1e3 / (byts / STREAM_TBS / 1e6)))
    L.append("")
    L += asm_section()
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
    print("\n".join(asm_section()))
else:
    table()
