#!/usr/bin/env python3
"""What the tracer column series (beom_set_tracer_column_series) costs on one GPU, at 4096 x 4096 x 4 with 4 tracers:

  python tools/tracer_column_series_cost.py [--reps 3] [--steps 20] --parent ab/prev.so [--parent-asm PARENT/resource_usage.txt] [--out ...]   the table
  python tools/tracer_column_series_cost.py --one [--steps 20]                 one process: a JSON line
  python tools/tracer_column_series_cost.py --trace                            (what the table starts under rocprofv3 --kernel-trace --stats)
  python tools/tracer_column_series_cost.py --asm-only [--parent-asm ...]      the `make asm` figures alone (needs no GPU)

(a) The table alternates fresh processes on one box (tools/column_series_cost.py's way): the parent commit's library
(BEOM_HIP_LIB) and this tree's, each stepping the frame with its tracers WITHOUT any recorder.  (b) The tree's process then
keeps the tracer column series at level 1, 2, 3, at stride 1 and at stride 10; every configuration is timed between two blocks
without a recorder in the same process and compared with their mean.  (c) One more process runs under rocprofv3 --kernel-trace
--stats (no counters in that run) with the tracer series and the tracer column series on one handle, and gives the column
record's launches (blocks + finish, its batches added up) next to the tracer series' row pair at the same level in the same
trace, and next to the time the compulsory words (1 + ntrc per cell-layer at level 1, 3 + ntrc above) would take at the
streaming rate of profiles/README.md's row of as many streams (5 in / 2 out: 6.0 TB/s).  (d) The `make asm` figures of the new
kernels and, given the parent's resource_usage.txt, the comparison of every earlier function's figures.
Every process that uses the GPU runs under its own `timeout -k 10`, and the first one that fails ends the run."""
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
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--parent", default=None)
ap.add_argument("--parent-asm", default=None, help="the parent commit's resource_usage.txt (make asm)")
ap.add_argument("--limit", type=int, default=420, help="seconds a process of the table may take (timeout -k 10)")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tracer_column_series_cost.txt"))
ap.add_argument("--frame", type=int, nargs=3, default=(4096, 4096, 4), metavar=("LM", "MM", "NLAY"))
ap.add_argument("--ntrc", type=int, default=4)
a = ap.parse_args()
CONFIGS = ((1, 1), (2, 1), (3, 1), (1, 10), (2, 10), (3, 10))         # (level, stride)
STREAM_TBS = 6.0                                     # profiles/README.md, the 5-in / 2-out row: 5 resp. 7 streams are read here
TRACE_RECORDS = 5
NEW = r"k_tracer_column_blocks|k_tracer_column_finish"


def engine():
    import numpy as np
    from beom_amd import capi, inputs as I
    from beom_amd.grid import read_input_data
    lm, mm, nlay = a.frame
    p, files = I.case_headline(lm, mm, nlay)
    f = read_input_data(p, files=files)
    e = capi.Engine(f)
    e.set_tracers(a.ntrc)
    h = np.asarray(f.hlay, dtype=np.float64)
    i, j = f.subc[0].astype(np.float64), f.subc[1].astype(np.float64)
    c = np.stack([np.broadcast_to(0.5 + 0.4 * np.sin(0.01 * i + t) * np.cos(0.013 * j), h.shape) for t in range(a.ntrc)])
    e.upload_tracers(q=np.ascontiguousarray(c * h[None]))
    return e


def one():
    import numpy as np
    e = engine()
    lm, mm, nlay = a.frame
    has = hasattr(e.lib, "beom_set_tracer_column_series") and not os.environ.get("BEOM_HIP_LIB")
    out = {"lm": lm, "mm": mm, "nlay": nlay, "ntrc": a.ntrc, "lib": "BEOM_HIP_LIB" if os.environ.get("BEOM_HIP_LIB") else "in-tree", "configs": {}}
    tstp = [1]
    series = [False]

    def steps():
        e.step(tstp[0], 10); tstp[0] += 10
        if series[0]:
            e.sync(); e.download_tracer_column_series()          # (outside the timed part: the recorder holds one call)
        blocks = []
        for _ in range(3):
            e.sync()
            t = time.perf_counter(); e.step(tstp[0], a.steps); e.sync(); blocks.append((time.perf_counter() - t) / a.steps * 1e6)
            tstp[0] += a.steps
            if series[0]:
                e.download_tracer_column_series()
        return {"step_us": round(statistics.median(blocks), 1), "step_us_blocks": [round(b, 1) for b in blocks], "last_step": tstp[0] - 1}

    before = out["configs"]["0"] = steps()
    if has:
        for level, stride in CONFIGS:
            e.set_tracer_column_series(level, stride, max(a.steps, 20)); series[0] = True
            rec = steps()
            rec["step_us_without_before"] = before["step_us"]
            e.sample_tracer_column_series(); e.sync()
            t = time.perf_counter()
            for _ in range(9):
                e.sample_tracer_column_series()
            e.sync()
            rec["sample_us"] = round((time.perf_counter() - t) / 9 * 1e6, 1)
            s = e.download_tracer_column_series()
            rec["count"] = s["count"]
            rec["sums_finite"] = bool(np.isfinite(s["inv"]).all() and np.isfinite(s["var"]).all())
            del s
            e.set_tracer_column_series(0); series[0] = False
            before = steps()
            rec["step_us_without_after"] = before["step_us"]
            out["configs"]["%d/%d" % (level, stride)] = rec
        out["configs"]["0 again"] = before
    print(json.dumps(out))
    e.close()


def trace():
    """TRACE_RECORDS records of the tracer series and of the tracer column series at level 1, 2, 3, both recorders on one
    handle: every sampled step launches the row pair, then the column pair."""
    e = engine()
    e.step(1, 3)
    t = 4
    for level in (1, 2, 3):
        e.set_tracer_series(level, 1, TRACE_RECORDS)
        e.set_tracer_column_series(level, 1, TRACE_RECORDS)
        e.step(t, TRACE_RECORDS)
        t += TRACE_RECORDS
        e.sync()
        e.download_tracer_series(); e.download_tracer_column_series()
    e.close()


KERNELS = r"k_tracer_(series_rows|series_chunks|column_blocks|column_finish)(?:<\s*(?:true|false|\(bool\)[01])\s*,\s*(?:\(int\))?(\d))?"


def traced():
    """{(family, level): {kernel: total ns}} of the two recorders' launches of a --trace process under rocprofv3.  The first
    kernel of a pair names its level; the second takes the level of the launch of its family before it."""
    d = tempfile.mkdtemp(prefix="tracer_column_series_trace_")
    cmd = ["timeout", "-k", "10", str(a.limit), "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--",
           sys.executable, os.path.abspath(__file__), "--trace", "--ntrc", str(a.ntrc), "--frame"] + [str(v) for v in a.frame]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        return None, "rocprofv3 failed (rc %d): %s" % (r.returncode, (r.stderr or r.stdout)[-400:].replace("\n", " | "))
    rows = []
    for fn in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        with open(fn) as fh:
            for row in csv.DictReader(fh):
                name = row.get("Kernel_Name", "")
                m = re.search(KERNELS, name)
                if m:
                    lv = m.group(2) or (re.search(r"k_tracer_(?:series_rows|column_blocks)ILb[01]ELi(\d)E", name) or [None, None])[1]
                    rows.append((int(row["Start_Timestamp"]), m.group(1), lv, int(row["End_Timestamp"]) - int(row["Start_Timestamp"])))
    rows.sort()
    out, level = {}, {"row": None, "col": None}
    for _, name, lv, ns in rows:
        fam = "row" if name.startswith("series") else "col"
        if lv is not None:
            level[fam] = int(lv)
        if level[fam] is None:
            continue
        k = out.setdefault((fam, level[fam]), {})
        k[name] = k.get(name, 0) + ns
        k[name + " launches"] = k.get(name + " launches", 0) + 1
    if not out:
        return None, "the trace names none of the kernels (%d rows)" % len(rows)
    return out, None


def _blocks(fn):
    out, order = {}, []
    for blk in re.split(r"(?=remark: [^\n]*Function Name:)", open(fn).read()):
        m = re.search(r"Function Name: (\S+)", blk)
        if not m:
            continue
        g = lambda k: (re.search(k + r": (\d+)", blk) or [None, "?"])[1]
        out[m.group(1)] = (g("VGPRs"), g("AGPRs"), g("TotalSGPRs"), g("VGPRs Spill"), g("SGPRs Spill"), g(r"ScratchSize \[bytes/lane\]"),
                           g(r"LDS Size \[bytes/block\]"), g(r"Occupancy \[waves/SIMD\]"))
        order.append(m.group(1))
    return out, order


def asm_section():
    fn = os.path.join(ROOT, "beom_amd", "csrc", "resource_usage.txt")
    if not os.path.exists(fn):
        return ["(no beom_amd/csrc/resource_usage.txt: run `make asm` for the register figures)"]
    mine, order = _blocks(fn)
    L = ["`make asm` figures (gfx950, -Rpass-analysis=kernel-resource-usage) of the new kernels and of the tracer series' row pair:"]
    for k in order:
        if re.search(NEW + r"|k_tracer_series_rows|k_tracer_series_chunks", k):
            L.append("  %-62s VGPRs %s  AGPRs %s  SGPRs %s  spills V/S %s/%s  scratch %s B/lane  LDS %s B  occupancy %s waves/SIMD" % ((k,) + mine[k]))
    new = [k for k in order if re.search(NEW, k)]
    L.append("new kernels: %d, the last %d functions of the listing: %s" % (len(new), len(new), order[-len(new):] == new if new else False))
    if a.parent_asm and os.path.exists(a.parent_asm):
        par, porder = _blocks(a.parent_asm)
        diff = [k for k in porder if mine.get(k) != par[k]]
        L.append("against the parent's listing: %d earlier functions, %d with other figures%s; their order kept: %s"
                 % (len(porder), len(diff), (" (" + ", ".join(diff[:8]) + ")") if diff else "", order[:len(porder)] == porder))
    else:
        L.append("(no --parent-asm: the earlier functions' figures are not compared)")
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
            r = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--one", "--steps", str(a.steps),
                                "--ntrc", str(a.ntrc), "--frame"] + [str(v) for v in a.frame], env=env, capture_output=True, text=True)
            if r.returncode != 0:                      # nothing more is started on the GPU
                sys.exit("%s failed (rc %d):\n%s\n%s" % (who, r.returncode, r.stdout[-2000:], r.stderr[-2000:]))
            rec = json.loads(r.stdout.strip().splitlines()[-1])
            runs[who].append(rec)
            log.append("# rep %d %-6s %s" % (rep, who, json.dumps(rec)))
            print(log[-1], flush=True)
    lm, mm, nlay = a.frame
    import socket
    L = ["Tracer column series (beom_set_tracer_column_series, beom_tracer_column_series.h): cost at %d x %d x %d, %d tracers      tools/tracer_column_series_cost.py"
         % (lm, mm, nlay, a.ntrc), "box: %s" % (socket.gethostname() or "?"), "",
         "%d alternations of two fresh processes (parent's library through BEOM_HIP_LIB and this tree's, the order swapped every time), %d steps per timed call,"
         % (a.reps, a.steps), "three calls per configuration, the median of the three; us per step (wall clock, stream synced).",
         "order of the processes: " + " ".join(l.split()[3] for l in log), ""]
    par = [r["configs"]["0"]["step_us"] for r in runs["parent"]]
    tre = [r["configs"]["0"]["step_us"] for r in runs["tree"]]
    L.append("(a) no recorder parent per alternation: %s   max - min %.1f" % (par, max(par) - min(par)))
    L.append("(a) no recorder tree   per alternation: %s   median %.1f against the parent's median %.1f (%+.2f %%)"
             % (tre, statistics.median(tre), statistics.median(par), (statistics.median(tre) / statistics.median(par) - 1) * 100))
    gap = statistics.median(tre) - statistics.median(par)
    ok = abs(gap) <= max(par) - min(par)
    L.append("condition (the tree's step without a recorder within the parent's own max - min): %s; the tree's own max - min %.1f"
             % ("met" if ok else "NOT met, the tree's median is %.1f us %s the parent's" % (abs(gap), "above" if gap > 0 else "below"), max(tre) - min(tre)))
    L.append("no recorder tree, at the end of the process: %s" % [r["configs"]["0 again"]["step_us"] for r in runs["tree"]])
    L.append("")
    L.append("(b) %-12s %12s %12s %12s %16s" % ("level / stride", "step us", "without us", "vs none us", "one sample us"))
    for level, stride in CONFIGS:
        k = "%d/%d" % (level, stride)
        st = statistics.median(r["configs"][k]["step_us"] for r in runs["tree"])
        base = statistics.median(0.5 * (r["configs"][k]["step_us_without_before"] + r["configs"][k]["step_us_without_after"]) for r in runs["tree"])
        su = statistics.median(r["configs"][k]["sample_us"] for r in runs["tree"])
        L.append("    %-12s %12.1f %12.1f %+12.1f %16.1f" % (k, st, base, st - base, su))
    L.append("")
    L.append("(without: the mean of the two blocks without a recorder timed around the configuration in the same process; vs none: the step with the")
    L.append(" recorder minus that; one sample: beom_sample_tracer_column_series alone, 9 launches between two syncs, wall clock.)")
    L.append("")
    tr, err = traced()
    L.append("(c) The launches of one record under rocprofv3 --kernel-trace --stats (a process of its own, no counters; mean over %d records, a record's" % TRACE_RECORDS)
    L.append("    batches added up), the tracer series' row pair at the same level in the same trace, and the compulsory words at %.1f TB/s:" % STREAM_TBS)
    if tr is None:
        L.append("  not measured: " + err)
    else:
        cl = nlay * (lm + 1) * (mm + 1)
        pair = {}
        for (fam, lv), ks in sorted(tr.items()):
            names = [k for k in ks if not k.endswith(" launches")]
            pair[(fam, lv)] = sum(ks[k] for k in names) / TRACE_RECORDS
            for k in names:
                L.append("  %s level %d  k_tracer_%-16s %3d launches  %9.1f us per record" % (fam, lv, k, ks[k + " launches"], ks[k] / TRACE_RECORDS / 1e3))
        for (fam, lv), ns in sorted(pair.items()):
            w = (1 if lv == 1 else 3) + a.ntrc
            byts = 8.0 * w * cl
            L.append("  %s level %d  pair %9.1f us   %d words = %.0f MB compulsory   %.2f TB/s   floor at %.1f TB/s %7.1f us   x%.2f"
                     % (fam, lv, ns / 1e3, w, byts / 1e6, byts / ns / 1e3, STREAM_TBS, byts / STREAM_TBS / 1e6, ns / 1e3 / (byts / STREAM_TBS / 1e6)))
        for lv in (1, 2, 3):
            if ("row", lv) in pair and ("col", lv) in pair:
                L.append("  level %d: column pair / row pair = %.2f" % (lv, pair[("col", lv)] / pair[("row", lv)]))
    L.append("")
    L.append("(d) " + asm_section()[0])
    L += asm_section()[1:]
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
