#!/usr/bin/env python3
"""What the column series (beom_set_column_series) costs on one GPU, at 4096 x 4096 x 4 (the headline frame):

  python tools/column_series_cost.py [--reps 3] [--steps 40] --parent ab/prev.so [--out profiles/column_series_cost.txt]   the alternated table
  python tools/column_series_cost.py --one [--steps 40]                                                                    one process: a JSON line
  python tools/column_series_cost.py --trace                          (what the table starts under rocprofv3 --kernel-trace --stats)
  python tools/column_series_cost.py --asm-only [--out ...]           the `make asm` figures alone (needs no GPU)

(a) The table alternates fresh processes on one box (tools/series_cost.py's way): the parent commit's library (BEOM_HIP_LIB)
and this tree's, each stepping WITHOUT any recorder.  (b) The tree's process then keeps the column series at level 1 and level
2, at stride 1 and at stride 10; every configuration is timed between two blocks without a recorder in the same process (the
step time drifts with the step number) and compared with their mean.  (c) One more process runs under rocprofv3 --kernel-trace
--stats (no counters in that run) and gives the column record's launches' own times next to the ROW series' launches at the
same level in the same trace, and next to the time the compulsory words (3 per cell-layer at level 1: hlay, u, v; 5 at level
2: and h_u, h_v) would take at the streaming rate of profiles/README.md's 14+6-stream row, 5.6 TB/s.
Every process that uses the GPU runs under its own `timeout -k 10`, and the first one that fails ends the run.  Without a
recorder the tree's step has to lie within the parent's own max - min over the alternations; the other figures are reported as
they come."""
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
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--parent", default=None)
ap.add_argument("--limit", type=int, default=420, help="seconds a process of the table may take (timeout -k 10)")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "column_series_cost.txt"))
ap.add_argument("--frame", type=int, nargs=3, default=(4096, 4096, 4), metavar=("LM", "MM", "NLAY"))
a = ap.parse_args()
CONFIGS = ((1, 1), (2, 1), (1, 10), (2, 10))         # (level, stride)
WORDS = {1: 3, 2: 5}                                 # compulsory words per cell-layer: hlay, u, v | and h_u, h_v
STREAM_TBS = 5.6                                     # profiles/README.md, the 14+6-stream row
TRACE_RECORDS = 7


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
    has = hasattr(e.lib, "beom_set_column_series") and not os.environ.get("BEOM_HIP_LIB")
    out = {"lm": lm, "mm": mm, "nlay": nlay, "lib": "BEOM_HIP_LIB" if os.environ.get("BEOM_HIP_LIB") else "in-tree", "configs": {}}
    tstp = [1]
    series = [False]

    def call(n):
        e.step(tstp[0], n); tstp[0] += n
        if series[0]:
            e.sync()
            return e.download_column_series()          # (outside the timed part: the recorder holds one call)
        return None

    def steps():
        call(10)
        blocks = []
        for _ in range(3):
            e.sync()
            t = time.perf_counter(); e.step(tstp[0], a.steps); e.sync(); blocks.append((time.perf_counter() - t) / a.steps * 1e6)
            tstp[0] += a.steps
            if series[0]:
                e.download_column_series()
        return {"step_us": round(statistics.median(blocks), 1), "step_us_blocks": [round(b, 1) for b in blocks], "last_step": tstp[0] - 1}

    before = out["configs"]["0"] = steps()
    if has:
        for level, stride in CONFIGS:
            e.set_column_series(level, stride, max(a.steps, 20)); series[0] = True
            rec = steps()
            rec["step_us_without_before"] = before["step_us"]
            e.sample_column_series(); e.sync()
            t = time.perf_counter()
            for _ in range(19):
                e.sample_column_series()
            e.sync()
            rec["sample_us"] = round((time.perf_counter() - t) / 19 * 1e6, 1)
            s = e.download_column_series()
            rec["count"] = s["count"]
            rec["finite"] = bool(np.isfinite(s["cols"]).all())
            raw = e.integrals()["raw"]
            pos = np.array([k % 4 != 3 or k == 4 * nlay for k in range(4 * nlay + 1)])      # (circ cancels: no scale of its own)
            rec["total_vs_integrals_rel"] = float(np.max(np.abs(s["total"][-1] - raw)[pos] / np.abs(raw)[pos]))
            del s
            e.set_column_series(0); series[0] = False
            before = steps()
            rec["step_us_without_after"] = before["step_us"]
            out["configs"]["%d/%d" % (level, stride)] = rec
        out["configs"]["0 again"] = before
    print(json.dumps(out))
    e.close()


def trace():
    """TRACE_RECORDS records of the row series and of the column series at level 1, then at level 2, both recorders on one
    handle: every sampled step launches the row pair, then the column pair."""
    e = engine()
    e.step(1, 3)
    t = 4
    for level in (1, 2):
        e.set_series(level, 1, TRACE_RECORDS)
        e.set_column_series(level, 1, TRACE_RECORDS)
        e.step(t, TRACE_RECORDS)
        t += TRACE_RECORDS
        e.sync()
        e.download_series(); e.download_column_series()
    e.close()


KERNELS = r"k_(integral_rows|series_rows|integral_chunks|column_blocks|column_finish)"


def traced():
    """{(who, name): [ns, ...]} of the two recorders' launches of a --trace process under rocprofv3, in launch order."""
    d = tempfile.mkdtemp(prefix="column_series_trace_")
    cmd = ["timeout", "-k", "10", str(a.limit), "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--",
           sys.executable, os.path.abspath(__file__), "--trace", "--frame"] + [str(v) for v in a.frame]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        return None, "rocprofv3 failed (rc %d): %s" % (r.returncode, (r.stderr or r.stdout)[-400:].replace("\n", " | "))
    rows = []
    for fn in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        with open(fn) as fh:
            for row in csv.DictReader(fh):
                m = re.search(KERNELS, row.get("Kernel_Name", ""))
                if m:
                    rows.append((int(row["Start_Timestamp"]), m.group(1), int(row["End_Timestamp"]) - int(row["Start_Timestamp"])))
    rows.sort()
    # a record of the column series is `batches` launches of each of its kernels: they are added up per record
    per = {}
    for _, name, ns in rows:
        per.setdefault(name, []).append(ns)
    out = {}
    nb = {n: len(per.get(n, [])) // (2 * TRACE_RECORDS) for n in ("column_blocks", "column_finish")}
    for n, b in nb.items():
        if b < 1:
            continue
        recs = [sum(per[n][k * b:(k + 1) * b]) for k in range(2 * TRACE_RECORDS)]
        out[("col level 1", n + " x%d" % b)] = recs[:TRACE_RECORDS]
        out[("col level 2", n + " x%d" % b)] = recs[TRACE_RECORDS:]
    out[("row level 1", "integral_rows")] = per.get("integral_rows", [])
    out[("row level 2", "series_rows")] = per.get("series_rows", [])
    ch = per.get("integral_chunks", [])
    out[("row level 1", "integral_chunks")] = ch[:TRACE_RECORDS]
    out[("row level 2", "integral_chunks")] = ch[TRACE_RECORDS:]
    return {k: v for k, v in out.items() if v}, None


def resource_lines():
    fn = os.path.join(ROOT, "beom_amd", "csrc", "resource_usage.txt")
    if not os.path.exists(fn):
        return ["(no beom_amd/csrc/resource_usage.txt: run `make asm` for the register figures)"]
    txt = open(fn).read()
    L = []
    for blk in re.split(r"(?=remark: [^\n]*Function Name:)", txt):
        m = re.search(r"Function Name: (\S+)", blk)
        if not m or not re.search(r"k_column_blocks|k_column_finish|k_series_rows|k_integral_rows|k_integral_chunks", m.group(1)):
            continue
        g = lambda k: (re.search(k + r": (\d+)", blk) or [None, "?"])[1]
        L.append("  %-48s VGPRs %s  AGPRs %s  SGPRs %s  spills V/S %s/%s  scratch %s B/lane  LDS %s B  occupancy %s waves/SIMD"
                 % (m.group(1), g("VGPRs"), g("AGPRs"), g("TotalSGPRs"), g("VGPRs Spill"), g("SGPRs Spill"), g(r"ScratchSize \[bytes/lane\]"),
                    g(r"LDS Size \[bytes/block\]"), g(r"Occupancy \[waves/SIMD\]")))
    return L or ["(resource_usage.txt names no k_column_blocks)"]


def listing_lines():
    """The same kernels' `Kernel info` blocks of the assembly listing, and what their bodies are made of."""
    fn = os.path.join(ROOT, "beom_amd", "csrc", "beom_engine.s")
    if not os.path.exists(fn):
        return ["(no beom_amd/csrc/beom_engine.s: run `make asm`)"]
    txt = open(fn).read()
    L = []
    for m in re.finditer(r"^(_Z\d+k_(?:column_blocks|column_finish|series_rows|integral_rows|integral_chunks)\S*):.*?; Kernel info:\n(.*?)\n; COMPUTE_PGM", txt, re.S | re.M):
        body, info = m.group(0), m.group(2)
        g = lambda k: (re.search(k + r":? =? ?(\d+)", info) or [None, "?"])[1]
        n = lambda pat: len(re.findall(pat, body))
        L.append("  %-48s NumVgprs %s  NumAgprs %s  TotalNumSgprs %s  ScratchSize %s  LDSByteSize %s  Occupancy %s  code %s B"
                 % (m.group(1), g("NumVgprs"), g("NumAgprs"), g("TotalNumSgprs"), g("ScratchSize"), g("LDSByteSize"), g("Occupancy"), g("codeLenInByte")))
        L.append("  %-48s global_load %d  global_store %d  ds_bpermute_b32 %d  ds_read/write %d  s_barrier %d  v_div_fmas_f64 %d  v_add_f64 %d  v_mul_f64 %d  s_waitcnt %d  scratch_ %d"
                 % ("", n(r"\tglobal_load"), n(r"\tglobal_store"), n(r"\tds_bpermute_b32"), n(r"\tds_(?:read|write)"), n(r"\ts_barrier"), n(r"\tv_div_fmas_f64"),
                    n(r"\tv_add_f64"), n(r"\tv_mul_f64"), n(r"\ts_waitcnt"), n(r"\tscratch_")))
    return L or ["(beom_engine.s names no k_column_blocks)"]


def asm_section():
    return ["`make asm` figures (gfx950) of the new kernels k_column_blocks<DENSE, LEVEL> and k_column_finish next to the row series'",
            "kernels (those unchanged from the parent commit).  -Rpass-analysis=kernel-resource-usage:"] + resource_lines() + \
           ["the assembly listing (beom_engine.s), per kernel its `Kernel info` and the instructions of its body (both bodies of a",
            "dense kernel, interior and general, counted together):"] + listing_lines()


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
    import socket
    box = socket.gethostname() or "?"
    L = ["Column series (beom_set_column_series, beom_column_series.h): cost at %d x %d x %d            tools/column_series_cost.py" % (lm, mm, nlay),
         "box: %s" % box, "",
         "%d alternations of two fresh processes (parent's library through BEOM_HIP_LIB and this tree's, the order swapped every time), %d steps per timed call,"
         % (a.reps, a.steps), "three calls per configuration, the median of the three; us per step (wall clock, stream synced).",
         "order of the processes: " + " ".join(l.split()[3] for l in log), ""]
    par = [r["configs"]["0"]["step_us"] for r in runs["parent"]]
    tre = [r["configs"]["0"]["step_us"] for r in runs["tree"]]
    L.append("(a) no recorder parent per alternation: %s   max - min %.1f" % (par, max(par) - min(par)))
    L.append("(a) no recorder tree   per alternation: %s   median %.1f against the parent's median %.1f (%+.2f %%)"
             % (tre, statistics.median(tre), statistics.median(par), (statistics.median(tre) / statistics.median(par) - 1) * 100))
    spread = max(par) - min(par)
    ok = abs(statistics.median(tre) - statistics.median(par)) <= spread
    L.append("condition (the tree's step without a recorder within the parent's own max - min): %s" % ("met" if ok else "NOT met"))
    again = [r["configs"]["0 again"]["step_us"] for r in runs["tree"]]
    L.append("no recorder tree, at the end of the process (step %d; the first figure ends at step %d): %s"
             % (runs["tree"][0]["configs"]["0 again"]["last_step"], runs["tree"][0]["configs"]["0"]["last_step"], again))
    L.append("")
    L.append("(b) %-12s %12s %12s %12s %16s" % ("level / stride", "step us", "without us", "vs none us", "one sample us"))
    for level, stride in CONFIGS:
        k = "%d/%d" % (level, stride)
        st = statistics.median(r["configs"][k]["step_us"] for r in runs["tree"])
        base = statistics.median(0.5 * (r["configs"][k]["step_us_without_before"] + r["configs"][k]["step_us_without_after"]) for r in runs["tree"])
        su = statistics.median(r["configs"][k]["sample_us"] for r in runs["tree"])
        L.append("    %-12s %12.1f %12.1f %+12.1f %16.1f" % (k, st, base, st - base, su))
    L.append("")
    L.append("(without: the mean of the two blocks without a recorder timed around the configuration in the same process;")
    L.append(" vs none: the step with the column series minus that; one sample: beom_sample_column_series alone, 19 launches between two syncs, wall clock.)")
    L.append("the tree over the columns of the last record against Engine.integrals() (another order of summation), largest relative difference of vol, ke, ens, eta2: %.2e"
             % max(r["configs"]["%d/%d" % c]["total_vs_integrals_rel"] for r in runs["tree"] for c in CONFIGS))
    L.append("")
    tr, err = traced()
    L.append("(c) The launches of one record under rocprofv3 --kernel-trace --stats (a process of its own, no counters; median over the records;")
    L.append("    a column record's batches added up), the row series' pair at the same level in the same trace, and the compulsory words at %.1f TB/s:" % STREAM_TBS)
    if tr is None:
        L.append("  not measured: " + err)
    else:
        cl = nlay * (lm + 1) * (mm + 1)
        pair = {}
        for (who, name), ns in sorted(tr.items()):
            t = statistics.median(ns)
            pair[who] = pair.get(who, 0.0) + t
            L.append("  %-12s k_%-20s %3d records  median %8.1f us  min %8.1f" % (who, name, len(ns), t / 1e3, min(ns) / 1e3))
        for who, w in (("row level 1", 3), ("col level 1", 3), ("row level 2", 5), ("col level 2", 5)):
            if who in pair:
                byts = 8.0 * w * cl
                L.append("  %-12s pair %8.1f us   %d words = %.0f MB compulsory   %.2f TB/s   floor at %.1f TB/s %7.1f us   x%.2f"
                         % (who, pair[who] / 1e3, w, byts / 1e6, byts / pair[who] / 1e3, STREAM_TBS, byts / STREAM_TBS / 1e6,
                            pair[who] / 1e3 / (byts / STREAM_TBS / 1e6)))
        for lv in (1, 2):
            if "row level %d" % lv in pair and "col level %d" % lv in pair:
                L.append("  level %d: column pair / row pair = %.2f" % (lv, pair["col level %d" % lv] / pair["row level %d" % lv]))
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
