#!/usr/bin/env python3
"""What the tracer series (beom_set_tracer_series) costs on one GPU, at 4096 x 4096 x 4 (the headline frame):

  python tools/tracer_series_cost.py [--reps 3] [--steps 20] --parent ab/prev.so [--out profiles/tracer_series_cost.txt]
  python tools/tracer_series_cost.py --one [--steps 20]                  one process: a JSON line
  python tools/tracer_series_cost.py --trace                             (what the table starts under rocprofv3 --kernel-trace --stats)
  python tools/tracer_series_cost.py --asm-only                          the `make asm` figures alone (needs no GPU)

(a) The table alternates fresh processes on one box (tools/series_cost.py's way): the parent commit's library (BEOM_HIP_LIB)
and this tree's, each stepping with 1 and with 4 tracers and WITHOUT a tracer series.  The yardstick is the parent's own
max - min over the alternations; the tree's median has to lie within it.  (b) The tree's process then keeps levels 1, 2, 3 at
stride 1 and at stride 10 on the 4 tracers; every configuration is timed between two blocks without a tracer series in the
same process and compared with their mean.  (c) One more process runs under rocprofv3 --kernel-trace --stats (no counters in
that run) and gives the sample launches' own times per record, next to the time the compulsory words (3 + ntrc per
cell-layer: hlay, h_u, h_v and q of every tracer; 1 + ntrc at level 1) would take at the streaming rate profiles/series_cost.txt
uses, 5.6 TB/s.  Every process that uses the GPU runs under its own `timeout -k 10`, and the first one that fails ends the
run."""
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
ap.add_argument("--limit", type=int, default=420, help="seconds a process of the table may take (timeout -k 10)")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tracer_series_cost.txt"))
ap.add_argument("--frame", type=int, nargs=3, default=(4096, 4096, 4), metavar=("LM", "MM", "NLAY"))
a = ap.parse_args()
NTRC = (1, 4)
CONFIGS = ((1, 1), (2, 1), (3, 1), (1, 10), (2, 10), (3, 10))         # (level, stride), on NTRC[-1] tracers
STREAM_TBS = 5.6                                                       # profiles/README.md, the 14+6-stream row
TRACE_RECORDS = 5
KERNELS = r"k_tracer_series_rows|k_tracer_series_chunks"


def engine(ntrc):
    from beom_amd import capi, inputs as I
    from beom_amd.grid import read_input_data
    lm, mm, nlay = a.frame
    p, files = I.case_headline(lm, mm, nlay)
    e = capi.Engine(read_input_data(p, files=files))
    tracers(e, ntrc)
    return e


def tracers(e, ntrc):
    """ntrc tracers whose concentration varies from cell to cell (another wave length and mean per tracer)."""
    import numpy as np
    e.set_tracers(ntrc)
    n1 = e.p.ndeg + 1
    x = np.arange(n1, dtype=np.float64)
    c = np.stack([np.broadcast_to(0.6 + 0.1 * t + 0.4 * np.sin((0.011 + 0.003 * t) * x), (e.p.nlay, n1)) for t in range(ntrc)])
    e.set_concentration(c)


def one():
    import numpy as np
    lm, mm, nlay = a.frame
    e = engine(NTRC[0])
    has = hasattr(e.lib, "beom_set_tracer_series") and not os.environ.get("BEOM_HIP_LIB")
    out = {"lm": lm, "mm": mm, "nlay": nlay, "lib": "BEOM_HIP_LIB" if os.environ.get("BEOM_HIP_LIB") else "in-tree", "plain": {}, "configs": {}}
    tstp = [1]
    rec_on = [False]

    def steps():
        e.step(tstp[0], 6); tstp[0] += 6
        if rec_on[0]:
            e.sync(); e.download_tracer_series()
        blocks = []
        for _ in range(3):
            e.sync()
            t = time.perf_counter(); e.step(tstp[0], a.steps); e.sync(); blocks.append((time.perf_counter() - t) / a.steps * 1e6)
            tstp[0] += a.steps
            if rec_on[0]:
                e.download_tracer_series()
        return {"step_us": round(statistics.median(blocks), 1), "step_us_blocks": [round(b, 1) for b in blocks], "last_step": tstp[0] - 1}

    for ntrc in NTRC:
        if ntrc != NTRC[0]:
            tracers(e, ntrc)
        before = out["plain"][str(ntrc)] = steps()
    if has:
        ntrc = NTRC[-1]
        for level, stride in CONFIGS:
            e.set_tracer_series(level, stride, max(a.steps, 20)); rec_on[0] = True
            rec = steps()
            rec["step_us_without_before"] = before["step_us"]
            e.sample_tracer_series(); e.sync()
            t = time.perf_counter()
            for _ in range(9):
                e.sample_tracer_series()
            e.sync()
            rec["sample_us"] = round((time.perf_counter() - t) / 9 * 1e6, 1)
            s = e.download_tracer_series()
            rec["count"] = s["count"]
            rec["no_nan"] = bool(not np.isnan(s["rows"]).any())
            rec["total_last"] = [float(v) for v in s["total"][-1].ravel()[:2]]
            del s
            e.set_tracer_series(0); rec_on[0] = False
            before = steps()
            rec["step_us_without_after"] = before["step_us"]
            out["configs"]["%d/%d" % (level, stride)] = rec
    print(json.dumps(out))
    e.close()


def trace():
    """Per tracer count of NTRC: TRACE_RECORDS records at level 1, 2 and 3, in this order."""
    e = engine(NTRC[0])
    t = 1
    e.step(t, 3); t += 3
    for ntrc in NTRC:
        if ntrc != NTRC[0]:
            tracers(e, ntrc)
        for level in (1, 2, 3):
            e.set_tracer_series(level, 1, TRACE_RECORDS)
            e.step(t, TRACE_RECORDS); t += TRACE_RECORDS
            e.sync()
            e.download_tracer_series()
    e.close()


def traced():
    """{(ntrc, level): {kernel: [ns per launch]}} of a --trace process under rocprofv3, the launches taken in order."""
    d = tempfile.mkdtemp(prefix="tracer_series_trace_")
    cmd = ["timeout", "-k", "10", str(a.limit), "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--",
           sys.executable, os.path.abspath(__file__), "--trace", "--frame"] + [str(v) for v in a.frame]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        return None, "rocprofv3 failed (rc %d): %s" % (r.returncode, (r.stderr or r.stdout)[-400:].replace("\n", " | "))
    rows = []
    for fn in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        with open(fn) as fh:
            for row in csv.DictReader(fh):
                m = re.search(r"k_tracer_series_(rows)(?:<[^,>]*, ?(\d)|ILb\dELi(\d))|k_tracer_series_(chunks)", row.get("Kernel_Name", ""))
                if m:
                    rows.append((int(row["Start_Timestamp"]), m.group(1) or m.group(4), m.group(2) or m.group(3),
                                 int(row["End_Timestamp"]) - int(row["Start_Timestamp"])))
    rows.sort()
    # the row kernel names its level; a change of level (or a return to level 1) starts the next (ntrc, level) group, and the
    # finisher belongs to the row launch in front of it
    out, group, k, last = {}, None, -1, None
    for _, name, level, ns in rows:
        if name == "rows":
            level = int(level)
            if level != last:
                if level == 1:
                    k += 1
                last = level
            group = (NTRC[min(k, len(NTRC) - 1)], level)
        if group is not None:
            out.setdefault(group, {}).setdefault(name, []).append(ns)
    return out, None


def resource_lines():
    fn = os.path.join(ROOT, "beom_amd", "csrc", "resource_usage.txt")
    if not os.path.exists(fn):
        return ["(no beom_amd/csrc/resource_usage.txt: run `make asm` for the register figures)"]
    txt = open(fn).read()
    L = []
    for blk in re.split(r"(?=remark: [^\n]*Function Name:)", txt):
        m = re.search(r"Function Name: (\S+)", blk)
        if not m or not re.search(KERNELS, m.group(1)):
            continue
        g = lambda k: (re.search(k + r": (\d+)", blk) or [None, "?"])[1]
        L.append("  %-56s VGPRs %s  AGPRs %s  SGPRs %s  spills V/S %s/%s  scratch %s B/lane  LDS %s B  occupancy %s waves/SIMD"
                 % (m.group(1), g("VGPRs"), g("AGPRs"), g("TotalSGPRs"), g("VGPRs Spill"), g("SGPRs Spill"), g(r"ScratchSize \[bytes/lane\]"),
                    g(r"LDS Size \[bytes/block\]"), g(r"Occupancy \[waves/SIMD\]")))
    return L or ["(resource_usage.txt names no k_tracer_series_rows)"]


def listing_lines():
    """The same kernels' `Kernel info` blocks of the assembly listing, and what their bodies are made of."""
    fn = os.path.join(ROOT, "beom_amd", "csrc", "beom_engine.s")
    if not os.path.exists(fn):
        return ["(no beom_amd/csrc/beom_engine.s: run `make asm`)"]
    txt = open(fn).read()
    L = []
    for m in re.finditer(r"^(_Z\d+(?:%s)\S*):.*?; Kernel info:\n(.*?)\n; COMPUTE_PGM" % KERNELS, txt, re.S | re.M):
        body, info = m.group(0), m.group(2)
        g = lambda k: (re.search(k + r":? =? ?(\d+)", info) or [None, "?"])[1]
        n = lambda pat: len(re.findall(pat, body))
        L.append("  %-56s NumVgprs %s  NumAgprs %s  TotalNumSgprs %s  ScratchSize %s  LDSByteSize %s  Occupancy %s  code %s B"
                 % (m.group(1), g("NumVgprs"), g("NumAgprs"), g("TotalNumSgprs"), g("ScratchSize"), g("LDSByteSize"), g("Occupancy"), g("codeLenInByte")))
        L.append("  %-56s global_load %d  global_store %d  ds_bpermute_b32 %d  v_div_fmas_f64 %d  v_add_f64 %d  v_mul_f64 %d  v_min_f64 %d  s_waitcnt %d  scratch_ %d"
                 % ("", n(r"\tglobal_load"), n(r"\tglobal_store"), n(r"\tds_bpermute_b32"), n(r"\tv_div_fmas_f64"), n(r"\tv_add_f64"),
                    n(r"\tv_mul_f64"), n(r"\tv_min_f64"), n(r"\ts_waitcnt"), n(r"\tscratch_")))
    return L or ["(beom_engine.s names no k_tracer_series_rows)"]


def asm_section():
    return ["`make asm` figures (gfx950) of the new kernels k_tracer_series_rows<DENSE, LEVEL> and k_tracer_series_chunks.",
            "-Rpass-analysis=kernel-resource-usage:"] + resource_lines() + \
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
    L = ["Tracer series (beom_set_tracer_series, beom_tracer_series.h): cost at %d x %d x %d            tools/tracer_series_cost.py" % (lm, mm, nlay),
         "box: %s" % (socket.gethostname() or "?"), "",
         "%d alternations of two fresh processes (parent's library through BEOM_HIP_LIB and this tree's, the order swapped every time), %d steps per timed call,"
         % (a.reps, a.steps), "three calls per configuration, the median of the three; us per step (wall clock, stream synced).",
         "order of the processes: " + " ".join(l.split()[3] for l in log), ""]
    ok = True
    for ntrc in NTRC:
        par = [r["plain"][str(ntrc)]["step_us"] for r in runs["parent"]]
        tre = [r["plain"][str(ntrc)]["step_us"] for r in runs["tree"]]
        spread = max(par) - min(par)
        inside = abs(statistics.median(tre) - statistics.median(par)) <= spread
        ok = ok and inside
        L.append("(a) %d tracer(s), no tracer series   parent per alternation: %s   max - min %.1f" % (ntrc, par, spread))
        L.append("(a) %d tracer(s), no tracer series   tree   per alternation: %s   median %.1f against the parent's median %.1f (%+.2f %%): %s"
                 % (ntrc, tre, statistics.median(tre), statistics.median(par), (statistics.median(tre) / statistics.median(par) - 1) * 100,
                    "within the parent's max - min" if inside else "NOT within the parent's max - min"))
    L.append("condition (the tree's step without a tracer series within the parent's own max - min, 1 and 4 tracers): %s" % ("met" if ok else "NOT met"))
    L.append("")
    L.append("(b) %d tracers   %-14s %12s %12s %12s %16s" % (NTRC[-1], "level / stride", "step us", "without us", "vs none us", "one sample us"))
    for level, stride in CONFIGS:
        k = "%d/%d" % (level, stride)
        st = statistics.median(r["configs"][k]["step_us"] for r in runs["tree"])
        base = statistics.median(0.5 * (r["configs"][k]["step_us_without_before"] + r["configs"][k]["step_us_without_after"]) for r in runs["tree"])
        su = statistics.median(r["configs"][k]["sample_us"] for r in runs["tree"])
        L.append("                %-14s %12.1f %12.1f %+12.1f %16.1f" % (k, st, base, st - base, su))
    L.append("")
    L.append("(without: the mean of the two blocks without a tracer series timed around the configuration in the same process;")
    L.append(" vs none: the step with the tracer series minus that; one sample: beom_sample_tracer_series alone, 9 records between two syncs, wall clock.)")
    L.append("no record holds a NaN: %s" % all(r["configs"]["%d/%d" % c]["no_nan"] for r in runs["tree"] for c in CONFIGS))
    L.append("")
    tr, err = traced()
    L.append("(c) The sample's launches under rocprofv3 --kernel-trace --stats (a process of its own, no counters), summed per record")
    L.append("    (a record is taken in batches of rows: several row launches and finishers), next to the compulsory words at %.1f TB/s:" % STREAM_TBS)
    if tr is None:
        L.append("  not measured: " + err)
    else:
        cl = nlay * (lm + 1) * (mm + 1)
        for (ntrc, level), ks in sorted(tr.items()):
            rows_ns, ch_ns = sum(ks.get("rows", [])) / TRACE_RECORDS, sum(ks.get("chunks", [])) / TRACE_RECORDS
            w = (3 if level >= 2 else 1) + ntrc
            byts = 8.0 * w * cl
            tot = rows_ns + ch_ns
            L.append("  %d tracer(s) level %d   rows %8.1f us (%d launches / record)   finisher %7.1f us   record %8.1f us   %d words = %.0f MB   %.2f TB/s   floor %7.1f us   x%.2f"
                     % (ntrc, level, rows_ns / 1e3, len(ks.get("rows", [])) // TRACE_RECORDS, ch_ns / 1e3, tot / 1e3, w, byts / 1e6, byts / tot / 1e3,
                        byts / STREAM_TBS / 1e6, tot / 1e3 / (byts / STREAM_TBS / 1e6)))
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
