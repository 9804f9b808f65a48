#!/usr/bin/env python3
"""What the conservation integrals (beom_integrals) cost on one GPU, on the frames of tools/bench_case.py:

  python tools/integrals_cost.py headline|headline_land|soliton [--calls 25] [--steps 40] [--host-route]
  BEOM_HIP_LIB=ab/prev.so python tools/integrals_cost.py CASE --steps-only      (an older build: the step alone)
  python tools/integrals_cost.py CASE --pmc                                     (under rocprofv3 --pmc: a few calls, no timing)

Prints one JSON line: the call (stream synced on both sides, median), one time step of the frame and the launches the
issue names for scale (update_h, Montgomery + viscosity), the step time with a call every 10 steps less the calls' own time,
and with --host-route what a user had before: download of hlay, u, v and the numpy restatement (tests/integrals_ref.py)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from beom_amd import capi, inputs as I
from beom_amd.grid import read_input_data


def with_land(pf):            # tools/bench_case.py: the headline basin with a land mass (5 % of the cells)
    p, files = pf
    h = files["h_bo"]
    x = np.arange(p.lm + 2)[:, None]; y = np.arange(p.mm + 2)[None, :]
    h[((x - 0.3 * p.lm) ** 2 + (y - 0.6 * p.mm) ** 2) < (0.126 * p.lm) ** 2] = 0.0
    files["init"][h == 0.0] = 0.0
    return p.replace(ndeg=I.get_nbr_deg_freedom(h)), files


CASES = {"headline": lambda: I.case_headline(4096, 4096, 4),
         "headline_land": lambda: with_land(I.case_headline(4096, 4096, 4)),
         "soliton": lambda: I.case_soliton(lm=2048, mm=256, dt_s=60.0)}

ap = argparse.ArgumentParser()
ap.add_argument("case", choices=sorted(CASES))
ap.add_argument("--calls", type=int, default=25)
ap.add_argument("--steps", type=int, default=40)
ap.add_argument("--steps-only", action="store_true")
ap.add_argument("--host-route", action="store_true")
ap.add_argument("--pmc", action="store_true")
a = ap.parse_args()

p, files = CASES[a.case]()
f = read_input_data(p, files=files)
e = capi.Engine(f)
e.step(1, 10)
out = {"case": a.case, "lm": p.lm, "mm": p.mm, "nlay": p.nlay, "ndeg": p.ndeg, "dense": int(e.is_dense) + int(e.is_embedded),
       "lib": os.environ.get("BEOM_HIP_LIB", "in-tree")}
if a.pmc:
    for _ in range(6):
        e.integrals()
    print(json.dumps(out)); sys.exit(0)


def steps_us(t0, n):
    e.sync()
    t = time.perf_counter(); e.step(t0, n); return (time.perf_counter() - t) / n * 1e6


tstp = 11
plain = []
for _ in range(3):
    plain.append(steps_us(tstp, a.steps)); tstp += a.steps
out["step_us"] = round(statistics.median(plain), 1)
ms, nl = e.profile_steps(tstp, 20); tstp += 20
names = ("h", "mont", "visc", "u", "v", "mont+visc", "u+v", "")
out["per_launch_us"] = {names[k]: round(ms[k] / nl[k] * 1e3, 1) for k in range(len(nl)) if nl[k]}
if not a.steps_only:
    e.integrals()                                     # (first call: allocations)
    calls = []
    for _ in range(a.calls):
        e.sync()
        t = time.perf_counter(); s = e.integrals(); calls.append((time.perf_counter() - t) * 1e6)
    out["integrals_call_us"] = round(statistics.median(calls), 1)
    out["integrals_call_us_min_max"] = [round(min(calls), 1), round(max(calls), 1)]
    out["finite"] = bool(np.isfinite(s["raw"]).all())
    # compulsory words per cell: hlay, u, v per layer; fcor, h_th; where the masks are arrays (land) mk_n, mk_u, mk_v, mkpe, mkpi
    per_cell = 3 * p.nlay + 2 + (5 if (e.is_embedded or not e.is_dense) else 0)
    out["compulsory_MB"] = round(p.ndeg * per_cell * 8 / 1e6, 1)
    with_calls = []
    for _ in range(3):                                # 40 steps with a call every 10, less the calls' own (median) time
        e.sync()
        t = time.perf_counter()
        for k in range(a.steps // 10):
            e.step(tstp, 10, sync=False); tstp += 10
            e.integrals()
        dt = (time.perf_counter() - t) * 1e6
        with_calls.append((dt - (a.steps // 10) * out["integrals_call_us"]) / (a.steps // 10 * 10))
    out["step_us_with_a_call_every_10_steps_less_the_calls"] = round(statistics.median(with_calls), 1)
    again = []
    for _ in range(3):
        again.append(steps_us(tstp, a.steps)); tstp += a.steps
    out["step_us_again"] = round(statistics.median(again), 1)
    if a.host_route:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import integrals_ref as R
        e.sync()
        t = time.perf_counter(); st = e.download(("hlay", "u", "v")); out["download_hlay_u_v_ms"] = round((time.perf_counter() - t) * 1e3, 1)
        t = time.perf_counter(); ref = R.integrals(f, st); out["numpy_restatement_ms"] = round((time.perf_counter() - t) * 1e3, 1)
        got = e.integrals()["raw"]
        out["bitwise_equal_to_restatement"] = bool(np.array_equal(got.view(np.uint64), ref.view(np.uint64)))
print(json.dumps(out))
e.close()
