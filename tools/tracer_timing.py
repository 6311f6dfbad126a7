#!/usr/bin/env python3
"""GPU box helper: ms per linear RK4 step with 0, 1 and 3 passive tracers (moka_set_tracers), each tracer count with harmonic
diffusion off and on (moka_set_tracer_diffusion, kappa = 0.02 dcEdge_min^2 / dt), in one process, the settings alternated round by
round and each step timed between two moka_mark events (median, min, max) -- first with the default kernel choice (the tracer launch
in its patch form), then with kernel variant 3 (generic dycore kernels, the tracer launch in its generic form).  The tracer launch
alone is the difference to the same run's tracer-free step, over the four launches of a step; the diffusion-off legs run the
instantiations of a state that never set a diffusivity, so they are the baseline of the diffusion-on legs.  Shader clock and package
power are sampled from sysfs while the 3-tracer steps run back to back, diffusion off and on (bench.py's under_load).  A third set of
legs gives every tracer a source (moka_tracer_source_upload; the SRC instantiations, one more own-row stream of 8 K nC bytes per sourced
tracer and launch), diffusion off, and with three tracers also on; they alternate with the other legs in the same rounds.  A fourth set
gives every tracer a biharmonic coefficient (moka_set_tracer_biharmonic, kappa4 = 0.002 dcEdge_min^4 / dt; the Laplacian launch and the BIH
instantiations), diffusion off and on; byte model per stage with B such tracers: 8 K nC (1 + 2 B) for the Laplacian launch, 8 K nC B more in
the tracer launch.  Config 4 (icosahedral
m = 320, 1 024 002 cells x 60 levels); --small: config 3 (m = 64).  Prints one JSON line and, with --out FILE, writes the summary
table there.

Contract bytes of the tracer launches of one step (what the algorithm has to move once): the stage's normalVelocity rows (4 nE), the
stage's and the next layerThickness rows (8 nC), the current level's for stages 2 / 3 (2 nC), and per tracer 16 cell streams (pphi
in x 4, phi_cur in x 2, Qn in x 3 / out x 4, pphi out x 3):  8 K (4 nE + 10 nC + 16 nT nC).

    python3 tools/tracer_timing.py [--small] [--rounds R] [--steps N] [--out profiles/tracer_summary.txt]"""
import argparse
import ctypes as C
import datetime as dt
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mpas-ocean.jl_amd"))
sys.path.insert(0, ROOT)
import numpy as np                         # noqa: E402
import moka_hip as mk                      # noqa: E402
from moka_hip import lib as L              # noqa: E402
from moka_hip import meshgen as mg         # noqa: E402
import bench                               # noqa: E402  (under_load)

ap = argparse.ArgumentParser()
ap.add_argument("--small", action="store_true")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--out", default=None)
args = ap.parse_args()

m, K = (64 if args.small else 320), 60
mesh = mg.icosahedral_mesh(m)
ssh, u, h, rest, dts = mg.sphere_synthetic_state(mesh, K)
cfg = {"time_management": {"config_start_time": dt.datetime(1, 1, 1), "config_run_duration": dt.timedelta(hours=1)},
       "time_integration": {"config_dt": dt.timedelta(seconds=dts), "config_number_of_time_levels": 2}}
b = mk.MokaHIP(0)
lib = L.lib()
rng = np.random.default_rng(1)
phi = rng.uniform(0.5, 1.5, (mesh.nCells, K))
counts = (0, 1, 3)
kappa = 0.02 * float(mesh.dcEdge.min()) ** 2 / dts
settings = [(0, False, False)] + [(n, d, False) for n in counts if n for d in (False, True)]
settings += [(n, False, True) for n in counts if n] + [(3, True, True)]
key = lambda n, d, s=False: f"{n}{'+diff' if d else ''}{'+src' if s else ''}"      # noqa: E731
kappa4 = 0.002 * float(mesh.dcEdge.min()) ** 4 / dts
bsettings = [(n, d) for n in counts if n for d in (False, True)]
qsrc = rng.uniform(-1.0, 1.0, (mesh.nCells, K)) * (float(h.mean()) / (1000.0 * dts))
result = {"cells": mesh.nCells, "edges": mesh.nEdges, "K": K, "rounds": args.rounds, "steps_per_round": args.steps, "kappa": kappa, "kappa4": kappa4,
          "forms": {}}
for variant, form in ((0, "patch"), (3, "generic")):
    b.set_kernel_variant(variant)
    Setup, Diag, Tend, Prog = mk.ocn_init_from_arrays(mesh, ssh, u, h, rest, cfg, b, multilayer=True)
    sh = Prog._state._h
    steps = {n: [] for n in counts}
    dsteps = {key(n, d): [] for n, d, s in settings if not s}
    ssteps = {key(n, d, True): [] for n, d, s in settings if s}
    bsteps = {key(n, d) + "+bih": [] for n, d in bsettings}
    bpath = 0
    path = 0
    for _ in range(args.rounds):
        for n, diff, src in settings:
            tr = mk.set_tracers(Prog, [phi] * n, diffusivity=kappa if diff else None, sources=[qsrc] * n if src else None)
            for _ in range(args.warmup):                                     # lazy allocations, LDS attributes, clocks
                L.check(lib.moka_step_rk4(sh, C.c_double(dts)), b._h)
            b.synchronize()
            b.marks_reset()
            b.mark()
            for _ in range(args.steps):
                L.check(lib.moka_step_rk4(sh, C.c_double(dts)), b._h)
                b.mark()
            b.synchronize()
            if src:
                ssteps[key(n, diff, True)] += list(b.marks_read())
                continue
            dsteps[key(n, diff)] += list(b.marks_read())
            if not diff:
                steps[n] = dsteps[key(n, False)]
            if n:
                path = tr.path()
        for n, diff in bsettings:                                            # the biharmonic legs, in the same round
            tr = mk.set_tracers(Prog, [phi] * n, diffusivity=kappa if diff else None, biharmonic=kappa4)
            for _ in range(args.warmup):
                L.check(lib.moka_step_rk4(sh, C.c_double(dts)), b._h)
            b.synchronize()
            b.marks_reset()
            b.mark()
            for _ in range(args.steps):
                L.check(lib.moka_step_rk4(sh, C.c_double(dts)), b._h)
                b.mark()
            b.synchronize()
            bsteps[key(n, diff) + "+bih"] += list(b.marks_read())
            bpath = tr.path()
    load = {}
    for diff in (False, True):                                               # clock and power while the 3-tracer steps run
        mk.set_tracers(Prog, [phi] * 3, diffusivity=kappa if diff else None)
        load[key(3, diff)] = bench.under_load(b, lambda: L.check(lib.moka_step_rk4(sh, C.c_double(dts)), b._h), seconds=1.5, batch=5)
    mk.set_tracers(Prog, [phi] * 3, diffusivity=kappa, biharmonic=kappa4)
    load["3+diff+bih"] = bench.under_load(b, lambda: L.check(lib.moka_step_rk4(sh, C.c_double(dts)), b._h), seconds=1.5, batch=5)
    mk.set_tracers(Prog, [])
    med = {n: statistics.median(v) for n, v in steps.items()}
    contract = {n: 8 * K * (4 * mesh.nEdges + 10 * mesh.nCells + 16 * n * mesh.nCells) for n in counts if n}
    result["forms"][form] = {
        "tracer_path": path, "ms_per_step_median": med, "ms_per_step_min": {n: min(v) for n, v in steps.items()},
        "increment_ms_per_step": {n: med[n] - med[0] for n in counts if n},
        "tracer_launch_ms": {n: (med[n] - med[0]) / 4 for n in counts if n},
        "contract_bytes_per_step": contract,
        "contract_TBps": {n: contract[n] / ((med[n] - med[0]) * 1e-3) / 1e12 for n in contract},
        "diffusion": {k: {"median": statistics.median(v), "min": min(v), "max": max(v),
                          "p25": statistics.quantiles(v, n=4)[0], "p75": statistics.quantiles(v, n=4)[2]} for k, v in dsteps.items()},
        "diffusion_launch_delta_ms": {n: (statistics.median(dsteps[key(n, True)]) - statistics.median(dsteps[key(n, False)])) / 4
                                      for n in counts if n},
        "sources": {k: {"median": statistics.median(v), "min": min(v), "max": max(v), "p25": statistics.quantiles(v, n=4)[0],
                        "p75": statistics.quantiles(v, n=4)[2],
                        "launch_delta_ms": (statistics.median(v) - statistics.median(dsteps[k[:-4]])) / 4} for k, v in ssteps.items()},
        "biharmonic": {k: {"median": statistics.median(v), "min": min(v), "max": max(v), "p25": statistics.quantiles(v, n=4)[0],
                           "p75": statistics.quantiles(v, n=4)[2],
                           "stage_delta_ms": (statistics.median(v) - statistics.median(dsteps[k[:-4]])) / 4} for k, v in bsteps.items()},
        "biharmonic_tracer_path": bpath,
        "biharmonic_model_stage_delta_ms": {n: 8 * K * mesh.nCells * (1 + 3 * n) / 1e9 for n in counts if n},   # ms at 1 TB/s; scaled below
        "under_load": load}
    Prog._state.close(); Setup.mesh.close()
b.set_kernel_variant(0)
bw = b.bw_probe()
result["copy_GBs"] = bw.get("copy_GBs")
for f in result["forms"].values():
    f["contract_fraction_of_copy_rate"] = {n: f["contract_TBps"][n] * 1e3 / result["copy_GBs"] for n in f["contract_TBps"]}
    f["biharmonic_model_stage_delta_ms"] = {n: v * 1e3 / result["copy_GBs"] for n, v in f["biharmonic_model_stage_delta_ms"].items()}
print(json.dumps(result), flush=True)
if args.out:
    with open(args.out, "w") as fh:
        fh.write(f"Passive tracer transport beside the linear RK4 step -- {mesh.nCells} cells x {K} levels, fp64, one MI355X.\n"
                 f"tools/tracer_timing.py ({args.rounds} rounds x {args.steps} steps after {args.warmup} warm-up steps, 0 / 1 / 3 tracers "
                 "alternated round by round in one\nprocess; medians of moka_mark intervals).  The tracer-free step of the same run is "
                 "the code path without the feature.\nThe tracer launch alone = (step with n tracers - tracer-free step) / 4 launches.  "
                 f"Copy rate of the same run (moka_bw_probe): {result['copy_GBs']:.0f} GB/s.\n\n")
        for form, f in result["forms"].items():
            fh.write(f"{form} form (moka_state_tracer_path = {f['tracer_path']}; kernel variant {0 if form == 'patch' else 3})\n"
                     "   tracers   ms / RK4 step (median)   min      increment   per tracer launch   contract bytes / step   "
                     "TB/s     of copy rate\n")
            for n in counts:
                line = f"   {n:<9d} {f['ms_per_step_median'][n]:<24.3f} {f['ms_per_step_min'][n]:<8.3f}"
                if n:
                    line += (f" {f['increment_ms_per_step'][n]:<11.3f} {f['tracer_launch_ms'][n]:<19.3f} "
                             f"{f['contract_bytes_per_step'][n] / 1e9:<23.2f} {f['contract_TBps'][n]:<8.2f} "
                             f"{f['contract_fraction_of_copy_rate'][n]:.2f}")
                fh.write(line.rstrip() + "\n")
            fh.write("\n   harmonic diffusion (kappa = 0.02 dcEdge_min^2 / dt on every tracer) off / on, ms / RK4 step\n"
                     "   setting   median    min       p25       p75       max       on - off per tracer launch\n")
            for k, d in f["diffusion"].items():
                line = f"   {k:<9s} {d['median']:<9.3f} {d['min']:<9.3f} {d['p25']:<9.3f} {d['p75']:<9.3f} {d['max']:<9.3f}"
                if k.endswith("+diff"):
                    line += f" {f['diffusion_launch_delta_ms'][int(k.split('+')[0])]:+.3f}"
                fh.write(line.rstrip() + "\n")
            fh.write("\n   a source on every tracer (moka_tracer_source_upload), ms / RK4 step; the leg without '+src' is the row above\n"
                     "   setting     median    min       p25       p75       max       with - without source per tracer launch\n")
            for k, d in f["sources"].items():
                fh.write(f"   {k:<11s} {d['median']:<9.3f} {d['min']:<9.3f} {d['p25']:<9.3f} {d['p75']:<9.3f} {d['max']:<9.3f} "
                         f"{d['launch_delta_ms']:+.3f}\n")
            fh.write(f"\n   a biharmonic coefficient on every tracer (moka_set_tracer_biharmonic, kappa4 = 0.002 dcEdge_min^4 / dt; tracer path "
                     f"{f['biharmonic_tracer_path']}), ms / RK4 step;\n   the leg without '+bih' is the row above.  Per stage = the Laplacian launch "
                     "+ what the tracer launch gains; model = 8 K nC (1 + 3 B) bytes at the copy rate\n"
                     "   setting       median    min       p25       p75       max       with - without per stage   model\n")
            for k, d in f["biharmonic"].items():
                fh.write(f"   {k:<13s} {d['median']:<9.3f} {d['min']:<9.3f} {d['p25']:<9.3f} {d['p75']:<9.3f} {d['max']:<9.3f} "
                         f"{d['stage_delta_ms']:<+26.3f} {f['biharmonic_model_stage_delta_ms'][int(k.split('+')[0])]:+.3f}\n")
            for k, u in f["under_load"].items():
                fh.write(f"   under load, {k}: sclk {u['sclk_mhz_mean']} MHz (min {u['sclk_mhz_min']}), power {u['power_w_mean']} W "
                         f"(max {u['power_w_max']}), {u['ms_per_call_sustained']:.3f} ms / step sustained\n")
            fh.write("\n")
