#!/usr/bin/env python3
"""GPU box helper: what the vertical pass of the tracers (moka_set_tracer_vertical_diffusion) costs forwards and backwards, against the
same tree with every kappaV zero, in one process.

Per round and tracer count (1, 4) the legs alternate: kappaV off / on for every tracer.  Each repetition records one RK4 step on a
tracer tape and sweeps it (zero seeds: the kernels' work does not depend on the values), with moka_mark around both; the pass is the
difference of the medians of the two legs.  Beside it, from the same run: the tracer stage launch, (step with tracers - step without) / 4,
which moves more bytes than the pass, and the pass's (1 + 2 nT) K nC 8 bytes at the copy rate of moka_bw_probe.

    python3 tools/tracer_vmix_timing.py [--small] [--rounds R] [--steps N] [--out FILE]"""
import argparse
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
from moka_hip import meshgen as mg         # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--small", action="store_true")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--out", default=None)
args = ap.parse_args()

m, K = (64 if args.small else 320), 60
mesh = mg.icosahedral_mesh(m)
ssh, u, h, rest, dts = mg.sphere_synthetic_state(mesh, K)
cfg = {"time_management": {"config_start_time": dt.datetime(1, 1, 1), "config_run_duration": dt.timedelta(hours=1)},
       "time_integration": {"config_dt": dt.timedelta(seconds=dts), "config_number_of_time_levels": 2}}
b = mk.MokaHIP(0)
phi = np.random.default_rng(1).uniform(0.5, 1.5, (mesh.nCells, K))
hm = float(np.mean(h))
kv = 10.0 * hm * hm / dts                  # s / hm^2 = 10
Setup, Diag, Tend, Prog = mk.ocn_init_from_arrays(mesh, ssh, u, h, rest, cfg, b, multilayer=True)
med = statistics.median


def timed(fn, reps):
    out = []
    for rep in range(args.warmup + reps):
        b.synchronize()
        b.marks_reset()
        b.mark()
        fn()
        b.mark()
        b.synchronize()
        if rep >= args.warmup:
            out.append(list(b.marks_read())[0])
    return out


bare = timed(lambda: mk.run_steps(Prog, mk.RungeKutta4, dts, 1), args.rounds * args.steps)
counts, legs = (1, 4), (("off", None), ("on", kv))
step = {(n, leg[0]): [] for n in counts for leg in legs}
sweep = {(n, leg[0]): [] for n in counts for leg in legs}
paths = {}
for _ in range(args.rounds):
    for n in counts:
        tr = mk.set_tracers(Prog, [phi] * n)
        tape = mk.TracerAdjointTape(Prog, 1)
        for name, value in legs:
            tr.set_vertical_diffusivity(value)
            for rep in range(args.warmup + args.steps):
                b.synchronize()
                b.marks_reset()
                b.mark()
                tape.step(dts)
                b.mark()
                for j in range(n):
                    tape.seed(j, None)
                b.mark()
                tape.sweep()
                b.mark()
                b.synchronize()
                iv = list(b.marks_read())
                if rep >= args.warmup:
                    step[(n, name)].append(iv[0])
                    sweep[(n, name)].append(iv[2])
            paths[name] = (tr.vmix_path(), tape.vmix_path())
        tape.close()
mk.set_tracers(Prog, [])
bw = b.bw_probe()
nC = mesh.nCells
rows = []
for n in counts:
    s0, s1, r0, r1 = (med(step[(n, "off")]), med(step[(n, "on")]), med(sweep[(n, "off")]), med(sweep[(n, "on")]))
    rows.append({"tracers": n, "step_off_ms": s0, "step_on_ms": s1, "forward_pass_ms": s1 - s0, "sweep_off_ms": r0, "sweep_on_ms": r1,
                 "reverse_pass_ms": r1 - r0, "tracer_stage_launch_ms": (s0 - med(bare)) / 4,
                 "bytes_model_ms": (1 + 2 * n) * K * nC * 8 / (bw.get("copy_GBs") * 1e9) * 1e3,
                 "step_on_min_max": (min(step[(n, "on")]), max(step[(n, "on")])), "step_off_min_max": (min(step[(n, "off")]), max(step[(n, "off")]))})
result = {"cells": nC, "K": K, "rounds": args.rounds, "steps_per_round": args.steps, "copy_GBs": bw.get("copy_GBs"),
          "step_without_tracers_ms": med(bare), "vmix_paths_forward_reverse": paths, "rows": rows}
print(json.dumps(result), flush=True)
if args.out:
    with open(args.out, "w") as fh:
        fh.write(f"The vertical pass beside the same taped step and sweep with every kappaV zero -- {nC} cells x {K} levels, fp64, linear dycore,\n"
                 f"s / hm^2 = 10 on every tracer, one MI355X.  tools/tracer_vmix_timing.py ({args.rounds} rounds x {args.steps} repetitions after "
                 f"{args.warmup} warm-up, the legs\nalternated in one process; medians of moka_mark intervals; the taped step includes the tape's copies in both legs).\n"
                 f"Copy rate of the same run (moka_bw_probe): {result['copy_GBs']:.0f} GB/s.  RK4 step without tracers: {med(bare):.3f} ms.  Form of the pass (forward, "
                 f"reverse): {paths['on']}; with kappaV off: {paths['off']}.\n\n"
                 "   tracers   step ms (off, on)     forward pass ms   sweep ms (off, on)    reverse pass ms   one tracer stage launch ms   (1 + 2 nT) K nC 8 B at the copy rate, ms\n")
        for r in rows:
            fh.write(f"   {r['tracers']:<9d} {r['step_off_ms']:<9.3f} {r['step_on_ms']:<11.3f} {r['forward_pass_ms']:<17.3f} {r['sweep_off_ms']:<9.3f} "
                     f"{r['sweep_on_ms']:<11.3f} {r['reverse_pass_ms']:<17.3f} {r['tracer_stage_launch_ms']:<28.3f} {r['bytes_model_ms']:.3f}\n")
Prog._state.close(); Setup.mesh.close()
