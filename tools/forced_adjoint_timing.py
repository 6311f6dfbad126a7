#!/usr/bin/env python3
"""GPU box helper: what the transposed vertical momentum pass of moka_forced_tape (the edge-column kernel plus the cell gather) costs
per reversed step, in both of its forms, beside the forward pass measured in the same process.

Per round the legs alternate: kernel variant 0 (tile forms) and 3 (column forms), each with the pass off and on (nuV + drag + stress).
A leg records `--steps` forced RK4 steps on a moka_forced_tape -- each between two moka_mark: the forward step -- seeds with
d sum(ssh^2) and sweeps between two marks: the reverse sweep, divided by the steps.  The pass = on - off, forward and reverse alike;
"grad": the on leg with all three gradients flagged.  --quadratic adds, on a tape of moka_forced_tape_create_quadratic, the legs
"qd" (on + Cd, with dt Cd sp / hm = 1/2 at the rms speed of the state: the QD instances and the transpose of the bottom-speed
stencil) and "qdgrad" (qd with the three gradients and D_cd flagged), in both forms; every other leg keeps its plain tape.  Beside it the copy rate of moka_bw_probe and the byte-bound estimates at that
rate: forward (2 nEdges + nCells) K 8 B (u in and out, the unique bytes of h_new); reverse (4 nEdges + 3 nCells) K 8 B (XU in and out,
un in, hbar out; the unique bytes of h_new; XH in and out -- hbar read back by the gather is counted as L2 traffic, not HBM).

    python3 tools/forced_adjoint_timing.py [--small] [--quadratic] [--rounds R] [--steps N] [--out FILE]"""
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
ap.add_argument("--quadratic", action="store_true")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--steps", type=int, default=2)
ap.add_argument("--out", default=None)
ap.add_argument("--note", default="")
args = ap.parse_args()

m, K = (64 if args.small else 320), 60
mesh = mg.icosahedral_mesh(m)
print(f"mesh: {mesh.nCells} cells, {mesh.nEdges} edges", flush=True)
ssh, u, h, rest, dts = mg.sphere_synthetic_state(mesh, K)
cfg = {"time_management": {"config_start_time": dt.datetime(1, 1, 1), "config_run_duration": dt.timedelta(hours=1)},
       "time_integration": {"config_dt": dt.timedelta(seconds=dts), "config_number_of_time_levels": 2}}
b = mk.MokaHIP(0)
hm = float(np.mean(h))
nu, drag = 4.0 * hm * hm / dts, 0.5 * hm / dts          # s / hm^2 = 4, q / hm = 1/2
tau = np.random.default_rng(1).uniform(-1.0, 1.0, mesh.nEdges) * hm / dts
Setup, Diag, Tend, Prog = mk.ocn_init_from_arrays(mesh, ssh, u, h, rest, cfg, b, multilayer=True)
med = statistics.median
ALL = {"viscosity": nu, "bottom_drag": drag, "surface_stress": tau}
LEGS = (("off", 0, {}, False), ("on", 0, ALL, False), ("grad", 0, ALL, True),
        ("off3", 3, {}, False), ("on3", 3, ALL, False), ("grad3", 3, ALL, True))
if args.quadratic:
    QD = dict(ALL, quadratic_drag=drag / max(float(np.sqrt(np.mean(u ** 2))), 1e-30))
    LEGS += (("qd", 0, QD, False), ("qdgrad", 0, QD, True), ("qd3", 3, QD, False), ("qdgrad3", 3, QD, True))
fwd = {name: [] for name, *_ in LEGS}
rev = {name: [] for name, *_ in LEGS}
paths = {}
for rnd in range(args.rounds + 1):          # round 0 warms up
    for name, variant, kw, grad in LEGS:
        b.set_kernel_variant(variant)
        quad = "quadratic_drag" in kw
        if quad:                                # (a plain tape refuses a state with Cd != 0, and Cd a state with a plain tape)
            mk.set_vertical_mixing(Prog)
            tape = mk.ForcedAdjointTape(Prog, args.steps, quadratic_drag=True)
            mk.set_vertical_mixing(Prog, **kw)
            tape.want_gradient(stress=grad, viscosity=grad, drag=grad, quadratic_drag=grad)
        else:
            mk.set_vertical_mixing(Prog, **kw)
            tape = mk.ForcedAdjointTape(Prog, args.steps)
            tape.want_gradient(stress=grad, viscosity=grad, drag=grad)
        for _ in range(args.steps):
            b.synchronize(); b.marks_reset(); b.mark()
            tape.step(dts)
            b.mark(); b.synchronize()
            if rnd:
                fwd[name].append(list(b.marks_read())[0])
        mk.lib.check(mk.lib.lib().moka_forced_adjoint_seed_sum_sq_ssh(tape._h), b._h)
        b.synchronize(); b.marks_reset(); b.mark()
        tape.sweep()
        b.mark(); b.synchronize()
        if rnd:
            rev[name].append(list(b.marks_read())[0] / args.steps)
        paths[name] = (mk.momentum_vmix_path(Prog), tape.vmix_path())
        tape.close()
        if quad:
            mk.set_vertical_mixing(Prog)
        Prog.normalVelocity[-1].set(u); Prog.layerThickness[-1].set(h); Prog.ssh[-1].set(ssh)      # every leg starts from the same state
        print(f"round {rnd} {name}: forward {fwd[name][-1:]}, reverse {rev[name][-1:]}", flush=True)
b.set_kernel_variant(0)
mk.set_vertical_mixing(Prog)
bw = b.bw_probe()
nC, nE = mesh.nCells, mesh.nEdges
rate = bw.get("copy_GBs") * 1e9
bound_f = (2 * nE + nC) * K * 8 / rate * 1e3
bound_r = (4 * nE + 3 * nC) * K * 8 / rate * 1e3
rows = []
extra = ("qd", "qdgrad") if args.quadratic else ()
for form, off, legs in (("tile", "off", ("on", "grad") + extra), ("column", "off3", ("on3", "grad3") + tuple(x + "3" for x in extra))):
    for leg in legs:
        pf, pr = med(fwd[leg]) - med(fwd[off]), med(rev[leg]) - med(rev[off])
        rows.append({"form": form, "paths": paths[leg], "leg": leg.rstrip("3"), "forward_pass_ms": pf, "reverse_pass_ms": pr,
                     "reverse_over_forward": pr / pf if pf > 0 else None, "byte_bound_over_reverse": bound_r / pr if pr > 0 else None,
                     "forward_step_off_on": (med(fwd[off]), med(fwd[leg])), "reverse_step_off_on": (med(rev[off]), med(rev[leg])),
                     "reverse_on_min_max": (min(rev[leg]), max(rev[leg])), "reverse_off_min_max": (min(rev[off]), max(rev[off]))})
result = {"cells": nC, "edges": nE, "K": K, "rounds": args.rounds, "steps": args.steps, "copy_GBs": bw.get("copy_GBs"),
          "byte_bound_forward_ms": bound_f, "byte_bound_reverse_ms": bound_r, "rows": rows}
print(json.dumps(result), flush=True)
if args.out:
    with open(args.out, "w") as fh:
        fh.write(f"The transposed vertical momentum pass of moka_forced_tape beside the forward pass -- {nC} cells, {nE} edges x {K} levels, fp64,\n"
                 f"linear dycore, s / hm^2 = 4, q / hm = 1/2, a stress on every edge, one MI355X.  tools/forced_adjoint_timing.py ({args.rounds} rounds\n"
                 f"after one warm-up round, {args.steps} recorded steps a leg, the legs alternated in one process; medians of moka_mark intervals around a\n"
                 "forced taped step and around the sweep / steps; the pass = on - off; grad: all three gradients flagged).\n"
                 f"Copy rate of the same run (moka_bw_probe): {result['copy_GBs']:.0f} GB/s.  Byte bounds at that rate: forward (2 nEdges + nCells) K 8 B:\n"
                 f"{bound_f:.3f} ms; reverse (4 nEdges + 3 nCells) K 8 B: {bound_r:.3f} ms.\n\n"
                 "   form     leg    forward pass ms   reverse pass ms   reverse / forward   byte bound / reverse   reversed step ms (off, on)\n")
        for r in rows:
            fh.write(f"   {r['form']:<8s} {r['leg']:<6s} {r['forward_pass_ms']:<17.3f} {r['reverse_pass_ms']:<17.3f} {(r['reverse_over_forward'] or 0):<19.3f} "
                     f"{(r['byte_bound_over_reverse'] or 0):<22.3f} {r['reverse_step_off_on'][0]:.3f}, {r['reverse_step_off_on'][1]:.3f}\n")
        if args.note:
            fh.write("\n" + args.note + "\n")
Prog._state.close(); Setup.mesh.close()
