#!/usr/bin/env python3
"""GPU box helper: what the vertical momentum pass (moka_set_vertical_viscosity, moka_surface_stress_upload) costs per RK4 step, in
both of its forms, against the same step with the pass off, in one process.

Per round the legs alternate: kernel variant 0 (the pass in its tile form) with the pass off / nuV only / nuV + drag + stress, then
kernel variant 3 (the column form; the dycore runs its generic kernels there, so that form has an off leg of its own).  Each
repetition is one RK4 step between two moka_mark; the pass is the difference of the medians of two legs.  Beside it, from the same
run: the copy rate of moka_bw_probe and the pass's bytes at that rate -- u in and out and the unique bytes of h_new,
(2 nEdges + nCells) K 8.

--field adds the legs of a viscosity per interface and edge (moka_vertical_viscosity_field_upload): "fld" (the field alone) and
"fldall" (field + drag + stress), whose pass reads K nEdges 8 bytes more.  --adjoint times, the same way, one reversed step of a
moka_forced_tape (moka_forced_adjoint_sweep over one recorded step: the transposed pass, the cell gather and the four transposed RK
stages) with the pass off, with the scalar nuV (four column sets a tile) and with the field (five), DF flagged in a fourth leg.

--quadratic adds the legs of the quadratic bottom drag (moka_set_quadratic_bottom_drag; Cd with dt Cd sp / hm = 1/2 at the rms speed of
the state): "lin" (nuV + r, the linear drag the others are read against), "qd" (nuV + Cd), "qdlin" (nuV + r + Cd), "qdall" (+ stress);
the step then issues the bottom-speed launch in front of the pass.

    python3 tools/momentum_vmix_timing.py [--small] [--field] [--quadratic] [--adjoint] [--rounds R] [--steps N] [--out FILE]"""
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
from moka_hip import lib as L              # noqa: E402
from moka_hip import meshgen as mg         # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--small", action="store_true")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--field", action="store_true")
ap.add_argument("--quadratic", action="store_true")
ap.add_argument("--adjoint", action="store_true")
ap.add_argument("--out", default=None)
args = ap.parse_args()

m, K = (64 if args.small else 320), 60
mesh = mg.icosahedral_mesh(m)
ssh, u, h, rest, dts = mg.sphere_synthetic_state(mesh, K)
cfg = {"time_management": {"config_start_time": dt.datetime(1, 1, 1), "config_run_duration": dt.timedelta(hours=1)},
       "time_integration": {"config_dt": dt.timedelta(seconds=dts), "config_number_of_time_levels": 2}}
b = mk.MokaHIP(0)
hm = float(np.mean(h))
nu, drag = 4.0 * hm * hm / dts, 0.5 * hm / dts          # s / hm^2 = 4, q / hm = 1/2
tau = np.random.default_rng(1).uniform(-1.0, 1.0, mesh.nEdges) * hm / dts
Setup, Diag, Tend, Prog = mk.ocn_init_from_arrays(mesh, ssh, u, h, rest, cfg, b, multilayer=True)
med = statistics.median
sh = Prog._state._h
LEGS = (("off", 0, {}), ("nu", 0, {"viscosity": nu}), ("all", 0, {"viscosity": nu, "bottom_drag": drag, "surface_stress": tau}),
        ("off3", 3, {}), ("nu3", 3, {"viscosity": nu}), ("all3", 3, {"viscosity": nu, "bottom_drag": drag, "surface_stress": tau}))
if args.field:
    # surface-intensified: 4 nuV at the first interface, falling to nuV / 4 at depth, a different factor in [0.5, 1.5] per edge
    fld = (nu * np.linspace(4.0, 0.25, K)[None, :] * np.random.default_rng(2).uniform(0.5, 1.5, (mesh.nEdges, 1))).copy()
    LEGS += (("fld", 0, {"viscosity_field": fld}), ("fldall", 0, {"viscosity_field": fld, "bottom_drag": drag, "surface_stress": tau}),
             ("fld3", 3, {"viscosity_field": fld}), ("fldall3", 3, {"viscosity_field": fld, "bottom_drag": drag, "surface_stress": tau}))
if args.quadratic:
    cd = drag / max(float(np.sqrt(np.mean(u ** 2))), 1e-30)
    for v, sfx in ((0, ""), (3, "3")):
        LEGS += (("lin" + sfx, v, {"viscosity": nu, "bottom_drag": drag}), ("qd" + sfx, v, {"viscosity": nu, "quadratic_drag": cd}),
                 ("qdlin" + sfx, v, {"viscosity": nu, "bottom_drag": drag, "quadratic_drag": cd}),
                 ("qdall" + sfx, v, {"viscosity": nu, "bottom_drag": drag, "surface_stress": tau, "quadratic_drag": cd}))
ms = {name: [] for name, _, _ in LEGS}
paths = {}
for _ in range(args.rounds):
    for name, variant, kw in LEGS:
        b.set_kernel_variant(variant)
        mk.set_vertical_mixing(Prog, **kw)
        for rep in range(args.warmup + args.steps):
            b.synchronize()
            b.marks_reset()
            b.mark()
            L.check(L.lib().moka_step_rk4(sh, dts), b._h)
            b.mark()
            b.synchronize()
            if rep >= args.warmup:
                ms[name].append(list(b.marks_read())[0])
        paths[name] = mk.momentum_vmix_path(Prog)
b.set_kernel_variant(0)
mk.set_vertical_mixing(Prog)
bw = b.bw_probe()
nC, nE = mesh.nCells, mesh.nEdges
bound = (2 * nE + nC) * K * 8 / (bw.get("copy_GBs") * 1e9) * 1e3
rows = []
extra = (("fld", "fldall") if args.field else ()) + (("lin", "qd", "qdlin", "qdall") if args.quadratic else ())
for form, off, legs in (("tile", "off", ("nu", "all") + extra), ("column", "off3", ("nu3", "all3") + tuple(x + "3" for x in extra))):
    for leg in legs:
        p = med(ms[leg]) - med(ms[off])
        rows.append({"form": form, "path": paths[leg], "switches": leg.rstrip("3"), "step_off_ms": med(ms[off]), "step_on_ms": med(ms[leg]),
                     "pass_ms": p, "share_of_byte_bound": bound / p if p > 0 else None,
                     "step_on_min_max": (min(ms[leg]), max(ms[leg])), "step_off_min_max": (min(ms[off]), max(ms[off]))})
adj = []
if args.adjoint:
    ALEGS = (("off", {}, False), ("nu", {"viscosity": nu, "bottom_drag": drag}, False)) + \
        ((("fld", {"viscosity_field": fld, "bottom_drag": drag}, False), ("fld+DF", {"viscosity_field": fld, "bottom_drag": drag}, True))
         if args.field else ())
    ams, apaths = {name: [] for name, _, _ in ALEGS}, {}
    for _ in range(args.rounds):
        for name, kw, want in ALEGS:
            mk.set_vertical_mixing(Prog, **kw)
            tape = mk.ForcedAdjointTape(Prog, 1)
            tape.want_gradient(viscosity_field=want)
            for rep in range(args.warmup + args.steps):
                tape.step(dts)
                L.check(L.lib().moka_forced_adjoint_seed_sum_sq_ssh(tape._h), b._h)
                b.synchronize()
                b.marks_reset()
                b.mark()
                tape.sweep()
                b.mark()
                b.synchronize()
                if rep >= args.warmup:
                    ams[name].append(list(b.marks_read())[0])
            apaths[name] = tape.vmix_path()
            tape.close()
    mk.set_vertical_mixing(Prog)
    for name, _, _ in ALEGS:
        adj.append({"leg": name, "path": apaths[name], "sweep_ms": med(ams[name]), "pass_ms": med(ams[name]) - med(ams["off"]),
                    "min_max": (min(ams[name]), max(ams[name]))})
result = {"cells": nC, "edges": nE, "K": K, "rounds": args.rounds, "steps_per_round": args.steps, "copy_GBs": bw.get("copy_GBs"),
          "byte_bound_ms": bound, "rows": rows, "adjoint": adj}
print(json.dumps(result), flush=True)
if args.out:
    with open(args.out, "w") as fh:
        fh.write(f"The vertical momentum pass beside the same RK4 step with the pass off -- {nC} cells, {nE} edges x {K} levels, fp64, linear dycore,\n"
                 f"s / hm^2 = 4, q / hm = 1/2, one MI355X.  tools/momentum_vmix_timing.py ({args.rounds} rounds x {args.steps} repetitions after "
                 f"{args.warmup} warm-up, the legs\nalternated in one process; medians of moka_mark intervals around one step; the pass = on - off).\n"
                 f"Copy rate of the same run (moka_bw_probe): {result['copy_GBs']:.0f} GB/s; (2 nEdges + nCells) K 8 B at that rate: {bound:.3f} ms.\n\n"
                 "   form     switches   step ms (off, on)     pass ms   byte bound / pass   step on min .. max\n")
        for r in rows:
            fh.write(f"   {r['form']:<8s} {r['switches']:<10s} {r['step_off_ms']:<9.3f} {r['step_on_ms']:<11.3f} {r['pass_ms']:<9.3f} "
                     f"{(r['share_of_byte_bound'] or 0):<19.3f} {r['step_on_min_max'][0]:.3f} .. {r['step_on_min_max'][1]:.3f}\n")
        if adj:
            fh.write("\nOne reversed step of a moka_forced_tape (sweep over one recorded step; the pass = leg - off):\n"
                     "   leg        path   sweep ms   pass ms    min .. max\n")
            for r in adj:
                fh.write(f"   {r['leg']:<10s} {r['path']:<6d} {r['sweep_ms']:<10.3f} {r['pass_ms']:<10.3f} {r['min_max'][0]:.3f} .. {r['min_max'][1]:.3f}\n")
Prog._state.close(); Setup.mesh.close()
