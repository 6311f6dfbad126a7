#!/usr/bin/env python3
"""GPU box helper for a kernel trace: two taped RK4 steps and their sweep of a small model with three tracers and vertical
diffusivities (5, 0, 2), on a tape without a flag (`plain`: only calls the commit before has too, so the same script runs on its tree)
or with tracers 0 and 1 flagged for d J / d kappaV (`flag`).  Run each mode under a kernel trace and compare the dispatch counts per
kernel: `plain` must agree name by name with the commit before and hold no k_vmix_*_grad dispatch.

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python3 tools/tracer_vgrad_launches.py plain|flag"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mpas-ocean.jl_amd"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import moka_hip as mk                      # noqa: E402
import tracer_cases as tc                  # noqa: E402

mode = sys.argv[1]
b = mk.MokaHIP(0)
md = tc.Model(b, "planar", 60)
f = tc.distinct_fields(md.mesh, 60, 3)
tr = mk.set_tracers(md.Prog, f, vertical=[5.0, 0.0, 2.0])
tape = mk.TracerAdjointTape(md.Prog, 2)
if mode == "flag":
    tape.want_vertical_gradient(0)
    tape.want_vertical_gradient(1)
tape.step(md.dt)
tape.step(md.dt)
tape.gradient(f)
print(mode, "vmix paths (forward, reverse):", tr.vmix_path(), tape.vmix_path())
tape.close()
md.close()
b.close()
