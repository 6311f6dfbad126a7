#!/usr/bin/env python3
"""GPU box helper for a kernel trace: three RK4 steps, one taped step and its sweep of a small model with three tracers, with the
vertical diffusivities never set (`never`), set to zeros (`zeros`) or set (`on`).  Run each mode under a kernel trace and compare the
dispatch counts per kernel: `never` and `zeros` must agree name by name and hold no k_vmix_* dispatch.

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python3 tools/tracer_vmix_launches.py never|zeros|on"""
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
vertical = {"never": None, "zeros": [0.0, 0.0, 0.0], "on": [5.0, 0.0, 2.0]}[mode]
tr = mk.set_tracers(md.Prog, f, vertical=vertical)
md.eager(3)
tape = mk.TracerAdjointTape(md.Prog, 1)
tape.step(md.dt)
tape.gradient(f)
print(mode, "vmix paths (forward, reverse):", tr.vmix_path(), tape.vmix_path())
tape.close()
md.close()
b.close()
