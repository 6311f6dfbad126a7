#!/usr/bin/env python3
"""bench.py -- cell-updates/s per RK4 step + achieved HBM GB/s of the fused stage kernel.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]

A "step" is one full 4-stage RK4 step of the shallow-water dycore over the whole synthetic mesh
(BASELINE.json metric).  Default workload = BASELINE config 4: ~1 M-cell (1 024 002) icosahedral
sphere x 60 layers, fp64, inputs resident in HBM before the timed region starts.
For N > 1 the driver launches this file under torch.distributed.run (one rank per GPU); the mesh is
partitioned across ranks (strong scaling) and halos are exchanged once per RK stage.
Prints ONE JSON line on rank 0.

A plain run does what the headline needs and no more: set-up (mesh, plan, upload, the library's placement search; for N > 1
the halo transport choice), W warm-up steps, K timed steps, the outputs (--dump-outputs), the line.
  * `value` / `ms_per_step` come from the MEDIAN of the K per-step times (one HIP event per step on the library's compute
    stream, max over ranks per step); the mean over the barrier-bracketed wall region is kept as `ms_per_step_wall_mean`;
  * `n_gpus` = DISTINCT devices the ranks use (`ranks`, `n_devices_visible`, `ranks_per_device`, `rehearsal`);
  * --dump-outputs DIR: the prognostic state the last timed step left (ssh, normalVelocity, layerThickness of the current
    time level) as DIR/<name>.npy in float64 -- every row, or a fixed seeded sample of rows where that exceeds 64 MiB.
--full adds what takes runs of its own, after the timed region:
  * `calibration`: a plain 16-byte-per-lane copy and a read-only sweep of a 4 GiB buffer timed with HIP events on the same
    stream right before the set-up and right after the timed region, plus the device's clock / power files from sysfs --
    so a slow box and a slow build can be told apart (`roofline.frac_of_copy_this_run`);
  * per-stage rooflines, the tendency / Forward-Euler / 13-stream entries and clocks under load (N = 1), the exchange report
    (N > 1), the CPU baselines (N = 1; --no-cpu drops them);
  * `config5`: BASELINE config 5 (3 696 642 cells x 80 layers, fp32 storage / fp64 arithmetic) timed in the same run
    (--no-config5 drops it).
"""
import argparse
import datetime as dt
import glob
import json
import os
import socket
import statistics
import sys
import time

os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # dmabuf IPC: what RCCL between processes needs on this driver stack

ROOT = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.join(ROOT, "mpas-ocean.jl_amd"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402,F401

HBM_PEAK_GBS = 8000.0          # MI355X_MICROARCH.md: 8.0 TB/s spec
HBM_COPY_GBS = 6290.0          # the guide's float4 copy ceiling; the same-run probe is what frac_of_copy_this_run uses
PROBE_BYTES = 4 << 30          # footprint of the same-run bandwidth probe (2 GiB source + 2 GiB destination)
DUMP_BYTES = 64 << 20          # --dump-outputs: upper limit of all files together
DUMP_SEED = 20251016           # --dump-outputs: the row sample where the whole state exceeds DUMP_BYTES

WORKLOADS = {
    # name: (icosahedral frequency m, layers[, state bytes, Schmidt stretch])  -- SURVEY.md section 8 size table
    "config4_1M_x60": (320, 60),
    "config3_41k_x60": (64, 60),
    "exp_1M_x64": (320, 64),          # experiment: 512-byte rows (cache-line aligned)
    "config2_41k_x1": (64, 1),
    "small_10k_x60": (32, 60),
    # BASELINE config 5: variable-resolution (~3-52 km) 3 696 642-cell sphere x 80 layers, fp32 state / fp64 arithmetic
    "config5_3.7M_x80_f32": (608, 80, 4, 4.47),
    "small_41k_x80_f32": (64, 80, 4, 4.47),
}


def algorithmic_bytes(nC, nE, K, S=8, I=4):
    """the one formula for algorithmic bytes (the contract formula: 5 streams per RK stage 1-3,
    3 for stage 4 = 18 per step)."""
    nnzEE = 10 * nE - 60
    nnzEC = 2 * nE
    b_mesh = nE * (2 * I + 3 * 8 + 2 * I) + nnzEE * (I + 8) + nnzEC * 2 * I + nC * (I + 8 + 8)
    b_tend = 2 * S * K * (nE + nC) + b_mesh
    b_step = 18 * S * K * (nE + nC) + 4 * b_mesh
    return b_mesh, b_tend, b_step


# State streams (one stream = S*K*(nE+nC) bytes) the stage-s launch has to move AT LEAST, aliasing taken into account:
# stage 1: Provis == Curr == the current level and New starts from it -> read 1, write Provis' and New = 3 (the contract
# formula counts 5); stages 2, 3: read Provis, Curr, New, write Provis', New' = 5; stage 4: read Provis, New, write New = 3.
STAGE_MIN_STREAMS = (3, 5, 5, 3)
STAGE_CONTRACT_STREAMS = (5, 5, 5, 3)


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def get_mesh(m, stretch=1.0):
    from moka_hip import meshgen as mg
    t0 = time.time()
    mesh = mg.icosahedral_mesh(m, stretch=stretch)
    log(f"[bench] mesh m={m}: {mesh.nCells} cells, {mesh.nEdges} edges built in {time.time() - t0:.1f}s")
    return mesh


def host_cores():
    """Threads this process may really use: affinity mask, cgroup quota, and the 16-core share a one-GPU box
    is given (oversubscribing the 256 hardware threads it *shows* made the OpenMP leg slower than 1 thread)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()
        if q != "max":
            n = min(n, max(1, int(float(q) / float(per))))
    except Exception:
        pass
    return max(1, min(n, int(os.environ.get("MOKA_BENCH_THREADS", "16"))))


# ---------------------------------------------------------------------------------------------------------------------
# clock / power state (plain sysfs reads; nothing here touches the GPU)
# ---------------------------------------------------------------------------------------------------------------------
def _read(path):
    try:
        with open(path) as f:
            return f.read()
    except Exception:
        return None


def _dpm_current(text):
    """'0: 500Mhz\\n1: 2394Mhz *\\n2: 2400Mhz' -> 2394 (MHz of the starred line), None when unreadable."""
    if not text:
        return None
    for line in text.splitlines():
        if line.rstrip().endswith("*"):
            for tok in line.replace("*", " ").split():
                t = tok.lower()
                if t.endswith("mhz"):
                    try:
                        return float(t[:-3])
                    except ValueError:
                        return None
    return None


def _power_watts(devdir):
    for name in ("power1_average", "power1_input"):
        for f in glob.glob(os.path.join(devdir, "hwmon", "hwmon*", name)):
            t = _read(f)
            if t:
                try:
                    return float(t.strip()) / 1e6
                except ValueError:
                    pass
    return None


def device_sysfs(pci_bus_id):
    """sclk / mclk / fclk (MHz, the current DPM level) and package power (W) of the device at `pci_bus_id`, plus the power of
    the OTHER GPUs of the host (a one-GPU box is a slice of an 8-GPU machine whose other cards may be busy)."""
    base = "/sys/bus/pci/devices"
    dev = os.path.join(base, pci_bus_id)
    out = {"pci_bus_id": pci_bus_id}
    if not os.path.isdir(dev):
        out["note"] = "device not found in sysfs"
        return out
    for k in ("sclk", "mclk", "fclk"):
        out[k + "_mhz"] = _dpm_current(_read(os.path.join(dev, "pp_dpm_" + k)))
    out["power_w"] = _power_watts(dev)
    busy = _read(os.path.join(dev, "gpu_busy_percent"))
    if busy and busy.strip().isdigit():
        out["busy_percent"] = int(busy.strip())
    mbusy = _read(os.path.join(dev, "mem_busy_percent"))
    if mbusy and mbusy.strip().isdigit():
        out["mem_busy_percent"] = int(mbusy.strip())
    # temperatures (hwmon: edge / junction / mem, millidegrees): HBM refreshes twice as often when hot
    temps = {}
    for t in glob.glob(os.path.join(dev, "hwmon", "hwmon*", "temp*_input")):
        label = (_read(t.replace("_input", "_label")) or os.path.basename(t)).strip()
        v = _read(t)
        if v and v.strip().lstrip("-").isdigit():
            temps[label] = round(int(v.strip()) / 1000.0, 1)
    if temps:
        out["temp_c"] = temps
    others = []
    for card in sorted(glob.glob("/sys/class/drm/card[0-9]*")):
        if "-" in os.path.basename(card):
            continue
        d = os.path.realpath(os.path.join(card, "device"))
        if os.path.basename(d).lower() == pci_bus_id.lower():
            continue
        w = _power_watts(d)
        if w is not None:
            others.append(round(w, 1))
    out["other_gpus_power_w"] = others
    return out


# ---------------------------------------------------------------------------------------------------------------------
# CPU baseline legs (the oracle as the timed thing: the only place bench.py uses it)
# ---------------------------------------------------------------------------------------------------------------------
def cpu_baseline(mesh, K, ssh, u, h, rest, dts, budget_s=25.0, mixed=False):
    """Oracle (C restatement of the reference loop nests) timed on this box's host cores: clean RK4 step,
    all cores (OpenMP), on the same mesh when one step fits the budget, else on a smaller sphere."""
    import oracle as orc
    cores = host_cores()
    orc.set_threads(cores)
    om = orc.OracleMesh(mesh, K, resting_thickness_sum=rest.sum(1), max_level_edge_top=K)
    st = orc.OracleState(om, ssh, u, h, mixed=mixed)
    t0 = time.time()
    st.step_rk4(dts)                   # warm-up (page faults) and a size probe
    t_probe = time.time() - t0
    n = max(1, min(5, int(budget_s / max(t_probe, 1e-3)) - 1))
    if t_probe > budget_s:
        n = 0
    t0 = time.time()
    for _ in range(n):
        st.step_rk4(dts)
    t = (time.time() - t0) / n if n else t_probe
    out = {"value": mesh.nCells * K / t, "unit": "cell-updates/s", "cores": cores, "kind": "port",
           "sample": f"{max(n, 1)} RK4 step(s) on {mesh.nCells} cells x {K} layers, "
                     f"oracle/moka_oracle.c with OpenMP on {cores} host threads (the box's CPU share for one GPU)",
           "ms_per_step": t * 1e3}
    if not mixed:
        # the reference's live path: reference_compat Forward-Euler steps (time_integration.jl:150-193), same threads
        fe = orc.OracleState(om, ssh, u, h)
        flags = orc.FE_REFERENCE_COMPAT if K == 1 else (orc.FE_REFERENCE_COMPAT & ~4)
        fe.step_fe(dts, flags)
        t0 = time.time()
        nf = 0
        while nf < 8 and time.time() - t0 < budget_s / 3:
            fe.step_fe(dts, flags)
            nf += 1
        out["forward_euler_compat"] = {"value": mesh.nCells * K / ((time.time() - t0) / nf), "unit": "cell-updates/s",
                                       "sample": f"{nf} reference_compat FE steps, same mesh and threads"}
    orc.set_threads(1)
    return out


def cpu_baseline_1t(mesh, K, ssh, u, h, rest, dts, budget_s=12.0, mixed=False):
    """Single-thread figure (what `julia mpas_ocean.jl` gives with JULIA_NUM_THREADS=1) on the SAME mesh as the GPU line:
    one warm-up step is the size probe; then as many steps as fit the budget (at least one)."""
    import oracle as orc
    orc.set_threads(1)
    om = orc.OracleMesh(mesh, K, resting_thickness_sum=rest.sum(1), max_level_edge_top=K)
    st = orc.OracleState(om, ssh, u, h, mixed=mixed)
    t0 = time.time()
    st.step_rk4(dts)
    t_probe = time.time() - t0
    n = max(1, min(5, int(budget_s / max(t_probe, 1e-3))))
    t0 = time.time()
    for _ in range(n):
        st.step_rk4(dts)
    t = (time.time() - t0) / n
    return {"value": mesh.nCells * K / t, "unit": "cell-updates/s", "cores": 1, "kind": "port",
            "sample": f"{n} RK4 step(s) on {mesh.nCells} cells x {K} layers (the GPU line's mesh), 1 thread",
            "ms_per_step": t * 1e3}


# ---------------------------------------------------------------------------------------------------------------------
# RCCL probe (child process)
# ---------------------------------------------------------------------------------------------------------------------
def rccl_probe_child(backend="nccl"):
    """Child process of probe_rccl: bring RCCL up between the ranks and move a few bytes the two ways the halo transports
    do (all_to_all_single with uneven splits, batched isend / irecv).  Exit code 0 = it works on this node.
    (backend = "gloo" runs the same exchange on CPU tensors: the rendezvous logic can then be tested without a GPU.)"""
    import torch
    import torch.distributed as dist
    rank, world, local = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"]), int(os.environ.get("LOCAL_RANK", "0"))
    if backend == "nccl":
        ndev = max(torch.cuda.device_count(), 1)
        if ndev < world:
            print(f"[rccl-probe] {world} ranks on {ndev} device(s): RCCL needs one device per rank", file=sys.stderr)
            sys.exit(3)
        torch.cuda.set_device(local % ndev)
        dev = torch.device("cuda", local % ndev)
        dist.init_process_group("nccl", device_id=dev, timeout=dt.timedelta(seconds=60))
    else:
        dev = torch.device("cpu")
        dist.init_process_group("gloo", timeout=dt.timedelta(seconds=60))
    ins = [(rank + q) % 3 + 1 if q != rank else 0 for q in range(world)]
    outs = [(q + rank) % 3 + 1 if q != rank else 0 for q in range(world)]
    send = torch.full((sum(ins),), float(rank), device=dev, dtype=torch.float64)
    recv = torch.zeros(sum(outs), device=dev, dtype=torch.float64)
    dist.all_to_all_single(recv, send, outs, ins)
    exp = torch.cat([torch.full((outs[q],), float(q), dtype=torch.float64) for q in range(world)])
    ok = torch.equal(recv.cpu(), exp)
    nxt, prv = (rank + 1) % world, (rank - 1) % world
    a, b = torch.full((5,), float(rank), device=dev), torch.zeros(5, device=dev)
    for w in dist.batch_isend_irecv([dist.P2POp(dist.irecv, b, prv), dist.P2POp(dist.isend, a, nxt)]):
        w.wait()
    if backend == "nccl":
        torch.cuda.synchronize()
    ok = ok and bool((b.cpu() == float(prv)).all())
    dist.barrier()
    dist.destroy_process_group()
    sys.exit(0 if ok else 4)


def probe_rccl(timeout_s=120, backend="nccl"):
    """Does RCCL work between the ranks of this launch?  Answered by a CHILD process per rank (its own rendezvous port),
    started before this process has touched the GPU: a wedged RCCL collective does not raise, it hangs until a watchdog
    kills the process -- so the risk is taken by a process whose only job is to take it.  True = every step ran.
    (A child that does not finish is killed and reported; this process goes on with the other transports -- nothing is
    ever re-exec'ed.)"""
    import subprocess
    env = dict(os.environ)
    env["MASTER_PORT"] = str(int(os.environ.get("MASTER_PORT", "29500")) + 23)
    env["MASTER_ADDR"] = os.environ.get("MASTER_ADDR", "127.0.0.1")
    # under torch.distributed.run the ranks are told to use the AGENT's store at MASTER_PORT; the children rendezvous among
    # themselves on another port, where child rank 0 has to host the store
    for k in [k for k in env if k.startswith("TORCHELASTIC_")]:
        env.pop(k)
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--rccl-probe", backend], env=env, timeout=timeout_s,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode != 0:
            log(f"[bench] RCCL probe failed (exit {r.returncode}): {r.stdout.strip().splitlines()[-1:] }")
        return r.returncode == 0
    except subprocess.TimeoutExpired:
        log(f"[bench] RCCL probe did not finish within {timeout_s} s (killed)")
        return False


# ---------------------------------------------------------------------------------------------------------------------
# measurement helpers
# ---------------------------------------------------------------------------------------------------------------------
def step_stats(ms):
    s = sorted(ms)
    med = statistics.median(s)
    # strays: samples beyond 1.5x the median -- single launches of 23-25 ms (the device stalls inside a kernel's own begin -> end
    # stamps) were seen in two traced runs of round 4; they move a mean, not the median the line reports
    return {"median": med, "min": s[0], "max": s[-1], "mean": sum(s) / len(s), "n": len(s), "strays": sum(1 for x in s if x > 1.5 * med)}


def calibrate(backend, tag):
    """One probe of the device as it is right now: copy / read rates (HIP events on the compute stream) + sysfs state."""
    t0 = time.time()
    cal = backend.bw_probe(PROBE_BYTES, 5)
    cal["sysfs"] = device_sysfs(backend.pci_bus_id())
    cal["probe_s"] = round(time.time() - t0, 2)
    log(f"[bench] calibration {tag}: copy {cal['copy_GBs']:.0f} GB/s (mean {cal['copy_GBs_mean']:.0f}), read {cal['read_GBs']:.0f} GB/s, "
        f"row gather {cal['gather_GBs']:.0f} GB/s, 3 reads + 2 writes {cal.get('streams5_GBs', float('nan')):.0f} GB/s, "
        f"128 MiB re-read {cal.get('reread128_GBs', float('nan')):.0f} GB/s, row gather over 32 GiB {cal.get('gather32G_GBs', float('nan')):.0f} GB/s, "
        f"sclk {cal['sysfs'].get('sclk_mhz')} MHz, {cal['sysfs'].get('power_w')} W")
    return cal


def under_load(backend, fn, seconds=1.0, batch=10):
    """Clock and power WHILE launches run: `fn` called back to back for ~`seconds` while a thread samples sysfs every 4 ms (the
    reads in calibrate() happen between timed regions, when the device idles at 2.4 GHz and < 400 W).  Every stage launch of this
    library runs the package at its power limit and the shader clock gives way (profiles/r04_variants.txt section 4): these figures
    say how far, on this box, in this run.  Outside every timed region."""
    import threading
    pci = backend.pci_bus_id()
    samples, stop = [], threading.Event()

    def sampler():
        while not stop.is_set():
            d = device_sysfs(pci)
            samples.append((d.get("sclk_mhz"), d.get("power_w"), d.get("fclk_mhz"), d.get("mclk_mhz")))
            time.sleep(0.004)
    th = threading.Thread(target=sampler, daemon=True)
    backend.synchronize()
    th.start()
    t0, n = time.perf_counter(), 0
    while time.perf_counter() - t0 < seconds:
        for _ in range(batch):
            fn()
        backend.synchronize()
        n += batch
    el = time.perf_counter() - t0
    stop.set()
    th.join()
    tail = samples[len(samples) // 4:]                    # the sensors average over tens of ms: drop the ramp
    col = lambda i: [x[i] for x in tail if x[i] is not None]  # noqa: E731
    mean = lambda v: (sum(v) / len(v)) if v else None         # noqa: E731
    return {"ms_per_call_sustained": el / max(n, 1) * 1e3, "calls": n, "sclk_mhz_mean": mean(col(0)), "sclk_mhz_min": min(col(0), default=None),
            "power_w_mean": mean(col(1)), "power_w_max": max(col(1), default=None), "fclk_mhz": mean(col(2)), "mclk_mhz": mean(col(3)),
            "samples": len(tail)}


def timed_steps(backend, step, steps, warmup, sync_all):
    """W warm-up steps, then exactly K timed steps between barrier + synchronize on both sides, with one HIP event per step on
    the compute stream.  Returns (wall seconds, [ms per step])."""
    import gc
    gc.collect()          # BEFORE the warm-up: a collection between warm-up and timed region is a host pause in which the device
    gc.disable()          # idles, clocks up and then meets its power limit again inside the timed steps.  (Disabled: a 24 ms
                          # host-side pause was seen once inside a 136 ms timed region; the collector is the one source of such
                          # pauses this process controls.)
    for _ in range(warmup):
        step()
    backend.marks_reset()
    sync_all()
    t0 = time.perf_counter()
    backend.mark()
    for _ in range(steps):
        step()
        backend.mark()
    sync_all()
    t1 = time.perf_counter()
    gc.enable()
    return t1 - t0, backend.marks_read()


def stage_rooflines(backend, step, nrec, stream_bytes, b_mesh, modes=(1, 2, 2, 3)):
    """Per-stage launch durations: a pass of the same steps with one HIP event between the launches."""
    settle(backend, step, batch=2)           # (the figures are means over the recorded steps: no transient among them)
    backend.stage_timing(True)
    for _ in range(nrec):
        step()
    ms4, nst = backend.stage_timing_read()
    backend.stage_timing(False)
    per_stage = []
    for sidx, ms in enumerate(ms4):
        bc = STAGE_CONTRACT_STREAMS[sidx] * stream_bytes + b_mesh
        bm = STAGE_MIN_STREAMS[sidx] * stream_bytes + b_mesh
        per_stage.append({"stage": sidx + 1, "kernel_mode": modes[sidx], "ms": ms,
                          "bytes_contract": bc, "frac_contract": bc / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                          "bytes_minimum": bm, "frac_minimum": bm / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS})
    return per_stage, nst, sum(ms4)


def rk4_13_stream_entry(mk, backend, step, steps, warmup, nCK, stream_bytes, b_mesh, b_step):
    """Second RK4 entry of the line: the opt-in 13-stream form (moka_set_tuning key 7; Float64 states on
    whole meshes).  NOT the reference's round-off (tests bound it: <= 1e-12 relative per step), so it is reported beside the
    headline, never as it: ms per step, the metric, `frac` on the contract bytes (the judge's formula) and on ITS OWN minimum
    bytes (13 state streams: 2 / 3 / 3 / 5), per stage."""
    from moka_hip import lib as _L
    _L.check(_L.lib().moka_set_tuning(7, 1))
    try:
        wall, ms = timed_steps(backend, step, steps, warmup, backend.synchronize)
        st = step_stats(ms)
        backend.stage_timing(True)
        for _ in range(min(steps, 10)):
            step()
        ms4, nst = backend.stage_timing_read()
        backend.stage_timing(False)
    finally:
        _L.check(_L.lib().moka_set_tuning(7, 0))
    step()                                   # (back in the reference's form: the buffer roles settle again)
    streams = (2, 3, 3, 5)
    own = sum(streams) * stream_bytes + 4 * b_mesh
    t = st["median"] * 1e-3
    return {"ms_per_step": st["median"], "step_ms": st, "value": nCK / t, "unit": "cell-updates/s",
            "frac_contract_bytes": b_step / t / 1e9 / HBM_PEAK_GBS, "own_minimum_bytes": own, "frac_own_minimum_bytes": own / t / 1e9 / HBM_PEAK_GBS,
            "per_stage": [{"stage": i + 1, "kernel_mode": (7, 8, 8, 9)[i], "ms": ms4[i], "state_streams": streams[i],
                           "frac_own_bytes": (streams[i] * stream_bytes + b_mesh) / (ms4[i] * 1e-3) / 1e9 / HBM_PEAK_GBS} for i in range(4)],
            "note": "moka_set_tuning(7, 1): stages 1-3 store only the provisional states, stage 4 forms New = C + ((P2 - C) + 2 (P3 - C) + "
                    "(P4 - C)) / 3 + dt/6 k4 from own rows; same Runge-Kutta step, other round-off than the reference's running sum "
                    "(time_integration.jl:134-135): opt-in, default off"}


def settle(backend, fn, seconds=0.05, batch=3):
    """Untimed launches of `fn` for `seconds`: behind any host pause the device needs ~35 ms of launches to be back in its
    steady state (power-limited clocks; tools/step_series.py: the first five RK4 steps behind a 50 ms pause run 13 ... 1 % slow).
    The main timed region has the driver's warm-up steps for that; the shorter loops below get this."""
    t0 = time.perf_counter()
    while True:
        for _ in range(batch):
            fn()
        backend.synchronize()
        if time.perf_counter() - t0 >= seconds:
            return


def single_gpu_extras(mk, backend, Setup, Diag, Tend, Prog, K, sbytes, dts, b_tend, iters):
    """The pure tendency launch (north_star's 40 % target is quoted on it) and the reference's live integrator."""
    out = {}
    mesh = Setup.mesh
    settle(backend, lambda: mk.computeTendency(mesh, Diag, Prog, Tend))
    backend.marks_reset(); backend.mark()
    for _ in range(iters):
        mk.computeTendency(mesh, Diag, Prog, Tend)
        backend.mark()                       # one HIP event per launch: the median is what is reported, like the step time
    per = sorted(backend.marks_read())
    tms = per[len(per) // 2]
    out["tendency_kernel"] = {"avg_launch_ms": tms, "launch_ms": {"median": tms, "min": per[0], "max": per[-1], "mean": sum(per) / len(per), "n": len(per)},
                              "algorithmic_bytes": b_tend,
                              "achieved_GBs": b_tend / (tms * 1e-3) / 1e9,
                              "frac_of_peak": b_tend / (tms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                              "note": "moka_tendencies back to back, one HIP event per launch; avg_launch_ms = the MEDIAN launch (one stray "
                                      "launch of 24.6 ms among ten pulled a mean from 3.76 to 5.84 ms in a traced run of round 4)"}
    # the reference's live integrator: reference_compat Forward-Euler steps (time_integration.jl:150-193), for the record.
    # Default = lean steps: the new time level and relativeVorticity are stored every step, the step's other DiagnosticVars /
    # TendencyVars are produced on the first read (bit-identical: tests) -- so the line also carries the step that stores
    # every array every step (moka_set_tuning(4, 0)).
    from moka_hip import lib as _L
    fe_flags = mk.REFERENCE_COMPAT if K == 1 else (mk.REFERENCE_COMPAT & ~4)
    nC = mesh.HorzMesh.data.nCells

    def fe_ms(lean):
        _L.check(_L.lib().moka_set_tuning(4, 1 if lean else 0))
        if sbytes == 4:     # an fp32-storage state has no DiagnosticVars to carry over right after RK4 steps
            mk.ocn_timestep(dts, Prog, Diag, Tend, Setup, mk.ForwardEuler, flags=0)
        settle(backend, lambda: mk.ocn_timestep(dts, Prog, Diag, Tend, Setup, mk.ForwardEuler, flags=fe_flags))
        backend.marks_reset(); backend.mark()
        for _ in range(iters):
            mk.ocn_timestep(dts, Prog, Diag, Tend, Setup, mk.ForwardEuler, flags=fe_flags)
            backend.mark()
        ms = step_stats(backend.marks_read())["median"]
        pending = int(_L.lib().moka_fe_lazy_pending(Prog._state._h))
        return ms, pending
    try:
        eager_ms, _ = fe_ms(False)
        lean_ms, pending = fe_ms(True)
    finally:
        _L.check(_L.lib().moka_set_tuning(4, 1))
    out["forward_euler_compat"] = {"ms_per_step": lean_ms, "value": nC * K / (lean_ms * 1e-3), "unit": "cell-updates/s",
                                   "arrays_pending_after_a_step": pending,
                                   "ms_per_step_all_arrays_stored": eager_ms, "value_all_arrays_stored": nC * K / (eager_ms * 1e-3),
                                   "note": "moka_step_fe, reference_compat flags (stale layerThicknessEdge, accumulating relativeVorticity), all "
                                           "levels, median of per-step HIP-event times; ms_per_step = lean steps (new level + relativeVorticity "
                                           "stored, tendencies / thicknessFlux / velocityDivCell / layerThicknessEdge on first read), "
                                           "ms_per_step_all_arrays_stored = every array stored every step"}
    return out


def exchange_report(mk, backend, model, step, sync_all, dist, group, rank, world, args, whole, ms_per_step):
    """N > 1: WHERE a shortfall against N x comes from.  A second pass of the same steps with the library's
    exchange statistics on (moka_halo_stats): per rank the host time inside moka_halo_push_wait, waiting for the own push kernel,
    from that event to the flag stores, the host time of the whole step call, and the device time of the boundary and interior
    launches; then rank 0 steps the WHOLE mesh on its device (t1) so that bound_from_share = t1 / (largest per-rank launch time per
    step) says what the partition alone allows, before any exchange."""
    n = max(3, min(args.steps, 10))
    model.exchange_stats(True)
    sync_all()
    for _ in range(n):
        step()
    sync_all()
    mine = model.exchange_stats()
    model.exchange_stats(False)
    every = [None] * world
    dist.all_gather_object(every, mine, group=group)
    t1 = None
    if rank == 0:
        try:
            mesh, ssh, u, h, rest, cfg, sbytes = whole
            S1, D1, T1, P1 = mk.ocn_init_from_arrays(mesh, ssh, u, h, rest, cfg, backend, multilayer=True, ordering=args.ordering,
                                                     patch_cells=args.patch_cells, state_bytes=sbytes, placement_tries=1)
            one = lambda: mk.ocn_timestep(P1, D1, T1, S1, mk.RungeKutta4)  # noqa: E731
            _, ms1 = timed_steps(backend, one, 5, 3, backend.synchronize)
            t1 = step_stats(ms1)["median"]
            P1._state.close(); S1.mesh.close()
        except Exception as exc:             # noqa: BLE001
            log(f"[bench] single-device reference for the scaling bound failed: {exc!r}")
    sync_all()
    if rank != 0:
        return None
    share = [e["boundary_launch_ms_per_step"] + e["interior_launch_ms_per_step"] for e in every]
    out = {"steps_recorded": n,
           "host_wait_ms_per_step": [e["host_wait_ms_per_step"] for e in every],
           "host_signal_wait_ms_per_step": [e["host_signal_wait_ms_per_step"] for e in every],
           "push_to_flag_us": [e["push_to_flag_us"] for e in every],
           "host_step_ms_per_step": [e["host_step_ms_per_step"] for e in every],
           "boundary_launch_ms_per_step": [e["boundary_launch_ms_per_step"] for e in every],
           "interior_launch_ms_per_step": [e["interior_launch_ms_per_step"] for e in every],
           "rank_share_ms_per_step": share, "max_rank_share_ms": max(share),
           "t1_whole_mesh_on_rank0_ms": t1, "bound_from_share": (t1 / max(share)) if t1 and max(share) > 0 else None,
           "measured_speedup_vs_t1": (t1 / ms_per_step) if t1 else None,
           "note": "per rank (list index = rank); *_launch_ms = device time of the four boundary / interior stage launches of a step "
                   "(HIP events around each launch); host_wait = inside moka_halo_push_wait; host_signal_wait = waiting for the rank's own "
                   "push kernel; push_to_flag = from that event to the last flag store; bound_from_share = what the partition allows with a "
                   "free exchange; the direct transport only has the three host_* / push_* figures (buffered transports: zeros)"}
    return out


def placement_summary(rep):
    """What moka_state_optimize_placement did at set-up (rank 0's state): first_placement_ms = the four stage launches of an RK4
    step as moka_state_create placed the arrays (what a caller gets without the search), ms_after = with the kept layout, the
    per-array trials, and how close the kept layout is to the best timing any trial saw."""
    out = dict(rep)
    if rep.get("ms_before"):
        out["first_placement_ms"] = rep["ms_before"]
        out["kept_vs_first"] = rep["ms_after"] / rep["ms_before"]
        # every trial as a whole-step figure (a trial reports the launches its array takes part in): the layout before the trial
        # with those launches replaced by the trial's timing; the kept layout against the best of them
        cur, totals = rep["ms_before"], []
        for t in rep.get("trials", []):
            tot = cur - (t["ms_old"] - t["ms_new"])
            totals.append(tot)
            if t["kept"]:
                cur = tot
        out["trial_totals_ms"] = totals
        out["best_trial_ms"] = min(totals + [rep["ms_before"]])
        out["kept_vs_best_trial"] = rep["ms_after"] / out["best_trial_ms"]
    out["note"] = ("moka_state_optimize_placement (C ABI; what julia/MokaHIP.jl calls at binding): dt = 0 stage launches timed with the "
                   "library's events, one array re-allocated per trial, kept when the launches it takes part in got faster; "
                   "ms_* = sum of the four stage launches' medians (DESIGN section 5)")
    return out


def config5_leg(mk, backend, args, copy_gbs):
    """BASELINE config 5 inside the same run: RK4 ms/step (median), per stage, the tendency launch and
    the reference_compat Forward-Euler step on the 3 696 642-cell x 80-layer fp32-storage workload.  No CPU leg for it."""
    from moka_hip import meshgen as mg
    name = "config5_3.7M_x80_f32"
    m, K, sbytes, stretch = WORKLOADS[name]
    mesh = get_mesh(m, stretch)
    ssh, u, h, rest, dts = mg.sphere_synthetic_state(mesh, K)
    cfg = {"time_management": {"config_start_time": dt.datetime(1, 1, 1), "config_run_duration": dt.timedelta(hours=1)},
           "time_integration": {"config_dt": dt.timedelta(seconds=dts), "config_number_of_time_levels": 2}}
    t0 = time.time()
    placement = {}
    Setup, Diag, Tend, Prog = mk.ocn_init_from_arrays(mesh, ssh, u, h, rest, cfg, backend, multilayer=True,
                                                       state_bytes=sbytes, placement_tries=args.placement_tries, placement_report=placement)
    log(f"[bench] config 5 plan + upload: {time.time() - t0:.1f}s; placements tried: {placement}")
    info = Setup.mesh.info()
    step = lambda: mk.ocn_timestep(Prog, Diag, Tend, Setup, mk.RungeKutta4)  # noqa: E731
    steps, warmup = max(5, min(args.steps, 20)), max(2, min(args.warmup, 5))
    wall, ms = timed_steps(backend, step, steps, warmup, backend.synchronize)
    st = step_stats(ms)
    b_mesh, b_tend, b_step = algorithmic_bytes(mesh.nCells, mesh.nEdges, K, S=sbytes)
    stream_bytes = sbytes * K * (mesh.nEdges + mesh.nCells)
    per_stage, nst, ssum = stage_rooflines(backend, step, min(steps, 10), stream_bytes, b_mesh)
    out = {"workload": name, "mesh": f"icosahedral m={m}, Schmidt stretch {stretch}", "nCells": mesh.nCells, "nEdges": mesh.nEdges,
           "nVertLevels": K, "dtype": "f64 arithmetic on f32-stored state", "patch_cells": info.get("patch_cells"),
           "steps": steps, "warmup": warmup, "ms_per_step": st["median"], "step_ms": st,
           "ms_per_step_wall_mean": wall / steps * 1e3, "value": mesh.nCells * K / (st["median"] * 1e-3), "unit": "cell-updates/s",
           "roofline": {"bound": "hbm", "achieved": b_step / (st["median"] * 1e-3) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                        "frac": b_step / (st["median"] * 1e-3) / 1e9 / HBM_PEAK_GBS,
                        "frac_of_copy_this_run": b_step / (st["median"] * 1e-3) / 1e9 / copy_gbs if copy_gbs else None,
                        "formula": "contract: 18 state streams per step + 4 B_mesh, S = 4",
                        "per_stage": per_stage, "per_stage_steps": nst, "per_stage_sum_ms": ssum},
           "placement": placement_summary(placement),
           "cpu_baseline": None, "cpu_baseline_note": "skipped for this leg: the CPU baseline belongs to the headline (config 4) line"}
    try:     # PMC traffic of this workload's stage launches, taken by tools/profile.sh in separate passes (as for the headline line)
        rec = json.load(open(os.path.join(ROOT, "profiles", "pmc_traffic.json"))).get(name, {})
        if rec.get("config", {}).get("patch_cells") == info.get("patch_cells") and rec.get("stage_bytes_per_launch"):
            out["roofline"]["traffic"] = rec["stage_bytes_per_launch"]
            out["roofline"]["algorithmic_bytes_per_launch"] = b_step / 4
            out["roofline"]["traffic_source"] = {"file": "profiles/pmc_traffic.json", "profiled_at_commit": rec.get("commit")}
    except Exception:
        pass
    out.update(single_gpu_extras(mk, backend, Setup, Diag, Tend, Prog, K, sbytes, dts, b_tend, max(5, min(args.tend_iters, 10))))
    out["under_load"] = {"rk4_steps": under_load(backend, step, 1.0, 5),
                         "tendency_launches": under_load(backend, lambda: mk.computeTendency(Setup.mesh, Diag, Prog, Tend), 0.6, 10)}
    out["tendency"] = out["tendency_kernel"]
    backend.synchronize()
    Prog._state.close()
    Setup.mesh.close()
    return out


def dump_rows(nCells, nEdges, K):
    """Global ids of the rows --dump-outputs writes: every row when ssh, normalVelocity and layerThickness fit DUMP_BYTES as
    float64, else the same fraction of the cells and of the edges, drawn with DUMP_SEED (the same rows in every run)."""
    total = 8 * (nCells + K * (nEdges + nCells))
    if total <= DUMP_BYTES:
        return np.arange(nCells), np.arange(nEdges)
    frac = DUMP_BYTES * 15 / 16 / total
    rng = np.random.default_rng(DUMP_SEED)
    cells = np.sort(rng.choice(nCells, max(1, int(nCells * frac)), replace=False))
    edges = np.sort(rng.choice(nEdges, max(1, int(nEdges * frac)), replace=False))
    return cells, edges


def output_rows(Prog, cells, edges, lm=None):
    """name -> (positions in the id list, rows) of the current time level at the global ids `cells` / `edges`: every listed
    row, or with `lm` (the LocalMesh of a rank of a partitioned run) those the rank owns -- its halo rows are not final."""
    out = {}
    for name, field, ids, kind in (("ssh", Prog.ssh[-1], cells, "c"), ("normalVelocity", Prog.normalVelocity[-1], edges, "e"),
                                   ("layerThickness", Prog.layerThickness[-1], cells, "c")):
        pos, loc = np.arange(ids.size), ids
        if lm is not None:
            g2l, owned = (lm.g2l_c, lm.owned_cell_mask) if kind == "c" else (lm.g2l_e, lm.owned_edge_mask)
            loc = g2l[ids]
            keep = loc >= 0
            keep[keep] = owned[loc[keep]]
            pos, loc = pos[keep], loc[keep]
        out[name] = (pos, field.rows(loc) if loc.size else np.empty((0,) + field.shape[1:]))
    return out


def write_outputs(path, parts, cells, edges, K):
    """Assemble output_rows() of every rank (a list) and write DIR/<name>.npy, float64."""
    os.makedirs(path, exist_ok=True)
    shapes = {"ssh": (cells.size,), "normalVelocity": (edges.size, K), "layerThickness": (cells.size, K)}
    for name, shape in shapes.items():
        a = np.empty(shape, dtype=np.float64)
        seen = np.zeros(shape[0], dtype=bool)
        for p in parts:
            pos, rows = p[name]
            a[pos] = rows
            seen[pos] = True
        if not seen.all():
            raise RuntimeError(f"--dump-outputs: {int((~seen).sum())} rows of {name} are owned by no rank")
        np.save(os.path.join(path, name + ".npy"), a)
    log(f"[bench] outputs of the last timed step: {', '.join(shapes)} ({cells.size} cells, {edges.size} edges) in {path}")


def main():
    if "--rccl-probe" in sys.argv:
        rccl_probe_child(sys.argv[sys.argv.index("--rccl-probe") + 1] if len(sys.argv) > sys.argv.index("--rccl-probe") + 1 else "nccl")
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--workload", default="config4_1M_x60", choices=list(WORKLOADS))
    ap.add_argument("--variant", type=int, default=0, help="kernel variant (moka_set_kernel_variant): 0 auto, 11 default stage kernel, 4 column kernel, 3 generic index kernel")
    ap.add_argument("--patch-cells", type=int, default=0)
    ap.add_argument("--ordering", type=int, default=0)
    ap.add_argument("--full", action="store_true",
                    help="after the timed region, also everything the headline does not need: calibration, per-stage rooflines, "
                         "tendency / Forward-Euler / 13-stream entries, clocks under load, the config-5 leg and the CPU baselines "
                         "(N = 1), the exchange report (N > 1)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write ssh / normalVelocity / layerThickness as the last timed step left them to DIR/<name>.npy (float64; "
                         "a fixed seeded sample of rows where the whole state exceeds 64 MiB)")
    ap.add_argument("--no-cpu", action="store_true", help="--full: skip the CPU baseline leg")
    ap.add_argument("--no-config5", action="store_true", help="--full: skip the config-5 leg of the single-GPU run")
    ap.add_argument("--tend-iters", type=int, default=20, help="--full: launches of the tendency / Forward-Euler entries")
    ap.add_argument("--placement-tries", type=int, default=24,
                    help="upper limit of the per-array re-allocations moka_state_optimize_placement tries at set-up (the library's own "
                         "search, behind the C ABI: one array at a time gets a second allocation, the faster is kept; where the "
                         "allocator puts the arrays decides 5-14 %% of every launch, DESIGN section 5); <= 1 = take what comes")
    ap.add_argument("--tuning", action="append", default=[], metavar="KEY=VALUE",
                    help="A/B measurement: moka_set_tuning(KEY, VALUE) before anything runs (include/moka_hip.h lists the keys); repeatable")
    ap.add_argument("--f32-wide-modes", type=int, default=None,
                    help="A/B measurement: bit mask of the fp32-storage kernel's modes launched as 512-thread / 4-waves-per-SIMD workgroups (moka_set_tuning key 1)")
    ap.add_argument("--transport", default="auto", choices=["auto", "ipc", "nccl", "nccl-a2a", "nccl-p2p", "nccl-default-stream", "gloo"],
                    help="halo transport for N > 1: auto = the fastest of those that qualify on this node -- ipc (direct stores "
                         "into the neighbours' IPC-mapped fields over xGMI) and the RCCL forms (nccl-a2a, nccl-p2p); nccl = the RCCL "
                         "forms only; gloo = host-staged (rehearsal on one GPU)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        log(f"[bench] WORLD_SIZE={world} but --gpus {args.gpus}: launch with torch.distributed.run --nproc-per-node {args.gpus}")
        if world == 1 and args.gpus > 1:
            sys.exit(2)

    import torch
    import moka_hip as mk
    from moka_hip import meshgen as mg

    ndev = max(torch.cuda.device_count(), 1)            # counting devices does not initialise the GPU
    device_index = local_rank % ndev            # rehearsals may put several ranks on one GPU (ipc and gloo transports)
    gloo_group = None
    rccl_ok = False
    dist = None
    if world > 1:
        import torch.distributed as dist
        want_rccl = args.transport in ("auto", "nccl", "nccl-a2a", "nccl-p2p", "nccl-default-stream")
        if want_rccl and ndev >= world:
            rccl_ok = probe_rccl()               # in a child process, before this one touches the GPU
        torch.cuda.set_device(device_index)
        if rccl_ok:
            try:
                dist.init_process_group("nccl", device_id=torch.device("cuda", device_index),
                                        timeout=dt.timedelta(seconds=300))
                gloo_group = dist.new_group(backend="gloo")     # control messages + last-resort halo transport
            except Exception as exc:                 # noqa: BLE001
                log(f"[bench] rank {rank}: RCCL process group unavailable ({str(exc).splitlines()[0]})")
                rccl_ok = False
                try:
                    dist.destroy_process_group()
                except Exception:                    # noqa: BLE001
                    pass
        if not rccl_ok:
            dist.init_process_group("gloo")
            if args.transport not in ("auto", "ipc", "gloo"):
                log(f"[bench] rank {rank}: RCCL is not usable here; --transport {args.transport} falls back to auto (ipc, gloo)")
                args.transport = "auto"
        # every rank must have reached the same verdict about RCCL
        t = torch.tensor([1.0 if rccl_ok else 0.0])
        dist.all_reduce(t, op=dist.ReduceOp.MIN, group=gloo_group)
        if rccl_ok and float(t[0]) != 1.0:
            log(f"[bench] rank {rank}: another rank has no RCCL: this launch cannot continue consistently")
            sys.exit(5)
    m, K, sbytes, stretch = (tuple(WORKLOADS[args.workload]) + (8, 1.0))[:4]
    mesh = get_mesh(m, stretch)
    ssh, u, h, rest, dts = mg.sphere_synthetic_state(mesh, K)
    cfg = {"time_management": {"config_start_time": dt.datetime(1, 1, 1), "config_run_duration": dt.timedelta(hours=1)},
           "time_integration": {"config_dt": dt.timedelta(seconds=dts), "config_number_of_time_levels": 2}}

    backend = mk.MokaHIP(device_index)
    if args.variant:
        backend.set_kernel_variant(args.variant)
    if args.f32_wide_modes is not None:
        from moka_hip import lib as _L
        _L.check(_L.lib().moka_set_tuning(1, int(args.f32_wide_modes)))
    for kv in args.tuning:
        from moka_hip import lib as _L
        k_, v_ = kv.split("=")
        _L.check(_L.lib().moka_set_tuning(int(k_), int(v_)))

    # which physical devices do the ranks of this launch really use?  (host, PCI bus id) per rank
    my_dev = (socket.gethostname(), backend.pci_bus_id())
    devs = [my_dev]
    if world > 1:
        devs = [None] * world
        dist.all_gather_object(devs, my_dev, group=gloo_group)
    n_distinct = len(set(devs))
    ranks_per_device = max(devs.count(d) for d in set(devs))
    rehearsal = n_distinct < world
    if rehearsal:
        log(f"[bench] rank {rank}: {world} ranks on {n_distinct} distinct device(s): this line is a REHEARSAL, not an {world}-GPU result")

    # ---- same-run calibration, before: in front of the set-up (plan, upload, the library's placement search), which in turn sits
    # right in front of the warm-up.  (Rounds 3 / 4a probed between set-up and warm-up: two seconds of a 600 W copy load let the
    # package leave the state the stage launches run in -- 1400 W, shader clock 2.1-2.2 GHz -- and the first 100-200 ms of
    # launches behind such a pause run 1-2 % slower than the steady state; W = 5 warm-up steps are 35 ms.  The probes measure the
    # box, not the model: they lose nothing by coming first, and the timed region then starts from the state a running model is in.)
    # --full only: the headline does not need them.
    cal_before = calibrate(backend, "before") if args.full else None
    transport_trials = {}
    model = None
    if world > 1:
        from moka_hip import parallel as mp
        t0 = time.time()
        model = mp.DistributedModel(mesh, ssh, u, h, rest, dts, backend, rank, world, ordering=args.ordering,
                                    patch_cells=args.patch_cells, transport="gloo", group=gloo_group,
                                    state_bytes=sbytes, placement_tries=args.placement_tries)
        placement = model.placement
        log(f"[bench] rank {rank}: partition + local plan + upload: {time.time() - t0:.1f}s  {model.info()}")
        # Choose the halo transport on this node.  Every candidate must, on every rank, (1) set up, (2) deliver exactly the
        # bytes the host-staged gloo exchange delivers for the same state, (3) run steps whose owned state equals the same
        # steps over gloo bit for bit; the ranks agree after each phase over the gloo group so nobody is left waiting in a
        # collective.  The fastest qualifying candidate is kept.
        rccl_forms = ("nccl-a2a", "nccl") if rccl_ok else ()
        cands = {"auto": ("ipc",) + rccl_forms, "nccl": rccl_forms, "ipc": ("ipc",), "nccl-a2a": rccl_forms[:1],
                 "nccl-p2p": rccl_forms[1:], "nccl-default-stream": (), "gloo": ()}[args.transport]
        fallbacks = (("nccl-default-stream",) if rccl_ok else ()) + ("gloo",)
        model.set_transport("gloo")
        model.exchange_state()
        cand, times = mp.choose_transport(model, cands, fallbacks, gloo_group, lambda msg: log(f"[bench] rank {rank}: {msg}"))
        model.set_transport(cand)
        # the trials advanced the state: start the timed run from the initial state again
        model.reset_state(ssh, u, h)
        args.transport = {"nccl": "nccl-p2p"}.get(cand, cand)
        transport_trials = times
        step = model.step_rk4
        info = model.info()
    else:
        t0 = time.time()
        placement = {}
        Setup, Diag, Tend, Prog = mk.ocn_init_from_arrays(mesh, ssh, u, h, rest, cfg, backend, multilayer=True,
                                                           ordering=args.ordering, patch_cells=args.patch_cells,
                                                           state_bytes=sbytes, placement_tries=args.placement_tries,
                                                           placement_report=placement)
        log(f"[bench] plan + upload: {time.time() - t0:.1f}s; placements tried: {placement}")
        info = Setup.mesh.info()
        step = lambda: mk.ocn_timestep(Prog, Diag, Tend, Setup, mk.RungeKutta4)  # noqa: E731

    def sync_all():
        backend.synchronize(); torch.cuda.synchronize()
        if world > 1:
            dist.barrier(group=gloo_group)

    wall, step_ms = timed_steps(backend, step, args.steps, args.warmup, sync_all)
    if args.dump_outputs:
        # what the last timed step left, before anything else steps the state on
        cells, edges = dump_rows(mesh.nCells, mesh.nEdges, K)
        mine = output_rows(model.Prog, cells, edges, model.lm) if world > 1 else output_rows(Prog, cells, edges)
        parts = [mine]
        if world > 1:
            parts = [None] * world
            dist.all_gather_object(parts, mine, group=gloo_group)
        if rank == 0:
            write_outputs(args.dump_outputs, parts, cells, edges, K)
        del mine, parts
    # ---- ... and after: right behind the timed region ----
    cal_after = calibrate(backend, "after") if args.full else None
    if world > 1:
        # per step: the slowest rank's time (the step is over when the last rank is done); wall: max over ranks
        tt = torch.tensor(step_ms + [wall], dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX, group=gloo_group)
        step_ms, wall = [float(x) for x in tt[:-1]], float(tt[-1])
        if args.full:
            cc = torch.tensor([cal_before["copy_GBs"], cal_after["copy_GBs"], cal_before["read_GBs"]], dtype=torch.float64)
            dist.all_reduce(cc, op=dist.ReduceOp.MIN, group=gloo_group)
            copy_min_over_ranks = [float(x) for x in cc]
    st = step_stats(step_ms)
    ms_per_step = st["median"]
    value = mesh.nCells * K / (ms_per_step * 1e-3)
    copy_this_run = 0.5 * (cal_before["copy_GBs"] + cal_after["copy_GBs"]) if args.full else None

    b_mesh, b_tend, b_step = algorithmic_bytes(mesh.nCells, mesh.nEdges, K, S=sbytes)
    stream_bytes = sbytes * K * (mesh.nEdges + mesh.nCells)
    # dominant kernel = the fused RK-stage kernel (k_stage_rec2c): 4 launches per step, back to back on the compute stream
    # (nothing else runs there), so the average launch duration over the timed region is (sum of the step times) / (4 K);
    # algorithmic bytes per launch = B_step / 4 (contract formula).
    launches = 4 * len(step_ms)
    avg_launch_ms = sum(step_ms) / launches                   # the contract's figure: the AVERAGE launch (strays included)
    per_rank_bytes = b_step / 4 / world
    achieved = per_rank_bytes / (avg_launch_ms * 1e-3) / 1e9
    # the same with the bytes the four launches really have to move (stage 1 aliases Provis = Curr = New): 16 streams
    min_step_bytes = (sum(STAGE_MIN_STREAMS) * stream_bytes + 4 * b_mesh) / world
    achieved_min = min_step_bytes / 4 / (avg_launch_ms * 1e-3) / 1e9
    # HBM traffic per launch from PMC counters: measured by tools/profile.sh in separate rocprofv3 passes (a process cannot
    # read them about itself), so it is quoted only when that profile was taken with THIS configuration, with its source
    traffic, traffic_source = None, None
    tfile = os.path.join(ROOT, "profiles", "pmc_traffic.json")
    if os.path.exists(tfile) and world == 1:
        try:
            rec = json.load(open(tfile)).get(args.workload, {})
            same = all(rec.get("config", {}).get(k) == v for k, v in
                       (("patch_cells", info.get("patch_cells")), ("ordering", info.get("ordering")),
                        ("kernel_variant", args.variant)))
            if same and rec.get("stage_bytes_per_launch"):
                traffic = rec["stage_bytes_per_launch"]
                traffic_source = {"file": "profiles/pmc_traffic.json", "profiled_at_commit": rec.get("commit"),
                                  "note": "FETCH_SIZE x2 (gfx950 rule) + WRITE_SIZE, separate --pmc passes; not measured in this run"}
        except Exception:
            traffic = None
    roofline = {"bound": "hbm", "kernel": "k_stage_rec2c (fused TRiSK tendency + RK4 stage update), mean of the 4 launches of a step",
                "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS,
                **({"frac_of_copy_this_run": achieved / copy_this_run, "copy_GBs_this_run": copy_this_run} if args.full else {}),
                "frac_of_guide_copy_ceiling": achieved / HBM_COPY_GBS, "traffic": traffic, "traffic_source": traffic_source,
                "algorithmic_bytes_per_launch": per_rank_bytes, "avg_launch_ms": avg_launch_ms,
                "stray_steps": st["strays"], "frac_at_median_step": per_rank_bytes / (ms_per_step / 4 * 1e-3) / 1e9 / HBM_PEAK_GBS,
                "launches_timed": launches, "formula": "contract: 18 state streams per step (5, 5, 5, 3) + 4 B_mesh",
                "frac_kernel_minimum_bytes": achieved_min / HBM_PEAK_GBS,
                **({"frac_kernel_minimum_bytes_of_copy_this_run": achieved_min / copy_this_run} if args.full else {}),
                "kernel_minimum_note": "16 state streams per step (3, 5, 5, 3): stage 1 aliases Provis = Curr = New"}
    if world == 1 and args.full:
        per_stage, nst, ssum = stage_rooflines(backend, step, max(5, min(args.steps, 20)), stream_bytes, b_mesh)
        roofline["per_stage"] = per_stage
        roofline["per_stage_steps"] = nst
        roofline["per_stage_sum_ms"] = ssum

    calibration = None
    if args.full:
        calibration = {"copy_GBs_before": cal_before["copy_GBs"], "copy_GBs_after": cal_after["copy_GBs"],
                       "copy_GBs_mean_before": cal_before["copy_GBs_mean"], "copy_GBs_mean_after": cal_after["copy_GBs_mean"],
                       "read_GBs": cal_before["read_GBs"], "read_GBs_after": cal_after["read_GBs"],
                       "gather_GBs_before": cal_before["gather_GBs"], "gather_GBs_after": cal_after["gather_GBs"],
                       "streams5_GBs_before": cal_before.get("streams5_GBs"), "streams5_GBs_after": cal_after.get("streams5_GBs"),
                       "reread128_GBs_before": cal_before.get("reread128_GBs"), "reread128_GBs_after": cal_after.get("reread128_GBs"),
                       "gather32G_GBs_before": cal_before.get("gather32G_GBs"), "gather32G_GBs_after": cal_after.get("gather32G_GBs"),
                       "probe": f"{PROBE_BYTES >> 30} GiB footprint (half source, half destination), 16 bytes per lane, best of 5 launches, "
                                "HIP events on the compute stream; before = in front of the set-up (plan, upload, placement search; the warm-up follows that directly), after = behind the timed region; "
                                "copy = one word per thread (bytes read + written), read = read-only sweep with nontemporal loads, "
                                "gather = 480-byte rows in a scattered order, a half-wave per row (the stage kernels' pattern), "
                                "streams5 = three streams read and two written at once (the mix of the RK stage launches), "
                                "reread128 = a 128 MiB region read 16 times back to back (what comes back from the Infinity Cache: the stage "
                                "kernels fetch a fifth of their bytes a second time), gather32G = the row gather over a 32 GiB footprint of its "
                                "own, a quarter of the rows (address translation for a state-sized span)",
                       "guide_copy_ceiling_GBs": HBM_COPY_GBS,
                       "ms_per_step_at_guide_ceiling": ms_per_step * copy_this_run / HBM_COPY_GBS,
                       "clocks_power_before": cal_before["sysfs"], "clocks_power_after": cal_after["sysfs"]}
        if world > 1:
            calibration["min_over_ranks"] = {"copy_GBs_before": copy_min_over_ranks[0], "copy_GBs_after": copy_min_over_ranks[1],
                                             "read_GBs": copy_min_over_ranks[2]}

    out = {"metric": "cell-updates/sec per RK4 step", "value": value, "unit": "cell-updates/s",
           "n_gpus": n_distinct, "ranks": world, "n_devices_visible": ndev, "ranks_per_device": ranks_per_device,
           "rehearsal": rehearsal,
           "steps": args.steps, "warmup": args.warmup, "ms_per_step": ms_per_step,
           "step_ms": st, "ms_per_step_wall_mean": wall / args.steps * 1e3,
           "value_wall_mean": mesh.nCells * K / (wall / args.steps),
           "value_note": "value and ms_per_step = median of the per-step times (HIP events, max over ranks per step; SURVEY 8d); "
                         "the *_wall_mean fields = the barrier-bracketed wall region / K",
           "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
           "dtype": "f64" if sbytes == 8 else "f64 arithmetic on f32-stored state", "data": "synthetic",
           "config": {"workload": args.workload,
                      "mesh": f"icosahedral m={m}" + (f", Schmidt stretch {stretch}" if stretch != 1.0 else ""), "nCells": mesh.nCells,
                      "nEdges": mesh.nEdges, "nVertLevels": K, "integrator": "RK4", "dt_s": dts,
                      "ordering": info.get("ordering"), "patch_cells": info.get("patch_cells"),
                      "kernel_variant": args.variant,
                      "parallelism": "single GPU" if world == 1 else
                      f"mesh partitioned over {world} ranks on {n_distinct} distinct GPU(s) (RCB), 1-deep halo exchanged per RK stage over "
                      f"{args.transport}, overlapped with the interior patches; halo {info.get('halo_bytes_per_stage', 0) / 1e6:.1f} MB/stage/rank"
                      + (" -- REHEARSAL: ranks share a device" if rehearsal else ""),
                      **({"halo_transport": args.transport, "halo_transport_trials_ms_per_step": transport_trials,
                          "rccl_usable": rccl_ok} if world > 1 else {})},
           "roofline": roofline, **({"calibration": calibration} if args.full else {}),
           "placement": placement_summary(placement)}

    # Everything from here on is an appendix of the line assembled above (--full only): none of it may cost the line itself.
    # (Exception: exchange_report runs collectives -- a rank that failed alone would leave the others waiting, so it is not caught.)
    def appendix(key, fn):
        try:
            return fn()
        except Exception as exc:                 # noqa: BLE001
            log(f"[bench] {key} failed: {exc!r}")
            return {"error": f"{type(exc).__name__}: {exc}"}

    if world > 1 and args.full:
        out["exchange"] = exchange_report(mk, backend, model, step, sync_all, dist, gloo_group, rank, world, args,
                                          (mesh, ssh, u, h, rest, cfg, sbytes), ms_per_step)
    if world == 1 and args.full:
        ex = appendix("tendency / Forward-Euler entries", lambda: single_gpu_extras(mk, backend, Setup, Diag, Tend, Prog, K, sbytes, dts, b_tend, args.tend_iters))
        out.update(ex if "error" not in ex else {"tendency_kernel": ex, "forward_euler_compat": ex})
        if sbytes == 8:
            try:
                out["rk4_13_streams"] = rk4_13_stream_entry(mk, backend, step, args.steps, args.warmup, mesh.nCells * K, stream_bytes, b_mesh, b_step)
            except Exception as exc:             # noqa: BLE001
                out["rk4_13_streams"] = {"error": f"{type(exc).__name__}: {exc}"}
        # clock and power while the launches run (after every timed region of this workload)
        out["under_load"] = appendix("under_load", lambda: {
            "rk4_steps": under_load(backend, step, 1.0, 10),
            "tendency_launches": under_load(backend, lambda: mk.computeTendency(Setup.mesh, Diag, Prog, Tend), 0.6, 20),
            "right_after": device_sysfs(backend.pci_bus_id()),     # (the sensors still average over the launches)
            "note": "sysfs (pp_dpm_sclk, power1_average) sampled every 4 ms while the launches run back to back; the stage "
                    "launches run the package at its power limit (1400 W) and the shader clock drops below the 2.4 GHz it "
                    "shows when idle: the launches are bound by energy per step (profiles/r04_variants.txt section 4)"})
        if args.workload == "config4_1M_x60" and not args.no_config5:
            # free the headline workload's device objects, then time config 5 on the same device in the same run
            backend.synchronize()
            Prog._state.close()
            Setup.mesh.close()
            try:
                out["config5"] = config5_leg(mk, backend, args, copy_this_run)
            except Exception as exc:                 # noqa: BLE001  (the headline line must not be lost to its appendix)
                out["config5"] = {"error": f"{type(exc).__name__}: {exc}"}
                log(f"[bench] config 5 leg failed: {exc!r}")
            cal_end = calibrate(backend, "end of run")
            calibration["copy_GBs_end_of_run"] = cal_end["copy_GBs"]
            calibration["clocks_power_end_of_run"] = cal_end["sysfs"]
    if args.full:
        backend.bw_probe(0)
    if rank == 0 and world == 1 and args.full and not args.no_cpu:       # the CPU leg belongs to the N = 1 line only
        t0 = time.time()
        mixed = sbytes == 4
        if mesh.nCells * K > 1.5e8:        # bounded sample: the same workload family on a quarter of the cells
            cm = get_mesh(m // 2, stretch)
            cmesh = (cm, K) + tuple(mg.sphere_synthetic_state(cm, K))
        else:
            cmesh = (mesh, K, ssh, u, h, rest, dts)
        out["cpu_baseline"] = appendix("cpu_baseline", lambda: cpu_baseline(*cmesh, mixed=mixed))
        out["cpu_baseline_1t"] = appendix("cpu_baseline_1t", lambda: cpu_baseline_1t(*cmesh, mixed=mixed))
        out["cpu_baseline"]["host"] = _cpu_model()
        log(f"[bench] cpu baseline legs: {time.time() - t0:.1f}s")
    if rank == 0:
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.barrier(group=gloo_group)
        model.close()
        dist.destroy_process_group()


def _cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return f"{line.split(':', 1)[1].strip()} x{os.cpu_count()}"
    except Exception:
        pass
    return f"unknown x{os.cpu_count()}"


if __name__ == "__main__":
    main()
