"""bench.py host-side contract: the algorithmic-bytes formula is SURVEY.md section 8(d)'s, sizes are BASELINE's."""
import importlib.util
import os
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
bench = importlib.util.module_from_spec(spec)
spec.loader.exec_module(bench)


def test_algorithmic_bytes_match_survey_numbers():
    nC, nE, K = 1024002, 3072000, 60                      # config 4 (SURVEY section 8 size table)
    b_mesh, b_tend, b_step = bench.algorithmic_bytes(nC, nE, K)
    assert abs(b_mesh / 1e9 - 0.56) < 0.01                # "B_mesh = 0.56 GB"
    assert abs(b_tend / 1e9 - 4.49) < 0.01                # "B_tend = 3.93 + 0.56 = 4.49 GB"
    assert abs(b_step / 1e9 - 37.6) < 0.1                 # "B_step = 37.6 GB"
    assert b_tend == 2 * 8 * K * (nE + nC) + b_mesh and b_step == 18 * 8 * K * (nE + nC) + 4 * b_mesh


def test_default_workload_is_config4():
    m, K = bench.WORKLOADS["config4_1M_x60"]
    assert 10 * m * m + 2 == 1024002 and K == 60
    assert bench.HBM_PEAK_GBS == 8000.0


def test_rccl_probe_rendezvous_in_child_processes():
    """bench.py asks a CHILD process per rank whether RCCL works (a wedged collective hangs rather than raises).  The
    children rendezvous on their own port, outside the launcher's agent store.  Run that logic under torch.distributed.run
    with the probe's exchange on gloo / CPU tensors: two ranks, both must report success."""
    import subprocess
    import sys
    import socket
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    code = ("import importlib.util, os, sys; spec = importlib.util.spec_from_file_location('bench', %r); "
            "b = importlib.util.module_from_spec(spec); spec.loader.exec_module(b); "
            "ok = b.probe_rccl(timeout_s=90, backend='gloo'); print('PROBE', os.environ['RANK'], ok); sys.exit(0 if ok else 1)"
            % os.path.join(ROOT, "bench.py"))
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
                        "--master-port", str(port), "--no-python", sys.executable, "-c", code],
                       capture_output=True, text=True, timeout=240, env=dict(os.environ, OMP_NUM_THREADS="1"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "PROBE 0 True" in r.stdout and "PROBE 1 True" in r.stdout


def test_sysfs_and_statistics_helpers(tmp_path):
    """The plain-file readers of the calibration record (no GPU involved) and the per-step statistics."""
    assert bench._dpm_current("0: 500Mhz\n1: 2394Mhz *\n2: 2400Mhz\n") == 2394.0
    assert bench._dpm_current("S: 94Mhz *\n0: 500Mhz\n1: 2400Mhz") == 94.0
    assert bench._dpm_current("0: 2000Mhz *") == 2000.0
    assert bench._dpm_current(None) is None and bench._dpm_current("garbage") is None
    hw = tmp_path / "hwmon" / "hwmon3"
    hw.mkdir(parents=True)
    (hw / "power1_input").write_text("554000000\n")
    assert bench._power_watts(str(tmp_path)) == 554.0
    assert bench._power_watts(str(tmp_path / "nothing")) is None
    d = bench.device_sysfs("ffff:ff:1f.7")                # not a device of this machine: reported, not raised
    assert d["pci_bus_id"] == "ffff:ff:1f.7" and "note" in d
    st = bench.step_stats([7.0, 6.8, 6.9, 9.5, 6.85])
    assert st["median"] == 6.9 and st["min"] == 6.8 and st["max"] == 9.5 and st["n"] == 5
    assert abs(st["mean"] - 7.41) < 1e-12


def test_dump_rows_fit_the_budget_and_are_the_same_every_run():
    """--dump-outputs: every row of a small state; a seeded sample of a large one, within 64 MiB, identical from run to run."""
    nC, nE = 10242, 30720
    cells, edges = bench.dump_rows(nC, nE, 60)
    assert np.array_equal(cells, np.arange(nC)) and np.array_equal(edges, np.arange(nE))
    for nC, nE, K in ((1024002, 3072000, 60), (3696642, 11089920, 80)):
        cells, edges = bench.dump_rows(nC, nE, K)
        assert 8 * (cells.size + K * (cells.size + edges.size)) <= bench.DUMP_BYTES
        assert cells.size > 1000 and edges.size > 1000
        assert np.all(np.diff(cells) > 0) and np.all(np.diff(edges) > 0) and cells[-1] < nC and edges[-1] < nE
        c2, e2 = bench.dump_rows(nC, nE, K)
        assert np.array_equal(cells, c2) and np.array_equal(edges, e2)


def test_dumped_rows_of_a_partitioned_run_assemble_to_the_whole(tmp_path):
    """Each rank reports the listed rows it owns; assembled on rank 0 they are the global arrays, every row exactly once."""
    from moka_hip import meshgen as mg
    from moka_hip import parallel as mp
    mesh, K, world = mg.icosahedral_mesh(6), 3, 3
    rng = np.random.default_rng(5)
    glob = {"ssh": rng.random(mesh.nCells), "normalVelocity": rng.random((mesh.nEdges, K)), "layerThickness": rng.random((mesh.nCells, K))}

    class Field:
        def __init__(self, a, g):
            self.a, self.g, self.shape = a, g, (g.size,) + a.shape[1:]

        def rows(self, ids):
            return self.a[self.g[ids]]

    part = mp.partition_cells(mesh, world)
    cells, edges = np.arange(0, mesh.nCells, 3), np.arange(1, mesh.nEdges, 2)
    parts = []
    for r in range(world):
        lm = mp.build_local(mesh, part, r, world)
        P = types.SimpleNamespace(ssh=[None, Field(glob["ssh"], lm.cells_g)],
                                  normalVelocity=[None, Field(glob["normalVelocity"], lm.edges_g)],
                                  layerThickness=[None, Field(glob["layerThickness"], lm.cells_g)])
        parts.append(bench.output_rows(P, cells, edges, lm))
    for name, ids in (("ssh", cells), ("normalVelocity", edges), ("layerThickness", cells)):
        assert sum(p[name][0].size for p in parts) == ids.size, name
    bench.write_outputs(str(tmp_path / "out"), parts, cells, edges, K)
    for name, ids in (("ssh", cells), ("normalVelocity", edges), ("layerThickness", cells)):
        got = np.load(tmp_path / "out" / f"{name}.npy")
        assert got.dtype == np.float64 and np.array_equal(got, glob[name][ids]), name


def _oracle_after(m, K, nsteps, clock_dt=True):
    """The single-domain oracle's state after `nsteps` RK4 steps of bench.py's synthetic workload on the m-sphere.
    clock_dt: dt as the one-rank model's clock holds it (microsecond resolution); the partitioned model steps with dt as given."""
    import datetime as dt
    import oracle as orc
    from moka_hip import meshgen as mg
    mesh = mg.icosahedral_mesh(m)
    ssh, u, h, rest, dts = mg.sphere_synthetic_state(mesh, K)
    if clock_dt:
        dts = dt.timedelta(seconds=dts).total_seconds()
    st = orc.OracleState(orc.OracleMesh(mesh, K, resting_thickness_sum=rest.sum(1), max_level_edge_top=K), ssh, u, h)
    for _ in range(nsteps):
        st.step_rk4(dts)
    return {"ssh": st.ssh[1], "normalVelocity": st.u[1], "layerThickness": st.h[1]}


def _check_outputs(path, expected):
    total = 0
    for name, exp in expected.items():
        got = np.load(os.path.join(path, f"{name}.npy"))
        total += got.nbytes
        assert got.dtype == np.float64 and np.array_equal(got, exp), name
    assert total <= bench.DUMP_BYTES


def _run_bench(args, nproc=1, timeout=420):
    """bench.py as the driver launches it (a child process; torch.distributed.run for N > 1): the JSON line it prints."""
    import json
    import socket
    import subprocess
    if nproc == 1:
        cmd = [sys.executable, os.path.join(ROOT, "bench.py")] + args
    else:
        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}", "--master-addr", "127.0.0.1",
               "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", str(nproc)] + args
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]            # ONE JSON line, from rank 0
    return json.loads(lines[0])


@pytest.mark.gpu
def test_bench_plain_run_is_the_headline_and_dumps_what_the_timed_steps_computed(tmp_path):
    """A plain run (no --full): the headline line, exactly --steps timed steps, none of the appendices; --dump-outputs holds
    the state after the warm-up and timed steps, bit for bit the oracle's."""
    b = _run_bench(["--workload", "small_10k_x60", "--steps", "3", "--warmup", "2", "--dump-outputs", str(tmp_path / "out")])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "n_gpus", "steps", "warmup", "config", "roofline"):
        assert k in b, k
    assert b["steps"] == 3 and b["step_ms"]["n"] == 3 and b["ms_per_step"] == b["step_ms"]["median"] > 0
    assert b["metric"] == "cell-updates/sec per RK4 step" and b["unit"] == "cell-updates/s" and b["dtype"] == "f64"
    for k in ("calibration", "cpu_baseline", "tendency_kernel", "forward_euler_compat", "rk4_13_streams", "under_load", "config5"):
        assert k not in b, k
    assert "per_stage" not in b["roofline"]
    _check_outputs(tmp_path / "out", _oracle_after(32, 60, 2 + 3))


@pytest.mark.gpu
def test_bench_line_on_one_gpu_small_workload():
    """The driver's contract on a small workload with --full: one JSON line with the metric, the roofline (with its calibration)
    and the CPU baseline; value = cells x layers / median step time."""
    b = _run_bench(["--workload", "small_10k_x60", "--steps", "6", "--warmup", "2", "--no-config5", "--tend-iters", "3", "--full"])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline", "cpu_baseline", "calibration", "step_ms"):
        assert k in b, k
    assert b["n_gpus"] == 1 and b["ranks"] == 1 and b["rehearsal"] is False and b["steps"] == 6 and b["dtype"] == "f64"
    assert b["config"]["workload"] == "small_10k_x60" and b["vs_baseline"] is None and b["higher_is_better"] is True
    nC, K = b["config"]["nCells"], b["config"]["nVertLevels"]
    assert abs(b["value"] - nC * K / (b["step_ms"]["median"] * 1e-3)) <= 1e-6 * b["value"]
    r = b["roofline"]
    assert r["bound"] == "hbm" and r["peak"] == 8000.0 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-12
    assert b["calibration"]["copy_GBs_before"] > 1000 and b["calibration"]["streams5_GBs_before"] > 1000
    assert b["cpu_baseline"]["kind"] == "port" and b["cpu_baseline"]["cores"] >= 1 and b["cpu_baseline"]["value"] > 0
    # round 4: medians everywhere a single stray launch could move a mean, and the line says how many strays there were
    assert b["step_ms"]["strays"] >= 0 and r["stray_steps"] == b["step_ms"]["strays"] and r["frac_at_median_step"] > 0
    t = b["tendency_kernel"]
    assert t["avg_launch_ms"] == t["launch_ms"]["median"] and t["launch_ms"]["n"] == 3 and t["launch_ms"]["min"] <= t["avg_launch_ms"] <= t["launch_ms"]["max"]
    for k in ("under_load", "placement", "rk4_13_streams", "forward_euler_compat"):
        assert k in b, k
    assert b["forward_euler_compat"]["arrays_pending_after_a_step"] == 1 and b["rk4_13_streams"]["ms_per_step"] > 0


@pytest.mark.gpu
def test_bench_two_ranks_on_one_gpu_is_labelled_a_rehearsal(tmp_path):
    """bench.py --gpus 2 --full the way the driver starts it, with both ranks on the one GPU of this box: the transport selection
    must qualify a transport (bitwise against the host-staged exchange), and the line must say what it is -- one distinct device,
    two ranks, a rehearsal -- instead of claiming two GPUs.  The outputs both ranks own assemble to the oracle's state."""
    b = _run_bench(["--workload", "small_10k_x60", "--steps", "4", "--warmup", "2", "--full", "--dump-outputs", str(tmp_path / "out")],
                   nproc=2)
    _check_outputs(tmp_path / "out", _oracle_after(32, 60, 2 + 4, clock_dt=False))
    assert b["ranks"] == 2 and b["n_gpus"] == 1 and b["n_devices_visible"] == 1 and b["ranks_per_device"] == 2 and b["rehearsal"] is True
    assert b["scaling"] == "strong" and b["config"]["halo_transport"] in ("ipc", "ipc-acq", "gloo", "nccl-a2a", "nccl-p2p")
    assert b["config"]["halo_transport"] in b["config"]["halo_transport_trials_ms_per_step"]
    assert b["value"] > 0 and "REHEARSAL" in b["config"]["parallelism"]
    # the line says where the time of a distributed step goes: per rank, from the library's own statistics
    ex = b["exchange"]
    for k in ("host_wait_ms_per_step", "host_signal_wait_ms_per_step", "push_to_flag_us", "host_step_ms_per_step",
              "boundary_launch_ms_per_step", "interior_launch_ms_per_step", "rank_share_ms_per_step"):
        assert len(ex[k]) == 2 and all(v >= 0.0 for v in ex[k]), k
    assert all(v > 0.0 for v in ex["interior_launch_ms_per_step"]) and ex["max_rank_share_ms"] == max(ex["rank_share_ms_per_step"])
    # (two ranks on ONE device: each rank's launches wait for the other's, so the bound itself means nothing here -- it is there)
    assert ex["t1_whole_mesh_on_rank0_ms"] > 0 and ex["bound_from_share"] > 0 and ex["measured_speedup_vs_t1"] > 0
    if b["config"]["halo_transport"].startswith("ipc"):
        assert all(v > 0.0 for v in ex["host_step_ms_per_step"])
