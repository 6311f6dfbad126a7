"""The index bookkeeping of the vertical momentum pass's tile forms (csrc/mvmix_index.hpp: tile spans, mv_slot, the LDS size at three and
four column sets) compiled for the host and walked by the stand-alone program tools/mvmix_index_check.cpp under the host sanitizers
(address, undefined).  No GPU, nothing loaded into this process: the program has its own main and runs as a child."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tile_index_arithmetic_under_the_host_sanitizers(tmp_path):
    exe = str(tmp_path / "mvmix_index_check")
    subprocess.check_call(["c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "mpas-ocean.jl_amd", "csrc"), os.path.join(ROOT, "tools", "mvmix_index_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "no finding" in out.stdout
