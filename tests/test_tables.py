"""What a context keeps resident on a device (csrc/rtgr_host.hpp: Resident<T>; csrc/rtgr_tables.hip): the bookkeeping of the tables named by an
id, without a device.  The lifetime of the tables on a device — load, unload, capture, replay, trim — is held by tests/test_grid_metric.py,
test_grid_metric_4d.py, test_textures.py and test_gpu_context.py."""
import os
import subprocess

from conftest import ROOT

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_resident_tables_bookkeeping(tmp_path):
    """Resident<GridTable> and Resident<TextureTable>: published ids are found and unknown ones are not; retire(id) moves exactly that
    entry and reports whether there was one; retire(0) is "all" (true even on an empty set) with zero_means_all — the texture rule — and
    "no such id" without — the grid rule; draining hands every pointer back exactly once, the retired ones alone or all of them
    (tests/c/resident_tables.cpp).  No device: nothing but the header is linked."""
    exe = str(tmp_path / "resident_tables")
    subprocess.check_call([HIPCC, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "raytracegr.jl_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c", "resident_tables.cpp"), "-o", exe])
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert res.stdout.strip() == f"{2 * 33} checks"
