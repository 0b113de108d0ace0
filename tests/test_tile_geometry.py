"""The window of grid cells around a tile (csrc/ssf_tile_geometry.hpp: CellWindow of the tile kernels, SegParams::win_cells_max and
the relabelling passes' geometry table): tests/cpp/tile_geometry_smoke.cpp, a program of its own over the header, which includes no
HIP header, built with the address and undefined-behaviour sanitizers and run as a process.  Its reference is the two host functions
the header replaced, as they stood at commit 8c714be.  The same program checks the plane filter's geometry (pf_window, pf_plan): every
node within F steps of a core tile in the reference's graph has a slot of its own in the tile's window, for every grid up to 48 x 30
with F <= 10 and the grids the GPU suite runs with F <= 13, and the plan of every such grid fits a workgroup's threads and LDS."""
import os
import subprocess

from conftest import ROOT

CPP = os.path.join(ROOT, "tests", "cpp")


def test_tile_geometry_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "tile_geometry_smoke")
    cmd = ["g++", "-std=c++11", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(CPP, "tile_geometry_smoke.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert r.returncode == 0 and "tile_geometry_smoke ok" in r.stdout, r.stdout
