"""The offsets of a call's host arrays in the staging buffer (csrc/ssf_stage_layout.hpp, used by StagedIo in ssf_handle.hpp for
ssf_render_model, ssf_query_rows, ssf_raycast, ssf_navgrid_build, ssf_navgrid_carve, ssf_navlive_overlay, ssf_navmem_update,
ssf_navdyn_blobs, ssf_navplan_field, ssf_navpose_field, ssf_navfrontier_regions, ssf_navpath_waypoints, ssf_navfoot_layers and the
four rollouts: ssf_navsteer_rollouts, ssf_navfoot_rollouts, ssf_navdyn_rollouts, ssf_navdyn_foot_rollouts):
tests/cpp/stage_layout_smoke.cpp, a program of its own over the part that includes no HIP header, built with the address and
undefined-behaviour sanitizers and run as a process."""
import os
import subprocess

from conftest import ROOT

CPP = os.path.join(ROOT, "tests", "cpp")


def test_stage_layout_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "stage_layout_smoke")
    cmd = ["g++", "-std=c++11", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(CPP, "stage_layout_smoke.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert r.returncode == 0 and "stage_layout_smoke ok" in r.stdout, r.stdout
