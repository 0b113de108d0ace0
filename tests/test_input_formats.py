"""Raw sensor frames (include/ssf_input.h) without a GPU: who exports the entry points, the new header on its own, the C++
surface with the uint16 overloads, the binding on a library without them, replay.py's option."""
import os
import subprocess

import pytest

from conftest import ROOT
from supersurfel_fusion_amd import binding, replay

INCLUDE = os.path.join(ROOT, "include")
CPP = os.path.join(ROOT, "tests", "cpp")


def exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], stdout=subprocess.PIPE, text=True, check=True).stdout
    return {l.split()[-1] for l in out.splitlines() if l.strip()}


def test_the_product_exports_the_input_format_entry_points(product_lib):
    assert set(binding.INPUT_FORMAT_SYMBOLS) <= exported(product_lib.path)
    assert product_lib.has_input_format


def test_the_checker_does_not_and_the_binding_says_so(oracle_lib):
    assert not set(binding.INPUT_FORMAT_SYMBOLS) & exported(oracle_lib.path)
    assert not oracle_lib.has_input_format
    f = binding.Fusion(oracle_lib, oracle_lib.default_config(width=64, height=48, fx=60.0, fy=60.0, cx=31.5, cy=23.5))
    with pytest.raises(binding.SsfError, match="does not export ssf_set_input_format"):
        f.set_input_format("bgr8", "u16", 0.0002)
    with pytest.raises(binding.SsfError, match="does not export ssf_get_input_format"):
        f.input_format()
    assert (f.color_format, f.depth_format) == ("rgb8", "f32")


def test_the_input_format_symbols_stay_out_of_ssf_h():
    """ssf.h is the ABI both libraries export (ABI_SYMBOLS); the new entry points live in ssf_input.h alone"""
    for nm in binding.INPUT_FORMAT_SYMBOLS:
        assert nm not in binding.ABI_SYMBOLS
        assert nm not in open(os.path.join(INCLUDE, "ssf.h")).read()
        assert nm not in open(os.path.join(INCLUDE, "ssf_testing.h")).read()
        assert nm in open(os.path.join(INCLUDE, "ssf_input.h")).read()
    assert "#define SSF_ABI_VERSION 3" in open(os.path.join(INCLUDE, "ssf.h")).read()


@pytest.mark.parametrize("lang", ["c", "c++"])
def test_the_header_compiles_on_its_own(lang, tmp_path):
    src = tmp_path / ("t.c" if lang == "c" else "t.cpp")
    src.write_text('#include "ssf_input.h"\n'
                   "int f(ssf_handle* h) { return ssf_set_input_format(h, SSF_COLOR_BGRA8, SSF_DEPTH_U16_SCALED, 0.0002); }\n"
                   "int g(const ssf_handle* h, int* c, int* d, double* s) { return ssf_get_input_format(h, c, d, s); }\n")
    cc, std = ("gcc", "-std=c99") if lang == "c" else ("g++", "-std=c++11")
    r = subprocess.run([cc, std, "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", INCLUDE, "-c", str(src), "-o", str(tmp_path / "t.o")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout


def build_smoke(lib_path, lib_name, exe):
    """tests/cpp/input_format_smoke.cpp (ssf.hpp's uint16 overloads and the cv::Mat double with CV_16UC1) linked against a library"""
    libdir = os.path.dirname(lib_path)
    cmd = ["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", "-I", INCLUDE, "-I", CPP, os.path.join(CPP, "input_format_smoke.cpp"),
           "-o", str(exe), "-L", libdir, "-l" + lib_name, "-Wl,-rpath," + libdir]
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


def test_ssf_hpp_raw_overloads_compile_and_link_against_the_product(product_lib, tmp_path):
    r = build_smoke(product_lib.path, "ssf_hip", tmp_path / "input_format_smoke")
    assert r.returncode == 0, r.stdout


def test_the_old_cv_double_still_compiles_the_cv_overload(tmp_path):
    """without CV_16UC1 the cv::Mat overload keeps its float-only body (tests/cpp/cv_double.hpp)"""
    src = tmp_path / "t.cpp"
    src.write_text('#include "cv_double.hpp"\n#include "ssf.hpp"\n'
                   "void f(supersurfel_fusion::SupersurfelFusion& s, const cv::Mat& a, const cv::Mat& b) { s.processFrame(a, b); }\n")
    r = subprocess.run(["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-I", INCLUDE, "-I", CPP, "-c", str(src), "-o", str(tmp_path / "t.o")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout


def test_the_replay_option_parses():
    a = replay.parse_args(["--npz", "frames.npz", "--raw-frames", "--depth-scale", "0.001"])
    assert a.raw_frames and a.depth_scale == 0.001 and a.npz == "frames.npz"
    assert not replay.parse_args(["--npz", "frames.npz"]).raw_frames


def test_raw_npz_frames_are_the_stored_counts():
    import numpy as np
    path = os.path.join(ROOT, "tests", "golden", "tum_fr3_walking_4frames.npz")
    for (s0, c0, f32), (s1, c1, d16) in zip(replay.frames_from_npz(path), replay.frames_from_npz(path, raw=True)):
        assert s0 == s1 and d16.dtype == np.uint16 and np.array_equal(c0, c1)
        assert np.array_equal(replay.convert_depth(d16, 0.0002).view(np.uint32), f32.view(np.uint32))
