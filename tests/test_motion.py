"""The geometric moving-object detector (include/ssf_motion.h) without a GPU: who exports the entry points, the header on its own,
the struct layouts of the binding, the C++ surface, replay.py's options, the refusals that need no device, and the numpy
restatement the GPU tests compare against (tests/motion_ref.py): known answers, the union-find form equal to the flood fill on
every adversarial image, and the end-to-end scene's mask equal to the pasted box."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import motion_ref as mr
from conftest import ROOT
from supersurfel_fusion_amd import binding, replay

INCLUDE = os.path.join(ROOT, "include")
CPP = os.path.join(ROOT, "tests", "cpp")
SHAPES = [(160, 128), (97, 61)]
f32 = np.float32


def exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], stdout=subprocess.PIPE, text=True, check=True).stdout
    return {l.split()[-1] for l in out.splitlines() if l.strip()}


@functools.lru_cache(maxsize=None)
def cases(W, H):
    return mr.cases(W, H)


def run(case, W, H, form="uf"):
    name, d, m, kw = case
    return mr.segment(d, m, form=form, **dict(mr.default_params(W, H), **kw))


def by_name(W, H, name):
    return [c for c in cases(W, H) if c[0] == name][0]


# ---- the surface ---------------------------------------------------------------------------------------------------------
def test_the_product_exports_the_five_entry_points(product_lib):
    assert len(binding.MOTION_SYMBOLS) == 5 and set(binding.MOTION_SYMBOLS) <= exported(product_lib.path)
    assert product_lib.has_motion


def test_the_checker_does_not_and_the_binding_says_so(oracle_lib):
    assert not set(binding.MOTION_SYMBOLS) & exported(oracle_lib.path)
    assert not oracle_lib.has_motion
    f = binding.Fusion(oracle_lib, oracle_lib.default_config(width=64, height=48, fx=60.0, fy=60.0, cx=31.5, cy=23.5))
    d, rgb = np.ones((48, 64), f32), np.zeros((48, 64, 3), np.uint8)
    for call, symbol in ((f.motion_default_params, "ssf_motion_default_params"), (lambda: f.motion_segment(d, d), "ssf_motion_segment"),
                         (lambda: f.motion_mask(d), "ssf_motion_mask"), (lambda: f.motion_mask_device(1, mask=1), "ssf_motion_mask"),
                         (f.last_motion_mask, "ssf_get_motion_mask"), (lambda: f.process_frame(rgb, d, motion=True), "ssf_process_frame_motion"),
                         (lambda: f.process_frame_device(1, 1, motion={}), "ssf_process_frame_motion")):
        with pytest.raises(binding.SsfError, match=symbol):
            call()


def test_the_motion_symbols_stay_out_of_ssf_h():
    for nm in binding.MOTION_SYMBOLS:
        assert nm not in binding.ABI_SYMBOLS
        assert nm not in open(os.path.join(INCLUDE, "ssf.h")).read()
        assert nm in open(os.path.join(INCLUDE, "ssf_motion.h")).read()
    assert "#define SSF_ABI_VERSION 3" in open(os.path.join(INCLUDE, "ssf.h")).read()


def test_the_motion_kernels_read_no_environment():
    txt = open(os.path.join(ROOT, "supersurfel_fusion_amd", "csrc", "ssf_motion.hip")).read()
    assert "getenv(" not in txt and "SSF_ENV" not in txt


def test_the_makefile_builds_the_file():
    mk = open(os.path.join(ROOT, "supersurfel_fusion_amd", "csrc", "Makefile")).read()
    srcs = [l for l in mk.splitlines() if l.startswith("SRCS")][0]
    hdrs = [l for l in mk.splitlines() if l.startswith("HDRS")][0]
    assert "ssf_motion.hip" in srcs.split() and "../../include/ssf_motion.h" in hdrs.split()


@pytest.mark.parametrize("lang", ["c", "c++"])
def test_the_header_compiles_on_its_own(lang, tmp_path):
    src = tmp_path / ("t.c" if lang == "c" else "t.cpp")
    src.write_text('#include "ssf_motion.h"\n'
                   "int f(ssf_handle* h, const void* d, const float* m, uint8_t* k, int32_t* l, uint8_t* c, float* o) {\n"
                   "    ssf_motion_params p; ssf_motion_stats s;\n"
                   "    if (ssf_motion_default_params(h, &p) != SSF_OK) return -1;\n"
                   "    p.min_seeds = 3; p.on_device = 0;\n"
                   "    return ssf_motion_segment(h, &p, d, m, k, l, c, &s) + ssf_motion_mask(h, &p, d, k, l, c, o, &s) +\n"
                   "           ssf_get_motion_mask(h, k, &s) + (int)s.pixels_masked + (int)SSF_MOTION_UNKNOWN; }\n")
    cc, std = ("gcc", "-std=c99") if lang == "c" else ("g++", "-std=c++11")
    r = subprocess.run([cc, std, "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", INCLUDE, "-c", str(src), "-o", str(tmp_path / "t.o")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout


def test_the_ctypes_structs_have_the_headers_layout(tmp_path):
    """a C probe prints sizeof and every offsetof of the two structs; the binding's ctypes structures must agree"""
    fields = {"ssf_motion_params": [nm for nm, _ in binding.SsfMotionParams._fields_],
              "ssf_motion_stats": [nm for nm, _ in binding.SsfMotionStats._fields_]}
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "ssf_motion.h"', "int main(void) {"]
    for st, names in fields.items():
        lines.append('    printf("%s.sizeof=%%zu\\n", sizeof(%s));' % (st, st))
        lines += ['    printf("%s.%s=%%zu\\n", offsetof(%s, %s));' % (st, nm, st, nm) for nm in names]
    lines += ['    printf("classes=%d%d%d%d\\n", SSF_MOTION_INVALID, SSF_MOTION_STATIC, SSF_MOTION_SEED, SSF_MOTION_UNKNOWN);', "    return 0; }"]
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines) + "\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", INCLUDE, str(src), "-o", str(tmp_path / "probe")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    got = dict(l.split("=") for l in subprocess.run([str(tmp_path / "probe")], stdout=subprocess.PIPE, text=True, check=True).stdout.split())
    for st, cls in (("ssf_motion_params", binding.SsfMotionParams), ("ssf_motion_stats", binding.SsfMotionStats)):
        assert int(got[st + ".sizeof"]) == C.sizeof(cls), st
        for nm in fields[st]:
            assert int(got["%s.%s" % (st, nm)]) == getattr(cls, nm).offset, (st, nm)
    assert got["classes"] == "%d%d%d%d" % tuple(binding.MOTION_CLASSES[k] for k in ("invalid", "static", "seed", "unknown"))
    assert (mr.INVALID, mr.STATIC, mr.SEED, mr.UNKNOWN) == (0, 1, 2, 3)


def test_ssf_hpp_motion_overloads_compile_and_link_against_the_product(product_lib, tmp_path):
    libdir = os.path.dirname(product_lib.path)
    cmd = ["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", "-I", INCLUDE, "-I", CPP, os.path.join(CPP, "motion_smoke.cpp"),
           "-o", str(tmp_path / "motion_smoke"), "-L", libdir, "-lssf_hip", "-Wl,-rpath," + libdir]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout


def test_the_pose_prior_overload_stays_unambiguous(tmp_path):
    src = tmp_path / "t.cpp"
    src.write_text('#include "ssf.hpp"\n'
                   "void f(supersurfel_fusion::SupersurfelFusion& s, const uint8_t* c, const float* d) {\n"
                   "    s.processFrame(c, d, nullptr); s.processFrame(c, d, supersurfel_fusion::MotionParams()); }\n")
    r = subprocess.run(["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-I", INCLUDE, "-c", str(src), "-o", str(tmp_path / "t.o")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout


def test_the_refusals_that_need_no_handle(product_lib):
    L = product_lib.lib
    p, s = binding.SsfMotionParams(), binding.SsfMotionStats()
    buf = (C.c_uint8 * 16)()
    assert L.ssf_motion_default_params(None, C.byref(p)) == -1
    assert L.ssf_motion_segment(None, C.byref(p), buf, buf, buf, None, None, C.byref(s)) == -1
    assert L.ssf_motion_mask(None, C.byref(p), buf, buf, None, None, None, C.byref(s)) == -1
    assert L.ssf_process_frame_motion(None, buf, buf, 0, None, C.byref(p), None) == -1
    assert L.ssf_get_motion_mask(None, buf, C.byref(s)) == -1


def test_the_replay_options_parse_and_exclude_each_other(capsys):
    a = replay.parse_args(["--npz", "frames.npz", "--detect-motion", "--motion-mask-dir", "masks"])
    assert a.detect_motion and a.motion_mask_dir == "masks"
    b = replay.parse_args(["--npz", "frames.npz"])
    assert not b.detect_motion and b.motion_mask_dir is None
    with pytest.raises(SystemExit):
        replay.parse_args(["--npz", "frames.npz", "--detect-motion", "--dynamic-masks", "m.npz"])
    with pytest.raises(SystemExit):
        replay.parse_args(["--npz", "frames.npz", "--motion-mask-dir", "masks"])            # (needs --detect-motion)
    capsys.readouterr()


def test_replay_refuses_motion_detection_on_a_pipelined_run():
    with pytest.raises(ValueError, match="sequential"):
        replay.replay(None, [], pipelined=True, detect_motion=True)


# ---- the restatement -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", SHAPES)
def test_the_union_find_form_equals_the_flood_fill_on_every_adversarial_image(W, H):
    for case in cases(W, H):
        a, b = run(case, W, H), run(case, W, H, "bfs")
        mr.assert_same(a, b, case[0])
        member = (a["cls"] == mr.SEED) | (a["cls"] == mr.UNKNOWN)
        assert ((a["label"] >= 0) == member).all() and (a["label"][member] <= np.arange(W * H).reshape(H, W)[member]).all()


@pytest.mark.parametrize("W,H", mr.TILE_SHAPES)
def test_the_two_forms_agree_on_the_tile_grids_the_other_shapes_miss(W, H):
    """one row of tiles, one column, a single tile, a last tile one cell wide: the references of the GPU test of the same shapes"""
    comps = {}
    for case in mr.tile_cases(W, H):
        a = run(case, W, H)
        mr.assert_same(a, run(case, W, H, "bfs"), case[0])
        comps[case[0]] = a["stats"]["n_components"]
    comps.pop("random")                                            # (no known answer: the two forms agreeing is its check)
    assert comps == dict(serpentine=1, comb=1, cross=1, full=1, spirals=2, checkerboard=(W * H + 1) // 2), comps


@pytest.mark.parametrize("W,H", SHAPES)
def test_known_answers_of_the_adversarial_images(W, H):
    st = {c[0]: run(c, W, H)["stats"] for c in cases(W, H)}
    assert st["serpentine"]["n_components"] == 1 and st["serpentine"]["pixels_masked"] == st["serpentine"]["n_seed"] > W * H // 2
    assert st["spirals"]["n_components"] == 2 and st["spirals"]["n_dynamic_components"] == 1
    assert st["spirals"]["pixels_masked"] == st["spirals"]["n_seed"] and st["spirals"]["n_unknown"] > 1000
    assert st["comb"]["n_components"] == 1 and st["full"]["n_components"] == 1 and st["full"]["pixels_masked"] == W * H
    assert st["full_unknown"] == dict(n_seed=0, n_unknown=W * H, n_components=1, n_dynamic_components=0, pixels_masked=0)
    assert st["checkerboard"]["n_components"] == st["checkerboard"]["n_seed"] == (W * H + 1) // 2
    assert st["diagonal_blobs"]["n_components"] == 4 and st["cross"]["n_components"] == 1
    assert st["min_seeds"] == dict(n_seed=23, n_unknown=0, n_components=2, n_dynamic_components=1, pixels_masked=12)
    assert st["unknown_per_seed"] == dict(n_seed=10, n_unknown=31, n_components=2, n_dynamic_components=1, pixels_masked=20)


def test_a_difference_on_the_link_threshold_links_and_one_ulp_above_does_not():
    W, H = SHAPES[0]
    out = run(by_name(W, H, "link_threshold"), W, H)
    lab = out["label"]
    assert (lab[0::2, 0] == lab[0::2, 1]).all() and (lab[0::2, 0] >= 0).all()
    assert (lab[0::2, 3] != lab[0::2, 4]).all() and (lab[0::2, 3] >= 0).all() and (lab[0::2, 4] >= 0).all()
    assert out["stats"]["n_components"] == 3 * (H // 2)
    noise = run(by_name(W, H, "link_noise"), W, H)["stats"]["n_components"]
    assert (H // 2) * W // 4 < noise < (H // 2) * W * 3 // 4          # (the ramp is cut at about every second step)


def test_a_pixel_exactly_tau_in_front_is_no_seed_and_one_ulp_more_is():
    W, H = SHAPES[0]
    name, d, m, kw = by_name(W, H, "tau_threshold")
    cls = run((name, d, m, kw), W, H)["cls"]
    assert (cls[0::2, 0::2] == mr.STATIC).all() and (cls[0::2, 1::4] == mr.SEED).all() and (cls[1::2, :] == mr.STATIC).all()


def test_invalid_depths_are_invalid_and_the_ends_of_the_range_are_valid():
    W, H = SHAPES[1]
    name, d, m, kw = by_name(W, H, "invalid_depths")
    cls = run((name, d, m, kw), W, H)["cls"]
    with np.errstate(invalid="ignore"):
        bad = ~np.isfinite(d) | (d < f32(0.2)) | (d > f32(5.0))
    assert bad.sum() > 100 and (cls[bad] == mr.INVALID).all() and (cls[~bad] != mr.INVALID).all()
    assert cls[0, 0] != mr.INVALID and cls[0, 1] != mr.INVALID


def test_uint16_depth_is_scaled_in_double_and_rounded_once():
    v = np.array([[0, 1, 5000, 65535]], np.uint16)
    got = mr.convert_depth(v, 0.0002)
    assert got.dtype == f32 and got[0].tolist() == [float(f32(float(x) * 0.0002)) for x in v[0]]


@pytest.mark.parametrize("W,H", SHAPES)
def test_on_the_end_to_end_scene_the_mask_is_exactly_the_pasted_box(W, H):
    """the wall is in the map (m = the scene's noise-free depth), the box is half a metre in front of it"""
    for k in (6, 7, 8):
        rgb, depth, clean, (y0, y1, x0, x1) = mr.box_scene(k, W, H)
        out = mr.segment(depth, clean, **mr.default_params(W, H))
        want = np.zeros((H, W), np.uint8)
        want[y0:y1, x0:x1] = 1
        assert np.array_equal(out["mask"], want), (k, int(out["mask"].sum()), int(want.sum()))
        assert out["stats"]["n_dynamic_components"] == 1 and out["stats"]["pixels_masked"] == (y1 - y0) * (x1 - x0)
        assert (rgb[y0:y1, x0:x1] == (200, 40, 40)).all()
