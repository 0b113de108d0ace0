"""Dense RGB-D odometry (include/ssf_odometry.h) without a GPU: who exports the entry points, the header on its own, the struct
layouts of the binding, the C++ surface, replay.py's option, and the numpy restatement the GPU tests compare against
(tests/odometry_ref.py): known answers of the pyramid, the range and format rules, the mask, the record of a frame against itself,
the header's overflow argument evaluated at 1280 x 960, the recovery of known motions on synthetic and real frames, and, for every
input of tests/test_odometry_edges_gpu.py (tests/odometry_cases.py), that the restatement's output on it has the property the input
was built for."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import odometry_cases as oc
import odometry_ref as orf
from conftest import ROOT
from odometry_cases import exact_frame
from supersurfel_fusion_amd import binding, replay, synthetic

INCLUDE = os.path.join(ROOT, "include")
CPP = os.path.join(ROOT, "tests", "cpp")
GOLD = os.path.join(ROOT, "tests", "golden")
f32 = np.float32

# profiles/odometry.txt (tools/odometry_probe.py --accuracy): (translation error m, rotation error rad) of the restatement with
# the default parameters; the result is deterministic, the tests allow twice these figures (room for later edits of the scene
# generator), and on top of that the estimate must be strictly closer to the truth than the identity in both
SYNTH = {
    False: [(0.00220, 0.00094), (0.00335, 0.00154), (0.00296, 0.00127), (0.00449, 0.00216), (0.00199, 0.00089), (0.00155, 0.00080),
            (0.00193, 0.00089), (0.00175, 0.00062), (0.00181, 0.00106), (0.00070, 0.00055), (0.00209, 0.00089), (0.00479, 0.00209)],
    True: [(0.00218, 0.00093), (0.00334, 0.00153), (0.00295, 0.00126), (0.00450, 0.00217), (0.00200, 0.00090), (0.00157, 0.00080),
           (0.00191, 0.00088), (0.00178, 0.00063), (0.00179, 0.00106), (0.00074, 0.00056), (0.00209, 0.00089), (0.00487, 0.00212)],
}
REAL = [(0.00647, 0.00781), (0.00709, 0.00411), (0.00541, 0.00499), (0.00091, 0.00522), (0.00283, 0.00203), (0.00558, 0.00805),
        (0.00449, 0.00739)]
# the recorded outcome per real pair: (valid, closer in translation, closer in angle)
REAL_OUTCOME = [(1, True, True)] * 7


def exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], stdout=subprocess.PIPE, text=True, check=True).stdout
    return {l.split()[-1] for l in out.splitlines() if l.strip()}


# ---- the surface ---------------------------------------------------------------------------------------------------------
def test_the_product_exports_the_seven_entry_points(product_lib):
    assert len(binding.ODOMETRY_SYMBOLS) == 7 and set(binding.ODOMETRY_SYMBOLS) <= exported(product_lib.path)
    assert "ssf_odometry_get_pyramid" in exported(product_lib.path)
    assert product_lib.has_odometry


def test_the_checker_does_not_and_the_binding_says_so(oracle_lib):
    assert not set(binding.ODOMETRY_SYMBOLS) & exported(oracle_lib.path)
    assert not oracle_lib.has_odometry
    f = binding.Fusion(oracle_lib, oracle_lib.default_config(width=64, height=48, fx=60.0, fy=60.0, cx=31.5, cy=23.5))
    d, rgb = np.ones((48, 64), f32), np.zeros((48, 64, 3), np.uint8)
    for call, symbol in ((f.odometry_default_params, "ssf_odometry_default_params"), (lambda: f.odometry_set_reference(rgb, d), "ssf_odometry_set_reference"),
                         (lambda: f.odometry_set_reference_device(1, 1), "ssf_odometry_set_reference"),
                         (lambda: f.odometry_linearise(0, orf.IDENTITY12), "ssf_odometry_linearise"), (lambda: f.odometry_estimate(rgb, d), "ssf_odometry_estimate"),
                         (lambda: f.odometry_estimate_device(1, 1), "ssf_odometry_estimate"), (lambda: f.odometry_track(rgb, d), "ssf_odometry_track"),
                         (lambda: f.odometry_track_device(1, 1), "ssf_odometry_track"), (f.odometry_last, "ssf_get_odometry"),
                         (lambda: f.odometry_pyramid(0, 0), "ssf_odometry_get_pyramid"),
                         (lambda: f.process_frame(rgb, d, odometry=True), "ssf_process_frame_odometry"),
                         (lambda: f.process_frame_device(1, 1, odometry={}), "ssf_process_frame_odometry")):
        with pytest.raises(binding.SsfError, match=symbol):
            call()


def test_the_odometry_symbols_stay_out_of_ssf_h():
    for nm in binding.ODOMETRY_SYMBOLS:
        assert nm not in binding.ABI_SYMBOLS
        assert nm not in open(os.path.join(INCLUDE, "ssf.h")).read()
        assert nm in open(os.path.join(INCLUDE, "ssf_odometry.h")).read()
    assert "#define SSF_ABI_VERSION 3" in open(os.path.join(INCLUDE, "ssf.h")).read()


def test_the_odometry_kernels_read_no_environment():
    txt = open(os.path.join(ROOT, "supersurfel_fusion_amd", "csrc", "ssf_odometry.hip")).read()
    assert "getenv(" not in txt and "SSF_ENV" not in txt
    assert "k_odo_linearise" in txt and "k_odo_pyramid" in txt


def test_the_makefile_builds_the_file():
    mk = open(os.path.join(ROOT, "supersurfel_fusion_amd", "csrc", "Makefile")).read()
    srcs = [l for l in mk.splitlines() if l.startswith("SRCS")][0]
    hdrs = [l for l in mk.splitlines() if l.startswith("HDRS")][0]
    assert "ssf_odometry.hip" in srcs.split() and "../../include/ssf_odometry.h" in hdrs.split()


@pytest.mark.parametrize("lang", ["c", "c++"])
def test_the_header_compiles_on_its_own(lang, tmp_path):
    src = tmp_path / ("t.c" if lang == "c" else "t.cpp")
    src.write_text('#include "ssf_odometry.h"\n'
                   "int f(ssf_handle* h, const void* c, const void* d, const uint8_t* m, float* t12, int64_t* rec, ssf_frame_result* out) {\n"
                   "    ssf_odometry_params p; ssf_odometry_result r;\n"
                   "    if (ssf_odometry_default_params(h, &p) != SSF_OK) return -1;\n"
                   "    p.levels = 3; p.iters[SSF_ODO_MAX_LEVELS - 1] = 0;\n"
                   "    return ssf_odometry_set_reference(h, c, d, 0, m) + ssf_odometry_linearise(h, &p, 0, t12, rec) +\n"
                   "           ssf_odometry_estimate(h, &p, c, d, 0, t12, t12, &r) + ssf_odometry_track(h, &p, c, d, 0, t12, &r) +\n"
                   "           ssf_process_frame_odometry(h, c, d, 0, &p, 0, out) + ssf_get_odometry(h, t12, t12, &r) + (int)r.pixels +\n"
                   "           (int)SSF_ODO_MOTION_GATE + SSF_ODO_RECORD + SSF_ODO_S_A + SSF_ODO_S_B + SSF_ODO_S_C + SSF_ODO_CLAMP_BITS; }\n")
    cc, std = ("gcc", "-std=c99") if lang == "c" else ("g++", "-std=c++11")
    r = subprocess.run([cc, std, "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", INCLUDE, "-c", str(src), "-o", str(tmp_path / "t.o")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout


def test_the_ctypes_structs_have_the_headers_layout(tmp_path):
    """a C probe prints sizeof and every offsetof of the two structs and the header's constants; the binding and the restatement agree"""
    fields = {"ssf_odometry_params": [nm for nm, _ in binding.SsfOdometryParams._fields_],
              "ssf_odometry_result": [nm for nm, _ in binding.SsfOdometryResult._fields_]}
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "ssf_odometry.h"', "int main(void) {"]
    for st, names in fields.items():
        lines.append('    printf("%s.sizeof=%%zu\\n", sizeof(%s));' % (st, st))
        lines += ['    printf("%s.%s=%%zu\\n", offsetof(%s, %s));' % (st, nm, st, nm) for nm in names]
    lines += ['    printf("reasons=%d%d%d%d%d\\n", SSF_ODO_CONVERGED, SSF_ODO_MAX_ITERATIONS, SSF_ODO_TOO_FEW_PIXELS, SSF_ODO_DEGENERATE, SSF_ODO_MOTION_GATE);',
              '    printf("consts=%d,%d,%d,%d,%d,%d,%d,%d\\n", SSF_ODO_MAX_LEVELS, SSF_ODO_MIN_W, SSF_ODO_MIN_H, SSF_ODO_RECORD, SSF_ODO_S_A, SSF_ODO_S_B, '
              'SSF_ODO_S_C, SSF_ODO_CLAMP_BITS);', "    return 0; }"]
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines) + "\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", INCLUDE, str(src), "-o", str(tmp_path / "probe")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    got = dict(l.split("=") for l in subprocess.run([str(tmp_path / "probe")], stdout=subprocess.PIPE, text=True, check=True).stdout.split())
    for st, cls in (("ssf_odometry_params", binding.SsfOdometryParams), ("ssf_odometry_result", binding.SsfOdometryResult)):
        assert int(got[st + ".sizeof"]) == C.sizeof(cls), st
        for nm in fields[st]:
            assert int(got["%s.%s" % (st, nm)]) == getattr(cls, nm).offset, (st, nm)
    assert got["reasons"] == "01234" and binding.ODOMETRY_REASONS == orf.REASONS and len(orf.REASONS) == 5
    assert got["consts"] == "%d,%d,%d,%d,%d,%d,%d,%d" % (orf.MAX_LEVELS, orf.MIN_W, orf.MIN_H, orf.RECORD, orf.S_A, orf.S_B, orf.S_C, orf.CLAMP_BITS)
    assert (binding.ODO_MAX_LEVELS, binding.ODO_RECORD) == (orf.MAX_LEVELS, orf.RECORD)


def test_the_documented_defaults_are_the_restatements_and_the_wrappers():
    """the defaults are written in four places: the header's text, ssf_odometry_default_params, ssf.hpp and odometry_ref.py"""
    p = orf.default_params()
    hdr = open(os.path.join(INCLUDE, "ssf_odometry.h")).read()
    hip = open(os.path.join(ROOT, "supersurfel_fusion_amd", "csrc", "ssf_odometry.hip")).read()
    hpp = open(os.path.join(INCLUDE, "ssf.hpp")).read()
    assert "levels 4, iters {4, 6, 8, 10, 10, 10}" in hdr and "r_max 0.5, huber 0.2," in hdr and "max_translation 0.3, max_rotation 0.35" in hdr
    assert "p->levels = 4;" in hip and "{4, 6, 8, 10, 10, 10}" in hip and "p->r_max = 0.5f; p->huber = 0.2f; p->min_pixel_share = 0.05f;" in hip
    assert "p->max_translation = 0.3f; p->max_rotation = 0.35f;" in hip and "p->tol_rot = 1e-4f; p->tol_trans = 1e-4f;" in hip
    assert "float r_max = 0.5f, huber = 0.2f, min_pixel_share = 0.05f, tol_rot = 1e-4f, tol_trans = 1e-4f, max_translation = 0.3f, max_rotation = 0.35f;" in hpp
    assert (p["levels"], p["iters"]) == (4, [4, 6, 8, 10, 10, 10])
    assert [float(p[k]) for k in ("r_max", "huber", "min_pixel_share", "tol_rot", "tol_trans", "max_translation", "max_rotation")] == \
        [float(f32(v)) for v in (0.5, 0.2, 0.05, 1e-4, 1e-4, 0.3, 0.35)]


def test_ssf_hpp_odometry_methods_compile_and_link_against_the_product(product_lib, tmp_path):
    libdir = os.path.dirname(product_lib.path)
    cmd = ["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", "-I", INCLUDE, "-I", CPP, os.path.join(CPP, "odometry_smoke.cpp"),
           "-o", str(tmp_path / "odometry_smoke"), "-L", libdir, "-lssf_hip", "-Wl,-rpath," + libdir]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout


def test_the_pose_prior_overload_stays_unambiguous_next_to_the_odometry_overloads(tmp_path):
    src = tmp_path / "t.cpp"
    src.write_text('#include "ssf.hpp"\n'
                   "void f(supersurfel_fusion::SupersurfelFusion& s, const uint8_t* c, const float* d, const uint16_t* u) {\n"
                   "    using namespace supersurfel_fusion;\n"
                   "    s.processFrame(c, d, nullptr); s.processFrame(c, d, MotionParams()); s.processFrame(c, d, OdometryParams());\n"
                   "    s.processFrame(c, u, OdometryParams()); s.processFrame(c, d, OdometryParams(), MotionParams());\n"
                   "    s.processFrame(c, d, MotionParams(), nullptr); s.setOdometryReference(c, d); s.setOdometryReference(c, u, nullptr);\n"
                   "    s.estimateOdometry(c, d); s.trackOdometry(c, u); }\n")
    r = subprocess.run(["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-I", INCLUDE, "-c", str(src), "-o", str(tmp_path / "t.o")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout


def test_the_refusals_that_need_no_handle(product_lib):
    L = product_lib.lib
    p, r = binding.SsfOdometryParams(), binding.SsfOdometryResult()
    buf = (C.c_uint8 * 512)()
    assert L.ssf_odometry_default_params(None, C.byref(p)) == -1
    assert L.ssf_odometry_set_reference(None, buf, buf, 0, None) == -1
    assert L.ssf_odometry_linearise(None, C.byref(p), 0, buf, buf) == -1
    assert L.ssf_odometry_estimate(None, C.byref(p), buf, buf, 0, None, buf, C.byref(r)) == -1
    assert L.ssf_odometry_track(None, C.byref(p), buf, buf, 0, buf, C.byref(r)) == -1
    assert L.ssf_process_frame_odometry(None, buf, buf, 0, C.byref(p), None, None) == -1
    assert L.ssf_get_odometry(None, buf, buf, C.byref(r)) == -1


def test_the_replay_option_parses_and_a_pipelined_run_is_refused(capsys):
    a = replay.parse_args(["--npz", "frames.npz", "--odometry-prior", "--detect-motion"])
    assert a.odometry_prior and a.detect_motion
    assert not replay.parse_args(["--npz", "frames.npz"]).odometry_prior
    with pytest.raises(SystemExit):
        replay.parse_args(["--npz", "frames.npz", "--odometry-prior", "--pipelined"])
    with pytest.raises(SystemExit):
        replay.parse_args(["--npz", "frames.npz", "--odometry-prior", "--dynamic-masks", "m"])
    capsys.readouterr()
    with pytest.raises(ValueError, match="sequential"):
        replay.replay(None, [], pipelined=True, odometry_prior=True)
    with pytest.raises(ValueError, match="mask_dir"):
        replay.replay(None, [], odometry_prior=True, mask_dir="m")


def test_replay_hands_the_frames_to_the_odometry_form_of_process_frame():
    class Fake:
        def __init__(self):
            self.calls = []

        def process_frame(self, rgb, depth, **kw):
            self.calls.append(kw)
            return dict(pose=orf.IDENTITY12, n_model=0)
    f = Fake()
    replay.replay(f, [("1.0", None, None), ("2.0", None, None)], odometry_prior=True)
    assert f.calls == [dict(odometry=True, motion=None)] * 2
    f = Fake()
    replay.replay(f, [("1.0", None, None)], odometry_prior=dict(levels=3), detect_motion=True)
    assert f.calls == [dict(odometry=dict(levels=3), motion=True)]


# ---- the restatement: known answers -----------------------------------------------------------------------------------------
def test_the_luma_is_an_exact_integer_scaled_by_a_power_of_two():
    rgb = np.array([[[0, 0, 0], [255, 255, 255], [255, 0, 0], [0, 255, 0], [0, 0, 255], [10, 20, 30]]], np.uint8)
    want = [0, 255, (77 * 255) >> 8, (150 * 255) >> 8, (29 * 255) >> 8, (770 + 3000 + 870) >> 8]
    got = orf.intensity(rgb)
    assert got.dtype == f32 and (got * 256).tolist() == [[float(v) for v in want]] and got.max() < 1
    assert np.array_equal(orf.intensity(rgb[..., ::-1], "bgr"), got)
    rgba = np.concatenate([rgb, np.full((1, 6, 1), 99, np.uint8)], -1)
    assert np.array_equal(orf.intensity(rgba, "rgba"), got) and np.array_equal(orf.intensity(rgba[..., [2, 1, 0, 3]], "bgra"), got)


def test_the_pyramid_of_a_hand_built_6x4_image():
    I = (np.arange(24, dtype=f32).reshape(4, 6) / f32(32)).astype(f32)
    D = np.array([[1, 2, 0, 0, 3, 0], [4, 1.5, 0, 0, 0, 0.5], [0, 0, 2, 2, 0, 0], [0, 7, 2, 1, 0, 0]], f32)
    In, Dn = orf.reduce_level(I, D)
    assert In.shape == (2, 3) and In.dtype == f32
    assert (In * 32).tolist() == [[3.5, 5.5, 7.5], [15.5, 17.5, 19.5]]                  # block means: exact in f32
    assert Dn.tolist() == [[1.0, 0.0, 0.5], [7.0, 1.0, 0.0]]                            # the smallest valid depth, 0 when none
    gx, gy = orf.gradients(I)
    assert (gx * 64).tolist() == [[1, 2, 2, 2, 2, 1]] * 4                               # central in the middle, one-sided * 0.5 at the border
    assert (gy * 64).tolist() == [[6] * 6, [12] * 6, [12] * 6, [6] * 6]
    assert orf.level_sizes(6, 4) == [(6, 4)] and orf.level_sizes(100, 60) == [(100, 60), (50, 30), (25, 15)]
    assert orf.level_sizes(64, 48) == [(64, 48), (32, 24), (16, 12)] and len(orf.level_sizes(1280, 960)) == 6
    K = orf.level_intrinsics((525.0, 520.0, 319.5, 239.5), 3)
    assert [tuple(float(v) for v in k) for k in K] == [(525.0, 520.0, 319.5, 239.5), (262.5, 260.0, 159.5, 119.5), (131.25, 130.0, 79.5, 59.5)]


def test_a_depth_one_ulp_outside_the_range_is_invalid_and_the_ends_are_valid():
    lo, hi = orf.RANGE
    d = np.array([[lo, np.nextafter(lo, f32(0)), hi, np.nextafter(hi, f32(9)), 0, np.nan, np.inf, -1, 1]], f32)
    assert orf.valid_depth(d).tolist() == [[True, False, True, False, False, False, False, False, True]]
    _, D = orf.level0(np.zeros((1, 9, 3), np.uint8), d)
    assert D.tolist() == [[float(lo), 0.0, float(hi), 0.0, 0.0, 0.0, 0.0, 0.0, 1.0]]


def test_uint16_depth_is_scaled_in_double_and_rounded_once():
    v = np.array([[0, 1, 5000, 65535]], np.uint16)
    got = orf.convert_depth(v, 0.0002)
    assert got.dtype == f32 and got[0].tolist() == [float(f32(float(x) * 0.0002)) for x in v[0]]


def test_a_frame_against_itself_at_the_identity_has_no_residual():
    rgb, depth, K = exact_frame()
    pyr = orf.pyramid(rgb, depth, K)
    for lv in pyr:
        rec = orf.record(lv, lv, orf.IDENTITY12, orf.params())
        inner = (lv["D"][:-1, :-1] != 0).sum()                    # (the last row and column have no four neighbours)
        assert rec[28] == inner > 0 and not rec[21:28].any() and rec[0] > 0 and rec[6] > 0
        assert np.array_equal(rec, orf.record(lv, lv, orf.IDENTITY12, orf.params(), exact=True))


def test_a_masked_pixel_contributes_nothing_to_the_record():
    rgb, depth, K = exact_frame(seed=1)
    rgb2 = exact_frame(seed=2)[0]
    depth[20, 30] = 1
    mask = np.zeros(depth.shape, np.uint8)
    mask[20, 30] = 7
    only = np.ones(depth.shape, np.uint8)
    only[20, 30] = 0
    cur = orf.pyramid(rgb2, depth, K)[0]
    p = orf.params(r_max=1.0)
    T = synthetic.pose12(synthetic.rot_y(0.01), [0.004, 0.0, 0.002])
    full, masked, alone = (orf.record(orf.pyramid(rgb, depth, K, mask=m)[0], cur, T, p) for m in (None, mask, only))
    assert alone[28] == 1 and alone[:21].any()
    assert np.array_equal(full - masked, alone)
    # on a coarser level the masked pixel no longer offers its depth to the block
    a, b = orf.pyramid(rgb, depth, K)[1]["D"], orf.pyramid(rgb, depth, K, mask=mask)[1]["D"]
    assert (a != b).sum() <= 1 and np.array_equal(orf.pyramid(rgb, depth, K)[1]["I"], orf.pyramid(rgb, depth, K, mask=mask)[1]["I"])


def test_no_term_of_a_worst_case_1280x960_image_saturates_and_no_sum_can_overflow():
    """the header's overflow argument evaluated: the steepest gradient everywhere (a 2 x 2-block checkerboard of 0 / 255), every
    depth at range_min, the current image the negative of the reference (|r| close to 1, gates wide open)"""
    W, H = 1280, 960
    K = synthetic.intrinsics(W, H)
    yy, xx = np.mgrid[0:H, 0:W]
    chk = (((xx // 2) + (yy // 2)) % 2).astype(np.uint8) * 255
    rgb = np.repeat(chk[..., None], 3, -1)
    depth = np.full((H, W), orf.RANGE[0], f32)
    K4 = (K["fx"], K["fy"], K["cx"], K["cy"])
    assert K["fx"] <= 2048 and orf.RANGE[0] >= f32(0.1)                               # the header's assumptions
    ref, cur = orf.pyramid(rgb, depth, K4)[0], orf.pyramid(255 - rgb, depth, K4)[0]
    assert abs(ref["gx"]).max() > 0.49 and abs(ref["gy"]).max() > 0.49 and abs(ref["gx"]).max() <= 0.5
    p = orf.params(r_max=1.0, huber=1.0)
    worst = 0
    for T in (orf.IDENTITY12, synthetic.pose12(synthetic.rot_y(0.02), [0.01, 0.0, 0.01])):
        q, n, J, r, w = orf.terms(ref, cur, T, p)
        assert n > W * H // 2 and abs(r).max() > 0.9 and max(abs(j).max() for j in J) < 2 ** 15
        assert abs(q[:21]).max() < orf.CLAMP and abs(q[21:27]).max() < 2 ** 39 and abs(q[27]).max() <= 2 ** orf.S_C
        worst = max(worst, int(abs(q).max()))
    assert 0 < worst < orf.CLAMP
    assert W * H < 2 ** 21 and (W * H) * orf.CLAMP < 2 ** 62                           # whatever the terms: no int64 sum overflows
    # and the clamp itself: a term beyond it saturates, a NaN gives 0
    big = orf.quantise(np.array([3e38, -3e38, np.nan, 1.0], f32), orf.S_A)
    assert big.tolist() == [orf.CLAMP, -orf.CLAMP, 0, 1 << orf.S_A]


# ---- recovery ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def synthetic_pyramid(k, noise):
    W, H = 160, 128
    K = synthetic.intrinsics(W, H)
    R, t = synthetic.orbit_pose(k)
    rgb, depth, _ = synthetic.render(R, t, W, H, noise=noise, rng=np.random.default_rng(1000 + k))
    return orf.pyramid(rgb, depth, (K["fx"], K["fy"], K["cx"], K["cy"]))


@pytest.mark.parametrize("noise", [False, True])
def test_recovery_on_synthetic_frames(noise, oracle_lib):
    """orbit_pose(k) -> orbit_pose(k + 1) at 160 x 128, k = 0 .. 11: the estimate is valid, strictly closer to the true relative
    motion than the identity in translation and in angle, and within twice the error measured in profiles/odometry.txt"""
    for k in range(12):
        true = orf.true_rel(synthetic.orbit_pose(k), synthetic.orbit_pose(k + 1))
        rel, res = orf.estimate(synthetic_pyramid(k, noise), synthetic_pyramid(k + 1, noise), orf.params(), oracle_lib)
        err, idn = orf.errors(rel, true), orf.errors(orf.IDENTITY12, true)
        print("k %d noise %s: %s err %s identity %s" % (k, noise, res, err, idn))
        assert res["valid"] == 1, (k, res)
        assert err[0] < idn[0] and err[1] < idn[1], (k, err, idn)
        assert err[0] <= 2 * SYNTH[noise][k][0] and err[1] <= 2 * SYNTH[noise][k][1], (k, err, SYNTH[noise][k])


def test_recovery_on_the_committed_fr1_xyz_frames(oracle_lib):
    """the seven consecutive pairs of the eight committed frames against tests/golden/fr1_xyz_gt.txt: exactly the recorded outcome
    (all seven valid and closer than the identity in both), within twice the recorded errors"""
    frames = list(replay.frames_from_npz(os.path.join(GOLD, "tum_fr1_xyz_8frames.npz")))
    stamps, xyz, quat = replay.read_trajectory(os.path.join(GOLD, "fr1_xyz_gt.txt"))
    assert [f[0] for f in frames] == list(stamps[:8])
    K = tuple(replay.BENCHMARK_LAUNCH[k] for k in ("fx", "fy", "cx", "cy"))
    pyr = [orf.pyramid(rgb, depth, K) for _, rgb, depth in frames]
    poses = [(orf.quat_to_R(quat[i]), np.asarray(xyz[i], np.float64)) for i in range(8)]
    outcome = []
    for i in range(7):
        true = orf.true_rel(poses[i], poses[i + 1])
        rel, res = orf.estimate(pyr[i], pyr[i + 1], orf.params(), oracle_lib)
        err, idn = orf.errors(rel, true), orf.errors(orf.IDENTITY12, true)
        print("pair %d: %s err %s identity %s" % (i, res, err, idn))
        outcome.append((res["valid"], err[0] < idn[0], err[1] < idn[1]))
        assert err[0] <= 2 * REAL[i][0] and err[1] <= 2 * REAL[i][1], (i, err, REAL[i])
    assert outcome == REAL_OUTCOME
    assert sum(1 for v, a, b in outcome if v and a and b) >= 5


def test_the_prior_composition_is_the_f32_product_of_the_two_poses():
    R, t = synthetic.orbit_pose(3)
    a, r = synthetic.pose12(R, t), synthetic.pose12(synthetic.rot_y(0.02), [0.01, 0.002, -0.004])
    got = orf.compose(a, r)
    want = np.concatenate([(R @ synthetic.rot_y(0.02)).ravel(), R @ np.array([0.01, 0.002, -0.004]) + t])
    assert got.dtype == f32 and np.abs(got - want).max() < 1e-6
    assert np.array_equal(orf.compose(orf.IDENTITY12, r), r)
    T = orf.from12(r)
    assert np.abs(orf.mat4_lmul(orf.invert(T), T) - np.eye(4)).max() < 1e-7


# ---- the inputs of tests/test_odometry_edges_gpu.py (tests/odometry_cases.py): each is shown to reach what it is there for ------
def test_644x410_has_six_levels_four_odd_reductions_and_more_pixels_than_the_launch_has_threads():
    W, H = oc.BIG
    assert W * H == 264040 > oc.MAX_BLOCKS * oc.BLOCK and -(-W * H // oc.BLOCK) == 1032
    assert orf.level_sizes(W, H) == oc.BIG_SIZES and len(oc.BIG_SIZES) == orf.MAX_LEVELS
    assert sum(1 for w, h in oc.BIG_SIZES[:-1] if w % 2 or h % 2) == 4
    W3, H3 = oc.THREE_TRIPS
    assert 2 * oc.MAX_BLOCKS * oc.BLOCK < W3 * H3 < 3 * oc.MAX_BLOCKS * oc.BLOCK
    assert [orf.level_sizes(w, h) for w, h, _ in oc.ODD] == [s for _, _, s in oc.ODD]
    for _, _, sizes in oc.ODD:                                           # every reduction but the first starts from an odd width or height
        assert all(w % 2 or h % 2 for w, h in sizes[1:-1]) and len(sizes) >= 3


def test_the_644x410_record_at_the_identity_has_more_than_half_of_every_level():
    W, H = oc.BIG
    ref, cur = oc.pyramid(0, W, H), oc.pyramid(1, W, H)
    p = orf.params(levels=6)
    counts = [int(orf.record(ref[l], cur[l], orf.IDENTITY12, p)[28]) for l in range(6)]
    assert all(2 * n > lv["W"] * lv["H"] for n, lv in zip(counts, ref)), counts
    assert counts[0] == 197048 and counts[5] == 200 and ref[5]["W"] * ref[5]["H"] == 240
    for l in (4, 5):
        assert np.array_equal(orf.record(ref[l], cur[l], oc.transform("small"), p), orf.record(ref[l], cur[l], oc.transform("small"), p, exact=True))
    assert 0 < int(orf.record(ref[5], cur[5], oc.transform("behind"), p)[28]) < counts[5]


def test_the_second_trip_of_644x410_has_pixels_of_its_own_and_the_two_masks_share_out_the_record():
    W, H = oc.BIG
    head, tail = oc.trip_masks(W, H)
    assert head.sum() == oc.MAX_BLOCKS * oc.BLOCK and tail.sum() == 1896 and not (head & tail).any() and (head | tail).all()
    assert head.ravel()[:oc.MAX_BLOCKS * oc.BLOCK].all()
    cur = oc.pyramid(1, W, H)[0]
    p = orf.params(levels=6)
    second, first, full = (orf.record(py[0], cur, orf.IDENTITY12, p) for py in (oc.masked_pyramid(0), oc.masked_pyramid(1), oc.pyramid(0, W, H)))
    assert second[28] == 936 >= 500 and first[28] == full[28] - 936
    assert np.array_equal(first + second, full)
    ys, xs = np.nonzero(oc.masked_pyramid(0)[0]["D"])
    assert (ys * W + xs).min() >= oc.MAX_BLOCKS * oc.BLOCK


def test_1024x513_has_pixels_in_the_record_from_all_three_trips():
    W, H = oc.THREE_TRIPS
    ref, cur = oc.pyramid(0, W, H)[0], oc.pyramid(1, W, H)[0]
    n = oc.MAX_BLOCKS * oc.BLOCK
    assert 2 * n == W * (H - 1)                                          # the third trip is exactly the last row
    counts = {}
    for trip, (lo, hi) in enumerate(((0, n), (n, 2 * n), (2 * n, W * H))):
        only = dict(ref, D=np.where((np.arange(W * H) >= lo) & (np.arange(W * H) < hi), ref["D"].ravel(), f32(0)).reshape(H, W))
        for nm, T in oc.three_trip_transforms():
            counts[(trip, nm)] = int(orf.record(only, cur, T, orf.params())[28])
    print(counts)
    assert counts[(0, "small")] > n // 2 and counts[(1, "small")] > n // 2 and counts[(0, "up")] > n // 2 and counts[(1, "up")] > n // 2
    assert counts[(2, "small")] == 0 and counts[(2, "up")] > W // 4      # (a quarter of the row: depth holes and the residual gate take the rest)


def test_the_dropped_column_of_an_odd_level_reaches_no_coarser_level_but_that_levels_gradients():
    """101 x 63 drops level 0's last column at once; 102 and 202 are even, so there the first dropped column is level 1's (51 and
    101 wide), made of level 0's last two"""
    assert [oc.first_odd_level(W) for W, _ in oc.DROPPED] == [(0, 100), (1, 100), (1, 200)]
    for W, H in oc.DROPPED:
        rgb, depth = oc.frame(0, W, H)
        rgb2, depth2, l = oc.dropped_column_changed(rgb, depth)
        assert (rgb2 != rgb).any(axis=(0, 2)).sum() == (depth2 != depth).any(axis=0).sum() == 1 << l
        a, b = orf.pyramid(rgb, depth, oc.K4(W, H)), orf.pyramid(rgb2, depth2, oc.K4(W, H))
        assert len(a) > l + 1 and a[l]["W"] % 2 == 1
        for x, y in zip(a[l + 1:], b[l + 1:]):
            assert all(np.array_equal(x[nm], y[nm]) for nm in ("I", "D", "gx", "gy"))
        for k, (x, y) in enumerate(zip(a[:l + 1], b[:l + 1])):
            c = 1 << (l - k)                                             # columns of level k behind the dropped one
            assert (x["I"][:, -c:] != y["I"][:, -c:]).all() and np.array_equal(x["I"][:, :-c], y["I"][:, :-c])
            assert (x["D"][:, -c:] != y["D"][:, -c:]).any() and np.array_equal(x["D"][:, :-c], y["D"][:, :-c])
            assert (x["gx"][:, -c - 1:] != y["gx"][:, -c - 1:]).any(axis=0)[[0, -1]].all() and np.array_equal(x["gx"][:, :-c - 1], y["gx"][:, :-c - 1])
            assert (x["gy"][:, -c:] != y["gy"][:, -c:]).any() and np.array_equal(x["gy"][:, :-c], y["gy"][:, :-c])


def test_the_odd_shapes_records_have_pixels_on_every_level_and_levels_6_is_clamped(oracle_lib):
    for W, H, sizes in oc.ODD:
        ref, cur = oc.pyramid(0, W, H), oc.pyramid(1, W, H)
        L = len(sizes)
        assert len(ref) == L == (3 if W == 102 else 4)
        for l in range(L):
            n = {nm: int(orf.record(ref[l], cur[l], T, orf.params(levels=6))[28]) for nm, T in oc.transforms()}
            assert 2 * n["identity"] > sizes[l][0] * sizes[l][1] and 0 < n["behind"] < n["mostly out"] < n["identity"] and n["none left"] == 0
        res = orf.estimate(ref, cur, orf.params(levels=6), oracle_lib)[1]
        assert res["levels"] == L and all(res["iters"][:L]) and res["iters"][L:] == [0] * (6 - L) and res["valid"] == 1


def test_the_planted_u16_counts_fall_on_both_sides_of_both_ends_of_the_range():
    W, H = oc.EDGE_SHAPE
    counts, planted = oc.u16_counts(oc.frame(0, W, H)[1])
    assert counts.dtype == np.uint16 and counts[0, :len(planted)].tolist() == planted and planted[:2] == [0, 65535]
    d = orf.convert_depth(np.array(planted, np.uint16), oc.U16_SCALE)
    ok = orf.valid_depth(d).tolist()
    lo, hi = orf.RANGE
    assert ok[0] is False and ok[1] is False and d[1] > hi
    assert ok[2:6].count(True) >= 1 and ok[2:6].count(False) >= 1 and ok[2:6] == sorted(ok[2:6])           # below range_min, then inside
    assert ok[6:10].count(True) >= 1 and ok[6:10].count(False) >= 1 and ok[6:10] == sorted(ok[6:10], reverse=True)
    assert d[2] < lo <= d[5] and d[6] <= hi < d[9]
    # random alpha bytes, and the four orders name the same image
    rgb = oc.frame(0, W, H)[0]
    want = orf.intensity(rgb)
    for fmt in ("rgb8", "bgr8", "rgba8", "bgra8"):
        c = oc.colour_as(rgb, fmt)
        assert c.shape[2] == (4 if fmt.endswith("a8") else 3) and np.array_equal(orf.intensity(c, fmt[:-1]), want)
        assert not fmt.endswith("a8") or len(np.unique(c[..., 3])) > 200
    assert not np.array_equal(orf.intensity(oc.colour_as(rgb, "bgra8"), "rgba"), want)                          # (r and b swapped shows)


def test_each_planted_depth_block_reduces_to_what_the_header_promises(oracle_lib):
    rgb, depth, blocks = oc.planted_depth_frame()
    lo, hi = orf.RANGE
    flat = np.concatenate([np.array(v, f32) for _, v, _ in blocks])
    for special in (lo, np.nextafter(lo, f32(0)), hi, np.nextafter(hi, f32(np.inf)), f32(-1), f32(1e-42)):
        assert (flat == special).any(), special
    assert np.isnan(flat).any() and np.isposinf(flat).any() and np.isneginf(flat).any() and (flat == 0).any()
    assert np.signbit(flat[flat == 0]).any() and not np.signbit(flat[flat == 0]).all() and 0 < f32(1e-42) < np.finfo(f32).tiny
    pyr = orf.pyramid(rgb, depth, oc.K4(64, 48))
    kinds = set()
    for (x, y), vals, want in blocks:
        assert x % 2 == 0 and y % 2 == 0 and np.array_equal(depth[y:y + 2, x:x + 2].ravel(), np.array(vals, f32), equal_nan=True)
        nvalid = int(orf.valid_depth(np.array(vals, f32)).sum())
        got = pyr[1]["D"][y // 2, x // 2]
        assert got == want and not np.signbit(got), ((x, y), got, want)
        assert want == (min(v for v in vals if orf.valid_depth(np.array([v], f32))[0]) if nvalid else 0)
        kinds.add(min(nvalid, 2))
    assert kinds == {0, 1, 2}
    for lv in pyr:
        assert np.isfinite(lv["D"]).all() and not np.signbit(lv["D"]).any()
    for T in (orf.IDENTITY12, oc.transform("small")):
        assert orf.record(pyr[0], pyr[0], T, orf.params())[28] > 64 * 48 // 2
    rel, res = orf.estimate(pyr, pyr, orf.params(levels=3), oracle_lib, init12=oc.transform("small"))
    assert np.isfinite(rel).all() and res["valid"] == 1 and sum(res["iters"]) > 3


def test_a_narrower_range_takes_pixels_out_of_the_pyramid_and_out_of_the_warp():
    W, H = oc.EDGE_SHAPE
    wide, narrow = [oc.pyramid(k, W, H) for k in (0, 1)], [oc.pyramid(k, W, H, oc.NARROW) for k in (0, 1)]
    assert 0 < (narrow[0][0]["D"] != 0).sum() < (wide[0][0]["D"] != 0).sum()
    for nm in ("small", "behind"):
        T = oc.transform(nm)
        n_wide = orf.record(wide[0][0], wide[1][0], T, orf.params())[28]
        n_narrow = orf.record(narrow[0][0], narrow[1][0], T, orf.params(), rng=oc.NARROW)[28]
        assert 0 < n_narrow < n_wide
    # the gate on Y.z with the same (narrow) pyramids: 1.5 m backwards puts warped depths below 0.6 m that stay above 0.2 m
    assert n_narrow < orf.record(narrow[0][0], narrow[1][0], oc.transform("behind"), orf.params(), rng=orf.RANGE)[28]


def test_the_border_shifts_count_exactly_the_pixels_whose_target_has_four_neighbours():
    rgb, depth, K = oc.border_frame()
    assert (depth == 1).all() and K == oc.EXACT_K
    lv = orf.pyramid(rgb, depth, K)[0]
    p = orf.params(r_max=1.0)
    want = {(-1, 0): 63 * 47, (0, 0): 63 * 47, (1, 0): 62 * 47, (62, 0): 1 * 47, (0, -1): 63 * 47, (0, 46): 63 * 1}
    assert list(want) == oc.BORDER_SHIFTS
    for (kx, ky), n in want.items():
        assert oc.border_count(kx, ky) == n
        q, got, _, r, _ = orf.terms(lv, lv, oc.shift12(kx, ky), p)
        assert got == n == orf.record(lv, lv, oc.shift12(kx, ky), p)[28], (kx, ky, got, n)
        # the warp is exact: the residual is the difference of two pixels of the image
        ys, xs = np.mgrid[0:48, 0:64]
        inside = (xs + kx >= 0) & (xs + kx <= 62) & (ys + ky >= 0) & (ys + ky <= 46)
        assert np.array_equal(r, (lv["I"][(ys + ky)[inside], (xs + kx)[inside]] - lv["I"][inside]))
    # one pixel further and nothing is left; the gate is strict: a target ON the last column is out
    assert orf.record(lv, lv, oc.shift12(63, 0), p)[28] == 0 and orf.record(lv, lv, oc.shift12(0, 47), p)[28] == 0


def test_every_parameter_edge_ends_the_restatements_loop_as_recorded(oracle_lib):
    W, H = oc.EDGE_SHAPE
    ref, cur = oc.pyramid(0, W, H), oc.pyramid(1, W, H)
    res = {nm: orf.estimate(ref, cur, orf.params(levels=3, **kw), oracle_lib) for nm, kw in oc.PARAM_EDGES}
    plain = orf.estimate(ref, cur, orf.params(levels=3), oracle_lib)
    r = res["huber=0"][1]
    assert (r["reason"], r["iters"][:3], r["mean_sq_residual"], r["valid"]) == ("converged", [1, 1, 1], 0.0, 1) and r["pixels"] > 0
    r = res["r_max=0"][1]
    assert (r["reason"], r["iters"][:3], r["valid"]) == ("too_few_pixels", [0, 0, 1], 0) and 0 < r["pixels"] < max(1, int(f32(0.05) * f32(25 * 15)))
    assert (res["tol=0"][1]["reason"], res["tol=0"][1]["iters"][:3]) == ("max_iterations", [4, 6, 8])
    assert (res["iters 2 0 3"][1]["reason"], res["iters 2 0 3"][1]["iters"][:3]) == ("max_iterations", [2, 0, 3])
    assert (res["iters 0 0 3"][1]["reason"], res["iters 0 0 3"][1]["iters"][:3]) == ("max_iterations", [0, 0, 3])
    r = res["max_rotation=0"]
    assert (r[1]["reason"], r[1]["valid"]) == ("motion_gate", 0) and np.array_equal(r[0], plain[0]) and plain[1]["valid"] == 1
    assert max(1, int(f32(1e-9) * f32(W * H))) == 1 and res["min_pixel_share tiny"][1]["valid"] == 1
    r = res["huber above r_max"][1]
    assert r["valid"] == 1 and 0 < r["pixels"] < plain[1]["pixels"] and r["mean_sq_residual"] < f32(0.05) ** 2


def test_a_few_reference_pixels_give_rank_deficient_but_finite_steps(oracle_lib):
    W, H = oc.EDGE_SHAPE
    rgb, depth = oc.frame(0, W, H)
    cur = oc.pyramid(1, W, H)
    p = orf.params(levels=1, min_pixel_share=0.0)
    reasons = set()
    for n in (1, 3, 5, 7):
        ref = orf.pyramid(rgb, depth, oc.K4(W, H), mask=oc.few_pixel_mask(n))
        assert (ref[0]["D"] != 0).sum() == n
        rec = orf.record(ref[0], cur[0], orf.IDENTITY12, p)
        assert rec[28] == n and rec[:21].any()                                        # (each pixel adds one row of J: fewer than six up to n = 5)
        rel, res = orf.estimate(ref, cur, p, oracle_lib)
        assert np.isfinite(rel).all() and res["reason"] != "degenerate"
        reasons.add(res["reason"])
    assert len(reasons) >= 2


def test_the_small_checkerboard_gives_the_largest_words_this_shape_can():
    W, H = oc.EDGE_SHAPE
    rgb, neg, depth = oc.checkerboard()
    ref, cur = orf.pyramid(rgb, depth, oc.K4(W, H))[0], orf.pyramid(neg, depth, oc.K4(W, H))[0]
    assert abs(ref["gx"]).max() > 0.49 and abs(ref["gy"]).max() > 0.49
    p = orf.params(r_max=2.0, huber=2.0)
    rec = orf.record(ref, cur, orf.IDENTITY12, p)
    assert rec[28] == 6161 and max(int(v).bit_length() for v in rec) == 49
    assert np.array_equal(rec, orf.record(ref, cur, orf.IDENTITY12, p, exact=True))
    q, _, _, r, w = orf.terms(ref, cur, orf.IDENTITY12, p)
    assert abs(r).max() > 0.9 and (w == 1).all() and 2 ** 35 <= abs(q).max() < orf.CLAMP
