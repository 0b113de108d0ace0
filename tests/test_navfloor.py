"""The rule of ssf_navfloor_fit (include/ssf_navfloor.h) on its numpy restatement (tests/navfloor_ref.py), without a GPU: which plane
wins on the scenes, the plane against an independent f64 least-squares plane over the same inliers and against the planted one, order
independence, the exactly level floor, the statuses, and that every parameter moved off its default changes some integer of a result
(the guard of the GPU file's parameter rows).  The host steps as the library compiles them (csrc/ssf_navfloor_solve.hpp) are pinned
against the restatement through a stand-alone C++ program."""
import os
import subprocess

import numpy as np
import pytest

import navfloor_ref as fr
import navgrid_ref as nr
from conftest import ROOT

f32 = np.float32
# The fit against np.linalg.lstsq over the same inliers: the two differ by the 2^-10 m quantisation of (x, y, z) and the f32 casts of
# the plane between rounds.  Measured on SCENES (this file, test_the_plane_against_least_squares prints them): at most 0.00216 degrees
# and 0.0806 mm (both on "the low rows win", 300 inliers a metre and more from the origin); allowed: four times that.
LSTSQ_ANGLE_DEG, LSTSQ_HEIGHT_M = 4 * 0.00216, 4 * 0.0806e-3


@pytest.fixture(scope="module")
def fits():
    """every scene once: name -> (model, planted, keywords, expected d, fit)"""
    out = {}
    for name, room_kw, kw, want_d in fr.SCENES + (fr.STEEP,):
        m, planted = fr.room(**room_kw)
        out[name] = (m, planted, kw, want_d, fr.fit(m, len(m["confidences"]) // 2, fr.CAMERA, fr.params(**kw)))
    return out


def angle_deg(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.degrees(np.arctan2(np.linalg.norm(np.cross(a, b)), a @ b)))


def planted_d(planted, level_d, origin):
    """the offset of the level plane at level_d, seen from `origin`"""
    return level_d - float(planted["normal"] @ np.asarray(origin, np.float64))


@pytest.mark.parametrize("name", [s[0] for s in fr.SCENES])
def test_the_scenes_find_the_plane_the_rule_names(name, fits):
    m, planted, kw, want_d, got = fits[name]
    assert got["status"] == fr.OK and got["rounds"] == 3, (name, got["status"])
    # within 0.5 degrees and 1 cm of the planted plane
    assert angle_deg(got["normal"], planted["normal"]) < 0.5, name
    assert abs(float(got["d"]) - planted_d(planted, want_d, got["origin"])) < 0.01, (name, got["d"])
    assert abs(float(got["camera_height"]) + float(got["d"])) < 1e-6      # origin = the camera: it sits -d above the plane
    if name in ("tilt 12 -7", "tilt 25 15", "level"):
        assert 2900 <= got["inliers"][2] <= 3100, got["inliers"]


def test_a_room_tilted_past_tilt_cos_finds_the_wall_not_the_floor(fits):
    """the header's stated limit: the dominant plane within tilt_cos of the hint"""
    m, planted, kw, _, got = fits[fr.STEEP[0]]
    assert got["status"] == fr.OK
    wall = fr.tilt_matrix((50.0, 0.0)) @ np.array([0.0, 0.0, 1.0])
    assert angle_deg(got["normal"], planted["normal"]) > 30.0
    assert min(angle_deg(got["normal"], wall), angle_deg(got["normal"], -wall)) < 1.0


def test_the_plane_against_least_squares(fits):
    """Yardstick: an independent f64 np.linalg.lstsq plane over exactly the inliers of the last round.  Measured: at most 0.00216 degrees
    and 0.0806 mm over SCENES (0.0002 degrees and 0.002 mm on the 3000-row floors); allowed four times that."""
    worst_a = worst_h = 0.0
    for name in [s[0] for s in fr.SCENES]:
        m, planted, kw, want_d, got = fits[name]
        # the last round's inliers gave the last plane: refit it independently
        n, off = fr.lstsq_plane(m, got["inlier_rows"])
        if n @ np.asarray(got["normal"], np.float64) < 0:
            n, off = -n, -off
        da = angle_deg(got["normal"], n)
        dh = abs(float(got["d"]) - (off - float(n @ np.asarray(got["origin"], np.float64))))
        print("%-34s angle %.6f deg  height %.6f mm  inliers %d  rms %.4f mm" % (name, da, dh * 1e3, len(got["inlier_rows"]), float(got["rms"][2]) * 1e3))
        worst_a, worst_h = max(worst_a, da), max(worst_h, dh)
    print("worst: %.6f deg %.6f mm" % (worst_a, worst_h * 1e3))
    assert worst_a <= LSTSQ_ANGLE_DEG and worst_h <= LSTSQ_HEIGHT_M, (worst_a, worst_h)


def test_a_permuted_model_gives_the_same_integers_and_bits(fits):
    m, planted, kw, _, want = fits["tilt 25 15"]
    perm = np.random.default_rng(5).permutation(len(m["confidences"]))
    got = fr.fit({k: np.ascontiguousarray(v[perm]) for k, v in m.items()}, len(perm), fr.CAMERA, fr.params(**kw))
    fr.same_fit(got, want, "permuted")
    assert sorted(perm[got["inlier_rows"]].tolist()) == sorted(want["inlier_rows"].tolist())


def test_a_flat_level_floor_has_no_slope_and_the_default_rotation():
    m = fr.flat_floor()
    got = fr.fit(m, 700, np.zeros(3, f32), fr.params())
    assert got["status"] == fr.OK and got["rounds"] == 3 and got["inliers"] == [2000] * 3 + [0] * 5
    assert got["alpha_beta"] == [(0.0, 0.0)] * 3
    assert np.array_equal(got["pose"][:9].view(np.uint32), nr.FLOOR_R.view(np.uint32))
    # the heights are exact, but z is quantised at 2^-10 m against the bin's middle: d ends within half a step of the truth
    assert np.array_equal(got["normal"], np.array([0, -1, 0], f32)) and abs(float(got["d"]) + 1.0) <= 2.0 ** -11 and got["camera_height"] == -got["d"]
    assert not got["rms"].any()
    assert int(got["dir_hist"][15, 15]) == 2000 and int(got["height_hist"].max()) == 2000
    # the grid's origin: on the plane, the camera's foot point in the middle
    q = fr.params()
    assert np.array_equal(got["pose"][9:], np.array([f32(-(q["width"] // 2)) * f32(q["res"]), -got["d"], f32(-(q["height"] // 2)) * f32(q["res"])], f32))


def test_the_statuses():
    m, _ = fr.room(tilt=(12.0, -7.0))
    n = len(m["confidences"])
    none = fr.fit(m, n, fr.CAMERA, fr.params(min_conf=1e9))
    assert none["status"] == fr.NO_FLOOR and none["candidates"] == 0 and none["rows_used"] == 0 and not none["dir_hist"].any()
    assert np.array_equal(none["normal"], np.array([0, -1, 0], f32)) and none["d"] == 0
    walls = dict(m, orientations=m["orientations"].copy())
    walls["orientations"][:, 6:9] = (1, 0, 0)
    none = fr.fit(walls, n, fr.CAMERA, fr.params())
    assert none["status"] == fr.NO_FLOOR and none["candidates"] == 0 and none["rows_used"] == n
    few = fr.fit(m, n, fr.CAMERA, fr.params(min_rows=100000))
    assert few["status"] == fr.NO_FLOOR and few["candidates"] > 0 and few["aligned"] > 0 and few["height_rows"] == 0 and few["rounds"] == 0
    # a floor that the first round finds and the second loses: fewer than min_rows within a tiny inlier distance
    lost = fr.fit(m, n, fr.CAMERA, fr.params(min_rows=1500, inlier_dist=1e-4))
    assert lost["status"] == fr.NO_FLOOR and lost["rounds"] == 1 and lost["inliers"][0] >= 1500 > lost["inliers"][1] > 0
    # collinear rows
    line = fr.flat_floor(200)
    line["positions"][:, 2] = 0.5
    deg = fr.fit(line, 200, np.zeros(3, f32), fr.params())
    assert deg["status"] == fr.DEGENERATE and deg["rounds"] == 0 and deg["inliers"][0] == 200
    assert np.array_equal(deg["normal"], np.array([0, -1, 0], f32)) and deg["d"] == fr.height_of_bin(deg["height_bin"], 0.02)


# every parameter off its default, with the scene on which that changes an integer of the result: tests/test_navfloor_gpu.py runs these rows
PARAMETER_ROWS = (
    ("tilt 25 15", dict(up=(0.3, -1.0, 0.2))), ("tilt 25 15", dict(origin=(0.5, -0.25, 1.0))), ("tilt 25 15", dict(tilt_cos=0.9)),
    ("tilt 25 15", dict(align_cos=0.999)), ("tilt 25 15", dict(height_res=0.05)), ("tilt 12 -7", dict(min_rows=100000)),
    ("the table wins", dict(floor_share256=26)), ("tilt 25 15", dict(refine_iters=1)), ("tilt 25 15", dict(first_dist=0.01)),
    ("tilt 25 15", dict(inlier_dist=0.004)), ("tilt 25 15", dict(min_conf=2.5)), ("tilt 25 15", dict(t_init=(41, 50))),
    ("tilt 25 15", dict(t_last=(0, 59))), ("tilt 25 15", dict(visible_only=True)),
)
# ... and those that only reach the pose and the bands
POSE_ROWS = (dict(width=300), dict(height=200), dict(res=0.1), dict(below=0.25), dict(step=0.1), dict(body_height=2.0))


def integers_of(fit):
    return [fit[k] if not isinstance(fit[k], np.ndarray) else fit[k].tolist() for k in fr.INTEGERS]


@pytest.mark.parametrize("name,kw", PARAMETER_ROWS)
def test_every_parameter_off_its_default_changes_an_integer(name, kw, fits):
    m, planted, base_kw, _, base = fits[name]
    got = fr.fit(m, len(m["confidences"]) // 2, fr.CAMERA, fr.params(**dict(base_kw, **kw)))
    assert integers_of(got) != integers_of(base), (name, kw)


def test_the_rows_name_every_parameter():
    named = set().union(*[set(kw) for _, kw in PARAMETER_ROWS], *[set(kw) for kw in POSE_ROWS])
    assert named == set(fr.DEFAULTS)


@pytest.mark.parametrize("kw", POSE_ROWS)
def test_the_grids_parameters_reach_the_pose_or_the_bands(kw, fits):
    m, planted, base_kw, _, base = fits["tilt 25 15"]
    got = fr.fit(m, len(m["confidences"]) // 2, fr.CAMERA, fr.params(**kw))
    changed = [k for k in ("pose", "z_min", "floor_max", "z_max", "width", "height", "res")
               if not np.array_equal(np.asarray(got[k], f32).view(np.uint32), np.asarray(base[k], f32).view(np.uint32))]
    assert changed, kw


# ---- the host steps as the library compiles them ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def solve_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("navfloor") / "navfloor_solve_check")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "supersurfel_fusion_amd", "csrc"),
                        os.path.join(ROOT, "tests", "cpp", "navfloor_solve_check.cpp"), "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    return exe


def run_check(exe, text):
    r = subprocess.run([exe], input=text, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    return [line.split() for line in r.stdout.splitlines()]


def bits(v):
    return ["%08x" % int(x) for x in np.asarray(v, f32).ravel().view(np.uint32)]


def test_the_compiled_solve_equals_the_restatement_on_records_at_the_bounds(solve_check):
    """random ten-word records at the bounds' magnitudes (sums near 2^60, N = 3 and N = 2^22): the __int128 -> double conversion and the
    operation order of a round, with =="""
    rng = np.random.default_rng(17)
    a, b = fr.hint_frame(fr.unit_up((0.1, -1.0, 0.05)))
    n = fr.unit_up((0.1, -1.0, 0.05))
    lines, wants = [], []
    for case in range(400):
        N = (3, 1 << 22, int(rng.integers(3, 1 << 22)))[case % 3]
        big = case % 4 != 0
        mag = (1 << 19) if big else 2000
        # moments of N points with coordinates of magnitude `mag`: means, then second moments at least the means' squares (or not: det <= 0)
        mx, my, mz = (int(v) for v in rng.integers(-mag, mag, 3))
        Sx, Sy, Sz = N * mx + int(rng.integers(-N, N)), N * my + int(rng.integers(-N, N)), N * mz + int(rng.integers(-N, N))
        vx, vy, vz = (int(v) for v in rng.integers(1, mag * mag // 4, 3))
        cxy, cxz, cyz = (int(v) for v in rng.integers(-mag * mag // 16, mag * mag // 16, 3))
        if case % 7 == 0:
            cxy = vx = vy                                             # singular
        s = [N, Sx, Sy, Sz, N * (mx * mx + vx), N * (mx * my + cxy), N * (my * my + vy), N * (mx * mz + cxz), N * (my * mz + cyz), N * (mz * mz + vz)]
        assert all(abs(v) < 1 << 62 for v in s)
        d = f32(rng.uniform(-2, 2))
        lines.append("round %d %s %s %s %s %s" % (3, " ".join(str(v) for v in s), " ".join(bits(n)), " ".join(bits(a)), " ".join(bits(b)), bits(d)[0]))
        status, n_new, d_new, rms, _ = fr.refine_round(s, 3, n, a, b, d)
        wants.append([str(status)] + (bits(n_new) + bits(d_new) + bits(rms) if status == fr.OK else []))
    got = run_check(solve_check, "\n".join(lines) + "\n")
    assert len(got) == len(wants)
    assert sum(1 for w in wants if w[0] == "0") > 200 and sum(1 for w in wants if w[0] == "2") > 20
    for k, (g, w) in enumerate(zip(got, wants)):
        assert g == w, (k, lines[k], g, w)


def test_the_compiled_winners_frames_and_poses_equal_the_restatement(solve_check):
    rng = np.random.default_rng(23)
    lines, wants = [], []
    for case in range(40):
        hist = np.zeros(fr.DIR_BINS * fr.DIR_BINS, np.uint32)
        if case:
            at = rng.integers(0, len(hist), 1 + case % 5 * 40)
            np.add.at(hist, at, rng.integers(1, 3 if case % 2 else 1000, len(at)).astype(np.uint32))
        if case == 1:
            hist[:] = 0; hist[0] = hist[30] = hist[960] = 5            # ties at the corners: the smallest index
        lines.append("dir " + " ".join(str(v) for v in hist))
        w = fr.direction_winner(hist)
        wants.append(["none"] if w is None else [str(v) for v in w])
    for case in range(40):
        hist = np.zeros(fr.HEIGHT_BINS, np.uint32)
        for _ in range(case % 4 + 1):
            c = int(rng.integers(0, fr.HEIGHT_BINS))
            lo, hi = max(0, c - 3), min(fr.HEIGHT_BINS, c + 4)
            hist[lo:hi] += rng.integers(0, 2000, hi - lo).astype(np.uint32)
        if case == 0:
            hist[:] = 0; hist[0] = 100; hist[2047] = 100
        min_rows, share = int(rng.integers(3, 400)), int(rng.integers(1, 257))
        lines.append("height %d %d " % (min_rows, share) + " ".join(str(v) for v in hist))
        w = fr.height_winner(hist, min_rows, share)
        wants.append(["none"] if w is None else [str(w[0]), str(w[1]), bits(fr.height_of_bin(w[0], 0.02))[0]])
    for case in range(60):
        up = rng.normal(size=3).astype(f32) if case else np.array([0, -1, 0], f32)
        if case in (1, 2, 3):
            up = np.eye(3, dtype=f32)[case - 1] * f32(-2.5)
        u = fr.unit_up(up)
        a, b = fr.hint_frame(u)
        nrm = fr.unit_up(u + rng.normal(0, 0.2, 3).astype(f32))
        S = [int(v) for v in rng.integers(-1 << 40, 1 << 40, 3)]
        n0 = fr.direction_normal(S)
        d, o, pc = f32(rng.uniform(-2, 2)), rng.uniform(-50, 50, 3).astype(f32), rng.uniform(-3, 3, 3).astype(f32)
        W, H, res = int(rng.integers(1, 4097)), int(rng.integers(1, 4097)), f32(rng.choice([0.05, 0.1, 0.03]))
        lines.append("pose %s %s %s %s %s %d %d %s %d %d %d %s" % (" ".join(bits(up)), " ".join(bits(nrm)), bits(d)[0], " ".join(bits(o)), " ".join(bits(pc)), W, H,
                                                              bits(res)[0], S[0], S[1], S[2], bits(f32(0.8))[0]))
        wants.append(bits(u) + bits(a) + bits(b) + bits(n0) + bits(fr.vote_scale(0.8)) + bits(fr.camera_height(pc, nrm, d)) + bits(fr.grid_pose(nrm, d, o, pc, a, b, W, H, res)))
    got = run_check(solve_check, "\n".join(lines) + "\n")
    assert len(got) == len(wants)
    for k, (g, w) in enumerate(zip(got, wants)):
        assert g == w, (k, lines[k][:80], g, w)
