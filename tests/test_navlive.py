"""The live obstacle layer (include/ssf_navlive.h) without a GPU: who exports the entry points, the header on its own, the struct
layouts of the binding, the C++ surface, replay.py's options, and the restatement the GPU tests compare against
(tests/navlive_ref.py): hand cases with known answers, and a guard that no parametrised scene of the GPU file is vacuous."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import navgrid_ref as nr
import navlive_ref as lr
from conftest import ROOT
from supersurfel_fusion_amd import binding, replay

INCLUDE = os.path.join(ROOT, "include")
CPP = os.path.join(ROOT, "tests", "cpp")


def exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], stdout=subprocess.PIPE, text=True, check=True).stdout
    return {l.split()[-1] for l in out.splitlines() if l.strip()}


# ---- static checks -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def live_lib(product_lib):
    return binding.load_live()


def test_the_live_library_exports_the_overlay_and_all_of_the_drive_library(live_lib, product_lib, oracle_lib):
    """libssf_hip_live.so = libssf_hip_drive.so's objects + ssf_navlive.hip; the five older tables and the oracle hold no name of it"""
    have, drive = exported(live_lib.path), exported(binding.DRIVE_LIB)
    hip_ids = lambda names: {nm for nm in names if nm.startswith("__hip_cuid_")}         # one per translation unit, named by content
    for names in (binding.NAVLIVE_SYMBOLS, binding.NAVPATH_SYMBOLS, binding.NAVFRONTIER_SYMBOLS, binding.NAVPLAN_SYMBOLS, binding.NAVCARVE_SYMBOLS,
                  binding.ABI_SYMBOLS):
        assert set(names) <= have
    assert live_lib.has_navlive and live_lib.has_navpath and live_lib.has_navfrontier and live_lib.has_navplan and live_lib.has_navcarve
    assert live_lib.has_navgrid and live_lib.has_motion and live_lib.backend == "hip-gfx950"
    assert drive - hip_ids(drive) <= have
    extra = have - drive - hip_ids(have)
    assert set(binding.NAVLIVE_SYMBOLS) <= extra
    kernels = extra - set(binding.NAVLIVE_SYMBOLS)
    assert kernels == {nm for nm in extra if "k_navlive_" in nm}, sorted(extra)
    assert all(any(k in nm for nm in kernels) for k in ("k_navlive_stamp", "k_navlive_march", "k_navlive_cells"))
    for other in (exported(product_lib.path), exported(binding.NAVCARVE_LIB), exported(binding.NAV_LIB), exported(binding.EXPLORE_LIB), drive,
                  exported(oracle_lib.path)):
        assert not [nm for nm in other if "navlive" in nm]
    for load in ("load_navcarve", "load_nav", "load_explore", "load_drive"):
        assert not getattr(binding, load)().has_navlive
    assert not product_lib.has_navlive and not oracle_lib.has_navlive


def test_an_oracle_backed_fusion_names_the_missing_symbol(oracle_lib):
    f = binding.Fusion(oracle_lib, oracle_lib.default_config(width=64, height=48, fx=60.0, fy=60.0, cx=31.5, cy=23.5))
    depth, state = np.ones((48, 64), np.float32), np.zeros((3, 3), np.int8)
    for call, symbol in ((lambda: f.nav_live(depth, state), "ssf_navlive_overlay"),
                         (lambda: f.nav_live_device(None, None, 3, 3), "ssf_navlive_overlay"),
                         (lambda: f.nav_live_plan(depth, state, [(1, 1)], [(0, 0)]), "ssf_navlive_overlay"),
                         (f.nav_live_default_params, "ssf_navlive_default_params")):
        with pytest.raises(binding.SsfError, match=symbol + ".*binding.load_live"):
            call()


@pytest.mark.parametrize("load", ["load_product", "load_nav", "load_drive"])
def test_an_older_library_names_the_overlay_symbol(load, product_lib):
    """the older libraries overlay no frame: the calls say which symbol is missing before anything runs"""
    lib = getattr(binding, load)()
    assert not lib.has_navlive
    f = binding.Fusion.__new__(binding.Fusion)                            # (no handle: the check comes before any call)
    f.L = lib
    depth, state = np.ones((48, 64), np.float32), np.zeros((3, 3), np.int8)
    with pytest.raises(binding.SsfError, match="ssf_navlive_overlay.*binding.load_live"):
        f.nav_live(depth, state)
    with pytest.raises(binding.SsfError, match="ssf_navlive_default_params"):
        f.nav_live_default_params()
    with pytest.raises(binding.SsfError, match="ssf_navlive_overlay"):
        f.nav_live_plan(depth, state, [(1, 1)], [(0, 0)], waypoints=True)


def test_the_overlay_symbols_stay_out_of_the_other_headers():
    for nm in binding.NAVLIVE_SYMBOLS:
        assert nm not in binding.ABI_SYMBOLS
        for hdr in ("ssf.h", "ssf_testing.h", "ssf_navgrid.h", "ssf_navcarve.h", "ssf_navplan.h", "ssf_navfrontier.h", "ssf_navpath.h", "ssf_motion.h"):
            assert nm not in open(os.path.join(INCLUDE, hdr)).read(), (nm, hdr)
        assert nm + "(" in open(os.path.join(INCLUDE, "ssf_navlive.h")).read()
    assert "#define SSF_ABI_VERSION 3" in open(os.path.join(INCLUDE, "ssf.h")).read()


@pytest.mark.parametrize("lang", ["c", "c++"])
def test_the_header_compiles_on_its_own(lang, tmp_path):
    src = tmp_path / ("t.c" if lang == "c" else "t.cpp")
    src.write_text('#include "ssf_navlive.h"\n'
                   "int f(ssf_handle* h, const float* depth, const uint8_t* mask, int8_t* state, int32_t* dist2, const float* grid_pose) {\n"
                   "    ssf_navlive_params p; ssf_navlive_stats s; ssf_navlive_out o;\n"
                   "    if (ssf_navlive_default_params(h, &p) != SSF_OK) return -1;\n"
                   "    p.grid_pose = grid_pose; p.width = 64; p.height = 48; p.mask_mode = 2; p.min_hits = 2; p.stride = 8;\n"
                   "    o.live_hits = 0; o.live_seen = 0; o.state = state; o.dist2 = dist2;\n"
                   "    if (ssf_navlive_overlay(h, &p, depth, mask, state, &o, &s) != SSF_OK) return -2;\n"
                   "    return (int)(s.cells_stamped + s.cells_opened + s.atomics) + (int)s.pose[9]; }\n")
    cc, std = ("gcc", "-std=c99") if lang == "c" else ("g++", "-std=c++11")
    r = subprocess.run([cc, std, "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", INCLUDE, "-c", str(src), "-o", str(tmp_path / "t.o")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout


def test_the_binding_structs_have_the_headers_layout(tmp_path):
    classes = (("ssf_navlive_params", binding.SsfNavLiveParams), ("ssf_navlive_out", binding.SsfNavLiveOut), ("ssf_navlive_stats", binding.SsfNavLiveStats))
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "ssf_navlive.h"', "int main(void) {"]
    for st, cls in classes:
        lines.append('    printf("%s %%zu\\n", sizeof(%s));' % (st, st))
        for nm, _ in cls._fields_:
            lines.append('    printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (st, nm, st, nm))
    lines += ["    return 0; }"]
    src = tmp_path / "off.c"
    src.write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "off")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", INCLUDE, str(src), "-o", exe], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    got = dict(l.split() for l in subprocess.run([exe], stdout=subprocess.PIPE, text=True, check=True).stdout.splitlines())
    for st, cls in classes:
        assert int(got[st]) == C.sizeof(cls), st
        for nm, _ in cls._fields_:
            assert int(got["%s.%s" % (st, nm)]) == getattr(cls, nm).offset, (st, nm)
    assert tuple(nm for nm, _ in binding.SsfNavLiveStats._fields_) == lr.STATS + ("atomics", "pose")
    assert tuple(nm for nm, _ in binding.SsfNavLiveOut._fields_) == binding.NAVLIVE_OUTPUT_NAMES == lr.OUTPUTS
    fields = [nm for nm, _ in binding.SsfNavLiveParams._fields_ if nm not in ("grid_pose", "cam_pose", "on_device", "frame_on_device")]
    assert fields == [nm for nm in lr.DEFAULTS if nm not in ("range_min", "range_max", "cfg_camera", "march")]


def test_ssf_hpp_overlay_members_compile_and_link_against_the_live_library(live_lib, tmp_path):
    libdir = os.path.dirname(live_lib.path)
    cmd = ["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", "-I", INCLUDE, "-I", CPP, os.path.join(CPP, "navlive_smoke.cpp"),
           "-o", str(tmp_path / "navlive_smoke"), "-L", libdir, "-lssf_hip_live", "-Wl,-rpath," + libdir]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout


def test_the_replay_options_parse():
    base = ["--npz", "frames.npz", "--nav-grid-dir", "grids"]
    assert replay.nav_live_of(replay.parse_args(base + ["--nav-live"])) == dict(min_hits=4, stride=4)
    a = replay.parse_args(base + ["--nav-live", "--nav-live-min-hits", "2", "--nav-live-stride", "8", "--nav-grid-carve"])
    assert replay.nav_live_of(a) == dict(min_hits=2, stride=8) and a.nav_grid_carve
    assert replay.nav_live_of(replay.parse_args(base)) is None
    for bad in (["--nav-live-min-hits", "2"], ["--nav-live-stride", "8"], ["--nav-live", "--nav-live-min-hits", "0"], ["--nav-live", "--nav-live-stride", "0"],
                ["--nav-live", "--nav-live-stride", "65"]):
        with pytest.raises(SystemExit):
            replay.parse_args(base + bad)
    with pytest.raises(SystemExit):                                      # without a grid directory there is nothing to stamp onto
        replay.parse_args(["--npz", "frames.npz", "--nav-live"])
    with pytest.raises(ValueError, match="nav_live needs nav_grid_dir"):
        replay.replay(None, [], nav_live=dict(min_hits=4, stride=4))


def test_the_restatements_defaults_are_the_headers():
    hdr = open(os.path.join(INCLUDE, "ssf_navlive.h")).read()
    for text in ("min_hits 4 (a speck filter", "stride 4, hit_margin_cells 1, min_seen 1, open_unknown 1, mask_mode 0", "design choices, not tuned values",
                 "width, height, res, floor_max, z_max and max_dist_cells are those of ssf_navgrid_default_params", "tt = d * l (one multiplication)",
                 "it is stateless", "a pixel stamps a POINT, not a footprint", "occupied cells are never cleared by live evidence"):
        assert text in hdr, text
    d = lr.DEFAULTS
    assert (d["min_hits"], d["stride"], d["hit_margin_cells"], d["min_seen"], d["open_unknown"], d["mask_mode"]) == (4, 4, 1.0, 1, True, 0)
    for key in ("width", "height", "res", "floor_max", "z_max", "max_dist_cells", "unknown_is_obstacle"):
        assert d[key] == nr.DEFAULTS[key], key


# ---- hand cases of the restatement ---------------------------------------------------------------------------------------------
WALL = dict(lr.CAMERA, width=33, height=31, res=0.05, max_dist_cells=6)
WALL_POSE = lr.room_pose(at=(0.8, 0.0, 0.225))                        # identity rotation: the optical axis is map z = grid y
WALL_ROW = 24                                                      # depth 1 from z = 0.225: grid y = 1.225, cell row 24


def wall(depth=1.0, state_in=None, mask=None, **kw):
    c = lr.params(**dict(WALL, **kw))
    d = np.full((128, 160), depth, np.float32)
    s = np.full((31, 33), -1, np.int8) if state_in is None else state_in
    return lr.overlay(d, mask, s, lr.grid_pose_at(), WALL_POSE, c)


def test_a_fronto_parallel_wall_is_one_row_of_cells_and_opens_the_cells_in_front_of_it():
    got = wall()
    s = got["stats"]
    occ = got["state"] == 100
    assert occ[WALL_ROW].sum() >= 20 and not occ[:WALL_ROW].any() and not occ[WALL_ROW + 1:].any()
    xs = np.flatnonzero(occ[WALL_ROW])
    assert (np.diff(xs) == 1).all() and xs[0] <= 6 and xs[-1] >= 26       # x = 0.8 -+ 0.53 m: one unbroken run
    assert s["pixels_valid"] == s["pixels_stamping"] == s["points_in_band"] == 160 * 128 == got["live_hits"].sum()
    assert (got["live_hits"][~occ] == 0).all() and s["cells_stamped"] == occ.sum() == s["cells_occupied"]
    opened = got["state"] == 0
    assert s["cells_opened"] == opened.sum() > 100 and not opened[WALL_ROW:].any()
    assert not (got["live_seen"][WALL_ROW + 1:] > 0).any()                 # none beyond the wall
    assert opened[5:WALL_ROW - 1, 16].all()                                # the column in front of the camera (x = 0.8: cell 16), up to the margin
    assert got["live_seen"][4, 16] == s["rays"] == s["rays_carving"] == 40 * 32          # every ray starts in the camera's cell (0.8, 0.225)
    assert s["ray_entries"] == got["live_seen"].sum() and (got["dist2"][occ] == 0).all() and got["dist2"][4, 16] == 36


def test_a_masked_box_under_the_three_mask_modes():
    mask = np.zeros((128, 160), np.uint8)
    mask[:, 50:100] = 7                                                  # whole pixel columns: the cells under them lose every point
    all_, only, rest = wall(), wall(mask=mask, mask_mode=1), wall(mask=mask, mask_mode=2)
    assert only["stats"]["pixels_stamping"] == 128 * 50 and rest["stats"]["pixels_stamping"] == 160 * 128 - 128 * 50
    assert (all_["live_hits"] == only["live_hits"] + rest["live_hits"]).all() and only["live_hits"].sum() == 128 * 50
    assert 0 < only["stats"]["cells_stamped"] < all_["stats"]["cells_stamped"]
    for got in (only, rest):                                             # the mask is not consulted by the rays
        assert (got["live_seen"] == all_["live_seen"]).all() and got["stats"]["pixels_valid"] == 160 * 128
    # the cells the box no longer occupies are seen through up to the margin only: they stay unknown, never free
    gone = (all_["state"] == 100) & (rest["state"] != 100)
    assert gone.any() and (rest["state"][gone] == -1).all()


def test_occupied_is_never_opened():
    got = wall(state_in=np.full((31, 33), 100, np.int8))
    assert (got["state"] == 100).all() and got["stats"]["cells_opened"] == 0 == got["stats"]["cells_stamped"] and got["live_seen"].sum() > 0
    s = np.full((31, 33), -1, np.int8)
    s[10, 16] = 100
    s[12, 16] = 0
    got = wall(state_in=s)
    assert got["live_seen"][10, 16] > 0 and got["state"][10, 16] == 100 and got["state"][12, 16] == 0 and got["state"][11, 16] == 0
    assert got["stats"]["cells_opened"] == (got["state"] == 0).sum() - 1
    closed = wall(state_in=s, open_unknown=False)
    assert closed["stats"]["cells_opened"] == 0 and (closed["state"] == 0).sum() == 1 and (closed["live_seen"] == got["live_seen"]).all()
    skipped = wall(state_in=s, open_unknown=False, march=False)           # nothing asks for the march: it is skipped
    assert skipped["live_seen"].sum() == 0 and skipped["stats"]["rays"] == 0 and (skipped["state"] == closed["state"]).all()


def test_min_hits_is_a_threshold():
    base = wall()
    n = int(base["live_hits"][WALL_ROW].max())
    iy, ix = WALL_ROW, int(base["live_hits"][WALL_ROW].argmax())
    assert n > 64
    assert wall(min_hits=n - 1)["state"][iy, ix] == 100 and wall(min_hits=n)["state"][iy, ix] == 100
    over = wall(min_hits=n + 1)
    assert over["state"][iy, ix] == -1 and over["stats"]["cells_stamped"] == 0 and (over["live_hits"] == base["live_hits"]).all()


def test_no_valid_pixel_is_the_identity():
    state_in = lr.state_pattern(33, 31, 9)
    want = np.where(state_in == 100, 100, np.where(state_in == 0, 0, -1)).astype(np.int8)
    assert ((state_in != want).sum() > 5)                                 # foreign values are in the pattern
    for depth in (0.0, np.nan, np.inf, -1.0, 0.19, 5.5):
        for unknown in (False, True):
            got = wall(depth=depth, state_in=state_in, unknown_is_obstacle=unknown)
            assert (got["state"] == want).all() and got["live_hits"].sum() == 0 == got["live_seen"].sum()
            assert (got["dist2"] == nr.clearance(want, 6, unknown)).all()
            s = got["stats"]
            assert s["pixels_valid"] == s["rays"] == s["cells_stamped"] == s["cells_opened"] == 0


def test_the_output_fed_back_is_a_fixed_point():
    for scene, fmt, stride in lr.GPU_CASES[:3]:
        i = lr.case_inputs(scene, fmt, stride)
        first = lr.case_reference(scene, fmt, stride)
        again = lr.overlay(i["depth"], None, first["state"], i["grid_pose"], i["cam_pose"], i["c"], fmt, i["depth_scale"])
        assert (again["state"] == first["state"]).all() and (again["dist2"] == first["dist2"]).all()
        assert again["stats"]["cells_stamped"] == 0 == again["stats"]["cells_opened"]


def test_the_boundary_cases_have_their_hand_written_answers():
    for name, d, at, kw, want in lr.boundary_cases():
        c = lr.params(**dict(lr.BOUNDARY, **kw))
        got = lr.overlay(np.full((1, 1), d, np.float32), None, np.full((4, 8), -1, np.int8), nr.IDENTITY, lr.boundary_pose(*at), c)
        lr.check_expectations(got, want, 8, 4, name)


def test_the_corner_bound_is_what_the_header_says():
    c = lr.params(**dict(lr.BOUNDARY, t_max=4.0))
    assert lr.corner_bound(c) == 32.0                                    # one pixel on the axis: l = 1, 4 / 0.125
    c = lr.params(**dict(WALL, t_max=1000.0))
    assert lr.corner_bound(c) > 40000 and lr.corner_bound(dict(c, t_max=1500.0)) > 65535


# ---- the guard against vacuous GPU tests -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene,fmt,stride", lr.GPU_CASES, ids=["%s-%s-stride%d" % c for c in lr.GPU_CASES])
def test_no_scene_of_the_gpu_file_is_vacuous(scene, fmt, stride):
    i = lr.case_inputs(scene, fmt, stride)
    got = lr.case_reference(scene, fmt, stride)
    s = got["stats"]
    d = lr.metres(i["depth"], fmt, i["depth_scale"])
    assert s["cells_stamped"] > 0 and s["cells_opened"] > 0, s
    assert int((~lr.valid_pixels(d, i["c"])).sum()) > 0
    assert int(got["live_hits"].max()) >= 64                             # contention inside a wave
    assert s["rays_carving"] > 0 and s["ray_entries"] > s["rays_carving"] and 0 < s["points_in_band"] <= s["pixels_stamping"]
    assert set(np.unique(i["state_in"])) - {-1, 0, 100}                  # foreign values of state_in are exercised


# ---- the guards of the parameter space, the masks and the round-edge rays of the GPU file ------------------------------------------
def changes(ref, unchanged, ids, rows_arrays, row, fmt):
    """the governed arrays of a row against the base case: all differ, or -- a row listed as unchanged -- none does"""
    base, got = ref(fmt, None), ref(fmt, row)
    differ = [bool((got[a] != base[a]).any()) for a in rows_arrays[row]]
    print(ids[row], fmt, {a: int((got[a] != base[a]).sum()) for a in rows_arrays[row]})
    if (ids[row], fmt) in unchanged:
        assert not any(differ), (ids[row], fmt, "is listed as a row that changes nothing")
    else:
        assert all(differ), (ids[row], fmt, "repeats the base case", rows_arrays[row], differ)


def substitutes(unchanged, ids, overrides, changed):
    """every row listed as unchanged names a row, and another row of the same parameter changes its array in that format"""
    for name, fmt in unchanged:
        over = overrides[ids.index(name)]
        others = [k for k, o in enumerate(overrides) if set(o) == set(over) and (ids[k], fmt) not in unchanged]
        assert others and all(changed(k, fmt) for k in others), (name, fmt)


@pytest.mark.parametrize("fmt", lr.PARAM_FORMATS)
@pytest.mark.parametrize("row", range(len(lr.PARAM_ROWS)), ids=lr.PARAM_IDS)
def test_every_row_of_the_parameter_space_changes_its_arrays(row, fmt):
    changes(lr.param_reference, lr.PARAM_UNCHANGED, lr.PARAM_IDS, [r[1] for r in lr.PARAM_ROWS], row, fmt)


def test_the_parameter_space_is_the_one_that_was_asked_for():
    over = [r[0] for r in lr.PARAM_ROWS]
    assert [o["hit_margin_cells"] for o in over if set(o) == {"hit_margin_cells"}] == [0.0, 0.37, 2.5, 40.0]
    assert [o["min_seen"] for o in over if set(o) == {"min_seen"}] == [2, 9] and [o["min_hits"] for o in over if set(o) == {"min_hits"}] == [1, 64]
    assert [o["max_dist_cells"] for o in over if set(o) == {"max_dist_cells"}] == [1, 40] and [o["stride"] for o in over if set(o) == {"stride"}] == [3, 7, 64]
    for o in (dict(open_unknown=0), dict(unknown_is_obstacle=1), dict(t_min=0.9, t_max=1.4), dict(floor_max=-0.3, z_max=0.1),
              dict(open_unknown=0, unknown_is_obstacle=1, hit_margin_cells=0.0), dict(min_hits=64, min_seen=9, stride=7)):
        assert o in over, o
    assert (lr.PARAM_SCENE, lr.PARAM_STRIDE, lr.PARAM_FORMATS) == ("room rolled", 4, ("f32", "u16"))
    assert all(160 % s or 128 % s for s in (3, 7, 64))                   # every stride of the rows leaves a remainder in the lattice
    changed = lambda k, fmt: all((lr.param_reference(fmt, k)[a] != lr.param_reference(fmt, None)[a]).any() for a in lr.PARAM_ROWS[k][1])
    substitutes(lr.PARAM_UNCHANGED, lr.PARAM_IDS, over, changed)
    # what the base case's cell rule sees: cells on both sides of min_seen 2 and 9, and of min_hits 64
    base = lr.param_reference("f32", None)
    assert ((base["live_seen"] >= 1) & (base["live_seen"] < 9)).any() and (base["live_seen"] >= 9).any() and (base["live_hits"] >= 64).any()
    # a margin of 40 cells is longer than every ray: none carves, and every pixel still counts as a ray
    far = lr.param_reference("f32", lr.PARAM_IDS.index("hit_margin_cells=40.0"))["stats"]
    assert far["rays_carving"] == 0 == far["ray_entries"] and far["rays"] == base["stats"]["rays"] > 0
    # margin 0: rays reach the cells their own pixels stamp
    zero = lr.param_reference("f32", lr.PARAM_IDS.index("hit_margin_cells=0.0"))
    stamped = base["live_hits"] >= 4
    assert (zero["live_hits"] == base["live_hits"]).all() and zero["live_seen"][stamped].sum() > base["live_seen"][stamped].sum() > 0


@pytest.mark.parametrize("fmt", ["f32", "u16"])
def test_the_mask_of_the_small_image_splits_its_pixels(fmt):
    i = lr.small_inputs(fmt)
    assert (i["depth"].shape, i["mask"].shape, i["state_in"].shape) == ((29, 37), (29, 37), (33, 31)) and set(np.unique(i["mask"])) == {0, 200}
    assert 37 % 16 and 29 % 16 and 37 % 3 and 29 % 3                     # partial pixel tiles and a remainder in the lattice, both ways
    run = lambda mode: lr.overlay(i["depth"], i["mask"], i["state_in"], i["grid_pose"], i["cam_pose"], lr.params(**dict(i["kw"], mask_mode=mode)),
                                  fmt, i["depth_scale"])
    all_, only, rest = run(0), run(1), run(2)
    for got in (only, rest):
        s = got["stats"]
        assert 0 < s["pixels_stamping"] < s["pixels_valid"] and s["cells_stamped"] > 0 and 0 < s["points_in_band"] < all_["stats"]["points_in_band"]
    assert only["stats"]["pixels_stamping"] + rest["stats"]["pixels_stamping"] == all_["stats"]["pixels_valid"] == (834 if fmt == "f32" else 835)
    print(fmt, only["stats"], rest["stats"])
    assert (only["stats"]["pixels_stamping"], rest["stats"]["pixels_stamping"]) == ((413, 421) if fmt == "f32" else (414, 421))
    assert (only["state"] != rest["state"]).any() and (only["live_seen"] == rest["live_seen"]).all()


def test_the_mask_modes_differ_on_the_large_image():
    i = lr.case_inputs(lr.PARAM_SCENE, "f32", 8)
    mask = lr.modes_mask()
    assert set(np.unique(mask)) == {0, 1, 3} and (mask[:, 60:100] == 1).all() and 0.3 < (mask[:, :60] != 0).mean() < 0.5
    got = [lr.overlay(i["depth"], mask, i["state_in"], i["grid_pose"], i["cam_pose"], lr.params(**dict(i["kw"], mask_mode=m))) for m in (0, 1, 2)]
    assert all((a["live_hits"] != b["live_hits"]).any() for a, b in ((got[0], got[1]), (got[0], got[2]), (got[1], got[2])))


@pytest.mark.parametrize("tilt", lr.EDGE_TILTS)
def test_the_round_edge_rays_end_on_both_sides_of_a_round(tilt):
    i = lr.edge_inputs(tilt)
    c = lr.params(**i["kw"])
    run = lambda d, i: lr.overlay(d, None, i["state_in"], i["grid_pose"], i["cam_pose"], c)
    s = run(i["depth"], i)["stats"]
    nu, nv = 64 // c["stride"], 2 // c["stride"]
    assert (nu * nv, nu * nv // 16) == (128, 8)                           # eight waves of sixteen rays
    assert (s["pixels_valid"], s["rays"], s["rays_carving"], s["ray_samples"]) == (126, 126, 126, 12167)
    n = lr.edge_ray_counts(tilt, lambda d, i: run(d, i)["stats"])
    assert n.sum() == s["ray_samples"] and [(v, u) for v, u in np.argwhere(n == 0)] == list(lr.EDGE_INVALID)
    assert set(n[0]) - {0} == set(range(49, 81)) and set(n[1]) - {0} == set(range(113, 145))
    for count in lr.EDGE_COUNTS:
        assert (n == count).any(), count
    # a wave's sixteen consecutive rays have eight or nine counts; a round ends between two waves (pixels 31 | 32 of either row)
    waves = [set(n.ravel()[k:k + 16]) for k in range(0, 128, 16)]
    assert all(len(w) >= 8 for w in waves) and 64 in waves[1] and 65 in waves[2] and 128 in waves[5] and 129 in waves[6]
    assert s["ray_entries"] > 6000 and s["cells_opened"] > 100 and s["cells_stamped"] > 30


@pytest.mark.parametrize("tilt", lr.EDGE_TILTS)
def test_the_shifted_round_edge_rays_end_a_round_inside_a_wave(tilt):
    i = lr.edge_inputs(tilt, 8)
    c = lr.params(**i["kw"])
    run = lambda d, i: lr.overlay(d, None, i["state_in"], i["grid_pose"], i["cam_pose"], c)
    s = run(i["depth"], i)["stats"]
    n = lr.edge_ray_counts(tilt, lambda d, i: run(d, i)["stats"], 8)
    assert (s["rays_carving"], s["ray_samples"]) == (126, n.sum()) and float(np.nanmax(i["depth"])) < c["t_max"]
    waves = [set(n.ravel()[k:k + 16]) for k in range(0, 128, 16)]
    assert {64, 65} <= waves[1] and {128, 129} <= waves[5] and lr.EDGE_SHIFTS == (0, 8)
