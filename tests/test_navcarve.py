"""The carved navigation grid (include/ssf_navcarve.h) without a GPU: who exports the entry points, the header on its own, the
struct layouts of the binding, the C++ surface, replay.py's options, and the numpy restatement the GPU tests compare against
(tests/navcarve_ref.py): the wall scene, hand-written boundary answers, an f64 formulation of its rays, extents and samples, and
the identity without views."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import navcarve_ref as nc
import navgrid_ref as nr
import raycast_ref as rr
from conftest import ROOT
from supersurfel_fusion_amd import binding, replay

INCLUDE = os.path.join(ROOT, "include")
CPP = os.path.join(ROOT, "tests", "cpp")
f32 = np.float32
CFG_CAMERA = dict(fx=150.0, fy=150.0, cx=79.5, cy=63.5, width=160, height=128)


def exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], stdout=subprocess.PIPE, text=True, check=True).stdout
    return {l.split()[-1] for l in out.splitlines() if l.strip()}


# ---- static checks -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def carve_lib():
    return binding.load_navcarve()


def test_the_carve_library_exports_the_carve_and_all_of_the_product(carve_lib, product_lib, oracle_lib):
    """libssf_hip_navcarve.so = the product's objects + ssf_navcarve.hip: its exports are the product's plus the carve's entry points
    and kernels; the product library's own table stays what it was (tests/test_math.py pins it), and the checker has none of it"""
    have, product = exported(carve_lib.path), exported(product_lib.path)
    hip_ids = lambda names: {nm for nm in names if nm.startswith("__hip_cuid_")}         # one per translation unit, named by content
    assert set(binding.NAVCARVE_SYMBOLS) <= have and carve_lib.has_navcarve and carve_lib.has_navgrid and carve_lib.has_raycast
    assert product - hip_ids(product) <= have
    extra = have - product - hip_ids(have)
    assert extra - set(binding.NAVCARVE_SYMBOLS) == {nm for nm in extra if "k_navcarve_" in nm}, sorted(extra)
    assert not set(binding.NAVCARVE_SYMBOLS) & product and not product_lib.has_navcarve
    assert not [nm for nm in product if "navcarve" in nm]
    assert not set(binding.NAVCARVE_SYMBOLS) & exported(oracle_lib.path) and not oracle_lib.has_navcarve
    assert set(binding.ABI_SYMBOLS) <= have and carve_lib.backend == "hip-gfx950"
    f = binding.Fusion(oracle_lib, oracle_lib.default_config(width=64, height=48, fx=60.0, fy=60.0, cx=31.5, cy=23.5))
    for call, symbol in ((lambda: f.nav_grid_carve(None), "ssf_navgrid_carve"), (lambda: f.nav_grid_carve_device(None), "ssf_navgrid_carve"),
                         (f.nav_grid_carve_default_params, "ssf_navcarve_default_params")):
        with pytest.raises(binding.SsfError, match=symbol):
            call()


def test_the_carve_symbols_stay_out_of_ssf_h():
    for nm in binding.NAVCARVE_SYMBOLS:
        assert nm not in binding.ABI_SYMBOLS
        assert nm not in open(os.path.join(INCLUDE, "ssf.h")).read()
        assert nm not in open(os.path.join(INCLUDE, "ssf_testing.h")).read()
        assert (nm + "(" in open(os.path.join(INCLUDE, "ssf_navcarve.h")).read()) != nm.startswith("ssf_debug_")      # the hooks: a header of their own
        assert (nm + "(" in open(os.path.join(INCLUDE, "ssf_navcarve_testing.h")).read()) == nm.startswith("ssf_debug_")
    assert "#define SSF_ABI_VERSION 3" in open(os.path.join(INCLUDE, "ssf.h")).read()


@pytest.mark.parametrize("lang", ["c", "c++"])
def test_the_header_compiles_on_its_own(lang, tmp_path):
    src = tmp_path / ("t.c" if lang == "c" else "t.cpp")
    src.write_text('#include "ssf_navcarve.h"\n'
                   "int f(ssf_handle* h, const float* views, int8_t* state, uint32_t* seen) {\n"
                   "    ssf_navgrid_params g; ssf_navcarve_params c; ssf_navcarve_stats s; ssf_navcarve_out o;\n"
                   "    if (ssf_navgrid_default_params(h, &g) != SSF_OK || ssf_navcarve_default_params(h, &c) != SSF_OK) return -1;\n"
                   "    c.views = views; c.n_views = 3; c.stride = 4;\n"
                   "    o.grid.zmin = 0; o.grid.zmax = 0; o.grid.hits = 0; o.grid.state = state; o.grid.dist2 = 0; o.seen = seen;\n"
                   "    return ssf_navgrid_carve(h, &g, &c, &o, &s) + (int)s.cells_carved + (int)s.grid.cells_free; }\n")
    cc, std = ("gcc", "-std=c99") if lang == "c" else ("g++", "-std=c++11")
    r = subprocess.run([cc, std, "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", INCLUDE, "-c", str(src), "-o", str(tmp_path / "t.o")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout


def test_the_binding_structs_have_the_headers_layout(tmp_path):
    classes = (("ssf_navcarve_params", binding.SsfNavCarveParams), ("ssf_navcarve_out", binding.SsfNavCarveOut),
               ("ssf_navcarve_stats", binding.SsfNavCarveStats))
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "ssf_navcarve.h"', "int main(void) {"]
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
    assert binding.NAVCARVE_OUTPUT_NAMES == nc.OUTPUTS
    assert tuple(nm for nm, _ in binding.SsfNavCarveStats._fields_[1:]) == nc.RAY_STATS


def test_ssf_hpp_carve_members_compile_and_link_against_the_carve_library(carve_lib, tmp_path):
    libdir = os.path.dirname(carve_lib.path)
    cmd = ["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", "-I", INCLUDE, "-I", CPP, os.path.join(CPP, "navcarve_smoke.cpp"),
           "-o", str(tmp_path / "navcarve_smoke"), "-L", libdir, "-lssf_hip_navcarve", "-Wl,-rpath," + libdir]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout


def test_the_replay_options_parse():
    a = replay.parse_args(["--npz", "frames.npz", "--nav-grid-dir", "grids", "--nav-grid-carve", "--nav-grid-carve-stride", "4"])
    assert a.nav_grid_dir == "grids" and a.nav_grid_carve is True and a.nav_grid_carve_stride == 4
    b = replay.parse_args(["--npz", "frames.npz", "--nav-grid-dir", "grids"])
    assert b.nav_grid_carve is False and b.nav_grid_carve_stride == 8
    with pytest.raises(SystemExit):
        replay.parse_args(["--npz", "frames.npz", "--nav-grid-carve"])          # needs --nav-grid-dir


def test_replay_thins_the_views_evenly():
    poses = np.arange(1000 * 12, dtype=np.float32).reshape(1000, 12)
    v = replay.thin_views(poses)
    assert v.shape == (256, 12) and v[0, 0] == 0 and v[-1, 0] == 999 * 12
    steps = np.diff(v[:, 0]) / 12
    assert steps.min() >= 3 and steps.max() <= 4
    assert np.array_equal(replay.thin_views(poses[:256]), poses[:256]) and replay.thin_views([]).shape == (0, 12)


def test_the_restatements_defaults_are_the_headers():
    hdr = open(os.path.join(INCLUDE, "ssf_navcarve.h")).read()
    for text in ("views NULL, n_views 0", "stride 8", "ray_min_conf 0, ray_splat_scale 0", "hit_margin_cells 1, carve_misses 0, min_seen 1"):
        assert text in hdr, text
    d = nc.DEFAULTS
    assert (d["cam_width"], d["stride"], d["t_min"], d["t_max"], d["ray_min_conf"], d["ray_splat_scale"], d["hit_margin_cells"],
            d["carve_misses"], d["min_seen"]) == (0, 8, 0.0, 0.0, 0.0, 0.0, 1.0, False, 1)
    c = nc.params(cfg_camera=CFG_CAMERA)
    assert (c["cam_width"], c["cam_height"], c["fx"], c["cy"], c["t_min"], c["t_max"]) == (160, 128, 150.0, 63.5, 0.2, 5.0)
    for text in ("the CURRENT map", "an obstacle cell is never carved", "a hole in the map is not evidence of free space",
                 "seen-through without observed floor is reported as free"):
        assert text in hdr, text


# ---- the restatement on the fixed scenes ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wall():
    m, n, pose, gkw, views, ckw = nc.wall_scene()
    q = nr.params(**gkw)
    return m, n, pose, q, views, ckw, {cm: nc.carve(m, n, pose, q, views, nc.params(carve_misses=cm, **ckw)) for cm in (False, True)}


@pytest.mark.parametrize("carve_misses", [False, True])
def test_the_wall_scene(carve_misses, wall):
    m, n, pose, q, views, ckw, res = wall
    got = res[carve_misses]
    assert n == 252 and got["seen"].shape == (31, 33)
    nc.check_wall(got, carve_misses, "the wall scene")
    s = got["stats"]
    assert [int((got["uncarved"] == v).sum()) for v in (0, 100, -1)] == [576, 21, 426]
    # the figures of the prototype this rule was written from: a cross-check of the restatement
    assert (s["rays"], s["rays_hit"], s["rays_invalid"]) == (320, 258, 0)
    assert (s["rays_carving"], s["ray_samples"], s["cells_carved"], s["cells_seen"], int(got["seen"].max())) == \
           ((320, 30534, 144, 403, 320) if carve_misses else (258, 10632, 78, 231, 258))
    assert int((got["seen"][got["state"] == 100] > 0).sum()) == (21 if carve_misses else 0)
    # the cells under the camera's own view, whose floor is not in the map, are the ones carved
    assert (got["state"][(got["uncarved"] < 0) & (got["seen"] > 0)] == 0).all()
    assert s["cells_free"] == 576 + s["cells_carved"] and s["cells_unknown"] == 426 - s["cells_carved"]
    assert np.array_equal(got["dist2"], nr.clearance(got["state"], q["max_dist_cells"], False))


def test_boundary_cases_with_hand_written_answers():
    m, gkw, cases = nc.boundary_cases()
    q = nr.params(**gkw)
    for name, views, carve, want in cases:
        got = nc.carve(m, 1, nr.IDENTITY, q, views, nc.params(**carve))
        nc.check_expectations(got, want, gkw["width"], gkw["height"], name)
        assert got["stats"]["ray_entries"] == int(got["seen"].sum())


def test_an_entry_counts_a_ray_not_its_samples():
    """a vertical ray through one cell's band: many accepted samples, one entry"""
    m, gkw, _ = nc.boundary_cases()
    down = nc.view_at(np.array([[1, 0, 0], [0, -1, 0], [0, 0, -1]], np.float64), (0.625, 0.625, 3.0)).reshape(1, 12)        # optical axis = map -z
    got = nc.carve(m, 1, nr.IDENTITY, nr.params(**gkw), down, nc.params(**dict(nc.BOUNDARY_CAMERA, carve_misses=True)))
    want = np.zeros((4, 8), np.uint32)
    want[2, 2] = 1                                                     # z = 3 .. -1 in steps of 1 / 8: the samples with 0 < z <= 1 are in cell (2, 2)
    assert np.array_equal(got["seen"], want) and got["stats"]["ray_samples"] == 33 and got["stats"]["ray_entries"] == 1


def test_the_restatement_agrees_with_the_f64_formulation(wall):
    m, n, pose, q, views, ckw, _ = wall
    scenes = [(m, n, pose, q, views, nc.params(carve_misses=True, **ckw))]
    hm = nr.hand_model(257, 1)
    q2 = nr.params(width=65, height=64, res=0.05)
    rng = np.random.default_rng(8)
    v2 = np.stack([nr.pose_about(nr.rot("y", rng.uniform(0, 360)) @ nr.rot("x", rng.uniform(-25, 10)), rng.uniform(-0.5, 0.5, 3)) for _ in range(3)])
    scenes.append((hm, 256, nr.caller_pose(q2), q2, v2, nc.params(fx=40.0, fy=40.0, cx=19.5, cy=15.5, cam_width=40, cam_height=32, stride=4, t_min=0.05,
                                                                  t_max=8.0, hit_margin_cells=0.5)))
    compared = rays_compared = 0
    for model, nvis, gp, gq, views, c in scenes:
        rays = nc.map_rays(views, c)
        got = rr.cast(model, nvis, rays, nr.IDENTITY, rr.params(t_min=c["t_min"], t_max=c["t_max"]))
        hit, valid = got["index"] >= 0, rr.transform(rays, nr.IDENTITY)[2]
        M = nc.extent(got["t"], hit, valid, gq, c)
        ref = nc.samples_f64(views, c, got["t"], hit, valid, gp, gq)
        for r in range(len(rays)):
            if ref["M_uncertain"][r]:
                continue
            assert M[r] == ref["M"][r], (r, M[r], ref["M"][r])
            rays_compared += 1
            if M[r] < 0:
                continue
            cell = nc.sample_cells(rays[r, :3], rays[r, 3:], int(M[r]), gp, gq)
            want, unc = ref["cells"][r]
            assert np.array_equal(cell[~unc], want[~unc]), (r, np.flatnonzero((cell != want) & ~unc))
            compared += int((~unc).sum())
    # not vacuous: most of the 560 rays, and at least a third of the wall scene's 30534 samples alone, are outside the guard band
    assert rays_compared > 400 and compared > 10000, (rays_compared, compared)


def test_without_views_the_grid_is_the_uncarved_one():
    m = nr.hand_model(257, 0)
    q = nr.params(width=33, height=31, res=0.05, unknown_is_obstacle=True)
    pose = nr.caller_pose(q)
    base = nr.build(m, 256, pose, q)
    got = nc.carve(m, 256, pose, q, np.zeros((0, 12), f32), nc.params(cfg_camera=CFG_CAMERA))
    for name in nr.OUTPUTS:
        assert np.array_equal(got[name].view(np.uint8), base[name].view(np.uint8)), name
    assert all(got["stats"][k] == base["stats"][k] for k in nr.STATS)
    assert not got["seen"].any() and all(got["stats"][k] == 0 for k in nc.RAY_STATS)


def test_the_device_tests_lattices_and_sample_counts():
    assert [(cw // s) * (ch // s) * n for cw, ch, s, n in nc.RAY_LATTICES] == [1, 63, 64, 65, 257, 1025]
    step = f32(0.25) * f32(0.5)
    assert [int(np.floor(f32(t) / step)) + 1 for t, _ in nc.SAMPLE_COUNTS] == [n for _, n in nc.SAMPLE_COUNTS] == [1, 63, 64, 65, 129]
