"""The navigation grid (include/ssf_navgrid.h) without a GPU: who exports the entry points, the header on its own, the struct
layouts of the binding, the C++ surface, replay.py's options, and the numpy restatement the GPU tests compare against
(tests/navgrid_ref.py): its clearance against a brute-force minimum, its sampling and banding against an f64 formulation, the
coverage of a horizontal disc, and hand-written boundary-exact answers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import navgrid_ref as nr
from conftest import ROOT
from supersurfel_fusion_amd import binding, replay

INCLUDE = os.path.join(ROOT, "include")
CPP = os.path.join(ROOT, "tests", "cpp")
f32 = np.float32


def exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], stdout=subprocess.PIPE, text=True, check=True).stdout
    return {l.split()[-1] for l in out.splitlines() if l.strip()}


# ---- static checks -----------------------------------------------------------------------------------------------------
def test_the_product_exports_the_navgrid_entry_points(product_lib):
    assert len(binding.NAVGRID_SYMBOLS) == 3
    assert set(binding.NAVGRID_SYMBOLS) <= exported(product_lib.path)
    assert product_lib.has_navgrid


def test_the_checker_does_not_and_the_binding_says_so(oracle_lib):
    assert not set(binding.NAVGRID_SYMBOLS) & exported(oracle_lib.path)
    assert not oracle_lib.has_navgrid
    f = binding.Fusion(oracle_lib, oracle_lib.default_config(width=64, height=48, fx=60.0, fy=60.0, cx=31.5, cy=23.5))
    for call, symbol in ((f.nav_grid, "ssf_navgrid_build"), (f.nav_grid_device, "ssf_navgrid_build"),
                         (f.nav_grid_default_params, "ssf_navgrid_default_params"), (f.nav_grid_default_pose, "ssf_navgrid_default_pose")):
        with pytest.raises(binding.SsfError, match=symbol):
            call()


def test_the_navgrid_symbols_stay_out_of_ssf_h():
    for nm in binding.NAVGRID_SYMBOLS:
        assert nm not in binding.ABI_SYMBOLS
        assert nm not in open(os.path.join(INCLUDE, "ssf.h")).read()
        assert nm not in open(os.path.join(INCLUDE, "ssf_testing.h")).read()
        assert nm in open(os.path.join(INCLUDE, "ssf_navgrid.h")).read()
    assert "#define SSF_ABI_VERSION 3" in open(os.path.join(INCLUDE, "ssf.h")).read()


def test_the_navgrid_kernels_read_no_environment_and_hold_no_assembly():
    txt = open(os.path.join(ROOT, "supersurfel_fusion_amd", "csrc", "ssf_navgrid.hip")).read()
    assert "getenv(" not in txt and "SSF_ENV" not in txt and "asm" not in txt


def test_float_order_bits_has_one_definition():
    """the order-preserving image of a float is shared (ssf_slots.hpp), not copied"""
    csrc = os.path.join(ROOT, "supersurfel_fusion_amd", "csrc")
    holders = [nm for nm in sorted(os.listdir(csrc)) if nm.endswith((".hip", ".hpp", ".inc")) and
               "uint32_t float_order_bits(uint32_t" in open(os.path.join(csrc, nm)).read()]
    assert holders == ["ssf_slots.hpp"]


@pytest.mark.parametrize("lang", ["c", "c++"])
def test_the_header_compiles_on_its_own(lang, tmp_path):
    src = tmp_path / ("t.c" if lang == "c" else "t.cpp")
    src.write_text('#include "ssf_navgrid.h"\n'
                   "int f(ssf_handle* h, int8_t* state, int32_t* dist2) {\n"
                   "    ssf_navgrid_params p; ssf_navgrid_stats s; ssf_navgrid_out o; float pose[12];\n"
                   "    if (ssf_navgrid_default_params(h, &p) != SSF_OK) return -1;\n"
                   "    p.width = 256; p.height = 128; p.unknown_is_obstacle = 1;\n"
                   "    if (ssf_navgrid_default_pose(h, &p, pose) != SSF_OK) return -2;\n"
                   "    p.pose = pose;\n"
                   "    o.zmin = 0; o.zmax = 0; o.hits = 0; o.state = state; o.dist2 = dist2;\n"
                   "    return ssf_navgrid_build(h, &p, &o, &s) + (int)s.cells_free + (int)s.pose[9]; }\n")
    cc, std = ("gcc", "-std=c99") if lang == "c" else ("g++", "-std=c++11")
    r = subprocess.run([cc, std, "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", INCLUDE, "-c", str(src), "-o", str(tmp_path / "t.o")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout


def test_the_binding_structs_have_the_headers_layout(tmp_path):
    classes = (("ssf_navgrid_params", binding.SsfNavGridParams), ("ssf_navgrid_out", binding.SsfNavGridOut),
               ("ssf_navgrid_stats", binding.SsfNavGridStats))
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "ssf_navgrid.h"', "int main(void) {"]
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
    assert binding.NAVGRID_OUTPUT_NAMES == tuple(nm for nm, _ in binding.SsfNavGridOut._fields_) == nr.OUTPUTS


def test_ssf_hpp_navgrid_members_compile_and_link_against_the_product(product_lib, tmp_path):
    libdir = os.path.dirname(product_lib.path)
    cmd = ["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", "-I", INCLUDE, "-I", CPP, os.path.join(CPP, "navgrid_smoke.cpp"),
           "-o", str(tmp_path / "navgrid_smoke"), "-L", libdir, "-lssf_hip", "-Wl,-rpath," + libdir]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout


def test_the_replay_options_parse():
    a = replay.parse_args(["--npz", "frames.npz", "--nav-grid-dir", "grids", "--nav-grid-every", "5", "--nav-grid-res", "0.1"])
    assert a.nav_grid_dir == "grids" and a.nav_grid_every == 5 and a.nav_grid_res == 0.1
    b = replay.parse_args(["--npz", "frames.npz"])
    assert b.nav_grid_dir is None and b.nav_grid_every == 30 and b.nav_grid_res == 0.05


def test_the_restatements_defaults_are_the_headers():
    hdr = open(os.path.join(INCLUDE, "ssf_navgrid.h")).read()
    for text in ("res 0.05 m, width = height = 512, min_hits 1", "floor_cos 0.8, splat_scale 2, max_steps 8, max_dist_cells 40",
                 "z_min -1.5", "floor_max -0.8", "z_max 0.5"):
        assert text in hdr, text
    d = nr.DEFAULTS
    assert (d["res"], d["width"], d["height"], d["min_hits"], d["floor_cos"], d["splat_scale"], d["max_steps"], d["max_dist_cells"]) == \
           (0.05, 512, 512, 1, 0.8, 2.0, 8, 40)
    assert (d["z_min"], d["floor_max"], d["z_max"]) == (-1.5, -0.8, 0.5)


# ---- the clearance against a brute-force minimum -----------------------------------------------------------------------------
def random_states(rng, H, W, p_occ, p_free):
    u = rng.uniform(size=(H, W))
    return np.where(u < p_occ, 100, np.where(u < p_occ + p_free, 0, -1)).astype(np.int8)


@pytest.mark.parametrize("unknown", [False, True])
def test_the_separable_clearance_is_the_brute_force_minimum(unknown):
    rng = np.random.default_rng(3)
    grids = [random_states(rng, H, W, p, 0.5) for H, W in ((1, 1), (1, 9), (9, 1), (5, 7), (33, 40)) for p in (0.02, 0.3)]
    grids += [np.full((33, 40), 0, np.int8), np.full((6, 5), 100, np.int8), np.full((4, 4), -1, np.int8)]       # no obstacle at all; all obstacles
    one = np.full((33, 40), 0, np.int8)
    one[32, 0] = 100                                                                                             # one obstacle in a corner
    grids.append(one)
    for state in grids:
        for R in (1, 2, 7, 40, 1024):                                # R = 1; R larger than the grid
            got, want = nr.clearance(state, R, unknown), nr.clearance_brute(state, R, unknown)
            assert got.dtype == np.int32 and np.array_equal(got, want), (state.shape, R, unknown)
            obst = (state == 100) | ((state < 0) & unknown)
            assert (got[obst] == 0).all() and (got[~obst] > 0).all() and got.max() <= R * R
            if not obst.any():
                assert (got == R * R).all()
    assert (nr.clearance(np.full((4, 4), -1, np.int8), 5, False) == 25).all() and (nr.clearance(np.full((4, 4), -1, np.int8), 5, True) == 0).all()
    assert nr.clearance(one, 1024, False)[0, 39] == 32 * 32 + 39 * 39


# ---- sampling and banding against the f64 formulation -----------------------------------------------------------------------
def test_the_restatement_agrees_with_the_f64_formulation():
    """outside the guard band (1e-4 cells of a cell edge, 1e-4 m of a band limit) the two formulations put every sample into the same
    cell and the same class; at most 1 % of the samples of a case are inside the band"""
    total = left_out = 0
    for n, nv in nr.SIZES:
        m = nr.hand_model(n, 1)
        for name, frame, kw in nr.grid_cases(33, 31, 0.05):
            q = nr.params(**kw)
            pose = nr.caller_pose(q) if frame else nr.default_pose(nr.IDENTITY, q)
            a, b = nr.all_samples(m, nv, pose, q), nr.samples_f64(m, nv, pose, q)
            if a is None:
                assert len(b["row"]) == 0
                continue
            # the same lattices: rows whose lattice differs are uncertain as a whole (h / step within the band of an integer)
            ka, kb = a["row"] * 4096 + (a["i"] + 16) * 64 + (a["j"] + 16), b["row"] * 4096 + (b["i"] + 16) * 64 + (b["j"] + 16)
            bad_rows = np.setxor1d(ka, kb) // 4096
            assert set(bad_rows.tolist()) <= set(b["row"][b["uncertain"]].tolist()), (n, name)
            keep_a, keep_b = ~np.isin(a["row"], bad_rows), ~np.isin(b["row"], bad_rows)
            a, b = {k: v[keep_a] for k, v in a.items()}, {k: v[keep_b] for k, v in b.items()}
            assert np.array_equal(a["row"], b["row"]) and np.array_equal(a["i"], b["i"]) and np.array_equal(a["j"], b["j"])
            sure = ~b["uncertain"]
            total += len(sure)
            left_out += int((~sure).sum()) + int((~keep_b).sum())
            assert (~sure).sum() <= 0.01 * max(len(sure), 100), (n, name, int((~sure).sum()), len(sure))
            for key in ("in_grid", "accepted", "obstacle", "floor"):
                assert np.array_equal(a[key][sure], b[key][sure]), (n, nv, name, key)
            acc = sure & b["accepted"]
            assert np.array_equal(a["gx"][acc].astype(np.int64), np.floor(b["gx"][acc]).astype(np.int64)), (n, name)
            assert np.array_equal(a["gy"][acc].astype(np.int64), np.floor(b["gy"][acc]).astype(np.int64)), (n, name)
            assert np.abs(a["z"][acc] - b["z"][acc]).max(initial=0) < 1e-5, (n, name)
    assert total > 100000 and left_out <= 0.01 * total, (total, left_out)


def test_the_hand_built_grids_are_not_trivial():
    """on the larger hand-built models every case has cells of all three states and clearances strictly between 0 and the cap, so
    the GPU comparisons cannot pass by writing one value everywhere"""
    m = nr.hand_model(1300, 0)
    for name, frame, kw in nr.grid_cases(65, 64, 0.05):
        q = nr.params(**kw)
        g = nr.build(m, 513, nr.caller_pose(q) if frame else nr.default_pose(nr.IDENTITY, q), q)
        s = g["stats"]
        assert min(s["cells_free"], s["cells_occupied"], s["cells_unknown"]) > 0, (name, s)
        assert 0 < s["samples_in_grid"] < s["samples"], (name, s)
        assert len(np.unique(g["dist2"])) > 1 and np.isfinite(g["zmin"]).any() and np.isinf(g["zmin"]).any(), name
        assert s["cells_free"] + s["cells_occupied"] + s["cells_unknown"] == 65 * 64


def test_a_horizontal_disc_leaves_no_interior_cell_unhit():
    """a horizontal disc with both half-axes above res hits every cell whose centre lies inside the ellipse shrunk by 0.75 res (at
    step = res / 2 and with the lattice not clipped)"""
    rng = np.random.default_rng(17)
    res, W, H = 0.05, 48, 40
    q = nr.params(width=W, height=H, res=res, z_min=-1.0, z_max=1.0, floor_max=0.5, max_steps=16)
    for trial in range(60):
        h1, h2 = rng.uniform(1.05 * res, 0.39, 2)                  # half-axes: above res, below max_steps * step = 0.4
        c = np.array([rng.uniform(0.8, 1.6), rng.uniform(0.7, 1.3), 0.0])
        a = rng.uniform(0, np.pi)
        e1, e2 = np.array([np.cos(a), np.sin(a), 0.0]), np.array([-np.sin(a), np.cos(a), 0.0])
        m = dict(positions=c[None], colors=np.zeros((1, 3)), stamps=np.zeros((1, 2)), orientations=np.concatenate([e1, e2, [0, 0, 1]])[None],
                 shapes=np.zeros((1, 6)), dims=np.array([[(h1 / 2) ** 2, (h2 / 2) ** 2]]), confidences=np.ones(1))
        m = {name: np.ascontiguousarray(m[name], dt) for name, _, dt in nr.FIELDS}
        g = nr.build(m, 1, nr.IDENTITY, q)
        ix, iy = np.meshgrid(np.arange(W), np.arange(H))
        d = np.stack([(ix + 0.5) * res - c[0], (iy + 0.5) * res - c[1]], axis=-1)
        u, v = d @ e1[:2], d @ e2[:2]
        inside = (u / (h1 - 0.75 * res)) ** 2 + (v / (h2 - 0.75 * res)) ** 2 <= 1.0
        assert inside.any() and (g["hits"][..., 0][inside] > 0).all(), (trial, h1, h2, int(inside.sum()), int((g["hits"][..., 0][inside] == 0).sum()))
        assert g["stats"]["samples_in_grid"] == g["stats"]["samples"]


# ---- boundary-exact rows ---------------------------------------------------------------------------------------------------
def test_the_restatement_on_boundary_exact_rows():
    m, kw, cases = nr.boundary_rows()
    q = nr.params(**kw)
    for name, rows, want in cases:
        sub = {k: v[rows] for k, v in m.items()}
        g = nr.build(sub, len(rows), nr.BOUNDARY_POSE, q)
        nr.check_expectations(g, want, q["width"], q["height"], name)
        assert g["stats"]["rows_used"] == len(rows)
        assert np.array_equal(g["state"], nr.states(g["hits"], 1))
    # the -0 case really holds samples of both signs
    z = nr.all_samples({k: v[[10]] for k, v in m.items()}, 1, nr.BOUNDARY_POSE, q)["z"]
    assert (z == 0).all() and np.signbit(z).any() and not np.signbit(z).all()
    # all rows at once: the hit counts add up cell by cell
    hits = sum(nr.build({k: v[rows] for k, v in m.items()}, len(rows), nr.BOUNDARY_POSE, q)["hits"].astype(np.int64) for _, rows, _ in cases)
    both = nr.build(m, len(m["confidences"]), nr.BOUNDARY_POSE, q)
    assert np.array_equal(both["hits"], hits)
    # state and clearance of the grid's row 0 by hand: the wall makes (1, 0) and (2, 0) obstacles, rows 2 and 10 make (4, 0) to
    # (7, 0) floor; the nearest obstacles of the floor cells are the clipped disc's (4, 1) and (6, 1) in the row above
    assert both["state"][0].tolist() == [-1, 100, 100, -1, 0, 0, 0, 0]
    assert both["dist2"][0].tolist() == [1, 0, 0, 1, 1, 2, 1, 2]
