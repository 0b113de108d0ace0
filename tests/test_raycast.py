"""Ray casts through the model (include/ssf_raycast.h) without a GPU: who exports the entry points, the header on its own, the struct
layouts of the binding, the C++ surface, replay.py's options, and the numpy restatement the GPU tests compare against
(tests/raycast_ref.py): against an f64 brute force, that its hand-built scenes are not trivial, and hand-written boundary-exact
answers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import raycast_ref as rr
from conftest import ROOT
from supersurfel_fusion_amd import binding, replay

INCLUDE = os.path.join(ROOT, "include")
CPP = os.path.join(ROOT, "tests", "cpp")
f32 = np.float32
# the scenes the restatement is examined on: (n, n_visible, seed), 1025 rays each
SCENES = ((257, 256, 0), (513, 257, 0), (513, 257, 2), (1300, 513, 1))


def exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], stdout=subprocess.PIPE, text=True, check=True).stdout
    return {l.split()[-1] for l in out.splitlines() if l.strip()}


@pytest.fixture(scope="module")
def scenes():
    """per scene: model, n_visible, rays, pose, params, the f32 restatement (with candidate counts) and the f64 brute force"""
    out = []
    for n, nv, seed in SCENES:
        m = rr.hand_model(n, seed)
        rays, pose, q = rr.scene_rays(m, 1025, seed), rr.scene_pose(seed), rr.params(**rr.scene_kw(seed))
        out.append(dict(name="n %d seed %d" % (n, seed), m=m, nv=nv, rays=rays, pose=pose, q=q, a=rr.cast(m, nv, rays, pose, q, detail=True),
                        b=rr.cast_f64(m, nv, rays, pose, q)))
    return out


# ---- static checks -----------------------------------------------------------------------------------------------------
def test_the_product_exports_the_raycast_entry_points(product_lib):
    assert binding.RAYCAST_SYMBOLS == ["ssf_raycast_default_params", "ssf_raycast"]
    assert set(binding.RAYCAST_SYMBOLS) <= exported(product_lib.path)
    assert product_lib.has_raycast


def test_the_checker_does_not_and_the_binding_says_so(oracle_lib):
    assert not set(binding.RAYCAST_SYMBOLS) & exported(oracle_lib.path)
    assert not oracle_lib.has_raycast
    f = binding.Fusion(oracle_lib, oracle_lib.default_config(width=64, height=48, fx=60.0, fy=60.0, cx=31.5, cy=23.5))
    rays = np.zeros((1, 6), f32)
    for call, symbol in ((lambda: f.raycast(rays), "ssf_raycast"), (lambda: f.raycast_device(0, 0), "ssf_raycast"),
                         (f.raycast_default_params, "ssf_raycast_default_params")):
        with pytest.raises(binding.SsfError, match=symbol):
            call()


def test_the_raycast_symbols_stay_out_of_ssf_h():
    for nm in binding.RAYCAST_SYMBOLS:
        assert nm not in binding.ABI_SYMBOLS
        assert nm + "(" not in open(os.path.join(INCLUDE, "ssf.h")).read()
        assert nm + "(" not in open(os.path.join(INCLUDE, "ssf_testing.h")).read()
        assert nm + "(" in open(os.path.join(INCLUDE, "ssf_raycast.h")).read()
    assert "#define SSF_ABI_VERSION 3" in open(os.path.join(INCLUDE, "ssf.h")).read()


def test_the_raycast_kernels_read_no_environment_and_hold_no_assembly():
    """(the one switch, the laboratory build's other march arm, sits behind SSF_EXPERIMENTS: the product's SSF_ENV_INT is its default)"""
    txt = open(os.path.join(ROOT, "supersurfel_fusion_amd", "csrc", "ssf_raycast.hip")).read()
    assert "getenv(" not in txt and "asm" not in txt
    assert txt.count("SSF_ENV") == 1 and txt.index("#ifdef SSF_EXPERIMENTS") < txt.index("SSF_ENV") < txt.index("#endif")


@pytest.mark.parametrize("lang", ["c", "c++"])
def test_the_header_compiles_on_its_own(lang, tmp_path):
    src = tmp_path / ("t.c" if lang == "c" else "t.cpp")
    src.write_text('#include "ssf_raycast.h"\n'
                   "int f(ssf_handle* h, const float* rays, int n, float* t, int32_t* index) {\n"
                   "    ssf_raycast_params p; ssf_raycast_stats s;\n"
                   "    if (ssf_raycast_default_params(h, &p) != SSF_OK) return -1;\n"
                   "    p.t_min = 0.1f; p.t_max = 30.0f; p.cell = 0.25f; p.hash_bits = 16; p.visible_only = 1;\n"
                   "    return ssf_raycast(h, &p, rays, n, t, index, 0, 0, 0, &s) + (int)s.rays_hit + (int)s.index_rebuilt; }\n")
    cc, std = ("gcc", "-std=c99") if lang == "c" else ("g++", "-std=c++11")
    r = subprocess.run([cc, std, "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", INCLUDE, "-c", str(src), "-o", str(tmp_path / "t.o")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout


def test_the_binding_structs_have_the_headers_layout(tmp_path):
    classes = (("ssf_raycast_params", binding.SsfRaycastParams), ("ssf_raycast_stats", binding.SsfRaycastStats))
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "ssf_raycast.h"', "int main(void) {"]
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
    assert binding.RAYCAST_OUTPUT_NAMES == rr.OUTPUTS
    assert set(rr.STATS) < {nm for nm, _ in binding.SsfRaycastStats._fields_}


def test_ssf_hpp_raycast_members_compile_and_link_against_the_product(product_lib, tmp_path):
    libdir = os.path.dirname(product_lib.path)
    cmd = ["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", "-I", INCLUDE, "-I", CPP, os.path.join(CPP, "raycast_smoke.cpp"),
           "-o", str(tmp_path / "raycast_smoke"), "-L", libdir, "-lssf_hip", "-Wl,-rpath," + libdir]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout


def test_the_replay_options_parse():
    a = replay.parse_args(["--npz", "frames.npz", "--laser-scan-dir", "scans", "--laser-scan-every", "5", "--laser-scan-beams", "720"])
    assert a.laser_scan_dir == "scans" and a.laser_scan_every == 5 and a.laser_scan_beams == 720
    b = replay.parse_args(["--npz", "frames.npz"])
    assert b.laser_scan_dir is None and b.laser_scan_every == 30 and b.laser_scan_beams == 360
    rays = replay.laser_scan_rays(8)
    assert rays.shape == (8, 6) and rays.dtype == np.float32 and not rays[:, :3].any() and not rays[:, 4].any()
    assert np.allclose(np.linalg.norm(rays[:, 3:], axis=1), 1.0, atol=1e-6)
    assert np.allclose(rays[4, 3:], (0, 0, 1), atol=1e-6) and np.allclose(rays[6, 3:], (1, 0, 0), atol=1e-6)      # forward, then the camera's x


def test_the_restatements_defaults_are_the_headers():
    hdr = open(os.path.join(INCLUDE, "ssf_raycast.h")).read()
    for text in ("cell: 0 = 0.125 m", "(s = splat_scale, 0 = 3)", "t_min = t_max = 0 means cfg.range_min / cfg.range_max", "T = 2^-7",
                 "more than 64 cells", "glo_j >= -32000 and ghi_j <= 32000", "dims.x < 2^-40", "* 1.0625f + hs * 0.03125f", "|c_j| * 2^-20 + cell * 2^-10"):
        assert text in hdr, text
    assert (rr.DEFAULT_CELL, rr.DEFAULT_SPLAT) == (0.125, 3.0)
    q = rr.params()
    assert (q["t_min"], q["t_max"], q["cell"], q["splat_scale"], q["min_conf"], q["visible_only"], q["hash_bits"]) == (0.2, 5.0, 0.125, 3.0, 0.0, False, 0)


# ---- the restatement against an f64 brute force ------------------------------------------------------------------------------
def test_the_restatement_agrees_with_the_f64_brute_force(scenes):
    """outside the rays with an f64 margin within a relative 1e-4 (the inside test's slack, the gap between the best and the second
    tt, tt against the range ends) both formulations name the same winner; fewer than 5 % of the rays are left out"""
    total = left_out = 0
    for sc in scenes:
        a, b = sc["a"], sc["b"]
        sure = ~b["uncertain"]
        total += len(sure)
        left_out += int((~sure).sum())
        assert (~sure).mean() < 0.05, (sc["name"], float((~sure).mean()))
        assert np.array_equal(a["index"][sure], b["index"][sure]), (sc["name"], np.flatnonzero(a["index"][sure] != b["index"][sure])[:10])
        hit = sure & (a["index"] >= 0)
        assert hit.sum() > 100
        # tt = num / den in f32: num and den are three products and two sums each of terms up to |w| and |D| (w = c - O, |w| <= tt |D| +
        # the disc's radius, below 1 m here), O itself three products and three sums of terms up to |O|: 16 roundings of 2^-24 bound
        # all of it, seen along D through 1 / cos of the angle between the ray and the normal
        O, D, _ = rr.transform(sc["rays"], sc["pose"])
        O, D = np.stack(O, axis=1).astype(np.float64), np.linalg.norm(np.stack(D, axis=1).astype(np.float64), axis=1)
        with np.errstate(all="ignore"):
            tol = 2.0 ** -20 * (np.abs(O).max(axis=1) + b["t"] * D + 1.0) / (D * b["cos"])
        assert (np.abs(a["t"].astype(np.float64) - b["t"])[hit] <= tol[hit]).all(), sc["name"]
    assert total == 1025 * len(SCENES) and left_out < 0.05 * total, (total, left_out)


def test_the_hand_built_scenes_are_not_trivial(scenes):
    """per scene: between a quarter and three quarters of the rays hit; some winners are not the row with the nearest centre; some rays
    have two or more candidates; there are exact ties in tt; both faces are hit; some rows are oversize and some are not -- so the GPU
    comparisons cannot pass by a trivial answer, and a wrong tie-break, a missing face or a dropped list would show"""
    for sc in scenes:
        a, b, m, q = sc["a"], sc["b"], sc["m"], sc["q"]
        n = len(a["t"])
        hit = a["index"] >= 0
        assert 0.25 * n <= hit.sum() <= 0.75 * n, (sc["name"], int(hit.sum()))
        assert a["stats"]["rays_hit"] == int(hit.sum()) and a["stats"]["rays_invalid"] == 0
        # the row with the nearest centre to the ray's origin, among the rows that take part
        O, D, _ = rr.transform(sc["rays"], sc["pose"])
        rows = rr.used_rows(m, sc["nv"], q)
        c = m["positions"][rows].astype(np.float64)
        d2 = ((c[None] - np.stack(O, axis=1).astype(np.float64)[:, None]) ** 2).sum(axis=2)
        nearest = rows[d2.argmin(axis=1)]
        assert (a["index"][hit] != nearest[hit]).sum() >= 20, sc["name"]
        assert (a["candidates"] >= 2).sum() >= 20, sc["name"]
        # exact ties: the winner has a coincident copy that is a candidate with the same tt bits (the copy is the next row)
        w = a["index"][hit]
        copies = np.flatnonzero((w + 1) % 40 == 39)
        ties = 0
        for r in np.flatnonzero(hit)[copies]:
            one = rr.cast({k: v[[a["index"][r] + 1]] for k, v in m.items()}, 1, sc["rays"][r:r + 1], sc["pose"], dict(q, min_conf=-1.0))
            ties += int(one["index"][0] == 0 and one["t"].view(np.uint32)[0] == a["t"].view(np.uint32)[r])
        assert ties >= 3, (sc["name"], ties)
        assert (b["face"] == 1).sum() >= 20 and (b["face"] == -1).sum() >= 20, sc["name"]
        over = rr.oversize(m, q) & rr.indexed_rows(m)
        assert 0 < over.sum() < 0.25 * len(over), (sc["name"], int(over.sum()))
        assert 0 < a["stats"]["rows_oversize"] == int(over.sum()) < a["stats"]["rows_indexed"]
        # every kind of oversize row is there: by its box, by the coordinate bound, by its axes
        assert over[7] and over[17] and over[27] and not over[0]
        # ... and the far rows are hit
        assert (np.isin(a["index"][hit], np.arange(17, len(over), 100))).any(), sc["name"]


# ---- boundary-exact rows ---------------------------------------------------------------------------------------------------
def test_the_restatement_on_boundary_exact_rows():
    m, cases = rr.boundary_cases()
    assert len(cases) >= 10
    for name, rows, rays, kw, want in cases:
        sub = {k: v[rows] for k, v in m.items()}
        for cell in (0.0, 1.0):                                         # (the rule does not depend on the index's cell)
            g = rr.cast(sub, len(rows), rays, rr.BOUNDARY_POSE, rr.params(cell=cell, **kw))
            rr.check_expectations(g, want, name)
            assert g["stats"]["rows_indexed"] == len(rows) and g["stats"]["rays"] == len(rays)
    # the discs are oversize at the default cell (10 x 10 x 2 cells) and in the grid at 1 m
    assert rr.oversize(m, rr.params(splat_scale=2.0)).all() and not rr.oversize(m, rr.params(splat_scale=2.0, cell=1.0)).any()
