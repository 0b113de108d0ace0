"""An oriented footprint on the navigation grid (include/ssf_navfoot.h) without a GPU: the footprint's cells (ssf_navfoot_spans is host
only) against the restatement (tests/navfoot_ref.py), their symmetries, the conservativeness of nav_foot_pad's pad, the sweep mask,
the restated rollouts against the disc's restatement, who exports the entry points, the header on its own, the struct layouts of the
binding, and guards that the scenes of the GPU file show what they are there to show."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import navfoot_ref as fr
import navsteer_ref as sr
from conftest import ROOT
from supersurfel_fusion_amd import binding

INCLUDE = os.path.join(ROOT, "include")
OLDER = ("NAVCARVE_LIB", "NAV_LIB", "EXPLORE_LIB", "DRIVE_LIB", "LIVE_LIB", "STEER_LIB")


def exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], stdout=subprocess.PIPE, text=True, check=True).stdout
    return {l.split()[-1] for l in out.splitlines() if l.strip()}


@pytest.fixture(scope="module")
def foot_lib(product_lib):
    return binding.load_foot()


# ---- who exports what ----------------------------------------------------------------------------------------------------------
def test_the_foot_library_exports_the_footprint_and_all_of_the_steer_library(foot_lib, product_lib, oracle_lib):
    """libssf_hip_foot.so = libssf_hip_steer.so's objects + ssf_navfoot.hip; the seven older tables and the oracle hold no name of it"""
    have, steer = exported(foot_lib.path), exported(binding.STEER_LIB)
    hip_ids = lambda names: {nm for nm in names if nm.startswith("__hip_cuid_")}         # one per translation unit, named by content
    for names in (binding.NAVFOOT_SYMBOLS, binding.NAVSTEER_SYMBOLS, binding.NAVLIVE_SYMBOLS, binding.NAVPATH_SYMBOLS, binding.NAVFRONTIER_SYMBOLS,
                  binding.NAVPLAN_SYMBOLS, binding.NAVCARVE_SYMBOLS, binding.ABI_SYMBOLS):
        assert set(names) <= have
    assert foot_lib.has_navfoot and foot_lib.has_navsteer and foot_lib.has_navlive and foot_lib.has_navplan and foot_lib.backend == "hip-gfx950"
    assert steer - hip_ids(steer) <= have
    extra = have - steer - hip_ids(have)
    assert set(binding.NAVFOOT_SYMBOLS) <= extra and len(binding.NAVFOOT_SYMBOLS) == 4
    kernels = extra - set(binding.NAVFOOT_SYMBOLS)
    assert kernels == {nm for nm in extra if "k_navfoot_" in nm}, sorted(extra)
    assert all(any(k in nm for nm in kernels) for k in ("k_navfoot_layers", "k_navfoot_pack", "k_navfoot_roll", "k_navfoot_pick"))
    for other in [exported(product_lib.path), exported(oracle_lib.path)] + [exported(getattr(binding, nm)) for nm in OLDER]:
        assert not [nm for nm in other if "navfoot" in nm]
    for load in ("load_navcarve", "load_nav", "load_explore", "load_drive", "load_live", "load_steer"):
        assert not getattr(binding, load)().has_navfoot
    assert not product_lib.has_navfoot and not oracle_lib.has_navfoot


def test_the_steer_library_exports_what_it_exported():
    """the walk moved into a header both files instantiate: libssf_hip_steer.so gains no symbol by it"""
    have, live = exported(binding.STEER_LIB), exported(binding.LIVE_LIB)
    extra = {nm for nm in have - live if not nm.startswith("__hip_cuid_")}
    assert extra == set(binding.NAVSTEER_SYMBOLS) | {nm for nm in extra if "k_navsteer_" in nm}, sorted(extra)
    assert len({nm for nm in extra if "k_navsteer_" in nm and "__device_stub__" not in nm}) == 3          # pack, roll, pick: no template instance


def test_the_product_library_exports_the_recorded_list(product_lib):
    out = subprocess.run(["nm", "-D", "--defined-only", product_lib.path], stdout=subprocess.PIPE, text=True, check=True).stdout
    have = sorted(l.split()[2] for l in out.splitlines() if len(l.split()) == 3)
    want = open(os.path.join(ROOT, "tests", "golden", "libssf_hip_dynsyms.txt")).read().split()
    assert have == sorted(want), sorted(set(have) ^ set(want))


def test_an_older_library_names_the_missing_symbol(product_lib):
    lib = binding.load_steer()
    assert not lib.has_navfoot
    f = binding.Fusion.__new__(binding.Fusion)                            # (no handle: the check comes before any call)
    f.L = lib
    state, dist2, poses = np.zeros((3, 3), np.int8), np.ones((3, 3), np.int32), np.zeros((1, 3), np.int32)
    with pytest.raises(binding.SsfError, match="ssf_navfoot_layers.*binding.load_foot"):
        f.nav_foot(state, front=1024)
    with pytest.raises(binding.SsfError, match="ssf_navfoot_rollouts.*binding.load_foot"):
        f.nav_foot_steer(np.ones((3, 3), np.uint32), dist2, poses, 1, cost_weight=0)
    with pytest.raises(binding.SsfError, match="ssf_navfoot_default_params"):
        f.nav_foot_default_params()
    with pytest.raises(binding.SsfError, match="ssf_navfoot_spans.*binding.load_foot"):
        binding.navfoot_spans(0, 0, 0, 0, 0, 1, lib)
    with pytest.raises(binding.SsfError, match="ssf_navfoot_rollouts.*binding.load_foot"):
        f.nav_live_foot_steer(np.ones((48, 64), np.float32), state, [(1, 1)], poses, dict(front=1024))


def test_the_footprint_symbols_stay_out_of_the_other_headers():
    for nm in binding.NAVFOOT_SYMBOLS:
        assert nm not in binding.ABI_SYMBOLS
        for hdr in ("ssf.h", "ssf_testing.h", "ssf_navgrid.h", "ssf_navplan.h", "ssf_navlive.h", "ssf_navsteer.h"):
            assert nm not in open(os.path.join(INCLUDE, hdr)).read(), (nm, hdr)
        assert nm + "(" in open(os.path.join(INCLUDE, "ssf_navfoot.h")).read()
    assert "#define SSF_ABI_VERSION 3" in open(os.path.join(INCLUDE, "ssf.h")).read()


@pytest.mark.parametrize("lang", ["c", "c++"])
def test_the_header_compiles_on_its_own(lang, tmp_path):
    src = tmp_path / ("t.c" if lang == "c" else "t.cpp")
    src.write_text('#include "ssf_navfoot.h"\n'
                   "int f(ssf_handle* h, const int8_t* state, uint32_t* mask, const int32_t* dist2, const int32_t* poses, int32_t* cmd) {\n"
                   "    ssf_navfoot_params p; ssf_navfoot_stats s; ssf_navfoot_out o; ssf_navsteer_params q; ssf_navsteer_out r; ssf_navsteer_stats t;\n"
                   "    int16_t spans[SSF_NAVFOOT_MAX_HEADINGS * SSF_NAVFOOT_ROWS * 2]; int32_t reach; int64_t cells;\n"
                   "    if (ssf_navfoot_spans(1024, 1024, 512, 512, 0, 8, spans, &reach, &cells) != SSF_OK || reach > SSF_NAVFOOT_MAX_REACH) return -1;\n"
                   "    if (ssf_navfoot_default_params(h, &p) != SSF_OK || ssf_navsteer_default_params(h, &q) != SSF_OK) return -2;\n"
                   "    p.front = SSF_NAVFOOT_MAX_SIDE; p.pad = SSF_NAVFOOT_MAX_PAD; o.free_mask = mask; o.n_free = 0;\n"
                   "    if (ssf_navfoot_layers(h, &p, state, &o, &s) != SSF_OK) return -3;\n"
                   "    q.n_poses = 1; q.cost_weight = 0;\n"
                   "    r.best = 0; r.best_cmd = cmd; r.best_score = 0; r.n_admissible = 0; r.pose_status = 0; r.best_len = 0; r.best_traj = 0;\n"
                   "    r.cand_free = 0; r.cand_min_d = 0; r.cand_end = 0; r.cand_end_cost = 0; r.cand_score = 0;\n"
                   "    if (ssf_navfoot_rollouts(h, &q, p.n_headings, mask, dist2, 0, poses, 0, &r, &t) != SSF_OK) return -4;\n"
                   "    return (int)(s.cells_all + s.kernel_cells + t.poses_ok); }\n")
    cc, std = ("gcc", "-std=c99") if lang == "c" else ("g++", "-std=c++11")
    r = subprocess.run([cc, std, "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", INCLUDE, "-c", str(src), "-o", str(tmp_path / "t.o")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout


def test_the_binding_structs_have_the_headers_layout(tmp_path):
    classes = (("ssf_navfoot_params", binding.SsfNavFootParams), ("ssf_navfoot_out", binding.SsfNavFootOut),
               ("ssf_navfoot_stats", binding.SsfNavFootStats))
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "ssf_navfoot.h"', "int main(void) {"]
    for st, cls in classes:
        lines.append('    printf("%s %%zu\\n", sizeof(%s));' % (st, st))
        for nm, _ in cls._fields_:
            lines.append('    printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (st, nm, st, nm))
    lines += ['    printf("consts %d %d %d %d\\n", SSF_NAVFOOT_MAX_REACH, SSF_NAVFOOT_ROWS, SSF_NAVFOOT_MAX_SIDE, SSF_NAVFOOT_MAX_PAD);', "    return 0; }"]
    src = tmp_path / "off.c"
    src.write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "off")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", INCLUDE, str(src), "-o", exe], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    rows = [l.split() for l in subprocess.run([exe], stdout=subprocess.PIPE, text=True, check=True).stdout.splitlines()]
    got = {r[0]: r[1] for r in rows if r[0] != "consts"}
    for st, cls in classes:
        assert int(got[st]) == C.sizeof(cls), st
        for nm, _ in cls._fields_:
            assert int(got["%s.%s" % (st, nm)]) == getattr(cls, nm).offset, (st, nm)
    consts = tuple(int(v) for v in [r for r in rows if r[0] == "consts"][0][1:])
    assert consts == (binding.NAVFOOT_MAX_REACH, binding.NAVFOOT_ROWS, binding.NAVFOOT_MAX_SIDE, binding.NAVFOOT_MAX_PAD)
    assert consts == (fr.MAX_REACH, fr.ROWS, fr.MAX_SIDE, fr.MAX_PAD) and binding.NAVFOOT_HEADINGS == fr.HEADINGS
    assert tuple(nm for nm, _ in binding.SsfNavFootStats._fields_) == fr.STATS


# ---- the footprint's cells -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 4, 32])
@pytest.mark.parametrize("name", list(fr.FOOTPRINTS))
def test_the_spans_equal_the_restatement(name, B, foot_lib):
    foot = fr.FOOTPRINTS[name]
    want, reach, cells, one = fr.cached(("spans", name, B), lambda: fr.spans(foot, B))
    got, got_reach, got_cells = binding.navfoot_spans(*foot, B, library=foot_lib)
    assert got.dtype == np.int16 and got.shape == (B, fr.ROWS, 2) and (got == want).all(), np.argwhere(got != want)[:5].tolist()
    assert (got_reach, got_cells) == (reach, cells) and reach <= fr.MAX_REACH
    assert one, "a row of covered cells is not one interval"
    assert (got[:, fr.MAX_REACH, 0] <= 0).all() and (got[:, fr.MAX_REACH, 1] >= 0).all()          # (0, 0) is covered in every bin
    if name == "point":
        assert cells == B and reach == 0 and (got[:, fr.MAX_REACH] == 0).all()
        assert (np.delete(got, fr.MAX_REACH, axis=1) == (1, 0)).all()
    if name == "line":                                                    # bin 0 is the ten cells (0..9, 0)
        assert got[0, fr.MAX_REACH].tolist() == [0, 9] and (np.delete(got[0], fr.MAX_REACH, axis=0) == (1, 0)).all() and reach == 9
    if name == "corner0":                                                 # 28 cells to every side: the square at bin 0, sqrt(2) * 28 = 39.6 on the diagonal
        assert got[0, fr.MAX_REACH].tolist() == [-28, 28] and reach == (28 if B == 1 else 39 if B >= 8 else 28)
    if name.startswith("corner"):
        assert reach >= 28


def test_the_half_turn_bin_is_the_mirror_and_the_swapped_footprint(foot_lib):
    """C[k + 512] = -C[k] and S likewise, exactly: bin b + B/2 covers (dx, dy) iff bin b covers (-dx, -dy), the body turned by a half
    turn; and that mirrored body is the one with front / back and left / right swapped, so bin b + B/2 IS bin b of the swapped one"""
    for foot in (fr.ASYM, fr.LINE, fr.CORNERS[1]):
        front, back, left, right, pad = foot
        for B in (2, 4, 32):
            a, _, _ = binding.navfoot_spans(front, back, left, right, pad, B, library=foot_lib)
            sw, _, _ = binding.navfoot_spans(back, front, right, left, pad, B, library=foot_lib)
            for k in range(B):
                half = (k + B // 2) % B
                assert (a[half] == sw[k]).all(), (foot, B, k)
                m = a[half, ::-1]                                        # row dy <-> row -dy, (lo, hi) -> (-hi, -lo)
                empty = a[k, :, 0] > a[k, :, 1]
                assert ((m[:, 0] > m[:, 1]) == empty).all(), (foot, B, k)
                assert (a[k, ~empty, 0] == -m[~empty, 1]).all() and (a[k, ~empty, 1] == -m[~empty, 0]).all(), (foot, B, k)
            assert not (a[0] == a[B // 2]).all() or foot[0] == foot[1]       # (not vacuous: an asymmetric body differs from its mirror)


@pytest.mark.parametrize("B,sides", [(4, (1024, 512, 512, 768)), (8, (2048, 1024, 1024, 1536)), (16, (6144, 1024, 2048, 3072)), (32, (6144, 1024, 2048, 3072))])
def test_the_helpers_pad_covers_every_cell_the_true_rectangle_touches(B, sides, foot_lib):
    """the conservativeness claim: for any position in the robot's cell and any heading in the bin, the cell of every point of the
    true rectangle (real trigonometry, no pad) is covered by the padded footprint at the bin"""
    front, back, left, right = sides                                      # (the larger the body, the more headings keep the pad <= 4096)
    pad = binding.Fusion.nav_foot_pad(front, back, left, right, B)
    assert pad == fr.pad_for(front, back, left, right, B) and pad <= fr.MAX_PAD
    sp, reach, _ = binding.navfoot_spans(front, back, left, right, pad, B, library=foot_lib)
    shift, half = fr.bins(B)
    rng = np.random.default_rng(5 + B)
    n = 2000
    b = rng.integers(0, B, n)
    h = (b << shift) + rng.integers(-half, half, n)                       # every heading whose bin is b
    pos = rng.random((n, 2)) * 1024.0
    pt = np.stack([rng.uniform(-back, front, n), rng.uniform(-right, left, n)], axis=1)
    # boundary points: the corners and edge midpoints, at the cell's corners and the bin's two ends
    edge = np.array([(front, left), (front, -right), (-back, left), (-back, -right), (front, 0), (-back, 0), (0, left), (0, -right)], np.float64)
    eb = rng.integers(0, B, 64)
    b = np.concatenate([b, eb])
    h = np.concatenate([h, (eb << shift) + np.where(np.arange(64) % 2 == 0, -half, half - 1)])
    pos = np.concatenate([pos, np.array([(0, 0), (1023.999, 0), (0, 1023.999), (1023.999, 1023.999)])[np.arange(64) % 4]])
    pt = np.concatenate([pt, edge[np.arange(64) % 8]])
    assert (fr.bin_of(h & 0xFFFF, B) == b).all()
    th = 2.0 * np.pi * h / 65536.0
    wx = pos[:, 0] + pt[:, 0] * np.cos(th) - pt[:, 1] * np.sin(th)
    wy = pos[:, 1] + pt[:, 0] * np.sin(th) + pt[:, 1] * np.cos(th)
    dx, dy = np.floor(wx / 1024.0).astype(int), np.floor(wy / 1024.0).astype(int)
    assert np.abs(dx).max() <= reach and np.abs(dy).max() <= reach
    lo, hi = sp[b, dy + fr.MAX_REACH, 0], sp[b, dy + fr.MAX_REACH, 1]
    miss = ~((lo <= dx) & (dx <= hi))
    assert not miss.any(), (int(miss.sum()), b[miss][:5], dx[miss][:5], dy[miss][:5])
    # and the pad is not idle: without it some touched cell is not covered
    sp0, _, _ = binding.navfoot_spans(front, back, left, right, 0, B, library=foot_lib)
    inside = np.abs(dy) <= fr.MAX_REACH
    assert (~((sp0[b, dy + fr.MAX_REACH, 0] <= dx) & (dx <= sp0[b, dy + fr.MAX_REACH, 1])))[inside].any()


def test_the_parameter_refusals_that_need_no_device(foot_lib):
    L = foot_lib.lib
    sp, reach, cells = np.zeros((32, 81, 2), np.int16), C.c_int32(0), C.c_int64(0)
    call = lambda *a: L.ssf_navfoot_spans(*a, sp.ctypes.data_as(C.c_void_p), C.byref(reach), C.byref(cells))
    assert call(0, 0, 0, 0, 0, 1) == 0 and call(24576, 24576, 24576, 24576, 4096, 32) == 0
    for bad in ((-1, 0, 0, 0, 0, 4), (0, 24577, 0, 0, 0, 4), (0, 0, -5, 0, 0, 4), (0, 0, 0, 1 << 20, 0, 4), (0, 0, 0, 0, -1, 4), (0, 0, 0, 0, 4097, 4),
                (0, 0, 0, 0, 0, 0), (0, 0, 0, 0, 0, 3), (0, 0, 0, 0, 0, 64), (0, 0, 0, 0, 0, -2)):
        assert call(*bad) != 0, bad
    assert L.ssf_navfoot_spans(0, 0, 0, 0, 0, 1, None, None, None) != 0
    assert L.ssf_navfoot_spans(1024, 0, 0, 0, 0, 2, None, C.byref(reach), None) == 0 and reach.value == 1
    for bad in ((0, 0, 0, 0, 0, 3), (30000, 0, 0, 0, 0, 4)):
        with pytest.raises(binding.SsfError, match="ssf_navfoot_spans refused"):
            binding.navfoot_spans(*bad, library=foot_lib)
    assert L.ssf_navfoot_default_params(None, None) != 0
    assert L.ssf_navfoot_layers(None, None, None, None, None) != 0
    assert L.ssf_navfoot_rollouts(None, None, 1, None, None, None, None, None, None, None) != 0
    with pytest.raises(binding.SsfError):
        binding.Fusion.nav_foot_pad(1024, 1024, 512, 512, 3)
    assert binding.Fusion.nav_foot_units(0.3, 0.3, 0.2, 0.2, 0.05) == dict(front=6144, back=6144, left=4096, right=4096)
    assert binding.Fusion.nav_foot_units(0.31, 0, 0, 0, 0.05)["front"] == 6349                                 # rounded up: 6348.8


# ---- the sweep mask ----------------------------------------------------------------------------------------------------------------------
def test_the_sweep_mask_by_hand():
    m = fr.sweep_mask
    assert m(0, -100, 32) == 1 and m(0, -1024, 32) == 1 and m(0, -1025, 32) == (1 << 31) | 1       # a + w = 0 is still bin 0; -1 is bin 31
    assert m(65535, 2048, 32) == 0b11 and m(65535, 0, 32) == 1 and m(65535, 1, 32) == 1            # 65535 lies in bin 0: the wrap
    assert m(0, 16384, 32) == (1 << 9) - 1 and m(0, -16384, 32) == 1 | (0xFF << 24)                  # a quarter turn: nine bins
    assert m(1024, 16384, 32) == ((1 << 9) - 1) << 1 and m(1023, 16384, 32) == (1 << 9) - 1
    assert all(bin(m(h, w, 32)).count("1") <= 32 // 4 + 2 for h in (0, 1, 1023, 1024, 65535, 33791) for w in (16384, -16384))
    assert m(12345, 0, 32) == 1 << fr.bin_of(12345, 32) and m(12345, 0, 8) == 1 << fr.bin_of(12345, 8)
    assert all(m(h, w, 1) == 1 for h in (0, 1, 32767, 32768, 65535) for w in (0, 1, -1, 16384, -16384))
    assert m(0, 0, 2) == 1 and m(0, 16384, 2) == 0b11 and m(0, 16383, 2) == 1 and m(0, -16384, 2) == 1 and m(0, -16385 + 1, 2) == 1
    assert m(16383, 1, 2) == 0b11 and m(16384, 0, 2) == 0b10 and m(49151, 16384, 2) == 0b11 and m(49152, 16384, 2) == 1
    assert m(65535, 16384, 2) == 0b01 and m(40000, -16384, 2) == 0b10


def test_the_sweep_mask_is_the_set_of_bins_of_the_headings_passed():
    rng = np.random.default_rng(11)
    for B in fr.HEADINGS:
        for h, w in zip(rng.integers(0, 65536, 60).tolist() + [0, 0, 65535, 65535], rng.integers(-16384, 16385, 60).tolist() + [-16384, 16384, 16384, -16384]):
            t = np.arange(min(0, w), max(0, w) + 1)
            want = 0
            for b in np.unique(fr.bin_of((h + t) & 0xFFFF, B)):
                want |= 1 << int(b)
            assert fr.sweep_mask(h, w, B) == want, (B, h, w)


# ---- the restated rollouts against the disc's restatement ------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", sr.GPU_CASES)
def test_the_point_footprint_with_one_bin_is_the_disc(scene):
    """with the point footprint and B = 1 the mask is `clear`, every need is bit 0, and the rule is ssf_navsteer.h's"""
    i = sr.scene(scene)
    c = i["c"]
    want = sr.case_reference(scene)
    lay = fr.layers(i["state"], c["allow_unknown"], fr.POINT, 1)
    assert (lay["free_mask"] == fr.clear_cells(i["state"], c["allow_unknown"])).all()
    got = fr.rollouts(lay["free_mask"], 1, i["dist2"], i["cost"] if c["cost_weight"] else None, i["poses"], i["targets"] if c["target_weight"] else None, c)
    for nm in sr.OUTPUTS:
        assert got[nm].dtype == want[nm].dtype and (got[nm] == want[nm]).all(), (scene, nm)
    for k in sr.STATS:
        assert got["stats"][k] == want["stats"][k], (scene, k)


# ---- the restated layers, by hand ----------------------------------------------------------------------------------------------------------
def test_one_obstacle_blocks_the_reflected_kernel():
    """one occupied cell at o: bit b of cell p is cleared iff o - p is covered in bin b, i.e. p lies in the kernel reflected through o"""
    B, foot = 8, fr.ASYM
    state = np.zeros((41, 43), np.int8)
    state[20, 21] = 100
    lay = fr.layers(state, 0, foot, B)
    cov = fr.covered(foot, B)
    R = fr.MAX_REACH
    inner = np.zeros((41, 43), bool)
    reach = lay["stats"]["reach"]
    inner[reach:41 - reach, reach:43 - reach] = True                     # (nearer the border the outside blocks as well)
    for b in range(B):
        blocked = ((lay["free_mask"] >> np.uint32(b)) & 1) == 0
        want = np.zeros((41, 43), bool)
        for r, c in np.argwhere(cov[b]):
            y, x = 20 - (r - R), 21 - (c - R)
            if 0 <= y < 41 and 0 <= x < 43:
                want[y, x] = True
        assert (blocked[inner] == want[inner]).all(), b
    assert lay["free_mask"][20, 21] == 0 and lay["n_free"][20, 21] == 0 and lay["stats"]["cells_clear"] == 41 * 43 - 1
    s = lay["stats"]
    assert s["cells_all"] + s["cells_some"] + s["cells_none"] == 41 * 43 and s["cells_some"] > 0 and s["cells_all"] > 0


def test_the_corridor_shows_what_the_disc_cannot():
    """the demonstration, on the restatements: an 11 x 5-cell robot one cell off the middle of a 7-cell corridor drives along it, cannot
    turn on the spot, and the disc of the circumscribed radius does not fit at all"""
    i = fr.corridor_scene()
    c = i["c"]
    lay = fr.cached("corridor layers", lambda: fr.layers(i["state"], 0, i["foot"], i["B"]))
    got = fr.cached("corridor rollouts", lambda: fr.rollouts(lay["free_mask"], i["B"], i["dist2"], i["cost"], i["poses"], None, c))
    v, w, _ = sr.lattice(c)
    assert (got["pose_status"] == 0).all() and (got["best_cmd"][:, 0] == v.max()).all() and (got["best_cmd"][:, 1] == 0).all()
    assert (got["best_len"] == c["n_steps"] + 1).all()
    for q in range(len(i["poses"])):
        tr = got["best_traj"][q, :got["best_len"][q]]
        assert (tr[:, 1] >> 10 == 18).all() and tr[-1, 0] - tr[0, 0] == 16 * 512          # along the corridor: sixteen steps of half a cell
    spin = (v == 0) & (w != 0)
    assert spin.sum() == 8 and set(np.unique(got["cand_free"][:, spin]).tolist()) <= {0, 1} and (got["cand_free"][:, spin] == 1).any()
    assert (got["cand_free"][:, (v == 0) & (w == 0)] == c["n_steps"]).all()
    radius2 = int(np.ceil((5632 ** 2 + 2560 ** 2) / 1024.0 ** 2))        # the circumscribed radius in cells, squared: 37
    assert radius2 == 37
    disc = sr.rollouts(i["state"], i["dist2"], i["cost"], i["poses"], None, dict(c, min_dist2=radius2))
    assert set(disc["pose_status"].tolist()) <= {2, 3} and (disc["best"] == -1).all()
    inscribed = sr.rollouts(i["state"], i["dist2"], i["cost"], i["poses"], None, dict(c, min_dist2=6))      # 2.5 cells, squared
    assert (inscribed["cand_free"][:, spin] == c["n_steps"]).all()          # ... and the inscribed disc turns on the spot into the wall


# ---- replay.py's options and the C++ surface ---------------------------------------------------------------------------------------------
def test_the_replay_options_parse():
    from supersurfel_fusion_amd import replay
    base = ["--npz", "frames.npz", "--nav-grid-dir", "grids", "--nav-plan-goal", "1.0", "2.0"]
    a = replay.parse_args(base + ["--nav-steer", "--nav-steer-footprint", "0.3", "0.3", "0.2", "0.2"])
    assert replay.nav_steer_of(a) == dict(horizon=32, speed=0.5, footprint=(0.3, 0.3, 0.2, 0.2), headings=16)
    a = replay.parse_args(base + ["--nav-steer", "--nav-steer-footprint", "0.3", "0.1", "0.2", "0.2", "--nav-steer-headings", "32", "--nav-steer-horizon", "8"])
    assert replay.nav_steer_of(a) == dict(horizon=8, speed=0.5, footprint=(0.3, 0.1, 0.2, 0.2), headings=32)
    assert replay.nav_steer_of(replay.parse_args(base + ["--nav-steer"])) == dict(horizon=32, speed=0.5)        # without it: as before
    for bad in (["--nav-steer-footprint", "0.3", "0.3", "0.2", "0.2"], ["--nav-steer", "--nav-steer-headings", "16"],
                ["--nav-steer", "--nav-steer-footprint", "0.3", "0.3", "0.2"], ["--nav-steer", "--nav-steer-footprint", "0.3", "-0.3", "0.2", "0.2"],
                ["--nav-steer", "--nav-steer-footprint", "0.3", "0.3", "0.2", "0.2", "--nav-steer-headings", "12"]):
        with pytest.raises(SystemExit):
            replay.parse_args(base + bad)


def test_the_replay_loads_the_library_that_exports_what_its_options_call(foot_lib):
    """main() takes its library from library_of(): with a footprint the one that exports ssf_navfoot_*, and without one what it took before"""
    from supersurfel_fusion_amd import replay
    grid = ["--npz", "frames.npz", "--nav-grid-dir", "grids"]
    base = grid + ["--nav-plan-goal", "1.0", "2.0"]
    foot = base + ["--nav-steer", "--nav-steer-footprint", "0.3", "0.3", "0.2", "0.2"]
    assert replay.library_of(replay.parse_args(foot)) == "load_foot"
    assert replay.library_of(replay.parse_args(foot + ["--nav-steer-headings", "8", "--nav-live", "--nav-grid-carve"])) == "load_foot"
    lib = getattr(binding, replay.library_of(replay.parse_args(foot)))()
    assert lib.has_navfoot and lib.has_navsteer and lib.path == foot_lib.path
    for more, want in ((["--nav-steer"], "load_steer"), (["--nav-live"], "load_live"), (["--nav-plan-waypoints"], "load_drive"), ([], "load_nav")):
        assert replay.library_of(replay.parse_args(base + more)) == want, more
    assert replay.library_of(replay.parse_args(grid + ["--nav-frontiers"])) == "load_explore"
    assert replay.library_of(replay.parse_args(grid + ["--nav-grid-carve"])) == "load_navcarve"
    assert replay.library_of(replay.parse_args(grid)) == "load_product" and replay.library_of(replay.parse_args(["--npz", "frames.npz"])) == "load_product"
    for name in ("load_steer", "load_live", "load_drive", "load_explore", "load_nav", "load_navcarve", "load_product"):
        assert callable(getattr(binding, name))


def test_ssf_hpp_footprint_members_compile_and_link_against_the_foot_library(foot_lib, tmp_path):
    libdir = os.path.dirname(foot_lib.path)
    cpp = os.path.join(ROOT, "tests", "cpp")
    exe = str(tmp_path / "navfoot_smoke")
    cmd = ["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", "-I", INCLUDE, "-I", cpp, os.path.join(cpp, "navfoot_smoke.cpp"),
           "-o", exe, "-L", libdir, "-lssf_hip_foot", "-Wl,-rpath," + libdir]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    # the sizes and the host helpers come before the program needs a device: they agree with the binding's
    r = subprocess.run([exe, "--sizes"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    assert "sizes params=%d out=%d stats=%d" % (C.sizeof(binding.SsfNavFootParams), C.sizeof(binding.SsfNavFootOut), C.sizeof(binding.SsfNavFootStats)) in r.stdout, r.stdout
    body = binding.Fusion.nav_foot_units(0.1, 0.05, 0.05, 0.05, float(np.float32(0.05)))
    assert body == dict(front=2048, back=1024, left=1024, right=1024)
    assert "units front=%d back=%d left=%d right=%d pad16=%d pad32=%d" % (body["front"], body["back"], body["left"], body["right"],
                                                                         binding.Fusion.nav_foot_pad(n_headings=16, **body),
                                                                         binding.Fusion.nav_foot_pad(n_headings=32, **body)) in r.stdout, r.stdout
    sp, reach, cells = binding.navfoot_spans(body["front"], body["back"], body["left"], body["right"], 0, 16, library=foot_lib)
    import navplan_ref as pr
    assert "spans rc=0 reach=%d cells=%d sum=%016x" % (reach, cells, pr.fnv1a(sp.tobytes())) in r.stdout, r.stdout
    # a program that steers with the disc alone still links against the steer library: the footprint's members leave no reference behind
    exe2 = str(tmp_path / "navsteer_smoke")
    r = subprocess.run(["g++", "-std=c++11", "-O1", "-I", INCLUDE, "-I", cpp, os.path.join(cpp, "navsteer_smoke.cpp"), "-o", exe2, "-L", libdir,
                        "-lssf_hip_steer", "-Wl,-rpath," + libdir], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
