"""Rows of the model selected on the device (include/ssf_query.h) without a GPU: who exports the entry points, the header on its
own, the struct layouts of the binding, the C++ surface, replay.py's option, and the numpy restatement the GPU tests compare
against (tests/query_ref.py): checked against an independent f64 formulation and against hand-written boundary-exact answers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import query_ref as qr
import util
from conftest import ROOT
from supersurfel_fusion_amd import binding, replay

INCLUDE = os.path.join(ROOT, "include")
CPP = os.path.join(ROOT, "tests", "cpp")
f32 = np.float32


def exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], stdout=subprocess.PIPE, text=True, check=True).stdout
    return {l.split()[-1] for l in out.splitlines() if l.strip()}


def test_the_product_exports_the_query_entry_points(product_lib):
    assert set(binding.QUERY_SYMBOLS) <= exported(product_lib.path)
    assert product_lib.has_query


def test_the_checker_does_not_and_the_binding_says_so(oracle_lib):
    assert not set(binding.QUERY_SYMBOLS) & exported(oracle_lib.path)
    assert not oracle_lib.has_query
    f = binding.Fusion(oracle_lib, oracle_lib.default_config(width=64, height=48, fx=60.0, fy=60.0, cx=31.5, cy=23.5))
    for call, symbol in ((f.query_model, "ssf_query_rows"), (f.query_count, "ssf_query_count"),
                         (lambda: f.query_rows_into({}, np.zeros(1, np.int32), 1), "ssf_query_rows"),
                         (lambda: f.query_model_device({}, capacity=0), "ssf_query_rows"),
                         (f.query_default_params, "ssf_query_default_params")):
        with pytest.raises(binding.SsfError, match=symbol):
            call()


def test_the_query_symbols_stay_out_of_ssf_h():
    for nm in binding.QUERY_SYMBOLS:
        assert nm not in binding.ABI_SYMBOLS
        assert nm not in open(os.path.join(INCLUDE, "ssf.h")).read()
        assert nm not in open(os.path.join(INCLUDE, "ssf_testing.h")).read()
        assert nm in open(os.path.join(INCLUDE, "ssf_query.h")).read()
    assert "#define SSF_ABI_VERSION 3" in open(os.path.join(INCLUDE, "ssf.h")).read()


def test_the_query_kernels_read_no_environment_and_hold_no_assembly():
    txt = open(os.path.join(ROOT, "supersurfel_fusion_amd", "csrc", "ssf_query.hip")).read()
    assert "getenv(" not in txt and "SSF_ENV" not in txt and "asm" not in txt


@pytest.mark.parametrize("lang", ["c", "c++"])
def test_the_header_compiles_on_its_own(lang, tmp_path):
    src = tmp_path / ("t.c" if lang == "c" else "t.cpp")
    src.write_text('#include "ssf_query.h"\n'
                   "int f(ssf_handle* h, ssf_surfels* out, int32_t* idx) {\n"
                   "    ssf_query_params p; ssf_query_stats s;\n"
                   "    if (ssf_query_default_params(h, &p) != SSF_OK) return -1;\n"
                   "    p.region = SSF_REGION_SPHERE; p.radius = 2.0f; p.visible_only = 1;\n"
                   "    if (ssf_query_count(h, &p, &s) != SSF_OK) return -2;\n"
                   "    return ssf_query_rows(h, &p, out, idx, (int)s.n_selected, &s) + (int)s.n_selected_visible; }\n")
    cc, std = ("gcc", "-std=c99") if lang == "c" else ("g++", "-std=c++11")
    r = subprocess.run([cc, std, "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", INCLUDE, "-c", str(src), "-o", str(tmp_path / "t.o")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout


def test_the_binding_structs_have_the_headers_layout(tmp_path):
    fields = {"ssf_query_params": [nm for nm, _ in binding.SsfQueryParams._fields_],
              "ssf_query_stats": [nm for nm, _ in binding.SsfQueryStats._fields_]}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "ssf_query.h"', "int main(void) {"]
    for st, names in fields.items():
        lines.append('    printf("%s %%zu\\n", sizeof(%s));' % (st, st))
        for nm in names:
            lines.append('    printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (st, nm, st, nm))
    lines += ["    return 0; }"]
    src = tmp_path / "off.c"
    src.write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "off")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", INCLUDE, str(src), "-o", exe], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    got = dict(l.split() for l in subprocess.run([exe], stdout=subprocess.PIPE, text=True, check=True).stdout.splitlines())
    for st, cls in (("ssf_query_params", binding.SsfQueryParams), ("ssf_query_stats", binding.SsfQueryStats)):
        assert int(got[st]) == C.sizeof(cls), st
        for nm, _ in cls._fields_:
            assert int(got["%s.%s" % (st, nm)]) == getattr(cls, nm).offset, (st, nm)
    assert binding.QUERY_REGIONS == dict(all=0, sphere=1, box=2, frustum=3)
    hdr = open(os.path.join(INCLUDE, "ssf_query.h")).read()
    assert "SSF_REGION_ALL = 0, SSF_REGION_SPHERE = 1, SSF_REGION_BOX = 2, SSF_REGION_FRUSTUM = 3" in hdr


def test_ssf_hpp_query_members_compile_and_link_against_the_product(product_lib, tmp_path):
    libdir = os.path.dirname(product_lib.path)
    cmd = ["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", "-I", INCLUDE, "-I", CPP, os.path.join(CPP, "query_smoke.cpp"),
           "-o", str(tmp_path / "query_smoke"), "-L", libdir, "-lssf_hip", "-Wl,-rpath," + libdir]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout


def test_the_replay_option_parses():
    a = replay.parse_args(["--npz", "frames.npz", "--local-cloud-dir", "clouds", "--local-cloud-radius", "1.5", "--local-cloud-every", "5"])
    assert a.local_cloud_dir == "clouds" and a.local_cloud_radius == 1.5 and a.local_cloud_every == 5
    b = replay.parse_args(["--npz", "frames.npz"])
    assert b.local_cloud_dir is None and b.local_cloud_radius == 2.0 and b.local_cloud_every == 30


# ---- the restatement ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def camera_and_range(product_lib):
    """the camera and depth range of the GPU tests' handles (160 x 128)"""
    c = util.make_cfg(product_lib, 160, 128)
    return dict(width=c.width, height=c.height, fx=c.fx, fy=c.fy, cx=c.cx, cy=c.cy), (c.range_min, c.range_max)


def hand_built_cases(camera, z_range):
    for n, nv in qr.SIZES:
        for seed in qr.SEEDS:
            m = qr.hand_model(n, seed)
            yield n, nv, seed, m, [(name, qr.IDENTITY if pose is None else pose, qr.params(**kw))
                                   for name, pose, kw in qr.region_queries(camera, z_range)]


def test_the_restatement_agrees_with_the_f64_formulation(camera_and_range):
    """outside the guard band the two formulations select the same rows; on every hand-built model at most 2 % of the rows are
    inside the band"""
    for n, nv, seed, m, queries in hand_built_cases(*camera_and_range):
        for name, pose, q in queries:
            idx, stats = qr.select(m, nv, pose, q)
            got = np.zeros(n, bool)
            got[idx] = True
            want, uncertain = qr.select_f64(m, nv, pose, q)
            assert uncertain.sum() <= 0.02 * n, (n, nv, seed, name, int(uncertain.sum()))
            assert np.array_equal(got[~uncertain], want[~uncertain]), (n, nv, seed, name)
            assert stats["n_selected"] == len(idx) and stats["n_scanned"] == (nv if q["visible_only"] else n)
            assert stats["n_selected_visible"] == int((idx < nv).sum())
            if len(idx):
                assert np.array_equal(stats["lo"], m["positions"][idx].min(axis=0) + f32(0))
                assert np.array_equal(stats["hi"], m["positions"][idx].max(axis=0) + f32(0))


def test_the_hand_built_queries_are_not_trivial(camera_and_range):
    """Over the queries of a hand-built model the restatement selects strictly between nothing and everything it looks at, so the
    GPU comparisons cannot pass by selecting nothing or everything.  (Summed over a model's queries: the one-row model and a
    model without visible rows under visible_only leave a single query no room to be strictly in between.  From 16 scanned rows
    on, every single query is strictly in between as well.)"""
    for n, nv, seed, m, queries in hand_built_cases(*camera_and_range):
        sel = scanned = 0
        for name, pose, q in queries:
            idx, stats = qr.select(m, nv, pose, q)
            sel += stats["n_selected"]
            scanned += stats["n_scanned"]
            if stats["n_scanned"] >= 16:
                assert 0 < stats["n_selected"] < stats["n_scanned"], (n, nv, seed, name, stats)
        assert 0 < sel < scanned, (n, nv, seed, sel, scanned)


def test_the_restatement_on_boundary_exact_rows():
    m, nv, cam, zr, cases = qr.boundary_rows()
    for name, kw, want in cases:
        idx, stats = qr.select(m, nv, qr.IDENTITY, qr.params(**kw))
        assert idx.tolist() == want, (name, idx.tolist(), want)
        assert stats["n_selected_visible"] == sum(1 for i in want if i < nv), name
        # visible_only: the same answer cut at n_visible
        idx_v, stats_v = qr.select(m, nv, qr.IDENTITY, qr.params(visible_only=True, **kw))
        assert idx_v.tolist() == [i for i in want if i < nv] and stats_v["n_scanned"] == nv, name
    # -0 coordinates: lo / hi report +0, whatever the order of the rows
    idx, stats = qr.select(m, nv, qr.IDENTITY, qr.params(**dict(cases[-1][1])))
    util.assert_same_bits(stats["lo"], np.array([0.0, 0.0, 0.25], f32), "lo")
    util.assert_same_bits(stats["hi"], np.array([0.0, 0.0, 1.0], f32), "hi")
    only = {k: v[[14]] for k, v in m.items()}
    _, s14 = qr.select(only, 1, qr.IDENTITY, qr.params())
    util.assert_same_bits(s14["lo"], np.array([0.0, 0.0, 1.0], f32), "lo of the -0 row alone")
    util.assert_same_bits(s14["hi"], np.array([0.0, 0.0, 1.0], f32), "hi of the -0 row alone")
    # nothing selected: a zero box
    _, s0 = qr.select(m, nv, qr.IDENTITY, qr.params(min_conf=100.0))
    assert s0["n_selected"] == 0 and not s0["lo"].any() and not s0["hi"].any()
