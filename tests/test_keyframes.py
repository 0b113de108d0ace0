"""The fern-coded keyframe database (include/ssf_keyframes.h) without a GPU: who exports the entry points, the header on its own,
the C++ surface, and the numpy restatement the GPU tests compare against (tests/keyframe_ref.py) -- its known answers, and the
proof, on frames of the synthetic orbit run through the CPU checker, that the sequence the GPU tests use is not trivial."""
import os
import re
import subprocess

import numpy as np
import pytest

import keyframe_ref as kr
import util
from conftest import ROOT
from supersurfel_fusion_amd import binding

INCLUDE = os.path.join(ROOT, "include")
CPP = os.path.join(ROOT, "tests", "cpp")
f32 = np.float32

# The sequence of the GPU tests: orbit frames (1 degree apart per index) in the order one handle processes them, at 320 x 240 with
# the library's defaults (B 8, 500 ferns, seed 1234, new_ratio 0.3, loop_ratio 0.2) and min_gap 5.  test_the_sequence_* below
# prove on the restatement alone what it contains: views that are new, views that are not, a revisit, the far side of the room.
SEQUENCE = [0, 1, 2, 3, 5, 6, 10, 45, 90, 180, 181, 270, 0, 3, 1]
SEQ_SIZE = (320, 240)
SEQ_PARAMS = dict(cell=8, n_ferns=500, seed=1234, min_gap=5, new_ratio=0.3, loop_ratio=0.2)
REVISIT = 12                                       # index into SEQUENCE of the second visit of orbit frame 0


def exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], stdout=subprocess.PIPE, text=True, check=True).stdout
    return {l.split()[-1] for l in out.splitlines() if l.strip()}


def run_sequence(lib, on_frame):
    """SEQUENCE through one handle of `lib`; on_frame(fusion, index, rgb) after every frame"""
    W, H = SEQ_SIZE
    f = binding.Fusion(lib, util.make_cfg(lib, W, H))
    for i, k in enumerate(SEQUENCE):
        rgb, depth = util.frame(k, W, H)
        f.process_frame(rgb, depth)
        on_frame(f, i, rgb)
    return f


def reference_records(lib):
    """the restatement over SEQUENCE: per frame the consider record, from the frames' colour and plane depth as `lib` extracts
    them, the stamp the handle shows after the frame and the frame's rows with conf > 0"""
    W, H = SEQ_SIZE
    cfg = util.make_cfg(lib, W, H)
    ferns = kr.generate_ferns(SEQ_PARAMS["seed"], SEQ_PARAMS["n_ferns"], W, H, SEQ_PARAMS["cell"], cfg.range_min, cfg.range_max)
    db = kr.Database(SEQ_PARAMS["n_ferns"], min_gap=SEQ_PARAMS["min_gap"], new_ratio=SEQ_PARAMS["new_ratio"],
                     loop_ratio=SEQ_PARAMS["loop_ratio"])
    recs, codes = [], []

    def on_frame(f, i, rgb):
        c = kr.encode_frame(ferns, rgb, f.plane_depth(), SEQ_PARAMS["cell"], cfg.range_min, cfg.range_max)
        n_rows = int((f.get_frame()["confidences"] > 0).sum())
        codes.append(c)
        recs.append(db.consider(c, f.counts()["stamp"], n_rows))

    run_sequence(lib, on_frame)
    return recs, codes, db


@pytest.fixture(scope="module")
def seq_ref(oracle_lib):
    return reference_records(oracle_lib)


# ---- the surface ---------------------------------------------------------------------------------------------------------------
def test_the_header_declares_exactly_the_symbols_the_binding_lists():
    txt = open(os.path.join(INCLUDE, "ssf_keyframes.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"\b(ssf_keyframes_[a-z_]+)\s*\(", code))
    assert declared == set(binding.KEYFRAME_SYMBOLS)
    assert len(binding.KEYFRAME_SYMBOLS) == 14


def test_the_keyframe_symbols_stay_out_of_ssf_h():
    for nm in binding.KEYFRAME_SYMBOLS:
        assert nm not in binding.ABI_SYMBOLS
        assert nm not in open(os.path.join(INCLUDE, "ssf.h")).read()
        assert nm not in open(os.path.join(INCLUDE, "ssf_testing.h")).read()
    assert "#define SSF_ABI_VERSION 3" in open(os.path.join(INCLUDE, "ssf.h")).read()


def test_the_product_exports_the_keyframe_entry_points(product_lib):
    assert set(binding.KEYFRAME_SYMBOLS) <= exported(product_lib.path)
    assert product_lib.has_keyframes
    assert product_lib.lib.ssf_abi_version() == 3


def test_the_checker_does_not_and_the_binding_says_so(oracle_lib):
    assert not set(binding.KEYFRAME_SYMBOLS) & exported(oracle_lib.path)
    assert not oracle_lib.has_keyframes
    f = binding.Fusion(oracle_lib, oracle_lib.default_config(width=64, height=48, fx=60.0, fy=60.0, cx=31.5, cy=23.5))
    z = np.zeros(500, np.uint8)
    calls = ((f.keyframes_default_params, "default_params"), (f.keyframes_configure, "configure"), (f.keyframes_info, "info"),
             (lambda: f.keyframes_set_ferns(np.zeros(500, binding.FERN_DTYPE)), "set_ferns"), (f.keyframes_get_ferns, "get_ferns"),
             (f.keyframes_encode, "encode"), (lambda: f.keyframes_query(z, 3), "query"), (f.keyframes_add, "add"),
             (f.keyframes_consider, "consider"), (lambda: f.keyframes_put(z, None, np.zeros(12, f32), 0), "put"),
             (lambda: f.keyframes_get(0), "get"), (lambda: f.keyframes_set_pose(0, np.zeros(12, f32)), "set_pose"),
             (lambda: f.keyframes_align(0), "align"), (f.keyframes_clear, "clear"))
    assert {"ssf_keyframes_" + s for _, s in calls} == set(binding.KEYFRAME_SYMBOLS)
    for call, s in calls:
        with pytest.raises(binding.SsfError, match="ssf_keyframes_" + s + ".*HIP product only"):
            call()


def test_the_keyframe_kernels_read_no_environment_and_use_no_float_atomics():
    txt = open(os.path.join(ROOT, "supersurfel_fusion_amd", "csrc", "ssf_keyframes.hip")).read()
    assert "getenv(" not in txt and "SSF_ENV" not in txt
    assert not re.findall(r"\batomic\w+\s*\(", txt)                  # no atomic at all: every sum is a shuffle or a ballot
    assert "asm" not in txt


@pytest.mark.parametrize("lang", ["c", "c++"])
def test_the_header_compiles_on_its_own(lang, tmp_path):
    src = tmp_path / ("t.c" if lang == "c" else "t.cpp")
    src.write_text('#include "ssf_keyframes.h"\n'
                   "int f(ssf_handle* h, uint8_t* c, ssf_surfels* s, float* p) {\n"
                   "    ssf_keyframes_params q; ssf_keyframe_result r; ssf_fern t[2]; int i = 0, n = 0; int64_t u = 0;\n"
                   "    if (ssf_keyframes_default_params(&q) != SSF_OK) return -1;\n"
                   "    q.cell = 16; q.n_ferns = SSF_KEYFRAMES_MAX_FERNS; q.max_rows = 100; q.loop_ratio = 0.1f;\n"
                   "    return ssf_keyframes_configure(h, &q) + ssf_keyframes_set_ferns(h, t, 2) + ssf_keyframes_get_ferns(h, t, 2) +\n"
                   "           ssf_keyframes_encode(h, c, 2) + ssf_keyframes_query(h, c, 1, -1, SSF_KEYFRAMES_MAX_CANDIDATES, &r) +\n"
                   "           ssf_keyframes_add(h, &i) + ssf_keyframes_consider(h, &r) + ssf_keyframes_put(h, c, s, 0, p, 3, &i) +\n"
                   "           ssf_keyframes_get(h, i, s, 0, &n, p, &n, c) + ssf_keyframes_set_pose(h, i, p) +\n"
                   "           ssf_keyframes_align(h, i, p, 0, p, &n, &n, &n) + ssf_keyframes_info(h, &n, &n, &u, &q) +\n"
                   "           ssf_keyframes_clear(h) + r.candidates[0].loop + (int)sizeof(ssf_fern); }\n")
    cc, std = ("gcc", "-std=c99") if lang == "c" else ("g++", "-std=c++11")
    r = subprocess.run([cc, std, "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", INCLUDE, "-c", str(src), "-o", str(tmp_path / "t.o")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout


def test_the_structures_of_the_binding_match_the_header(tmp_path):
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ssf_keyframes.h"\n'
                   'int main(void) { printf("%d %d %d %d %d\\n", (int)sizeof(ssf_keyframes_params), (int)sizeof(ssf_fern),\n'
                   "    (int)sizeof(ssf_keyframe_result), (int)offsetof(ssf_keyframes_params, max_rows), (int)offsetof(ssf_fern, depth_mm)); return 0; }\n")
    exe = str(tmp_path / "s")
    subprocess.run(["gcc", "-I", INCLUDE, str(src), "-o", exe], check=True)
    out = subprocess.run([exe], stdout=subprocess.PIPE, text=True, check=True).stdout.split()
    import ctypes as C
    assert [int(v) for v in out] == [C.sizeof(binding.SsfKeyframesParams), binding.FERN_DTYPE.itemsize, C.sizeof(binding.SsfKeyframeResult),
                                     binding.SsfKeyframesParams.max_rows.offset, binding.FERN_DTYPE.fields["depth_mm"][1]]


def test_ssf_hpp_keyframe_surface_compiles_and_links_against_the_product(product_lib, tmp_path):
    libdir = os.path.dirname(product_lib.path)
    cmd = ["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", "-I", INCLUDE, "-I", CPP, os.path.join(CPP, "keyframes_smoke.cpp"),
           "-o", str(tmp_path / "keyframes_smoke"), "-L", libdir, "-lssf_hip", "-Wl,-rpath," + libdir]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout


def test_the_default_parameters():
    txt = open(os.path.join(ROOT, "supersurfel_fusion_amd", "csrc", "ssf_keyframes.hip")).read()
    assert "p->cell = 8; p->n_ferns = 500; p->seed = 1234; p->max_keyframes = 256; p->min_gap = 30; p->max_rows = 0;" in txt
    assert "p->new_ratio = 0.3f; p->loop_ratio = 0.2f;" in txt


# ---- the restatement's known answers -------------------------------------------------------------------------------------------
def test_generator_known_answers():
    # splitmix64 from state 0: the published first outputs
    s, z0 = kr.splitmix64(0)
    s, z1 = kr.splitmix64(s)
    assert (z0, z1) == (0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4)
    # the first three ferns of seed 1234 on the 40 x 30 grid of a 320 x 240 image, depth in [200, 5000) mm
    f = kr.generate_ferns(1234, 500, 320, 240, 8, 0.2, 5.0)
    assert [tuple(int(v) for v in e) for e in f[:3].tolist()] == [(35, 14, 218, 51, 165, 0, 2329), (30, 23, 131, 99, 111, 0, 703),
                                                                 (5, 24, 230, 255, 206, 0, 3898)]
    assert f["x"].max() < 40 and f["y"].max() < 30 and f["depth_mm"].min() >= 200 and f["depth_mm"].max() < 5000
    assert np.array_equal(kr.generate_ferns(1234, 3, 320, 240, 8, 0.2, 5.0), f[:3])         # a prefix: six draws per fern, in order
    assert not np.array_equal(kr.generate_ferns(1235, 3, 320, 240, 8, 0.2, 5.0), f[:3])
    assert kr.depth_range_mm(0.2, 5.0) == (200, 5000)


def test_coarse_image_and_codes_known_answers():
    B = 4
    rgb = np.zeros((9, 13, 3), np.uint8)                               # 3 x 2 cells; a column and a row are beyond the grid
    rgb[:4, :4] = (10, 20, 30); rgb[0, 0] = (11, 20, 255)              # cell (0, 0): r (160 + 1 + 8) / 16 = 10, b (480 + 225 + 8) / 16 = 44
    rgb[4:8, 8:12] = 255
    d = np.full((9, 13), np.nan, f32)
    d[:4, :4] = 1.0; d[0, 0] = 0.1; d[0, 1] = np.inf; d[0, 2] = 5.0004997; d[0, 3] = 0.2     # too near, not finite, too far, just inside
    d[4:8, 4:8] = f32(1.2345)                                          # lrintf(1234.5 (f32: 1234.4999...)) = 1234
    mean, cnt, dmm = kr.coarse_image(rgb, d, B, 0.2, 5.0)
    assert mean.shape == (2, 3, 3) and mean[0, 0].tolist() == [10, 20, 44] and mean[1, 2].tolist() == [255, 255, 255]
    assert cnt.tolist() == [[13, 0, 0], [0, 16, 0]]
    assert dmm.tolist() == [[(12 * 1000 + 200 + 6) // 13, 0, 0], [0, int(np.rint(f32(1.2345) * f32(1000))), 0]]
    ferns = np.array([(0, 0, 9, 20, 43, 0, 937), (0, 0, 10, 19, 44, 0, 938), (1, 1, 0, 0, 0, 0, 0), (2, 1, 254, 255, 0, 0, 0),
                      (1, 0, 0, 0, 0, 0, 0)], binding.FERN_DTYPE)
    assert dmm[0, 0] == 938
    #        r > 9, g == 20, b > 43, d > 937 | g > 19 only      | depth only (> 0) | r, b; no depth: cnt == 0 | nothing
    assert kr.encode(ferns, mean, cnt, dmm).tolist() == [1 | 4 | 8, 2, 8, 1 | 4, 0]


def test_packing_round_trip_and_layout():
    rng = np.random.default_rng(4)
    for n in (1, 8, 63, 64, 500, 513, 4096):
        c = rng.integers(0, 16, n).astype(np.uint8)
        w = kr.pack(c)
        assert len(w) % 64 == 0 and len(w) == kr.packed_words(n) and len(w) * 8 >= n > (len(w) - 64) * 8
        assert np.array_equal(kr.unpack(w, n), c)
        assert not w[(n + 7) // 8:].any()
        if n % 8:
            assert w[n // 8] >> np.uint32(4 * (n % 8)) == 0          # the padding nibbles are zero
    assert kr.pack([1, 2, 3, 4, 5, 6, 7, 8, 15])[:2].tolist() == [0x87654321, 0xF]
    assert kr.packed_words(500) == 64 and kr.packed_words(513) == 128


def test_diff_against_a_plain_loop_and_the_packed_form():
    rng = np.random.default_rng(5)
    for n in (1, 63, 500, 513):
        a, b = rng.integers(0, 16, n).astype(np.uint8), rng.integers(0, 16, n).astype(np.uint8)
        b[::3] = a[::3]
        want = 0
        for i in range(n):
            want += 1 if int(a[i]) != int(b[i]) else 0
        assert kr.diff(a, b) == want and kr.diff(a, a) == 0
        x = kr.pack(a) ^ kr.pack(b)                                   # what the search kernel does with the packed words
        x |= x >> np.uint32(1); x |= x >> np.uint32(2)
        assert sum(bin(int(v) & 0x11111111).count("1") for v in x) == want


def test_query_order_ties_gap_and_the_empty_store():
    n = 40
    db = kr.Database(n, min_gap=10, loop_ratio=0.2)
    q = np.zeros(n, np.uint8)
    assert db.query(q, 100) == dict(min_diff_all=n + 1, candidates=[])
    rec = db.consider(q, 0)
    assert rec["added"] and rec["id"] == 0 and rec["min_diff_all"] == n + 1 and rec["candidates"] == [] and rec["n_keyframes"] == 1

    def codes(d):
        c = q.copy(); c[:d] = 7
        return c
    for d, stamp in ((5, 50), (3, 60), (5, 10), (3, 95), (9, 20), (8, 90), (3, 20)):      # ids 1 .. 7
        db.put(codes(d), stamp)
    r = db.query(q, 100)
    # stamp <= 90 only (id 4 is too recent), (diff, id) ascending: equal diffs -> the lower id first
    assert [(c["id"], c["diff"]) for c in r["candidates"]] == [(0, 0), (2, 3), (7, 3), (1, 5), (3, 5), (6, 8), (5, 9)]
    assert [c["loop"] for c in r["candidates"]] == [True, True, True, True, True, True, False]       # 8 / 40 <= 0.2 < 9 / 40
    assert r["min_diff_all"] == 0
    assert [c["id"] for c in db.query(q, 100, k=2)["candidates"]] == [0, 2]
    assert [c["id"] for c in db.query(q, 100, min_gap=0)["candidates"]][:4] == [0, 2, 4, 7]
    assert db.query(q, 5)["candidates"] == [] and db.query(q, 5)["min_diff_all"] == 0      # min_diff_all ignores the gap
    # the ratios are f32 divisions compared with f32 thresholds
    assert kr.loop_flag(100, 500, 0.2) and not kr.loop_flag(101, 500, 0.2)
    d2 = kr.Database(10, new_ratio=0.3)
    d2.put(np.zeros(10, np.uint8), 0)
    three = np.zeros(10, np.uint8); three[:3] = 1
    assert bool(f32(3) / f32(10) >= f32(0.3)) == d2.consider(three, 1)["added"]
    # a full store: the record says so and nothing changes
    d3 = kr.Database(10, max_keyframes=1, new_ratio=0.3)
    d3.put(np.zeros(10, np.uint8), 0)
    r = d3.consider(np.full(10, 5, np.uint8), 9)
    assert r["full"] and not r["added"] and r["id"] == -1 and d3.K == 1 and r["n_keyframes"] == 1
    d4 = kr.Database(10, max_rows=100, new_ratio=0.3)
    assert d4.consider(np.zeros(10, np.uint8), 0, n_rows=60)["added"]
    r = d4.consider(np.full(10, 5, np.uint8), 1, n_rows=41)
    assert r["full"] and d4.K == 1
    assert d4.consider(np.full(10, 5, np.uint8), 1, n_rows=40)["added"]


# ---- the GPU tests' sequence is not trivial (asserted on the restatement, fed by the CPU checker) -------------------------------
def test_the_sequence_adds_keyframes_and_declines_frames(seq_ref):
    recs, codes, db = seq_ref
    added = [i for i, r in enumerate(recs) if r["added"]]
    assert len(added) >= 3 and len(recs) - len(added) >= 3 and not any(r["full"] for r in recs)
    assert [SEQUENCE[i] for i in added] == [0, 5, 10, 45, 90, 180, 270]
    assert [r["id"] for r in recs if r["added"]] == list(range(len(added)))
    assert all(0 < c.sum() < 15 * len(c) for c in codes) and all((c >> 3).any() for c in codes)       # the depth bit is alive
    assert all(n > 100 for n in db.rows)


def test_the_sequence_finds_the_revisit(seq_ref):
    recs, codes, _ = seq_ref
    assert SEQUENCE[REVISIT] == SEQUENCE[0] and REVISIT >= SEQ_PARAMS["min_gap"]
    r = recs[REVISIT]
    assert not r["added"] and r["candidates"], r
    first = r["candidates"][0]
    assert first["id"] == recs[0]["id"] == 0 and first["loop"] and first["stamp"] == 1
    assert first["diff"] == kr.diff(codes[0], codes[REVISIT]) <= 0.2 * 500


def test_the_sequence_never_flags_the_far_side_of_the_room(seq_ref):
    recs, _, _ = seq_ref
    kf_frame = [SEQUENCE[i] for i, r in enumerate(recs) if r["added"]]
    seen = 0
    for i, r in enumerate(recs):
        for c in r["candidates"]:
            apart = abs((SEQUENCE[i] - kf_frame[c["id"]] + 180) % 360 - 180)          # degrees between the two views
            if apart >= 90:
                seen += 1
                assert not c["loop"], (i, c)
    assert seen >= 5                                                  # such candidates do come up (and are turned down)
