"""The fern-coded keyframe database (include/ssf_keyframes.h) on the GPU: the product against the numpy restatement
(tests/keyframe_ref.py).  Every comparison is an equality of integers or bits; there is no tolerance in this file.  The sequence
of frames and its parameters are tests/test_keyframes.py's, where the restatement alone proves them non-trivial."""
import os
import subprocess

import numpy as np
import pytest

import keyframe_ref as kr
import test_align as ta
import test_keyframes as tk
import util
from conftest import ROOT
from supersurfel_fusion_amd import binding, replay, synthetic

pytestmark = pytest.mark.gpu
f32 = np.float32
GOLD = os.path.join(ROOT, "tests", "golden")
CELLS = (4, 8, 16)
FERN_COUNTS = (1, 63, 64, 500, 513)
SMALL = dict(max_keyframes=2, max_rows=1)          # encode-only databases: no pool worth the name


def record_of(rec):
    return {k: rec[k] for k in ("added", "id", "full", "min_diff_all", "n_keyframes", "candidates")}


def check_encode(f, rgb, what):
    """every (B, n) on the handle's current frame: the generated ferns and the codes equal the restatement's"""
    pd = f.plane_depth()
    for B in CELLS:
        for n in FERN_COUNTS:
            f.keyframes_configure(cell=B, n_ferns=n, seed=77 + n, **SMALL)
            ferns = kr.generate_ferns(77 + n, n, f.W, f.H, B, f.cfg.range_min, f.cfg.range_max)
            got = f.keyframes_get_ferns()
            assert got.tobytes() == ferns.tobytes(), (what, B, n)
            want = kr.encode_frame(ferns, rgb, pd, B, f.cfg.range_min, f.cfg.range_max)
            codes = f.keyframes_encode()
            assert codes.dtype == np.uint8 and np.array_equal(codes, want), (what, B, n, int((codes != want).sum()))
            assert np.array_equal(f.keyframes_encode(), codes)
            f.keyframes_clear()
    return pd


@pytest.mark.parametrize("size", [(320, 240), (640, 480)])
def test_encode_on_orbit_frames(size, product_lib):
    W, H = size
    f = binding.Fusion(product_lib, util.make_cfg(product_lib, W, H))
    for k, holes in ((0, 0.0), (7, 0.15)):
        R, t = synthetic.orbit_pose(k)
        rgb, depth, _ = synthetic.render(R, t, W, H, noise=True, holes=holes, rng=np.random.default_rng(1000 + k))
        f.process_frame(rgb, depth)
        pd = check_encode(f, rgb, "orbit %d" % k)
    assert (~np.isfinite(pd)).any()                                  # the sentinel planes were part of it


def test_encode_on_the_real_frames(product_lib):
    path = os.path.join(GOLD, "tum_fr1_xyz_8frames.npz")
    f = binding.Fusion(product_lib, product_lib.default_config(**dict(replay.BENCHMARK_LAUNCH, nb_supersurfels_max=20000)))
    n_frames, holes = 0, 0
    for stamp, rgb, depth in replay.frames_from_npz(path):
        f.process_frame(rgb, depth)
        pd = check_encode(f, rgb, "fr1_xyz " + stamp)
        holes += int((~np.isfinite(pd)).sum())
        n_frames += 1
    assert n_frames == 8 and holes > 0


def test_encode_of_raw_sensor_frames_gives_the_same_codes(product_lib):
    W, H = 320, 240
    rgb, depth = util.frame(4, W, H)
    d16 = np.clip(np.rint(depth.astype(np.float64) * 5000.0), 0, 65535).astype(np.uint16)
    d32 = replay.convert_depth(d16, 0.0002)
    fa = binding.Fusion(product_lib, util.make_cfg(product_lib, W, H))
    fb = binding.Fusion(product_lib, util.make_cfg(product_lib, W, H))
    fb.set_input_format("bgr8", "u16", 0.0002)
    fa.process_frame(rgb, d32)
    fb.process_frame(np.ascontiguousarray(rgb[..., ::-1]), d16)
    for f in (fa, fb):
        f.keyframes_configure(**SMALL)
    ca, cb = fa.keyframes_encode(), fb.keyframes_encode()
    ferns = kr.generate_ferns(1234, 500, W, H, 8, fa.cfg.range_min, fa.cfg.range_max)
    assert np.array_equal(ca, cb) and np.array_equal(ca, kr.encode_frame(ferns, rgb, fa.plane_depth(), 8, fa.cfg.range_min, fa.cfg.range_max))


@pytest.mark.parametrize("n", [500, 513])
def test_query_at_scale(n, product_lib):
    K = 5000
    rng = np.random.default_rng(21)
    f = binding.Fusion(product_lib, util.make_cfg(product_lib, 160, 128))
    f.keyframes_configure(n_ferns=n, max_keyframes=K, max_rows=8, min_gap=40, loop_ratio=0.2)
    query = rng.integers(0, 16, n).astype(np.uint8)
    codes = rng.integers(0, 16, (K, n)).astype(np.uint8)
    near = rng.choice(K, 400, replace=False)
    for j, i in enumerate(near):                                     # near views: the query with a few ferns changed
        codes[i] = query
        d = (0, 3, 3, 3, 5, 5, 17, 17, 40, 41)[j % 10] if j < 20 else int(rng.integers(6, n // 2))
        idx = rng.choice(n, d, replace=False)
        codes[i, idx] = (query[idx] + 1 + rng.integers(0, 15, d)) % 16      # each one differs: diff == d exactly
    stamps = rng.integers(-1000, 100000, K)
    stamps[near[:5]] = (99960, 99961, 50, 50, 100000)                # on both sides of the gap
    pose = np.arange(12, dtype=f32)
    db = kr.Database(n, max_keyframes=K, min_gap=40, loop_ratio=0.2)
    for i in range(K):
        assert f.keyframes_put(codes[i], None, pose, int(stamps[i])) == i
    db.codes, db.stamps, db.rows = codes, [int(s) for s in stamps], [0] * K
    assert f.keyframes_info()["n_keyframes"] == K
    for stamp, gap, k in ((100000, -1, 8), (100000, 0, 8), (100000, 39, 8), (100000, 41, 5), (60, 10, 8), (60, 0, 1), (-5000, 0, 8),
                          (2 ** 31 - 1, 0, 8), (-2 ** 31, 2 ** 31 - 1, 8), (100000, 5, 0)):
        want = db.query(query, stamp, None if gap < 0 else gap, k)
        got = f.keyframes_query(query, stamp, gap, k)
        assert got["min_diff_all"] == want["min_diff_all"] == 0 and got["candidates"] == want["candidates"], (stamp, gap, k, got, want)
        assert not got["added"] and got["id"] == -1 and not got["full"] and got["n_keyframes"] == K
        again = f.keyframes_query(query, stamp, gap, k)
        assert again == got                                          # twice in a row: the same bytes
    full = f.keyframes_query(query, 100000, 0, 8)["candidates"]
    assert [c["diff"] for c in full] == sorted(c["diff"] for c in full) and len(full) == 8
    top = f.keyframes_query(query, 10 ** 6, 0, 8)["candidates"]       # two keyframes at diff 0, six at diff 3: ties decided by id
    assert [c["diff"] for c in top] == [0, 0, 3, 3, 3, 3, 3, 3]
    assert [c["id"] for c in top[:2]] == sorted(c["id"] for c in top[:2]) and [c["id"] for c in top[2:]] == sorted(c["id"] for c in top[2:])
    # another query vector: nothing planted around it
    other = rng.integers(0, 16, n).astype(np.uint8)
    assert f.keyframes_query(other, 100000, 0, 8)["candidates"] == db.query(other, 100000, 0, 8)["candidates"]
    assert f.keyframes_query(other, 100000, 0, 8)["min_diff_all"] == db.query(other, 100000, 0, 8)["min_diff_all"] > 0
    # the store is full now
    with pytest.raises(binding.SsfError, match=r"\(-4\).*full"):
        f.keyframes_put(query, None, pose, 0)
    g = f.keyframes_get(int(near[0]))
    assert np.array_equal(g["codes"], codes[near[0]]) and g["stamp"] == stamps[near[0]] and np.array_equal(g["pose"], pose)
    assert len(g["rows"]["confidences"]) == 0


def test_consider_over_the_proven_sequence(oracle_lib, product_lib):
    W, H = tk.SEQ_SIZE
    oracle_recs, oracle_codes, _ = tk.reference_records(oracle_lib)  # what the CPU tests assert (a) - (c) on
    cfg = util.make_cfg(product_lib, W, H)
    ferns = kr.generate_ferns(tk.SEQ_PARAMS["seed"], tk.SEQ_PARAMS["n_ferns"], W, H, tk.SEQ_PARAMS["cell"], cfg.range_min, cfg.range_max)
    db = kr.Database(500, min_gap=tk.SEQ_PARAMS["min_gap"], new_ratio=tk.SEQ_PARAMS["new_ratio"], loop_ratio=tk.SEQ_PARAMS["loop_ratio"])
    f = binding.Fusion(product_lib, cfg)
    f.keyframes_configure(**tk.SEQ_PARAMS)
    stored = {}
    for i, k in enumerate(tk.SEQUENCE):
        rgb, depth = util.frame(k, W, H)
        f.process_frame(rgb, depth)
        fr = f.get_frame()
        keep = fr["confidences"] > 0
        codes = kr.encode_frame(ferns, rgb, f.plane_depth(), 8, cfg.range_min, cfg.range_max)
        want = db.consider(codes, f.counts()["stamp"], int(keep.sum()))
        assert np.array_equal(f.keyframes_encode(), codes) and np.array_equal(codes, oracle_codes[i])
        assert record_of(f.keyframes_query()) == dict(want, added=False, id=-1, full=False, n_keyframes=want["n_keyframes"] - int(want["added"]))
        got = f.keyframes_consider()
        assert record_of(got) == want == oracle_recs[i], (i, got, want)
        if got["added"]:
            stored[got["id"]] = ({name: fr[name][keep] for name in fr}, f.get_pose(), f.counts()["stamp"], codes)
    assert len(stored) == 7 and f.keyframes_info()["n_keyframes"] == 7
    assert f.keyframes_info()["rows_used"] == sum(len(s[0]["confidences"]) for s in stored.values())
    for kid, (rows, pose, stamp, codes) in stored.items():           # after all the later frames: nothing was overwritten
        g = f.keyframes_get(kid)
        assert g["stamp"] == stamp and np.array_equal(g["codes"], codes)
        util.assert_same_bits(g["pose"], pose, "keyframe pose")
        assert 100 < len(rows["confidences"]) <= f.S
        for name in rows:
            util.assert_same_bits(g["rows"][name], rows[name], "keyframe %d %s" % (kid, name))
    moved = np.arange(12, dtype=f32)
    f.keyframes_set_pose(3, moved)
    assert np.array_equal(f.keyframes_get(3)["pose"], moved)
    util.assert_same_bits(f.keyframes_get(2)["pose"], stored[2][1], "the neighbour's pose")


def test_align_from_the_store(product_lib):
    W, H = 320, 240
    f = binding.Fusion(product_lib, util.make_cfg(product_lib, W, H))
    f.keyframes_configure()
    f.process_frame(*util.frame(0, W, H))
    assert f.keyframes_consider()["added"]
    for k in (1, 2, 3):
        f.process_frame(*util.frame(k, W, H))
    Rk, tk_ = synthetic.orbit_pose(0); Rc, tc = synthetic.orbit_pose(3)
    gt = synthetic.pose12(Rc.T @ Rk, Rc.T @ (tk_ - tc))
    rows = f.keyframes_get(0)["rows"]
    src = {name: rows[name] for name in ("positions", "colors", "orientations")}
    for init in (ta.perturbed(gt), ta.perturbed(gt, seed=9), None):
        a, b = f.align(src, init), f.keyframes_align(0, init)
        assert (a["valid"], a["iters"], a["pairs"]) == (b["valid"], b["iters"], b["pairs"]), (a, b)
        util.assert_same_bits(a["rel_pose"], b["rel_pose"], "align rel_pose")
    a, b = f.align(dict(src, confidences=rows["confidences"]), ta.perturbed(gt)), f.keyframes_align(0, ta.perturbed(gt), use_conf=True)
    assert (a["valid"], a["iters"], a["pairs"]) == (b["valid"], b["iters"], b["pairs"])
    util.assert_same_bits(a["rel_pose"], b["rel_pose"], "align rel_pose (stored confidences)")
    # the pair of test_align.py (keyframe 0 against frame 3, the same prior): the same recovery
    init = ta.perturbed(gt)
    out = f.keyframes_align(0, init)
    assert out["valid"] and out["iters"] == 10 and out["pairs"] > 100
    Rr = out["rel_pose"][:9].reshape(3, 3).astype(np.float64); tr = out["rel_pose"][9:].astype(np.float64)
    Ri = init[:9].reshape(3, 3).astype(np.float64); ti = init[9:].astype(np.float64)
    R_est = Rr.T @ Ri; t_est = Rr.T @ (ti - tr)
    Rg = gt[:9].reshape(3, 3); tg = gt[9:]
    ang = np.degrees(np.arccos(np.clip((np.trace(R_est @ Rg.T) - 1) / 2, -1, 1)))
    assert np.linalg.norm(t_est - tg) < 0.6 * np.linalg.norm(ti - tg) and ang < 0.5
    far = gt.copy(); far[9:] += 2.0
    out = f.keyframes_align(0, far)
    assert not out["valid"] and out["iters"] == 1 and out["pairs"] < 100


def test_consider_between_frames_changes_no_pose_or_model_bit(product_lib):
    W, H = 320, 240
    fa = binding.Fusion(product_lib, util.make_cfg(product_lib, W, H))
    fb = binding.Fusion(product_lib, util.make_cfg(product_lib, W, H))
    fb.keyframes_configure(min_gap=1, new_ratio=0.05)
    n_added = 0
    for k in range(6):
        rgb, depth = util.frame(2 * k, W, H)
        util.same_result(fa.process_frame(rgb, depth), fb.process_frame(rgb, depth))
        rec = fb.keyframes_consider()
        n_added += int(rec["added"])
        for c in rec["candidates"]:
            fb.keyframes_align(c["id"])
        fb.keyframes_query(min_gap=0)
    assert n_added >= 3
    util.compare_state(fa, fb)


def test_put_get_round_trip_and_own_ferns(product_lib):
    W, H = 320, 240
    f = binding.Fusion(product_lib, util.make_cfg(product_lib, W, H))
    f.keyframes_configure(n_ferns=63, max_keyframes=4, max_rows=1000)
    rng = np.random.default_rng(8)
    ferns = np.zeros(63, binding.FERN_DTYPE)
    ferns["x"] = rng.integers(0, W // 8, 63); ferns["y"] = rng.integers(0, H // 8, 63)
    for c in "rgb":
        ferns[c] = rng.integers(0, 256, 63)
    ferns["depth_mm"] = rng.integers(200, 5000, 63)
    f.keyframes_set_ferns(ferns)
    assert f.keyframes_get_ferns().tobytes() == ferns.tobytes()
    rgb, depth = util.frame(0, W, H)
    f.process_frame(rgb, depth)
    want = kr.encode_frame(ferns, rgb, f.plane_depth(), 8, f.cfg.range_min, f.cfg.range_max)
    assert np.array_equal(f.keyframes_encode(), want)
    bad = ferns.copy(); bad["x"][5] = W // 8
    with pytest.raises(binding.SsfError, match="outside"):
        f.keyframes_set_ferns(bad)
    kid = f.keyframes_add()
    assert kid == 0
    with pytest.raises(binding.SsfError, match="stored under the present table"):
        f.keyframes_set_ferns(ferns)
    a = f.keyframes_get(0)
    assert np.array_equal(a["codes"], want)
    kid = f.keyframes_put(a["codes"], a["rows"], a["pose"], -3)
    b = f.keyframes_get(kid)
    assert kid == 1 and b["stamp"] == -3 and np.array_equal(b["codes"], a["codes"])
    for name in a["rows"]:
        util.assert_same_bits(a["rows"][name], b["rows"][name], "round trip " + name)
    r = f.keyframes_query(min_gap=0)
    assert [(c["id"], c["diff"]) for c in r["candidates"]] == [(0, 0), (1, 0)]


def test_refusals(product_lib):
    W, H = 160, 128
    f = binding.Fusion(product_lib, util.make_cfg(product_lib, W, H))
    for call in (f.keyframes_consider, f.keyframes_encode, f.keyframes_add, f.keyframes_query, lambda: f.keyframes_get(0),
                 lambda: f.keyframes_align(0), f.keyframes_get_ferns):
        with pytest.raises(binding.SsfError, match=r"\(-5\).*ssf_keyframes_configure"):      # SSF_ERR_STATE before configure
            call()
    assert f.keyframes_info() == dict(configured=False, n_keyframes=0, rows_used=0, params=dict.fromkeys(
        ("cell", "n_ferns", "seed", "max_keyframes", "min_gap", "max_rows", "new_ratio", "loop_ratio"), 0))
    for bad in (dict(cell=5), dict(cell=32), dict(n_ferns=0), dict(n_ferns=4097), dict(max_keyframes=0), dict(min_gap=-1), dict(max_rows=-1),
                dict(new_ratio=float("nan")), dict(loop_ratio=float("inf"))):
        with pytest.raises(binding.SsfError, match=r"ssf_keyframes_configure failed \(-1\)"):
            f.keyframes_configure(**bad)
    f.keyframes_configure(max_keyframes=2)
    info = f.keyframes_info()
    assert info["configured"] and info["params"]["max_rows"] == 2 * f.S and info["params"]["n_ferns"] == 500
    with pytest.raises(binding.SsfError, match=r"\(-5\).*live"):
        f.keyframes_configure()
    for call in (f.keyframes_consider, f.keyframes_encode, f.keyframes_add, f.keyframes_query):
        with pytest.raises(binding.SsfError, match=r"\(-5\).*no frame"):
            call()
    for k in range(2):
        f.process_frame(*util.frame(k, W, H))
        assert f.keyframes_add() == k
    for call in (lambda: f.keyframes_get(2), lambda: f.keyframes_get(-1), lambda: f.keyframes_align(2), lambda: f.keyframes_set_pose(7, np.zeros(12, f32))):
        with pytest.raises(binding.SsfError, match=r"\(-1\).*no keyframe"):
            call()
    with pytest.raises(binding.SsfError, match=r"\(-1\)"):
        f.keyframes_query(np.full(500, 16, np.uint8), 5)
    # a full store: the explicit add is refused, consider reports it, nothing changes
    f.process_frame(*util.frame(60, W, H))
    before = [f.keyframes_get(k) for k in range(2)]
    with pytest.raises(binding.SsfError, match=r"ssf_keyframes_add failed \(-4\).*full"):
        f.keyframes_add()
    rec = f.keyframes_consider()
    assert rec["full"] and not rec["added"] and rec["id"] == -1 and rec["n_keyframes"] == 2
    assert f.keyframes_info()["n_keyframes"] == 2
    for k in range(2):
        g = f.keyframes_get(k)
        assert np.array_equal(g["codes"], before[k]["codes"]) and g["stamp"] == before[k]["stamp"]
        util.assert_same_bits(g["rows"]["positions"], before[k]["rows"]["positions"], "rows of a full store")
    # frames pending in the extract pipeline
    fp = binding.Fusion(product_lib, util.make_cfg(product_lib, W, H, pipeline_depth=1, extract_batch=1))
    fp.keyframes_configure()
    frames = [util.frame(k, W, H) for k in range(2)]
    fp.submit_frame(*frames[0])
    with pytest.raises(binding.SsfError, match=r"\(-5\).*pending"):
        fp.keyframes_consider()
    fp.process_submitted()
    assert fp.keyframes_consider()["added"]
    # a frame that came in as tables has no colour map
    ft = binding.Fusion(product_lib, util.make_cfg(product_lib, W, H))
    ft.keyframes_configure()
    ft.submit_frame_tables(f.index_map(), f.plane_depth(), f.get_frame())
    ft.process_submitted()
    with pytest.raises(binding.SsfError, match=r"\(-5\).*colour map"):
        ft.keyframes_consider()
    ft.process_frame(*util.frame(1, W, H))
    assert ft.keyframes_consider()["added"]
    # a sharded handle
    fs = binding.Fusion(product_lib, util.make_cfg(product_lib, W, H, rank=0, nranks=2))
    with pytest.raises(binding.SsfError, match=r"\(-5\).*sharded"):
        fs.keyframes_configure()
    # clear, then reuse
    f.keyframes_clear()
    assert not f.keyframes_info()["configured"]
    with pytest.raises(binding.SsfError, match=r"\(-5\).*ssf_keyframes_configure"):
        f.keyframes_consider()
    f.keyframes_configure(cell=16, n_ferns=64, max_keyframes=3)
    rec = f.keyframes_consider()
    assert rec["added"] and rec["id"] == 0 and rec["min_diff_all"] == 65 and f.keyframes_info()["n_keyframes"] == 1


def test_kernel_times_appear_under_profile(product_lib):
    W, H = 320, 240
    f = binding.Fusion(product_lib, util.make_cfg(product_lib, W, H, profile=1))
    f.keyframes_configure(min_gap=0)
    for k in (0, 1):
        f.process_frame(*util.frame(k, W, H))
        f.keyframes_consider()
    f.keyframes_align(0)
    t = f.kernel_times(128)
    for name in ("kf_encode", "kf_search", "kf_select", "kf_align_prep"):
        assert name in t and t[name][1] >= 1, (name, sorted(t))
    assert t["kf_encode"][1] == 2 and t["kf_search"][1] == 1


def fnv(*arrays):
    h = 1469598103934665603
    for a in arrays:
        for b in np.ascontiguousarray(a).tobytes():
            h = ((h ^ b) * 1099511628211) & ((1 << 64) - 1)
    return h


def test_keyframes_smoke_cpp_agrees_with_the_python_mirror(product_lib, tmp_path):
    W, H, n = 320, 240, 5
    frames = [util.frame(k, W, H) for k in (0, 1, 8, 16, 0)]
    raw = tmp_path / "frames.bin"
    with open(raw, "wb") as fh:
        for rgb, depth in frames:
            fh.write(np.ascontiguousarray(rgb, np.uint8).tobytes()); fh.write(np.ascontiguousarray(depth, f32).tobytes())
    exe = tmp_path / "keyframes_smoke"
    libdir = os.path.dirname(product_lib.path)
    cmd = ["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "keyframes_smoke.cpp"), "-o", str(exe), "-L", libdir, "-lssf_hip", "-Wl,-rpath," + libdir]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    K = synthetic.intrinsics(W, H)
    r = subprocess.run([str(exe), str(W), str(H), str(n), str(raw)] + [repr(float(K[k])) for k in ("fx", "fy", "cx", "cy")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    lines = r.stdout.strip().splitlines()
    f = binding.Fusion(product_lib, product_lib.default_config(nb_supersurfels_max=50000, lambda_pos=10.0, lambda_bound=1000.0,
                                                               lambda_size=1000.0, lambda_disp=1e8,
                                                               **{k: K[k] for k in ("width", "height", "fx", "fy", "cx", "cy")}))
    f.keyframes_configure(min_gap=2, max_keyframes=16)
    ferns = f.keyframes_get_ferns()
    assert lines[0] == "ferns %d %016x" % (len(ferns), fnv(ferns))
    for k, (rgb, depth) in enumerate(frames):
        f.process_frame(rgb, depth)
        rec = f.keyframes_consider()
        want = "frame %d added=%d id=%d full=%d min=%d n=%d cand=%d" % (k, rec["added"], rec["id"], rec["full"], rec["min_diff_all"],
                                                                        rec["n_keyframes"], len(rec["candidates"]))
        want += "".join(" (%d %d %d %d)" % (c["id"], c["diff"], c["stamp"], c["loop"]) for c in rec["candidates"])
        assert lines[1 + k] == want
    assert "cand=0" not in lines[n] and lines[n].split("(")[1].startswith("0 ")      # the revisit names keyframe 0 first
    q = f.keyframes_query(f.keyframes_encode(), 1000, 0, 3)
    assert lines[n + 1] == "query min=%d cand=%d first=%d" % (q["min_diff_all"], len(q["candidates"]), q["candidates"][0]["id"])
    g = f.keyframes_get(0)
    assert lines[n + 2] == "keyframe0 rows=%d stamp=%d %016x" % (len(g["rows"]["confidences"]), g["stamp"],
                                                                fnv(g["rows"]["positions"], g["rows"]["orientations"], g["codes"]))
    a = f.keyframes_align(0)
    assert lines[n + 3] == "align valid=%d iters=%d pairs=%d %016x" % (a["valid"], a["iters"], a["pairs"], fnv(a["rel_pose"]))
    assert a["valid"]                                                # the same view, no prior needed
    assert lines[n + 4] == "put id=%d n=%d" % (f.keyframes_info()["n_keyframes"], f.keyframes_info()["n_keyframes"] + 1)
    assert lines[n + 5] == "refused_after_clear 1"


def test_replay_keeps_a_keyframe_log(product_lib, tmp_path):
    path = os.path.join(GOLD, "tum_fr1_xyz_8frames.npz")
    cfg = dict(replay.BENCHMARK_LAUNCH, nb_supersurfels_max=20000)
    fa = binding.Fusion(product_lib, product_lib.default_config(**cfg))
    fb = binding.Fusion(product_lib, product_lib.default_config(**cfg))
    la, _ = replay.replay(fa, replay.frames_from_npz(path))
    log = tmp_path / "keyframes.txt"
    lb, _ = replay.replay(fb, replay.frames_from_npz(path), keyframes=dict(min_gap=2, new_ratio=0.01, loop_ratio=1.0), keyframe_log=str(log))
    assert la == lb                                                  # the trajectory does not notice
    lines = log.read_text().splitlines()
    stamps = [s for s, _, _ in replay.frames_from_npz(path)]
    assert lines == fb.keyframe_lines and [l.split()[0] for l in lines] == stamps
    assert lines[0].split()[1:] == ["0", "501"]                      # the first frame is stored; nothing to compare it with
    stored = [l.split()[1] for l in lines]
    assert [s for s in stored if s != "-"] == [str(k) for k in range(fb.keyframes_info()["n_keyframes"])]
    verdicts = [w for l in lines[2:] for w in l.split()[3:]]
    assert verdicts and all(w.count(":") == 3 and w.split(":")[2] in ("valid", "invalid") for w in verdicts)
    assert any(w.split(":")[2] == "valid" for w in verdicts)         # consecutive real frames do register
    fp = binding.Fusion(product_lib, product_lib.default_config(pipeline_depth=2, extract_batch=4, **cfg))
    with pytest.raises(ValueError, match="pipelined"):
        replay.replay(fp, replay.frames_from_npz(path), pipelined=True, keyframes={})
