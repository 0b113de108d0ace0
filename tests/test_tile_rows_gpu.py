"""The tile-sorted copy of the visible rows (csrc/ssf_tile_rows.inc; TileCopy::make_if_large in csrc/ssf_host.hip), looked at directly.
Every consumer of the copy is order-free, so the frame results cannot tell a sorted copy from an unsorted one: here the sort's own
output (ssf_debug_tile_copy: the records, the bin totals) is compared with the numpy restatement of its key (tests/tile_rows_ref.py,
checked on the CPU by tests/test_tile_rows.py), and the threshold that switches the copy on is crossed in the middle of sequences
whose every result is the oracle's, with ssf_tile_copy_frames saying on which frames the copy was made.  All comparisons are exact."""
import ctypes as C
import functools

import numpy as np
import pytest

import mathops as mo
import tile_rows_ref as tr
import util
from supersurfel_fusion_amd import binding, synthetic

pytestmark = pytest.mark.gpu

F = np.float32
SSF_OK, SSF_ERR_INVALID_ARG, SSF_ERR_STATE = 0, -1, -5


# ---- the sort itself ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def handles(product_lib):
    """one handle per camera, for all cases on it (a case only sets a model: no frame is processed)"""
    made = {}

    def get(W, H):
        if (W, H) not in made:
            S = ((W + 15) // 16) * ((H + 15) // 16)
            cap = max(S, max(tr.SMALL_SIZES if (W, H) == tr.SMALL else tr.OTHER_SIZES))
            made[(W, H)] = binding.Fusion(product_lib, util.make_cfg(product_lib, W, H, nb_supersurfels_max=cap, pipeline_depth=0, extract_batch=1))
        return made[(W, H)]
    yield get
    for f in made.values():
        f.close()


def index_word(out):
    return out["records"].view(np.uint32)[:, 7].astype(np.int64)


def check_sorted_copy(out, stored, ref_bins, nbins, what):
    """the four properties of a sorted copy of `stored` (get_model of the n visible rows) under the reference bins"""
    n = len(ref_bins)
    rec = out["records"].view(np.uint32)
    assert rec.shape == (n, 12) and out["totals"].shape == (nbins,), what
    idx = index_word(out)
    # 1. the index words are a permutation of 0 .. n - 1: no row lost, none twice
    assert np.array_equal(np.sort(idx), np.arange(n)), (what, "rows lost or duplicated", n, len(np.unique(idx)), int(idx.min()), int(idx.max()))
    # 2. record j carries the fields of the row it names, bit for bit
    fields = (("position", rec[:, 0:3], stored["positions"].view(np.uint32)[idx]),
              ("confidence", rec[:, 3], stored["confidences"].view(np.uint32)[idx]),
              ("Lab", rec[:, 4:7], out["lab_src"].view(np.uint32)[idx]),
              ("normal", rec[:, 8:11], np.ascontiguousarray(stored["orientations"][:, 6:9]).view(np.uint32)[idx]),
              ("padding word", rec[:, 11], np.zeros(n, np.uint32)))
    for name, got, want in fields:
        bad = np.flatnonzero((got != want).reshape(n, -1).any(axis=1))
        assert bad.size == 0, (what, name, "of %d records differ, first at output position %d (row %d)" % (bad.size, bad[0], idx[bad[0]]))
    # 3. the reference bin of the row at output position j does not decrease with j
    along = ref_bins[idx]
    down = np.flatnonzero(np.diff(along) < 0)
    assert down.size == 0, (what, "%d descents in the bins along the copy, first at output position %d: bin %d then %d" % (
        down.size, down[0] if down.size else -1, along[down[0]] if down.size else -1, along[down[0] + 1] if down.size else -1))
    # 4. the totals are the reference's counts, so the runs start where the totals say
    want = np.bincount(ref_bins, minlength=nbins)
    bad = np.flatnonzero(out["totals"].astype(np.int64) != want)
    assert bad.size == 0, (what, "totals differ in %d bins, first bin %d: %d, reference %d" % (bad.size, bad[0], out["totals"][bad[0]], want[bad[0]]))


def run_case(f, family, name, W, H, n):
    model, T, _ = tr.case(family, name, W, H, n)
    f.set_model(model, n, 30)
    assert f.counts()["n_visible"] == n
    out = f.debug_tile_copy(T)
    stored = f.get_model(0, n)
    for key in ("positions", "confidences", "orientations"):
        util.assert_same_bits(stored[key].view(np.uint32), np.ascontiguousarray(model[key]).view(np.uint32), "stored " + key)
    ref = tr.bin_of(tr.camera(W, H), T, model["positions"])
    check_sorted_copy(out, stored, ref, tr.geometry(W, H)[2], "%s under %s, %d rows at %d x %d" % (family, name, n, W, H))
    return out, model


@pytest.mark.parametrize("family", sorted(tr.FAMILIES))
@pytest.mark.parametrize("n", tr.SMALL_SIZES)
def test_small_camera(n, family, handles):
    """21 bins; grids of 1, 2, 8, 9, 16 and 18 workgroups, rows that fill the last workgroup, leave one row of it, one short of it"""
    W, H = tr.SMALL
    for name in tr.FAMILIES[family]:
        run_case(handles(W, H), family, name, W, H, n)


@pytest.mark.parametrize("family", ["uniform", "edges"])
@pytest.mark.parametrize("n", tr.OTHER_SIZES)
@pytest.mark.parametrize("shape", tr.OTHER_SHAPES)
def test_other_cameras(shape, n, family, handles):
    """partial tiles (9 bins), two bins, 1057 bins (the scatter's scan of the totals takes a second, partial turn), exactly 4096"""
    W, H = shape
    for name in tr.FAMILIES[family]:
        run_case(handles(W, H), family, name, W, H, n)


def test_the_stored_lab_is_the_lab_of_the_rows(handles, oracle_lib):
    """lab_src, which the records' colours are compared with, is rgb_to_lab of the stored colours (the oracle's, tests/test_math.py)"""
    W, H = tr.SMALL
    out, model = run_case(handles(W, H), "uniform", "oblique", W, H, 4097)
    fn = oracle_lib.lib.ssf_oracle_mathbatch
    fn.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_size_t]; fn.restype = C.c_int
    want = mo.evaluate(fn, "rgb_to_lab", model["colors"])
    mo.assert_same("rgb_to_lab", model["colors"], out["lab_src"].view(np.uint32), want, ("stored Lab", "oracle"))


def test_twice_gives_the_same_bins(handles):
    """the order inside a bin is arbitrary; the totals and the rows of each bin are not"""
    W, H = tr.SMALL
    f = handles(W, H)
    model, T, _ = tr.case("uniform", "oblique", W, H, 9 * 4096)
    f.set_model(model, 9 * 4096, 30)
    a, b = f.debug_tile_copy(T), f.debug_tile_copy(T)
    assert np.array_equal(a["totals"], b["totals"]) and a["totals"].sum() == 9 * 4096
    start = np.concatenate([[0], np.cumsum(a["totals"].astype(np.int64))])
    ia, ib = index_word(a), index_word(b)
    for k in range(len(a["totals"])):
        assert np.array_equal(np.sort(ia[start[k]:start[k + 1]]), np.sort(ib[start[k]:start[k + 1]])), k
    c = f.debug_tile_copy(tr.transform_named("identity"))          # another transform, the same buffers
    assert not np.array_equal(c["totals"], a["totals"])
    check_sorted_copy(c, f.get_model(0, 9 * 4096), tr.bin_of(tr.camera(W, H), tr.transform_named("identity"), model["positions"]), 21, "second transform")


def test_no_visible_rows(handles):
    W, H = tr.SMALL
    f = handles(W, H)
    model, T, _ = tr.case("uniform", "identity", W, H, 63)
    f.set_model(model, 0, 30)
    out = f.debug_tile_copy(T)
    assert out["records"].shape == (0, 12) and out["totals"].shape == (21,) and not out["totals"].any()


def raw_call(lib, h, T, rec, tot, lab=None):
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    return lib.lib.ssf_debug_tile_copy(h, p(T), p(rec), p(tot), p(lab))


def test_refusals(product_lib):
    W, H = tr.SMALL
    T, rec, tot = tr.transform_named("identity"), np.zeros((64, 12), F), np.zeros(21, np.uint32)
    model = tr.case("uniform", "identity", W, H, 63)[0]
    f = binding.Fusion(product_lib, util.make_cfg(product_lib, W, H, nb_supersurfels_max=4096, pipeline_depth=1))
    f.set_model(model, 63, 30)
    assert raw_call(product_lib, None, T, rec, tot) == SSF_ERR_INVALID_ARG
    assert raw_call(product_lib, f.h, None, rec, tot) == SSF_ERR_INVALID_ARG
    assert raw_call(product_lib, f.h, T, None, tot) == SSF_ERR_INVALID_ARG
    assert raw_call(product_lib, f.h, T, rec, None) == SSF_ERR_INVALID_ARG
    assert product_lib.lib.ssf_tile_copy_frames(None) == -1 and f.tile_copy_frames() == 0
    assert raw_call(product_lib, f.h, T, rec, tot) == SSF_OK and tot.sum() == 63          # (lab_src may be NULL)
    # frames pending in the extract pipeline
    f.submit_frame(*util.frame(0, W, H))
    assert raw_call(product_lib, f.h, T, rec, tot) == SSF_ERR_STATE
    f.process_submitted()
    assert f.tile_copy_frames() == 0, "the read-out counted as a frame's copy"
    f.close()
    # a sharded handle
    g = binding.Fusion(product_lib, util.make_cfg(product_lib, W, H, nb_supersurfels_max=4096, rank=0, nranks=2, shard_tile=0.25))
    g.set_model(model, 63, 30)
    assert raw_call(product_lib, g.h, T, rec, tot) == SSF_ERR_STATE
    with pytest.raises(binding.SsfError):
        g.debug_tile_copy(T)
    g.close()


def test_a_frame_too_fine_for_the_histogram(product_lib):
    """2048 x 2048 is 4097 bins, one more than a workgroup's histogram holds: the read-out refuses, and the threshold at 0 leaves the
    copy off -- a frame over 4097 visible rows is tracked without it, with the result of a handle that never sorts.  (Two product
    handles and a flat synthetic wall: the CPU oracle would take many seconds for a frame of this size.)"""
    W, H = tr.TOO_FINE
    assert tr.geometry(W, H)[2] == tr.MAX_BINS + 1
    n = 4097
    model, T, _ = tr.case("uniform", "identity", 2080, 2016, n)
    rng = np.random.default_rng(7)
    rgb = rng.integers(90, 160, (H, W, 3), dtype=np.uint8)
    depth = np.full((H, W), 2.0, F)
    handles, results = [], []
    for threshold in (0, -1):
        f = binding.Fusion(product_lib, util.make_cfg(product_lib, W, H, nb_supersurfels_max=20000, pipeline_depth=0, extract_batch=1))
        f.set_model(model, n, 30)
        f.set_bin_min_rows(threshold)
        rec, tot = np.zeros((n, 12), F), np.zeros(tr.MAX_BINS + 1, np.uint32)
        assert raw_call(product_lib, f.h, T, rec, tot) == SSF_ERR_STATE and not rec.any() and not tot.any()
        results.append(f.process_frame(rgb, depth))
        assert results[-1]["icp_iters"] > 0 and f.tile_copy_frames() == 0
        handles.append(f)
    util.same_result(*results)
    util.compare_state(*handles, maps=False, frame_surfels=False)
    for f in handles:
        f.close()


# ---- frames: the threshold, against the oracle ----------------------------------------------------------------------------------
W, H = 160, 128
NSEED = 30000
SWEEP = tuple(4 * (j if j < 8 else 15 - j) for j in range(16))        # the orbit swept out 28 degrees and back, 4 degrees a frame


@functools.lru_cache(maxsize=None)
def seeded_rows():
    return synthetic.seed_model_cam0(NSEED, W, H, stamp=30)


def seeded(lib, **kw):
    model, nvis = seeded_rows()
    f = binding.Fusion(lib, util.make_cfg(lib, W, H, nb_supersurfels_max=NSEED + 8192, **kw))
    f.set_model(model, nvis, 30)
    return f


@functools.lru_cache(maxsize=None)
def frames(ks):
    return tuple((np.ascontiguousarray(r), np.ascontiguousarray(d)) for r, d in (util.frame(k, W, H, noise=True, holes=0.02) for k in ks))


_oracle = {}


def oracle_run(oracle_lib, ks, priors=None, **kw):
    """the oracle's results, final handle and the series "visible rows before frame k": computed once per case, never modified"""
    key = (ks, priors is not None, tuple(sorted(kw.items())))
    if key not in _oracle:
        fo = seeded(oracle_lib, **kw)
        before, want = [fo.counts()["n_visible"]], []
        for k, (r, d) in enumerate(frames(ks)):
            want.append(fo.process_frame(r, d, prior_pose=None if priors is None else priors[k]))
            before.append(want[-1]["n_visible"])
        _oracle[key] = (want, fo, before[:-1])
    return _oracle[key]


def copies(before, threshold):
    """make_if_large's rule on the series: a frame that iterates (visible rows, icp_iter > 0) with `threshold` visible rows or more"""
    return [b > 0 and b >= threshold for b in before]


def crossing(oracle_lib):
    """the sweep, the oracle's run of it and a threshold strictly inside the series' range that the series crosses upward and downward
    after the first tracked frame (checked on the oracle alone)"""
    want, fo, before = oracle_run(oracle_lib, SWEEP)
    assert all(r["icp_iters"] > 0 for r in want)
    threshold = (min(before) + max(before)) // 2
    assert min(before) < threshold < max(before), before
    on = copies(before, threshold)
    ups = [k for k in range(2, len(on)) if on[k] and not on[k - 1]]
    downs = [k for k in range(2, len(on)) if not on[k] and on[k - 1]]
    assert ups and downs and 0 < sum(on) < len(on), (before, threshold)
    return want, fo, before, threshold, on


def check(want, fo, got, fh):
    for a, b in zip(want, got):
        util.same_result(a, b)
    util.compare_state(fo, fh, maps=False, frame_surfels=False)


@pytest.mark.parametrize("pipelined", [False, True])
def test_the_threshold_is_crossed_both_ways(pipelined, oracle_lib, product_lib):
    """16 frames over a seeded map; the visible rows rise past the threshold and fall below it again.  Pipelined, the first copy's
    buffers are allocated with frames in flight."""
    want, fo, before, threshold, on = crossing(oracle_lib)
    fh = seeded(product_lib, **(dict(pipeline_depth=2, extract_batch=2) if pipelined else {}))
    fh.set_bin_min_rows(threshold)
    fr = frames(SWEEP)
    got = fh.process_sequence([r.ctypes.data for r, _ in fr], [d.ctypes.data for _, d in fr], on_device=False) if pipelined \
        else [fh.process_frame(r, d) for r, d in fr]
    check(want, fo, got, fh)
    assert fh.tile_copy_frames() == sum(on), (fh.tile_copy_frames(), before, threshold)
    assert 0 < sum(on) < len(SWEEP)
    fh.close()


def test_the_copy_switches_the_resident_launch_off_and_on(oracle_lib, product_lib):
    """frame by frame on one handle: a frame below the threshold takes the resident ICP launch (the settings of
    tests/test_icp_resident_gpu.py: one frame in flight, no pre-filter), a frame at or above it makes the copy instead"""
    want, fo, before, threshold, on = crossing(oracle_lib)
    fh = seeded(product_lib)
    fh.set_bin_min_rows(threshold)
    got = []
    for k, (r, d) in enumerate(frames(SWEEP)):
        c0, r0 = fh.tile_copy_frames(), fh.resident_icp_frames()
        got.append(fh.process_frame(r, d))
        assert (fh.tile_copy_frames() - c0, fh.resident_icp_frames() - r0) == ((1, 0) if on[k] else (0, 1)), (k, before[k], threshold)
    check(want, fo, got, fh)
    assert fh.tile_copy_frames() > 0 and fh.resident_icp_frames() > 0
    assert fh.tile_copy_frames() + fh.resident_icp_frames() == len(SWEEP)
    fh.close()


def test_at_the_threshold_is_above_it(oracle_lib, product_lib):
    """n_visible >= min_rows: a threshold of exactly the visible rows makes the copy, one more does not"""
    want, fo, before = oracle_run(oracle_lib, (0,))
    nvis = before[0]
    assert nvis == seeded_rows()[1] > 1000 and want[0]["icp_iters"] > 0
    for threshold, made in ((nvis, 1), (nvis + 1, 0)):
        fh = seeded(product_lib)
        fh.set_bin_min_rows(threshold)
        got = [fh.process_frame(*frames((0,))[0])]
        check(want, fo, got, fh)
        assert fh.tile_copy_frames() == made, (threshold, nvis)
        fh.close()


def test_the_pre_filter_in_the_frame_with_the_copy_forced(oracle_lib, product_lib):
    ks = tuple(range(5))
    want, fo, before = oracle_run(oracle_lib, ks, depth_prefilter=1)
    fh = seeded(product_lib, depth_prefilter=1)
    fh.set_bin_min_rows(0)
    got = [fh.process_frame(r, d) for r, d in frames(ks)]
    check(want, fo, got, fh)
    assert fh.tile_copy_frames() == sum(1 for r in got if r["icp_iters"] > 0) == len(ks)
    fh.close()


def test_a_prior_pose_is_the_sort_key(oracle_lib, product_lib):
    """the rows are sorted under the frame's INITIAL transform: with a prior a few centimetres and degrees off the final pose the
    key is the prior, and the results are still the oracle's"""
    ks = tuple(range(5))
    a = np.deg2rad(2.5)
    off = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]) @ synthetic.rot_x(np.deg2rad(-1.5))
    priors = tuple(synthetic.pose12(synthetic.relative_pose(k)[0] @ off, synthetic.relative_pose(k)[1] + np.array([0.03, -0.02, 0.04])) for k in ks)
    want, fo, before = oracle_run(oracle_lib, ks, priors=priors)
    moved = [float(np.abs(r["pose"] - p).max()) for r, p in zip(want, priors)]
    assert all(r["icp_iters"] > 1 for r in want) and max(moved) > 0.01, moved
    fh = seeded(product_lib)
    fh.set_bin_min_rows(0)
    got = [fh.process_frame(r, d, prior_pose=priors[k]) for k, (r, d) in enumerate(frames(ks))]
    check(want, fo, got, fh)
    assert fh.tile_copy_frames() == len(ks)
    fh.close()


@pytest.mark.parametrize("forced", [False, True])
def test_the_read_out_between_frames_changes_nothing(forced, product_lib):
    """two product handles on the same frames, one of them read out between the frames (with the copy forced its buffers are the
    frames' own): every later frame result and the final state agree to the bit"""
    ks = tuple(range(4))
    fa, fb = seeded(product_lib), seeded(product_lib)
    if forced:
        fa.set_bin_min_rows(0); fb.set_bin_min_rows(0)
    cam = tr.camera(W, H)
    for k, (r, d) in enumerate(frames(ks)):
        T = tr.transform_named(("oblique", "identity", "nan")[k % 3])
        out = fa.debug_tile_copy(T)
        n = fa.counts()["n_visible"]
        stored = fa.get_model(0, n)
        check_sorted_copy(out, stored, tr.bin_of(cam, T, stored["positions"]), 21, "between frames, before frame %d" % k)
        util.same_result(fa.process_frame(r, d), fb.process_frame(r, d))
    util.compare_state(fa, fb)
    assert fa.tile_copy_frames() == fb.tile_copy_frames() == (len(ks) if forced else 0)
    fa.close(); fb.close()
