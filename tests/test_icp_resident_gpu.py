"""The resident ICP launch (include/ssf_track.h, k_icp_resident in csrc/ssf_track_fuse.hip): on a single shard, for a frame
without a tile-sorted copy of its rows, the iterations of a frame and its association run in ONE launch whose lanes keep their
rows in registers and are sent one word per iteration.  The sums are exact integers and the association takes minima: every
result must be the oracle's to the bit, whichever path a frame takes -- and the tests that expect the resident path check that
it was taken (ssf_resident_icp_frames, ssf_waiter_matches).

Small frames (160x128, 320x240) over a seeded model cut to an exact number of visible rows: the visible rows lead the seeded
arrays, so the first frame's launch has exactly that many rows (a partial last workgroup, which is also the collector)."""
import ctypes as C
import functools

import numpy as np
import pytest

import util
from supersurfel_fusion_amd import binding, synthetic

pytestmark = pytest.mark.gpu

W, H = 160, 128
NF = 4


@functools.lru_cache(maxsize=None)
def seeded_rows(width, height):
    model, nvis = synthetic.seed_model_cam0(30000, width, height, stamp=30)
    assert nvis >= 1000, nvis
    return model, nvis


def handle(lib, n_visible, width=W, height=H, tail=0, **kw):
    """a handle whose model is the first n_visible VISIBLE seeded rows (and `tail` rows from the out-of-view end)"""
    model, nvis = seeded_rows(width, height)
    rows = {k: np.concatenate([v[:n_visible], v[nvis:nvis + tail]]) for k, v in model.items()}
    f = binding.Fusion(lib, util.make_cfg(lib, width, height, nb_supersurfels_max=16384, **kw))
    f.set_model(rows, n_visible, 30)
    return f


@functools.lru_cache(maxsize=None)
def frames(width=W, height=H, n=NF):
    return tuple((np.ascontiguousarray(r), np.ascontiguousarray(d)) for r, d in
                 (util.frame(k, width, height, noise=True, holes=0.02) for k in range(n)))


_oracle = {}


def oracle_run(oracle_lib, n_visible, width=W, height=H, tail=0, priors=None, n=NF, **kw):
    """the oracle's results and final handle for a case: computed once, shared, never modified"""
    key = (n_visible, width, height, tail, None if priors is None else tuple(k for k, p in enumerate(priors) if p is not None), n, tuple(sorted(kw.items())))
    if key not in _oracle:
        fo = handle(oracle_lib, n_visible, width, height, tail, **kw)
        res = [fo.process_frame(r, d, prior_pose=None if priors is None else priors[k]) for k, (r, d) in enumerate(frames(width, height, n))]
        _oracle[key] = (res, fo)
    return _oracle[key]


def waiter_matches(lib, f):
    lib.lib.ssf_waiter_matches.restype = C.c_longlong
    lib.lib.ssf_waiter_matches.argtypes = [C.c_void_p]
    return lib.lib.ssf_waiter_matches(f.h)


def check(want, fo, got, fh):
    for a, b in zip(want, got):
        util.same_result(a, b)
    util.compare_state(fo, fh, maps=False, frame_surfels=False)


def tracked(results):
    return sum(1 for r in results if r["icp_iters"] > 0)


@pytest.mark.parametrize("n_visible", [1, 255, 256, 257, 1000])
def test_visible_counts_around_a_workgroup(n_visible, oracle_lib, product_lib):
    """one row, one short of a workgroup, exactly one, one more (the collector is a workgroup of ONE row), several with a partial last"""
    want, fo = oracle_run(oracle_lib, n_visible)
    fh = handle(product_lib, n_visible)
    got = [fh.process_frame(r, d) for r, d in frames()]
    check(want, fo, got, fh)
    assert want[0]["icp_iters"] > 0
    assert fh.resident_icp_frames() == tracked(got) == NF, (fh.resident_icp_frames(), [r["icp_iters"] for r in got])
    assert waiter_matches(product_lib, fh) == NF


def test_a_loop_that_converges_and_one_that_ends_at_the_cap(oracle_lib, product_lib):
    want, fo = oracle_run(oracle_lib, 1000)
    assert all(1 < r["icp_iters"] < 10 for r in want), [r["icp_iters"] for r in want]      # several words, then the loop converges
    fh = handle(product_lib, 1000)
    got = [fh.process_frame(r, d) for r, d in frames()]
    check(want, fo, got, fh)
    assert fh.resident_icp_frames() == NF and waiter_matches(product_lib, fh) == NF
    want, fo = oracle_run(oracle_lib, 1000, icp_force_iters=1)
    assert all(r["icp_iters"] == 10 for r in want)
    fh = handle(product_lib, 1000, icp_force_iters=1)
    got = [fh.process_frame(r, d) for r, d in frames()]
    check(want, fo, got, fh)
    assert fh.resident_icp_frames() == NF and waiter_matches(product_lib, fh) == NF


def test_a_single_iteration(oracle_lib, product_lib):
    """icp_iter = 1: the launch runs its first round and the only word it is ever sent ends it"""
    want, fo = oracle_run(oracle_lib, 1000, icp_iter=1)
    fh = handle(product_lib, 1000, icp_iter=1)
    got = [fh.process_frame(r, d) for r, d in frames()]
    check(want, fo, got, fh)
    assert all(r["icp_iters"] == 1 for r in got)
    assert fh.resident_icp_frames() == NF and waiter_matches(product_lib, fh) == NF


def pipelined_with_priors(lib, priors, n):
    f = handle(lib, 1000, pipeline_depth=2, extract_batch=2)
    got, nsub = [], 0
    for k in range(n):
        while nsub < n and f.can_submit():
            f.submit_frame(*frames(W, H, n)[nsub]); nsub += 1
        got.append(f.process_submitted(prior_pose=priors[k]).as_dict())
    return got, f


def test_a_record_made_ahead_is_consumed_and_a_supplied_prior_discards_it(oracle_lib, lab_lib, monkeypatch):
    """Pipelined frames can have their first record accumulated by the frame before (k_move_rows<true>): the resident launch then
    starts at its SECOND word.  A frame that comes with a pose prior drops that record and its launch starts with a first round of
    its own.  A product handle first tries that form after 48 pipelined frames (AheadTuner), so the form is pinned here: the lab
    build of the same sources reads SSF_ICP_AHEAD = 2 when a handle is created (always accumulate ahead, the track stream waits
    for the next frame's extract).  Both sequences must be the oracle's to the bit, records must really have been consumed, and
    the sequence with priors must have consumed fewer."""
    n = 6
    monkeypatch.setenv("SSF_ICP_AHEAD", "2")
    none = [None] * n
    priors = [None, None, synthetic.pose12(*synthetic.relative_pose(2)), synthetic.pose12(*synthetic.relative_pose(3)), None, None]
    want_a, fo_a = oracle_run(oracle_lib, 1000, n=n)
    got_a, fa = pipelined_with_priors(lab_lib, none, n)
    check(want_a, fo_a, got_a, fa)
    want_b, fo_b = oracle_run(oracle_lib, 1000, priors=priors, n=n)
    got_b, fb = pipelined_with_priors(lab_lib, priors, n)
    check(want_b, fo_b, got_b, fb)
    assert fa.resident_icp_frames() == n and fb.resident_icp_frames() == n
    assert waiter_matches(lab_lib, fa) == n and waiter_matches(lab_lib, fb) == n
    ahead_a, ahead_b = fa.resident_icp_ahead_frames(), fb.resident_icp_ahead_frames()
    print("launches that started at word 1: %d without priors, %d with priors on frames 2 and 3" % (ahead_a, ahead_b))
    assert ahead_a >= 2, "no record made ahead was consumed: the launch never started at its second word"
    assert 1 <= ahead_b < ahead_a, (ahead_a, ahead_b)


def test_no_visible_rows(oracle_lib, product_lib):
    """a model with nothing in view: the first frame runs no loop (and no launch), the later ones track what it inserted"""
    want, fo = oracle_run(oracle_lib, 0, tail=500)
    fh = handle(product_lib, 0, tail=500)
    got = [fh.process_frame(r, d) for r, d in frames()]
    check(want, fo, got, fh)
    assert got[0]["icp_iters"] == 0 and tracked(got) >= 1
    assert fh.resident_icp_frames() == tracked(got) and waiter_matches(product_lib, fh) == tracked(got)


def test_pipelined_batches_against_one_frame_in_flight(oracle_lib, product_lib):
    want, fo = oracle_run(oracle_lib, 1000)
    fp = handle(product_lib, 1000, pipeline_depth=2, extract_batch=2)
    got_p = fp.process_sequence([r.ctypes.data for r, _ in frames()], [d.ctypes.data for _, d in frames()], on_device=False)
    f1 = handle(product_lib, 1000)
    got_1 = [f1.process_frame(r, d) for r, d in frames()]
    check(want, fo, got_p, fp)
    check(want, fo, got_1, f1)
    util.compare_state(fp, f1, maps=False, frame_surfels=False)
    assert fp.resident_icp_frames() == NF and f1.resident_icp_frames() == NF
    assert waiter_matches(product_lib, fp) == NF and waiter_matches(product_lib, f1) == NF


def test_both_paths_agree(oracle_lib, product_lib):
    """the limit at 0 (one launch per iteration, as before) against the limit high, on two product handles"""
    want, fo = oracle_run(oracle_lib, 1000)
    fa, fb = handle(product_lib, 1000), handle(product_lib, 1000)
    fa.set_resident_icp_max_rows(0); fb.set_resident_icp_max_rows(1 << 30)
    got_a = [fa.process_frame(r, d) for r, d in frames()]
    got_b = [fb.process_frame(r, d) for r, d in frames()]
    check(want, fo, got_a, fa)
    check(want, fo, got_b, fb)
    util.compare_state(fa, fb)
    assert fa.resident_icp_frames() == 0 and fb.resident_icp_frames() == NF
    assert waiter_matches(product_lib, fa) == NF and waiter_matches(product_lib, fb) == NF


def test_the_path_changes_between_frames(oracle_lib, product_lib):
    """the limit just below the visible count in the middle of a sequence, then back"""
    want, fo = oracle_run(oracle_lib, 1000)
    fh = handle(product_lib, 1000)
    got = [fh.process_frame(*frames()[0])]
    assert fh.resident_icp_frames() == 1
    fh.set_resident_icp_max_rows(got[0]["n_visible"] - 1)
    got.append(fh.process_frame(*frames()[1]))
    assert fh.resident_icp_frames() == 1, "a frame above the limit took the resident launch"
    fh.set_resident_icp_max_rows(got[1]["n_visible"])
    got.append(fh.process_frame(*frames()[2]))
    assert fh.resident_icp_frames() == 2, "a frame at the limit did not take the resident launch"
    fh.set_resident_icp_max_rows(0)
    got.append(fh.process_frame(*frames()[3]))
    assert fh.resident_icp_frames() == 2
    check(want, fo, got, fh)
    assert waiter_matches(product_lib, fh) == NF


def test_the_tile_sorted_copy_wins(oracle_lib, product_lib):
    """a frame that streams the tile-sorted copy of its rows (forced here) keeps the launches of that path, whatever the limit"""
    w, h = 320, 240
    want, fo = oracle_run(oracle_lib, 1000, w, h)
    fh = handle(product_lib, 1000, w, h)
    fh.set_bin_min_rows(0); fh.set_resident_icp_max_rows(1 << 30)
    got = [fh.process_frame(r, d) for r, d in frames(w, h)]
    check(want, fo, got, fh)
    assert tracked(got) == NF and fh.resident_icp_frames() == 0 and waiter_matches(product_lib, fh) == NF
    fh.set_bin_min_rows(-1)                       # and back: the next frame is the resident launch's
    fo2 = handle(oracle_lib, 1000, w, h)
    for r, d in frames(w, h):
        fo2.process_frame(r, d)
    extra = util.frame(NF, w, h, noise=True, holes=0.02)
    util.same_result(fo2.process_frame(*extra), fh.process_frame(*extra))
    util.compare_state(fo2, fh, maps=False, frame_surfels=False)
    assert fh.resident_icp_frames() == 1 and waiter_matches(product_lib, fh) == NF + 1


def test_the_pre_filter_in_the_frame_keeps_the_launches_per_iteration(oracle_lib, product_lib):
    """with cfg.depth_prefilter the pipeline is bound by its extract stage and the resident launch is not taken (ssf_host.hip,
    icp_resident_ok): same results, the waiting launches as before"""
    want, fo = oracle_run(oracle_lib, 1000, depth_prefilter=1)
    fh = handle(product_lib, 1000, depth_prefilter=1)
    got = [fh.process_frame(r, d) for r, d in frames()]
    check(want, fo, got, fh)
    assert tracked(got) == NF and fh.resident_icp_frames() == 0 and waiter_matches(product_lib, fh) == NF
