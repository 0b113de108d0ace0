"""The replicas of the association table (csrc/ssf_device.hpp, assoc_stride; k_icp_resident / k_icp in csrc/ssf_track_fuse.hip): a
frame of a single shard whose association runs inside an ICP launch bids into one of eight tables, chosen by the XCD the
workgroup runs on, and the readers of the fuse launch take the minimum over table 0 and the eight (assoc_best).  Keys are unique
and MIN is order-free, so every result and the final state must be the oracle's to the bit whichever table a bid went to -- and
on every path that stays on table 0 (k_match as a launch of its own, the tile-sorted copy, the late-word repair's second pass).

Built like tests/test_icp_resident_gpu.py: 160x128 frames (S = 80 frame supersurfels), a seeded model cut to an exact number of
visible rows, 4 frames.  From 2049 rows on the launch has more than eight workgroups, so more than one replica receives bids;
4000 rows over 80 words are 50 bids per word.  On the lab build of the same sources the cases also assert, through
ssf_dbg_assoc_replica_frames, that the intended path was taken; the product is compared with the oracle only."""
import ctypes as C
import functools

import numpy as np
import pytest

import util
from supersurfel_fusion_amd import binding, synthetic

pytestmark = pytest.mark.gpu

W, H = 160, 128
NF = 4
NO_MATCH = np.uint64(0x7FFFFFFFFFFFFFFF)


@functools.lru_cache(maxsize=None)
def seeded_rows(width, height):
    model, nvis = synthetic.seed_model_cam0(60000, width, height, stamp=30)
    assert nvis >= 4000, nvis
    return model, nvis


def model_rows(n_visible, width=W, height=H, ties=()):
    """the first n_visible VISIBLE seeded rows; ties: the rows at which rows [0, 256) sit once more -- further workgroups bid the
    same distance bits for the same frame supersurfels under larger ids"""
    model, _ = seeded_rows(width, height)
    rows = {k: v[:n_visible].copy() for k, v in model.items()}
    for at in ties:
        assert at % 256 == 0 and 256 <= at and at + 256 <= n_visible
        for v in rows.values():
            v[at:at + 256] = v[0:256]
    return rows


def handle(lib, n_visible, width=W, height=H, ties=(), **kw):
    f = binding.Fusion(lib, util.make_cfg(lib, width, height, nb_supersurfels_max=16384, **kw))
    f.set_model(model_rows(n_visible, width, height, ties), n_visible, 30)
    return f


@functools.lru_cache(maxsize=None)
def frames(width=W, height=H, n=NF):
    return tuple((np.ascontiguousarray(r), np.ascontiguousarray(d)) for r, d in
                 (util.frame(k, width, height, noise=True, holes=0.02) for k in range(n)))


_oracle = {}


def oracle_run(oracle_lib, n_visible, width=W, height=H, ties=(), **kw):
    """the oracle's results and final handle for a case: computed once, shared, never modified"""
    key = (n_visible, width, height, ties, tuple(sorted(kw.items())))
    if key not in _oracle:
        fo = handle(oracle_lib, n_visible, width, height, ties, **kw)
        _oracle[key] = ([fo.process_frame(r, d) for r, d in frames(width, height)], fo)
    return _oracle[key]


def counter(lib, name, f):
    fn = getattr(lib.lib, name)
    fn.restype = C.c_longlong
    fn.argtypes = [C.c_void_p]
    return fn(f.h)


def replica_frames(lib, f):
    """frames that bid into the replicas; None on the product, which has no such counter"""
    return counter(lib, "ssf_dbg_assoc_replica_frames", f) if hasattr(lib.lib, "ssf_dbg_assoc_replica_frames") else None


def check(want, fo, got, fh):
    for a, b in zip(want, got):
        util.same_result(a, b)
    util.compare_state(fo, fh, maps=False, frame_surfels=False)


def tracked(results):
    return sum(1 for r in results if r["icp_iters"] > 0)


def run(lib, n_visible, width=W, height=H, ties=(), before=None, **kw):
    fh = handle(lib, n_visible, width, height, ties, **kw)
    if before:
        before(fh)
    return [fh.process_frame(r, d) for r, d in frames(width, height)], fh


@pytest.fixture(params=["product", "lab"])
def lib(request, product_lib, lab_lib):
    return product_lib if request.param == "product" else lab_lib


@pytest.mark.parametrize("n_visible", [1, 257, 2049, 4000])
def test_workgroup_counts(n_visible, oracle_lib, lib):
    """one workgroup of one row, two, nine (the ninth shares an XCD with the first), sixteen with 50 bids per word"""
    want, fo = oracle_run(oracle_lib, n_visible)
    got, fh = run(lib, n_visible)
    check(want, fo, got, fh)
    assert fh.resident_icp_frames() == tracked(got) == NF
    n = replica_frames(lib, fh)
    assert n is None or n == NF, n


@pytest.mark.parametrize("ties", [(2048,), (2048, 2304)], ids=["workgroups_0_8", "workgroups_0_8_9"])
def test_ties_across_workgroups_go_to_the_smaller_id(ties, oracle_lib, lib):
    """Rows [0, 256) also sit at [2048, 2304): workgroups 0 and 8 bid equal distance bits for the same words, and the word the
    readers see must carry the smaller id.  Workgroups are dealt to the XCDs in turn, so 0 and 8 normally share one and meet in ONE
    replica; the second case puts the rows at [2304, 2560) as well -- workgroup 9, the next XCD -- so that equal distance bits sit
    in two DIFFERENT replicas and the tie is settled by assoc_best's minimum over the tables.  First, on the ORACLE's own
    association table of the first frame (the stage seam): at least one winner must be such a row and none a copy, or the case
    proves nothing."""
    fs = handle(oracle_lib, 4000, ties=ties)
    fs.stage_extract(*frames()[0]); fs.icp_begin()
    while fs.icp_update(fs.icp_accumulate()):
        pass
    fs.icp_end()
    best, _ = fs.match()
    ids = (best[best != NO_MATCH] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    assert (ids < 256).sum() >= 1, "no duplicated row wins a frame supersurfel"
    for at in ties:
        assert not ((ids >= at) & (ids < at + 256)).any(), "a copy won against its original: the oracle's tie rule is not smaller-id"
    want, fo = oracle_run(oracle_lib, 4000, ties=ties)
    got, fh = run(lib, 4000, ties=ties)
    check(want, fo, got, fh)
    n = replica_frames(lib, fh)
    assert n is None or n == NF, n


def test_the_waiting_launch_bids_into_the_replicas_too(oracle_lib, lib):
    """the resident limit at 0: a launch per iteration, the one waiting at the end of the loop associates (SSF_ICP_GO_MATCH)"""
    want, fo = oracle_run(oracle_lib, 4000)
    got, fh = run(lib, 4000, before=lambda f: f.set_resident_icp_max_rows(0))
    check(want, fo, got, fh)
    assert fh.resident_icp_frames() == 0 and counter(lib, "ssf_waiter_matches", fh) == NF
    n = replica_frames(lib, fh)
    assert n is None or n == NF, n
    # ... and with the pre-filter in the frame, which keeps the launches per iteration by itself
    want, fo = oracle_run(oracle_lib, 2049, depth_prefilter=1)
    got, fh = run(lib, 2049, depth_prefilter=1)
    check(want, fo, got, fh)
    assert fh.resident_icp_frames() == 0 and counter(lib, "ssf_waiter_matches", fh) == NF
    n = replica_frames(lib, fh)
    assert n is None or n == NF, n


def test_k_match_as_a_launch_of_its_own_stays_on_table_0(oracle_lib, lib):
    """profile = 1 times every kernel by itself: no launch made ahead, the association is k_match, the readers read one word"""
    want, fo = oracle_run(oracle_lib, 4000, profile=1)
    got, fh = run(lib, 4000, profile=1)
    check(want, fo, got, fh)
    assert counter(lib, "ssf_waiter_matches", fh) == 0
    n = replica_frames(lib, fh)
    assert n is None or n == 0, n


def test_a_late_word_is_repaired_over_the_replicas(oracle_lib, lab_lib):
    """The stall hook of the lab build in front of the host's word (tests/test_parity_gpu.py): whatever part of the grid still
    bids does so into the replicas, the full k_match that repairs the frame bids into table 0, and the readers' minimum over the
    nine is the full pass."""
    want, fo = oracle_run(oracle_lib, 2049)
    L = lab_lib.lib
    L.ssf_dbg_stall_before_match_us.argtypes = [C.c_void_p, C.c_longlong]; L.ssf_dbg_stall_before_match_us.restype = None
    got, fh = run(lab_lib, 2049, before=lambda f: L.ssf_dbg_stall_before_match_us(f.h, 350000))
    check(want, fo, got, fh)
    assert counter(lab_lib, "ssf_waiter_match_repairs", fh) >= 1, "no frame was repaired: the path was not taken"
    assert replica_frames(lab_lib, fh) == NF


def test_the_tile_sorted_path_stays_on_table_0(oracle_lib, lib):
    """a frame that streams the tile-sorted copy of its rows (forced): its XCDs already bid for disjoint frame supersurfels"""
    w, h = 320, 240
    want, fo = oracle_run(oracle_lib, 2049, w, h)
    got, fh = run(lib, 2049, w, h, before=lambda f: f.set_bin_min_rows(0))
    check(want, fo, got, fh)
    assert tracked(got) == NF and fh.resident_icp_frames() == 0 and counter(lib, "ssf_waiter_matches", fh) == NF
    n = replica_frames(lib, fh)
    assert n is None or n == 0, n
