"""The fused row-move launch (k_move_rows<true, .> in csrc/ssf_track_fuse.hip): while the rows that stay or come into view move to the
new visible array, the launch accumulates the next frame's first ICP record.  Its two gathers travel beside the prefix, and a
workgroup that moves no row into the new visible array -- a visible block past the last row, an out-of-view block whose rows are
only removed -- leaves before it touches the prefix, the ICP table or the row count.  The sums are exact integers: every result
and the final state must be the oracle's to the bit, from whichever kind of workgroup the record's terms come.

Pipelined frames (160x128) over a seeded model cut to an exact number of visible rows, as in test_icp_resident_gpu.py; the lab
build of the same sources with SSF_ICP_AHEAD = 2 pins the fused form (a product handle first tries it after 48 pipelined frames),
and ssf_resident_icp_ahead_frames shows that the records made ahead were really consumed."""
import numpy as np
import pytest

import util
from supersurfel_fusion_amd import binding
from test_icp_resident_gpu import W, H, check, frames, seeded_rows

pytestmark = pytest.mark.gpu

NF = 6
COUNTS = [1, 255, 256, 257, 1000]      # a block of one row, a partial last block, exactly one block, one row in the block at nbr - 1, several blocks
IN_VIEW_TAIL = 300                     # rows in view under camera 0, handed over as out-of-view rows: they come back in frame 0


def rows_for(n_visible, in_view_tail=0, tail=0):
    """the first n_visible VISIBLE seeded rows, declared visible; behind them `in_view_tail` further visible rows and `tail` rows
    from the out-of-view end, both handed over as out-of-view rows.  Every second row of `tail` is stale (never seen again since
    frame 0, confidence below the threshold): frame 0 removes it, so the blocks of the tail have slots to free and no row to move"""
    model, nvis = seeded_rows(W, H)
    assert n_visible + in_view_tail <= nvis
    take = np.concatenate([np.arange(n_visible), np.arange(nvis - in_view_tail, nvis), np.arange(nvis, nvis + tail)])
    rows = {k: v[take].copy() for k, v in model.items()}
    stale = n_visible + in_view_tail + np.arange(0, tail, 2)
    rows["stamps"][stale, 1] = 0
    rows["confidences"][stale] = 1.0
    assert 1.0 < util.BENCH_PARAMS["conf_thresh"] and 31 > util.BENCH_PARAMS["delta_t"]
    return rows


def handle(lib, n_visible, in_view_tail=0, tail=0, **kw):
    f = binding.Fusion(lib, util.make_cfg(lib, W, H, nb_supersurfels_max=16384, **kw))
    f.set_model(rows_for(n_visible, in_view_tail, tail), n_visible, 30)
    return f


_oracle = {}


def oracle_run(oracle_lib, n_visible, in_view_tail=0, tail=0):
    """the oracle's results and final handle for a case: computed once, shared, never modified"""
    key = (n_visible, in_view_tail, tail)
    if key not in _oracle:
        fo = handle(oracle_lib, n_visible, in_view_tail, tail)
        _oracle[key] = ([fo.process_frame(r, d) for r, d in frames(W, H, NF)], fo)
    return _oracle[key]


def pipelined(lib, n_visible, in_view_tail=0, tail=0):
    f = handle(lib, n_visible, in_view_tail, tail, pipeline_depth=2, extract_batch=2)
    got, nsub = [], 0
    for k in range(NF):
        while nsub < NF and f.can_submit():
            f.submit_frame(*frames(W, H, NF)[nsub]); nsub += 1
        got.append(f.process_submitted().as_dict())
    return got, f


def run_case(oracle_lib, lab_lib, monkeypatch, n_visible, in_view_tail=0, tail=0, min_ahead=2):
    monkeypatch.setenv("SSF_ICP_AHEAD", "2")
    want, fo = oracle_run(oracle_lib, n_visible, in_view_tail, tail)
    got, fh = pipelined(lab_lib, n_visible, in_view_tail, tail)
    check(want, fo, got, fh)
    tracked = sum(1 for r in got if r["icp_iters"] > 0)
    ahead = fh.resident_icp_ahead_frames()
    print("n_visible %d (+%d in view, +%d out of view in the tail): %d frames tracked, %d launches started at word 1; n_visible by frame %s"
          % (n_visible, in_view_tail, tail, tracked, ahead, [r["n_visible"] for r in got]))
    assert fh.resident_icp_frames() == tracked
    assert ahead >= min_ahead, "no record made ahead was consumed: the launch never started at its second word"
    return want


def came_back(want, n_visible):
    """from the oracle's own result: rows returned through the out-of-view blocks in frame 0 (more rows are visible after it than
    were visible before plus the rows it inserted)"""
    return want[0]["n_visible"] > n_visible + want[0]["n_inserted"]


@pytest.mark.parametrize("n_visible", COUNTS)
def test_visible_blocks_alone(n_visible, oracle_lib, lab_lib, monkeypatch):
    """no out-of-view rows: every term of the record comes from the blocks of the visible array, the grid's other visible blocks
    (the host sizes it by an upper bound) hold no row and leave at once"""
    run_case(oracle_lib, lab_lib, monkeypatch, n_visible)


@pytest.mark.parametrize("n_visible", COUNTS)
def test_rows_that_come_back_into_view(n_visible, oracle_lib, lab_lib, monkeypatch):
    """300 rows that are in view, handed over as out-of-view rows: frame 0 brings them back through an out-of-view block, whose
    gathers travel beside the prefix over the out-of-view groups"""
    want = run_case(oracle_lib, lab_lib, monkeypatch, n_visible, in_view_tail=IN_VIEW_TAIL)
    assert came_back(want, n_visible), (want[0]["n_visible"], n_visible, want[0]["n_inserted"])


def test_the_first_record_from_out_of_view_blocks_alone(oracle_lib, lab_lib, monkeypatch):
    """no row declared visible, 500 rows in view in the tail: frame 0 runs no loop, and no old visible row adds to the record its
    move makes for frame 1"""
    want = run_case(oracle_lib, lab_lib, monkeypatch, 0, in_view_tail=500, min_ahead=1)
    assert want[0]["icp_iters"] == 0 and want[1]["icp_iters"] > 0
    assert came_back(want, 0), (want[0]["n_visible"], want[0]["n_inserted"])


@pytest.mark.parametrize("n_visible", COUNTS)
def test_out_of_view_blocks_that_add_nothing(n_visible, oracle_lib, lab_lib, monkeypatch):
    """500 rows that are truly out of view in the tail, half of them removed by frame 0: their blocks free the slots, take no part
    in the record and leave before its table"""
    want = run_case(oracle_lib, lab_lib, monkeypatch, n_visible, tail=500)
    assert not came_back(want, n_visible)
    assert want[0]["n_removed"] >= 250, want[0]["n_removed"]


def test_blocks_with_rows_that_come_back_and_rows_that_are_removed(oracle_lib, lab_lib, monkeypatch):
    """the two kinds of out-of-view rows side by side in one block of 256 slots"""
    want = run_case(oracle_lib, lab_lib, monkeypatch, 1000, in_view_tail=IN_VIEW_TAIL, tail=500)
    assert came_back(want, 1000) and want[0]["n_removed"] >= 250
