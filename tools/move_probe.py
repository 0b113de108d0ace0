"""Where the time goes inside ONE fused row-move launch (k_move_rows<true, .>, csrc/ssf_track_fuse.hip): every workgroup leaves its
ticks of the 100 MHz wall clock (lab build: ssf_dbg_move_trace) -- entry | row and state arrived | prefix known | stores issued |
terms in the ICP table | fold done | end -- reported by the kind of workgroup: visible blocks, visible blocks past the last row,
out-of-view blocks with rows that come back, out-of-view blocks whose rows are only removed, out-of-view blocks where nothing moves.

The bench map (640x480, 1 M seeded rows), pipelined 2 x 8 with SSF_ICP_AHEAD = 2 (every move launch is the fused one), two ways:
  alone     the device is idle when the frame is processed: the next batch's extract has finished, nothing else is submitted
  in place  the pipeline is kept full, extract batches run beside the track chain
SSF_PRODUCT_VARIANT=<tag> takes another build with -DSSF_EXPERIMENTS (tools/build_variant.sh <tag> -DSSF_EXPERIMENTS)."""
import ctypes as C, os, sys, warnings
warnings.simplefilter("ignore", RuntimeWarning)      # (a step no workgroup of a kind reaches: a column of NaN)
os.environ.setdefault("SSF_ICP_AHEAD", "2")
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np
import torch
import util
from supersurfel_fusion_amd import binding, synthetic

lib = binding.load_product() if os.environ.get("SSF_PRODUCT_VARIANT") else binding.load_lab()
lib.lib.ssf_dbg_move_trace.argtypes = [C.c_int]
lib.lib.ssf_dbg_move_trace_read.restype = C.c_int
lib.lib.ssf_dbg_move_trace_read.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
W, H, NFRAMES, BATCH = 640, 480, 48, 8
KINDS = {1: "visible", 17: "visible, past the last row", 2: "out of view, rows come back", 3: "out of view, rows only removed", 4: "out of view, nothing moves"}
STEPS = ("row+state", "prefix", "stores", "terms", "fold", "end")
frames = [util.frame(k % 16, W, H) for k in range(16)]
model, nvis = synthetic.seed_model_cam0(1000000, W, H)


def report(title, launches):
    """launches: arrays (workgroups, 8) of one fused launch each; microseconds, medians over the launches of per-launch figures"""
    print("%s: %d fused launches, %d workgroups each" % (title, len(launches), int(np.median([len(t) for t in launches]))))
    rows = {}
    for t in launches:
        us = (t[:, :7].astype(np.int64) - t[:, 0].astype(np.int64).min()) / 100.0
        kind = (t[:, 7] & 0xFF).astype(int)
        for k in KINDS:
            a = us[kind == k]
            if not len(a):
                continue
            r = [len(a), a[:, 0].min(), np.median(a[:, 0]), a[:, 0].max()]
            for s in range(1, 7):
                ok = t[kind == k][:, s] != 0
                d = a[ok, s] - a[ok, 0]
                r += [np.median(d), d.max()] if ok.any() else [np.nan, np.nan]
            r.append(a[:, 6].max())
            rows.setdefault(k, []).append(r)
    for k, rs in rows.items():
        m = np.nanmedian(np.array(rs, float), axis=0)
        print("   %-32s %5d workgroups  entry %.2f / %.2f / %.2f (first / median / last)  launch-relative end of the last %.2f" % (KINDS[k], m[0], m[1], m[2], m[3], m[-1]))
        print("      after the workgroup's entry, median (max):  " + "  ".join("%s %.2f (%.2f)" % (n, m[4 + 2 * i], m[5 + 2 * i]) for i, n in enumerate(STEPS) if not np.isnan(m[4 + 2 * i])))
    ends = [((t[:, 6].astype(np.int64).max() - t[:, 0].astype(np.int64).min()) / 100.0) for t in launches]
    print("   first entry to last end: median %.2f us, min %.2f, max %.2f" % (np.median(ends), min(ends), max(ends)))


def sweep(k):
    """the camera goes along the orbit and back"""
    return k % 30 if k % 30 < 16 else 30 - k % 30


def run(alone):
    f = binding.Fusion(lib, util.make_cfg(lib, W, H, nb_supersurfels_max=1100000, pipeline_depth=2, extract_batch=BATCH))
    f.set_model(model, nvis, 30)
    buf = np.zeros((65536, 8), np.uint64)
    launches, nsub = [], 0
    for k in range(NFRAMES):
        while nsub < NFRAMES and f.can_submit() and (not alone or nsub < k + 2 * BATCH):
            f.submit_frame(*frames[sweep(nsub)]); nsub += 1
        if alone:
            torch.cuda.synchronize()
        f.process_submitted()
        n = lib.lib.ssf_dbg_move_trace_read(f.h, buf.ctypes.data, 65536)
        if k < 8 or n <= 0:
            continue
        t = buf[:n].copy()
        t = t[t[:, 0] >= t[:, 0].max() - 100000]          # (workgroups of an earlier, larger launch: more than a millisecond older)
        if (t[:, 7] & 0x100).any():
            launches.append(t)
    print("resident launches that started at word 1: %d of %d frames" % (f.resident_icp_ahead_frames(), NFRAMES))
    report("alone on the part" if alone else "in place, pipeline full", launches)


print("build:", os.environ.get("SSF_PRODUCT_VARIANT", "lab"))
lib.lib.ssf_dbg_move_trace(1)
run(True)
run(False)
lib.lib.ssf_dbg_move_trace(0)
