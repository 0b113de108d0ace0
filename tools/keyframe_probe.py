"""ssf_keyframes_* (include/ssf_keyframes.h) at 640 x 480 with 500 ferns on frames of the synthetic orbit.

Reports, with a warm-up and --reps repetitions (median, min .. max, microseconds of wall clock around the call):
  * keyframes_consider with K = 0, 256, 1 000, 10 000 stored keyframes (filled through keyframes_put with random codes and no rows;
    new_ratio is set out of reach so that the store does not grow while it is timed; K = 0 always adds, its database is rebuilt
    before every call, outside the timed region), and its kernel times under profile = 1 (kf_encode, kf_search, kf_select);
  * keyframes_add (encode + the stable compaction of the frame's rows into the pool);
  * keyframes_align of a stored keyframe beside align() of the same rows handed over from the host, on the same pair of frames
    (the difference is the row-sized upload and the Lab loop on the host); the two results are compared bit for bit;
  * for scale, process_frame on the same handle (one frame in flight, no pipelining).
Prints a table and one JSON line.

    python tools/keyframe_probe.py [--reps 20] [--sizes 0,256,1000,10000]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from supersurfel_fusion_amd import binding, synthetic  # noqa: E402

W, H, N_FERNS = 640, 480, 500


def spread(fn, reps, before=None):
    """microseconds of `reps` calls after one warm-up call: (median, min, max)"""
    t = []
    for k in range(reps + 1):
        if before:
            before()
        t0 = time.perf_counter()
        fn()
        if k:
            t.append(1e6 * (time.perf_counter() - t0))
    return float(np.median(t)), float(min(t)), float(max(t))


def frame(k):
    R, t = synthetic.orbit_pose(k)
    rgb, depth, _ = synthetic.render(R, t, W, H, noise=True, rng=np.random.default_rng(1000 + k))
    return rgb, depth


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sizes", default="0,256,1000,10000")
    a = ap.parse_args()
    sizes = [int(s) for s in a.sizes.split(",")]
    lib = binding.load_product()
    K = synthetic.intrinsics(W, H)
    f = binding.Fusion(lib, lib.default_config(**dict({k: K[k] for k in ("width", "height", "fx", "fy", "cx", "cy")}, nb_supersurfels_max=50000,
                                                       lambda_pos=10.0, lambda_size=1000.0, lambda_disp=1e8, icp_cov_thresh=0.05)))
    frames = [frame(k) for k in range(4)]
    t_frame = spread(lambda: f.process_frame(*frames[3]), a.reps, before=lambda: [f.process_frame(*fr) for fr in frames[:3]])
    rng = np.random.default_rng(5)
    pose = np.zeros(12, np.float32)
    rows_cap = 4 * f.S
    out = dict(size=[W, H], ferns=N_FERNS, reps=a.reps, process_frame_us=[round(x, 1) for x in t_frame], consider={})

    print("%d x %d, %d ferns, S = %d superpixels; wall clock in us: median (min .. max) of %d" % (W, H, N_FERNS, f.S, a.reps))
    print("  %-34s %9.1f  (%.1f .. %.1f)   [for scale: one frame in flight]" % (("process_frame",) + t_frame))
    for n_kf in sizes:
        def build():
            f.keyframes_clear()
            f.keyframes_configure(n_ferns=N_FERNS, max_keyframes=n_kf + 4, max_rows=rows_cap, min_gap=0, new_ratio=2.0)
            for _ in range(n_kf):
                f.keyframes_put(rng.integers(0, 16, N_FERNS).astype(np.uint8), None, pose, 0)
        build()
        t = spread(f.keyframes_consider, a.reps, before=build if n_kf == 0 else None)
        f.set_profile(1)
        if n_kf == 0:
            build()
        f.keyframes_consider()
        f.reset_kernel_times()
        for _ in range(a.reps):
            if n_kf == 0:
                build()
            f.keyframes_consider()
        kt = f.kernel_times(128)
        f.set_profile(0)
        us = {k: round(1e3 * kt[k][0] / max(kt[k][1], 1), 2) for k in ("kf_encode", "kf_search", "kf_select") if k in kt}
        print("  %-34s %9.1f  (%.1f .. %.1f)   kernels: %s" % (("keyframes_consider, K = %d" % n_kf,) + t + (us,)))
        out["consider"][str(n_kf)] = dict(wall_us=[round(x, 1) for x in t], kernel_us=us)

    f.keyframes_clear()
    f.keyframes_configure(n_ferns=N_FERNS, max_keyframes=a.reps + 4)
    t_add = spread(f.keyframes_add, a.reps)
    print("  %-34s %9.1f  (%.1f .. %.1f)   (%d rows stored per keyframe)" % (("keyframes_add",) + t_add + (len(f.keyframes_get(0)["rows"]["confidences"]),)))

    # keyframe = frame 0, current frame = frame 3
    f2 = binding.Fusion(lib, f.cfg)
    f2.keyframes_configure(n_ferns=N_FERNS)
    f2.process_frame(*frames[0])
    kid = f2.keyframes_add()
    for fr in frames[1:]:
        f2.process_frame(*fr)
    rows = f2.keyframes_get(kid)["rows"]
    src = {k: rows[k] for k in ("positions", "colors", "orientations")}
    t_dev = spread(lambda: f2.keyframes_align(kid), a.reps)
    t_host = spread(lambda: f2.align(src), a.reps)
    ra, rb = f2.keyframes_align(kid), f2.align(src)
    same = bool(ra["rel_pose"].tobytes() == rb["rel_pose"].tobytes() and (ra["valid"], ra["iters"], ra["pairs"]) == (rb["valid"], rb["iters"], rb["pairs"]))
    print("  %-34s %9.1f  (%.1f .. %.1f)   (%d rows, %d iterations, %d pairs)" % (("keyframes_align (stored rows)",) + t_dev + (len(rows["confidences"]), ra["iters"], ra["pairs"])))
    print("  %-34s %9.1f  (%.1f .. %.1f)   same result bit for bit: %s" % (("align (rows from the host)",) + t_host + (same,)))
    out.update(add_us=[round(x, 1) for x in t_add], keyframes_align_us=[round(x, 1) for x in t_dev], align_us=[round(x, 1) for x in t_host],
               align_same=same)
    print(json.dumps(out))
    f.close(); f2.close()
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
