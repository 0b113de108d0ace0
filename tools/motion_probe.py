"""The geometric moving-object detector (include/ssf_motion.h) at 640x480: per-kernel times under profile = 1 and the stats, on
  * the tum_fr3_walking_4frames golden: the map built from its first three frames, the mask taken for the fourth (ssf_motion_mask,
    render included: render_prep / render_fill / render_tile are listed next to the motion_* kernels);
  * a serpentine worst case (ssf_motion_segment: a one-pixel corridor over the whole image, one component whose only path is
    about W * H / 2 long).
For scale, the same session measures one frame in flight (process_frame of the golden's fourth frame on the map of the first three,
no mask) with this build and, with --baseline-variant TAG, with another build of the library next to the product
(csrc/variants/TAG/libssf_hip.so).  The figure in profiles/motion_mask.txt used TAG = parent, the parent commit's sources built with
the product's own Makefile:

    mkdir /tmp/parent && git archive HEAD~1 supersurfel_fusion_amd/csrc include | tar -x -C /tmp/parent
    make -C /tmp/parent/supersurfel_fusion_amd/csrc -j16 libssf_hip.so
    mkdir -p supersurfel_fusion_amd/csrc/variants/parent
    cp /tmp/parent/supersurfel_fusion_amd/csrc/libssf_hip.so supersurfel_fusion_amd/csrc/variants/parent/

(HEAD~1 = the commit before this detector; from a checkout of that commit, `tools/build_variant.sh parent` does the same.)

    python tools/motion_probe.py [--reps 20] [--baseline-variant parent] [--out profiles/motion_mask.txt]

No time is gated.  For a kernel trace run it under rocprofv3 --kernel-trace --stats; for counters, a run of its own."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from supersurfel_fusion_amd import binding, replay  # noqa: E402

MOTION = ("motion_classify", "motion_label", "motion_merge", "motion_flatten", "motion_decide")
RENDER = ("render_prep", "render_fill", "render_tile")
GOLD = os.path.join(ROOT, "tests", "golden", "tum_fr3_walking_4frames.npz")


def serpentine(W, H):
    """depth, model depth: the corridor at 1 m in front of a map at 2 m (all seeds), everything else on the map"""
    m = np.zeros((H, W), bool)
    m[0::2, :] = True
    m[1::4, W - 1] = True
    m[3::4, 0] = True
    return np.where(m, np.float32(1), np.float32(2)).astype(np.float32), np.full((H, W), 2, np.float32)


def kernel_us(f, fn, reps, names):
    f.set_profile(1)
    fn()
    f.reset_kernel_times()
    for _ in range(reps):
        fn()
    kt = f.kernel_times()
    f.set_profile(0)
    return {k: round(1e3 * kt[k][0] / max(kt[k][1], 1), 1) for k in names if k in kt}


def wall_us(fn, reps):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return round(1e6 * float(np.median(t)), 1)


def frame_in_flight_us(lib, frames, reps):
    """process_frame of the last frame on the map of the others, no mask: median wall clock over fresh handles"""
    t = []
    for _ in range(reps):
        f = binding.Fusion(lib, lib.default_config(**dict(replay.BENCHMARK_LAUNCH, nb_supersurfels_max=20000)))
        for _, rgb, depth in frames[:-1]:
            f.process_frame(rgb, depth)
        t0 = time.perf_counter()
        f.process_frame(frames[-1][1], frames[-1][2])
        t.append(time.perf_counter() - t0)
        f.close()
    return round(1e6 * float(np.median(t)), 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--baseline-variant", default=None, metavar="TAG")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    lib = binding.load_product()
    frames = list(replay.frames_from_npz(GOLD))
    rows = []
    f = binding.Fusion(lib, lib.default_config(**dict(replay.BENCHMARK_LAUNCH, nb_supersurfels_max=20000)))
    W, H = f.W, f.H
    for _, rgb, depth in frames[:3]:
        f.process_frame(rgb, depth)
    depth = np.ascontiguousarray(frames[3][2], np.float32)
    d_depth = torch.from_numpy(depth).cuda()
    d_mask = torch.empty((H, W), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    call = lambda: f.motion_mask_device(d_depth, mask=d_mask)
    st = call()
    rows.append(dict(input="tum_fr3_walking_4frames: map of frames 0-2, mask of frame 3", call="ssf_motion_mask (device pointers)",
                     width=W, height=H, model_rows=f.counts()["n_model"], wall_us=wall_us(call, a.reps),
                     kernel_us=kernel_us(f, call, a.reps, RENDER + MOTION), stats=st))
    sd, sm = serpentine(W, H)
    d_sd, d_sm = torch.from_numpy(sd).cuda(), torch.from_numpy(sm).cuda()
    torch.cuda.synchronize()
    call = lambda: f.motion_mask_device(d_sd, mask=d_mask, model_depth=d_sm)
    st = call()
    rows.append(dict(input="serpentine: a one-pixel corridor over the whole image", call="ssf_motion_segment (device pointers)", width=W,
                     height=H, wall_us=wall_us(call, a.reps), kernel_us=kernel_us(f, call, a.reps, MOTION), stats=st))
    f.close()
    reps = max(3, a.reps // 4)
    rows.append(dict(input="tum_fr3_walking_4frames: frame 3 on the map of frames 0-2", call="process_frame, no mask (this build)",
                     wall_us=frame_in_flight_us(lib, frames, reps)))
    if a.baseline_variant:
        base = binding.Library(os.path.join(os.path.dirname(binding.PRODUCT_LIB), "variants", a.baseline_variant, "libssf_hip.so"))
        rows.append(dict(input="tum_fr3_walking_4frames: frame 3 on the map of frames 0-2",
                         call="process_frame, no mask (variant %s, has_motion=%s)" % (a.baseline_variant, base.has_motion),
                         wall_us=frame_in_flight_us(base, frames, reps)))
    lines = []
    for r in rows:
        lines.append("%s\n  %s: %.1f us wall clock" % (r["input"], r["call"], r["wall_us"]))
        if "kernel_us" in r:
            lines.append("  kernels (us, mean of %d): %s ; motion_* sum %.1f" % (
                a.reps, ", ".join("%s %.1f" % kv for kv in r["kernel_us"].items()), sum(v for k, v in r["kernel_us"].items() if k in MOTION)))
            lines.append("  stats: %s" % json.dumps(r["stats"]))
        lines.append("  " + json.dumps(r))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
