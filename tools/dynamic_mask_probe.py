"""Pixel masks (include/ssf_dynamic.h) against none, frames through ssf_process_sequence(_pixmask).

720 frames (the 8 real fr1_xyz frames, cycled back and forth), pipeline depth 2 x 8 frames per launch, device-resident and host
frames, each without a mask and with a fixed rectangle over ~20 % of the image.  A fresh handle per run (warm-up sequence first);
arms alternate, `--reps` rounds.  Prints frames/s per run and a JSON line per run.

    python tools/dynamic_mask_probe.py [--frames 720] [--reps 3] [--kinds device,host]

For kernel times run it under rocprofv3 --kernel-trace --stats: the masked batches launch k_render_moments<., true> and
k_finalize_surfels<true>, the others the <., false> instantiations."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from supersurfel_fusion_amd import binding, replay  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
WARMUP = 24


def run(lib, kind, masked, order, rgb, f32, mask):
    import torch
    cfg = dict(replay.BENCHMARK_LAUNCH, nb_supersurfels_max=100000, pipeline_depth=2, extract_batch=8)
    f = binding.Fusion(lib, lib.default_config(**cfg))
    if kind == "device":
        dr = [torch.from_numpy(c).cuda() for c in rgb]
        dd = [torch.from_numpy(d).cuda() for d in f32]
        dm = torch.from_numpy(mask).cuda()
        torch.cuda.synchronize()
        rp_all, dp_all, mp = [dr[k].data_ptr() for k in order], [dd[k].data_ptr() for k in order], dm.data_ptr()
        on_device = True
    else:
        rp_all, dp_all, mp = [rgb[k].ctypes.data for k in order], [f32[k].ctypes.data for k in order], mask.ctypes.data
        on_device = False
    masks = [mp] * len(order) if masked else None
    f.process_sequence(rp_all[:WARMUP], dp_all[:WARMUP], on_device, mask_ptrs=masks[:WARMUP] if masks else None)
    prep = f.prepare_sequence(rp_all[WARMUP:], dp_all[WARMUP:])
    t0 = time.perf_counter()
    res = f.process_prepared(prep, on_device, mask_ptrs=masks[WARMUP:] if masks else None)
    dt = time.perf_counter() - t0
    n = len(order) - WARMUP
    out = dict(kind=kind, masked=masked, frames=n, frames_per_sec=round(n / dt, 1), us_per_frame=round(1e6 * dt / n, 2),
               mask_share=round(float((mask != 0).mean()), 3), last_n_model=res[n - 1].n_model)
    f.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--frames", type=int, default=720)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kinds", default="device,host")
    a = ap.parse_args()
    lib = binding.load_product()
    z = list(replay.frames_from_npz(os.path.join(GOLD, "tum_fr1_xyz_8frames.npz")))
    rgb = [np.ascontiguousarray(c) for _, c, _ in z]
    f32 = [np.ascontiguousarray(d) for _, _, d in z]
    H, W = f32[0].shape
    mask = np.zeros((H, W), np.uint8)
    mask[int(0.3 * H):int(0.75 * H), int(0.3 * W):int(0.75 * W)] = 255          # ~20 % of the pixels
    m = len(z)
    period = 2 * m - 2
    order = [(i % period) if (i % period) < m else period - (i % period) for i in range(WARMUP + a.frames)]
    kinds = a.kinds.split(",")
    results = []
    for rep in range(a.reps):
        for kind in kinds:
            for masked in ((False, True) if rep % 2 == 0 else (True, False)):
                r = run(lib, kind, masked, order, rgb, f32, mask)
                r["rep"] = rep
                results.append(r)
                print("rep %d %-6s mask %d: %8.1f frames/s  %7.2f us/frame" % (rep, kind, masked, r["frames_per_sec"], r["us_per_frame"]), flush=True)
                print("JSON " + json.dumps(r), flush=True)
    for kind in kinds:
        for masked in (False, True):
            v = [r["frames_per_sec"] for r in results if r["kind"] == kind and r["masked"] == masked]
            print("%-6s mask %d: frames/s %s  mean %.1f" % (kind, masked, " ".join("%.1f" % x for x in v), sum(v) / len(v)))


if __name__ == "__main__":
    main()
