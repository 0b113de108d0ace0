"""ssf_render_model (include/ssf_render.h) on the metric's map: synthetic.seed_model_cam0 at ~1 M rows through ssf_set_model with
the bench's visible split, rendered from camera 0 at 640x480 and 1280x960, every live row and the visible rows only.

Per arm: wall-clock microseconds per render (host outputs: depth, index, rgb8, colour, normal copied back; and device outputs),
the kernel split under profile = 1 (render_prep: live scan + prep + tile-count scan, render_fill, render_tile), fragments per
pixel, list entries and rows per second; and for comparison the copy a node pays today: ssf_get_model of the whole map.
Prints a table and one JSON line per arm.

    python tools/render_probe.py [--rows 1000000] [--reps 20]

For a kernel trace run it under rocprofv3 --kernel-trace --stats; for counters, a run of its own."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from supersurfel_fusion_amd import binding, synthetic  # noqa: E402

OUT = ("depth", "index", "rgb8", "color", "normal")


def timed(fn, reps):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return 1e6 * float(np.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    import torch
    lib = binding.load_product()
    W0, H0 = 640, 480
    model, nvis = synthetic.seed_model_cam0(a.rows, W0, H0, stamp=30)
    K0 = synthetic.intrinsics(W0, H0)
    cfg = lib.default_config(**{k: K0[k] for k in ("width", "height", "fx", "fy", "cx", "cy")}, nb_supersurfels_max=a.rows)
    f = binding.Fusion(lib, cfg)
    f.set_model(model, nvis, 30)
    print("map: %d rows, %d visible" % (a.rows, nvis))
    t_copy = timed(lambda: f.get_model(), max(3, a.reps // 4))
    print("ssf_get_model of the whole map: %.0f us (%.1f MB)" % (t_copy, 104e-6 * a.rows))
    print(json.dumps(dict(arm="get_model", rows=a.rows, us=round(t_copy, 1), mb=round(104e-6 * a.rows, 1))))
    pose = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float32)
    print("%-10s %-8s %9s %9s %9s %9s %9s %8s %10s %12s %10s" % ("camera", "rows", "host_us", "dev_us", "prep_us", "fill_us",
                                                                 "tile_us", "frag/px", "list", "frags/s", "rows/s"))
    for W, H in ((640, 480), (1280, 960)):
        K = synthetic.intrinsics(W, H)
        cam = {k: K[k] for k in ("width", "height", "fx", "fy", "cx", "cy")}
        dev = {nm: torch.empty((H, W) + ((3,) if nm in ("rgb8", "color", "normal") else ()),
                               dtype={"depth": torch.float32, "index": torch.int32, "rgb8": torch.uint8}.get(nm, torch.float32),
                               device="cuda") for nm in OUT}
        ptrs = {nm: t.data_ptr() for nm, t in dev.items()}
        for vis in (False, True):
            host_us = timed(lambda: f.render_model(pose=pose, camera=cam, visible_only=vis), a.reps)
            dev_us = timed(lambda: f.render_model_device(pose=pose, camera=cam, visible_only=vis, **ptrs), a.reps)
            f.set_profile(1)
            f.render_model_device(pose=pose, camera=cam, visible_only=vis, **ptrs)
            f.reset_kernel_times()
            for _ in range(a.reps):
                st = f.render_model_device(pose=pose, camera=cam, visible_only=vis, **ptrs)
            kt = f.kernel_times()
            f.set_profile(0)
            ms = {k: 1e3 * kt[k][0] / max(kt[k][1], 1) for k in ("render_prep", "render_fill", "render_tile") if k in kt}
            ksum = sum(ms.values())
            rows = nvis if vis else a.rows
            row = dict(arm="render", width=W, height=H, visible_only=vis, rows=rows, host_us=round(host_us, 1), device_us=round(dev_us, 1),
                       kernel_us={k: round(v, 1) for k, v in ms.items()}, kernel_sum_us=round(ksum, 1),
                       fragments=st["fragments"], fragments_per_pixel=round(st["fragments"] / (W * H), 1),
                       list_entries=st["list_entries"], pixels_filled=st["pixels_filled"], rows_shown=st["rows_shown"],
                       fragments_per_s=round(st["fragments"] / (dev_us * 1e-6), 0), rows_per_s=round(rows / (dev_us * 1e-6), 0))
            print("%-10s %-8s %9.1f %9.1f %9.1f %9.1f %9.1f %8.1f %10d %12.3g %10.3g" % (
                "%dx%d" % (W, H), "visible" if vis else "all", host_us, dev_us, ms.get("render_prep", 0), ms.get("render_fill", 0),
                ms.get("render_tile", 0), row["fragments_per_pixel"], st["list_entries"], row["fragments_per_s"], row["rows_per_s"]))
            print(json.dumps(row))
    f.close()


if __name__ == "__main__":
    main()
