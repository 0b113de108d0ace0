"""ssf_navgrid_build (include/ssf_navgrid.h) measured on two maps: the metric's (synthetic.seed_model_cam0 at ~1 M rows through
ssf_set_model with the bench's visible split, as tools/query_probe.py) and the map of the 8 committed TUM fr1_xyz frames.  Two
grids each, in the default frame (floor-aligned about the camera): 512 x 512 at 0.05 m and 1024 x 1024 at 0.025 m.  The height
bands are taken from the map (neither scene has a floor a metre below its first camera): z_min / z_max enclose every row,
floor_max is the median height, so about half the samples are floor-band and half obstacle-band samples.

Per arm: kernel milliseconds per call by hipEvent through ssf_get_kernel_times (profile = 1; per kernel and summed, the median of
--reps calls after 3 warm-ups), the wall clock of the whole call with host outputs (all five arrays copied out) and with device
outputs, the average samples per row and list entries per tile, and beside them what a caller had to do without this call:
get_model of everything, then tests/navgrid_ref.py's build() on the host (wall clock; --host-reps runs, it is slow).  The device
grid is compared with that host grid on the way (every output and stat, 0 bits).  No threshold is asserted: the table is the
record.

    python tools/navgrid_probe.py [--rows 1000000] [--reps 20] [--host-reps 1] [--out profiles/navgrid.txt]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from supersurfel_fusion_amd import binding, replay, synthetic  # noqa: E402
import navgrid_ref as nr  # noqa: E402

WARM = 3
KERNELS = ("navgrid_prep", "navgrid_fill", "navgrid_tile", "navgrid_cells", "navgrid_columns", "navgrid_rows")
GRIDS = ((512, 512, 0.05), (1024, 1024, 0.025))


def median_wall_ms(fn, reps, warm=WARM):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(t))


def median_kernel_ms(f, fn, reps):
    f.set_profile(1)
    per = []
    for k in range(WARM + reps):
        f.reset_kernel_times()
        fn()
        kt = f.kernel_times()
        if k >= WARM:
            per.append({nm: kt[nm][0] for nm in KERNELS if nm in kt})
    f.set_profile(0)
    return float(np.median([sum(p.values()) for p in per])), {nm: float(np.median([p.get(nm, 0.0) for p in per])) for nm in KERNELS}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--out", default=None, help="also write the table and the JSON lines to this file")
    a = ap.parse_args()
    import torch
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    lib = binding.load_product()
    W, H = 640, 480
    K = synthetic.intrinsics(W, H)
    cam = {k: K[k] for k in ("width", "height", "fx", "fy", "cx", "cy")}
    maps = []
    model, nvis = synthetic.seed_model_cam0(a.rows, W, H, stamp=30)
    f = binding.Fusion(lib, lib.default_config(**cam, nb_supersurfels_max=a.rows))
    f.set_model(model, nvis, 30)
    maps.append(("synthetic %d rows" % a.rows, f))
    g = binding.Fusion(lib, lib.default_config(**dict(replay.BENCHMARK_LAUNCH, nb_supersurfels_max=20000)))
    replay.replay(g, replay.frames_from_npz(os.path.join(ROOT, "tests", "golden", "tum_fr1_xyz_8frames.npz")))
    maps.append(("fr1_xyz 8 frames", g))
    say("%d calls per figure after %d warm-ups (the host alternative: %d); MI355X; times in ms" % (a.reps, WARM, a.host_reps))
    say("%-24s %-16s %9s %9s %9s %8s %8s %8s %8s %8s %8s %8s %10s %10s %12s" % ("map", "grid", "rows", "smp/row", "ent/tile", "prep", "fill", "tile", "cells",
                                                                              "columns", "rows_k", "kernels", "host_wall", "dev_wall", "copy+numpy"))
    for label, f in maps:
        m = f.get_model()
        n, nv = f.counts()["n_model"], f.counts()["n_visible"]
        y = m["positions"][:, 1]
        bands = dict(z_min=float(-y.max() - 0.1), z_max=float(-y.min() + 0.1), floor_max=float(-np.median(y)))
        t_copy = median_wall_ms(lambda: f.get_model(), 5)
        say("%s: %d rows, %d visible; get_model of the whole map %.2f ms wall (%.1f MB); bands %s" % (label, n, nv, t_copy, 104e-6 * n, json.dumps(bands)))
        for gw, gh, res in GRIDS:
            kw = dict(width=gw, height=gh, res=res, **bands)
            got = f.nav_grid(**kw)
            st = got["stats"]
            t0 = time.perf_counter()
            for _ in range(a.host_reps):
                want = nr.build(f.get_model(), nv, nr.default_pose(f.get_pose(), nr.params(**kw)), nr.params(**kw))
            base = 1e3 * (time.perf_counter() - t0) / a.host_reps
            same = all(np.array_equal(got[nm].view(np.uint8), want[nm].view(np.uint8)) for nm in nr.OUTPUTS) and \
                all(st[k] == want["stats"][k] for k in nr.STATS)
            P = gw * gh
            dev = {nm: torch.zeros(P * (2 if nm == "hits" else 1), dtype={"uint32": torch.int32}.get(np.dtype(dt).name) or
                                   getattr(torch, np.dtype(dt).name), device="cuda") for nm, dt, _ in binding.NAVGRID_OUTPUTS}
            kern, split = median_kernel_ms(f, lambda: f.nav_grid_device(**dict(kw, **dev)), a.reps)
            host_wall = median_wall_ms(lambda: f.nav_grid(**kw), a.reps)
            dev_wall = median_wall_ms(lambda: f.nav_grid_device(**dict(kw, **dev)), a.reps)
            dist_wall = median_wall_ms(lambda: f.nav_grid(outputs=("state", "dist2"), **kw), a.reps)
            ntiles = ((gw + 31) // 32) * ((gh + 31) // 32)
            row = dict(map=label, grid="%dx%d@%g" % (gw, gh, res), rows=n, rows_used=st["rows_used"], samples=st["samples"],
                       samples_in_grid=st["samples_in_grid"], samples_per_row=round(st["samples"] / max(1, st["rows_used"]), 2),
                       list_entries=st["list_entries"], entries_per_tile=round(st["list_entries"] / ntiles, 1),
                       cells=dict(free=st["cells_free"], occupied=st["cells_occupied"], unknown=st["cells_unknown"]),
                       kernel_ms={k: round(v, 4) for k, v in split.items()}, kernels_ms=round(kern, 4), host_wall_ms=round(host_wall, 3),
                       device_wall_ms=round(dev_wall, 3), state_dist2_host_wall_ms=round(dist_wall, 3),
                       get_model_numpy_wall_ms=round(base, 1), equals_the_host_grid=bool(same))
            say("%-24s %-16s %9d %9.2f %9.1f %8.4f %8.4f %8.4f %8.4f %8.4f %8.4f %8.4f %10.3f %10.3f %12.1f" % (
                label, row["grid"], st["rows_used"], row["samples_per_row"], row["entries_per_tile"], split["navgrid_prep"], split["navgrid_fill"],
                split["navgrid_tile"], split["navgrid_cells"], split["navgrid_columns"], split["navgrid_rows"], kern, host_wall, dev_wall, base))
            say(json.dumps(row))
    for _, f in maps:
        f.close()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
