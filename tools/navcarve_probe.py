"""ssf_navgrid_carve (include/ssf_navcarve.h) on the 1 M-row map of the other probes: synthetic.seed_model_cam0 through
ssf_set_model, --views views along the synthetic orbit (synthetic.relative_pose), 640 x 480 intrinsics on a pixel lattice of
--stride, a 512 x 512 grid at 0.05 m in the default frame with the height bands taken from the map (as tools/navgrid_probe.py).

Reports, with warm-ups and --reps repetitions (medians; kernels by the hipEvent brackets of ssf_get_kernel_times under profile = 1):
  * nav_grid ALONE (ssf_navgrid_build into device memory): per kernel, summed, and the wall clock of the call -- the figure to
    compare between two builds of the library (--lib PATH loads another one, e.g. a build of the parent commit; a library that
    does not export the carve gets this part only);
  * the carve into device memory: per kernel (navgrid_*, navcarve_rays, raycast_march, navcarve_march), the wall clock of the whole
    call, rays / hits / samples / entries, and the atomics issued on `seen` per entry;
  * the alternative a caller has today: Fusion.raycast for the same rays (host rays in, t and index out) plus the numpy carve of
    tests/navcarve_ref.py, on all views or the first --host-views (the numpy part is a Python loop over the rays: slow), with the
    device's `seen` for those views compared bit for bit.
Prints a table and JSON lines; --out also writes them to a file.  No threshold is asserted: the table is the record.

    python tools/navcarve_probe.py [--rows 1000000] [--views 64] [--stride 8] [--reps 10] [--host-views 0] [--lib PATH] [--grid-only] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from supersurfel_fusion_amd import binding, synthetic  # noqa: E402
import navcarve_ref as nc  # noqa: E402
import navgrid_ref as nr  # noqa: E402
import raycast_ref as rr  # noqa: E402

WARM = 3
GRID_KERNELS = ("navgrid_prep", "navgrid_fill", "navgrid_tile", "navgrid_cells", "navgrid_columns", "navgrid_rows")
CARVE_KERNELS = GRID_KERNELS + ("navcarve_rays", "raycast_march", "navcarve_march")


def measure(f, fn, names, reps):
    """(median kernel ms by name, median wall ms of the call with profile off)"""
    f.set_profile(1)
    per = []
    for k in range(WARM + reps):
        f.reset_kernel_times()
        fn()
        kt = f.kernel_times()
        if k >= WARM:
            per.append([kt.get(nm, (0.0, 0))[0] for nm in names])
    f.set_profile(0)
    wall = []
    for k in range(WARM + reps):
        t0 = time.perf_counter()
        fn()
        if k >= WARM:
            wall.append(time.perf_counter() - t0)
    return dict(zip(names, np.median(np.array(per), axis=0).tolist())), 1e3 * float(np.median(wall))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--views", type=int, default=64)
    ap.add_argument("--stride", type=int, default=8)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-views", type=int, default=0, help="views of the host alternative (0 = all)")
    ap.add_argument("--lib", default=None, help="the library to load instead of libssf_hip_navcarve.so")
    ap.add_argument("--label", default=None)
    ap.add_argument("--grid-only", action="store_true", help="nav_grid alone, nothing else (the comparison between two builds)")
    ap.add_argument("--out", default=None, help="also append the table and the JSON lines to this file")
    a = ap.parse_args()
    import torch
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    lib = binding.Library(a.lib) if a.lib else binding.load_navcarve()
    label = a.label or (a.lib or "navcarve")
    W, H = 640, 480
    K = synthetic.intrinsics(W, H)
    cam = {k: K[k] for k in ("width", "height", "fx", "fy", "cx", "cy")}
    model, nvis = synthetic.seed_model_cam0(a.rows, W, H, stamp=30)
    f = binding.Fusion(lib, lib.default_config(**cam, nb_supersurfels_max=a.rows + 4096))
    f.set_model(model, nvis, 30)
    y = model["positions"][:, 1]
    bands = dict(z_min=float(-y.max() - 0.1), z_max=float(-y.min() + 0.1), floor_max=float(-np.median(y)))
    kw = dict(width=512, height=512, res=0.05, **bands)
    P = 512 * 512
    dev = {nm: torch.zeros(P * (2 if nm == "hits" else 1), dtype={"uint32": torch.int32}.get(np.dtype(dt).name) or getattr(torch, np.dtype(dt).name),
                           device="cuda") for nm, dt, _ in binding.NAVGRID_OUTPUTS}
    say("[%s] map: synthetic %d rows, %d visible; grid 512x512@0.05, bands %s; %d calls per figure after %d warm-ups; times in ms" %
        (label, a.rows, nvis, json.dumps(bands), a.reps, WARM))
    # ---- nav_grid alone
    kern, wall = measure(f, lambda: f.nav_grid_device(**dict(kw, **dev)), GRID_KERNELS, a.reps)
    say("[%s] nav_grid alone: %s | kernels %.4f | wall %.3f" % (label, "  ".join("%s %.4f" % (k[8:], v) for k, v in kern.items()), sum(kern.values()), wall))
    say(json.dumps(dict(label=label, what="nav_grid alone", kernel_ms={k: round(v, 4) for k, v in kern.items()}, kernels_ms=round(sum(kern.values()), 4),
                        wall_ms=round(wall, 3))))
    if lib.has_navcarve and not a.grid_only:
        views = np.stack([nr.pose_about(*synthetic.relative_pose(k)) for k in range(a.views)])      # (the map frame is the first camera's)
        carve = dict(stride=a.stride)
        seen = torch.zeros(P, dtype=torch.int32, device="cuda")
        stats = []
        kern, wall = measure(f, lambda: stats.append(f.nav_grid_carve_device(views, carve=carve, seen=seen, **dict(kw, **dev))), CARVE_KERNELS, a.reps)
        st, last = stats[-1], f.debug_navcarve_last()
        say("[%s] carve, %d views, stride %d: %d rays, %d hit, %d carving, %d samples, %d entries, %d cells seen, %d carved; %d atomics = %.3f per entry" %
            (label, a.views, a.stride, st["rays"], st["rays_hit"], st["rays_carving"], st["ray_samples"], st["ray_entries"], st["cells_seen"],
             st["cells_carved"], last["atomics"], last["atomics"] / max(1, st["ray_entries"])))
        say("[%s] carve kernels: %s | kernels %.4f | wall of the whole call %.3f" %
            (label, "  ".join("%s %.4f" % (k, v) for k, v in kern.items()), sum(kern.values()), wall))
        say(json.dumps(dict(label=label, what="carve", views=a.views, stride=a.stride, stats={k: v for k, v in st.items() if k != "pose"},
                            atomics=last["atomics"], chunks=last["chunks"], kernel_ms={k: round(v, 4) for k, v in kern.items()},
                            kernels_ms=round(sum(kern.values()), 4), wall_ms=round(wall, 3))))
        # ---- today's route on the first views: the rays cast by the device, the carve in numpy
        hv = views[:a.host_views] if 0 < a.host_views < a.views else views
        q = nr.params(**kw)
        c = nc.params(cfg_camera=cam, range_min=f.cfg.range_min, range_max=f.cfg.range_max, **carve)
        pose = nr.default_pose(f.get_pose(), q)
        t0 = time.perf_counter()
        rays = nc.map_rays(hv, c)
        got = f.raycast(rays, outputs=("t", "index"), pose=nr.IDENTITY, t_min=c["t_min"], t_max=c["t_max"])
        t_cast = time.perf_counter() - t0
        t0 = time.perf_counter()
        hit, valid = got["index"] >= 0, rr.transform(rays, nr.IDENTITY)[2]
        M = nc.extent(got["t"], hit, valid, q, c)
        want = np.zeros(P, np.uint32)
        for r in np.flatnonzero(M >= 0):
            cell = nc.sample_cells(rays[r, :3], rays[r, 3:], int(M[r]), pose, q)
            np.add.at(want, cell[nc.entries(cell)], 1)
        t_np = time.perf_counter() - t0
        sub = f.nav_grid_carve(hv, outputs=("seen",), carve=carve, **kw)
        equal = bool(np.array_equal(sub["seen"].ravel(), want))
        t_call = []
        for _ in range(3):
            t0 = time.perf_counter()
            f.nav_grid_carve_device(hv, carve=carve, seen=seen, **dict(kw, **dev))
            t_call.append(time.perf_counter() - t0)
        say("[%s] today's route on %d views (%d rays): Fusion.raycast %.2f ms + numpy carve %.1f ms = %.1f ms (%.1f ms per view, without the grid "
            "itself); the device call for the same views, grid included: %.3f ms; seen equal bit for bit: %s" %
            (label, len(hv), len(rays), 1e3 * t_cast, 1e3 * t_np, 1e3 * (t_cast + t_np), 1e3 * (t_cast + t_np) / len(hv), 1e3 * float(np.median(t_call)), equal))
        say(json.dumps(dict(label=label, what="today's route", host_views=len(hv), rays=len(rays), raycast_ms=round(1e3 * t_cast, 3),
                            numpy_carve_ms=round(1e3 * t_np, 1), device_call_ms=round(1e3 * float(np.median(t_call)), 3), seen_equal=equal)))
    f.close()
    if a.out:
        with open(a.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
