"""ssf_raycast (include/ssf_raycast.h) on the 1 M-row map of the other probes: synthetic.seed_model_cam0 through ssf_set_model, rays
from the first camera (the map frame's origin) in device memory.

Reports, with warm-ups and --reps repetitions (medians of the hipEvent brackets of ssf_get_kernel_times under profile = 1):
  * raycast_march for 1 k, 64 k and 1 M rays, as a lidar FAN (rings of constant elevation, neighbours in memory are neighbours in
    space) and SHUFFLED (the same rays in random order), for both forms of the march: one ray per wave (the product) and one ray per
    lane (the laboratory build's arm, SSF_RAYCAST_LANE=1) -- the two give the same bits, which is checked;
  * the index's build: raycast_prep (prep + count), raycast_scan, raycast_fill, and their share of HBM peak from the algorithmic
    traffic (prep: 104 B read + 80 B written per row; count: 16 B per row; fill: 16 B per row + 4 B per entry);
  * the alternative a caller has today: get_model (104 B per row) plus the numpy brute force of tests/raycast_ref.py on --host-rays
    rays, and whether the device results equal it bit for bit.
Prints tables and JSON lines.

    python tools/raycast_probe.py [--rows 1000000] [--reps 10] [--host-rays 64] [--cell 0]

For a kernel trace run it under rocprofv3 --kernel-trace --stats; for counters, a run of its own."""
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
import raycast_ref  # noqa: E402

HBM_PEAK_GBS = 8000.0


def lidar_fan(n):
    """n unit rays from the origin: rings of constant elevation (-25 .. 25 degrees about the camera's x-z plane), each a full
    circle, ring-major: consecutive rays are neighbours in azimuth"""
    rings = max(1, int(round(np.sqrt(n / 16.0))))
    per = (n + rings - 1) // rings
    el = np.deg2rad(np.linspace(-25.0, 25.0, rings))[:, None]
    az = (-np.pi + np.arange(per) * (2.0 * np.pi / per))[None, :]
    d = np.stack([np.cos(el) * np.sin(az), np.sin(el) * np.ones_like(az), np.cos(el) * np.cos(az)], axis=-1).reshape(-1, 3)[:n]
    return np.concatenate([np.zeros_like(d), d], axis=1).astype(np.float32)


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-rays", type=int, default=64)
    ap.add_argument("--cell", type=float, default=0.0)
    ap.add_argument("--counts", type=int, nargs="*", default=[1000, 65536, 1000000])
    a = ap.parse_args()
    lib = binding.load_lab()
    W, H = 640, 480
    K = synthetic.intrinsics(W, H)
    f = binding.Fusion(lib, lib.default_config(**dict({k: K[k] for k in ("width", "height", "fx", "fy", "cx", "cy")},
                                                       nb_supersurfels_max=a.rows + 4096, profile=1)))
    model, nvis = synthetic.seed_model_cam0(a.rows, W, H, stamp=30)
    f.set_model(model, nvis, 30)
    kw = dict(t_min=0.2, t_max=30.0, cell=a.cell)
    pose = raycast_ref.IDENTITY

    def kernel_ms(fn, names, reps, warm=2):
        rows = []
        for k in range(warm + reps):
            f.reset_kernel_times()
            fn()
            kt = f.kernel_times()
            if k >= warm:
                rows.append([kt.get(nm, (0.0, 0))[0] for nm in names])
        return dict(zip(names, np.median(np.array(rows), axis=0).tolist()))

    # ---- the build: every call with another hash_bits rebuilds; alternate between two values around the default's
    one = torch.from_numpy(lidar_fan(64)).cuda()
    t1 = torch.zeros(64, dtype=torch.float32, device="cuda")
    st = f.raycast_device(one, 64, t=t1, pose=pose, **kw)
    flip = [0]

    def rebuild():
        flip[0] ^= 1
        s = f.raycast_device(one, 64, t=t1, pose=pose, hash_bits=(18 if flip[0] else 19), **kw)
        assert s["index_rebuilt"] == 1
    names = ("raycast_prep", "raycast_scan", "raycast_fill", "raycast_march")
    b = kernel_ms(rebuild, names, a.reps)
    rows_n, ent = st["rows_indexed"], st["index_entries"]
    traffic = dict(raycast_prep=rows_n * (104 + 80 + 16), raycast_fill=rows_n * 16 + ent * 8)
    print("map: synthetic %d rows, %d visible; cell %s; index: %d rows (%d oversize), %d entries (%.1f per row), default table" %
          (a.rows, nvis, a.cell or "default", rows_n, st["rows_oversize"], ent, ent / max(rows_n - st["rows_oversize"], 1)))
    print("build (hash_bits 18 / 19 alternating; ms, median of %d): prep+count %.4f  scan %.4f  fill %.4f  total %.4f" %
          (a.reps, b["raycast_prep"], b["raycast_scan"], b["raycast_fill"], b["raycast_prep"] + b["raycast_scan"] + b["raycast_fill"]))
    share = {k: traffic[k] / (b[k] * 1e-3) / 1e9 / HBM_PEAK_GBS for k in traffic}
    print("share of HBM peak (%.0f GB/s) from the algorithmic traffic: prep+count %.1f %% (%.1f MB)  fill %.1f %% (%.1f MB)" %
          (HBM_PEAK_GBS, 100 * share["raycast_prep"], traffic["raycast_prep"] / 1e6, 100 * share["raycast_fill"], traffic["raycast_fill"] / 1e6))
    print(json.dumps(dict(rows=a.rows, rows_indexed=rows_n, rows_oversize=st["rows_oversize"], index_entries=ent, build_ms=b,
                          hbm_share={k: round(v, 4) for k, v in share.items()})))

    # ---- the march, both forms
    print("%-9s %-9s %9s %10s %12s %12s %12s %10s" % ("rays", "order", "hit", "cells/ray", "tested/ray", "wave ms", "lane ms", "same bits"))
    rng = np.random.default_rng(5)
    for n in a.counts:
        fan = lidar_fan(n)
        for order, rays in (("fan", fan), ("shuffled", fan[rng.permutation(n)])):
            d = torch.from_numpy(rays).cuda()
            outs = {nm: torch.zeros(n * (3 if tail else 1), dtype=torch.int32 if dt is np.int32 else torch.float32, device="cuda")
                    for nm, dt, tail in binding.RAYCAST_OUTPUTS}
            res = {}
            for form in ("wave", "lane"):
                if form == "lane":
                    os.environ["SSF_RAYCAST_LANE"] = "1"
                else:
                    os.environ.pop("SSF_RAYCAST_LANE", None)
                stats = []
                ms = kernel_ms(lambda: stats.append(f.raycast_device(d, n, pose=pose, **dict(kw, **outs))), ("raycast_march",), a.reps)["raycast_march"]
                assert stats[-1]["index_rebuilt"] == 0
                res[form] = (ms, stats[-1], {nm: t.cpu().numpy().copy() for nm, t in outs.items()})
            os.environ.pop("SSF_RAYCAST_LANE", None)
            same = all(np.array_equal(res["wave"][2][nm].view(np.uint32), res["lane"][2][nm].view(np.uint32)) for nm in outs)
            s = res["wave"][1]
            print("%-9d %-9s %9d %10.1f %12.1f %12.4f %12.4f %10s" % (n, order, s["rays_hit"], s["cells_visited"] / n, s["candidates_tested"] / n,
                                                                     res["wave"][0], res["lane"][0], same))
            print(json.dumps(dict(rays=n, order=order, rays_hit=s["rays_hit"], cells_visited=s["cells_visited"], candidates_tested=s["candidates_tested"],
                                  wave_ms=res["wave"][0], lane_ms=res["lane"][0], lane_cells_visited=res["lane"][1]["cells_visited"], same_bits=same)))

    # ---- today's route: the whole model out, the brute force on the host
    t0 = time.perf_counter()
    host = f.get_model()
    t_get = time.perf_counter() - t0
    rays = lidar_fan(a.host_rays)
    t0 = time.perf_counter()
    want = raycast_ref.cast(host, nvis, rays, pose, raycast_ref.params(**kw), chunk=8)
    t_np = time.perf_counter() - t0
    got = f.raycast(rays, pose=pose, **kw)
    same = all(np.array_equal(np.ascontiguousarray(got[nm]).view(np.uint32), np.ascontiguousarray(want[nm]).view(np.uint32)) for nm in raycast_ref.OUTPUTS)
    print("today's route: get_model %.1f ms (%.1f MB) + numpy brute force of %d rays %.1f ms = %.2f ms per ray; the device call equals it bit for bit: %s" %
          (1e3 * t_get, 104e-6 * a.rows, a.host_rays, 1e3 * t_np, 1e3 * t_np / a.host_rays, same))
    print(json.dumps(dict(get_model_ms=1e3 * t_get, host_rays=a.host_rays, numpy_ms=1e3 * t_np, equals_the_host=same)))


if __name__ == "__main__":
    main()
