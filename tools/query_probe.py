"""ssf_query_count / ssf_query_rows (include/ssf_query.h) on the metric's map: synthetic.seed_model_cam0 at ~1 M rows through
ssf_set_model with the bench's visible split (as tools/render_probe.py).  Three selections -- a 2 m sphere about the camera, the
camera's frustum, min_conf = conf_thresh over the whole map -- each with all fields and with positions + colours only.

Per arm: kernel milliseconds per call by hipEvent through ssf_get_kernel_times (profile = 1: query_select + query_scan for a count,
+ query_gather for the rows; the median of --reps calls after 3 warm-ups), the wall clock of the whole call with host outputs
(the copy of the selected rows included) and with device outputs, and beside them the same selection done the way it had to be
done without these calls: get_model of everything, then a numpy filter on the host (wall clock, median).  No threshold is
asserted: the table is the record.

    python tools/query_probe.py [--rows 1000000] [--reps 20] [--out profiles/query.txt]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from supersurfel_fusion_amd import binding, synthetic  # noqa: E402

ALL = tuple(name for name, _, _ in binding.SURFEL_FIELDS)
WARM = 3


def median_wall_ms(fn, reps):
    for _ in range(WARM):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(t))


def median_kernel_ms(f, fn, reps):
    """median over the calls of the summed query_* hipEvent brackets of one call, and the per-kernel medians"""
    f.set_profile(1)
    per = []
    for k in range(WARM + reps):
        f.reset_kernel_times()
        fn()
        kt = f.kernel_times()
        if k >= WARM:
            per.append({nm: kt[nm][0] for nm in ("query_select", "query_scan", "query_gather") if nm in kt})
    f.set_profile(0)
    names = sorted({nm for p in per for nm in p})
    return float(np.median([sum(p.values()) for p in per])), {nm: float(np.median([p.get(nm, 0.0) for p in per])) for nm in names}


def host_filter(model, kind, cam, zr, conf_thresh):
    """the selection by numpy on a host copy of the whole model (camera 0 = the identity pose)"""
    pos = model["positions"]
    if kind == "sphere":
        return np.flatnonzero((pos * pos).sum(axis=1) <= np.float32(4.0))
    if kind == "conf":
        return np.flatnonzero(model["confidences"] > np.float32(conf_thresh))
    z = pos[:, 2]
    with np.errstate(all="ignore"):
        u = np.float32(cam["fx"]) * pos[:, 0] / z + np.float32(cam["cx"])
        v = np.float32(cam["fy"]) * pos[:, 1] / z + np.float32(cam["cy"])
    return np.flatnonzero((z >= zr[0]) & (z <= zr[1]) & (u >= -0.5) & (u < cam["width"] - 0.5) & (v >= -0.5) & (v < cam["height"] - 0.5))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None, help="also write the table and the JSON lines to this file")
    a = ap.parse_args()
    import torch
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    lib = binding.load_product()
    W, H = 640, 480
    model, nvis = synthetic.seed_model_cam0(a.rows, W, H, stamp=30)
    K = synthetic.intrinsics(W, H)
    cam = {k: K[k] for k in ("width", "height", "fx", "fy", "cx", "cy")}
    cfg = lib.default_config(**cam, nb_supersurfels_max=a.rows)
    f = binding.Fusion(lib, cfg)
    f.set_model(model, nvis, 30)
    zr = (cfg.range_min, cfg.range_max)
    pose = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float32)
    say("map: %d rows, %d visible; %d calls per figure after %d warm-ups; MI355X" % (a.rows, nvis, a.reps, WARM))
    t_copy = median_wall_ms(lambda: f.get_model(), max(5, a.reps // 4))
    say("get_model of the whole map: %.2f ms wall (%.1f MB)" % (t_copy, 104e-6 * a.rows))
    arms = (("sphere 2 m", "sphere", dict(region="sphere", radius=2.0, pose=pose)),
            ("frustum", "frustum", dict(region="frustum", pose=pose)),
            ("conf > conf_thresh", "conf", dict(min_conf=cfg.conf_thresh)))
    say("%-20s %-18s %9s %10s %10s %10s %11s %11s %13s" % ("selection", "fields", "selected", "count_ms", "rows_ms", "gather_ms",
                                                        "host_wall", "dev_wall", "copy+numpy"))
    for label, kind, kw in arms:
        n = f.query_count(**kw)["n_selected"]
        host_n = len(host_filter(f.get_model(), kind, cam, zr, cfg.conf_thresh))
        for fields in (ALL, ("positions", "colors")):
            shape = {name: (k, dt) for name, k, dt in binding.SURFEL_FIELDS}
            arrays = {nm: np.zeros((max(n, 1), shape[nm][0]) if shape[nm][0] > 1 else (max(n, 1),), shape[nm][1]) for nm in fields}
            index = np.zeros(max(n, 1), np.int32)
            dev = {nm: torch.zeros(arrays[nm].shape, dtype=getattr(torch, np.dtype(shape[nm][1]).name), device="cuda") for nm in fields}
            dindex = torch.zeros(max(n, 1), dtype=torch.int32, device="cuda")
            count_ms, _ = median_kernel_ms(f, lambda: f.query_count(**kw), a.reps)
            rows_ms, split = median_kernel_ms(f, lambda: f.query_model_device(dev, index=dindex, **kw), a.reps)
            host_wall = median_wall_ms(lambda: f.query_rows_into(arrays, index, max(n, 1), **kw), a.reps)
            dev_wall = median_wall_ms(lambda: f.query_model_device(dev, index=dindex, **kw), a.reps)

            def baseline():
                m = f.get_model()
                idx = host_filter(m, kind, cam, zr, cfg.conf_thresh)
                return {nm: m[nm][idx] for nm in fields}, idx
            base = median_wall_ms(baseline, max(5, a.reps // 4))
            row = dict(arm=label, fields="all" if fields == ALL else "+".join(fields), rows=a.rows, selected=n, host_filter_selected=host_n,
                       count_kernel_ms=round(count_ms, 4), rows_kernel_ms=round(rows_ms, 4),
                       kernel_split_ms={k: round(v, 4) for k, v in split.items()}, rows_host_wall_ms=round(host_wall, 3),
                       rows_device_wall_ms=round(dev_wall, 3), get_model_numpy_wall_ms=round(base, 2))
            say("%-20s %-18s %9d %10.4f %10.4f %10.4f %11.3f %11.3f %13.2f" % (label, row["fields"], n, count_ms, rows_ms,
                                                                           split.get("query_gather", 0.0), host_wall, dev_wall, base))
            say(json.dumps(row))
    f.close()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
