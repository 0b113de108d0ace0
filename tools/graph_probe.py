"""ssf_graph_* (include/ssf_graph.h) on the 1 M-row map of tools/deform_probe.py: synthetic.seed_model_cam0 through ssf_set_model
with births swept over --frames stamps, N / 50 nodes.

Reports, with a warm-up and --reps repetitions (median, min .. max):
  * the kernel times under profile = 1: graph_rank (keys + counting sort), graph_sample, graph_bind, apply_deformation;
  * the wall time of graph_build and of graph_apply (node transforms uploaded, same kernels, resident binding);
  * today's route on the same handle: get_model, the binding on the host (tests/graph_ref.py: numpy, reported separately), and
    apply_deformation with its row-sized upload, on the same nodes, transforms and binding;
  * graph_bind's share of HBM peak from its algorithmic traffic (20 B read + 32 B written per row + the node table once).
The two deformed maps are compared bit for bit.  Prints a table and one JSON line.

    python tools/graph_probe.py [--rows 1000000] [--reps 10] [--stride 50] [--look 20] [--frames 600]

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
import graph_ref  # noqa: E402

HBM_PEAK_GBS = 8000.0


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--stride", type=int, default=50)
    ap.add_argument("--look", type=int, default=20)
    ap.add_argument("--frames", type=int, default=600)
    a = ap.parse_args()
    lib = binding.load_product()
    W, H = 640, 480
    K = synthetic.intrinsics(W, H)
    f = binding.Fusion(lib, lib.default_config(**dict({k: K[k] for k in ("width", "height", "fx", "fy", "cx", "cy")},
                                                       nb_supersurfels_max=a.rows + 4096)))
    model, nvis = synthetic.seed_model_cam0(a.rows, W, H, stamp=30)
    pos = model["positions"].reshape(a.rows, 3)
    rng = np.random.default_rng(3)
    st = model["stamps"].reshape(a.rows, 2).copy()
    st[:, 0] = ((np.arctan2(pos[:, 2], pos[:, 0]) + np.pi) / (2 * np.pi) * a.frames + rng.integers(0, 30, a.rows)).astype(np.int32)
    model["stamps"] = st.reshape(model["stamps"].shape)
    reset = lambda: f.set_model(model, nvis, a.frames + 40)          # noqa: E731
    reset()

    build = lambda: f.graph_build(stride=a.stride, look=a.look)      # noqa: E731
    t_build = spread(build, a.reps)
    m = f.graph_info()["n_nodes"]
    npos, nt0, nrows = f.graph_nodes()
    w4, idx4 = f.graph_binding()
    ang = rng.uniform(-0.01, 0.01, (m, 3))
    R = np.stack([(synthetic.rot_y(x[1]) @ synthetic.rot_x(x[0])).reshape(9) for x in ang]).astype(np.float32)
    t = rng.uniform(-1e-3, 1e-3, (m, 3)).astype(np.float32)

    # the resident route: every repetition starts from the same map and a fresh graph (not timed)
    t_apply = spread(lambda: f.graph_apply(R, t), a.reps, before=lambda: (reset(), build()))
    deformed_graph = f.get_model()
    # today's route on the same handle
    t_get = spread(lambda: f.get_model(), max(3, a.reps // 2), before=None)
    reset()
    t0 = time.perf_counter()
    (hp, ht, hr), (hw, hi) = graph_ref.bind_model(f.get_model(), a.stride, a.look)
    t_host = 1e6 * (time.perf_counter() - t0)
    same_graph = bool(np.array_equal(hr, nrows) and hw.tobytes() == w4.tobytes() and hi.tobytes() == idx4.tobytes())
    t_old = spread(lambda: f.apply_deformation(npos, R, t, w4, idx4), a.reps, before=reset)
    deformed_old = f.get_model()
    same_map = all(deformed_graph[k].tobytes() == deformed_old[k].tobytes() for k in deformed_old)

    f.set_profile(1)
    reset(); build(); f.graph_apply(R, t)
    f.reset_kernel_times()
    for _ in range(a.reps):
        reset(); build(); f.graph_apply(R, t)
    kt = f.kernel_times()
    f.set_profile(0)
    # per build / per apply: graph_rank is two timed groups per build (keys, then the sort passes)
    us = {k: 1e3 * kt[k][0] / a.reps for k in ("graph_rank", "graph_sample", "graph_bind", "apply_deformation") if k in kt}
    bind_bytes = 52.0 * a.rows + 16.0 * m
    bind_gbs = bind_bytes / (us.get("graph_bind", float("nan")) * 1e3)

    print("map: %d rows (%d visible), %d stamps, stride %d, look %d -> %d nodes" % (a.rows, nvis, a.frames, a.stride, a.look, m))
    print("kernels under profile = 1 (us per build / per apply, mean of %d):" % a.reps)
    for k, v in us.items():
        print("  %-18s %9.1f   (%d timed groups per call)" % (k, v, kt[k][1] // a.reps))
    print("  graph_bind: %.1f MB algorithmic -> %.0f GB/s = %.3f of %.0f GB/s HBM peak" % (bind_bytes / 1e6, bind_gbs, bind_gbs / HBM_PEAK_GBS, HBM_PEAK_GBS))
    print("wall clock, us (median, min .. max of %d):" % a.reps)
    for name, v in (("graph_build", t_build), ("graph_apply", t_apply), ("get_model", t_get), ("apply_deformation", t_old)):
        print("  %-18s %10.0f  %10.0f .. %-10.0f" % (name, v[0], v[1], v[2]))
    print("  %-18s %10.0f  (numpy, one run)" % ("host binding", t_host))
    print("  resident route  build + apply                       : %10.0f" % (t_build[0] + t_apply[0]))
    print("  today's route   get_model + host + apply_deformation: %10.0f" % (t_get[0] + t_host + t_old[0]))
    print("graph_apply / apply_deformation = %.3f   host graph == device graph: %s   deformed maps identical: %s" % (
        t_apply[0] / t_old[0], same_graph, same_map))
    print(json.dumps(dict(rows=a.rows, nodes=m, stride=a.stride, look=a.look, kernel_us={k: round(v, 1) for k, v in us.items()},
                          graph_build_us=[round(x) for x in t_build], graph_apply_us=[round(x) for x in t_apply],
                          get_model_us=[round(x) for x in t_get], host_binding_us=round(t_host),
                          apply_deformation_us=[round(x) for x in t_old], apply_ratio=round(t_apply[0] / t_old[0], 3),
                          bind_gbs=round(bind_gbs, 1), bind_hbm_fraction=round(bind_gbs / HBM_PEAK_GBS, 4),
                          same_graph=same_graph, same_map=same_map)))
    f.close()
    return 0 if (same_graph and same_map) else 1


if __name__ == "__main__":
    sys.exit(main())
