"""ssf_graph_solve (include/ssf_graph_solve.h) on the seeded map of tools/graph_probe.py: births swept over --frames stamps, the rows
born in the last 30 % rotated by --deg degrees about the vertical through their centroid, the rest pinned; --constraints random
rows are the constraints.

Reports per map size (--rows, several allowed):
  * graph_solve: wall time, outer steps, inner iterations per step, how the last inner loop ended, microseconds per inner
    iteration (the graph_solve kernel time under profile = 1 over the iterations) and launches per iteration (3, by construction);
  * the host route on the same inputs: graph_nodes + graph_bind_points + the scipy direct Gauss-Newton of the CPU test
    (tests/graph_solve_ref.py: direct_gauss_newton) + graph_apply; the relative gap of the two final energies.
Prints a table and one JSON line per size; --out appends the text to a file (profiles/graph_solve.txt).

    python tools/graph_solve_probe.py [--rows 1000000 100000] [--stride 50] [--look 20] [--constraints 10000] [--no-host]"""
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
import graph_solve_ref as gs  # noqa: E402

f32, f64 = np.float32, np.float64


def rot_y(deg):
    a = np.deg2rad(deg)
    return np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])


def probe(lib, rows, a, say):
    W, H = 640, 480
    K = synthetic.intrinsics(W, H)
    f = binding.Fusion(lib, lib.default_config(**dict({k: K[k] for k in ("width", "height", "fx", "fy", "cx", "cy")},
                                                       nb_supersurfels_max=rows + 4096, profile=1)))
    model, nvis = synthetic.seed_model_cam0(rows, W, H, stamp=30)
    pos = np.ascontiguousarray(model["positions"], f32).reshape(rows, 3)
    rng = np.random.default_rng(3)
    az = np.arctan2(pos[:, 2], pos[:, 0])
    t0 = ((az + np.pi) / (2 * np.pi) * a.frames + rng.integers(0, max(1, a.frames // 20), rows)).astype(np.int32)
    st = model["stamps"].reshape(rows, 2).copy(); st[:, 0] = t0
    model["stamps"] = st.reshape(model["stamps"].shape)
    f.set_model(model, nvis, a.frames + 100)
    m = f.graph_build(stride=a.stride, look=a.look)
    pick = rng.choice(rows, min(a.constraints, rows), replace=False)
    late = t0 >= int(0.7 * a.frames)
    c = pos[late].mean(axis=0).astype(f64)
    target = np.where(late[:, None], (pos.astype(f64) - c) @ rot_y(a.deg).T + c, pos.astype(f64)).astype(f32)
    src, ts, dst = pos[pick], t0[pick], target[pick]
    f.graph_solve(src, ts, dst, max_outer=1, max_inner=16)           # warm-up: buffers allocated, code loaded
    k0 = f.kernel_times().get("graph_solve", (0.0, 0))[0]
    t = time.perf_counter()
    res = f.graph_solve(src, ts, dst)
    wall = time.perf_counter() - t
    dev_ms = f.kernel_times()["graph_solve"][0] - k0
    inner = sum(res["inner"])
    out = dict(rows=rows, nodes=m, constraints=len(src), wall_ms=1e3 * wall, outer=res["outer"], inner=res["inner"],
               inner_end=binding.GRAPH_SOLVE_ENDS[res["inner_end"]], e_before=res["e_before"], e_after=res["e_after"],
               us_per_inner_wall=1e6 * wall / max(inner, 1), kernel_ms=dev_ms, launches_per_inner=3)
    say("rows %d nodes %d constraints %d: graph_solve %.2f ms wall (kernel brackets %.2f ms), outer %d, inner %s (%d), last loop ended by %s,"
        " %.1f us per inner iteration (wall), 3 launches per iteration, E %.6e -> %.9e"
        % (rows, m, len(src), 1e3 * wall, dev_ms, res["outer"], res["inner"], inner, out["inner_end"], out["us_per_inner_wall"],
           res["e_before"], res["e_after"]))
    if not a.no_host:
        t = time.perf_counter()
        npos, nt0, _ = f.graph_nodes()
        w4, idx4 = f.graph_bind_points(src, ts)
        edges = f.graph_edges()
        t1 = time.perf_counter()
        Rd, td, E = gs.direct_gauss_newton(npos, edges, w4, idx4, src, dst)
        t2 = time.perf_counter()
        f.graph_apply(Rd.astype(f32), td.astype(f32))
        t3 = time.perf_counter()
        out.update(host_fetch_ms=1e3 * (t1 - t), host_solve_ms=1e3 * (t2 - t1), host_apply_ms=1e3 * (t3 - t2), host_outer=len(E) - 1,
                   energy_gap=abs(E[-1] - res["e_after"]) / E[-1])
        say("  host route: nodes + bind_points + edges %.2f ms, scipy direct Gauss-Newton %.1f ms (%d steps), graph_apply %.2f ms;"
            " E %.9e, relative gap to graph_solve %.2e" % (out["host_fetch_ms"], out["host_solve_ms"], len(E) - 1, out["host_apply_ms"],
                                                          E[-1], out["energy_gap"]))
    say(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[1000000, 100000])
    ap.add_argument("--stride", type=int, default=50)
    ap.add_argument("--look", type=int, default=20)
    ap.add_argument("--frames", type=int, default=600)
    ap.add_argument("--constraints", type=int, default=10000)
    ap.add_argument("--deg", type=float, default=3.0)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True); lines.append(s)
    lib = binding.load_product()
    for rows in a.rows:
        probe(lib, rows, a, say)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
