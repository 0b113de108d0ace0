"""numpy restatement of include/ssf_graph.h: the deformation graph's nodes (sample) and the per-row binding (bind), every step one
f32 operation in the header's order, so the GPU results are compared with it bit for bit."""
import numpy as np

f32 = np.float32
u32 = np.uint32
u64 = np.uint64


def eligible(positions, confidences, min_conf=0.0):
    """rows that may become nodes: conf > min_conf (strict) and a finite position"""
    pos = np.asarray(positions, f32).reshape(-1, 3)
    return (np.asarray(confidences, f32) > f32(min_conf)) & np.isfinite(pos).all(axis=1)


def sample(positions, t_init, confidences, stride=50, min_conf=0.0):
    """the logical rows that are nodes, in node order: every stride-th eligible row of the order (t_init, logical index)"""
    t0 = np.asarray(t_init, np.int32)
    rows = np.flatnonzero(eligible(positions, confidences, min_conf))
    order = rows[np.lexsort((rows, t0[rows]))]
    return order[::int(stride)].astype(np.int32)


def nodes_of(model, stride=50, min_conf=0.0):
    """(positions m x 3, t_init m, rows m) of a model dict as Fusion.get_model returns it"""
    pos = np.ascontiguousarray(model["positions"], f32).reshape(-1, 3)
    t0 = np.ascontiguousarray(model["stamps"], np.int32).reshape(-1, 2)[:, 0]
    rows = sample(pos, t0, model["confidences"], stride, min_conf)
    return pos[rows].copy(), t0[rows].copy(), rows


def bind(points, t_init, node_pos, node_t, look=20, chunk=65536):
    """steps 1-6 for every point: (weights4 n x 4 f32, idx4 n x 4 i32, fallback n bool, lo n, W)"""
    pos = np.ascontiguousarray(points, f32).reshape(-1, 3)
    t0 = np.asarray(t_init, np.int32).ravel()
    npos = np.ascontiguousarray(node_pos, f32).reshape(-1, 3)
    nt0 = np.asarray(node_t, np.int32).ravel()
    n, m, L = len(pos), len(npos), int(look)
    assert m >= 5 and L >= 3 and len(t0) == n and len(nt0) == m
    W = min(m, 2 * L)
    w4, idx4 = np.empty((n, 4), f32), np.empty((n, 4), np.int32)
    bad_all, lo_all = np.empty(n, bool), np.empty(n, np.int64)
    for a in range(0, n, chunk):
        p, t = pos[a:a + chunk], t0[a:a + chunk]
        c = np.searchsorted(nt0, t, side="left")
        lo = np.clip(c - L, 0, max(0, m - 2 * L))
        k = lo[:, None] + np.arange(W)[None, :]
        with np.errstate(all="ignore"):
            d = p[:, None, :] - npos[k]
            d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        assert d2.dtype == f32
        key = (d2.view(u32).astype(u64) << u64(32)) | k.astype(u64)
        key = np.sort(key, axis=1)[:, :5]
        idx = (key & u64(0xFFFFFFFF)).astype(np.int32)
        with np.errstate(all="ignore"):
            dist = np.sqrt((key >> u64(32)).astype(u32).view(f32))
            dmax = dist[:, 4:5]
            r = f32(1) - dist[:, :4] / dmax
            w = r * r
            s = ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]
            wn = w / s[:, None]
        assert wn.dtype == f32
        fin = np.isfinite(p).all(axis=1)
        bad = ~((dmax[:, 0] != 0) & (s > 0) & fin)          # (dmax NaN: s is NaN, not > 0)
        wn[bad] = f32(0.25)
        i4 = idx[:, :4].copy()
        i4[~fin] = (lo[~fin, None] + np.arange(4)[None, :]).astype(np.int32)
        w4[a:a + chunk], idx4[a:a + chunk], bad_all[a:a + chunk], lo_all[a:a + chunk] = wn, i4, bad, lo
    return w4, idx4, bad_all, lo_all, W


def bind_model(model, stride=50, look=20, min_conf=0.0):
    """nodes and binding of a model dict: ((node positions, t_init, rows), (weights4, idx4))"""
    npos, nt0, rows = nodes_of(model, stride, min_conf)
    pos = np.ascontiguousarray(model["positions"], f32).reshape(-1, 3)
    t0 = np.ascontiguousarray(model["stamps"], np.int32).reshape(-1, 2)[:, 0]
    w4, idx4 = bind(pos, t0, npos, nt0, look)[:2]
    return (npos, nt0, rows), (w4, idx4)
