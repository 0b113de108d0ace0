"""The sort key of the tile-sorted copy (csrc/ssf_tile_rows.inc, bin_of) restated in numpy float32, one IEEE operation at a time in
the source's order, and the cases tests/test_tile_rows.py (CPU) and tests/test_tile_rows_gpu.py (GPU) run it on.  Not a test module.

A case is (model, T12, aim): a model for Fusion.set_model whose rows are ALL visible rows, the transform the rows are sorted under
(R row-major, then t: ps = R pos + t) and the occupancy of the bins its builder aims at.  What a row's bin IS comes from bin_of
below; the CPU test checks that the aim was met."""
import numpy as np

from supersurfel_fusion_amd import synthetic

TILE = 32                                    # BIN_TILE
MAX_BINS = 4096                              # BIN_MAX_BINS: a frame of more bins never makes the copy
ROWS_PER_WG = 4096                           # BIN_ROWS_PER_WG

# the sizes of the GPU test on the small camera: around one workgroup's rows, every residue of the chunk order that has a branch of
# its own (nwg & 7), empty and full segments of the scan (nwg < 8, = 8, 9, 16, 17)
SMALL = (160, 128)
SMALL_SIZES = (1, 63, 1024, 4095, 4096, 4097, 8191, 7 * 4096 + 5, 8 * 4096, 8 * 4096 + 1, 9 * 4096, 15 * 4096 + 100, 16 * 4096, 17 * 4096 + 3)
# partial tiles | two bins | a second, partial turn of the scatter's carry loop | exactly 4096 bins, four full turns
OTHER_SHAPES = ((97, 61), (32, 32), (1056, 1024), (2080, 2016))
OTHER_SIZES = (4097, 9 * 4096 + 1)
TOO_FINE = (2048, 2048)                      # 4097 bins

F = np.float32


def geometry(W, H):
    """(tiles per row, tiles per column, bins): the real tiles and one more bin for rows that project nowhere"""
    nbx, nby = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    return nbx, nby, nbx * nby + 1


def camera(W, H):
    """the test configuration's camera (util.make_cfg: synthetic.intrinsics) as the handle holds it: float32"""
    K = synthetic.intrinsics(W, H)
    return dict(W=W, H=H, fx=F(K["fx"]), fy=F(K["fy"]), cx=F(K["cx"]), cy=F(K["cy"]))


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def dot3(a, b):
    """ssf_math.hpp: (a.x * b.x + a.y * b.y) + a.z * b.z; a: three float32 scalars, b: (n, 3) float32"""
    return (a[0] * b[:, 0] + a[1] * b[:, 1]) + a[2] * b[:, 2]


def transform(T12, pos):
    """add(m3_mulv(R, pos), t) -> (n, 3) float32"""
    T = np.asarray(T12, F).reshape(12)
    pos = np.asarray(pos, F).reshape(-1, 3)
    with np.errstate(all="ignore"):
        return np.stack([dot3(T[0:3], pos) + T[9], dot3(T[3:6], pos) + T[10], dot3(T[6:9], pos) + T[11]], axis=1)


def pixel_round(v):
    """ssf_math.hpp pixel_round: round half away from zero for |v| < 2^23, -1 otherwise (NaN included) -> int32"""
    v = np.asarray(v, F)
    with np.errstate(all="ignore"):
        ok = np.abs(v) < F(8388608.0)
        t = np.trunc(v)
        t = np.where(np.abs(v - t) >= F(0.5), t + np.where(v < F(0.0), F(-1.0), F(1.0)), t).astype(F)
        return np.where(ok, np.where(ok, t, F(0.0)).astype(np.int32), np.int32(-1)).astype(np.int32)


def project(cam, ps):
    """ps.x * fx / ps.z + cx, ps.y * fy / ps.z + cy, as float32 before pixel_round"""
    with np.errstate(all="ignore"):
        return ps[:, 0] * cam["fx"] / ps[:, 2] + cam["cx"], ps[:, 1] * cam["fy"] / ps[:, 2] + cam["cy"]


def bin_of(cam, T12, pos):
    """the bin of every row -> int64 array"""
    nbx, _, nbins = geometry(cam["W"], cam["H"])
    ps = transform(T12, pos)
    uf, vf = project(cam, ps)
    u, v = pixel_round(uf).astype(np.int64), pixel_round(vf).astype(np.int64)
    with np.errstate(all="ignore"):
        inside = (ps[:, 2] > F(0.0)) & (u >= 0) & (u < cam["W"]) & (v >= 0) & (v < cam["H"])
    return np.where(inside, (np.maximum(v, 0) // TILE) * nbx + np.maximum(u, 0) // TILE, nbins - 1)


def half_fraction(cam, T12, pos):
    """the restated v - trunc(v) of both projections, float32 (n, 2): +-0.5 exactly is where pixel_round's tie rule decides"""
    uf, vf = project(cam, transform(T12, pos))
    with np.errstate(all="ignore"):
        return np.stack([uf - np.trunc(uf), vf - np.trunc(vf)], axis=1), np.stack([uf, vf], axis=1)


def bin_of_f64(cam, T12, pos):
    """the same formula in float64 (an independent evaluation, for the CPU test's sanity check) -> (bins, margin): margin = how far, in
    pixels, the nearer projection is from a rounding boundary k + 0.5 (inf where the row is behind the camera by more than 1 mm)"""
    nbx, _, nbins = geometry(cam["W"], cam["H"])
    T = np.asarray(T12, F).astype(np.float64)
    ps = np.asarray(pos, F).astype(np.float64) @ T[:9].reshape(3, 3).T + T[9:]
    with np.errstate(all="ignore"):
        u = ps[:, 0] * float(cam["fx"]) / ps[:, 2] + float(cam["cx"])
        v = ps[:, 1] * float(cam["fy"]) / ps[:, 2] + float(cam["cy"])
        ru, rv = np.sign(u) * np.floor(np.abs(u) + 0.5), np.sign(v) * np.floor(np.abs(v) + 0.5)
        inside = (ps[:, 2] > 0) & (ru >= 0) & (ru < cam["W"]) & (rv >= 0) & (rv < cam["H"])
        b = np.where(inside, (np.where(inside, rv, 0) // TILE) * nbx + np.where(inside, ru, 0) // TILE, nbins - 1).astype(np.int64)
        margin = np.minimum(np.abs(u - (np.floor(u) + 0.5)), np.abs(v - (np.floor(v) + 0.5)))
        margin = np.where(ps[:, 2] < -1e-3, np.inf, np.where(ps[:, 2] > 1e-3, margin, 0.0))
    return b, np.nan_to_num(margin, nan=0.0)


# ---- transforms -----------------------------------------------------------------------------------------------------------------
def transform_named(name):
    if name == "identity":
        return np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], F)
    if name == "nan":                        # a NaN in R: u = pixel_round(NaN) = -1 for every row, the last bin
        T = transform_named("oblique")
        T[0] = np.nan
        return T
    assert name == "oblique"                 # 20 degrees about (1, 2, 3) / |.| with a translation: no element of R is 0 or 1
    k = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    a = np.deg2rad(20.0)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)
    return np.concatenate([R.reshape(9), [0.1, -0.05, 0.2]]).astype(F)


TRANSFORMS = ("identity", "oblique", "nan")


def to_model_frame(T12, ps):
    """positions whose transform under T12 is (close to) the camera-space points ps: R^T (ps - t) in float64, rounded to float32.
    Under the identity the points themselves, bit for bit."""
    T = np.asarray(T12, F)
    if np.array_equal(T, transform_named("identity")):
        return np.asarray(ps, F)
    T = np.nan_to_num(T.astype(np.float64), nan=1.0)
    with np.errstate(all="ignore"):
        return ((np.asarray(ps, np.float64) - T[9:]) @ T[:9].reshape(3, 3)).astype(F)


# ---- cases ----------------------------------------------------------------------------------------------------------------------
def model_of(pos, seed):
    """a model whose rows all differ in every field the copy carries (position, confidence, colour, normal)"""
    pos = np.asarray(pos, F).reshape(-1, 3)
    n = len(pos)
    rng = np.random.default_rng(seed)
    ori = rng.standard_normal((n, 3, 3))
    ori /= np.linalg.norm(ori, axis=2, keepdims=True)
    return dict(positions=pos, colors=rng.uniform(0, 255, (n, 3)).astype(F), stamps=np.tile(np.array([[0, 29]], np.int32), (n, 1)),
                orientations=ori.reshape(n, 9).astype(F), shapes=rng.uniform(1e-4, 1e-3, (n, 6)).astype(F),
                dims=rng.uniform(1e-4, 1e-3, (n, 2)).astype(F), confidences=rng.uniform(1.0, 5000.0, n).astype(F))


def back_project(cam, u, v, z):
    """camera-space points (float64) that project to the pixel coordinates (u, v) at depth z"""
    return np.stack([(u - float(cam["cx"])) * z / float(cam["fx"]), (v - float(cam["cy"])) * z / float(cam["fy"]), z], axis=1)


def pixels_in_bins(cam, bins, rng):
    """pixel coordinates uniform over the tiles named by `bins` (real bins), a quarter pixel inside the tile's rounding cell edges"""
    nbx = geometry(cam["W"], cam["H"])[0]
    bins = np.asarray(bins, np.int64)
    x0, y0 = (bins % nbx) * TILE, (bins // nbx) * TILE
    x1, y1 = np.minimum(x0 + TILE - 1, cam["W"] - 1), np.minimum(y0 + TILE - 1, cam["H"] - 1)
    return rng.uniform(x0 - 0.25, x1 + 0.25), rng.uniform(y0 - 0.25, y1 + 0.25)


def rows_in_bins(cam, T12, bins, rng):
    u, v = pixels_in_bins(cam, bins, rng)
    return to_model_frame(T12, back_project(cam, u, v, rng.uniform(0.5, 4.0, len(u))))


def uniform(cam, T12, n, rng):
    """pixels uniform over the image at depths 0.5 to 4 m: the rows deal themselves over the real tiles in a seeded order (so that
    n rows populate min(n, tiles) of them, and consecutive rows lie in unrelated tiles, as rows in arrival order do); every tenth
    row is outside the image or behind the camera, in turn"""
    nreal = geometry(cam["W"], cam["H"])[2] - 1
    i = np.arange(n)
    out = i % 10 == 9
    order = rng.permutation(nreal)
    k = np.cumsum(~out) - 1
    u, v = pixels_in_bins(cam, order[np.maximum(k, 0) % nreal], rng)
    z = rng.uniform(0.5, 4.0, n)
    beside = out & (i % 20 == 9)
    behind = out & (i % 20 == 19)
    u = np.where(beside, u + cam["W"] + 3.0, u)
    z = np.where(behind, -z, z)
    return to_model_frame(T12, back_project(cam, u, v, z))


def uniform_outside(n):
    """how many of uniform's n rows are outside the image or behind the camera"""
    return n // 10


def one_bin(cam, T12, n, rng, which):
    nreal = geometry(cam["W"], cam["H"])[2] - 1
    b = nreal // 2 if which == "middle" else nreal - 1
    return rows_in_bins(cam, T12, np.full(n, b), rng), b


def nowhere(cam, T12, n, rng):
    """every row behind the camera"""
    u, v = rng.uniform(0, cam["W"] - 1, n), rng.uniform(0, cam["H"] - 1, n)
    return to_model_frame(T12, back_project(cam, u, v, -rng.uniform(0.5, 4.0, n)))


def even_bins(cam, T12, n, rng):
    """only every second real bin populated (0, 2, 4, ..), none in the last bin"""
    nreal = geometry(cam["W"], cam["H"])[2] - 1
    even = np.arange(0, nreal, 2)
    return rows_in_bins(cam, T12, even[rng.permutation(n) % len(even)], rng)


def two_far_bins(cam, T12, n, rng):
    """rows alternate between bin 0 and the last real bin"""
    nreal = geometry(cam["W"], cam["H"])[2] - 1
    return rows_in_bins(cam, T12, np.where(np.arange(n) % 2 == 0, 0, nreal - 1), rng)


DEPTHS = tuple(F(z) for z in (1.0, 2.0, 0.5, 1.5, 3.0, 0.75, 1.25))


def solve_at(p, f, c, z):
    """x float32 for which the restated x * f / z + c is EXACTLY the float32 p (the nearest such to the float64 solution), or None"""
    p, f, c, z = F(p), F(f), F(c), F(z)
    x0 = F((float(p) - float(c)) * float(z) / float(f))
    up, down = [x0], []
    for _ in range(64):
        up.append(np.nextafter(up[-1], F(np.inf)))
        down.append(np.nextafter((down or [x0])[-1], F(-np.inf)))
    cand = np.array(down[::-1] + up, F)
    with np.errstate(all="ignore"):
        hit = np.flatnonzero(cand * f / z + c == p)
    return cand[hit[np.argmin(np.abs(hit - 64))]] if hit.size else None


def solve_exact(p, f, c):
    """(x, z) with solve_at's property at the first of DEPTHS that has one, or None"""
    for z in DEPTHS:
        x = solve_at(p, f, c, z)
        if x is not None:
            return x, z
    return None


def half_targets(size):
    """the projections a half away from an integer that the edges family aims at, along an image side of `size` pixels: both sides
    of 0, the first tile border, the image border from inside and from outside"""
    return (-0.5, 0.5, TILE - 0.5, size - 1.5, size - 0.5)


def edge_rows(cam):
    """camera-space rows (float32, exact under the identity) at the boundaries of bin_of's rule"""
    W, H = cam["W"], cam["H"]
    rows = []
    mid_u, mid_v = float(min(W - 1, 16)), float(min(H - 1, 16))

    def at(pu, pv):
        """a row whose restated projections are exactly (pu, pv), at the first depth that allows both"""
        for z in DEPTHS:
            x, y = solve_at(pu, cam["fx"], cam["cx"], z), solve_at(pv, cam["fy"], cam["cy"], z)
            if x is not None and y is not None:
                rows.append((x, y, z))
                return

    # projections exactly a half away from an integer, in u and in v, and both at once
    for p in half_targets(W):
        at(p, mid_v)
    for p in half_targets(H):
        at(mid_u, p)
    for pu in half_targets(W):
        for pv in half_targets(H):
            at(pu, pv)
    # rows exactly on tile borders and on their neighbours: integer projections at the first and last pixel of tiles and of the image
    for p in (0.0, TILE - 1.0, float(TILE), W - 1.0, float(W)):
        at(p, mid_v)
    for p in (0.0, TILE - 1.0, float(TILE), H - 1.0, float(H)):
        at(mid_u, p)
    # the float32 neighbours of the halves (not ties: they go the other way)
    for base, size, along_u in ((TILE - 0.5, W, True), (-0.5, W, True), (W - 0.5, W, True), (TILE - 0.5, H, False), (-0.5, H, False), (H - 0.5, H, False)):
        for toward in (-np.inf, np.inf):
            p = np.nextafter(F(base), F(toward))
            at(p, mid_v) if along_u else at(mid_u, p)
    x, y = F(0.05), F(-0.03)
    tiny = np.array([1], np.uint32).view(F)[0]                       # the smallest denormal
    den = np.array([0x00400000], np.uint32).view(F)[0]               # a denormal with one mantissa bit
    # ps.z of 0, -0, denormals: beside the axis (the quotient overflows) and on it (0 / denormal = 0: the row IS in the image)
    for z in (F(0.0), F(-0.0), tiny, den, -tiny):
        rows += [(x, y, z), (F(0.0), F(0.0), z), (F(-0.0), F(0.0), z)]
    # NaN and +-inf in each position component
    for bad in (F(np.nan), F(np.inf), F(-np.inf)):
        rows += [(bad, y, F(1.0)), (x, bad, F(1.0)), (x, y, bad)]
    # projections beyond 2^23 in magnitude (pixel_round's -1), just below it (a pixel far outside), beyond int32
    for big in (F(1.0e7), F(-1.0e7), F(3.0e9), F(-3.0e9), F(3.0e38)):
        rows += [(big, y, F(1.0)), (x, big, F(1.0))]
    near = solve_exact(8388607.0, cam["fx"], cam["cx"])
    if near is not None:
        rows += [(near[0], y * near[1], near[1]), (-near[0], y * near[1], near[1])]
    return np.array(rows, F).reshape(-1, 3)


def edges(cam, T12, n, rng):
    """the boundary rows first; past them, in turn, a boundary row again and a row somewhere in the image"""
    special = edge_rows(cam)
    i = np.arange(n)
    ps = special[i % len(special)].astype(np.float64)
    fill = uniform(cam, transform_named("identity"), n, rng).astype(np.float64)
    return to_model_frame(T12, np.where(((i >= len(special)) & (i % 2 == 1))[:, None], fill, ps))


# family -> the transforms it runs under
FAMILIES = {"uniform": TRANSFORMS, "one_bin_middle": ("oblique",), "one_bin_last": ("identity",), "nowhere": ("identity", "oblique"),
            "even_bins": ("oblique",), "two_far_bins": ("identity",), "edges": ("identity", "oblique")}


def case(family, transform_name, W, H, n):
    """(model, T12, aim): aim describes the occupancy the builder aims at (the CPU test checks it against bin_of)"""
    cam = camera(W, H)
    T12 = transform_named(transform_name)
    seed = [sorted(FAMILIES).index(family), TRANSFORMS.index(transform_name), W, H, n]
    rng = np.random.default_rng(seed)
    nbins = geometry(W, H)[2]
    place = transform_named("oblique") if transform_name == "nan" else T12     # (under the NaN transform the rows are placed for the oblique one)
    if family == "uniform":
        pos, aim = uniform(cam, place, n, rng), dict(kind="uniform", outside=uniform_outside(n))
    elif family in ("one_bin_middle", "one_bin_last"):
        pos, b = one_bin(cam, place, n, rng, family[8:])
        aim = dict(kind="bins", bins=[b])
    elif family == "nowhere":
        pos, aim = nowhere(cam, place, n, rng), dict(kind="bins", bins=[nbins - 1])
    elif family == "even_bins":
        pos, aim = even_bins(cam, place, n, rng), dict(kind="bins", bins=list(range(0, nbins - 1, 2))[:n])
    elif family == "two_far_bins":
        pos, aim = two_far_bins(cam, place, n, rng), dict(kind="alternate", bins=[0, nbins - 2])
    else:
        assert family == "edges"
        pos, aim = edges(cam, place, n, rng), dict(kind="edges")
    if transform_name == "nan":
        aim = dict(kind="bins", bins=[nbins - 1])
    return model_of(pos, seed), T12, aim


def small_cases():
    return [(fam, tr, n) for n in SMALL_SIZES for fam in FAMILIES for tr in FAMILIES[fam]]


def other_cases():
    return [(fam, tr, W, H, n) for (W, H) in OTHER_SHAPES for n in OTHER_SIZES for fam in ("uniform", "edges") for tr in FAMILIES[fam]]
