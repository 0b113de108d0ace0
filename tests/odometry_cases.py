"""The inputs of the odometry edge tests, built once and shared: tests/test_odometry.py asserts on the restatement (tests/odometry_ref.py)
that each of them exercises what it is meant to, tests/test_odometry_edges_gpu.py runs the very same arrays through the device.  Nothing
here touches a GPU."""
import functools

import numpy as np

import odometry_ref as orf
import util
from supersurfel_fusion_amd import synthetic

f32 = np.float32
HOLES = 0.25
MAX_BLOCKS, BLOCK = 1024, 256                       # ODO_MAX_BLOCKS workgroups of 256 threads (csrc/ssf_odometry.hip)
BIG = (644, 410)                                    # 264 040 pixels = 1032 workgroups, six levels, four reductions from an odd size
BIG_SIZES = [(644, 410), (322, 205), (161, 102), (80, 51), (40, 25), (20, 12)]
THREE_TRIPS = (1024, 513)                           # 525 312 pixels: every workgroup walks twice, the first 4 three times
ODD = [(102, 62, [(102, 62), (51, 31), (25, 15)]), (202, 126, [(202, 126), (101, 63), (50, 31), (25, 15)])]
NARROW = (f32(0.6), f32(2.5))
U16_SCALE = 0.0002
EXACT_K = (64.0, 64.0, 31.5, 23.5)


def K4(W, H):
    K = synthetic.intrinsics(W, H)
    return tuple(f32(K[k]) for k in ("fx", "fy", "cx", "cy"))


@functools.lru_cache(maxsize=None)
def frame(k, W, H):
    rgb, depth = util.frame(k, W, H, noise=True, holes=HOLES)
    rgb.setflags(write=False)
    depth.setflags(write=False)
    return rgb, depth


@functools.lru_cache(maxsize=None)
def pyramid(k, W, H, rng=orf.RANGE):
    rgb, depth = frame(k, W, H)
    return orf.pyramid(rgb, depth, K4(W, H), rng=rng)


def pose12(R, t):
    return synthetic.pose12(R, t)


def true_rel12(k):
    R, t = orf.true_rel(synthetic.orbit_pose(k), synthetic.orbit_pose(k + 1))
    return pose12(R, t)


def transforms():
    """reference camera -> current camera: the identity, a small motion, most pixels out of the image, none left (everything
    beyond range_max), the nearer part of the scene behind the camera (1.5 m backwards)"""
    return [("identity", orf.IDENTITY12), ("small", pose12(synthetic.rot_y(0.01) @ synthetic.rot_x(-0.004), [0.01, -0.003, -0.005])),
            ("mostly out", pose12(synthetic.rot_y(0.75), [0.0, 0.0, 0.0])), ("none left", pose12(np.eye(3), [0.0, 0.0, 10.0])),
            ("behind", pose12(synthetic.rot_y(0.05), [0.0, 0.0, -1.5]))]


def transform(name):
    return dict(transforms())[name]


# ---- 1. the strided launch ------------------------------------------------------------------------------------------------------
def trip_masks(W, H):
    """(head, tail): head masks the first MAX_BLOCKS * BLOCK pixels in row-major order -- what is left is reached by a thread of
    k_odo_linearise only on its second trip -- and tail masks the rest"""
    head = np.zeros(W * H, np.uint8)
    head[:MAX_BLOCKS * BLOCK] = 1
    return head.reshape(H, W), (1 - head).reshape(H, W)


def three_trip_transforms():
    """THREE_TRIPS' third trip is the image's last row, which the border gate takes out unless the warp moves it up: "up" does"""
    return [("small", transform("small")), ("up", pose12(synthetic.rot_x(0.006), [0.0, -0.004, 0.0]))]


@functools.lru_cache(maxsize=None)
def masked_pyramid(which):
    W, H = BIG
    rgb, depth = frame(0, W, H)
    return orf.pyramid(rgb, depth, K4(W, H), mask=trip_masks(W, H)[which])


# ---- 2. the dropped column ------------------------------------------------------------------------------------------------------
DROPPED = [(101, 63), (102, 62), (202, 126)]          # level 0 is odd itself | level 1 is the first odd one (51 and 101 wide)


def first_odd_level(W):
    """(l, x0): the first level with an odd width, and the first level-0 column that only feeds its last column -- the one the
    reduction to level l + 1 drops"""
    l, w = 0, W
    while w % 2 == 0:
        l, w = l + 1, w // 2
    return l, (w - 1) << l


def dropped_column_changed(rgb, depth):
    """(rgb, depth, l): the frame with other level-0 columns behind the dropped column of level l: every colour byte inverted,
    every depth there a valid 1.25 m"""
    l, x0 = first_odd_level(rgb.shape[1])
    rgb, depth = rgb.copy(), depth.copy()
    rgb[:, x0:] = 255 - rgb[:, x0:]
    depth[:, x0:] = f32(1.25)
    return rgb, depth, l


# ---- 3. the input formats -------------------------------------------------------------------------------------------------------
def u16_counts(depth, scale=U16_SCALE, rng=orf.RANGE):
    """the depth as uint16 counts, with planted counts in the first row: 0, 65535, and the two counts around each end of the range"""
    counts = np.clip(np.rint(depth.astype(np.float64) / scale), 0, 65535).astype(np.uint16)
    lo, hi = int(np.floor(float(rng[0]) / scale)), int(np.floor(float(rng[1]) / scale))
    planted = [0, 65535, lo - 1, lo, lo + 1, lo + 2, hi - 1, hi, hi + 1, hi + 2]
    counts[0, :len(planted)] = planted
    return counts, planted


def colour_as(rgb, fmt, seed=11):
    """an RGB8 image in another channel order; a four-channel format gets random alpha bytes"""
    c = rgb if fmt.startswith("rgb") else rgb[..., ::-1]
    if fmt.endswith("a8"):
        alpha = np.random.default_rng(seed).integers(0, 256, rgb.shape[:2] + (1,)).astype(np.uint8)
        c = np.concatenate([c, alpha], -1)
    return np.ascontiguousarray(c)


# ---- 4. depth validation ---------------------------------------------------------------------------------------------------------
def planted_depth_frame(rng=orf.RANGE):
    """(rgb, depth, blocks) at 64 x 48: a rendered frame with 2 x 2 blocks of chosen depths at even (x, y); blocks = [((x, y), the
    four values a b / c d, what the header promises for the block's pixel of level 1)]"""
    W, H = 64, 48
    rgb, depth = (a.copy() for a in frame(0, W, H))
    lo, hi = rng
    below, above = np.nextafter(lo, f32(0)), np.nextafter(hi, f32(np.inf))
    tiny = f32(1e-42)                                                   # a denormal
    nan, inf = f32(np.nan), f32(np.inf)
    blocks = [((4, 4), [below, above, nan, inf], f32(0)),               # nothing valid
              ((10, 4), [-inf, f32(-1), f32(-0.0), tiny], f32(0)),
              ((16, 4), [f32(0), f32(0), nan, f32(-0.0)], f32(0)),
              ((4, 10), [f32(0), nan, hi, f32(-1)], hi),                # exactly one valid
              ((10, 10), [below, f32(0), tiny, lo], lo),
              ((16, 10), [above, inf, -inf, hi], hi),
              ((22, 10), [lo, below, above, nan], lo),
              ((4, 16), [lo, f32(1.5), f32(2.0), hi], lo),              # range_min next to larger depths
              ((10, 16), [f32(1.5), lo, nan, f32(3.0)], lo),
              ((62, 46), [hi, above, inf, f32(-0.0)], hi)]              # the image's last block
    for (x, y), vals, _ in blocks:
        depth[y:y + 2, x:x + 2] = np.array(vals, f32).reshape(2, 2)
    return rgb, depth, blocks


# ---- 5. the warp's border ----------------------------------------------------------------------------------------------------------
def exact_frame(W=64, H=48, seed=0):
    """a frame whose warp at the identity is exact: power-of-two focal length and depths, half-integer principal point"""
    rng = np.random.default_rng(seed)
    rgb = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
    depth = rng.choice(np.array([0, 0.5, 1, 2, 4], f32), (H, W)).astype(f32)
    return rgb, depth, (64.0, 64.0, W / 2 - 0.5, H / 2 - 0.5)


BORDER_SHIFTS = [(-1, 0), (0, 0), (1, 0), (62, 0), (0, -1), (0, 46)]


def border_frame():
    """exact_frame with every depth 1: a translation of k / 64 along x or y moves every u or v by exactly k pixels"""
    rgb, depth, K = exact_frame()
    assert K == EXACT_K
    return rgb, np.ones_like(depth), K


def shift12(kx, ky):
    return pose12(np.eye(3), [kx / 64.0, ky / 64.0, 0.0])


def border_count(kx, ky, W=64, H=48):
    """reference pixels whose target (x + kx, y + ky) lies in [0, W - 2] x [0, H - 2]"""
    nx = sum(1 for x in range(W) if 0 <= x + kx <= W - 2)
    ny = sum(1 for y in range(H) if 0 <= y + ky <= H - 2)
    return nx * ny


# ---- 6. parameter edges ---------------------------------------------------------------------------------------------------------
EDGE_SHAPE = (102, 62)
PARAM_EDGES = [("huber=0", dict(huber=0.0)), ("r_max=0", dict(r_max=0.0)), ("tol=0", dict(tol_rot=0.0, tol_trans=0.0)),
               ("iters 2 0 3", dict(iters=[2, 0, 3])), ("iters 0 0 3", dict(iters=[0, 0, 3])), ("max_rotation=0", dict(max_rotation=0.0)),
               ("min_pixel_share tiny", dict(min_pixel_share=1e-9)), ("huber above r_max", dict(huber=1.0, r_max=0.05))]


def few_pixel_mask(n):
    """a ref_mask for EDGE_SHAPE's frame 0 that leaves n valid reference pixels, spread over the textured ones of the image's middle"""
    W, H = EDGE_SHAPE
    lv = pyramid(0, W, H)[0]
    ok = (lv["D"] != 0) & (np.abs(lv["gx"]) + np.abs(lv["gy"]) > f32(0.02))
    ys, xs = np.nonzero(ok[10:H - 10, 10:W - 10])
    pick = np.linspace(0, len(ys) - 1, n + 2).astype(int)[1:-1]
    mask = np.ones((H, W), np.uint8)
    mask[ys[pick] + 10, xs[pick] + 10] = 0
    return mask


def checkerboard():
    """(rgb, its negative, depth) at EDGE_SHAPE: 2 x 2-pixel blocks of 0 / 255, the steepest gradient everywhere, every depth range_min"""
    W, H = EDGE_SHAPE
    yy, xx = np.mgrid[0:H, 0:W]
    chk = (((xx // 2) + (yy // 2)) % 2).astype(np.uint8) * 255
    rgb = np.ascontiguousarray(np.repeat(chk[..., None], 3, -1))
    return rgb, 255 - rgb, np.full((H, W), orf.RANGE[0], f32)
