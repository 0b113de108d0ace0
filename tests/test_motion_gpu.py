"""The geometric moving-object detector (include/ssf_motion.h) on the MI355X against the numpy restatement (tests/motion_ref.py):
mask, label, class image and the five stats at 0 bits on hand-built adversarial images (ssf_motion_segment), on maps set by hand
and built from frames (ssf_motion_mask), the frame path with the detected mask (ssf_process_frame_motion), plus no side effects,
determinism, device outputs, profiling names and the refusals."""
import functools

import numpy as np
import pytest

import motion_ref as mr
import render_ref as rr
import util
from dynamic_mask_ref import vote
from supersurfel_fusion_amd import binding

pytestmark = pytest.mark.gpu
SHAPES = [(160, 128), (97, 61)]
f32 = np.float32


def handle(lib, W, H, **kw):
    return binding.Fusion(lib, util.make_cfg(lib, W, H, **kw))


def cam_of(f):
    c = f.cfg
    return dict(width=c.width, height=c.height, fx=c.fx, fy=c.fy, cx=c.cx, cy=c.cy)


def z_range(f):
    return (f.cfg.range_min, f.cfg.range_max)


@functools.lru_cache(maxsize=None)
def cases(W, H):
    return mr.cases(W, H)


@functools.lru_cache(maxsize=None)
def reference(W, H, name):
    n, d, m, kw = [c for c in cases(W, H) if c[0] == name][0]
    return mr.segment(d, m, **dict(mr.default_params(W, H), **kw))


def to_device(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def params_of(f, **kw):
    """the rule's parameters as the library defaults them, overridden"""
    p = f.motion_default_params()
    return dict({k: p[k] for k in ("front_abs", "front_quad", "link_abs", "link_rel", "min_seeds", "unknown_per_seed")}, **kw)


def model_depth_ref(f, pose=None, min_conf=0.0, splat_scale=3.0):
    cnt = f.counts()
    return mr.model_depth(f.get_model(), cnt["n_visible"], f.get_pose() if pose is None else np.asarray(pose, f32).ravel(), cam_of(f),
                          z_range(f), min_conf, splat_scale)


# ---- ssf_motion_segment on hand-built images -----------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", SHAPES)
def test_hand_built_images_against_the_restatement(W, H, product_lib):
    f = handle(product_lib, W, H)
    assert f.motion_default_params()["min_seeds"] == mr.default_params(W, H)["min_seeds"]
    for name, d, m, kw in cases(W, H):
        got = f.motion_segment(d, m, params=kw)
        mr.assert_same(got, reference(W, H, name), name)
    # a subset of the outputs gives the same images
    name, d, m, kw = cases(W, H)[0]
    only = f.motion_segment(d, m, params=kw, outputs=("label",))
    assert sorted(only) == ["label", "stats"]
    mr.assert_same(only, reference(W, H, name), "label alone")


@pytest.mark.parametrize("W,H", mr.TILE_SHAPES)
def test_the_tile_grids_the_other_shapes_miss(W, H, product_lib):
    """one row of tiles, one column, a single tile (no merge launch), a last tile one cell wide"""
    f = handle(product_lib, W, H)
    for name, d, m, kw in mr.tile_cases(W, H):
        mr.assert_same(f.motion_segment(d, m, params=kw), mr.segment(d, m, **dict(mr.default_params(W, H), **kw)), name)


@pytest.mark.parametrize("W,H", SHAPES)
def test_uint16_depth_through_the_input_format(W, H, product_lib):
    f = handle(product_lib, W, H)
    scale = 0.0002
    f.set_input_format("rgb8", "u16", scale)
    for name, d, m, kw in cases(W, H):
        if name not in ("spirals", "random", "link_noise", "cross"):
            continue
        counts = np.clip(np.rint(d.astype(np.float64) / scale), 0, 65535).astype(np.uint16)
        ref = mr.segment(counts, m, depth_scale=scale, **dict(mr.default_params(W, H), **kw))
        mr.assert_same(f.motion_segment(counts, m, params=kw), ref, "u16 " + name)
        dev = to_device(counts)
        mask = to_device(np.full((H, W), 9, np.uint8))
        st = f.motion_mask_device(dev, mask=mask, params=kw, model_depth=to_device(m))
        assert st == ref["stats"] and np.array_equal(mask.cpu().numpy(), ref["mask"])


def test_device_outputs_equal_the_host_outputs_and_the_call_is_deterministic(product_lib):
    import torch
    W, H = 160, 128
    f = handle(product_lib, W, H)
    for name in ("random", "serpentine", "invalid_depths"):
        n, d, m, kw = [c for c in cases(W, H) if c[0] == name][0]
        host = f.motion_segment(d, m, params=kw)
        mr.assert_same(f.motion_segment(d, m, params=kw), host, "the same call again")
        dd, dm = to_device(d), to_device(m)
        out = dict(mask=torch.full((H, W), 7, dtype=torch.uint8, device="cuda"), label=torch.full((H, W), 7, dtype=torch.int32, device="cuda"),
                   cls=torch.full((H, W), 7, dtype=torch.uint8, device="cuda"))
        torch.cuda.synchronize()
        for _ in range(2):
            st = f.motion_mask_device(dd, params=kw, model_depth=dm, **out)
            got = {k: t.cpu().numpy() for k, t in out.items()}
            got["stats"] = st
            mr.assert_same(got, host, "device " + name)
        # one output alone: the others are not touched
        out["label"].fill_(7)
        torch.cuda.synchronize()
        assert f.motion_mask_device(dd, params=kw, model_depth=dm, mask=out["mask"]) == host["stats"]
        assert bool((out["label"] == 7).all())


def test_the_kernels_are_timed_under_profile(product_lib):
    W, H = 160, 128
    f = handle(product_lib, W, H, profile=1)
    f.reset_kernel_times()
    n, d, m, kw = cases(W, H)[0]
    f.motion_segment(d, m, params=kw)
    names = f.kernel_times()
    for k in ("motion_classify", "motion_label", "motion_merge", "motion_flatten", "motion_decide"):
        assert k in names and names[k][1] >= 1, (k, names)


# ---- ssf_motion_mask on maps set by hand -----------------------------------------------------------------------------------
def scene_depth(m, rng):
    """a depth frame for a rendered map m: the map's own depth, holes, a few blobs in front of it and some pixels behind it"""
    H, W = m.shape
    d = np.where(m > 0, m, f32(1.5)).astype(f32)
    d[rng.random((H, W)) < 0.03] = 0
    for _ in range(6):
        y, x = int(rng.integers(0, H - 12)), int(rng.integers(0, W - 16))
        d[y:y + 12, x:x + 16] = np.maximum(f32(0.3), d[y:y + 12, x:x + 16].min() - f32(rng.uniform(0.05, 0.6)))
    far = rng.random((H, W)) < 0.05
    d[far] += f32(0.3)
    return d


@pytest.mark.parametrize("W,H", SHAPES)
def test_motion_mask_on_maps_set_by_hand(W, H, product_lib):
    f = handle(product_lib, W, H)
    K = cam_of(f)
    rng = np.random.default_rng(3)
    # a wall of discs at z = 2 m that covers most of the view, confidences alternating 10 / 1
    gx, gy = np.meshgrid(np.linspace(-1.2, 1.2, 25), np.linspace(-0.9, 0.9, 19))
    wall = rr.disc_rows(np.stack([gx.ravel(), gy.ravel(), np.full(gx.size, 2.0)], 1), (1, 0, 0), (0, 1, 0), (0.0009, 0.0009))
    wall["confidences"][1::2] = 1.0
    maps = [(rr.adversarial_model(np.random.default_rng(1), 400, W, H, K["fx"], with_huge=False), 250), (wall, len(wall["confidences"]))]
    pose = np.array([0.9993908, 0, 0.0348995, 0, 1, 0, -0.0348995, 0, 0.9993908, 0.03, -0.02, -0.05], f32)
    for i, (model, nvis) in enumerate(maps):
        f.set_model(model, nvis, 5)
        for kw in (dict(), dict(pose=pose), dict(min_conf=1.0), dict(splat_scale=1.5, min_seeds=4)):
            m_ref = model_depth_ref(f, kw.get("pose"), kw.get("min_conf", 0.0), kw.get("splat_scale", 3.0))
            d = scene_depth(m_ref, rng)
            got = f.motion_mask(d, params=kw, model_depth=True)
            util.assert_same_bits(got["model_depth"], m_ref, "model depth against render_ref")
            rkw = dict(pose=kw.get("pose"), min_conf=kw.get("min_conf", 0.0), splat_scale=kw.get("splat_scale", 3.0))
            util.assert_same_bits(got["model_depth"], f.render_model(outputs=("depth",), **rkw)["depth"], "model depth against render_model")
            rule = {k: v for k, v in kw.items() if k == "min_seeds"}
            ref = mr.segment(d, m_ref, z_range=z_range(f), **params_of(f, **rule))
            mr.assert_same(got, ref, "map %d %s" % (i, sorted(kw)))
            if not kw:
                assert ref["stats"]["n_seed"] > 0 and (i == 1 or ref["stats"]["n_unknown"] > 0)      # (the wall may fill the view)
    # min_conf = 1 hides every second disc of the wall: more of the view is unknown
    assert (model_depth_ref(f, min_conf=1.0) == 0).sum() > (model_depth_ref(f) == 0).sum()


def test_an_empty_model_gives_an_empty_mask(product_lib):
    W, H = 97, 61
    f = handle(product_lib, W, H)
    rgb, depth = util.frame(0, W, H)
    got = f.motion_mask(depth)
    valid = (depth >= f32(f.cfg.range_min)) & (depth <= f32(f.cfg.range_max))
    assert not got["mask"].any() and got["stats"]["n_seed"] == 0 and got["stats"]["n_unknown"] == int(valid.sum())
    assert ((got["cls"] == mr.UNKNOWN) == valid).all()
    g = handle(product_lib, W, H)
    util.same_result(f.process_frame(rgb, depth, motion=True), g.process_frame(rgb, depth))
    util.compare_state(f, g)
    mask, st = f.last_motion_mask()
    assert not mask.any() and st == got["stats"]


# ---- a map built from frames, a box pasted in front of it ------------------------------------------------------------------
def test_a_box_in_front_of_a_map_built_from_frames(product_lib):
    W, H = 160, 128
    f = handle(product_lib, W, H)
    with pytest.raises(binding.SsfError, match=r"\(-5\)"):
        f.last_motion_mask()                                       # (no frame has gone through the detector yet)
    for k in range(6):
        f.process_frame(*util.frame(k, W, H), motion=True)
    for k in (6, 7, 8):
        rgb, depth, _, (y0, y1, x0, x1) = mr.box_scene(k, W, H)
        m_ref = model_depth_ref(f)                                 # the map and pose BEFORE the frame
        ref = mr.segment(depth, m_ref, z_range=z_range(f), **params_of(f))
        f.process_frame(rgb, depth, motion=True)
        mask, st = f.last_motion_mask()
        mr.assert_same(dict(mask=mask, stats=st), ref, "frame %d" % k)
        assert mask[y0:y1, x0:x1].all(), "the box is not masked"
        label = f.index_map()
        want = vote(label, mask, f.S)
        got, n = f.dynamic_superpixels()
        util.assert_same_bits(got, want, "dynamic superpixels")
        assert n == int(want.sum()) > 0
        box = np.zeros((H, W), bool)
        box[y0:y1, x0:x1] = True
        total = np.bincount(label.ravel(), minlength=f.S)[:f.S]
        inbox = np.bincount(label.ravel()[box.ravel()], minlength=f.S)[:f.S]
        half = (inbox > 0) & (2 * inbox >= total)
        assert half.sum() > 0 and (f.get_frame()["confidences"][half] == -1).all()


# ---- ssf_process_frame_motion = ssf_motion_mask + ssf_process_frame_pixmask ------------------------------------------------
@pytest.mark.parametrize("with_prior", [False, True])
def test_process_frame_motion_equals_mask_then_pixmask(with_prior, product_lib):
    import torch
    W, H = 160, 128
    A, B = handle(product_lib, W, H), handle(product_lib, W, H)
    kw = dict(min_seeds=10, front_abs=0.04)
    for k in range(8):
        rgb, depth = util.frame(k, W, H) if k < 4 else mr.box_scene(k, W, H)[:2]
        prior = None
        if with_prior and k > 0:
            prior = A.get_pose().copy()
            prior[9] += f32(0.002)
        ra = A.process_frame(rgb, depth, prior_pose=prior, motion=kw)
        d_rgb, d_depth = to_device(rgb), to_device(depth)
        d_mask = torch.full((H, W), 3, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        st = B.motion_mask_device(d_depth, mask=d_mask, params=dict(kw, pose=prior))
        rb = B.process_frame_device(d_rgb.data_ptr(), d_depth.data_ptr(), prior_pose=prior, pixel_mask=d_mask.data_ptr()).as_dict()
        util.same_result(ra, rb)
        mask, sa = A.last_motion_mask()
        assert sa == st and np.array_equal(mask, d_mask.cpu().numpy())
        util.assert_same_bits(A.dynamic_superpixels()[0], B.dynamic_superpixels()[0], "vote")
        if k >= 4:
            assert st["pixels_masked"] > 0
    util.compare_state(A, B)
    # the device frame form of the same call
    rgb, depth = mr.box_scene(8, W, H)[:2]
    d_rgb, d_depth = to_device(rgb), to_device(depth)
    ra = A.process_frame_device(d_rgb.data_ptr(), d_depth.data_ptr(), motion=kw).as_dict()
    util.same_result(ra, B.process_frame(rgb, depth, motion=kw))
    util.compare_state(A, B)


def test_motion_mask_calls_change_no_later_result(product_lib):
    W, H = 160, 128
    A, B = handle(product_lib, W, H), handle(product_lib, W, H)
    look = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0.1, 0.0, -0.1], f32)
    for k in range(0, 24, 3):
        rgb, depth = util.frame(k, W, H)
        a = A.motion_mask(depth)
        mr.assert_same(A.motion_mask(depth), a, "the same call again")
        A.motion_mask(depth, params=dict(pose=look, min_conf=1.0), outputs=("label",))
        A.motion_segment(depth, np.full((H, W), 2, f32))
        util.same_result(A.process_frame(rgb, depth), B.process_frame(rgb, depth))
    util.compare_state(A, B)


# ---- misuse --------------------------------------------------------------------------------------------------------------
def test_the_refusals(product_lib):
    W, H = 97, 61
    f = handle(product_lib, W, H)
    rgb, depth = util.frame(0, W, H)
    f.process_frame(rgb, depth)
    m = np.full((H, W), 2, f32)
    for kw in (dict(front_abs=-0.1), dict(front_quad=float("nan")), dict(link_abs=float("inf")), dict(link_rel=-1.0), dict(min_seeds=0),
               dict(unknown_per_seed=-1)):
        for call in (lambda: f.motion_mask(depth, params=kw), lambda: f.motion_segment(depth, m, params=kw),
                     lambda: f.process_frame(rgb, depth, motion=kw)):
            with pytest.raises(binding.SsfError, match=r"\(-1\)"):
                call()
    with pytest.raises(binding.SsfError, match=r"\(-1\)"):
        f.motion_mask(depth, outputs=())
    with pytest.raises(binding.SsfError, match=r"\(-1\)"):
        f.motion_segment(depth, m, outputs=())
    # a device depth pointer not aligned for the input format
    d_depth = to_device(np.zeros(H * W + 1, f32))
    d_mask = to_device(np.zeros((H, W), np.uint8))
    with pytest.raises(binding.SsfError, match=r"\(-1\)"):
        f.motion_mask_device(d_depth.data_ptr() + 2, mask=d_mask)
    # the handle keeps working
    ref = mr.segment(depth, model_depth_ref(f), z_range=z_range(f), **params_of(f))
    mr.assert_same(f.motion_mask(depth), ref, "after the refusals")
    # frames pending in the extract pipeline
    g = handle(product_lib, W, H, pipeline_depth=2, extract_batch=2)
    g.submit_frame(rgb, depth)
    assert g.pending_frames() > 0
    for call in (lambda: g.motion_mask(depth), lambda: g.motion_segment(depth, m), lambda: g.process_frame(rgb, depth, motion=True)):
        with pytest.raises(binding.SsfError, match=r"\(-5\)"):
            call()
    while g.pending_frames() > 0:
        g.process_submitted()
    g.motion_mask(depth)
    # a sharded handle
    s = handle(product_lib, W, H, rank=0, nranks=2, shard_tile=0.25)
    with pytest.raises(binding.SsfError, match=r"\(-5\)"):
        s.motion_mask(depth)
