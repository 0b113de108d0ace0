"""ssf_render_model (include/ssf_render.h) on the MI355X against the numpy restatement (tests/render_ref.py): all five images and
the three stats at 0 bits, on hand-built adversarial maps, maps built by processing frames, the metric's ~1 M-row map; plus
no side effects on the frame path, device outputs and the refusals."""
import os

import numpy as np
import pytest

import render_ref as rr
import util
from conftest import ROOT
from supersurfel_fusion_amd import binding, replay, synthetic

GOLD = os.path.join(ROOT, "tests", "golden")
pytestmark = pytest.mark.gpu


def handle(lib, W, H, **kw):
    return binding.Fusion(lib, util.make_cfg(lib, W, H, **kw))


def cam_of(f):
    c = f.cfg
    return dict(width=c.width, height=c.height, fx=c.fx, fy=c.fy, cx=c.cx, cy=c.cy)


def check(f, pose=None, camera=None, z_range=None, min_conf=0.0, s=3.0, visible_only=False, form="fragments", what=""):
    """render on the device and in numpy from get_model's rows; returns the device render"""
    got = f.render_model(pose=pose, camera=camera, z_range=z_range, min_conf=min_conf, splat_scale=s, visible_only=visible_only)
    cnt = f.counts()
    ref = rr.render(f.get_model(), cnt["n_visible"], f.get_pose() if pose is None else np.asarray(pose, np.float32).ravel(),
                    cam_of(f) if camera is None else camera,
                    (f.cfg.range_min, f.cfg.range_max) if z_range is None else z_range, min_conf, s, visible_only, form)
    rr.assert_same_render(got, ref, what)
    return got


def pose_about(R, t):
    return np.concatenate([np.asarray(R, np.float32).ravel(), np.asarray(t, np.float32)]).astype(np.float32)


def rot_y(deg):
    a = np.deg2rad(deg)
    return np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])


# ---- hand-built maps against brute force -----------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", [(160, 128), (97, 61)])
def test_hand_built_maps_against_brute_force(W, H, product_lib):
    f = handle(product_lib, W, H)
    K = cam_of(f)
    for seed in range(3):
        m = rr.adversarial_model(np.random.default_rng(seed), 400, W, H, K["fx"], with_huge=(seed == 2))
        f.set_model(m, 250, 5)
        for kw in (dict(), dict(min_conf=1.0), dict(visible_only=True), dict(s=1.5, z_range=(0.1, 3.0)),
                   dict(pose=pose_about(rot_y(4.0), (0.05, -0.02, -0.1))),
                   dict(camera=dict(width=W + 13, height=H - 7, fx=0.7 * K["fx"], fy=0.8 * K["fy"], cx=0.4 * W, cy=0.6 * H))):
            check(f, form="brute", what="seed %d %s" % (seed, sorted(kw)), **kw)


def test_discs_that_cover_the_image_grow_the_list(product_lib):
    """a small map first (small list), then 300 discs each covering the whole image: the list buffer grows"""
    W, H = 160, 128
    f = handle(product_lib, W, H)
    rng = np.random.default_rng(7)
    small = rr.adversarial_model(rng, 50, W, H, cam_of(f)["fx"], with_huge=False)
    f.set_model(small, 50, 1)
    a = check(f, form="brute", what="small")
    n = 300
    c = np.stack([rng.uniform(-0.05, 0.05, n), rng.uniform(-0.05, 0.05, n), rng.uniform(0.5, 3.0, n)], 1)
    big = rr.disc_rows(c, (1, 0, 0), (0, 1, 0), (25.0, 25.0), 5.0, colors=rng.uniform(0, 255, (n, 3)))
    f.set_model(big, 300, 2)
    b = check(f, form="brute", what="whole-image discs")
    assert b["stats"]["list_entries"] >= n * ((W + 15) // 16) * ((H + 15) // 16) > 4 * a["stats"]["list_entries"]
    assert b["stats"]["pixels_filled"] == W * H
    check(f, form="brute", visible_only=True, what="again")


# ---- maps built by processing frames ---------------------------------------------------------------------------------
def test_a_map_built_from_synthetic_frames(product_lib):
    """44 frames of a camera panning 1.5 degrees per frame (with the true pose as the prior): the rows of the first frames leave
    the view and live in the out-of-view store"""
    W, H = 320, 240
    f = handle(product_lib, W, H, nb_supersurfels_max=40000)
    R0, t0 = synthetic.orbit_pose(0)
    for k in range(44):
        rgb, depth, _ = synthetic.render(R0 @ rot_y(1.5 * k), t0, W, H, noise=True, rng=np.random.default_rng(1000 + k))
        f.process_frame(rgb, depth, prior_pose=pose_about(rot_y(1.5 * k), np.zeros(3)))
    cnt = f.counts()
    assert cnt["n_model"] > cnt["n_visible"] > 0, cnt
    p = f.get_pose()
    R, t = p[:9].reshape(3, 3), p[9:]
    poses = [None, pose_about(R @ rot_y(8.0), t + np.float32(0.1) * R[:, 0]), rr.IDENTITY]     # (frame 0's view: rows now out of view)
    shown_oov = 0
    for i, pose in enumerate(poses):
        for kw in (dict(), dict(visible_only=True), dict(min_conf=f.cfg.conf_thresh)):
            got = check(f, pose=pose, what="pose %d %s" % (i, sorted(kw)), **kw)
            if i == 2 and not kw:
                shown_oov = int((got["index"] >= cnt["n_visible"]).sum())
    assert shown_oov > 0, "the look back shows no out-of-view row"


def test_a_map_built_from_tum_fr1_xyz(product_lib):
    cfg = dict(replay.BENCHMARK_LAUNCH, nb_supersurfels_max=20000)
    f = binding.Fusion(product_lib, product_lib.default_config(**cfg))
    replay.replay(f, replay.frames_from_npz(os.path.join(GOLD, "tum_fr1_xyz_8frames.npz")))
    p = f.get_pose()
    R, t = p[:9].reshape(3, 3), p[9:]
    for i, pose in enumerate([None, pose_about(R @ rot_y(-10.0), t - np.float32(0.2) * R[:, 2]), pose_about(R @ rot_y(150.0), t)]):
        for kw in (dict(), dict(visible_only=True), dict(min_conf=f.cfg.conf_thresh)):
            check(f, pose=pose, what="fr1_xyz pose %d %s" % (i, sorted(kw)), **kw)


def test_the_metric_map_at_640x480(product_lib):
    """the ~1 M-row seeded map with the bench's visible split, against the fragment form"""
    W, H = 640, 480
    model, nvis = synthetic.seed_model_cam0(1000000, W, H, stamp=30)
    f = handle(product_lib, W, H, nb_supersurfels_max=1000000)
    f.set_model(model, nvis, 30)
    got = check(f, pose=rr.IDENTITY, what="seed_model 1M")
    assert got["stats"]["pixels_filled"] > W * H // 2 and got["stats"]["rows_shown"] > 1000


# ---- no side effects -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pipelined", [False, True])
def test_a_render_changes_no_later_result(pipelined, product_lib):
    W, H = 160, 128
    kw = dict(pipeline_depth=2, extract_batch=2) if pipelined else {}
    A, B = handle(product_lib, W, H, **kw), handle(product_lib, W, H, **kw)
    frames = [util.frame(k, W, H) for k in range(0, 36, 3)]
    look_back = pose_about(*synthetic.relative_pose(0))

    def render_all(f):
        f.render_model()
        f.render_model(pose=look_back, visible_only=True, outputs=("depth", "normal"))
        f.render_model(camera=dict(width=300, height=200, fx=200.0, fy=200.0, cx=150.0, cy=100.0), outputs=("index",))

    if not pipelined:
        for rgb, depth in frames:
            ra = A.process_frame(rgb, depth)
            render_all(A)
            util.same_result(ra, B.process_frame(rgb, depth))
    else:
        nsub = 0
        for k in range(len(frames)):
            for f in (A, B):
                n = nsub
                while n < len(frames) and f.can_submit():
                    f.submit_frame(*frames[n]); n += 1
            nsub = n
            assert A.pending_frames() > 0
            with pytest.raises(binding.SsfError, match=r"\(-5\)"):
                A.render_model()
            ra, rb = A.process_submitted().as_dict(), B.process_submitted().as_dict()
            util.same_result(ra, rb)
            if A.pending_frames() == 0:
                render_all(A)
        assert A.pending_frames() == 0
        render_all(A)
    util.compare_state(A, B)
    # ... and a frame after the last render still agrees
    rgb, depth = util.frame(40, W, H)
    if pipelined:
        A.submit_frame(rgb, depth); B.submit_frame(rgb, depth)
        util.same_result(A.process_submitted().as_dict(), B.process_submitted().as_dict())
    else:
        util.same_result(A.process_frame(rgb, depth), B.process_frame(rgb, depth))
    util.compare_state(A, B)


# ---- device outputs, profiling, misuse -------------------------------------------------------------------------------
def test_device_outputs_equal_the_host_outputs(product_lib):
    import torch
    W, H = 160, 128
    f = handle(product_lib, W, H)
    for k in range(0, 12, 3):
        f.process_frame(*util.frame(k, W, H))
    host = f.render_model()
    dev = {nm: torch.full((H, W) + tail, 7, dtype=getattr(torch, np.dtype(dt).name), device="cuda")
           for nm, dt, tail in binding.RENDER_OUTPUTS}
    torch.cuda.synchronize()
    st = f.render_model_device(**{nm: t.data_ptr() for nm, t in dev.items()})
    for nm, t in dev.items():
        util.assert_same_bits(t.cpu().numpy(), host[nm], "device " + nm)
    assert st == host["stats"]
    # a subset of the outputs: the others are not touched
    dev["index"].fill_(7)
    dev["depth"].fill_(0)
    torch.cuda.synchronize()
    st2 = f.render_model_device(depth=dev["depth"].data_ptr())
    assert st2 == host["stats"] and bool((dev["index"] == 7).all())
    util.assert_same_bits(dev["depth"].cpu().numpy(), host["depth"], "device depth alone")


def test_render_kernels_are_timed_under_profile(product_lib):
    W, H = 160, 128
    f = handle(product_lib, W, H, profile=1)
    f.process_frame(*util.frame(0, W, H))
    f.reset_kernel_times()
    f.render_model()
    names = f.kernel_times()
    for k in ("render_prep", "render_fill", "render_tile"):
        assert k in names and names[k][1] >= 1, (k, names)


def test_an_empty_model_renders_empty_images(product_lib):
    W, H = 97, 61
    f = handle(product_lib, W, H)
    got = f.render_model()
    assert got["stats"] == dict(fragments=0, pixels_filled=0, rows_shown=0, list_entries=0)
    assert not got["depth"].any() and (got["index"] == -1).all() and not got["rgb8"].any() and not got["color"].any()
    assert not got["normal"].any()
    assert got["depth"].shape == (H, W) and got["rgb8"].shape == (H, W, 3)


def test_the_refusals(product_lib):
    W, H = 97, 61
    f = handle(product_lib, W, H)
    f.process_frame(*util.frame(0, W, H))
    K = cam_of(f)
    bad = [dict(z_range=(0.0, 1.0)), dict(z_range=(-1.0, 1.0)), dict(z_range=(2.0, 2.0)), dict(z_range=(3.0, 1.0)),
           dict(camera=dict(K, width=4097)), dict(camera=dict(K, height=0)), dict(camera=dict(K, width=-3)),
           dict(camera=dict(K, fx=0.0)), dict(camera=dict(K, fy=float("nan"))), dict(camera=dict(K, fx=float("inf"))),
           dict(splat_scale=-1.0)]
    for kw in bad:
        with pytest.raises(binding.SsfError, match=r"\(-1\)"):
            f.render_model(**kw)
    with pytest.raises(binding.SsfError, match=r"\(-1\)"):
        f.render_model(outputs=())
    # the handle keeps working: a render and a frame after the refusals
    check(f, what="after the refusals")
    f.process_frame(*util.frame(1, W, H))
    check(f, what="after a frame")
    assert f.render_default_params()["width"] == W
    # a sharded handle is not rendered
    g = handle(product_lib, W, H, rank=0, nranks=2, shard_tile=0.25)
    with pytest.raises(binding.SsfError, match=r"\(-5\)"):
        g.render_model()


@pytest.mark.parametrize("pipelined", [False, True])
def test_replay_writes_renders(pipelined, product_lib, tmp_path):
    """replay(render_dir=...) draws the model after frames 0, 3, 6 at the tracked pose: the files hold what render_model
    returns there, and the trajectory is the one without renders"""
    path = os.path.join(GOLD, "tum_fr1_xyz_8frames.npz")
    kw = dict(pipeline_depth=2, extract_batch=2) if pipelined else {}
    cfg = dict(replay.BENCHMARK_LAUNCH, nb_supersurfels_max=20000, **kw)
    f = binding.Fusion(product_lib, product_lib.default_config(**cfg))
    g = binding.Fusion(product_lib, product_lib.default_config(**cfg))
    lines, _ = replay.replay(f, replay.frames_from_npz(path), pipelined=pipelined, render_dir=str(tmp_path), render_every=3)
    stamps = [ln.split()[0] for ln in lines]
    want = [stamps[k] for k in (0, 3, 6)]
    assert sorted(p for p in os.listdir(str(tmp_path))) == sorted([s + "_depth.npy" for s in want] + [s + "_rgb.png" for s in want])
    lines_g, _ = replay.replay(g, replay.frames_from_npz(path), pipelined=pipelined)
    assert lines == lines_g
    from PIL import Image
    got = f.render_model(outputs=("depth", "rgb8"))
    # the last render was at frame 6; f has processed frame 7 since: compare the last file against a fresh handle at frame 6
    h = binding.Fusion(product_lib, product_lib.default_config(**cfg))
    replay.replay(h, list(replay.frames_from_npz(path))[:7], pipelined=pipelined)
    ref = h.render_model(outputs=("depth", "rgb8"))
    util.assert_same_bits(np.load(str(tmp_path / (want[2] + "_depth.npy"))), ref["depth"], "depth file")
    util.assert_same_bits(np.asarray(Image.open(str(tmp_path / (want[2] + "_rgb.png")))), ref["rgb8"], "rgb file")
    assert got["depth"].shape == ref["depth"].shape
