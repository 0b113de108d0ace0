"""Raw sensor frames (include/ssf_input.h): BGR / RGBA / BGRA colour and uint16 depth with a scale, read by the kernels that
load the pixels.  The reference run is the product on the default path (RGB8 + float metres) fed the host conversion the
reference's nodes apply (replay.convert_depth); every run on raw frames must be bit-identical to it."""
import math
import os

import numpy as np
import pytest

import util
from supersurfel_fusion_amd import binding, replay

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
SCALE = 0.0002
COLORS = ("rgb8", "bgr8", "rgba8", "bgra8")
ERR_INVALID_ARG, ERR_STATE = -1, -5


def quantised(k, W, H, scale=SCALE):
    """synthetic frame k with its depth quantised to sensor counts: (rgb, d16, the float metres the default path gets)"""
    rgb, depth = util.frame(k, W, H, noise=True, holes=0.02)
    d16 = np.clip(np.rint(np.asarray(depth, np.float64) / scale), 0, 65535).astype(np.uint16)
    return rgb, d16, replay.convert_depth(d16, scale)


def raw_color(rgb, fmt):
    """an RGB image in colour layout fmt (the alpha byte holds junk: it must be ignored)"""
    if fmt in ("bgr8", "bgra8"):
        rgb = rgb[..., ::-1]
    if fmt in ("rgba8", "bgra8"):
        alpha = (np.arange(rgb.shape[0] * rgb.shape[1]) * 37 % 251).astype(np.uint8).reshape(rgb.shape[0], rgb.shape[1], 1)
        rgb = np.concatenate([rgb, alpha], axis=2)
    return np.ascontiguousarray(rgb, np.uint8)


def raw_depth(d16, f32, fmt):
    return d16 if fmt == "u16" else f32


def fusion(lib, W, H, color="rgb8", depth="f32", scale=SCALE, **kw):
    f = binding.Fusion(lib, util.make_cfg(lib, W, H, **kw))
    if (color, depth) != ("rgb8", "f32"):
        f.set_input_format(color, depth, scale)
    return f


def to_device(a):
    """a device copy, complete before its address is handed to the library (whose streams do not wait for torch's)"""
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:                  # (same bytes; torch's uint16 tensors lack copies on some builds)
        a = a.view(np.int16)
    t = torch.from_numpy(a).cuda()
    torch.cuda.synchronize()
    return t


@pytest.mark.parametrize("prefilter", [0, 1])
@pytest.mark.parametrize("depth", ["f32", "u16"])
@pytest.mark.parametrize("color", COLORS)
def test_every_format_is_bit_identical_to_the_float_rgb_path(color, depth, prefilter, product_lib):
    W, H, n = 320, 240, 3
    fr = fusion(product_lib, W, H, depth_prefilter=prefilter)
    fx = fusion(product_lib, W, H, color, depth, depth_prefilter=prefilter)
    assert fx.input_format() == dict(color=color, depth=depth, depth_scale=SCALE if depth == "u16" else 1.0)
    for k in range(n):
        rgb, d16, f32 = quantised(k, W, H)
        util.same_result(fr.process_frame(rgb, f32), fx.process_frame(raw_color(rgb, color), raw_depth(d16, f32, depth)))
    util.compare_state(fr, fx)


@pytest.mark.parametrize("prefilter", [0, 1])
@pytest.mark.parametrize("color", ["bgr8", "bgra8"])
def test_full_size_frames(color, prefilter, product_lib):
    W, H = 640, 480
    fr = fusion(product_lib, W, H, depth_prefilter=prefilter, nb_supersurfels_max=40000)
    fx = fusion(product_lib, W, H, color, "u16", depth_prefilter=prefilter, nb_supersurfels_max=40000)
    for k in range(2):
        rgb, d16, f32 = quantised(k, W, H)
        util.same_result(fr.process_frame(rgb, f32), fx.process_frame(raw_color(rgb, color), d16))
    util.compare_state(fr, fx)


@pytest.mark.parametrize("on_device", [False, True])
@pytest.mark.parametrize("prefilter", [0, 1])
def test_pipelined_host_and_device_frames(prefilter, on_device, product_lib):
    """pipeline depth 2, 8 frames per launch, 11 frames (the last batch partial)"""
    W, H, nf = 320, 240, 11
    frames = [quantised(k, W, H) for k in range(nf)]
    fr = fusion(product_lib, W, H, depth_prefilter=prefilter)
    want = [fr.process_frame(rgb, f32) for rgb, _, f32 in frames]
    fx = fusion(product_lib, W, H, "bgra8", "u16", depth_prefilter=prefilter, pipeline_depth=2, extract_batch=8)
    inputs = [(raw_color(rgb, "bgra8"), d16) for rgb, d16, _ in frames]
    if on_device:
        inputs = [(to_device(c), to_device(d)) for c, d in inputs]
    got, nsub = [], 0
    for k in range(nf):
        while nsub < nf and fx.can_submit():
            c, d = inputs[nsub]
            if on_device:
                fx.submit_frame(c.data_ptr(), d.data_ptr(), on_device=True)
            else:
                fx.submit_frame(c, d)
            nsub += 1
        got.append(fx.process_submitted().as_dict())
    for a, b in zip(want, got):
        util.same_result(a, b)
    util.compare_state(fr, fx)


def test_one_frame_in_flight_device_frames(product_lib):
    W, H, n = 320, 240, 3
    fr, fx = fusion(product_lib, W, H, depth_prefilter=1), fusion(product_lib, W, H, "rgba8", "u16", depth_prefilter=1)
    for k in range(n):
        rgb, d16, f32 = quantised(k, W, H)
        c, d = to_device(raw_color(rgb, "rgba8")), to_device(d16)
        util.same_result(fr.process_frame(rgb, f32), fx.process_frame_device(c.data_ptr(), d.data_ptr()).as_dict())
    util.compare_state(fr, fx)


@pytest.mark.parametrize("prefilter", [0, 1])
def test_sequence_of_host_frames_through_the_upload_ring(prefilter, product_lib):
    """ssf_process_sequence with host frames: the upload ring (50 slots at depth 2 x 8 frames) wraps.  The raw handle first
    runs a sequence in the default format -- the ring is created for it -- and then one of BGRA8 + u16 frames."""
    W, H, n1, n2 = 320, 240, 12, 64
    frames = [quantised(k, W, H) for k in range(n1 + n2)]
    fr = fusion(product_lib, W, H, depth_prefilter=prefilter, pipeline_depth=2, extract_batch=8)
    fx = fusion(product_lib, W, H, depth_prefilter=prefilter, pipeline_depth=2, extract_batch=8)
    rp, dp, keep_r = fr.host_sequence([f[0] for f in frames], [f[2] for f in frames])
    want = fr.process_sequence(rp, dp, on_device=False)
    rp, dp, keep_a = fx.host_sequence([f[0] for f in frames[:n1]], [f[2] for f in frames[:n1]])
    got = fx.process_sequence(rp, dp, on_device=False)
    fx.set_input_format("bgra8", "u16", SCALE)
    rp, dp, keep_b = fx.host_sequence([raw_color(f[0], "bgra8") for f in frames[n1:]], [f[1] for f in frames[n1:]])
    got += fx.process_sequence(rp, dp, on_device=False)
    assert len(got) == n1 + n2
    for a, b in zip(want, got):
        util.same_result(a, b)
    util.compare_state(fr, fx)


def test_sequence_of_device_frames(product_lib):
    W, H, n = 320, 240, 20
    frames = [quantised(k, W, H) for k in range(n)]
    fr = fusion(product_lib, W, H, depth_prefilter=1, pipeline_depth=2, extract_batch=8)
    fx = fusion(product_lib, W, H, "bgr8", "u16", depth_prefilter=1, pipeline_depth=2, extract_batch=8)
    ref = [(to_device(rgb), to_device(f32)) for rgb, _, f32 in frames]
    raw = [(to_device(raw_color(rgb, "bgr8")), to_device(d16)) for rgb, d16, _ in frames]
    want = fr.process_sequence([c.data_ptr() for c, _ in ref], [d.data_ptr() for _, d in ref], on_device=True)
    got = fx.process_sequence([c.data_ptr() for c, _ in raw], [d.data_ptr() for _, d in raw], on_device=True)
    for a, b in zip(want, got):
        util.same_result(a, b)
    util.compare_state(fr, fx)


@pytest.mark.parametrize("prefilter", [0, 1])
def test_stage_extract(prefilter, product_lib):
    W, H = 320, 240
    rgb, d16, f32 = quantised(4, W, H)
    fr = fusion(product_lib, W, H, depth_prefilter=prefilter)
    fx = fusion(product_lib, W, H, "bgra8", "u16", depth_prefilter=prefilter)
    fr.stage_extract(rgb, f32)
    fx.stage_extract(raw_color(rgb, "bgra8"), d16)
    util.compare_state(fr, fx)
    c, d = to_device(raw_color(rgb, "bgra8")), to_device(d16)
    fx.stage_extract(c.data_ptr(), d.data_ptr(), on_device=True)
    fr.stage_extract(rgb, f32)
    util.compare_state(fr, fx)


def test_raw_frames_against_the_oracle(oracle_lib, product_lib):
    """the checker on the float RGB frames the node builds, the product on the sensor's BGR8 + u16 frames"""
    W, H, n = 320, 240, 3
    fo = fusion(oracle_lib, W, H, depth_prefilter=1)
    fx = fusion(product_lib, W, H, "bgr8", "u16", depth_prefilter=1)
    for k in range(n):
        rgb, d16, f32 = quantised(k, W, H)
        util.same_result(fo.process_frame(rgb, f32), fx.process_frame(raw_color(rgb, "bgr8"), d16))
    util.compare_state(fo, fx)


@pytest.mark.parametrize("archive,intrinsics", [("tum_fr1_xyz_8frames.npz", {}), ("tum_fr3_walking_4frames.npz", replay.FR3_INTRINSICS)])
def test_golden_frames_as_stored(archive, intrinsics, product_lib):
    """the real frames as the sensor delivered them (u16 depth, 5000 counts per metre), colour flipped to BGR8: the same
    trajectory and model as frames_from_npz's converted frames"""
    path = os.path.join(GOLD, archive)
    cfg = dict(replay.BENCHMARK_LAUNCH, nb_supersurfels_max=20000, **intrinsics)
    fr = binding.Fusion(product_lib, product_lib.default_config(**cfg))
    fx = binding.Fusion(product_lib, product_lib.default_config(**cfg))
    fx.set_input_format("bgr8", "u16", 0.0002)
    lr, rr = replay.replay(fr, replay.frames_from_npz(path))
    raw = ((s, np.ascontiguousarray(c[..., ::-1]), d) for s, c, d in replay.frames_from_npz(path, raw=True))
    lx, rx = replay.replay(fx, raw)
    assert lx == lr and len(lx) == (8 if "fr1" in archive else 4)
    for a, b in zip(rr, rx):
        util.same_result(a, b)
    util.compare_state(fr, fx)


def test_pipelined_replay_of_raw_frames(product_lib, tmp_path):
    """replay.py's raw option on a pipelined handle writes the same estimated.txt, byte for byte"""
    path = os.path.join(GOLD, "tum_fr1_xyz_8frames.npz")
    cfg = dict(replay.BENCHMARK_LAUNCH, nb_supersurfels_max=20000, pipeline_depth=2, extract_batch=4)
    fr = binding.Fusion(product_lib, product_lib.default_config(**cfg))
    fx = binding.Fusion(product_lib, product_lib.default_config(**cfg))
    fx.set_input_format("rgb8", "u16", 0.0002)
    replay.replay(fr, replay.frames_from_npz(path), str(tmp_path / "a.txt"), pipelined=True)
    replay.replay(fx, replay.frames_from_npz(path, raw=True), str(tmp_path / "b.txt"), pipelined=True)
    assert (tmp_path / "a.txt").read_bytes() == (tmp_path / "b.txt").read_bytes()


@pytest.mark.parametrize("W,H", [(320, 240), (161, 123)])
def test_bilateral_filter_on_u16(W, H, product_lib):
    rng = np.random.default_rng(7)
    d16 = rng.integers(0, 65536, size=(H, W)).astype(np.uint16)
    d16[rng.random((H, W)) < 0.2] = 0
    d16[:, :4] = 1; d16[-3:, :] = 65535
    for scale in (SCALE, 1e-6, 1.0):
        f = binding.Fusion(product_lib, util.make_cfg(product_lib, W, H))
        want = f.bilateral_filter(replay.convert_depth(d16, scale))
        f.set_input_format("rgb8", "u16", scale)
        got = f.bilateral_filter(d16)
        util.assert_same_bits(want, got, "bilateral filter, scale %g" % scale)
        d = to_device(d16)
        import torch
        out = torch.zeros((H, W), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        assert product_lib.lib.ssf_bilateral_filter(f.h, binding.C.c_void_p(d.data_ptr()), binding.C.c_void_p(out.data_ptr()), 1) == 0
        util.assert_same_bits(want, out.cpu().numpy(), "bilateral filter on device, scale %g" % scale)


@pytest.mark.parametrize("scale", [1e-6, 1.0])
@pytest.mark.parametrize("prefilter", [0, 1])
def test_hostile_values_and_odd_widths(scale, prefilter, product_lib):
    """counts 0 / 1 / 65535 next to ordinary depth, extreme scales, an image width that is no multiple of anything"""
    W, H = 161, 123
    fr = fusion(product_lib, W, H, depth_prefilter=prefilter)
    fx = fusion(product_lib, W, H, "bgra8", "u16", scale, depth_prefilter=prefilter)
    for k in range(2):
        rgb, d16, _ = quantised(k, W, H, scale=max(scale, SCALE))
        d16 = d16.copy()
        d16[::7, :] = 0; d16[:, ::11] = 1; d16[3::13, :] = 65535
        f32 = replay.convert_depth(d16, scale)
        util.same_result(fr.process_frame(rgb, f32), fx.process_frame(raw_color(rgb, "bgra8"), d16))
    util.compare_state(fr, fx)


def test_misuse(product_lib):
    W, H = 320, 240
    L = product_lib.lib
    f = fusion(product_lib, W, H, pipeline_depth=1, extract_batch=4)
    # bad scale, unknown enums
    for scale in (0.0, -1.0, math.nan, math.inf):
        assert L.ssf_set_input_format(f.h, 0, 1, scale) == ERR_INVALID_ARG
    assert L.ssf_set_input_format(f.h, 4, 0, 1.0) == ERR_INVALID_ARG
    assert L.ssf_set_input_format(f.h, -1, 0, 1.0) == ERR_INVALID_ARG
    assert L.ssf_set_input_format(f.h, 0, 2, 1.0) == ERR_INVALID_ARG
    with pytest.raises(binding.SsfError, match=r"\(-1\)"):
        f.set_input_format("bgr8", "u16", 0.0)
    with pytest.raises(binding.SsfError, match="unknown input format"):
        f.set_input_format("yuv", "u16", SCALE)
    assert f.input_format() == dict(color="rgb8", depth="f32", depth_scale=1.0)       # nothing changed
    # a change while a frame is pending
    rgb, d16, f32 = quantised(0, W, H)
    f.submit_frame(rgb, f32)
    assert f.pending_frames() == 1
    with pytest.raises(binding.SsfError, match=r"\(-5\)"):
        f.set_input_format("bgr8", "u16", SCALE)
    f.process_submitted()
    f.set_input_format("rgba8", "u16", SCALE)
    # misaligned device pointers: u16 depth at an odd address, 4-byte colour at an address that is 2 mod 4
    c, d = to_device(np.zeros(4 * W * H + 8, np.uint8)), to_device(np.zeros(W * H + 4, np.uint16))
    cp, dp = c.data_ptr(), d.data_ptr()
    assert L.ssf_submit_frame(f.h, binding.C.c_void_p(cp), binding.C.c_void_p(dp + 1), 1, None) == ERR_INVALID_ARG
    assert L.ssf_submit_frame(f.h, binding.C.c_void_p(cp + 2), binding.C.c_void_p(dp), 1, None) == ERR_INVALID_ARG
    res = binding.SsfFrameResult()
    assert L.ssf_process_frame_device(f.h, binding.C.c_void_p(cp + 1), binding.C.c_void_p(dp), None, None, binding.C.byref(res)) == ERR_INVALID_ARG
    assert L.ssf_stage_extract(f.h, binding.C.c_void_p(cp), binding.C.c_void_p(dp + 1), 1, None) == ERR_INVALID_ARG
    ptrs = (binding.C.c_void_p * 1)(cp), (binding.C.c_void_p * 1)(dp + 1)
    assert L.ssf_process_sequence(f.h, ptrs[0], ptrs[1], 1, 1, (binding.SsfFrameResult * 1)()) == ERR_INVALID_ARG
    assert L.ssf_bilateral_filter(f.h, binding.C.c_void_p(dp + 1), binding.C.c_void_p(cp), 1) == ERR_INVALID_ARG
    assert f.pending_frames() == 0
    # dtype / shape mismatches in the binding are refused, not cast
    with pytest.raises(binding.SsfError, match="depth frame must be uint16"):
        f.process_frame(raw_color(rgb, "rgba8"), f32)
    with pytest.raises(binding.SsfError, match="colour frame must be uint8 240x320x4"):
        f.process_frame(rgb, d16)
    with pytest.raises(binding.SsfError, match="depth frame must be uint16"):
        f.submit_frame(raw_color(rgb, "rgba8"), d16.astype(np.int32))
    assert f.pending_frames() == 0
    # the handle is still usable: the next frame is the one a fresh reference handle computes as its second
    fr = fusion(product_lib, W, H)
    fr.process_frame(rgb, f32)
    rgb1, d161, f321 = quantised(1, W, H)
    util.same_result(fr.process_frame(rgb1, f321), f.process_frame(raw_color(rgb1, "rgba8"), d161))


def test_ssf_hpp_raw_overloads_on_the_hip_library(product_lib, tmp_path):
    """tests/cpp/input_format_smoke.cpp: setInputFormat(BGR8, U16), processFrame through the cv::Mat CV_16UC1 overload and the
    uint16 pointer overload, processSequence with uint16 depth -- the poses of the float RGB path, bit for bit"""
    import subprocess
    from supersurfel_fusion_amd import synthetic
    from test_input_formats import build_smoke
    W, H, n = 160, 128, 4
    frames = [quantised(k, W, H) for k in range(n)]
    raw = tmp_path / "frames.bin"
    with open(raw, "wb") as f:
        for rgb, d16, _ in frames:
            f.write(raw_color(rgb, "bgr8").tobytes()); f.write(d16.tobytes())
    exe = tmp_path / "input_format_smoke"
    r = build_smoke(product_lib.path, "ssf_hip", exe)
    assert r.returncode == 0, r.stdout
    K = synthetic.intrinsics(W, H)
    r = subprocess.run([str(exe), str(W), str(H), str(n), str(raw)] + [repr(float(K[k])) for k in ("fx", "fy", "cx", "cy")] + [repr(SCALE)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout
    lines = r.stdout.strip().splitlines()
    assert lines[0] == "float_refused 1"
    fr = binding.Fusion(product_lib, product_lib.default_config(nb_supersurfels_max=50000, lambda_pos=10.0, lambda_bound=1000.0, lambda_size=1000.0,
                                                                lambda_disp=1e8, depth_prefilter=0,
                                                                **{k: K[k] for k in ("width", "height", "fx", "fy", "cx", "cy")}))
    for k, (rgb, _, f32) in enumerate(frames):
        res = fr.process_frame(rgb, f32)
        want = " ".join("%08x" % v for v in res["pose"].astype(np.float32).view(np.uint32)) + " n=%d" % res["n_model"]
        assert lines[1 + k] == "frame%d %s" % (k, want)
        assert lines[1 + n + k] == "frame%d %s" % (100 + k, want)
