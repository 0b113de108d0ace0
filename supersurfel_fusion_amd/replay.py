"""TUM RGB-D replay harness: the counterpart of the reference's benchmark node
(node/supersurfel_fusion_rgbd_benchmark_node.cpp:573-744) for the hot path.

It reproduces the node's call pattern exactly: parse `associations_with_gt.txt` (stamp rgb-path stamp
depth-path [stamp tx ty tz qx qy qz qw]), decode the PNGs, keep RGB order, convert the 16-bit depth
with `depth_scale` (0.0002 for TUM's 5000 counts per metre, launch/supersurfel_fusion_rgbd_benchmark.launch:47),
call process_frame once per line and append `stamp tx ty tz qx qy qz qw` to the trajectory file
(`estimated.txt`, same layout as the files the reference commits next to its datasets).  Optionally
the model is exported in the reference's text format at the end (exportModel,
core/src/supersurfel_fusion.cu:595-633).

The depth pre-filter of processFrame (cv::cuda::bilateralFilter(depth, -1, 0.03, 4.5), supersurfel_fusion.cu:180)
is ON, as in the reference (BENCHMARK_LAUNCH below).  Sparse VO, MOD and loop closure of the reference are out of
scope: the pose prior is the previous pose.  Pre-decoded frames (np.savez archives produced by `pack_frames`) replace the PNG files on
boxes without the dataset.

--raw-frames hands the decoded colour and the 16-bit depth to the handle as they are (Fusion.set_input_format, include/ssf_input.h):
the conversion happens in the kernels that load the pixels, and estimated.txt is the same, bit for bit.

--dynamic-masks DIR hands a detector's per-pixel mask of moving objects to the handle with each frame (include/ssf_dynamic.h):
DIR/<rgb stamp>.png (any 8-bit image; a colour one counts a pixel as masked when any channel is non-zero) or DIR/<rgb stamp>.npy
(H x W), non-zero = dynamic.  A frame without a file has no mask.  Superpixels of which at least half the pixels are masked get
confidence -1 and take no part in tracking or fusion.

--detect-motion lets the library make that mask itself from each depth frame and the map as it stands after the frame before
(include/ssf_motion.h: pixels clearly in front of the map, grown over depth-continuous pixels the map does not show).  The mask of
frame k needs the map after frame k - 1, so the run is sequential: not with --pipelined, and not with --dynamic-masks.
--motion-mask-dir DIR writes every frame's mask to DIR/<rgb stamp>.png (0 / 255).

--odometry-prior gives every frame but the first a pose prior from the library's dense RGB-D odometry against the frame before
(include/ssf_odometry.h); a frame whose estimate is invalid is tracked from the previous pose as without the option.  The prior of
frame k needs the pose of frame k - 1, so the run is sequential: not with --pipelined.  Together with --detect-motion the mask is
rendered at the odometry prior."""
import argparse
import os

import numpy as np

# The rgbd_benchmark launch column (launch/supersurfel_fusion_rgbd_benchmark.launch) with TUM fr1
# intrinsics (rgbd_benchmark/fr1_cam.yaml): what SupersurfelFusionRGBDBenchmarkNode hands to initialize().
BENCHMARK_LAUNCH = dict(width=640, height=480, fx=525.0, fy=525.0, cx=319.5, cy=239.5, cell_size=16, seg_iter=10,
                        lambda_pos=10.0, lambda_bound=1000.0, lambda_size=1000.0, lambda_disp=1e8, thresh_disp=1e-4,
                        filter_iter=3, filter_alpha=0.1, filter_beta=1.0, filter_threshold=0.05, range_min=0.2, range_max=5.0,
                        delta_t=20, conf_thresh=2560.0, nb_supersurfels_max=100000, icp_iter=10, icp_cov_thresh=0.05,
                        depth_prefilter=1, prefilter_sigma_color=0.03, prefilter_sigma_space=4.5)
# rgbd_benchmark/fr3_cam.yaml: the intrinsics the launch file loads for rgbd_dataset_freiburg3_walking_halfsphere
FR3_INTRINSICS = dict(fx=535.4, fy=539.2, cx=320.1, cy=247.6)


def read_associations(path, max_frames=None):
    """-> list of dict(stamp, rgb, depth, gt) ; gt = (t[3], q[4] xyzw) or None"""
    out = []
    with open(path) as f:
        for line in f:
            w = line.split()
            if len(w) < 4:
                break                                   # the node stops at the first short line (:592-593)
            gt = None
            if len(w) >= 12:
                v = [float(x) for x in w[5:12]]
                gt = (np.array(v[:3]), np.array(v[3:7]))
            out.append(dict(stamp=w[0], rgb=w[1], depth=w[3], gt=gt))
            if max_frames and len(out) >= max_frames:
                break
    return out


def decode_frame(dataset_dir, entry, depth_scale, raw=False):
    """(rgb u8 HxWx3, depth): float32 metres, or with raw the sensor's uint16 counts"""
    from PIL import Image
    rgb = np.asarray(Image.open(os.path.join(dataset_dir, entry["rgb"])).convert("RGB"), np.uint8)
    d16 = np.asarray(Image.open(os.path.join(dataset_dir, entry["depth"])), np.uint16)
    return rgb, (d16 if raw else convert_depth(d16, depth_scale))


def convert_depth(d16, depth_scale):
    """depth_u16.convertTo(depth, CV_32FC1, depthScale): float(v) * scale evaluated in double, rounded to f32"""
    return (d16.astype(np.float64) * float(depth_scale)).astype(np.float32)


def pack_frames(dataset_dir, assoc_path, out_npz, n):
    """Pre-decode the first n frames into one archive (rgb u8, depth u16, association lines)."""
    ent = read_associations(assoc_path, n)
    from PIL import Image
    arrs = {"lines": np.array([l for l in open(assoc_path).read().split("\n")[:n]])}
    for i, e in enumerate(ent):
        arrs["rgb%d" % i] = np.asarray(Image.open(os.path.join(dataset_dir, e["rgb"])).convert("RGB"), np.uint8)
        arrs["depth%d" % i] = np.asarray(Image.open(os.path.join(dataset_dir, e["depth"])), np.uint16)
    save_npz_parts(out_npz, arrs)


def npz_parts(path):
    """the files of a frame archive: `path` itself, or its parts <stem>.part<k>.npz (save_npz_parts), in frame order"""
    if os.path.exists(path):
        return [path]
    stem = path[:-4] if path.endswith(".npz") else path
    parts, k = [], 0
    while os.path.exists("%s.part%d.npz" % (stem, k)):
        parts.append("%s.part%d.npz" % (stem, k)); k += 1
    return parts


def save_npz_parts(path, arrs):
    """A frame archive (lines, rgb<k>, depth<k>) as one compressed file per frame, <stem>.part<k>.npz (part 0 also holds the
    association lines): every file of a committed archive stays below 1 MiB.  load_npz reads it back whole."""
    stem = path[:-4] if path.endswith(".npz") else path
    k = 0
    while "rgb%d" % k in arrs:
        part = {"rgb%d" % k: arrs["rgb%d" % k], "depth%d" % k: arrs["depth%d" % k]}
        if k == 0:
            part["lines"] = arrs["lines"]
        np.savez_compressed("%s.part%d.npz" % (stem, k), **part)
        k += 1


def load_npz(path):
    """the arrays of a frame archive, whole or in parts (npz_parts), as one dict"""
    parts = npz_parts(path)
    if not parts:
        raise FileNotFoundError(path)
    out = {}
    for p in parts:
        with np.load(p) as z:
            out.update({k: z[k] for k in z.files})
    return out


def rot_to_quat_xyzw(R):
    """tf::Matrix3x3::getRotation (Shoemake), the conversion the node applies before writing"""
    R = np.asarray(R, np.float64)
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    q = np.zeros(4)
    if tr > 0:
        s = np.sqrt(tr + 1.0)
        q[3] = 0.5 * s; s = 0.5 / s
        q[0] = (R[2, 1] - R[1, 2]) * s; q[1] = (R[0, 2] - R[2, 0]) * s; q[2] = (R[1, 0] - R[0, 1]) * s
    else:
        i = 0 if R[0, 0] >= R[1, 1] and R[0, 0] >= R[2, 2] else (1 if R[1, 1] >= R[2, 2] else 2)
        j, k = (i + 1) % 3, (i + 2) % 3
        s = np.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0)
        q[i] = 0.5 * s; s = 0.5 / s
        q[3] = (R[k, j] - R[j, k]) * s; q[j] = (R[j, i] + R[i, j]) * s; q[k] = (R[k, i] + R[i, k]) * s
    return q


def tum_line(stamp, pose12):
    """`stamp tx ty tz qx qy qz qw` with ostream's default 6 significant digits (:727-729)"""
    R = np.asarray(pose12[:9], np.float64).reshape(3, 3)
    t = np.asarray(pose12[9:], np.float64)
    q = rot_to_quat_xyzw(R)
    return " ".join([stamp] + ["%g" % v for v in list(t) + list(q)])


def read_pixel_mask(mask_dir, stamp, shape):
    """the pixel mask of the frame with rgb stamp `stamp` (H x W uint8, non-zero = dynamic), or None without a file"""
    npy, png = os.path.join(mask_dir, stamp + ".npy"), os.path.join(mask_dir, stamp + ".png")
    if os.path.exists(npy):
        m = np.load(npy)
    elif os.path.exists(png):
        from PIL import Image
        m = np.asarray(Image.open(png))
    else:
        return None
    if m.ndim == 3:
        m = m.any(axis=2)
    if m.shape != tuple(shape):
        raise ValueError("mask of %s is %s, the frame is %s" % (stamp, m.shape, tuple(shape)))
    return (np.asarray(m) != 0).astype(np.uint8)


def write_motion_mask(fusion, mask_dir, stamp):
    """the mask the library detected for the frame just processed (include/ssf_motion.h): mask_dir/<stamp>.png, 0 / 255 -- the form
    read_pixel_mask reads back"""
    from PIL import Image
    mask, _ = fusion.last_motion_mask()
    os.makedirs(mask_dir, exist_ok=True)
    Image.fromarray(mask * np.uint8(255)).save(os.path.join(mask_dir, stamp + ".png"))


def write_render(fusion, render_dir, stamp):
    """the model drawn at the tracked pose with the handle's camera (include/ssf_render.h): render_dir/<stamp>_rgb.png and
    render_dir/<stamp>_depth.npy (float32 metres, 0 = no supersurfel)"""
    from PIL import Image
    out = fusion.render_model(outputs=("depth", "rgb8"))
    os.makedirs(render_dir, exist_ok=True)
    Image.fromarray(out["rgb8"]).save(os.path.join(render_dir, stamp + "_rgb.png"))
    np.save(os.path.join(render_dir, stamp + "_depth.npy"), out["depth"])
    return out["stats"]


def write_local_cloud(fusion, cloud_dir, k, radius):
    """the part of the map within `radius` of the tracked pose's position, selected on the device (include/ssf_query.h, a sphere
    query: the reference's extractLocalPointCloud): cloud_dir/<k as %06d>.npz with positions, colors, normals (orientation row 2)
    and index (the rows' logical indices in get_model's order)"""
    out = fusion.query_model(fields=("positions", "colors", "orientations"), region="sphere", radius=radius)
    os.makedirs(cloud_dir, exist_ok=True)
    np.savez(os.path.join(cloud_dir, "%06d.npz" % k), positions=out["positions"], colors=out["colors"],
             normals=np.ascontiguousarray(out["orientations"][:, 6:9]), index=out["index"])
    return out["stats"]


def thin_views(poses, most=256):
    """at most `most` of the poses (12 floats each), evenly thinned, the first and the last kept: n x 12 f32"""
    v = np.asarray(poses, np.float32).reshape(-1, 12)
    if len(v) > most:
        v = v[np.round(np.linspace(0, len(v) - 1, most)).astype(np.int64)]
    return np.ascontiguousarray(v)


def plan_cells(pose, res, cam_t, goals_m):
    """the camera's cell (the plan's start) and the goals' cells: cam_t is the camera position in the map frame, goals_m are
    (X, Y) in metres in the grid frame whose 12 floats are `pose`; cell = floor(metres / res)"""
    R, t = np.asarray(pose[:9], np.float64).reshape(3, 3), np.asarray(pose[9:], np.float64)
    c = R.T @ (np.asarray(cam_t, np.float64) - t)
    start = np.floor(c[:2] / res).astype(np.int32).reshape(1, 2)
    goals = np.floor(np.asarray(goals_m, np.float64).reshape(-1, 2) / res).astype(np.int32)
    return start, goals


NAV_STEER_DT = 0.1                     # seconds per rollout step of --nav-steer
NAV_FRAME_DT = 1.0 / 30.0              # seconds between two frames, for --nav-steer-movers' velocities (the sequences here are 30 Hz)
# The tracker's steps_since is a whole number of rollout steps >= 1.  Grids fewer than three frames apart (--nav-grid-every 1 or 2) are
# 0.33 or 0.67 of a step apart and count as one step, so their movers' velocities come out up to three times too small; from three
# frames on the interval is rounded to the nearest step.  The replay is a demonstration: a control loop passes its own step count.


def steer_pose(pose, res, cam_pose):
    """the tracked camera projected into the grid whose 12 floats are `pose`, in the units of include/ssf_navsteer.h: its position
    (1024 sub-units per cell) and the heading of its optical axis in the grid's plane (65536 per turn): 1 x 3 int32"""
    R, t = np.asarray(pose[:9], np.float64).reshape(3, 3), np.asarray(pose[9:], np.float64)
    cam = np.asarray(cam_pose, np.float64)
    c = R.T @ (cam[9:12] - t)
    z = R.T @ cam[[2, 5, 8]]                                               # the camera's viewing direction in the grid frame
    yaw = float(np.arctan2(z[1], z[0]))
    return np.array([[np.floor(c[0] / res * 1024.0), np.floor(c[1] / res * 1024.0), int(np.rint(yaw / (2.0 * np.pi) * 65536.0)) & 0xFFFF]]).astype(np.int32)


def steer_lattice(speed, res):
    """the lattice of --nav-steer: 9 speeds from 0 to `speed` m/s (capped at one cell per step of NAV_STEER_DT), the default 33 turn rates"""
    top = min(1024, int(np.floor(speed * NAV_STEER_DT * 1024.0 / res)))
    return dict(n_v=9, v_min=0, v_step=top // 8) if top >= 8 else dict(n_v=1, v_min=top, v_step=0)


def write_nav_grid(fusion, grid_dir, k, res, carve_views=None, carve_stride=8, plan=None, frontiers=None, waypoints=None, live=None, steer=None,
                   fit_floor=None):
    """the navigation grid of the map, built on the device (include/ssf_navgrid.h) at the default size and frame (floor-aligned
    about the tracked camera) with cells of `res` metres: grid_dir/<k as %06d>.pgm -- the state in map_server's convention (205
    unknown, 254 free, 0 occupied; the image's top row is the grid's last) --, <k>.yaml beside it (map_server's keys; origin = the
    grid's corner along its own x and y axes; grid_to_map = the grid frame's 12 floats) and <k>_dist2.npy (squared clearance in
    cells).  carve_views (n x 12 camera poses): the grid is carved along their rays on a pixel lattice of carve_stride
    (include/ssf_navcarve.h), the files show the carved state, and <k>_seen.npy holds the ray entries per cell.
    plan (dict(goals=(X, Y) pairs in metres in the grid frame, frontier=bool, radius=metres)): the cost-to-goal field of that grid
    for a robot of that radius, from the camera's cell (include/ssf_navplan.h): <k>_cost.npy (u32, 0xFFFFFFFF = not reached),
    <k>_path.npy (the cells (ix, iy) from the camera's cell to the goal) and <k>_plan.json (the stats, the start and its status).
    frontiers (dict(min_cells, gain_radius)): the grid's frontier as regions (include/ssf_navfrontier.h), ranked by the cost of
    driving to them from the camera's cell for a robot of the plan's radius (0 without a plan): <k>_frontiers.json (regions = the
    table's records, order, stats, start) and <k>_frontier_regions.npy (the map: table index, -1 no member, -2 not in the table).
    waypoints (dict(lookahead=cells, los_radius=metres), with a plan only): the plan's path reduced to any-angle waypoints
    (include/ssf_navpath.h) that keep the path's clearance up to the squared los_radius and at least that: <k>_waypoints.npy ((n, 4)
    int32: ix, iy, index into the path with bit 30 on a forced step, seg_min) and <k>_waypoints.json (stats, status, path_min).
    live (dict(depth=the depth image of the frame just processed, min_hits, stride)): that frame stamped onto the grid
    (include/ssf_navlive.h) from the tracked pose: <k>_live_state.npy and <k>_live_dist2.npy, and one log line with the stats; the
    map's own grid, plan and regions above are written as without it.  With live['memory'] = dict(forget=ticks, slices=n) the frame goes
    into a height-sliced layer that remembers (include/ssf_navmem.h) instead: the tick is k + 1, marks and seen-through both expire
    after `forget` ticks (0: never), the layer is kept in live['memory'] from grid to grid as long as the grid's frame and size stay
    (it does not scroll), <k>_live_marks.npy, <k>_live_mark_tick.npy and <k>_live_seen_tick.npy are written as well, and the log
    line starts with nav-memory.
    steer (dict(horizon=steps, speed=metres per second), with a plan only): the velocity command of include/ssf_navsteer.h from the
    tracked camera projected into the grid (steer_pose), over steer_lattice's candidates with steps of NAV_STEER_DT seconds, on the
    live layer's state and dist2 when there is one and the grid's otherwise, with the plan's field as the cost and the plan's
    radius: <k>_steer_traj.npy ((best_len, 3) int32: x, y, heading of the winner's arc) and one log line with the command and the stats.
    With steer['footprint'] = (front, back, left, right) in metres from the robot's centre (and steer['headings'], default 16) the
    rollouts test that oriented rectangle instead of the disc alone (include/ssf_navfoot.h): its heading layers are made on the same
    state with nav_foot_pad's pad and written to <k>_foot_mask.npy (uint32 per cell: bit b = the body fits at heading bin b), with
    one nav-foot log line; the command is logged as without it.  With steer['poses'] = dict(turn_cost) as well, the rollouts' cost term
    is no longer the disc's field but the projection of the plan over (x, y, heading) for that body (include/ssf_navpose.h), from the
    plan's goal cells at any heading and the steer pose: <k>_pose_cost.npy (cell_cost), <k>_pose_bin.npy, <k>_pose_path.npy ((len, 3)
    int32: ix, iy, bin) and one nav-pose log line with the start's status and cost and the stats.
    With steer['movers'] = dict(tracker=a binding.MoverTracker, last=None) and a live layer, the rollouts steer among the frame's moving
    objects (include/ssf_navdyn.h): the motion detector's mask keeps them OUT of the live layer (mask_mode 2), its labels and the depth
    give their blobs in the grid frame, the tracker turns this table and the one of the grid before into movers (steps_since from
    the frames between the two at NAV_FRAME_DT seconds each), and nav_dyn_steer / nav_dyn_foot_steer refuse the steps that meet
    them: <k>_blobs.npy ((n, 8) int32), <k>_movers.npy ((n, 6) int32) and one nav-movers log line.
    fit_floor (dict(up=(X, Y, Z) or None)): the grid is built in the frame and bands of a floor plane fitted to the map just before it
    (include/ssf_navfloor.h) instead of the default ones, the live layer takes the same frame and bands, and the plane and the fit's
    counts go into <k>_floor.json with one nav-floor log line"""
    gkw = dict(res=res)
    if fit_floor is not None:
        import json
        fit = fusion.nav_floor(histograms=False, res=res, up=fit_floor.get("up"))
        gkw = dict(fit["grid"])
        os.makedirs(grid_dir, exist_ok=True)
        with open(os.path.join(grid_dir, "%06d_floor.json" % k), "w") as f:
            json.dump(dict({nm: fit[nm] for nm in ("status", "status_name", "rounds", "rows_used", "candidates", "direction_rows", "aligned",
                                                   "height_out_of_range", "height_rows", "height_bin", "inliers")},
                           normal=[float(v) for v in fit["normal"]], d=float(fit["d"]), origin=[float(v) for v in fit["origin"]],
                           camera_height=float(fit["camera_height"]), dir_bin=list(fit["dir_bin"]), rms=[float(v) for v in fit["rms"]],
                           z_min=gkw["z_min"], floor_max=gkw["floor_max"], z_max=gkw["z_max"]), f, sort_keys=True)
        print("nav-floor %06d: status=%s rounds=%d camera_height=%.3f candidates=%d inliers=%d" % (k, fit["status_name"], fit["rounds"],
              float(fit["camera_height"]), fit["candidates"], fit["inliers"][max(0, fit["rounds"] - 1)]))
    if carve_views is None:
        out = fusion.nav_grid(outputs=("state", "dist2"), **gkw)
    else:
        out = fusion.nav_grid_carve(thin_views(carve_views), outputs=("state", "dist2", "seen"), carve=dict(stride=carve_stride), **gkw)
    state, pose = out["state"], out["stats"]["pose"]
    os.makedirs(grid_dir, exist_ok=True)
    name = "%06d" % k
    img = np.where(state == 100, 0, np.where(state == 0, 254, 205)).astype(np.uint8)[::-1]
    with open(os.path.join(grid_dir, name + ".pgm"), "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (img.shape[1], img.shape[0]))
        f.write(np.ascontiguousarray(img).tobytes())
    R, t = pose[:9].reshape(3, 3).astype(np.float64), pose[9:].astype(np.float64)
    with open(os.path.join(grid_dir, name + ".yaml"), "w") as f:
        f.write("image: %s.pgm\nresolution: %.9g\norigin: [%.9g, %.9g, 0.0]\nnegate: 0\noccupied_thresh: 0.65\nfree_thresh: 0.196\n"
                % (name, res, float(R[:, 0] @ t), float(R[:, 1] @ t)))
        f.write("grid_to_map: [%s]\n" % ", ".join("%.9g" % v for v in pose))
    np.save(os.path.join(grid_dir, name + "_dist2.npy"), out["dist2"])
    if carve_views is not None:
        np.save(os.path.join(grid_dir, name + "_seen.npy"), out["seen"])
    lv = None
    movers = None
    if live is not None:
        mm = None
        if steer is not None and steer.get("movers") is not None:
            mm = fusion.motion_mask(live["depth"], outputs=("mask", "label"))
            table = fusion.nav_dyn_blobs(live["depth"], mm["mask"], mm["label"], grid_pose=pose, width=state.shape[1], height=state.shape[0], res=res)
            track = steer["movers"]
            frames_since = 1 if track.get("last") is None else max(1, k - track["last"])
            movers = track["tracker"].update(table["blobs"], max(1, int(round(frames_since * NAV_FRAME_DT / NAV_STEER_DT))))
            track["last"] = k
            np.save(os.path.join(grid_dir, name + "_blobs.npy"), table["blobs"])
            np.save(os.path.join(grid_dir, name + "_movers.npy"), movers)
            print("nav-movers %s: movers=%d pixels_masked=%d %s" % (name, len(movers), mm["stats"]["pixels_masked"],
                                                                   " ".join("%s=%d" % (nm, n) for nm, n in table["stats"].items())))
        lkw = dict(mask=None if mm is None else mm["mask"], grid_pose=pose, res=res, min_hits=int(live.get("min_hits", 4)),
                   stride=int(live.get("stride", 4)), mask_mode=0 if mm is None else 2)
        if fit_floor is not None:
            lkw.update(floor_max=gkw["floor_max"], z_max=gkw["z_max"])
        keep = live.get("memory")
        if keep is None:
            lv = fusion.nav_live(live["depth"], state, outputs=("state", "dist2"), **lkw)
        else:
            # the layer lives in the grid's frame and does not scroll (include/ssf_navmem.h): a grid of another frame or size starts afresh
            mem = keep.get("layer")
            fresh = mem is None or (mem.height, mem.width) != state.shape or not np.array_equal(keep.get("pose"), pose)
            if fresh:
                from .binding import LiveMemory
                mem = keep["layer"] = LiveMemory(state.shape[1], state.shape[0])
                keep["pose"] = np.array(pose, np.float32)
            forget = int(keep.get("forget", 0))
            lv = fusion.nav_memory(live["depth"], state, memory=mem, tick=k + 1, outputs=("state", "dist2"), slices=int(keep.get("slices", 16)),
                                   max_mark_age=forget, max_seen_age=forget, **lkw)
            for nm, a in zip(("marks", "mark_tick", "seen_tick"), mem.arrays()):
                np.save(os.path.join(grid_dir, name + "_live_" + nm + ".npy"), a)
        np.save(os.path.join(grid_dir, name + "_live_state.npy"), lv["state"])
        np.save(os.path.join(grid_dir, name + "_live_dist2.npy"), lv["dist2"])
        print("%s %s: %s%s" % ("nav-live" if keep is None else "nav-memory", name, "" if keep is None else "tick=%d fresh=%d " % (k + 1, fresh),
                               " ".join("%s=%d" % (nm, v) for nm, v in lv["stats"].items() if nm != "pose")))
    if plan is not None:
        import json
        start, goals = plan_cells(pose, res, fusion.get_pose()[9:12], plan.get("goals") or [])
        cells = int(np.ceil(float(plan.get("radius") or 0.0) / res))
        got = fusion.nav_plan(state, out["dist2"], goals, start, outputs=("cost", "start_cost", "start_status", "path"),
                              goals_from_frontier=bool(plan.get("frontier")), min_dist2=cells * cells, max_path=4 * sum(state.shape))
        np.save(os.path.join(grid_dir, name + "_cost.npy"), got["cost"])
        np.save(os.path.join(grid_dir, name + "_path.npy"), got["path"][0])
        with open(os.path.join(grid_dir, name + "_plan.json"), "w") as f:
            json.dump(dict(got["stats"], start=[int(v) for v in start[0]], start_status=int(got["start_status"][0]),
                           start_cost=int(got["start_cost"][0]), min_dist2=cells * cells), f, sort_keys=True)
        if waypoints is not None:
            los = int(np.ceil(float(waypoints.get("los_radius") or 0.0) / res))
            kw = dict(min_dist2=cells * cells, los_dist2=los * los, keep_clearance=1, clearance_cap=min(los * los, 1024 * 1024),
                      lookahead=int(waypoints.get("lookahead", 256)))
            wp = fusion.nav_waypoints(state, out["dist2"], [got["path"][0]], **kw)
            np.save(os.path.join(grid_dir, name + "_waypoints.npy"), wp["waypoints"][0])
            with open(os.path.join(grid_dir, name + "_waypoints.json"), "w") as f:
                json.dump(dict(wp["stats"], status=int(wp["status"][0]), path_min=int(wp["path_min"][0]), **kw), f, sort_keys=True)
        if steer is not None:
            on = lv if lv is not None else dict(state=state, dist2=out["dist2"])
            kw = dict(cost=got["cost"], min_dist2=cells * cells, n_steps=int(steer.get("horizon", 32)), **steer_lattice(float(steer.get("speed", 0.5)), res))
            if steer.get("footprint") is not None:
                body, bins = fusion.nav_foot_units(*[float(v) for v in steer["footprint"]], res), int(steer.get("headings", 16))
                lay = fusion.nav_foot(on["state"], n_headings=bins, pad=fusion.nav_foot_pad(n_headings=bins, **body), **body)
                np.save(os.path.join(grid_dir, name + "_foot_mask.npy"), lay["free_mask"])
                print("nav-foot %s: headings=%d %s" % (name, bins, " ".join("%s=%d" % (nm, n) for nm, n in lay["stats"].items())))
                at = steer_pose(pose, res, fusion.get_pose())
                if steer.get("poses") is not None:
                    pp = fusion.nav_pose_plan(lay["free_mask"], on["dist2"], [(int(g[0]), int(g[1]), -1) for g in goals], at,
                                              outputs=("cell_cost", "cell_bin", "start_cost", "start_status", "path"), n_headings=bins,
                                              min_dist2=cells * cells, turn_cost=int(steer["poses"].get("turn_cost", 5)), max_path=16 * sum(state.shape))
                    for nm in ("cell_cost", "cell_bin"):
                        np.save(os.path.join(grid_dir, name + "_pose_" + nm[5:] + ".npy"), pp[nm])
                    np.save(os.path.join(grid_dir, name + "_pose_path.npy"), pp["path"][0])
                    print("nav-pose %s: headings=%d status=%d cost=%d path=%d %s" % (name, bins, int(pp["start_status"][0]), int(pp["start_cost"][0]),
                                                                                    len(pp["path"][0]), " ".join("%s=%d" % (nm, n) for nm, n in pp["stats"].items())))
                    kw["cost"] = pp["cell_cost"]
                st = fusion.nav_foot_steer(lay["free_mask"], on["dist2"], at, bins, **kw) if movers is None else \
                    fusion.nav_dyn_foot_steer(lay["free_mask"], on["dist2"], at, bins, movers=movers, **kw)
            elif movers is not None:
                st = fusion.nav_dyn_steer(on["state"], on["dist2"], steer_pose(pose, res, fusion.get_pose()), movers=movers, **kw)
            else:
                st = fusion.nav_steer(on["state"], on["dist2"], steer_pose(pose, res, fusion.get_pose()), **kw)
            np.save(os.path.join(grid_dir, name + "_steer_traj.npy"), st["best_traj"][0])
            v, w = int(st["best_cmd"][0, 0]), int(st["best_cmd"][0, 1])
            print("nav-steer %s: status=%d best=%d v=%d w=%d linear_x=%.4f angular_z=%.4f score=%d n_admissible=%d best_len=%d %s"
                  % (name, int(st["pose_status"][0]), int(st["best"][0]), v, w, v * res / (1024.0 * NAV_STEER_DT), w * 2.0 * np.pi / (65536.0 * NAV_STEER_DT),
                     int(st["best_score"][0]), int(st["n_admissible"][0]), int(st["best_len"][0]),
                     " ".join("%s=%d" % (nm, n) for nm, n in st["stats"].items())))
    if frontiers is not None:
        import json
        start, _ = plan_cells(pose, res, fusion.get_pose()[9:12], [])
        cells = int(np.ceil(float((plan or {}).get("radius") or 0.0) / res))
        field = fusion.nav_plan(state, out["dist2"], start, outputs=("cost",), min_dist2=cells * cells)
        got = fusion.nav_frontiers(state, out["dist2"], field["cost"], min_cells=int(frontiers.get("min_cells", 1)),
                                   gain_radius=int(frontiers.get("gain_radius", 0)))
        np.save(os.path.join(grid_dir, name + "_frontier_regions.npy"), got["region"])
        with open(os.path.join(grid_dir, name + "_frontiers.json"), "w") as f:
            json.dump(dict(regions=[{nm: int(r[nm]) for nm in got["regions"].dtype.names} for r in got["regions"]],
                           order=[int(i) for i in got["order"]], stats=got["stats"], start=[int(v) for v in start[0]]), f, sort_keys=True)
    return out["stats"]


def keyframe_line(fusion, stamp, rec):
    """one line of the keyframe log: stamp, the id the frame was stored under (or -; "full" when the store had no room),
    min_diff_all, then every loop candidate as id:diff with the verdict of aligning it against the frame (include/ssf_keyframes.h;
    no prior: the identity, so a verdict is only expected to be valid for a near revisit)"""
    parts = [stamp, "full" if rec["full"] else (str(rec["id"]) if rec["added"] else "-"), str(rec["min_diff_all"])]
    for c in rec["candidates"]:
        if c["loop"]:
            a = fusion.keyframes_align(c["id"])
            parts.append("%d:%d:%s:pairs=%d" % (c["id"], c["diff"], "valid" if a["valid"] else "invalid", a["pairs"]))
    return " ".join(parts)


def laser_scan_rays(beams):
    """beams unit rays from the origin in the x-z plane of the camera frame (the plane of a level camera; y is down), beam i at
    angle -pi + i * 2 pi / beams about -y from the viewing direction z: n x 6 f32"""
    a = -np.pi + np.arange(int(beams)) * (2.0 * np.pi / int(beams))
    rays = np.zeros((int(beams), 6), np.float32)
    rays[:, 3], rays[:, 5] = np.sin(a), np.cos(a)
    return rays


def write_laser_scan(fusion, scan_dir, k, beams):
    """a planar laser scan simulated from the map on the device (include/ssf_raycast.h): `beams` rays from the tracked pose over the
    full circle in the camera's x-z plane (laser_scan_rays), within the configured depth range: scan_dir/<k as %06d>.npy, the
    ranges in metres as f32, +inf where nothing is hit (REP 117)"""
    t = fusion.raycast(laser_scan_rays(beams), outputs=("t",))["t"]
    os.makedirs(scan_dir, exist_ok=True)
    np.save(os.path.join(scan_dir, "%06d.npy" % k), np.where(t > 0, t, np.float32(np.inf)).astype(np.float32))


def replay(fusion, frames, out_path=None, export_model=None, pipelined=False, mask_dir=None, render_dir=None, render_every=30,
           keyframes=None, keyframe_log=None, local_cloud_dir=None, local_cloud_radius=2.0, local_cloud_every=30, detect_motion=False,
           motion_mask_dir=None, odometry_prior=False, nav_grid_dir=None, nav_grid_every=30, nav_grid_res=0.05,
           nav_grid_carve=False, nav_grid_carve_stride=8, nav_plan=None, nav_frontiers=None, nav_waypoints=None, nav_live=None, nav_steer=None, laser_scan_dir=None, laser_scan_every=30, laser_scan_beams=360,
           nav_fit_floor=None):
    """frames: iterable of (stamp, rgb u8 HxWx3, depth HxW in the handle's input format: f32 metres by default).  Returns (lines, results).
    pipelined: decode / submit ahead while earlier frames are tracked and fused (ssf_submit_frame /
    ssf_process_submitted, for handles created with pipeline_depth / extract_batch > 0 / 1); the trajectory is the
    same, bit for bit, as with one process_frame per line.
    mask_dir: per-frame pixel masks (read_pixel_mask), handed over with their frames (include/ssf_dynamic.h).
    render_dir: after frames 0, render_every, 2 render_every, ... the model is drawn at the tracked pose (write_render); pipelined,
    submission pauses at such a frame until it has been processed (a render needs no frame pending).
    local_cloud_dir: after frames 0, local_cloud_every, 2 local_cloud_every, ... the rows within local_cloud_radius of the tracked
    pose are written (write_local_cloud, numbered by frame); pipelined, submission pauses as for a render.
    nav_grid_dir: after frames 0, nav_grid_every, 2 nav_grid_every, ... the navigation grid of the map with cells of nav_grid_res
    metres is written (write_nav_grid, numbered by frame); pipelined, submission pauses as for a render.  nav_grid_carve: the grid
    is carved along the rays of the poses estimated so far (thin_views: at most 256 of them) on a pixel lattice of
    nav_grid_carve_stride, and <k>_seen.npy is written as well.  nav_plan (write_nav_grid's plan): the field, path and stats of a
    plan from the camera's cell are written next to each grid.  nav_frontiers (write_nav_grid's frontiers): the frontier regions
    of each grid, ranked from the camera's cell, are written next to it.  nav_live (dict(min_hits, stride)): the depth image of the
    frame just processed is stamped onto each grid (write_nav_grid's live; with a 'memory' dict(forget, slices) into the layer that
    remembers, one layer for the whole sequence).  nav_waypoints (write_nav_grid's waypoints; needs nav_plan):
    the plan's path reduced to waypoints is written next to it.  nav_steer (write_nav_grid's steer; needs nav_plan): the velocity command
    from the tracked camera's pose on each grid is logged and its arc written next to it.  nav_fit_floor (write_nav_grid's fit_floor):
    every grid is built in the frame of a floor plane fitted just before it.
    laser_scan_dir: after frames 0, laser_scan_every, 2 laser_scan_every, ... a planar scan of laser_scan_beams beams from the tracked
    pose is written (write_laser_scan, numbered by frame); pipelined, submission pauses as for a render.
    keyframes: a dict of ssf_keyframes_params fields ({} = the defaults): the keyframe database is configured and
    keyframes_consider runs after every frame (not pipelined: it needs no frame pending); keyframe_log: where keyframe_line's
    lines go (they are also kept in fusion.keyframe_lines).
    detect_motion: True or a dict of ssf_motion_params fields: every frame is processed with the pixel mask the library detects
    from its depth and the map (include/ssf_motion.h); sequential only, and not together with mask_dir.  motion_mask_dir: where
    write_motion_mask puts each of those masks.
    odometry_prior: True or a dict of ssf_odometry_params fields: every frame's pose prior comes from the library's dense odometry
    against the frame before (include/ssf_odometry.h); sequential only, not together with mask_dir; with detect_motion the mask
    is rendered at that prior."""
    lines, results = [], []
    if nav_grid_carve and not nav_grid_dir:
        raise ValueError("nav_grid_carve needs nav_grid_dir")
    if nav_plan is not None and not nav_grid_dir:
        raise ValueError("nav_plan needs nav_grid_dir")
    if nav_waypoints is not None and nav_plan is None:
        raise ValueError("nav_waypoints needs nav_plan")
    if nav_frontiers is not None and not nav_grid_dir:
        raise ValueError("nav_frontiers needs nav_grid_dir")
    if nav_live is not None and not nav_grid_dir:
        raise ValueError("nav_live needs nav_grid_dir")
    if nav_steer is not None and nav_plan is None:
        raise ValueError("nav_steer needs nav_plan")
    if nav_fit_floor is not None and not nav_grid_dir:
        raise ValueError("nav_fit_floor needs nav_grid_dir")
    if nav_steer is not None and nav_steer.get("movers") is not None:
        if nav_live is None:
            raise ValueError("nav_steer's movers need nav_live")
        nav_steer = dict(nav_steer, movers=mover_tracker_of(nav_steer["movers"], nav_grid_res))      # (one tracker for the whole sequence)
    if nav_live is not None and nav_live.get("memory") is not None:
        nav_live = dict(nav_live, memory=dict(nav_live["memory"]))            # (one layer for the whole sequence)
    live_of = (lambda depth: dict(nav_live, depth=depth)) if nav_live is not None else (lambda depth: None)
    carve_views = (lambda: [r["pose"] for r in results]) if nav_grid_carve else (lambda: None)
    if odometry_prior:
        if pipelined:
            raise ValueError("the odometry prior needs sequential processing (the prior of frame k is composed with the pose of frame "
                             "k - 1): replay it without pipelined")
        if mask_dir:
            raise ValueError("odometry_prior combines with detect_motion, not with mask_dir")
    if detect_motion:
        if pipelined:
            raise ValueError("motion detection needs sequential processing (the mask of frame k is taken against the map after frame "
                             "k - 1): replay it without pipelined")
        if mask_dir:
            raise ValueError("detect_motion makes the pixel masks itself: not together with mask_dir")
    elif motion_mask_dir:
        raise ValueError("motion_mask_dir needs detect_motion")
    if keyframes is not None:
        if pipelined:
            raise ValueError("the keyframe database is consulted between frames: replay it without pipelined")
        fusion.keyframes_configure(**keyframes)
        fusion.keyframe_lines = []
    render_every = max(1, int(render_every))
    local_cloud_every = max(1, int(local_cloud_every))
    nav_grid_every = max(1, int(nav_grid_every))
    laser_scan_every = max(1, int(laser_scan_every))
    # a frame after which the model is looked at (a render, a local cloud): nothing may be pending then
    looks = lambda k: bool((render_dir and k % render_every == 0) or (local_cloud_dir and k % local_cloud_every == 0) or
                           (nav_grid_dir and k % nav_grid_every == 0) or (laser_scan_dir and k % laser_scan_every == 0))
    mask_of = (lambda stamp, depth: read_pixel_mask(mask_dir, stamp, np.shape(depth))) if mask_dir else (lambda stamp, depth: None)
    if not pipelined:
        for stamp, rgb, depth in frames:
            m = mask_of(stamp, depth)
            if odometry_prior:
                r = fusion.process_frame(rgb, depth, odometry=odometry_prior, motion=detect_motion or None)
                if detect_motion and motion_mask_dir:
                    write_motion_mask(fusion, motion_mask_dir, stamp)
            elif detect_motion:
                r = fusion.process_frame(rgb, depth, motion=detect_motion)
                if motion_mask_dir:
                    write_motion_mask(fusion, motion_mask_dir, stamp)
            else:
                r = fusion.process_frame(rgb, depth) if m is None else fusion.process_frame(rgb, depth, pixel_mask=m)
            results.append(r)
            lines.append(tum_line(stamp, r["pose"]))
            if keyframes is not None:
                fusion.keyframe_lines.append(keyframe_line(fusion, stamp, fusion.keyframes_consider()))
            if render_dir and (len(lines) - 1) % render_every == 0:
                write_render(fusion, render_dir, stamp)
            if local_cloud_dir and (len(lines) - 1) % local_cloud_every == 0:
                write_local_cloud(fusion, local_cloud_dir, len(lines) - 1, local_cloud_radius)
            if nav_grid_dir and (len(lines) - 1) % nav_grid_every == 0:
                write_nav_grid(fusion, nav_grid_dir, len(lines) - 1, nav_grid_res, carve_views(), nav_grid_carve_stride, nav_plan, nav_frontiers,
                               nav_waypoints, live_of(depth), nav_steer, nav_fit_floor)
            if laser_scan_dir and (len(lines) - 1) % laser_scan_every == 0:
                write_laser_scan(fusion, laser_scan_dir, len(lines) - 1, laser_scan_beams)
    else:
        it, stamps, done = iter(frames), [], False
        held = []                                         # submitted host buffers stay alive until their frame is processed
        while True:
            while not done and fusion.can_submit() and not (len(stamps) > len(lines) and looks(len(stamps) - 1)):
                try:
                    stamp, rgb, depth = next(it)
                except StopIteration:
                    done = True
                    break
                rgb, depth = fusion._frame(rgb, depth)
                m = mask_of(stamp, depth)
                if m is None:
                    fusion.submit_frame(rgb, depth)       # (the copy is asynchronous: ssf.h, ssf_submit_frame)
                else:
                    fusion.submit_frame(rgb, depth, pixel_mask=m)
                held.append((rgb, depth, m))
                stamps.append(stamp)
            if fusion.pending_frames() == 0:
                break
            r = fusion.process_submitted().as_dict()
            last_depth = held.pop(0)[1]
            results.append(r)
            lines.append(tum_line(stamps[len(lines)], r["pose"]))
            if render_dir and (len(lines) - 1) % render_every == 0:
                write_render(fusion, render_dir, stamps[len(lines) - 1])
            if local_cloud_dir and (len(lines) - 1) % local_cloud_every == 0:
                write_local_cloud(fusion, local_cloud_dir, len(lines) - 1, local_cloud_radius)
            if nav_grid_dir and (len(lines) - 1) % nav_grid_every == 0:
                write_nav_grid(fusion, nav_grid_dir, len(lines) - 1, nav_grid_res, carve_views(), nav_grid_carve_stride, nav_plan, nav_frontiers,
                               nav_waypoints, live_of(last_depth), nav_steer, nav_fit_floor)
            if laser_scan_dir and (len(lines) - 1) % laser_scan_every == 0:
                write_laser_scan(fusion, laser_scan_dir, len(lines) - 1, laser_scan_beams)
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")
    if keyframes is not None and keyframe_log:
        with open(keyframe_log, "w") as f:
            f.write("".join(l + "\n" for l in fusion.keyframe_lines))
    if export_model:
        fusion.export_model_txt(export_model)
    return lines, results


def stage_figures(fusion, raw_depth):
    """Per-stage figures of the frame just processed against the RAW sensor depth it came from (a real-data sanity check
    of the extract stage that does not go through the trajectory): the plane-rendered depth of a3-a5 against the raw
    depth on the inlier pixels, the inlier share of the valid-depth pixels, the share of superpixels that became
    valid frame supersurfels (a6)."""
    plane = fusion.plane_depth().astype(np.float64)
    inl = fusion.inlier_map() != 0
    raw = np.asarray(raw_depth, np.float64)
    ok = inl & (raw > 0) & np.isfinite(plane)
    rel = np.abs(plane[ok] - raw[ok]) / raw[ok]
    fr = fusion.get_frame()
    return dict(plane_vs_raw_median=float(np.median(rel)) if rel.size else float("nan"),
                plane_vs_raw_p90=float(np.percentile(rel, 90)) if rel.size else float("nan"),
                inlier_share_of_valid_depth=float(ok.sum() / max(1, (raw > 0).sum())),
                valid_supersurfel_share=float((fr["confidences"] > 0).mean()))


def quat_xyzw_to_rot(q):
    x, y, z, w = [float(v) for v in q]
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def prior_consistency(fusion, frames, prior_xyz, prior_quat):
    """Every frame (rgb, depth) is processed with prior_xyz[i] / prior_quat[i] (camera-to-map, TUM order) as its pose
    prior -- processFrame's `pose = vo->getPose()` -- and the size of the ICP correction is recorded where the ICP
    result was accepted.  Frame 0 builds the map at its prior."""
    dt, da, valid, n = [], [], 0, 0
    for i, (rgb, depth) in enumerate(frames):
        R = quat_xyzw_to_rot(prior_quat[i])
        prior = np.concatenate([R.reshape(-1), np.asarray(prior_xyz[i], np.float64)]).astype(np.float32)
        r = fusion.process_frame(rgb, depth, prior_pose=prior)
        n += 1
        if i == 0 or not r["icp_valid"]:
            continue
        valid += 1
        P = np.asarray(r["pose"], np.float64)
        dR = R.T @ P[:9].reshape(3, 3)
        dt.append(float(np.linalg.norm(P[9:] - prior_xyz[i])))
        da.append(float(np.degrees(np.arccos(np.clip((np.trace(dR) - 1.0) / 2.0, -1.0, 1.0)))))
    return dict(frames=n, icp_valid_frames=valid,
                correction_translation_median_m=float(np.median(dt)) if dt else None,
                correction_translation_p90_m=float(np.percentile(dt, 90)) if dt else None,
                correction_rotation_median_deg=float(np.median(da)) if da else None,
                correction_rotation_p90_deg=float(np.percentile(da, 90)) if da else None)


def frames_from_dataset(dataset_dir, depth_scale=0.0002, max_frames=None, raw=False):
    for e in read_associations(os.path.join(dataset_dir, "associations_with_gt.txt"), max_frames):
        rgb, depth = decode_frame(dataset_dir, e, depth_scale, raw)
        yield e["stamp"], rgb, depth


def frames_from_npz(path, depth_scale=0.0002, raw=False):
    """(stamp, rgb, depth) of a frame archive; depth in float32 metres, or with raw the stored uint16 counts"""
    z = load_npz(path)
    i = 0
    while "rgb%d" % i in z:
        stamp = str(z["lines"][i]).split()[0]
        d16 = z["depth%d" % i]
        yield stamp, z["rgb%d" % i], (d16 if raw else convert_depth(d16, depth_scale))
        i += 1


def read_trajectory(path):
    """TUM trajectory file -> (stamps, xyz (n,3), quat xyzw (n,4)); '#' lines skipped"""
    rows = [l.split() for l in open(path) if l.strip() and not l.startswith("#")]
    v = np.array([[float(x) for x in r[1:8]] for r in rows])
    return [r[0] for r in rows], v[:, :3], v[:, 3:7]


def ate_rmse(est_xyz, gt_xyz):
    """Absolute trajectory error after Horn alignment (rigid, no scale), as the TUM tools compute it."""
    est, gt = np.asarray(est_xyz, np.float64), np.asarray(gt_xyz, np.float64)
    mu_e, mu_g = est.mean(0), gt.mean(0)
    Wm = (gt - mu_g).T @ (est - mu_e)
    U, _, Vt = np.linalg.svd(Wm)
    S = np.eye(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        S[2, 2] = -1
    R = U @ S @ Vt
    err = (gt - mu_g) - (est - mu_e) @ R.T
    return float(np.sqrt((err ** 2).sum(1).mean()))


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--dataset", help="TUM sequence directory with associations_with_gt.txt")
    ap.add_argument("--npz", help="pre-decoded frames (pack_frames) instead of --dataset")
    ap.add_argument("--out", default="estimated.txt")
    ap.add_argument("--depth-scale", type=float, default=0.0002)
    ap.add_argument("--max-frames", type=int, default=None)
    ap.add_argument("--export-model", default=None)
    ap.add_argument("--pipelined", action="store_true", help="extract of later frames runs ahead (pipeline_depth 2, extract_batch 4)")
    ap.add_argument("--raw-frames", action="store_true",
                    help="hand the decoded colour and the uint16 depth to the handle unconverted (input format rgb8 + u16 x --depth-scale)")
    ap.add_argument("--dynamic-masks", default=None, metavar="DIR",
                    help="per-frame pixel masks of moving objects: DIR/<rgb stamp>.png or .npy, non-zero = dynamic; no file = no mask")
    ap.add_argument("--detect-motion", action="store_true",
                    help="the library detects the moving objects itself from each depth frame and the map (sequential: not with "
                         "--pipelined; not with --dynamic-masks)")
    ap.add_argument("--motion-mask-dir", default=None, metavar="DIR", help="with --detect-motion: every frame's mask as DIR/<rgb stamp>.png")
    ap.add_argument("--odometry-prior", action="store_true",
                    help="the pose prior of every frame comes from the library's dense RGB-D odometry against the frame before "
                         "(sequential: not with --pipelined; not with --dynamic-masks; combines with --detect-motion)")
    ap.add_argument("--render-dir", default=None, metavar="DIR",
                    help="every --render-every frames, the model drawn at the tracked pose: DIR/<stamp>_rgb.png and DIR/<stamp>_depth.npy")
    ap.add_argument("--render-every", type=int, default=30, metavar="K")
    ap.add_argument("--local-cloud-dir", default=None, metavar="DIR",
                    help="every --local-cloud-every frames, the rows within --local-cloud-radius of the tracked pose, selected on the "
                         "device: DIR/<frame number as %%06d>.npz (positions, colors, normals, index)")
    ap.add_argument("--local-cloud-radius", type=float, default=2.0, metavar="R", help="metres (default 2)")
    ap.add_argument("--local-cloud-every", type=int, default=30, metavar="K")
    ap.add_argument("--nav-grid-dir", default=None, metavar="DIR",
                    help="every --nav-grid-every frames, the navigation grid of the map built on the device: DIR/<frame number as %%06d>.pgm "
                         "(map_server's convention), .yaml and _dist2.npy (squared clearance in cells)")
    ap.add_argument("--nav-grid-every", type=int, default=30, metavar="K")
    ap.add_argument("--nav-grid-res", type=float, default=0.05, metavar="R", help="metres per cell (default 0.05)")
    ap.add_argument("--nav-grid-fit-floor", action="store_true",
                    help="with --nav-grid-dir: every grid is built in the frame and bands of a floor plane fitted to the map just before it "
                         "(include/ssf_navfloor.h); the plane and the fit's counts go into _floor.json next to the grid")
    ap.add_argument("--nav-floor-up", nargs=3, type=float, default=None, metavar=("X", "Y", "Z"),
                    help="with --nav-grid-fit-floor: the up hint in the map frame (default 0 -1 0: the first camera's y points down)")
    ap.add_argument("--nav-grid-carve", action="store_true",
                    help="with --nav-grid-dir: carve free space along the rays of the poses estimated so far (at most 256, evenly thinned); "
                         "the files show the carved state, and _seen.npy (ray entries per cell) is written as well")
    ap.add_argument("--nav-grid-carve-stride", type=int, default=8, metavar="S", help="pixel lattice of the carving rays (default 8)")
    ap.add_argument("--nav-plan-goal", nargs=2, type=float, action="append", default=None, metavar=("X", "Y"),
                    help="with --nav-grid-dir: plan on every grid from the camera's cell to this goal (metres in the grid frame; repeatable); "
                         "_cost.npy, _path.npy and _plan.json are written next to the grid")
    ap.add_argument("--nav-plan-frontier", action="store_true", help="with --nav-grid-dir: every frontier cell of the grid is a goal")
    ap.add_argument("--nav-plan-radius", type=float, default=0.0, metavar="R",
                    help="the robot's radius in metres: cells with less clearance are not traversable (min_dist2 = ceil(R / res)^2)")
    ap.add_argument("--nav-plan-waypoints", action="store_true",
                    help="with --nav-plan-goal or --nav-plan-frontier: the plan's path reduced to any-angle waypoints on the device; "
                         "_waypoints.npy and _waypoints.json are written next to the plan's files")
    ap.add_argument("--nav-plan-lookahead", type=int, default=None, metavar="N", help="cells of the path looked ahead per waypoint, 1..4096 (default 256)")
    ap.add_argument("--nav-plan-los-radius", type=float, default=None, metavar="R",
                    help="metres: every cell of a straight leg keeps this clearance where the path has it (default 0)")
    ap.add_argument("--nav-frontiers", action="store_true",
                    help="with --nav-grid-dir: the frontier of every grid as regions, ranked by the cost of driving to them from the camera's "
                         "cell; _frontiers.json (table, order, stats) and _frontier_regions.npy (the map) are written next to the grid")
    ap.add_argument("--nav-frontier-min-cells", type=int, default=None, metavar="N", help="regions of fewer cells are dropped (default 1)")
    ap.add_argument("--nav-frontier-gain-radius", type=int, default=None, metavar="R",
                    help="cells, 0..128: count the unknown cells seen along rays of this length from each region (default 0: no gain)")
    ap.add_argument("--nav-live", action="store_true",
                    help="with --nav-grid-dir: the depth image of the frame just processed stamped onto every grid on the device (the live "
                         "obstacle layer); _live_state.npy and _live_dist2.npy are written next to the grid, and one log line with the stats")
    ap.add_argument("--nav-live-min-hits", type=int, default=None, metavar="N", help="points of the frame that make a cell occupied (default 4)")
    ap.add_argument("--nav-live-stride", type=int, default=None, metavar="S", help="pixel lattice of the see-through rays, 1..64 (default 4)")
    ap.add_argument("--nav-live-memory", action="store_true",
                    help="with --nav-live: the frame goes into a height-sliced live layer that remembers and is cleared when seen through "
                         "(include/ssf_navmem.h; the tick is the frame index + 1); _live_marks.npy, _live_mark_tick.npy and _live_seen_tick.npy "
                         "are written as well, and the log line starts with nav-memory")
    ap.add_argument("--nav-live-forget", type=int, default=None, metavar="TICKS",
                    help="with --nav-live-memory: marks and seen-through cells expire after this many frames without refreshment (default 0: never)")
    ap.add_argument("--nav-live-slices", type=int, default=None, metavar="N", help="with --nav-live-memory: height slices of the obstacle band, 1..32 (default 16)")
    ap.add_argument("--nav-steer", action="store_true",
                    help="with --nav-plan-goal or --nav-plan-frontier: the velocity command from the tracked camera's pose on each grid, rolled out "
                         "and scored on the device (include/ssf_navsteer.h): one nav-steer log line and <k>_steer_traj.npy per grid")
    ap.add_argument("--nav-steer-horizon", type=int, default=None, metavar="T", help="steps of 0.1 s per rollout, 1..256 (default 32)")
    ap.add_argument("--nav-steer-speed", type=float, default=None, metavar="V", help="the largest speed of the candidates in m/s, > 0 (default 0.5)")
    ap.add_argument("--nav-steer-footprint", type=float, nargs=4, default=None, metavar=("FRONT", "BACK", "LEFT", "RIGHT"),
                    help="with --nav-steer: the robot's body as a rectangle, metres from its centre; the rollouts test it at the headings they "
                         "sweep (include/ssf_navfoot.h) and <k>_foot_mask.npy holds its heading layers")
    ap.add_argument("--nav-steer-movers", action="store_true",
                    help="with --nav-steer and --nav-live: steer among the frame's moving objects (include/ssf_navdyn.h): the motion detector's "
                         "pixels stay out of the live layer and go to the rollouts as predicted discs: <k>_blobs.npy, <k>_movers.npy and one "
                         "nav-movers log line per grid")
    ap.add_argument("--nav-steer-mover-inflate", type=float, default=None, metavar="R", help="metres added to every mover's radius: the robot's own (default 0.3)")
    ap.add_argument("--nav-steer-mover-gate", type=float, default=None, metavar="G",
                    help="the largest distance in metres between a blob and the blob of the grid before that it is taken to be (default 1.0)")
    ap.add_argument("--nav-steer-headings", type=int, default=None, metavar="B", help="heading bins of --nav-steer-footprint: 1, 2, 4, 8, 16 or 32 (default 16)")
    ap.add_argument("--nav-plan-poses", action="store_true",
                    help="with --nav-steer-footprint and --nav-plan-goal: plan over (x, y, heading) for that body (include/ssf_navpose.h) and score the "
                         "rollouts on its field instead of the disc's: one nav-pose log line, <k>_pose_cost.npy, <k>_pose_bin.npy and <k>_pose_path.npy")
    ap.add_argument("--nav-plan-turn-cost", type=int, default=None, metavar="C", help="with --nav-plan-poses: the cost of turning by one heading bin, 1..1000 (default 5)")
    ap.add_argument("--laser-scan-dir", default=None, metavar="DIR",
                    help="every --laser-scan-every frames, a planar laser scan simulated from the map on the device, from the tracked pose: "
                         "DIR/<frame number as %%06d>.npy (ranges in metres, +inf where nothing is hit)")
    ap.add_argument("--laser-scan-every", type=int, default=30, metavar="K")
    ap.add_argument("--laser-scan-beams", type=int, default=360, metavar="N", help="beams over the full circle (default 360)")
    ap.add_argument("--keyframes", action="store_true",
                    help="keep the fern-coded keyframe database: after every frame one line (stamp, stored id or -, min_diff_all, loop candidates "
                         "with their alignment verdict); not with --pipelined")
    ap.add_argument("--keyframe-log", default=None, metavar="FILE", help="write those lines to FILE instead of the terminal")
    a = ap.parse_args(argv)
    if a.detect_motion and a.dynamic_masks:
        ap.error("--detect-motion and --dynamic-masks exclude each other: the library makes the masks, or a detector does")
    if a.detect_motion and a.pipelined:
        ap.error("--detect-motion needs sequential processing (the mask of frame k is taken against the map after frame k - 1): "
                 "not with --pipelined")
    if a.odometry_prior and a.pipelined:
        ap.error("--odometry-prior needs sequential processing (the prior of frame k is composed with the pose of frame k - 1): "
                 "not with --pipelined")
    if a.odometry_prior and a.dynamic_masks:
        ap.error("--odometry-prior combines with --detect-motion, not with --dynamic-masks")
    if a.motion_mask_dir and not a.detect_motion:
        ap.error("--motion-mask-dir needs --detect-motion")
    if a.nav_grid_carve and not a.nav_grid_dir:
        ap.error("--nav-grid-carve needs --nav-grid-dir")
    if a.nav_grid_fit_floor and not a.nav_grid_dir:
        ap.error("--nav-grid-fit-floor needs --nav-grid-dir")
    if a.nav_floor_up is not None and not a.nav_grid_fit_floor:
        ap.error("--nav-floor-up goes with --nav-grid-fit-floor")
    if a.nav_floor_up is not None and not any(a.nav_floor_up):
        ap.error("--nav-floor-up is not zero")
    if (a.nav_plan_goal or a.nav_plan_frontier) and not a.nav_grid_dir:
        ap.error("--nav-plan-goal and --nav-plan-frontier need --nav-grid-dir")
    if a.nav_plan_radius < 0.0 or (a.nav_plan_radius > 0.0 and not (a.nav_plan_goal or a.nav_plan_frontier)):
        ap.error("--nav-plan-radius is >= 0 and goes with --nav-plan-goal or --nav-plan-frontier")
    if a.nav_plan_waypoints and not (a.nav_plan_goal or a.nav_plan_frontier):
        ap.error("--nav-plan-waypoints goes with --nav-plan-goal or --nav-plan-frontier")
    if (a.nav_plan_lookahead is not None or a.nav_plan_los_radius is not None) and not a.nav_plan_waypoints:
        ap.error("--nav-plan-lookahead and --nav-plan-los-radius go with --nav-plan-waypoints")
    if a.nav_plan_lookahead is not None and not 1 <= a.nav_plan_lookahead <= 4096:
        ap.error("--nav-plan-lookahead is 1..4096")
    if a.nav_plan_los_radius is not None and a.nav_plan_los_radius < 0.0:
        ap.error("--nav-plan-los-radius is >= 0")
    if a.nav_frontiers and not a.nav_grid_dir:
        ap.error("--nav-frontiers needs --nav-grid-dir")
    if a.nav_live and not a.nav_grid_dir:
        ap.error("--nav-live needs --nav-grid-dir")
    if (a.nav_live_min_hits is not None or a.nav_live_stride is not None) and not a.nav_live:
        ap.error("--nav-live-min-hits and --nav-live-stride go with --nav-live")
    if a.nav_live_min_hits is not None and a.nav_live_min_hits < 1:
        ap.error("--nav-live-min-hits is >= 1")
    if a.nav_live_stride is not None and not 1 <= a.nav_live_stride <= 64:
        ap.error("--nav-live-stride is 1..64")
    if a.nav_live_memory and not a.nav_live:
        ap.error("--nav-live-memory goes with --nav-live")
    if (a.nav_live_forget is not None or a.nav_live_slices is not None) and not a.nav_live_memory:
        ap.error("--nav-live-forget and --nav-live-slices go with --nav-live-memory")
    if a.nav_live_forget is not None and not 0 <= a.nav_live_forget <= 0xFFFFFFFF:
        ap.error("--nav-live-forget is 0..4294967295")
    if a.nav_live_slices is not None and not 1 <= a.nav_live_slices <= 32:
        ap.error("--nav-live-slices is 1..32")
    if a.nav_steer and not (a.nav_plan_goal or a.nav_plan_frontier):
        ap.error("--nav-steer goes with --nav-plan-goal or --nav-plan-frontier")
    if (a.nav_steer_horizon is not None or a.nav_steer_speed is not None) and not a.nav_steer:
        ap.error("--nav-steer-horizon and --nav-steer-speed go with --nav-steer")
    if a.nav_steer_horizon is not None and not 1 <= a.nav_steer_horizon <= 256:
        ap.error("--nav-steer-horizon is 1..256")
    if a.nav_steer_speed is not None and not a.nav_steer_speed > 0.0:
        ap.error("--nav-steer-speed is > 0")
    if a.nav_steer_footprint is not None and not a.nav_steer:
        ap.error("--nav-steer-footprint goes with --nav-steer")
    if a.nav_steer_footprint is not None and min(a.nav_steer_footprint) < 0.0:
        ap.error("--nav-steer-footprint takes four lengths >= 0")
    if a.nav_steer_headings is not None and a.nav_steer_footprint is None:
        ap.error("--nav-steer-headings goes with --nav-steer-footprint")
    if a.nav_steer_headings is not None and a.nav_steer_headings not in (1, 2, 4, 8, 16, 32):
        ap.error("--nav-steer-headings is 1, 2, 4, 8, 16 or 32")
    if a.nav_steer_movers and not (a.nav_steer and a.nav_live):
        ap.error("--nav-steer-movers goes with --nav-steer and --nav-live")
    if (a.nav_steer_mover_inflate is not None or a.nav_steer_mover_gate is not None) and not a.nav_steer_movers:
        ap.error("--nav-steer-mover-inflate and --nav-steer-mover-gate go with --nav-steer-movers")
    if a.nav_steer_mover_inflate is not None and not a.nav_steer_mover_inflate >= 0.0:
        ap.error("--nav-steer-mover-inflate is >= 0")
    if a.nav_steer_mover_gate is not None and not a.nav_steer_mover_gate > 0.0:
        ap.error("--nav-steer-mover-gate is > 0")
    if a.nav_plan_poses and (a.nav_steer_footprint is None or not a.nav_plan_goal):
        ap.error("--nav-plan-poses goes with --nav-steer-footprint and --nav-plan-goal (its goals are cells, not the frontier)")
    if a.nav_plan_turn_cost is not None and not a.nav_plan_poses:
        ap.error("--nav-plan-turn-cost goes with --nav-plan-poses")
    if a.nav_plan_turn_cost is not None and not 1 <= a.nav_plan_turn_cost <= 1000:
        ap.error("--nav-plan-turn-cost is 1..1000")
    if (a.nav_frontier_min_cells is not None or a.nav_frontier_gain_radius is not None) and not a.nav_frontiers:
        ap.error("--nav-frontier-min-cells and --nav-frontier-gain-radius go with --nav-frontiers")
    if a.nav_frontier_min_cells is not None and a.nav_frontier_min_cells < 1:
        ap.error("--nav-frontier-min-cells is >= 1")
    if a.nav_frontier_gain_radius is not None and not 0 <= a.nav_frontier_gain_radius <= 128:
        ap.error("--nav-frontier-gain-radius is 0..128")
    return a


def nav_plan_of(a):
    """replay()'s nav_plan from the parsed options, or None"""
    if not (a.nav_plan_goal or a.nav_plan_frontier):
        return None
    return dict(goals=[tuple(g) for g in (a.nav_plan_goal or [])], frontier=bool(a.nav_plan_frontier), radius=float(a.nav_plan_radius))


def nav_waypoints_of(a):
    """replay()'s nav_waypoints from the parsed options, or None"""
    if not a.nav_plan_waypoints:
        return None
    return dict(lookahead=256 if a.nav_plan_lookahead is None else int(a.nav_plan_lookahead),
                los_radius=0.0 if a.nav_plan_los_radius is None else float(a.nav_plan_los_radius))


def nav_live_of(a):
    """replay()'s nav_live from the parsed options, or None"""
    if not a.nav_live:
        return None
    live = dict(min_hits=4 if a.nav_live_min_hits is None else int(a.nav_live_min_hits), stride=4 if a.nav_live_stride is None else int(a.nav_live_stride))
    if a.nav_live_memory:
        live["memory"] = dict(forget=0 if a.nav_live_forget is None else int(a.nav_live_forget), slices=16 if a.nav_live_slices is None else int(a.nav_live_slices))
    return live


def nav_steer_of(a):
    """replay()'s nav_steer from the parsed options, or None"""
    if not a.nav_steer:
        return None
    steer = dict(horizon=32 if a.nav_steer_horizon is None else int(a.nav_steer_horizon), speed=0.5 if a.nav_steer_speed is None else float(a.nav_steer_speed))
    if a.nav_steer_footprint is not None:
        steer.update(footprint=tuple(float(v) for v in a.nav_steer_footprint), headings=16 if a.nav_steer_headings is None else int(a.nav_steer_headings))
    if a.nav_plan_poses:
        steer.update(poses=dict(turn_cost=5 if a.nav_plan_turn_cost is None else int(a.nav_plan_turn_cost)))
    if a.nav_steer_movers:
        steer.update(movers=dict(inflate=0.3 if a.nav_steer_mover_inflate is None else float(a.nav_steer_mover_inflate),
                                 gate=1.0 if a.nav_steer_mover_gate is None else float(a.nav_steer_mover_gate)))
    return steer


def mover_tracker_of(movers, res):
    """write_nav_grid's steer['movers'] from nav_steer_of's: the tracker with the gate and the inflation in sub-units of a grid of `res`"""
    from . import binding
    units = lambda metres: int(round(float(metres) / res * 1024.0))
    return dict(tracker=binding.MoverTracker(gate=units(movers.get("gate", 1.0)), inflate=units(movers.get("inflate", 0.3))), last=None)


def nav_frontiers_of(a):
    """replay()'s nav_frontiers from the parsed options, or None"""
    if not a.nav_frontiers:
        return None
    return dict(min_cells=1 if a.nav_frontier_min_cells is None else int(a.nav_frontier_min_cells),
                gain_radius=0 if a.nav_frontier_gain_radius is None else int(a.nav_frontier_gain_radius))


def nav_fit_floor_of(a):
    """replay()'s nav_fit_floor from the parsed options, or None"""
    if not a.nav_grid_fit_floor:
        return None
    return dict(up=None if a.nav_floor_up is None else tuple(float(v) for v in a.nav_floor_up))


def library_of(a):
    """the name of binding's loader of the library that exports every entry point the parsed options ask for (the carve's, the plan's,
    the regions', the waypoints', the live layer's, the commands', the footprint's, the pose plan's and the movers' entry points: libraries
    of their own, each holding the one before it)"""
    if nav_fit_floor_of(a) is not None:
        return "load_floor"                                               # (the last of the chain: it holds whatever else is asked for)
    steer = nav_steer_of(a)
    if (nav_live_of(a) or {}).get("memory") is not None:
        return "load_mem"                                                 # (it holds whatever else is asked for without the fit)
    if steer:
        if steer.get("movers") is not None:
            return "load_dyn"
        if steer.get("poses") is not None:
            return "load_pose"
        return "load_foot" if steer.get("footprint") is not None else "load_steer"
    if nav_live_of(a):
        return "load_live"
    if nav_waypoints_of(a):
        return "load_drive"
    if nav_frontiers_of(a):
        return "load_explore"
    if nav_plan_of(a):
        return "load_nav"
    return "load_navcarve" if a.nav_grid_carve else "load_product"


def main(argv=None):
    a = parse_args(argv)
    from . import binding
    plan, frontiers, waypoints, live, steer = nav_plan_of(a), nav_frontiers_of(a), nav_waypoints_of(a), nav_live_of(a), nav_steer_of(a)
    lib = getattr(binding, library_of(a))()
    cfg = lib.default_config(pipeline_depth=2 if a.pipelined else 0, extract_batch=4 if a.pipelined else 1, **BENCHMARK_LAUNCH)
    f = binding.Fusion(lib, cfg)
    if a.raw_frames:
        f.set_input_format("rgb8", "u16", a.depth_scale)
    frames = (frames_from_npz(a.npz, a.depth_scale, a.raw_frames) if a.npz
              else frames_from_dataset(a.dataset, a.depth_scale, a.max_frames, a.raw_frames))
    lines, res = replay(f, frames, a.out, a.export_model, pipelined=a.pipelined, mask_dir=a.dynamic_masks,
                        render_dir=a.render_dir, render_every=a.render_every, local_cloud_dir=a.local_cloud_dir,
                        local_cloud_radius=a.local_cloud_radius, local_cloud_every=a.local_cloud_every, keyframes={} if a.keyframes else None,
                        keyframe_log=a.keyframe_log, detect_motion=a.detect_motion, motion_mask_dir=a.motion_mask_dir,
                        odometry_prior=a.odometry_prior, nav_grid_dir=a.nav_grid_dir, nav_grid_every=a.nav_grid_every,
                        nav_grid_res=a.nav_grid_res, nav_grid_carve=a.nav_grid_carve, nav_grid_carve_stride=a.nav_grid_carve_stride, nav_plan=plan,
                        nav_frontiers=frontiers, nav_waypoints=waypoints, nav_live=live, nav_steer=steer,
                        laser_scan_dir=a.laser_scan_dir, laser_scan_every=a.laser_scan_every,
                        laser_scan_beams=a.laser_scan_beams, nav_fit_floor=nav_fit_floor_of(a))
    if a.keyframes and not a.keyframe_log:
        print("\n".join(f.keyframe_lines))
    print("%d frames -> %s ; %d supersurfels" % (len(lines), a.out, res[-1]["n_model"] if res else 0))


if __name__ == "__main__":
    main()
