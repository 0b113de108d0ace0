"""ctypes binding of the C ABI in include/ssf.h.

The binding is library-agnostic: it drives whatever shared object exporting this ABI it is handed.
The product entry point is load_product() (libssf_hip.so, hand-written HIP for gfx950); tests and
the bench's cpu_baseline leg hand the same class the CPU checker library.  Names follow the reference's C++ surface
(core/include/supersurfel_fusion/supersurfel_fusion.hpp:40-143): Fusion.process_frame ==
SupersurfelFusion::processFrame, get_pose == getPose, get_model == getModel, ...
"""
import ctypes as C
import os
import numpy as np

ICP_RECORD = 29
MIGRANT_WORDS = 28
_HERE = os.path.dirname(os.path.abspath(__file__))
PRODUCT_LIB = os.path.join(_HERE, "csrc", "libssf_hip.so")
# the product's objects plus the carve of the navigation grid (include/ssf_navcarve.h; csrc/Makefile): everything the product exports,
# and the carve's entry points, which the product library does not export
NAVCARVE_LIB = os.path.join(_HERE, "csrc", "libssf_hip_navcarve.so")
# the product's objects, the carve and the plan on the navigation grid (include/ssf_navplan.h): the one library of a robot that
# builds, carves and plans.  Neither of the two libraries above exports the plan's entry points
NAV_LIB = os.path.join(_HERE, "csrc", "libssf_hip_nav.so")
# nav's objects and the frontier regions (include/ssf_navfrontier.h): the one library of a robot that builds, carves, plans and
# explores.  None of the three libraries above exports the regions' entry points
EXPLORE_LIB = os.path.join(_HERE, "csrc", "libssf_hip_explore.so")
# explore's objects and the waypoints of the plan's paths (include/ssf_navpath.h): the one library of a robot that builds, carves, plans,
# explores and drives.  None of the four libraries above exports the waypoints' entry points
DRIVE_LIB = os.path.join(_HERE, "csrc", "libssf_hip_drive.so")
# drive's objects and the live obstacle layer (include/ssf_navlive.h): the one library of a robot that also stamps the depth frame of
# the instant onto its grid.  None of the five libraries above exports the overlay's entry points
LIVE_LIB = os.path.join(_HERE, "csrc", "libssf_hip_live.so")
# live's objects and the velocity commands (include/ssf_navsteer.h): the one library of a robot that also steers on its grid.  None of
# the six libraries above exports the rollouts' entry points
STEER_LIB = os.path.join(_HERE, "csrc", "libssf_hip_steer.so")
# steer's objects and the oriented footprint (include/ssf_navfoot.h): the one library of a robot whose base is not round.  None of the
# seven libraries above exports the footprint's entry points
FOOT_LIB = os.path.join(_HERE, "csrc", "libssf_hip_foot.so")
# foot's objects and the plan over (x, y, heading) (include/ssf_navpose.h): the one library of a robot whose global plan knows its
# body as well.  None of the eight libraries above exports the pose plan's entry points
POSE_LIB = os.path.join(_HERE, "csrc", "libssf_hip_pose.so")
# pose's objects and steering among movers (include/ssf_navdyn.h): the one library of a robot that also drives among people.  None
# of the nine libraries above exports the movers' entry points
DYN_LIB = os.path.join(_HERE, "csrc", "libssf_hip_dyn.so")
# dyn's objects and the live layer with memory (include/ssf_navmem.h): the one library of a robot whose live obstacles outlive their
# time in view and are cleared when seen through.  None of the ten libraries above exports the memory's entry points
MEM_LIB = os.path.join(_HERE, "csrc", "libssf_hip_mem.so")
# mem's objects and the fitted floor plane (include/ssf_navfloor.h): the one library of a robot that also finds the grid's frame and
# bands in its map.  None of the eleven libraries above exports the fit's entry points
FLOOR_LIB = os.path.join(_HERE, "csrc", "libssf_hip_floor.so")


class SsfConfig(C.Structure):
    _fields_ = [
        ("width", C.c_int), ("height", C.c_int),
        ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
        ("cell_size", C.c_int), ("lambda_pos", C.c_float), ("lambda_bound", C.c_float),
        ("lambda_size", C.c_float), ("lambda_disp", C.c_float), ("thresh_disp", C.c_float),
        ("seg_iter", C.c_int), ("seg_use_ransac", C.c_int), ("nb_samples", C.c_int),
        ("filter_iter", C.c_int), ("filter_alpha", C.c_float), ("filter_beta", C.c_float),
        ("filter_threshold", C.c_float), ("range_min", C.c_float), ("range_max", C.c_float),
        ("delta_t", C.c_int), ("conf_thresh", C.c_float), ("nb_supersurfels_max", C.c_int),
        ("icp_iter", C.c_int), ("icp_cov_thresh", C.c_double),
        ("rng_seed", C.c_uint64), ("icp_force_iters", C.c_int), ("device_id", C.c_int),
        ("stream", C.c_void_p), ("rank", C.c_int), ("nranks", C.c_int),
        ("shard_tile", C.c_float), ("depth_prefilter", C.c_int), ("prefilter_sigma_color", C.c_float),
        ("prefilter_sigma_space", C.c_float), ("profile", C.c_int), ("pipeline_depth", C.c_int), ("extract_batch", C.c_int),
    ]


class SsfSurfels(C.Structure):
    _fields_ = [("positions", C.c_void_p), ("colors", C.c_void_p), ("stamps", C.c_void_p),
                ("orientations", C.c_void_p), ("shapes", C.c_void_p), ("dims", C.c_void_p),
                ("confidences", C.c_void_p)]


class SsfFrameResult(C.Structure):
    _fields_ = [("pose", C.c_float * 12), ("icp_valid", C.c_int), ("icp_iters", C.c_int),
                ("n_model", C.c_int), ("n_visible", C.c_int), ("n_removed", C.c_int),
                ("n_inserted", C.c_int), ("n_updated", C.c_int), ("stamp", C.c_int),
                ("stage_ms", C.c_float * 3)]

    def as_dict(self):
        return dict(pose=np.array(self.pose[:], np.float32), icp_valid=self.icp_valid,
                    icp_iters=self.icp_iters, n_model=self.n_model, n_visible=self.n_visible,
                    n_removed=self.n_removed, n_inserted=self.n_inserted, n_updated=self.n_updated,
                    stamp=self.stamp, stage_ms=list(self.stage_ms[:]))


# every symbol include/ssf.h declares (tests check that each one is exported)
ABI_SYMBOLS = [
    "ssf_abi_version", "ssf_backend_name", "ssf_default_config", "ssf_create", "ssf_destroy",
    "ssf_last_error", "ssf_process_frame", "ssf_process_frame_device", "ssf_stage_extract",
    "ssf_debug_set_max_passes", "ssf_debug_set_bin_min_rows", "ssf_stage_set_shard", "ssf_stage_icp_begin",
    "ssf_stage_icp_accumulate", "ssf_stage_icp_update", "ssf_stage_icp_end", "ssf_stage_match",
    "ssf_stage_fuse", "ssf_get_pose", "ssf_set_pose", "ssf_get_counts", "ssf_get_model",
    "ssf_get_frame", "ssf_set_model", "ssf_get_index_map", "ssf_get_boundary_map",
    "ssf_get_inlier_map", "ssf_get_plane_depth", "ssf_get_superpixels", "ssf_get_model_device", "ssf_get_frame_device",
    "ssf_export_model_txt", "ssf_apply_deformation", "ssf_get_kernel_times",
    "ssf_reset_kernel_times", "ssf_set_profile", "ssf_bilateral_filter", "ssf_submit_frame",
    "ssf_process_submitted", "ssf_pending_frames", "ssf_pipeline_capacity", "ssf_can_submit", "ssf_stage_begin_submitted",
    "ssf_stage_icp_accumulate_device", "ssf_stage_icp_fetch", "ssf_stage_match_device", "ssf_stage_fuse_device",
    "ssf_comm_unique_id", "ssf_comm_attach", "ssf_comm_info", "ssf_p2p_export", "ssf_p2p_attach", "ssf_p2p_region", "ssf_p2p_attach_local", "ssf_p2p_configure", "ssf_rehome_begin", "ssf_rehome_end", "ssf_get_global_counts", "ssf_align", "ssf_fern_codes", "ssf_process_sequence", "ssf_debug_recentre", "ssf_debug_recentre_count", "ssf_get_preview_image", "ssf_stage_fuse_begin", "ssf_stage_fuse_end", "ssf_stage_fuse_begin_device", "ssf_stage_fuse_end_device",
    "ssf_sequence_times", "ssf_sequence_marks", "ssf_stream_copy_rate", "ssf_upload_stats", "ssf_pooled_streams", "ssf_waiter_matches", "ssf_waiter_match_repairs", "ssf_tuner_state", "ssf_submit_frame_tables", "ssf_comm_deal_extract",
]

# the input-format entry points of include/ssf_input.h: exported by the HIP product only, not part of ssf.h (ABI_SYMBOLS)
INPUT_FORMAT_SYMBOLS = ["ssf_set_input_format", "ssf_get_input_format"]
# ssf_color_format / ssf_depth_format: name -> (enum value, bytes per pixel)
COLOR_FORMATS = {"rgb8": (0, 3), "bgr8": (1, 3), "rgba8": (2, 4), "bgra8": (3, 4)}
DEPTH_FORMATS = {"f32": (0, 4), "u16": (1, 2)}
# the pixel-mask entry points of include/ssf_dynamic.h: exported by the HIP product only, not part of ssf.h (ABI_SYMBOLS)
DYNAMIC_MASK_SYMBOLS = ["ssf_process_frame_pixmask", "ssf_submit_frame_pixmask", "ssf_process_sequence_pixmask",
                        "ssf_stage_extract_pixmask", "ssf_get_dynamic_superpixels"]
# the model drawn into a virtual camera (include/ssf_render.h): exported by the HIP product only, not part of ssf.h (ABI_SYMBOLS)
RENDER_SYMBOLS = ["ssf_render_default_params", "ssf_render_model"]
# the deformation graph's nodes and per-row binding (include/ssf_graph.h): exported by the HIP product only, not part of ssf.h
GRAPH_SYMBOLS = ["ssf_graph_default_params", "ssf_graph_build", "ssf_graph_get_nodes", "ssf_graph_get_binding",
                 "ssf_graph_bind_points", "ssf_graph_apply", "ssf_graph_info"]
# the graph's optimisation (include/ssf_graph_solve.h): HIP product only
GRAPH_SOLVE_SYMBOLS = ["ssf_graph_solve_default_params", "ssf_graph_get_edges", "ssf_graph_solve", "ssf_graph_get_transforms",
                       "ssf_graph_apply_solved"]
# the fern-coded keyframe database (include/ssf_keyframes.h): exported by the HIP product only, not part of ssf.h (ABI_SYMBOLS)
KEYFRAME_SYMBOLS = ["ssf_keyframes_default_params", "ssf_keyframes_configure", "ssf_keyframes_set_ferns", "ssf_keyframes_get_ferns",
                    "ssf_keyframes_encode", "ssf_keyframes_query", "ssf_keyframes_add", "ssf_keyframes_consider", "ssf_keyframes_put",
                    "ssf_keyframes_get", "ssf_keyframes_set_pose", "ssf_keyframes_align", "ssf_keyframes_info", "ssf_keyframes_clear"]
KEYFRAMES_MAX_FERNS = 4096
KEYFRAMES_MAX_CANDIDATES = 8
# ssf_fern as a numpy record (12 bytes)
FERN_DTYPE = np.dtype([("x", np.uint16), ("y", np.uint16), ("r", np.uint8), ("g", np.uint8), ("b", np.uint8), ("pad", np.uint8),
                       ("depth_mm", np.uint32)])
# rows of the model selected on the device (include/ssf_query.h): exported by the HIP product only, not part of ssf.h (ABI_SYMBOLS)
QUERY_SYMBOLS = ["ssf_query_default_params", "ssf_query_count", "ssf_query_rows"]
QUERY_REGIONS = {"all": 0, "sphere": 1, "box": 2, "frustum": 3}
# the floor-plane navigation grid (include/ssf_navgrid.h): exported by the HIP product only, not part of ssf.h (ABI_SYMBOLS)
NAVGRID_SYMBOLS = ["ssf_navgrid_default_params", "ssf_navgrid_default_pose", "ssf_navgrid_build"]
# the arrays of ssf_navgrid_out, in its field order: name, dtype, per-cell shape
NAVGRID_OUTPUTS = (("zmin", np.float32, ()), ("zmax", np.float32, ()), ("hits", np.uint32, (2,)), ("state", np.int8, ()),
                   ("dist2", np.int32, ()))
NAVGRID_OUTPUT_NAMES = tuple(nm for nm, _, _ in NAVGRID_OUTPUTS)
# the navigation grid with free space carved along camera rays (include/ssf_navcarve.h): exported by libssf_hip_navcarve.so only
# (load_navcarve), not part of ssf.h
NAVCARVE_SYMBOLS = ["ssf_navcarve_default_params", "ssf_navgrid_carve", "ssf_debug_navcarve_set_chunk_rays", "ssf_debug_navcarve_last"]
NAVCARVE_OUTPUTS = NAVGRID_OUTPUTS + (("seen", np.uint32, ()),)
NAVCARVE_OUTPUT_NAMES = tuple(nm for nm, _, _ in NAVCARVE_OUTPUTS)
# the plan on the navigation grid (include/ssf_navplan.h): exported by libssf_hip_nav.so only (load_nav), not part of ssf.h
NAVPLAN_SYMBOLS = ["ssf_navplan_default_params", "ssf_navplan_field", "ssf_debug_navplan_set_round_batch", "ssf_debug_navplan_last"]
NAVPLAN_OUTPUT_NAMES = ("cost", "frontier", "start_cost", "start_status", "path_len", "path")
NAVPLAN_UNREACHED = 0xFFFFFFFF
# the frontier regions of the navigation grid (include/ssf_navfrontier.h): exported by libssf_hip_explore.so only (load_explore)
NAVFRONTIER_SYMBOLS = ["ssf_navfrontier_default_params", "ssf_navfrontier_regions"]
NAVFRONTIER_MAX_REGIONS = 65536
# ssf_navfrontier_region as a numpy record (56 bytes)
NAVFRONTIER_REGION_DTYPE = np.dtype([("sum_x", np.int64), ("sum_y", np.int64), ("label", np.int32), ("cells", np.int32), ("x0", np.int32),
                                     ("y0", np.int32), ("x1", np.int32), ("y1", np.int32), ("rep_x", np.int32), ("rep_y", np.int32),
                                     ("rep_cost", np.uint32), ("gain", np.int32)])
# the waypoints of the plan's paths (include/ssf_navpath.h): exported by libssf_hip_drive.so only (load_drive)
NAVPATH_SYMBOLS = ["ssf_navpath_default_params", "ssf_navpath_waypoints"]
NAVPATH_OUTPUT_NAMES = ("n_waypoints", "status", "waypoints", "path_min")
NAVPATH_FORCED = 1 << 30             # bit 30 of a waypoint's index word: the segment that leads to it was not visible
# the live obstacle layer (include/ssf_navlive.h): exported by libssf_hip_live.so only (load_live)
NAVLIVE_SYMBOLS = ["ssf_navlive_default_params", "ssf_navlive_overlay"]
NAVLIVE_OUTPUTS = (("live_hits", np.uint32), ("live_seen", np.uint32), ("state", np.int8), ("dist2", np.int32))
NAVLIVE_OUTPUT_NAMES = tuple(nm for nm, _ in NAVLIVE_OUTPUTS)
# the live layer with memory (include/ssf_navmem.h): exported by libssf_hip_mem.so only (load_mem)
NAVMEM_SYMBOLS = ["ssf_navmem_default_params", "ssf_navmem_update"]
NAVMEM_LAYER_NAMES = ("marks", "mark_tick", "seen_tick")
NAVMEM_OUTPUTS = (("marks", np.uint32), ("mark_tick", np.uint32), ("seen_tick", np.uint32), ("live_hits", np.uint32), ("hit_bits", np.uint32),
                  ("seen_bits", np.uint32), ("state", np.int8), ("dist2", np.int32))
NAVMEM_OUTPUT_NAMES = tuple(nm for nm, _ in NAVMEM_OUTPUTS)
# the fitted floor plane (include/ssf_navfloor.h): exported by libssf_hip_floor.so only (load_floor)
NAVFLOOR_SYMBOLS = ["ssf_navfloor_default_params", "ssf_navfloor_fit"]
NAVFLOOR_STATUS = ("ok", "no_floor", "degenerate")
NAVFLOOR_DIR_BINS, NAVFLOOR_HEIGHT_BINS, NAVFLOOR_MAX_ROUNDS = 31, 2048, 8
# the velocity commands (include/ssf_navsteer.h): exported by libssf_hip_steer.so only (load_steer)
NAVSTEER_SYMBOLS = ["ssf_navsteer_rollouts", "ssf_navsteer_default_params", "ssf_navsteer_direction_table"]
# (name, dtype, per pose or per candidate, trailing shape; 'T1' = n_steps + 1)
NAVSTEER_OUTPUTS = (("best", np.int32, "pose", ()), ("best_cmd", np.int32, "pose", (2,)), ("best_score", np.int64, "pose", ()),
                    ("n_admissible", np.int32, "pose", ()), ("pose_status", np.int32, "pose", ()), ("best_len", np.int32, "pose", ()),
                    ("best_traj", np.int32, "pose", ("T1", 3)), ("cand_free", np.int32, "cand", ()), ("cand_min_d", np.int32, "cand", ()),
                    ("cand_end", np.int32, "cand", (3,)), ("cand_end_cost", np.uint32, "cand", ()), ("cand_score", np.int64, "cand", ()))
NAVSTEER_OUTPUT_NAMES = tuple(o[0] for o in NAVSTEER_OUTPUTS)
NAVSTEER_POSE_OUTPUTS = tuple(o[0] for o in NAVSTEER_OUTPUTS if o[2] == "pose")
NAVSTEER_SUBUNITS, NAVSTEER_TURN, NAVSTEER_NO_COST = 1024, 65536, 0xFFFFFFFF
# the oriented footprint (include/ssf_navfoot.h): exported by libssf_hip_foot.so only (load_foot)
NAVFOOT_SYMBOLS = ["ssf_navfoot_spans", "ssf_navfoot_default_params", "ssf_navfoot_layers", "ssf_navfoot_rollouts"]
NAVFOOT_MAX_REACH, NAVFOOT_ROWS, NAVFOOT_MAX_SIDE, NAVFOOT_MAX_PAD = 40, 81, 24576, 4096
NAVFOOT_HEADINGS = (1, 2, 4, 8, 16, 32)
# the plan over (x, y, heading) (include/ssf_navpose.h): exported by libssf_hip_pose.so only (load_pose)
NAVPOSE_SYMBOLS = ["ssf_navpose_moves", "ssf_navpose_default_params", "ssf_navpose_field"]
NAVPOSE_OUTPUT_NAMES = ("cost", "cell_cost", "cell_bin", "start_cost", "start_status", "path_len", "path")
NAVPOSE_UNREACHED, NAVPOSE_NO_BIN, NAVPOSE_TILE, NAVPOSE_ROUND_BATCH, NAVPOSE_MAX_STATES = 0xFFFFFFFF, 255, 16, 16, 1 << 26
# steering among movers (include/ssf_navdyn.h): exported by libssf_hip_dyn.so only (load_dyn)
NAVDYN_SYMBOLS = ["ssf_navdyn_default_params", "ssf_navdyn_rollouts", "ssf_navdyn_foot_rollouts", "ssf_navdyn_default_blob_params",
                  "ssf_navdyn_blobs"]
# the arrays of ssf_navdyn_out, as NAVSTEER_OUTPUTS
NAVDYN_OUTPUTS = (("cand_hit", np.int32, "cand", ()), ("cand_min_gap", np.int32, "cand", ()), ("best_min_gap", np.int32, "pose", ()))
NAVDYN_OUTPUT_NAMES = tuple(o[0] for o in NAVDYN_OUTPUTS)
NAVDYN_MAX_MOVERS, NAVDYN_MOVER_WORDS, NAVDYN_MAX_BLOBS, NAVDYN_BLOB_WORDS = 64, 6, 64, 8
# the bounds of a mover (x, y, vx, vy, r, grow): |x|, |y|; |vx|, |vy|; r; grow
NAVDYN_MAX_XY, NAVDYN_MAX_V, NAVDYN_MAX_R, NAVDYN_MAX_GROW = 1 << 24, 4096, 1 << 20, 4096
# rays cast through the model (include/ssf_raycast.h): exported by the HIP product only, not part of ssf.h (ABI_SYMBOLS)
RAYCAST_SYMBOLS = ["ssf_raycast_default_params", "ssf_raycast"]
# the output arrays of ssf_raycast, in its argument order: name, dtype, per-ray shape
RAYCAST_OUTPUTS = (("t", np.float32, ()), ("index", np.int32, ()), ("point", np.float32, (3,)), ("normal", np.float32, (3,)),
                   ("color", np.float32, (3,)))
RAYCAST_OUTPUT_NAMES = tuple(nm for nm, _, _ in RAYCAST_OUTPUTS)
# the track stage's test hooks and counters -- the resident ICP launch, the tile-sorted copy (include/ssf_track.h): HIP product only,
# not part of ssf.h
TRACK_SYMBOLS = ["ssf_debug_set_resident_icp_max_rows", "ssf_resident_icp_frames", "ssf_resident_icp_ahead_frames",
                 "ssf_tile_copy_frames", "ssf_debug_tile_copy"]
# the geometric moving-object detector (include/ssf_motion.h): exported by the HIP product only, not part of ssf.h (ABI_SYMBOLS)
MOTION_SYMBOLS = ["ssf_motion_default_params", "ssf_motion_segment", "ssf_motion_mask", "ssf_process_frame_motion", "ssf_get_motion_mask"]
# dense RGB-D odometry, the pose prior of the library's own (include/ssf_odometry.h): HIP product only, not part of ssf.h
ODOMETRY_SYMBOLS = ["ssf_odometry_default_params", "ssf_odometry_set_reference", "ssf_odometry_linearise", "ssf_odometry_estimate",
                    "ssf_odometry_track", "ssf_process_frame_odometry", "ssf_get_odometry"]
ODOMETRY_REASONS = ("converged", "max_iterations", "too_few_pixels", "degenerate", "motion_gate")
ODO_MAX_LEVELS, ODO_RECORD = 6, 29
MOTION_CLASSES = {"invalid": 0, "static": 1, "seed": 2, "unknown": 3}
# the images of ssf_motion_segment / ssf_motion_mask, in their argument order: name, dtype
MOTION_OUTPUTS = (("mask", np.uint8), ("label", np.int32), ("cls", np.uint8))
MOTION_OUTPUT_NAMES = tuple(nm for nm, _ in MOTION_OUTPUTS)
# the images of ssf_render_model, in its argument order: name, dtype, per-pixel shape
RENDER_OUTPUTS = (("depth", np.float32, ()), ("index", np.int32, ()), ("rgb8", np.uint8, (3,)), ("color", np.float32, (3,)),
                  ("normal", np.float32, (3,)))
RENDER_OUTPUT_NAMES = tuple(nm for nm, _, _ in RENDER_OUTPUTS)

SURFEL_FIELDS = (("positions", 3, np.float32), ("colors", 3, np.float32), ("stamps", 2, np.int32),
                 ("orientations", 9, np.float32), ("shapes", 6, np.float32),
                 ("dims", 2, np.float32), ("confidences", 1, np.float32))


class SsfError(RuntimeError):
    pass


class SsfRenderParams(C.Structure):
    """ssf_render_params (include/ssf_render.h)"""
    _fields_ = [("pose", C.c_void_p), ("width", C.c_int), ("height", C.c_int)] + \
               [(nm, C.c_float) for nm in ("fx", "fy", "cx", "cy", "z_min", "z_max", "min_conf", "splat_scale")] + \
               [("visible_only", C.c_int), ("on_device", C.c_int)]


class SsfRenderStats(C.Structure):
    """ssf_render_stats (include/ssf_render.h)"""
    _fields_ = [(nm, C.c_int64) for nm in ("fragments", "pixels_filled", "rows_shown", "list_entries")]

    def as_dict(self):
        return {nm: int(getattr(self, nm)) for nm, _ in self._fields_}


class SsfMotionParams(C.Structure):
    """ssf_motion_params (include/ssf_motion.h)"""
    _fields_ = [("pose", C.c_void_p)] + \
               [(nm, C.c_float) for nm in ("min_conf", "splat_scale", "front_abs", "front_quad", "link_abs", "link_rel")] + \
               [("min_seeds", C.c_int), ("unknown_per_seed", C.c_int), ("on_device", C.c_int)]


class SsfMotionStats(C.Structure):
    """ssf_motion_stats (include/ssf_motion.h)"""
    _fields_ = [(nm, C.c_int64) for nm in ("n_seed", "n_unknown", "n_components", "n_dynamic_components", "pixels_masked")]

    def as_dict(self):
        return {nm: int(getattr(self, nm)) for nm, _ in self._fields_}


class SsfOdometryParams(C.Structure):
    """ssf_odometry_params (include/ssf_odometry.h)"""
    _fields_ = [("levels", C.c_int), ("iters", C.c_int * ODO_MAX_LEVELS)] + \
               [(nm, C.c_float) for nm in ("r_max", "huber", "min_pixel_share", "tol_rot", "tol_trans", "max_translation", "max_rotation")]

    def as_dict(self):
        return {nm: (list(self.iters) if nm == "iters" else getattr(self, nm)) for nm, _ in self._fields_}


class SsfOdometryResult(C.Structure):
    """ssf_odometry_result (include/ssf_odometry.h)"""
    _fields_ = [("valid", C.c_int), ("reason", C.c_int), ("levels", C.c_int), ("iters", C.c_int * ODO_MAX_LEVELS), ("pixels", C.c_int64),
                ("mean_sq_residual", C.c_double)]

    def as_dict(self):
        return dict(valid=int(self.valid), reason=ODOMETRY_REASONS[self.reason], levels=int(self.levels), iters=list(self.iters),
                    pixels=int(self.pixels), mean_sq_residual=float(self.mean_sq_residual))


class SsfQueryParams(C.Structure):
    """ssf_query_params (include/ssf_query.h)"""
    _fields_ = [("min_conf", C.c_float), ("t_init_min", C.c_int32), ("t_init_max", C.c_int32), ("t_last_min", C.c_int32),
                ("t_last_max", C.c_int32), ("visible_only", C.c_int), ("region", C.c_int), ("pose", C.c_void_p),
                ("radius", C.c_float), ("half", C.c_float * 3), ("width", C.c_int), ("height", C.c_int)] + \
               [(nm, C.c_float) for nm in ("fx", "fy", "cx", "cy", "z_min", "z_max")] + [("on_device", C.c_int)]


class SsfQueryStats(C.Structure):
    """ssf_query_stats (include/ssf_query.h)"""
    _fields_ = [("n_scanned", C.c_int64), ("n_selected", C.c_int64), ("n_selected_visible", C.c_int64),
                ("lo", C.c_float * 3), ("hi", C.c_float * 3)]

    def as_dict(self):
        return dict(n_scanned=int(self.n_scanned), n_selected=int(self.n_selected), n_selected_visible=int(self.n_selected_visible),
                    lo=np.array(self.lo[:], np.float32), hi=np.array(self.hi[:], np.float32))


class SsfNavGridParams(C.Structure):
    """ssf_navgrid_params (include/ssf_navgrid.h)"""
    _fields_ = [("pose", C.c_void_p), ("width", C.c_int), ("height", C.c_int)] + \
               [(nm, C.c_float) for nm in ("res", "z_min", "z_max", "floor_max", "floor_cos", "min_conf")] + \
               [(nm, C.c_int32) for nm in ("t_init_min", "t_init_max", "t_last_min", "t_last_max")] + \
               [("visible_only", C.c_int), ("splat_scale", C.c_float)] + \
               [(nm, C.c_int) for nm in ("max_steps", "min_hits", "max_dist_cells", "unknown_is_obstacle", "on_device")]


class SsfNavGridOut(C.Structure):
    """ssf_navgrid_out (include/ssf_navgrid.h)"""
    _fields_ = [(nm, C.c_void_p) for nm in ("zmin", "zmax", "hits", "state", "dist2")]


class SsfNavGridStats(C.Structure):
    """ssf_navgrid_stats (include/ssf_navgrid.h)"""
    _fields_ = [(nm, C.c_int64) for nm in ("rows_used", "samples", "samples_in_grid", "cells_free", "cells_occupied", "cells_unknown",
                                           "list_entries")] + [("pose", C.c_float * 12)]

    def as_dict(self):
        d = {nm: int(getattr(self, nm)) for nm, _ in self._fields_ if nm != "pose"}
        d["pose"] = np.array(self.pose[:], np.float32)
        return d


class SsfNavCarveParams(C.Structure):
    """ssf_navcarve_params (include/ssf_navcarve.h)"""
    _fields_ = [("views", C.c_void_p), ("n_views", C.c_int)] + [(nm, C.c_float) for nm in ("fx", "fy", "cx", "cy")] + \
               [(nm, C.c_int) for nm in ("cam_width", "cam_height", "stride")] + \
               [(nm, C.c_float) for nm in ("t_min", "t_max", "ray_min_conf", "ray_splat_scale", "hit_margin_cells")] + \
               [("carve_misses", C.c_int), ("min_seen", C.c_int)]


class SsfNavCarveOut(C.Structure):
    """ssf_navcarve_out (include/ssf_navcarve.h)"""
    _fields_ = [("grid", SsfNavGridOut), ("seen", C.c_void_p)]


class SsfNavCarveStats(C.Structure):
    """ssf_navcarve_stats (include/ssf_navcarve.h)"""
    _fields_ = [("grid", SsfNavGridStats)] + [(nm, C.c_int64) for nm in ("rays", "rays_hit", "rays_invalid", "rays_carving", "ray_samples",
                                                                         "ray_entries", "cells_seen", "cells_carved")]

    def as_dict(self):
        d = self.grid.as_dict()
        d.update({nm: int(getattr(self, nm)) for nm, _ in self._fields_ if nm != "grid"})
        return d


class SsfNavPlanParams(C.Structure):
    """ssf_navplan_params (include/ssf_navplan.h)"""
    _fields_ = [(nm, C.c_int) for nm in ("width", "height", "min_dist2", "soft_dist2", "near_penalty", "allow_unknown")] + \
               [("goals", C.c_void_p), ("n_goals", C.c_int), ("goals_from_frontier", C.c_int), ("starts", C.c_void_p), ("n_starts", C.c_int),
                ("max_path", C.c_int), ("on_device", C.c_int)]


class SsfNavPlanOut(C.Structure):
    """ssf_navplan_out (include/ssf_navplan.h)"""
    _fields_ = [(nm, C.c_void_p) for nm in NAVPLAN_OUTPUT_NAMES]


class SsfNavPlanStats(C.Structure):
    """ssf_navplan_stats (include/ssf_navplan.h)"""
    _fields_ = [(nm, C.c_int64) for nm in ("cells_traversable", "cells_reached", "frontier_cells", "frontier_goals", "goals_used", "goals_blocked",
                                           "goals_outside", "max_cost", "rounds", "tile_visits")]

    def as_dict(self):
        return {nm: int(getattr(self, nm)) for nm, _ in self._fields_}


class SsfNavFrontierParams(C.Structure):
    """ssf_navfrontier_params (include/ssf_navfrontier.h)"""
    _fields_ = [(nm, C.c_int) for nm in ("width", "height", "connectivity", "traversable_only", "min_dist2", "min_cells", "reachable_only",
                                         "max_regions", "gain_radius", "cost_weight", "gain_weight", "size_weight", "on_device")]


class SsfNavFrontierRegion(C.Structure):
    """ssf_navfrontier_region (include/ssf_navfrontier.h); NAVFRONTIER_REGION_DTYPE is the same record for numpy"""
    _fields_ = [("sum_x", C.c_int64), ("sum_y", C.c_int64)] + \
               [(nm, C.c_int32) for nm in ("label", "cells", "x0", "y0", "x1", "y1", "rep_x", "rep_y")] + [("rep_cost", C.c_uint32), ("gain", C.c_int32)]


class SsfNavFrontierOut(C.Structure):
    """ssf_navfrontier_out (include/ssf_navfrontier.h)"""
    _fields_ = [("region", C.c_void_p), ("regions", C.c_void_p), ("order", C.c_void_p)]


class SsfNavFrontierStats(C.Structure):
    """ssf_navfrontier_stats (include/ssf_navfrontier.h)"""
    _fields_ = [(nm, C.c_int64) for nm in ("frontier_cells", "regions_found", "regions_small", "regions_unreached", "regions_kept",
                                           "regions_written", "largest_cells", "gain_rays", "merge_pairs")]

    def as_dict(self):
        return {nm: int(getattr(self, nm)) for nm, _ in self._fields_}


class SsfNavPathParams(C.Structure):
    """ssf_navpath_params (include/ssf_navpath.h)"""
    _fields_ = [(nm, C.c_int) for nm in ("width", "height", "min_dist2", "allow_unknown", "los_dist2", "keep_clearance", "clearance_cap", "lookahead",
                                         "n_paths", "max_path", "max_waypoints", "on_device")]


class SsfNavPathOut(C.Structure):
    """ssf_navpath_out (include/ssf_navpath.h)"""
    _fields_ = [(nm, C.c_void_p) for nm in NAVPATH_OUTPUT_NAMES]


class SsfNavPathStats(C.Structure):
    """ssf_navpath_stats (include/ssf_navpath.h)"""
    _fields_ = [(nm, C.c_int64) for nm in ("paths_ok", "paths_bad", "paths_truncated", "waypoints", "forced_steps", "cells_in", "segments_tested")]

    def as_dict(self):
        return {nm: int(getattr(self, nm)) for nm, _ in self._fields_}


class SsfNavLiveParams(C.Structure):
    """ssf_navlive_params (include/ssf_navlive.h)"""
    _fields_ = [("grid_pose", C.c_void_p), ("width", C.c_int), ("height", C.c_int), ("res", C.c_float), ("floor_max", C.c_float),
                ("z_max", C.c_float), ("max_dist_cells", C.c_int), ("unknown_is_obstacle", C.c_int), ("cam_pose", C.c_void_p),
                ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("cam_width", C.c_int), ("cam_height", C.c_int),
                ("t_min", C.c_float), ("t_max", C.c_float), ("mask_mode", C.c_int), ("min_hits", C.c_int), ("stride", C.c_int),
                ("hit_margin_cells", C.c_float), ("min_seen", C.c_int), ("open_unknown", C.c_int), ("on_device", C.c_int),
                ("frame_on_device", C.c_int)]


class SsfNavLiveOut(C.Structure):
    """ssf_navlive_out (include/ssf_navlive.h)"""
    _fields_ = [(nm, C.c_void_p) for nm in NAVLIVE_OUTPUT_NAMES]


class SsfNavLiveStats(C.Structure):
    """ssf_navlive_stats (include/ssf_navlive.h)"""
    _fields_ = [(nm, C.c_int64) for nm in ("pixels_valid", "pixels_stamping", "points_in_band", "rays", "rays_carving", "ray_samples",
                                           "ray_entries", "cells_stamped", "cells_opened", "cells_free", "cells_occupied", "cells_unknown",
                                           "atomics")] + [("pose", C.c_float * 12)]

    def as_dict(self):
        d = {nm: int(getattr(self, nm)) for nm, _ in self._fields_ if nm != "pose"}
        d["pose"] = np.array(self.pose, np.float32)
        return d


class SsfNavMemParams(C.Structure):
    """ssf_navmem_params (include/ssf_navmem.h)"""
    _fields_ = [("grid_pose", C.c_void_p), ("width", C.c_int), ("height", C.c_int), ("res", C.c_float), ("floor_max", C.c_float),
                ("z_max", C.c_float), ("max_dist_cells", C.c_int), ("unknown_is_obstacle", C.c_int), ("cam_pose", C.c_void_p),
                ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("cam_width", C.c_int), ("cam_height", C.c_int),
                ("t_min", C.c_float), ("t_max", C.c_float), ("mask_mode", C.c_int), ("min_hits", C.c_int), ("stride", C.c_int),
                ("hit_margin_cells", C.c_float), ("open_unknown", C.c_int), ("slices", C.c_int), ("tick", C.c_uint32),
                ("max_mark_age", C.c_uint32), ("max_seen_age", C.c_uint32), ("on_device", C.c_int),
                ("frame_on_device", C.c_int)]


class SsfNavMemLayer(C.Structure):
    """ssf_navmem_layer (include/ssf_navmem.h)"""
    _fields_ = [(nm, C.c_void_p) for nm in NAVMEM_LAYER_NAMES]


class SsfNavMemOut(C.Structure):
    """ssf_navmem_out (include/ssf_navmem.h)"""
    _fields_ = [(nm, C.c_void_p) for nm in NAVMEM_OUTPUT_NAMES]


class SsfNavMemStats(C.Structure):
    """ssf_navmem_stats (include/ssf_navmem.h)"""
    _fields_ = [(nm, C.c_int64) for nm in ("pixels_valid", "pixels_stamping", "points_in_band", "rays", "rays_carving", "ray_samples",
                                           "cells_marked", "cells_newly_marked", "cells_cleared", "cells_expired", "bits_cleared",
                                           "cells_remembered", "cells_opened", "cells_free", "cells_occupied", "cells_unknown",
                                           "atomics")] + [("pose", C.c_float * 12)]

    def as_dict(self):
        d = {nm: int(getattr(self, nm)) for nm, _ in self._fields_ if nm != "pose"}
        d["pose"] = np.array(self.pose, np.float32)
        return d


class SsfNavFloorParams(C.Structure):
    """ssf_navfloor_params (include/ssf_navfloor.h)"""
    _fields_ = [("origin", C.c_void_p), ("up", C.c_float * 3), ("tilt_cos", C.c_float), ("align_cos", C.c_float), ("height_res", C.c_float),
                ("min_rows", C.c_int), ("floor_share256", C.c_int), ("refine_iters", C.c_int), ("first_dist", C.c_float), ("inlier_dist", C.c_float),
                ("min_conf", C.c_float), ("t_init_min", C.c_int32), ("t_init_max", C.c_int32), ("t_last_min", C.c_int32), ("t_last_max", C.c_int32),
                ("visible_only", C.c_int), ("width", C.c_int), ("height", C.c_int), ("res", C.c_float), ("below", C.c_float), ("step", C.c_float),
                ("body_height", C.c_float)]


class SsfNavFloorOut(C.Structure):
    """ssf_navfloor_out (include/ssf_navfloor.h)"""
    _fields_ = [("dir_hist", C.c_void_p), ("height_hist", C.c_void_p)]


class SsfNavFloorFitResult(C.Structure):
    """ssf_navfloor_fit_result (include/ssf_navfloor.h)"""
    _fields_ = [("status", C.c_int), ("rounds", C.c_int), ("normal", C.c_float * 3), ("d", C.c_float), ("origin", C.c_float * 3),
                ("camera_height", C.c_float), ("rows_used", C.c_int64), ("candidates", C.c_int64), ("direction_rows", C.c_int64),
                ("aligned", C.c_int64), ("height_out_of_range", C.c_int64), ("height_rows", C.c_int64), ("dir_bin", C.c_int * 2),
                ("height_bin", C.c_int), ("reserved", C.c_int), ("inliers", C.c_int64 * 8), ("rms", C.c_float * 8), ("sums", (C.c_int64 * 10) * 8),
                ("pose", C.c_float * 12), ("z_min", C.c_float), ("floor_max", C.c_float), ("z_max", C.c_float), ("width", C.c_int),
                ("height", C.c_int), ("res", C.c_float)]

    def as_dict(self):
        d = {nm: int(getattr(self, nm)) for nm in ("status", "rounds", "rows_used", "candidates", "direction_rows", "aligned", "height_out_of_range",
                                                   "height_rows", "height_bin", "width", "height")}
        for nm in ("d", "camera_height", "z_min", "floor_max", "z_max", "res"):
            d[nm] = np.float32(getattr(self, nm))
        for nm in ("normal", "origin", "rms", "pose"):
            d[nm] = np.array(getattr(self, nm), np.float32)
        d["dir_bin"] = (int(self.dir_bin[0]), int(self.dir_bin[1]))
        d["inliers"] = [int(v) for v in self.inliers]
        d["sums"] = np.array([[int(v) for v in row] for row in self.sums], np.int64)
        d["status_name"] = NAVFLOOR_STATUS[self.status]
        return d


class SsfNavSteerParams(C.Structure):
    """ssf_navsteer_params (include/ssf_navsteer.h)"""
    _fields_ = [(nm, C.c_int) for nm in ("width", "height", "min_dist2", "allow_unknown", "clearance_cap", "n_poses", "n_v", "n_w", "v_min", "v_step",
                                         "w_min", "w_step", "n_steps", "min_free_steps", "brake_div", "cost_weight", "target_weight", "clear_weight",
                                         "speed_weight", "turn_weight", "walk", "on_device")]


class SsfNavSteerOut(C.Structure):
    """ssf_navsteer_out (include/ssf_navsteer.h)"""
    _fields_ = [(nm, C.c_void_p) for nm in NAVSTEER_OUTPUT_NAMES]


class SsfNavSteerStats(C.Structure):
    """ssf_navsteer_stats (include/ssf_navsteer.h)"""
    _fields_ = [(nm, C.c_int64) for nm in ("poses_ok", "poses_blocked", "poses_stuck", "candidates", "admissible", "collided", "steps_taken",
                                           "windows_staged", "windows_global")]

    def as_dict(self):
        return {nm: int(getattr(self, nm)) for nm, _ in self._fields_}


class SsfNavDynParams(C.Structure):
    """ssf_navdyn_params (include/ssf_navdyn.h)"""
    _fields_ = [(nm, C.c_int) for nm in ("n_movers", "mover_cap", "mover_weight")]


class SsfNavDynOut(C.Structure):
    """ssf_navdyn_out (include/ssf_navdyn.h)"""
    _fields_ = [(nm, C.c_void_p) for nm in NAVDYN_OUTPUT_NAMES]


class SsfNavDynStats(C.Structure):
    """ssf_navdyn_stats (include/ssf_navdyn.h)"""
    _fields_ = [("hit_movers", C.c_int64)]

    def as_dict(self):
        return {nm: int(getattr(self, nm)) for nm, _ in self._fields_}


class SsfNavDynBlobParams(C.Structure):
    """ssf_navdyn_blob_params (include/ssf_navdyn.h)"""
    _fields_ = [("grid_pose", C.c_void_p), ("width", C.c_int), ("height", C.c_int), ("res", C.c_float), ("floor_max", C.c_float),
                ("z_max", C.c_float), ("cam_pose", C.c_void_p), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("cam_width", C.c_int), ("cam_height", C.c_int), ("t_min", C.c_float), ("t_max", C.c_float), ("min_points", C.c_int),
                ("max_blobs", C.c_int), ("direct", C.c_int), ("on_device", C.c_int), ("frame_on_device", C.c_int)]


class SsfNavDynBlobStats(C.Structure):
    """ssf_navdyn_blob_stats (include/ssf_navdyn.h)"""
    _fields_ = [(nm, C.c_int64) for nm in ("pixels_member", "pixels_valid", "points_in_band", "labels_seen", "blobs_kept", "blobs_written")]

    def as_dict(self):
        return {nm: int(getattr(self, nm)) for nm, _ in self._fields_}


class SsfNavPoseParams(C.Structure):
    """ssf_navpose_params (include/ssf_navpose.h)"""
    _fields_ = [(nm, C.c_int) for nm in ("width", "height", "n_headings", "min_dist2", "soft_dist2", "near_penalty", "move_tol", "allow_reverse",
                                         "reverse_cost", "turn_cost")] + \
               [("goals", C.c_void_p), ("n_goals", C.c_int), ("starts", C.c_void_p), ("n_starts", C.c_int), ("max_path", C.c_int), ("on_device", C.c_int)]


class SsfNavPoseOut(C.Structure):
    """ssf_navpose_out (include/ssf_navpose.h)"""
    _fields_ = [(nm, C.c_void_p) for nm in NAVPOSE_OUTPUT_NAMES]


class SsfNavPoseStats(C.Structure):
    """ssf_navpose_stats (include/ssf_navpose.h)"""
    _fields_ = [(nm, C.c_int64) for nm in ("states_traversable", "states_reached", "cells_reached", "goals_used", "goals_blocked", "goals_outside",
                                           "max_cost", "rounds", "tile_visits")]

    def as_dict(self):
        return {nm: int(getattr(self, nm)) for nm, _ in self._fields_}


class SsfNavFootParams(C.Structure):
    """ssf_navfoot_params (include/ssf_navfoot.h)"""
    _fields_ = [(nm, C.c_int) for nm in ("width", "height", "allow_unknown", "n_headings", "front", "back", "left", "right", "pad", "on_device")]


class SsfNavFootOut(C.Structure):
    """ssf_navfoot_out (include/ssf_navfoot.h)"""
    _fields_ = [("free_mask", C.c_void_p), ("n_free", C.c_void_p)]


class SsfNavFootStats(C.Structure):
    """ssf_navfoot_stats (include/ssf_navfoot.h)"""
    _fields_ = [(nm, C.c_int64) for nm in ("cells_clear", "cells_all", "cells_some", "cells_none", "reach", "kernel_cells")]

    def as_dict(self):
        return {nm: int(getattr(self, nm)) for nm, _ in self._fields_}


class SsfRaycastParams(C.Structure):
    """ssf_raycast_params (include/ssf_raycast.h)"""
    _fields_ = [("pose", C.c_void_p), ("t_min", C.c_float), ("t_max", C.c_float), ("min_conf", C.c_float), ("splat_scale", C.c_float),
                ("visible_only", C.c_int), ("on_device", C.c_int), ("cell", C.c_float), ("hash_bits", C.c_int)]


class SsfRaycastStats(C.Structure):
    """ssf_raycast_stats (include/ssf_raycast.h)"""
    _fields_ = [(nm, C.c_int64) for nm in ("rays", "rays_hit", "rays_invalid", "rows_indexed", "rows_oversize", "index_entries",
                                           "cells_visited", "candidates_tested", "index_rebuilt")]

    def as_dict(self):
        return {nm: int(getattr(self, nm)) for nm, _ in self._fields_}


class SsfGraphParams(C.Structure):
    """ssf_graph_params (include/ssf_graph.h)"""
    _fields_ = [("stride", C.c_int), ("look", C.c_int), ("min_conf", C.c_float)]


GRAPH_SOLVE_MAX_OUTER = 64
GRAPH_SOLVE_ENDS = ("tolerance", "max_inner", "breakdown", "zero")


class SsfGraphSolveParams(C.Structure):
    """ssf_graph_solve_params (include/ssf_graph_solve.h)"""
    _fields_ = [(nm, C.c_double) for nm in ("w_rot", "w_reg", "w_con", "inner_tol", "outer_tol", "damping")] + \
               [(nm, C.c_int) for nm in ("max_outer", "max_inner", "inner_check")]


class SsfGraphSolveResult(C.Structure):
    """ssf_graph_solve_result (include/ssf_graph_solve.h)"""
    _fields_ = [(nm, C.c_double) for nm in ("e_before", "e_after", "e_rot", "e_reg", "e_con")] + \
               [("outer", C.c_int), ("inner_end", C.c_int), ("inner", C.c_int * GRAPH_SOLVE_MAX_OUTER)]

    def as_dict(self):
        d = {nm: getattr(self, nm) for nm in ("e_before", "e_after", "e_rot", "e_reg", "e_con", "outer", "inner_end")}
        d["inner"] = [int(v) for v in self.inner[:self.outer]]
        return d


class SsfKeyframesParams(C.Structure):
    """ssf_keyframes_params (include/ssf_keyframes.h)"""
    _fields_ = [("cell", C.c_int), ("n_ferns", C.c_int), ("seed", C.c_uint64), ("max_keyframes", C.c_int), ("min_gap", C.c_int),
                ("max_rows", C.c_int64), ("new_ratio", C.c_float), ("loop_ratio", C.c_float)]

    def as_dict(self):
        return {nm: getattr(self, nm) for nm, _ in self._fields_}


class SsfKeyframeCandidate(C.Structure):
    _fields_ = [(nm, C.c_int32) for nm in ("id", "diff", "stamp", "loop")]


class SsfKeyframeResult(C.Structure):
    """ssf_keyframe_result (include/ssf_keyframes.h)"""
    _fields_ = [(nm, C.c_int32) for nm in ("added", "id", "full", "min_diff_all", "n_keyframes", "n_candidates")] + \
               [("candidates", SsfKeyframeCandidate * KEYFRAMES_MAX_CANDIDATES)]

    def as_dict(self):
        c = [dict(id=int(e.id), diff=int(e.diff), stamp=int(e.stamp), loop=bool(e.loop)) for e in self.candidates[:self.n_candidates]]
        return dict(added=bool(self.added), id=int(self.id), full=bool(self.full), min_diff_all=int(self.min_diff_all),
                    n_keyframes=int(self.n_keyframes), candidates=c)


class Library:
    """A loaded libssf_*.so."""

    def __init__(self, path):
        if not os.path.exists(path):
            raise SsfError("shared library not found: %s (run __graft_entry__.build())" % path)
        self.path = path
        self.lib = C.CDLL(path)
        L = self.lib
        L.ssf_backend_name.restype = C.c_char_p
        L.ssf_last_error.restype = C.c_char_p
        L.ssf_last_error.argtypes = [C.c_void_p]
        L.ssf_default_config.argtypes = [C.POINTER(SsfConfig)]
        L.ssf_create.argtypes = [C.POINTER(SsfConfig), C.POINTER(C.c_void_p)]
        L.ssf_destroy.argtypes = [C.c_void_p]
        L.ssf_destroy.restype = None
        vp = C.c_void_p
        L.ssf_process_frame.argtypes = [vp, vp, vp, vp, vp, C.POINTER(SsfFrameResult)]
        L.ssf_process_frame_device.argtypes = [vp, vp, vp, vp, vp, C.POINTER(SsfFrameResult)]
        L.ssf_stage_extract.argtypes = [vp, vp, vp, C.c_int, vp]
        L.ssf_debug_set_max_passes.argtypes = [vp, C.c_int]
        L.ssf_debug_set_bin_min_rows.argtypes = [vp, C.c_int]
        L.ssf_debug_recentre.argtypes = [vp]
        L.ssf_debug_recentre_count.argtypes = [vp]
        L.ssf_debug_recentre_count.restype = C.c_longlong
        L.ssf_stage_set_shard.argtypes = [vp, C.c_int64, C.c_int64, C.c_int64]
        L.ssf_stage_icp_begin.argtypes = [vp, vp]
        L.ssf_stage_icp_accumulate.argtypes = [vp, vp]
        L.ssf_stage_icp_update.argtypes = [vp, vp, C.POINTER(C.c_int)]
        L.ssf_stage_icp_end.argtypes = [vp, C.POINTER(C.c_int)]
        L.ssf_stage_match.argtypes = [vp, vp, vp]
        L.ssf_stage_fuse.argtypes = [vp, vp, vp, C.POINTER(SsfFrameResult)]
        L.ssf_get_pose.argtypes = [vp, vp]
        L.ssf_set_pose.argtypes = [vp, vp]
        L.ssf_get_counts.argtypes = [vp] + [C.POINTER(C.c_int)] * 4
        L.ssf_get_model.argtypes = [vp, C.c_int, C.c_int, C.POINTER(SsfSurfels)]
        L.ssf_get_frame.argtypes = [vp, C.POINTER(SsfSurfels)]
        L.ssf_set_model.argtypes = [vp, C.POINTER(SsfSurfels), C.c_int, C.c_int, C.c_int]
        for nm in ("ssf_get_index_map", "ssf_get_boundary_map", "ssf_get_inlier_map",
                   "ssf_get_plane_depth", "ssf_get_superpixels", "ssf_get_preview_image"):
            getattr(L, nm).argtypes = [vp, vp]
        L.ssf_get_model_device.argtypes = [vp, C.POINTER(SsfSurfels), C.POINTER(C.c_int)]
        L.ssf_export_model_txt.argtypes = [vp, C.c_char_p]
        L.ssf_apply_deformation.argtypes = [vp, vp, vp, vp, C.c_int, vp, vp]
        L.ssf_get_kernel_times.argtypes = [vp, vp, vp, vp, C.c_int]
        L.ssf_reset_kernel_times.argtypes = [vp]
        L.ssf_set_profile.argtypes = [vp, C.c_int]
        L.ssf_bilateral_filter.argtypes = [vp, vp, vp, C.c_int]
        L.ssf_submit_frame.argtypes = [vp, vp, vp, C.c_int, vp]
        L.ssf_process_sequence.argtypes = [vp, vp, vp, C.c_int, C.c_int, vp]
        L.ssf_process_submitted.argtypes = [vp, vp, C.POINTER(SsfFrameResult)]
        L.ssf_pending_frames.argtypes = [vp]
        L.ssf_pipeline_capacity.argtypes = [vp]
        L.ssf_can_submit.argtypes = [vp]
        L.ssf_align.argtypes = [vp, C.POINTER(SsfSurfels), C.c_int, vp, vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.ssf_fern_codes.argtypes = [vp, vp, vp, C.c_int, C.c_int, vp, vp, vp, C.c_int, vp]
        L.ssf_comm_unique_id.argtypes = [vp]
        L.ssf_comm_attach.argtypes = [vp, vp]
        L.ssf_p2p_export.argtypes = [vp, vp]
        L.ssf_p2p_attach.argtypes = [vp, vp]
        L.ssf_p2p_region.argtypes = [vp, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
        L.ssf_p2p_attach_local.argtypes = [vp, C.POINTER(C.c_void_p)]
        L.ssf_p2p_configure.argtypes = [vp, C.c_int, C.c_double]
        L.ssf_rehome_begin.argtypes = [vp, vp, C.c_int, C.POINTER(C.c_int)]
        L.ssf_rehome_end.argtypes = [vp, vp, C.c_int]
        L.ssf_get_global_counts.argtypes = [vp, vp]
        L.ssf_stage_begin_submitted.argtypes = [vp]
        L.ssf_stage_icp_accumulate_device.argtypes = [vp, vp]
        L.ssf_stage_icp_fetch.argtypes = [vp, vp, vp]
        L.ssf_stage_match_device.argtypes = [vp, vp, vp]
        L.ssf_stage_fuse_device.argtypes = [vp, vp, vp, C.POINTER(SsfFrameResult)]
        L.ssf_stage_fuse_begin.argtypes = [vp, vp, vp, vp]
        L.ssf_stage_fuse_end.argtypes = [vp, vp, C.POINTER(SsfFrameResult)]
        L.ssf_stage_fuse_begin_device.argtypes = [vp, vp, vp, vp]
        L.ssf_stage_fuse_end_device.argtypes = [vp, vp, C.POINTER(SsfFrameResult)]
        self.has_input_format = all(hasattr(L, nm) for nm in INPUT_FORMAT_SYMBOLS)
        if self.has_input_format:
            L.ssf_set_input_format.argtypes = [vp, C.c_int, C.c_int, C.c_double]
            L.ssf_get_input_format.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_double)]
        self.has_dynamic_mask = all(hasattr(L, nm) for nm in DYNAMIC_MASK_SYMBOLS)
        if self.has_dynamic_mask:
            L.ssf_process_frame_pixmask.argtypes = [vp, vp, vp, C.c_int, vp, vp, C.POINTER(SsfFrameResult)]
            L.ssf_submit_frame_pixmask.argtypes = [vp, vp, vp, C.c_int, vp]
            L.ssf_process_sequence_pixmask.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int, vp]
            L.ssf_stage_extract_pixmask.argtypes = [vp, vp, vp, C.c_int, vp]
            L.ssf_get_dynamic_superpixels.argtypes = [vp, vp, C.POINTER(C.c_int)]
        self.has_render = all(hasattr(L, nm) for nm in RENDER_SYMBOLS)
        if self.has_render:
            L.ssf_render_default_params.argtypes = [vp, C.POINTER(SsfRenderParams)]
            L.ssf_render_model.argtypes = [vp, C.POINTER(SsfRenderParams), vp, vp, vp, vp, vp, C.POINTER(SsfRenderStats)]
        self.has_query = all(hasattr(L, nm) for nm in QUERY_SYMBOLS)
        if self.has_query:
            L.ssf_query_default_params.argtypes = [vp, C.POINTER(SsfQueryParams)]
            L.ssf_query_count.argtypes = [vp, C.POINTER(SsfQueryParams), C.POINTER(SsfQueryStats)]
            L.ssf_query_rows.argtypes = [vp, C.POINTER(SsfQueryParams), C.POINTER(SsfSurfels), vp, C.c_int, C.POINTER(SsfQueryStats)]
        self.has_raycast = all(hasattr(L, nm) for nm in RAYCAST_SYMBOLS)
        if self.has_raycast:
            L.ssf_raycast_default_params.argtypes = [vp, C.POINTER(SsfRaycastParams)]
            L.ssf_raycast.argtypes = [vp, C.POINTER(SsfRaycastParams), vp, C.c_int, vp, vp, vp, vp, vp, C.POINTER(SsfRaycastStats)]
        self.has_navcarve = all(hasattr(L, nm) for nm in NAVCARVE_SYMBOLS)
        if self.has_navcarve:
            L.ssf_navcarve_default_params.argtypes = [vp, C.POINTER(SsfNavCarveParams)]
            L.ssf_navgrid_carve.argtypes = [vp, C.POINTER(SsfNavGridParams), C.POINTER(SsfNavCarveParams), C.POINTER(SsfNavCarveOut),
                                            C.POINTER(SsfNavCarveStats)]
            L.ssf_debug_navcarve_set_chunk_rays.argtypes = [vp, C.c_int]
            L.ssf_debug_navcarve_last.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        self.has_navplan = all(hasattr(L, nm) for nm in NAVPLAN_SYMBOLS)
        if self.has_navplan:
            L.ssf_navplan_default_params.argtypes = [vp, C.POINTER(SsfNavPlanParams)]
            L.ssf_navplan_field.argtypes = [vp, C.POINTER(SsfNavPlanParams), vp, vp, C.POINTER(SsfNavPlanOut), C.POINTER(SsfNavPlanStats)]
            L.ssf_debug_navplan_set_round_batch.argtypes = [vp, C.c_int]
            L.ssf_debug_navplan_last.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        self.has_navfrontier = all(hasattr(L, nm) for nm in NAVFRONTIER_SYMBOLS)
        if self.has_navfrontier:
            L.ssf_navfrontier_default_params.argtypes = [vp, C.POINTER(SsfNavFrontierParams)]
            L.ssf_navfrontier_regions.argtypes = [vp, C.POINTER(SsfNavFrontierParams), vp, vp, vp, C.POINTER(SsfNavFrontierOut),
                                                  C.POINTER(SsfNavFrontierStats)]
        self.has_navpath = all(hasattr(L, nm) for nm in NAVPATH_SYMBOLS)
        if self.has_navpath:
            L.ssf_navpath_default_params.argtypes = [vp, C.POINTER(SsfNavPathParams)]
            L.ssf_navpath_waypoints.argtypes = [vp, C.POINTER(SsfNavPathParams), vp, vp, vp, vp, C.POINTER(SsfNavPathOut), C.POINTER(SsfNavPathStats)]
        self.has_navlive = all(hasattr(L, nm) for nm in NAVLIVE_SYMBOLS)
        if self.has_navlive:
            L.ssf_navlive_default_params.argtypes = [vp, C.POINTER(SsfNavLiveParams)]
            L.ssf_navlive_overlay.argtypes = [vp, C.POINTER(SsfNavLiveParams), vp, vp, vp, C.POINTER(SsfNavLiveOut), C.POINTER(SsfNavLiveStats)]
        self.has_navsteer = all(hasattr(L, nm) for nm in NAVSTEER_SYMBOLS)
        if self.has_navsteer:
            L.ssf_navsteer_default_params.argtypes = [vp, C.POINTER(SsfNavSteerParams)]
            L.ssf_navsteer_direction_table.argtypes = [vp, vp]
            L.ssf_navsteer_rollouts.argtypes = [vp, C.POINTER(SsfNavSteerParams), vp, vp, vp, vp, vp, C.POINTER(SsfNavSteerOut),
                                                C.POINTER(SsfNavSteerStats)]
        self.has_navfoot = all(hasattr(L, nm) for nm in NAVFOOT_SYMBOLS)
        if self.has_navfoot:
            L.ssf_navfoot_spans.argtypes = [C.c_int] * 6 + [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int64)]
            L.ssf_navfoot_default_params.argtypes = [vp, C.POINTER(SsfNavFootParams)]
            L.ssf_navfoot_layers.argtypes = [vp, C.POINTER(SsfNavFootParams), vp, C.POINTER(SsfNavFootOut), C.POINTER(SsfNavFootStats)]
            L.ssf_navfoot_rollouts.argtypes = [vp, C.POINTER(SsfNavSteerParams), C.c_int, vp, vp, vp, vp, vp, C.POINTER(SsfNavSteerOut),
                                               C.POINTER(SsfNavSteerStats)]
        self.has_navpose = all(hasattr(L, nm) for nm in NAVPOSE_SYMBOLS)
        if self.has_navpose:
            L.ssf_navpose_moves.argtypes = [C.c_int, C.c_int, C.c_int, vp]
            L.ssf_navpose_default_params.argtypes = [vp, C.POINTER(SsfNavPoseParams)]
            L.ssf_navpose_field.argtypes = [vp, C.POINTER(SsfNavPoseParams), vp, vp, C.POINTER(SsfNavPoseOut), C.POINTER(SsfNavPoseStats)]
        self.has_navdyn = all(hasattr(L, nm) for nm in NAVDYN_SYMBOLS)
        if self.has_navdyn:
            sp, dp = C.POINTER(SsfNavSteerParams), C.POINTER(SsfNavDynParams)
            tail = [C.POINTER(SsfNavSteerOut), C.POINTER(SsfNavDynOut), C.POINTER(SsfNavSteerStats), C.POINTER(SsfNavDynStats)]
            L.ssf_navdyn_default_params.argtypes = [vp, dp]
            L.ssf_navdyn_rollouts.argtypes = [vp, sp, dp, vp, vp, vp, vp, vp, vp] + tail
            L.ssf_navdyn_foot_rollouts.argtypes = [vp, sp, dp, C.c_int, vp, vp, vp, vp, vp, vp] + tail
            L.ssf_navdyn_default_blob_params.argtypes = [vp, C.POINTER(SsfNavDynBlobParams)]
            L.ssf_navdyn_blobs.argtypes = [vp, C.POINTER(SsfNavDynBlobParams), vp, vp, vp, vp, C.POINTER(SsfNavDynBlobStats)]
        self.has_navmem = all(hasattr(L, nm) for nm in NAVMEM_SYMBOLS)
        if self.has_navmem:
            L.ssf_navmem_default_params.argtypes = [vp, C.POINTER(SsfNavMemParams)]
            L.ssf_navmem_update.argtypes = [vp, C.POINTER(SsfNavMemParams), vp, vp, vp, C.POINTER(SsfNavMemLayer), C.POINTER(SsfNavMemOut),
                                            C.POINTER(SsfNavMemStats)]
        self.has_navfloor = all(hasattr(L, nm) for nm in NAVFLOOR_SYMBOLS)
        if self.has_navfloor:
            L.ssf_navfloor_default_params.argtypes = [vp, C.POINTER(SsfNavFloorParams)]
            L.ssf_navfloor_fit.argtypes = [vp, C.POINTER(SsfNavFloorParams), C.POINTER(SsfNavFloorOut), C.POINTER(SsfNavFloorFitResult)]
        self.has_navgrid = all(hasattr(L, nm) for nm in NAVGRID_SYMBOLS)
        if self.has_navgrid:
            L.ssf_navgrid_default_params.argtypes = [vp, C.POINTER(SsfNavGridParams)]
            L.ssf_navgrid_default_pose.argtypes = [vp, C.POINTER(SsfNavGridParams), vp]
            L.ssf_navgrid_build.argtypes = [vp, C.POINTER(SsfNavGridParams), C.POINTER(SsfNavGridOut), C.POINTER(SsfNavGridStats)]
        self.has_track = all(hasattr(L, nm) for nm in TRACK_SYMBOLS)
        if self.has_track:
            L.ssf_debug_set_resident_icp_max_rows.argtypes = [vp, C.c_int]
            L.ssf_resident_icp_frames.argtypes = [vp]
            L.ssf_resident_icp_frames.restype = C.c_longlong
            L.ssf_resident_icp_ahead_frames.argtypes = [vp]
            L.ssf_resident_icp_ahead_frames.restype = C.c_longlong
            L.ssf_tile_copy_frames.argtypes = [vp]
            L.ssf_tile_copy_frames.restype = C.c_longlong
            L.ssf_debug_tile_copy.argtypes = [vp, vp, vp, vp, vp]
        self.has_motion = all(hasattr(L, nm) for nm in MOTION_SYMBOLS)
        if self.has_motion:
            mp, ms = C.POINTER(SsfMotionParams), C.POINTER(SsfMotionStats)
            L.ssf_motion_default_params.argtypes = [vp, mp]
            L.ssf_motion_segment.argtypes = [vp, mp, vp, vp, vp, vp, vp, ms]
            L.ssf_motion_mask.argtypes = [vp, mp, vp, vp, vp, vp, vp, ms]
            L.ssf_process_frame_motion.argtypes = [vp, vp, vp, C.c_int, vp, mp, C.POINTER(SsfFrameResult)]
            L.ssf_get_motion_mask.argtypes = [vp, vp, ms]
        self.has_odometry = all(hasattr(L, nm) for nm in ODOMETRY_SYMBOLS)
        if self.has_odometry:
            op, orr = C.POINTER(SsfOdometryParams), C.POINTER(SsfOdometryResult)
            L.ssf_odometry_default_params.argtypes = [vp, op]
            L.ssf_odometry_set_reference.argtypes = [vp, vp, vp, C.c_int, vp]
            L.ssf_odometry_linearise.argtypes = [vp, op, C.c_int, vp, vp]
            L.ssf_odometry_estimate.argtypes = [vp, op, vp, vp, C.c_int, vp, vp, orr]
            L.ssf_odometry_track.argtypes = [vp, op, vp, vp, C.c_int, vp, orr]
            L.ssf_process_frame_odometry.argtypes = [vp, vp, vp, C.c_int, op, C.POINTER(SsfMotionParams), C.POINTER(SsfFrameResult)]
            L.ssf_get_odometry.argtypes = [vp, vp, vp, orr]
            L.ssf_odometry_get_pyramid.argtypes = [vp, C.c_int, C.c_int, vp, vp, vp, vp, C.POINTER(C.c_int), C.POINTER(C.c_int), vp]
        self.has_graph = all(hasattr(L, nm) for nm in GRAPH_SYMBOLS)
        if self.has_graph:
            ip = C.POINTER(C.c_int)
            L.ssf_graph_default_params.argtypes = [C.POINTER(SsfGraphParams)]
            L.ssf_graph_build.argtypes = [vp, C.POINTER(SsfGraphParams), ip]
            L.ssf_graph_get_nodes.argtypes = [vp, vp, vp, vp, C.c_int]
            L.ssf_graph_get_binding.argtypes = [vp, vp, vp, C.c_int]
            L.ssf_graph_bind_points.argtypes = [vp, vp, vp, C.c_int, vp, vp]
            L.ssf_graph_apply.argtypes = [vp, vp, vp]
            L.ssf_graph_info.argtypes = [vp, ip, ip, ip]
        self.has_graph_solve = all(hasattr(L, nm) for nm in GRAPH_SOLVE_SYMBOLS)
        if self.has_graph_solve:
            L.ssf_graph_solve_default_params.argtypes = [C.POINTER(SsfGraphSolveParams)]
            L.ssf_graph_get_edges.argtypes = [vp, vp, C.c_int]
            L.ssf_graph_solve.argtypes = [vp, C.POINTER(SsfGraphSolveParams), vp, vp, vp, C.c_int, C.POINTER(SsfGraphSolveResult)]
            L.ssf_graph_get_transforms.argtypes = [vp, vp, vp, C.c_int]
            L.ssf_graph_apply_solved.argtypes = [vp]
        self.has_keyframes = all(hasattr(L, nm) for nm in KEYFRAME_SYMBOLS)
        if self.has_keyframes:
            ip, kp, kr = C.POINTER(C.c_int), C.POINTER(SsfKeyframesParams), C.POINTER(SsfKeyframeResult)
            L.ssf_keyframes_default_params.argtypes = [kp]
            L.ssf_keyframes_configure.argtypes = [vp, kp]
            L.ssf_keyframes_set_ferns.argtypes = [vp, vp, C.c_int]
            L.ssf_keyframes_get_ferns.argtypes = [vp, vp, C.c_int]
            L.ssf_keyframes_encode.argtypes = [vp, vp, C.c_int]
            L.ssf_keyframes_query.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, kr]
            L.ssf_keyframes_add.argtypes = [vp, ip]
            L.ssf_keyframes_consider.argtypes = [vp, kr]
            L.ssf_keyframes_put.argtypes = [vp, vp, C.POINTER(SsfSurfels), C.c_int, vp, C.c_int, ip]
            L.ssf_keyframes_get.argtypes = [vp, C.c_int, C.POINTER(SsfSurfels), C.c_int, ip, vp, ip, vp]
            L.ssf_keyframes_set_pose.argtypes = [vp, C.c_int, vp]
            L.ssf_keyframes_align.argtypes = [vp, C.c_int, vp, C.c_int, vp, ip, ip, ip]
            L.ssf_keyframes_info.argtypes = [vp, ip, ip, C.POINTER(C.c_int64), kp]
            L.ssf_keyframes_clear.argtypes = [vp]

    @property
    def backend(self):
        return self.lib.ssf_backend_name().decode()

    def default_config(self, **kw):
        cfg = SsfConfig()
        self.lib.ssf_default_config(C.byref(cfg))
        for k, v in kw.items():
            if not hasattr(cfg, k):
                raise AttributeError("ssf_config has no field %r" % k)
            setattr(cfg, k, v)
        return cfg


def load_product():
    """Load the HIP product library.  Fails loudly when it has not been built; there is no
    CPU fallback.  torch is imported first so that exactly one HIP runtime (the one torch
    ships, SONAME libamdhip64.so.7) lives in the process."""
    import torch  # noqa: F401  (loads libamdhip64 before our library resolves it)
    # SSF_PRODUCT_VARIANT=<tag>: a differently compiled build of the SAME sources next to the product (csrc/variants/<tag>/):
    # `lab` = -DSSF_EXPERIMENTS, the environment switches and measurement arms behind DESIGN.md's A/B tables (built by
    # csrc/Makefile; the product itself reads no environment variable); others by tools/build_variant.sh
    tag = os.environ.get("SSF_PRODUCT_VARIANT")
    return Library(os.path.join(_HERE, "csrc", "variants", tag, "libssf_hip.so") if tag else PRODUCT_LIB)


def load_navcarve():
    """Load libssf_hip_navcarve.so: the product's objects with the carve of the navigation grid linked in (include/ssf_navcarve.h).
    A handle belongs to the library that created it: create the Fusion from THIS library to call nav_grid_carve on it.  Fails
    loudly when it has not been built."""
    import torch  # noqa: F401  (loads libamdhip64 before our library resolves it)
    return Library(NAVCARVE_LIB)


def load_nav():
    """Load libssf_hip_nav.so: the product's objects with the carve and the plan on the navigation grid linked in
    (include/ssf_navcarve.h, include/ssf_navplan.h).  A handle belongs to the library that created it: create the Fusion from THIS
    library to call nav_plan on it.  Fails loudly when it has not been built."""
    import torch  # noqa: F401  (loads libamdhip64 before our library resolves it)
    return Library(NAV_LIB)


def load_explore():
    """Load libssf_hip_explore.so: nav's objects (the product, the carve, the plan) with the frontier regions linked in
    (include/ssf_navfrontier.h).  A handle belongs to the library that created it: create the Fusion from THIS library to call
    nav_frontiers or nav_explore on it.  Fails loudly when it has not been built."""
    import torch  # noqa: F401  (loads libamdhip64 before our library resolves it)
    return Library(EXPLORE_LIB)


def load_drive():
    """Load libssf_hip_drive.so: explore's objects (the product, the carve, the plan, the frontier regions) with the waypoints linked
    in (include/ssf_navpath.h).  A handle belongs to the library that created it: create the Fusion from THIS library to call
    nav_waypoints or nav_plan_waypoints on it.  Fails loudly when it has not been built."""
    import torch  # noqa: F401  (loads libamdhip64 before our library resolves it)
    return Library(DRIVE_LIB)


def load_live():
    """Load libssf_hip_live.so: drive's objects (the product, the carve, the plan, the frontier regions, the waypoints) with the live
    obstacle layer linked in (include/ssf_navlive.h).  A handle belongs to the library that created it: create the Fusion from THIS
    library to call nav_live or nav_live_plan on it.  Fails loudly when it has not been built."""
    import torch  # noqa: F401  (loads libamdhip64 before our library resolves it)
    return Library(LIVE_LIB)


def load_steer():
    """Load libssf_hip_steer.so: live's objects (the product, the carve, the plan, the frontier regions, the waypoints, the live
    obstacle layer) with the velocity commands linked in (include/ssf_navsteer.h).  A handle belongs to the library that created it:
    create the Fusion from THIS library to call nav_steer or nav_live_steer on it.  Fails loudly when it has not been built."""
    import torch  # noqa: F401  (loads libamdhip64 before our library resolves it)
    return Library(STEER_LIB)


def navsteer_direction_table(library=None):
    """(C, S): the 1024-entry direction table of include/ssf_navsteer.h step 1, int32 each, as ssf_navsteer_direction_table returns it.
    It takes no handle and touches no device.  library: a Library that exports it (default: load_steer())."""
    lib = library or load_steer()
    if not lib.has_navsteer:
        raise SsfError("%s does not export ssf_navsteer_direction_table: it steers nothing (include/ssf_navsteer.h: libssf_hip_steer.so, "
                       "binding.load_steer)" % lib.path)
    c, s = np.zeros(1024, np.int32), np.zeros(1024, np.int32)
    rc = lib.lib.ssf_navsteer_direction_table(_ptr(c), _ptr(s))
    if rc != 0:
        raise SsfError("ssf_navsteer_direction_table failed (%d)" % rc)
    return c, s


def load_foot():
    """Load libssf_hip_foot.so: steer's objects (the product and every navigation call up to the velocity commands) with the oriented
    footprint linked in (include/ssf_navfoot.h).  A handle belongs to the library that created it: create the Fusion from THIS
    library to call nav_foot, nav_foot_steer or nav_live_foot_steer on it.  Fails loudly when it has not been built."""
    import torch  # noqa: F401  (loads libamdhip64 before our library resolves it)
    return Library(FOOT_LIB)


def navfoot_spans(front, back, left, right, pad, n_headings, library=None):
    """(spans, reach, kernel_cells): the cells a rectangular footprint covers at every heading bin (include/ssf_navfoot.h step 1), as
    ssf_navfoot_spans returns them: spans n_headings x 81 x 2 int16, (lo, hi) of the covered dx for dy = -40..40, (1, 0) where empty.
    front, back, left, right and pad in sub-units.  It takes no handle and touches no device.  library: a Library that exports it
    (default: load_foot())."""
    lib = library or load_foot()
    if not lib.has_navfoot:
        raise SsfError("%s does not export ssf_navfoot_spans: it holds no footprint (include/ssf_navfoot.h: libssf_hip_foot.so, "
                       "binding.load_foot)" % lib.path)
    B = int(n_headings)
    spans = np.zeros((B if B in NAVFOOT_HEADINGS else 1, NAVFOOT_ROWS, 2), np.int16)
    reach, cells = C.c_int32(0), C.c_int64(0)
    rc = lib.lib.ssf_navfoot_spans(int(front), int(back), int(left), int(right), int(pad), B, _ptr(spans), C.byref(reach), C.byref(cells))
    if rc != 0:
        raise SsfError("ssf_navfoot_spans refused the footprint (%d): sides 0..%d, pad 0..%d, n_headings one of %s, reach <= %d cells"
                       % (rc, NAVFOOT_MAX_SIDE, NAVFOOT_MAX_PAD, NAVFOOT_HEADINGS, NAVFOOT_MAX_REACH))
    return spans, int(reach.value), int(cells.value)


def load_pose():
    """Load libssf_hip_pose.so: foot's objects (the product and every navigation call up to the oriented footprint) with the plan over
    (x, y, heading) linked in (include/ssf_navpose.h).  A handle belongs to the library that created it: create the Fusion from THIS
    library to call nav_pose_plan or nav_live_pose_steer on it.  Fails loudly when it has not been built."""
    import torch  # noqa: F401  (loads libamdhip64 before our library resolves it)
    return Library(POSE_LIB)


def navpose_moves(n_headings, move_tol, allow_reverse, library=None):
    """The move table of include/ssf_navpose.h step 5 as ssf_navpose_moves returns it: n_headings x 8 int8, 0 = not a move of the bin,
    1 = forward, 2 = reverse.  It takes no handle and touches no device.  library: a Library that exports it (default: load_pose())."""
    lib = library or load_pose()
    if not lib.has_navpose:
        raise SsfError("%s does not export ssf_navpose_moves: it plans over no headings (include/ssf_navpose.h: libssf_hip_pose.so, "
                       "binding.load_pose)" % lib.path)
    B = int(n_headings)
    out = np.zeros((B if B in NAVFOOT_HEADINGS else 1, 8), np.int8)
    rc = lib.lib.ssf_navpose_moves(B, int(move_tol), int(allow_reverse), _ptr(out))
    if rc != 0:
        raise SsfError("ssf_navpose_moves refused its arguments (%d): n_headings one of %s, move_tol 0..256, allow_reverse 0 or 1"
                       % (rc, NAVFOOT_HEADINGS))
    return out


def load_dyn():
    """Load libssf_hip_dyn.so: pose's objects (the product and every navigation call up to the plan over headings) with steering among
    movers linked in (include/ssf_navdyn.h).  A handle belongs to the library that created it: create the Fusion from THIS library to
    call nav_dyn_steer, nav_dyn_blobs or nav_live_dyn_steer on it.  Fails loudly when it has not been built."""
    import torch  # noqa: F401  (loads libamdhip64 before our library resolves it)
    return Library(DYN_LIB)


def load_mem():
    """Load libssf_hip_mem.so: dyn's objects (the product and every navigation call up to steering among movers) with the live layer
    with memory linked in (include/ssf_navmem.h).  A handle belongs to the library that created it: create the Fusion from THIS library
    to call nav_memory, nav_memory_plan or nav_memory_dyn_steer on it.  Fails loudly when it has not been built."""
    import torch  # noqa: F401  (loads libamdhip64 before our library resolves it)
    return Library(MEM_LIB)


def load_floor():
    """Load libssf_hip_floor.so: mem's objects (the product and every navigation call up to the live layer with memory) with the fitted
    floor plane linked in (include/ssf_navfloor.h).  A handle belongs to the library that created it: create the Fusion from THIS
    library to call nav_floor or nav_floor_grid on it.  Fails loudly when it has not been built."""
    import torch  # noqa: F401  (loads libamdhip64 before our library resolves it)
    return Library(FLOOR_LIB)


class LiveMemory:
    """The caller's memory of the live layer (include/ssf_navmem.h): marks, mark_tick and seen_tick, each height x width uint32, as
    numpy arrays (device=False) or torch tensors on the device, and the tick of the last update (0: none yet).  The handle keeps
    nothing of it: Fusion.nav_memory and its siblings read it, write it back in place and advance the tick."""

    def __init__(self, width, height, device=False):
        self.width, self.height, self.device = int(width), int(height), bool(device)
        if self.width < 1 or self.height < 1:
            raise SsfError("LiveMemory needs width and height >= 1, got %d x %d" % (self.width, self.height))
        if self.device:
            import torch
            zeros = lambda: torch.zeros((self.height, self.width), dtype=torch.int32, device=torch.device("cuda"))      # (u32 words)
        else:
            zeros = lambda: np.zeros((self.height, self.width), np.uint32)
        self.marks, self.mark_tick, self.seen_tick = zeros(), zeros(), zeros()
        self.tick = 0

    def clear(self):
        """forget everything: the three arrays to zero in place, the tick to 0"""
        for a in self.arrays():
            if self.device:
                a.zero_()
            else:
                a[...] = 0
        self.tick = 0

    def arrays(self):
        return (self.marks, self.mark_tick, self.seen_tick)

    def numpy(self):
        """dict of the three arrays as uint32 numpy arrays (copies of device tensors)"""
        if self.device:
            return {nm: a.cpu().numpy().view(np.uint32) for nm, a in zip(NAVMEM_LAYER_NAMES, self.arrays())}
        return {nm: a.copy() for nm, a in zip(NAVMEM_LAYER_NAMES, self.arrays())}

    def next_tick(self, tick=None):
        """the tick of the next update: the caller's (it must not be 0), or the last one + 1 (modulo 2^32, skipping 0)"""
        if tick is None:
            tick = (self.tick + 1) & 0xFFFFFFFF or 1
        tick = int(tick)
        if not 1 <= tick <= 0xFFFFFFFF:
            raise SsfError("a tick is 1 .. 2^32 - 1, got %d" % tick)
        return tick


class MoverTracker:
    """From two successive blob tables (nav_dyn_blobs) to the movers of nav_dyn_steer: host only, integer only, the rule of
    include/ssf_navdyn.h part C (ssf.hpp's supersurfel_fusion::MoverTracker states the same).  gate: the largest centre distance of a match,
    sub-units; inflate: added to every radius (the robot's own radius goes here); grow: the growth of a matched mover, sub-units per
    step; grow_unmatched: that of a blob with no predecessor, whose velocity is unknown and taken as 0."""

    def __init__(self, gate=2048, inflate=0, grow=16, grow_unmatched=128):
        self.gate, self.inflate, self.grow, self.grow_unmatched = int(gate), int(inflate), int(grow), int(grow_unmatched)
        self.prev = np.zeros((0, NAVDYN_BLOB_WORDS), np.int32)

    def reset(self):
        self.prev = np.zeros((0, NAVDYN_BLOB_WORDS), np.int32)

    def update(self, blobs, steps_since=1):
        """blobs: n x 8 int32 rows (label, n, cx, cy, r, ex, ey, 0), n <= 64; steps_since >= 1: the rollout steps between the previous
        table and this one.  Returns n x 6 int32 (x, y, vx, vy, r, grow), every field clamped to the call's bounds."""
        blobs = np.ascontiguousarray(blobs, np.int32).reshape(-1, NAVDYN_BLOB_WORDS)
        steps = int(steps_since)
        if steps < 1 or blobs.shape[0] > NAVDYN_MAX_BLOBS:
            raise SsfError("MoverTracker.update takes at most %d blobs and steps_since >= 1" % NAVDYN_MAX_BLOBS)
        clamp = lambda v, lo, hi: lo if v < lo else (hi if v > hi else v)
        used = [False] * self.prev.shape[0]
        out = np.zeros((blobs.shape[0], NAVDYN_MOVER_WORDS), np.int32)
        for i in range(blobs.shape[0]):
            cx, cy, r = int(blobs[i, 2]), int(blobs[i, 3]), int(blobs[i, 4])
            best = None
            for j in range(self.prev.shape[0]):
                if used[j]:
                    continue
                d2 = (cx - int(self.prev[j, 2])) ** 2 + (cy - int(self.prev[j, 3])) ** 2
                if d2 <= self.gate * self.gate and (best is None or d2 < best[0]):      # (j grows: the smaller index wins a tie)
                    best = (d2, j)
            vx = vy = 0
            grow = self.grow_unmatched
            if best is not None:
                j = best[1]
                used[j] = True
                vx, vy = (cx - int(self.prev[j, 2])) // steps, (cy - int(self.prev[j, 3])) // steps       # (floor)
                grow = self.grow
            out[i] = (clamp(cx, -NAVDYN_MAX_XY, NAVDYN_MAX_XY), clamp(cy, -NAVDYN_MAX_XY, NAVDYN_MAX_XY), clamp(vx, -NAVDYN_MAX_V, NAVDYN_MAX_V),
                      clamp(vy, -NAVDYN_MAX_V, NAVDYN_MAX_V), clamp(r + self.inflate, 0, NAVDYN_MAX_R), clamp(grow, 0, NAVDYN_MAX_GROW))
        self.prev = blobs.copy()
        return out


def load_lab():
    """The laboratory build of the product sources (csrc/variants/lab, -DSSF_EXPERIMENTS): for the tests and tools that
    exercise a measurement arm or an environment switch."""
    import torch  # noqa: F401
    return Library(os.path.join(_HERE, "csrc", "variants", "lab", "libssf_hip.so"))


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _alloc_surfels(n):
    arrs = {name: np.zeros((n, k) if k > 1 else (n,), dt) for name, k, dt in SURFEL_FIELDS}
    st = SsfSurfels(*[arrs[name].ctypes.data_as(C.c_void_p) for name, _, _ in SURFEL_FIELDS])
    return arrs, st


class Fusion:
    """Host-side mirror of supersurfel_fusion::SupersurfelFusion for the hot path."""

    def __init__(self, library, cfg):
        self.L = library
        self.cfg = cfg
        self.h = C.c_void_p()
        rc = library.lib.ssf_create(C.byref(cfg), C.byref(self.h))
        if rc != 0:
            raise SsfError("ssf_create failed (%d): %s" % (rc, library.lib.ssf_last_error(None).decode()))
        self.W, self.H = cfg.width, cfg.height
        self.S = self.counts()["n_superpixels"]
        self.color_format, self.depth_format = "rgb8", "f32"      # set_input_format
        self._held = []          # host buffers of submitted frames: they must outlive the asynchronous copy (ssf.h)

    def close(self):
        if self.h:
            self.L.lib.ssf_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc, what):
        if rc != 0:
            raise SsfError("%s failed (%d): %s" % (what, rc, self.L.lib.ssf_last_error(self.h).decode()))

    # ---- input format (include/ssf_input.h) ---------------------------------------------------
    def set_input_format(self, color="rgb8", depth="f32", depth_scale=1.0):
        """How every frame entry point reads its images from now on: colour 'rgb8' | 'bgr8' | 'rgba8' | 'bgra8' (H x W x 3 / 4
        uint8, alpha ignored), depth 'f32' (H x W float32 metres) | 'u16' (H x W uint16 counts, metres = count * depth_scale
        evaluated in double and rounded once to float32).  Not while frames are pending."""
        if not self.L.has_input_format:
            raise SsfError("%s does not export ssf_set_input_format: it reads RGB8 colour and float32 metres only" % self.L.path)
        if color not in COLOR_FORMATS or depth not in DEPTH_FORMATS:
            raise SsfError("unknown input format %r / %r (colour: %s; depth: %s)" % (color, depth, ", ".join(COLOR_FORMATS),
                                                                                   ", ".join(DEPTH_FORMATS)))
        self._ck(self.L.lib.ssf_set_input_format(self.h, COLOR_FORMATS[color][0], DEPTH_FORMATS[depth][0], float(depth_scale)),
                 "ssf_set_input_format")
        self.color_format, self.depth_format = color, depth

    def input_format(self):
        """dict(color, depth, depth_scale) as the library reports it"""
        if not self.L.has_input_format:
            raise SsfError("%s does not export ssf_get_input_format" % self.L.path)
        c, d, sc = C.c_int(), C.c_int(), C.c_double()
        self._ck(self.L.lib.ssf_get_input_format(self.h, C.byref(c), C.byref(d), C.byref(sc)), "ssf_get_input_format")
        return dict(color={v[0]: k for k, v in COLOR_FORMATS.items()}[c.value],
                    depth={v[0]: k for k, v in DEPTH_FORMATS.items()}[d.value], depth_scale=sc.value)

    def _frame(self, rgb, depth):
        """contiguous host arrays of one frame in the handle's input format.  The default format (RGB8 + float32 metres)
        converts what it is given, as it always has; any other format refuses a dtype or shape that does not match it
        (a cast would turn depth counts into 'metres')."""
        if (self.color_format, self.depth_format) == ("rgb8", "f32"):
            rgb, depth = np.ascontiguousarray(rgb, np.uint8), np.ascontiguousarray(depth, np.float32)
            assert rgb.shape == (self.H, self.W, 3) and depth.shape == (self.H, self.W)
            return rgb, depth
        return self._color_array(rgb), self._depth_array(depth)

    def _color_array(self, rgb):
        ch = COLOR_FORMATS[self.color_format][1]
        rgb = np.asarray(rgb)
        if rgb.dtype != np.uint8 or rgb.shape != (self.H, self.W, ch):
            raise SsfError("colour frame must be uint8 %dx%dx%d for input format %s, got %s %s" % (
                self.H, self.W, ch, self.color_format, rgb.dtype, rgb.shape))
        return np.ascontiguousarray(rgb)

    def _depth_array(self, depth):
        dt = np.uint16 if self.depth_format == "u16" else np.float32
        depth = np.asarray(depth)
        if depth.dtype != dt or depth.shape != (self.H, self.W):
            raise SsfError("depth frame must be %s %dx%d for input format %s, got %s %s" % (
                np.dtype(dt).name, self.H, self.W, self.depth_format, depth.dtype, depth.shape))
        return np.ascontiguousarray(depth)

    # ---- pixel masks (include/ssf_dynamic.h) --------------------------------------------------
    def _need_pixmask(self, symbol):
        if not self.L.has_dynamic_mask:
            raise SsfError("%s does not export %s: it takes no pixel masks (include/ssf_dynamic.h)" % (self.L.path, symbol))

    def _pixel_mask(self, pixel_mask, on_device=False):
        """the ctypes argument of a pixel mask: None, a device address (int) when on_device, else an H x W uint8 host array
        (bool is taken as is: one byte per pixel).  Anything else is refused, not cast."""
        if pixel_mask is None:
            return None, None
        if on_device:
            if not isinstance(pixel_mask, (int, np.integer)):
                raise SsfError("a device pixel mask is a device address (int), got %s" % type(pixel_mask).__name__)
            return C.c_void_p(int(pixel_mask)), None
        m = np.asarray(pixel_mask)
        if m.dtype not in (np.uint8, np.bool_) or m.shape != (self.H, self.W):
            raise SsfError("pixel mask must be uint8 (or bool) %dx%d, got %s %s" % (self.H, self.W, m.dtype, m.shape))
        m = np.ascontiguousarray(m).view(np.uint8)
        return _ptr(m), m

    def dynamic_superpixels(self):
        """(S uint8 array, count): the pixel-mask vote of the current frame, 1 = dynamic (all 0 without a pixel mask)"""
        self._need_pixmask("ssf_get_dynamic_superpixels")
        out = np.zeros(self.S, np.uint8)
        n = C.c_int()
        self._ck(self.L.lib.ssf_get_dynamic_superpixels(self.h, _ptr(out), C.byref(n)), "ssf_get_dynamic_superpixels")
        return out, n.value

    # ---- the model drawn into a virtual camera (include/ssf_render.h) ----------------------------
    def _need_render(self, symbol):
        if not self.L.has_render:
            raise SsfError("%s does not export %s: it does not render the model (include/ssf_render.h)" % (self.L.path, symbol))

    def _render_params(self, pose, camera, z_range, min_conf, splat_scale, visible_only, on_device):
        """(SsfRenderParams, the pose array it points into, (W, H)).  pose: 12 floats or a 3 x 4 [R | t] camera-to-map (None =
        the handle's pose); camera: dict(width, height, fx, fy, cx, cy) (None = the handle's camera); z_range: (z_min, z_max)
        (None = cfg.range_min / range_max)."""
        p = SsfRenderParams()
        keep = None
        if pose is not None:
            pose = np.asarray(pose, np.float32)
            if pose.shape == (3, 4):
                pose = np.concatenate([pose[:, :3].ravel(), pose[:, 3]])
            if pose.size != 12:
                raise SsfError("a render pose is 12 floats (R row-major, then t) or 3 x 4 [R | t], got shape %s" % (pose.shape,))
            keep = np.ascontiguousarray(pose.ravel(), np.float32)
            p.pose = keep.ctypes.data
        W, H = self.W, self.H
        if camera is not None:
            W, H = int(camera["width"]), int(camera["height"])
            p.width, p.height = W, H
            p.fx, p.fy, p.cx, p.cy = (float(camera[k]) for k in ("fx", "fy", "cx", "cy"))
        if z_range is not None:
            p.z_min, p.z_max = float(z_range[0]), float(z_range[1])
        p.min_conf, p.splat_scale = float(min_conf), float(splat_scale)
        p.visible_only, p.on_device = int(bool(visible_only)), int(bool(on_device))
        return p, keep, (W, H)

    def render_model(self, pose=None, camera=None, z_range=None, min_conf=0.0, splat_scale=3.0, visible_only=False,
                     outputs=RENDER_OUTPUT_NAMES):
        """The model drawn into a pinhole camera (ssf_render_model): dict of the requested images (depth H x W f32, index H x W
        i32, rgb8 / color / normal H x W x 3) and 'stats' (fragments, pixels_filled, rows_shown, list_entries)."""
        self._need_render("ssf_render_model")
        bad = [nm for nm in outputs if nm not in RENDER_OUTPUT_NAMES]
        if bad:
            raise SsfError("unknown render outputs %s (known: %s)" % (bad, ", ".join(RENDER_OUTPUT_NAMES)))
        p, keep, (W, H) = self._render_params(pose, camera, z_range, min_conf, splat_scale, visible_only, False)
        if W == 0:
            W, H = self.W, self.H            # (width 0: the handle's camera)
        if not (1 <= W <= 4096 and 1 <= H <= 4096):
            W = H = 1                        # (the library refuses the size and writes nothing)
        out = {nm: np.empty((H, W) + tail, dt) for nm, dt, tail in RENDER_OUTPUTS if nm in outputs}
        st = SsfRenderStats()
        self._ck(self.L.lib.ssf_render_model(self.h, C.byref(p), *[_ptr(out.get(nm)) for nm in RENDER_OUTPUT_NAMES], C.byref(st)),
                 "ssf_render_model")
        out["stats"] = st.as_dict()
        return out

    def render_model_device(self, depth=None, index=None, rgb8=None, color=None, normal=None, pose=None, camera=None,
                            z_range=None, min_conf=0.0, splat_scale=3.0, visible_only=False):
        """ssf_render_model into device memory: each output is None or the device address (int) of a contiguous buffer of the
        shape and dtype render_model returns (e.g. a torch tensor's data_ptr()).  Returns the stats dict."""
        self._need_render("ssf_render_model")
        p, keep, _ = self._render_params(pose, camera, z_range, min_conf, splat_scale, visible_only, True)
        ptrs = [None if a is None else C.c_void_p(int(a)) for a in (depth, index, rgb8, color, normal)]
        st = SsfRenderStats()
        self._ck(self.L.lib.ssf_render_model(self.h, C.byref(p), *ptrs, C.byref(st)), "ssf_render_model")
        return st.as_dict()

    def render_default_params(self):
        """ssf_render_default_params as a dict"""
        self._need_render("ssf_render_default_params")
        p = SsfRenderParams()
        self._ck(self.L.lib.ssf_render_default_params(self.h, C.byref(p)), "ssf_render_default_params")
        return {nm: getattr(p, nm) for nm, _ in p._fields_ if nm != "pose"}

    # ---- moving objects from the depth frame and the map (include/ssf_motion.h) --------------------
    def _need_motion(self, symbol):
        if not self.L.has_motion:
            raise SsfError("%s does not export %s: it does not detect motion (include/ssf_motion.h, HIP product only)"
                           % (self.L.path, symbol))

    def _motion_params(self, params, on_device):
        """(SsfMotionParams, the pose array it points into): the library's defaults overridden by the dict `params`; its
        'pose' is 12 floats or a 3 x 4 [R | t] camera-to-map (None = the handle's pose)."""
        p = SsfMotionParams()
        self._ck(self.L.lib.ssf_motion_default_params(self.h, C.byref(p)), "ssf_motion_default_params")
        keep = None
        for k, v in dict(params or {}).items():
            if k == "pose":
                if v is not None:
                    pose = np.asarray(v, np.float32)
                    if pose.shape == (3, 4):
                        pose = np.concatenate([pose[:, :3].ravel(), pose[:, 3]])
                    if pose.size != 12:
                        raise SsfError("a motion pose is 12 floats (R row-major, then t) or 3 x 4 [R | t], got shape %s" % (pose.shape,))
                    keep = np.ascontiguousarray(pose.ravel(), np.float32)
                    p.pose = keep.ctypes.data
            elif k == "on_device" or k not in [nm for nm, _ in p._fields_]:
                raise SsfError("ssf_motion_params has no settable field %r" % k)
            else:
                setattr(p, k, v)
        p.on_device = int(bool(on_device))
        return p, keep

    def motion_default_params(self):
        """ssf_motion_default_params as a dict (design choices, not tuned values: include/ssf_motion.h)"""
        self._need_motion("ssf_motion_default_params")
        p = SsfMotionParams()
        self._ck(self.L.lib.ssf_motion_default_params(self.h, C.byref(p)), "ssf_motion_default_params")
        return {nm: getattr(p, nm) for nm, _ in p._fields_ if nm not in ("pose", "on_device")}

    def _motion_outputs(self, outputs):
        bad = [nm for nm in outputs if nm not in MOTION_OUTPUT_NAMES]
        if bad:
            raise SsfError("unknown motion outputs %s (known: %s)" % (bad, ", ".join(MOTION_OUTPUT_NAMES)))
        return {nm: np.empty((self.H, self.W), dt) for nm, dt in MOTION_OUTPUTS if nm in outputs}

    def motion_segment(self, depth, model_depth, params=None, outputs=MOTION_OUTPUT_NAMES):
        """ssf_motion_segment on two host images (depth in the handle's input format, model_depth H x W float32): dict of the
        requested images (mask u8, label i32, cls u8) and 'stats'."""
        self._need_motion("ssf_motion_segment")
        depth = self._depth_array(depth)
        model_depth = np.asarray(model_depth)
        if model_depth.dtype != np.float32 or model_depth.shape != (self.H, self.W):
            raise SsfError("model depth must be float32 %dx%d, got %s %s" % (self.H, self.W, model_depth.dtype, model_depth.shape))
        model_depth = np.ascontiguousarray(model_depth)
        p, keep = self._motion_params(params, False)
        out = self._motion_outputs(outputs)
        st = SsfMotionStats()
        self._ck(self.L.lib.ssf_motion_segment(self.h, C.byref(p), _ptr(depth), _ptr(model_depth),
                                               *[_ptr(out.get(nm)) for nm in MOTION_OUTPUT_NAMES], C.byref(st)), "ssf_motion_segment")
        out["stats"] = st.as_dict()
        return out

    def motion_mask(self, depth, params=None, outputs=MOTION_OUTPUT_NAMES, model_depth=False):
        """ssf_motion_mask on a host depth image: dict of the requested images, 'stats' and, with model_depth=True, the
        rendered 'model_depth'."""
        self._need_motion("ssf_motion_mask")
        depth = self._depth_array(depth)
        p, keep = self._motion_params(params, False)
        out = self._motion_outputs(outputs)
        md = np.empty((self.H, self.W), np.float32) if model_depth else None
        st = SsfMotionStats()
        self._ck(self.L.lib.ssf_motion_mask(self.h, C.byref(p), _ptr(depth), *[_ptr(out.get(nm)) for nm in MOTION_OUTPUT_NAMES],
                                            _ptr(md), C.byref(st)), "ssf_motion_mask")
        if model_depth:
            out["model_depth"] = md
        out["stats"] = st.as_dict()
        return out

    @staticmethod
    def _dev_addr(a):
        """a device address: None, an int, or anything with data_ptr() (a torch tensor)"""
        if a is None:
            return None
        return C.c_void_p(int(a.data_ptr() if hasattr(a, "data_ptr") else a))

    def motion_mask_device(self, depth, mask=None, label=None, cls=None, model_depth_out=None, params=None, model_depth=None):
        """ssf_motion_mask (or, with model_depth given, ssf_motion_segment) on device memory: every image is None, a device
        address (int) or a tensor (data_ptr()) of the shape and dtype motion_mask returns.  `mask` is what
        process_frame_device(pixel_mask=...) takes.  Returns the stats dict."""
        self._need_motion("ssf_motion_segment" if model_depth is not None else "ssf_motion_mask")
        p, keep = self._motion_params(params, True)
        st = SsfMotionStats()
        outs = [self._dev_addr(a) for a in (mask, label, cls)]
        if model_depth is not None:
            self._ck(self.L.lib.ssf_motion_segment(self.h, C.byref(p), self._dev_addr(depth), self._dev_addr(model_depth), *outs, C.byref(st)),
                     "ssf_motion_segment")
        else:
            self._ck(self.L.lib.ssf_motion_mask(self.h, C.byref(p), self._dev_addr(depth), *outs, self._dev_addr(model_depth_out),
                                                C.byref(st)), "ssf_motion_mask")
        return st.as_dict()

    def last_motion_mask(self):
        """(H x W uint8 mask, stats dict) of the last process_frame(..., motion=...) (ssf_get_motion_mask)"""
        self._need_motion("ssf_get_motion_mask")
        mask = np.empty((self.H, self.W), np.uint8)
        st = SsfMotionStats()
        self._ck(self.L.lib.ssf_get_motion_mask(self.h, _ptr(mask), C.byref(st)), "ssf_get_motion_mask")
        return mask, st.as_dict()

    def _process_frame_motion(self, rgb_ptr, depth_ptr, on_device, prior, motion):
        self._need_motion("ssf_process_frame_motion")
        if not (motion is True or isinstance(motion, dict)):
            raise SsfError("motion is None, True or a dict of ssf_motion_params fields, got %r" % (motion,))
        p, keep = self._motion_params(None if motion is True else motion, on_device)
        res = SsfFrameResult()
        self._ck(self.L.lib.ssf_process_frame_motion(self.h, rgb_ptr, depth_ptr, int(bool(on_device)), _ptr(prior), C.byref(p), C.byref(res)),
                 "ssf_process_frame_motion")
        return res

    # ---- dense RGB-D odometry: the pose prior of the library's own (include/ssf_odometry.h) ---------
    def _need_odometry(self, symbol):
        if not self.L.has_odometry:
            raise SsfError("%s does not export %s: it has no dense odometry (include/ssf_odometry.h, HIP product only)"
                           % (self.L.path, symbol))

    def _odometry_params(self, params):
        """SsfOdometryParams: the library's defaults overridden by the dict `params` ('iters': a list, level 0 first)"""
        p = SsfOdometryParams()
        self._ck(self.L.lib.ssf_odometry_default_params(self.h, C.byref(p)), "ssf_odometry_default_params")
        for k, v in dict(params or {}).items():
            if k not in [nm for nm, _ in p._fields_]:
                raise SsfError("ssf_odometry_params has no field %r" % k)
            if k == "iters":
                v = list(v)
                if len(v) > ODO_MAX_LEVELS:
                    raise SsfError("iters has at most %d entries" % ODO_MAX_LEVELS)
                for l, n in enumerate(v):
                    p.iters[l] = int(n)
            else:
                setattr(p, k, v)
        return p

    @staticmethod
    def _pose12(pose, what):
        if pose is None:
            return None
        pose = np.asarray(pose, np.float32)
        if pose.shape == (3, 4):
            pose = np.concatenate([pose[:, :3].ravel(), pose[:, 3]])
        if pose.size != 12:
            raise SsfError("%s is 12 floats (R row-major, then t) or 3 x 4 [R | t], got shape %s" % (what, pose.shape))
        return np.ascontiguousarray(pose.ravel(), np.float32)

    def odometry_default_params(self):
        """ssf_odometry_default_params as a dict (design choices, not tuned values: include/ssf_odometry.h)"""
        self._need_odometry("ssf_odometry_default_params")
        return self._odometry_params(None).as_dict()

    def odometry_set_reference(self, rgb, depth, ref_mask=None):
        """the pyramid of a host frame becomes the resident reference, with the handle's pose; ref_mask: H x W, non-zero = ignore"""
        self._need_odometry("ssf_odometry_set_reference")
        rgb, depth = self._frame(rgb, depth)
        m = None
        if ref_mask is not None:
            m = np.ascontiguousarray(np.asarray(ref_mask) != 0, np.uint8)
            if m.shape != (self.H, self.W):
                raise SsfError("ref_mask must be %dx%d, got %s" % (self.H, self.W, m.shape))
        self._ck(self.L.lib.ssf_odometry_set_reference(self.h, _ptr(rgb), _ptr(depth), 0, _ptr(m)), "ssf_odometry_set_reference")

    def odometry_set_reference_device(self, d_rgb, d_depth, ref_mask=None):
        """... on device memory (addresses or tensors; ref_mask a device H x W uint8 image or None)"""
        self._need_odometry("ssf_odometry_set_reference")
        self._ck(self.L.lib.ssf_odometry_set_reference(self.h, self._dev_addr(d_rgb), self._dev_addr(d_depth), 1, self._dev_addr(ref_mask)),
                 "ssf_odometry_set_reference")

    def odometry_linearise(self, level, T12, params=None):
        """the 29 int64 words of the normal equations of the current pyramid against the reference at T (reference camera ->
        current camera), level `level`"""
        self._need_odometry("ssf_odometry_linearise")
        p = self._odometry_params(params)
        T = self._pose12(T12, "T12")
        rec = np.zeros(ODO_RECORD, np.int64)
        self._ck(self.L.lib.ssf_odometry_linearise(self.h, C.byref(p), int(level), _ptr(T), _ptr(rec)), "ssf_odometry_linearise")
        return rec

    def _odometry_estimate(self, rgb_ptr, depth_ptr, on_device, init, params):
        p = self._odometry_params(params)
        init = self._pose12(init, "init12")
        rel, res = np.zeros(12, np.float32), SsfOdometryResult()
        self._ck(self.L.lib.ssf_odometry_estimate(self.h, C.byref(p), rgb_ptr, depth_ptr, int(on_device), _ptr(init), _ptr(rel), C.byref(res)),
                 "ssf_odometry_estimate")
        return rel, res.as_dict()

    def odometry_estimate(self, rgb, depth, init12=None, params=None):
        """(rel, result): rel = current camera -> reference camera, 12 floats; the reference stays"""
        self._need_odometry("ssf_odometry_estimate")
        rgb, depth = self._frame(rgb, depth)
        return self._odometry_estimate(_ptr(rgb), _ptr(depth), 0, init12, params)

    def odometry_estimate_device(self, d_rgb, d_depth, init12=None, params=None):
        self._need_odometry("ssf_odometry_estimate")
        return self._odometry_estimate(self._dev_addr(d_rgb), self._dev_addr(d_depth), 1, init12, params)

    def _odometry_track(self, rgb_ptr, depth_ptr, on_device, params):
        p = self._odometry_params(params)
        prior, res = np.zeros(12, np.float32), SsfOdometryResult()
        self._ck(self.L.lib.ssf_odometry_track(self.h, C.byref(p), rgb_ptr, depth_ptr, int(on_device), _ptr(prior), C.byref(res)),
                 "ssf_odometry_track")
        return (prior if res.valid else None), res.as_dict()

    def odometry_track(self, rgb, depth, params=None):
        """(prior, result): prior = the pose prior of this frame (12 floats, what process_frame(prior_pose=...) takes), None when
        the estimate is invalid; the frame becomes the reference"""
        self._need_odometry("ssf_odometry_track")
        rgb, depth = self._frame(rgb, depth)
        return self._odometry_track(_ptr(rgb), _ptr(depth), 0, params)

    def odometry_track_device(self, d_rgb, d_depth, params=None):
        self._need_odometry("ssf_odometry_track")
        return self._odometry_track(self._dev_addr(d_rgb), self._dev_addr(d_depth), 1, params)

    def odometry_last(self):
        """dict(rel, prior (None when invalid), result) of the last track (ssf_get_odometry)"""
        self._need_odometry("ssf_get_odometry")
        rel, prior, res = np.zeros(12, np.float32), np.zeros(12, np.float32), SsfOdometryResult()
        self._ck(self.L.lib.ssf_get_odometry(self.h, _ptr(rel), _ptr(prior), C.byref(res)), "ssf_get_odometry")
        return dict(rel=rel, prior=prior if res.valid else None, result=res.as_dict())

    def odometry_pyramid(self, which, level):
        """level `level` of the reference (which = 0) or current (1) pyramid: dict(I, D, gx, gy, intrinsics (fx, fy, cx, cy))"""
        self._need_odometry("ssf_odometry_get_pyramid")
        w, h, k = C.c_int(), C.c_int(), np.zeros(4, np.float32)
        self._ck(self.L.lib.ssf_odometry_get_pyramid(self.h, int(which), int(level), None, None, None, None, C.byref(w), C.byref(h), _ptr(k)),
                 "ssf_odometry_get_pyramid")
        out = {nm: np.empty((h.value, w.value), np.float32) for nm in ("I", "D", "gx", "gy")}
        self._ck(self.L.lib.ssf_odometry_get_pyramid(self.h, int(which), int(level), *[_ptr(out[nm]) for nm in ("I", "D", "gx", "gy")],
                                                     None, None, None), "ssf_odometry_get_pyramid")
        out["intrinsics"] = k
        return out

    def _process_frame_odometry(self, rgb_ptr, depth_ptr, on_device, odometry, motion):
        self._need_odometry("ssf_process_frame_odometry")
        if not (odometry is True or isinstance(odometry, dict)):
            raise SsfError("odometry is None, True or a dict of ssf_odometry_params fields, got %r" % (odometry,))
        p = self._odometry_params(None if odometry is True else odometry)
        mp, keep = None, None
        if motion is not None:
            self._need_motion("ssf_process_frame_motion")
            if not (motion is True or isinstance(motion, dict)):
                raise SsfError("motion is None, True or a dict of ssf_motion_params fields, got %r" % (motion,))
            m, keep = self._motion_params(None if motion is True else motion, on_device)
            mp = C.byref(m)
        res = SsfFrameResult()
        self._ck(self.L.lib.ssf_process_frame_odometry(self.h, rgb_ptr, depth_ptr, int(bool(on_device)), C.byref(p), mp, C.byref(res)),
                 "ssf_process_frame_odometry")
        return res

    # ---- rows selected on the device by region, age and confidence (include/ssf_query.h) ----------
    def _need_query(self, symbol):
        if not self.L.has_query:
            raise SsfError("%s does not export %s: it does not query the model (include/ssf_query.h, HIP product only)"
                           % (self.L.path, symbol))

    def _query_params(self, on_device, min_conf=0.0, t_init=None, t_last=None, visible_only=False, region="all", pose=None,
                      radius=0.0, half=(0.0, 0.0, 0.0), camera=None, z_range=None):
        """(SsfQueryParams, the pose array it points into).  t_init / t_last: (min, max) of stamps.x / stamps.y (None = any);
        region: "all", "sphere" (radius about the pose's t), "box" (half extents in the pose's frame) or "frustum" (camera:
        dict(width, height, fx, fy, cx, cy), None = the handle's; z_range: (z_min, z_max), None = cfg.range_min / range_max);
        pose: 12 floats or a 3 x 4 [R | t] frame-to-map (None = the handle's pose)."""
        p = SsfQueryParams()
        self._ck(self.L.lib.ssf_query_default_params(self.h, C.byref(p)), "ssf_query_default_params")
        keep = None
        if pose is not None:
            pose = np.asarray(pose, np.float32)
            if pose.shape == (3, 4):
                pose = np.concatenate([pose[:, :3].ravel(), pose[:, 3]])
            if pose.size != 12:
                raise SsfError("a query pose is 12 floats (R row-major, then t) or 3 x 4 [R | t], got shape %s" % (pose.shape,))
            keep = np.ascontiguousarray(pose.ravel(), np.float32)
            p.pose = keep.ctypes.data
        p.min_conf = float(min_conf)
        if t_init is not None:
            p.t_init_min, p.t_init_max = int(t_init[0]), int(t_init[1])
        if t_last is not None:
            p.t_last_min, p.t_last_max = int(t_last[0]), int(t_last[1])
        if isinstance(region, str) and region not in QUERY_REGIONS:
            raise SsfError("unknown query region %r (known: %s)" % (region, ", ".join(QUERY_REGIONS)))
        p.region = QUERY_REGIONS[region] if isinstance(region, str) else int(region)
        p.radius = float(radius)
        p.half[0], p.half[1], p.half[2] = (float(v) for v in half)
        if camera is not None:
            p.width, p.height = int(camera["width"]), int(camera["height"])
            p.fx, p.fy, p.cx, p.cy = (float(camera[k]) for k in ("fx", "fy", "cx", "cy"))
        if z_range is not None:
            p.z_min, p.z_max = float(z_range[0]), float(z_range[1])
        p.visible_only, p.on_device = int(bool(visible_only)), int(bool(on_device))
        return p, keep

    def _query_rows(self, p, ptrs, index_ptr, capacity):
        """ssf_query_rows with raw pointers (field name -> address or None); returns the stats dict.  An SsfError raised here
        carries .rc and .stats (filled for SSF_ERR_CAPACITY: -4)"""
        st = SsfQueryStats()
        surf = SsfSurfels(*[ptrs.get(name) for name, _, _ in SURFEL_FIELDS])
        rc = self.L.lib.ssf_query_rows(self.h, C.byref(p), C.byref(surf) if any(ptrs.get(name) for name, _, _ in SURFEL_FIELDS) else None,
                                       index_ptr, int(capacity), C.byref(st))
        if rc != 0:
            e = SsfError("ssf_query_rows failed (%d): %s" % (rc, self.L.lib.ssf_last_error(self.h).decode()))
            e.rc, e.stats = rc, st.as_dict()
            raise e
        return st.as_dict()

    def query_default_params(self):
        """ssf_query_default_params as a dict"""
        self._need_query("ssf_query_default_params")
        p = SsfQueryParams()
        self._ck(self.L.lib.ssf_query_default_params(self.h, C.byref(p)), "ssf_query_default_params")
        return {nm: (list(getattr(p, nm)) if nm == "half" else getattr(p, nm)) for nm, _ in p._fields_ if nm != "pose"}

    def query_count(self, **kw):
        """How many rows a query selects, and their bounding box (ssf_query_count): the stats dict (n_scanned, n_selected,
        n_selected_visible, lo, hi).  Keywords: _query_params."""
        self._need_query("ssf_query_count")
        p, keep = self._query_params(False, **kw)
        st = SsfQueryStats()
        self._ck(self.L.lib.ssf_query_count(self.h, C.byref(p), C.byref(st)), "ssf_query_count")
        return st.as_dict()

    def query_rows_into(self, arrays, index, capacity, **kw):
        """ssf_query_rows into the caller's numpy arrays (dict: field name -> array, missing = not produced; index: int32 array
        or None), at most `capacity` rows.  Returns the stats dict."""
        self._need_query("ssf_query_rows")
        p, keep = self._query_params(False, **kw)
        return self._query_rows(p, {name: _ptr(a) for name, a in arrays.items()}, _ptr(index), capacity)

    def query_model(self, fields=tuple(name for name, _, _ in SURFEL_FIELDS), **kw):
        """The rows a query selects (ssf_query_rows): dict of the requested fields (arrays of n_selected rows, in get_model's
        layout and order), 'index' (their logical indices: get_model()[name][index] are the same rows) and 'stats'.  The
        buffers are sized from a count; should the call still report SSF_ERR_CAPACITY, it is repeated once with the size it names."""
        self._need_query("ssf_query_rows")
        known = {name: (k, dt) for name, k, dt in SURFEL_FIELDS}
        bad = [nm for nm in fields if nm not in known]
        if bad:
            raise SsfError("unknown model fields %s (known: %s)" % (bad, ", ".join(known)))
        p, keep = self._query_params(False, **kw)
        st = SsfQueryStats()
        self._ck(self.L.lib.ssf_query_count(self.h, C.byref(p), C.byref(st)), "ssf_query_count")
        n = int(st.n_selected)
        for attempt in (0, 1):
            out = {nm: np.zeros((n, known[nm][0]) if known[nm][0] > 1 else (n,), known[nm][1]) for nm in fields}
            index = np.zeros(n, np.int32)
            try:
                stats = self._query_rows(p, {nm: _ptr(a) for nm, a in out.items()}, _ptr(index), n)
                break
            except SsfError as e:
                if attempt or getattr(e, "rc", 0) != -4:
                    raise
                n = e.stats["n_selected"]
        m = stats["n_selected"]
        out = {nm: a[:m] for nm, a in out.items()}
        out["index"], out["stats"] = index[:m], stats
        return out

    def query_model_device(self, tensors, index=None, capacity=None, **kw):
        """ssf_query_rows into device memory: tensors maps field names to contiguous torch tensors on the device (rows x
        get_model's per-row shape and dtype; a device address as int also works, then give capacity), index an int32 tensor or
        None.  capacity: rows the outputs hold (default: the smallest first dimension).  Returns the stats dict."""
        self._need_query("ssf_query_rows")
        p, keep = self._query_params(True, **kw)
        outs = dict(tensors)
        if capacity is None:
            capacity = min(int(t.shape[0]) for t in list(outs.values()) + ([index] if index is not None else []))
        addr = lambda t: None if t is None else C.c_void_p(int(t) if isinstance(t, int) else t.data_ptr())
        return self._query_rows(p, {nm: addr(t) for nm, t in outs.items()}, addr(index), capacity)

    # ---- the floor-plane navigation grid: height, occupancy, clearance (include/ssf_navgrid.h) ------
    def _need_navgrid(self, symbol):
        if not self.L.has_navgrid:
            raise SsfError("%s does not export %s: it builds no navigation grid (include/ssf_navgrid.h, HIP product only)"
                           % (self.L.path, symbol))

    def _navgrid_params(self, on_device, pose=None, t_init=None, t_last=None, visible_only=False, unknown_is_obstacle=False, **kw):
        """(SsfNavGridParams, the pose array it points into).  pose: 12 floats or a 3 x 4 [R | t] grid-to-map (None = floor-aligned
        about the camera: include/ssf_navgrid.h); t_init / t_last: (min, max) of stamps.x / stamps.y (None = any); the other
        keywords are fields of ssf_navgrid_params (width, height, res, z_min, z_max, floor_max, floor_cos, min_conf, splat_scale,
        max_steps, min_hits, max_dist_cells), each at ssf_navgrid_default_params' value when missing."""
        p = SsfNavGridParams()
        self._ck(self.L.lib.ssf_navgrid_default_params(self.h, C.byref(p)), "ssf_navgrid_default_params")
        keep = None
        if pose is not None:
            pose = np.asarray(pose, np.float32)
            if pose.shape == (3, 4):
                pose = np.concatenate([pose[:, :3].ravel(), pose[:, 3]])
            if pose.size != 12:
                raise SsfError("a grid pose is 12 floats (R row-major, then t) or 3 x 4 [R | t], got shape %s" % (pose.shape,))
            keep = np.ascontiguousarray(pose.ravel(), np.float32)
            p.pose = keep.ctypes.data
        if t_init is not None:
            p.t_init_min, p.t_init_max = int(t_init[0]), int(t_init[1])
        if t_last is not None:
            p.t_last_min, p.t_last_max = int(t_last[0]), int(t_last[1])
        kinds = dict(p._fields_)
        for nm, v in kw.items():
            if nm not in kinds or nm in ("pose", "on_device") or nm.startswith("t_"):
                raise SsfError("unknown navigation grid parameter %r" % nm)
            setattr(p, nm, float(v) if kinds[nm] is C.c_float else int(v))
        p.visible_only, p.unknown_is_obstacle, p.on_device = int(bool(visible_only)), int(bool(unknown_is_obstacle)), int(bool(on_device))
        return p, keep

    def _navgrid_build(self, p, ptrs):
        st = SsfNavGridStats()
        out = SsfNavGridOut(*[ptrs.get(nm) for nm in NAVGRID_OUTPUT_NAMES])
        self._ck(self.L.lib.ssf_navgrid_build(self.h, C.byref(p), C.byref(out), C.byref(st)), "ssf_navgrid_build")
        return st.as_dict()

    def nav_grid(self, outputs=NAVGRID_OUTPUT_NAMES, **kw):
        """The navigation grid of the model (ssf_navgrid_build): dict of the requested arrays (zmin / zmax H x W f32, hits H x W x 2
        u32 (floor, obstacle), state H x W i8 (100 occupied, 0 free, -1 unknown), dist2 H x W i32: squared cells to the nearest
        obstacle cell, capped) and 'stats' (the counts, and 'pose': the grid frame used).  Keywords: _navgrid_params."""
        self._need_navgrid("ssf_navgrid_build")
        bad = [nm for nm in outputs if nm not in NAVGRID_OUTPUT_NAMES]
        if bad:
            raise SsfError("unknown navigation grid outputs %s (known: %s)" % (bad, ", ".join(NAVGRID_OUTPUT_NAMES)))
        p, keep = self._navgrid_params(False, **kw)
        W, H = p.width, p.height
        if not (1 <= W <= 4096 and 1 <= H <= 4096):
            W = H = 1                        # (the library refuses the size and writes nothing)
        out = {nm: np.empty((H, W) + tail, dt) for nm, dt, tail in NAVGRID_OUTPUTS if nm in outputs}
        stats = self._navgrid_build(p, {nm: _ptr(a) for nm, a in out.items()})
        out["stats"] = stats
        return out

    def nav_grid_device(self, zmin=None, zmax=None, hits=None, state=None, dist2=None, **kw):
        """ssf_navgrid_build into device memory: each output is None, a contiguous torch tensor on the device or the device address
        (int) of a buffer of the shape and dtype nav_grid returns.  Returns the stats dict."""
        self._need_navgrid("ssf_navgrid_build")
        p, keep = self._navgrid_params(True, **kw)
        addr = lambda t: None if t is None else C.c_void_p(int(t) if isinstance(t, int) else t.data_ptr())
        return self._navgrid_build(p, dict(zmin=addr(zmin), zmax=addr(zmax), hits=addr(hits), state=addr(state), dist2=addr(dist2)))

    def nav_grid_default_params(self):
        """ssf_navgrid_default_params as a dict"""
        self._need_navgrid("ssf_navgrid_default_params")
        p = SsfNavGridParams()
        self._ck(self.L.lib.ssf_navgrid_default_params(self.h, C.byref(p)), "ssf_navgrid_default_params")
        return {nm: getattr(p, nm) for nm, _ in p._fields_ if nm != "pose"}

    def nav_grid_default_pose(self, **kw):
        """the grid frame that pose=None means now (ssf_navgrid_default_pose): 12 floats, grid-to-map"""
        self._need_navgrid("ssf_navgrid_default_pose")
        p, keep = self._navgrid_params(False, **kw)
        pose = np.zeros(12, np.float32)
        self._ck(self.L.lib.ssf_navgrid_default_pose(self.h, C.byref(p), _ptr(pose)), "ssf_navgrid_default_pose")
        return pose

    # ---- the fitted floor plane: the grid's own frame and bands (include/ssf_navfloor.h) ------
    def _need_navfloor(self, symbol):
        if not self.L.has_navfloor:
            raise SsfError("%s does not export %s: it fits no floor plane (include/ssf_navfloor.h: libssf_hip_floor.so, binding.load_floor)"
                           % (self.L.path, symbol))

    def _navfloor_params(self, up=None, origin=None, t_init=None, t_last=None, visible_only=False, **kw):
        """(SsfNavFloorParams, the origin array it points into).  up: 3 floats (None = (0, -1, 0)); origin: 3 floats in the map frame
        (None = the camera position); t_init / t_last: (min, max) of stamps.x / stamps.y (None = any); the other keywords are fields of
        ssf_navfloor_params, each at ssf_navfloor_default_params' value when missing."""
        p = SsfNavFloorParams()
        self._ck(self.L.lib.ssf_navfloor_default_params(self.h, C.byref(p)), "ssf_navfloor_default_params")
        keep = None
        if up is not None:
            up = np.asarray(up, np.float32).ravel()
            if up.size != 3:
                raise SsfError("an up hint is 3 floats, got %d" % up.size)
            p.up[0], p.up[1], p.up[2] = float(up[0]), float(up[1]), float(up[2])
        if origin is not None:
            keep = np.ascontiguousarray(np.asarray(origin, np.float32).ravel())
            if keep.size != 3:
                raise SsfError("an origin is 3 floats, got %d" % keep.size)
            p.origin = keep.ctypes.data
        if t_init is not None:
            p.t_init_min, p.t_init_max = int(t_init[0]), int(t_init[1])
        if t_last is not None:
            p.t_last_min, p.t_last_max = int(t_last[0]), int(t_last[1])
        kinds = dict(p._fields_)
        for nm, v in kw.items():
            if nm not in kinds or nm in ("origin", "up", "visible_only") or nm.startswith("t_"):
                raise SsfError("unknown floor fit parameter %r" % nm)
            setattr(p, nm, float(v) if kinds[nm] is C.c_float else int(v))
        p.visible_only = int(bool(visible_only))
        return p, keep

    def nav_floor(self, histograms=True, **kw):
        """The floor plane of the model (ssf_navfloor_fit): dict of the result -- status (and status_name), the plane normal . (c -
        origin) = d, camera_height, the exact counts, the winners, per round inliers / rms / sums, pose and the three bands -- with
        'dir_hist' (31 x 31 u32) and 'height_hist' (2048 u32) unless histograms is False, and 'grid' = dict(pose, z_min, floor_max, z_max,
        width, height, res): what nav_grid, nav_grid_carve and the live calls take where they take those keywords.  Keywords:
        _navfloor_params."""
        self._need_navfloor("ssf_navfloor_fit")
        p, keep = self._navfloor_params(**kw)
        res = SsfNavFloorFitResult()
        dh, hh = np.zeros((NAVFLOOR_DIR_BINS, NAVFLOOR_DIR_BINS), np.uint32), np.zeros(NAVFLOOR_HEIGHT_BINS, np.uint32)
        out = SsfNavFloorOut(_ptr(dh), _ptr(hh)) if histograms else SsfNavFloorOut(None, None)
        self._ck(self.L.lib.ssf_navfloor_fit(self.h, C.byref(p), C.byref(out), C.byref(res)), "ssf_navfloor_fit")
        d = res.as_dict()
        if histograms:
            d["dir_hist"], d["height_hist"] = dh, hh
        d["grid"] = dict(pose=d["pose"].copy(), z_min=float(d["z_min"]), floor_max=float(d["floor_max"]), z_max=float(d["z_max"]), width=d["width"],
                         height=d["height"], res=float(d["res"]))
        return d

    def nav_floor_default_params(self):
        """ssf_navfloor_default_params as a dict"""
        self._need_navfloor("ssf_navfloor_default_params")
        p = SsfNavFloorParams()
        self._ck(self.L.lib.ssf_navfloor_default_params(self.h, C.byref(p)), "ssf_navfloor_default_params")
        d = {nm: getattr(p, nm) for nm, _ in p._fields_ if nm not in ("origin", "up")}
        d["up"] = tuple(float(v) for v in p.up)
        return d

    def nav_floor_grid(self, outputs=NAVGRID_OUTPUT_NAMES, floor=None, **grid_kw):
        """The fit, then the navigation grid in its frame and bands: dict(floor = nav_floor's dict, grid = nav_grid's).  floor: the fit's
        keywords (width, height and res come from grid_kw); grid_kw: nav_grid's other keywords (no pose, no bands: they are the fit's)."""
        self._need_navfloor("ssf_navfloor_fit")
        bad = [nm for nm in ("pose", "z_min", "z_max", "floor_max") if nm in grid_kw]
        if bad:
            raise SsfError("nav_floor_grid takes %s from the fit" % ", ".join(bad))
        size = {nm: grid_kw.pop(nm) for nm in ("width", "height", "res") if nm in grid_kw}
        fit = self.nav_floor(histograms=False, **dict(floor or {}, **size))
        return dict(floor=fit, grid=self.nav_grid(outputs=outputs, **dict(grid_kw, **fit["grid"])))

    # ---- the navigation grid with free space carved along camera rays (include/ssf_navcarve.h) ------
    def _need_navcarve(self, symbol):
        if not self.L.has_navcarve:
            raise SsfError("%s does not export %s: it carves no navigation grid (include/ssf_navcarve.h: libssf_hip_navcarve.so, binding.load_navcarve)"
                           % (self.L.path, symbol))

    def _navcarve_params(self, views, carve):
        """(SsfNavCarveParams, the views array it points into).  views: n x 12 floats or n x 3 x 4 [R | t], camera-to-map, host memory
        (None or empty: no views); carve: the other fields of ssf_navcarve_params by name, each at ssf_navcarve_default_params'
        value when missing."""
        c = SsfNavCarveParams()
        self._ck(self.L.lib.ssf_navcarve_default_params(self.h, C.byref(c)), "ssf_navcarve_default_params")
        keep = None
        if views is not None and np.size(views):
            v = np.asarray(views, np.float32)
            if v.ndim == 3 and v.shape[1:] == (3, 4):
                v = np.concatenate([v[:, :, :3].reshape(len(v), 9), v[:, :, 3]], axis=1)
            if v.ndim != 2 or v.shape[1] != 12:
                raise SsfError("views are n x 12 floats (R row-major, then t) or n x 3 x 4 [R | t], got shape %s" % (v.shape,))
            keep = np.ascontiguousarray(v, np.float32)
            c.views, c.n_views = keep.ctypes.data, len(keep)
        kinds = dict(c._fields_)
        for nm, val in (carve or {}).items():
            if nm not in kinds or nm in ("views", "n_views"):
                raise SsfError("unknown carve parameter %r" % nm)
            setattr(c, nm, float(val) if kinds[nm] is C.c_float else int(val))
        return c, keep

    def _navgrid_carve(self, p, c, ptrs):
        st = SsfNavCarveStats()
        out = SsfNavCarveOut(SsfNavGridOut(*[ptrs.get(nm) for nm in NAVGRID_OUTPUT_NAMES]), ptrs.get("seen"))
        self._ck(self.L.lib.ssf_navgrid_carve(self.h, C.byref(p), C.byref(c), C.byref(out), C.byref(st)), "ssf_navgrid_carve")
        return st.as_dict()

    def nav_grid_carve(self, views, outputs=NAVCARVE_OUTPUT_NAMES, carve=None, **kw):
        """The navigation grid with free space carved along the rays of `views` (ssf_navgrid_carve): nav_grid's dict (the state and
        dist2 carved) plus seen (H x W u32: ray entries per cell) and the carve's counts in 'stats'.  views, carve:
        _navcarve_params; the other keywords: _navgrid_params."""
        self._need_navcarve("ssf_navgrid_carve")
        bad = [nm for nm in outputs if nm not in NAVCARVE_OUTPUT_NAMES]
        if bad:
            raise SsfError("unknown carved grid outputs %s (known: %s)" % (bad, ", ".join(NAVCARVE_OUTPUT_NAMES)))
        p, keep = self._navgrid_params(False, **kw)
        c, keep_views = self._navcarve_params(views, carve)
        W, H = p.width, p.height
        if not (1 <= W <= 4096 and 1 <= H <= 4096):
            W = H = 1                        # (the library refuses the size and writes nothing)
        out = {nm: np.empty((H, W) + tail, dt) for nm, dt, tail in NAVCARVE_OUTPUTS if nm in outputs}
        stats = self._navgrid_carve(p, c, {nm: _ptr(a) for nm, a in out.items()})
        out["stats"] = stats
        return out

    def nav_grid_carve_device(self, views, zmin=None, zmax=None, hits=None, state=None, dist2=None, seen=None, carve=None, **kw):
        """ssf_navgrid_carve into device memory: each output is None, a contiguous torch tensor on the device or the device address
        (int) of a buffer of the shape and dtype nav_grid_carve returns; the views stay host memory.  Returns the stats dict."""
        self._need_navcarve("ssf_navgrid_carve")
        p, keep = self._navgrid_params(True, **kw)
        c, keep_views = self._navcarve_params(views, carve)
        addr = lambda t: None if t is None else C.c_void_p(int(t) if isinstance(t, int) else t.data_ptr())
        return self._navgrid_carve(p, c, dict(zmin=addr(zmin), zmax=addr(zmax), hits=addr(hits), state=addr(state), dist2=addr(dist2),
                                              seen=addr(seen)))

    def nav_grid_carve_default_params(self):
        """ssf_navcarve_default_params as a dict"""
        self._need_navcarve("ssf_navcarve_default_params")
        c = SsfNavCarveParams()
        self._ck(self.L.lib.ssf_navcarve_default_params(self.h, C.byref(c)), "ssf_navcarve_default_params")
        return {nm: getattr(c, nm) for nm, _ in c._fields_ if nm != "views"}

    def debug_navcarve_set_chunk_rays(self, max_rays):
        """test hook: the rays per chunk of nav_grid_carve (0 = the default); results do not depend on it"""
        self._need_navcarve("ssf_debug_navcarve_set_chunk_rays")
        self._ck(self.L.lib.ssf_debug_navcarve_set_chunk_rays(self.h, int(max_rays)), "ssf_debug_navcarve_set_chunk_rays")

    def debug_navcarve_last(self):
        """dict(chunks, atomics) of the last nav_grid_carve of this handle"""
        self._need_navcarve("ssf_debug_navcarve_last")
        a, b = C.c_int64(0), C.c_int64(0)
        self._ck(self.L.lib.ssf_debug_navcarve_last(self.h, C.byref(a), C.byref(b)), "ssf_debug_navcarve_last")
        return dict(chunks=int(a.value), atomics=int(b.value))

    # ---- plan on the navigation grid: cost-to-goal field and paths (include/ssf_navplan.h) ------------
    def _need_navplan(self, symbol):
        if not self.L.has_navplan:
            raise SsfError("%s does not export %s: it plans on no navigation grid (include/ssf_navplan.h: libssf_hip_nav.so, binding.load_nav)"
                           % (self.L.path, symbol))

    @staticmethod
    def _cell_list(cells, what):
        """n x 2 int32 (ix, iy), contiguous; None or empty: no cells"""
        if cells is None or np.size(cells) == 0:
            return np.zeros((0, 2), np.int32)
        a = np.asarray(cells)
        if a.ndim != 2 or a.shape[1] != 2:
            raise SsfError("%s are n x 2 cells (ix, iy), got shape %s" % (what, a.shape))
        return np.ascontiguousarray(a, np.int32)

    def _navplan_params(self, on_device, width, height, goals, starts, params):
        """(SsfNavPlanParams, the goal and start arrays it points into).  goals, starts: n x 2 cells (ix, iy), host memory; params:
        the other fields of ssf_navplan_params by name, each at ssf_navplan_default_params' value when missing."""
        p = SsfNavPlanParams()
        self._ck(self.L.lib.ssf_navplan_default_params(self.h, C.byref(p)), "ssf_navplan_default_params")
        g, s = self._cell_list(goals, "goals"), self._cell_list(starts, "starts")
        kinds = dict(p._fields_)
        for nm, val in params.items():
            if nm not in kinds or nm in ("width", "height", "goals", "n_goals", "starts", "n_starts", "on_device"):
                raise SsfError("unknown plan parameter %r" % nm)
            setattr(p, nm, int(val))
        p.width, p.height, p.on_device = int(width), int(height), int(bool(on_device))
        p.goals, p.n_goals = (g.ctypes.data if len(g) else None), len(g)
        p.starts, p.n_starts = (s.ctypes.data if len(s) else None), len(s)
        return p, (g, s)

    def _navplan_field(self, p, state, dist2, ptrs):
        st = SsfNavPlanStats()
        out = SsfNavPlanOut(*[ptrs.get(nm) for nm in NAVPLAN_OUTPUT_NAMES])
        self._ck(self.L.lib.ssf_navplan_field(self.h, C.byref(p), state, dist2, C.byref(out), C.byref(st)), "ssf_navplan_field")
        return st.as_dict()

    def nav_plan(self, state, dist2, goals=None, starts=None, outputs=NAVPLAN_OUTPUT_NAMES, **params):
        """The cost-to-goal field of a navigation grid and the paths down it (ssf_navplan_field).  state H x W int8 and dist2
        H x W int32 as nav_grid / nav_grid_carve return them; goals, starts: n x 2 cells (ix, iy).  Returns a dict of the requested
        outputs -- cost H x W u32 (0xFFFFFFFF: not reached), frontier H x W u8, start_cost (n u32), start_status (n i32), path_len
        (n i32), path: a list with one (len, 2) int32 array per start -- and 'stats'.  params: min_dist2, soft_dist2, near_penalty,
        allow_unknown, goals_from_frontier, max_path."""
        self._need_navplan("ssf_navplan_field")
        bad = [nm for nm in outputs if nm not in NAVPLAN_OUTPUT_NAMES]
        if bad:
            raise SsfError("unknown plan outputs %s (known: %s)" % (bad, ", ".join(NAVPLAN_OUTPUT_NAMES)))
        state, dist2 = np.ascontiguousarray(state, np.int8), np.ascontiguousarray(dist2, np.int32)
        if state.ndim != 2 or dist2.shape != state.shape:
            raise SsfError("state and dist2 are H x W arrays of one shape, got %s and %s" % (state.shape, dist2.shape))
        H, W = state.shape
        p, keep = self._navplan_params(False, W, H, goals, starts, params)
        n, mp = p.n_starts, max(p.max_path, 0)
        shapes = dict(cost=((H, W), np.uint32), frontier=((H, W), np.uint8), start_cost=((n,), np.uint32), start_status=((n,), np.int32),
                      path_len=((n,), np.int32), path=((n, min(mp, 1 << 20), 2), np.int32))
        want = set(outputs)
        if "path" in want:
            want.add("path_len")                     # (the lengths cut the paths)
        out = {nm: np.zeros(*shapes[nm]) for nm in NAVPLAN_OUTPUT_NAMES if nm in want}
        stats = self._navplan_field(p, _ptr(state), _ptr(dist2), {nm: _ptr(a) for nm, a in out.items()})
        if "path" in out:
            out["path"] = [out["path"][i, :out["path_len"][i]].copy() for i in range(n)]
        if "path_len" not in outputs:
            out.pop("path_len", None)
        out["stats"] = stats
        return out

    def nav_plan_device(self, state, dist2, width, height, goals=None, starts=None, cost=None, frontier=None, start_cost=None, start_status=None,
                        path_len=None, path=None, **params):
        """ssf_navplan_field on device memory: state, dist2 and each output are a contiguous torch tensor on the device or the device
        address (int) of a buffer of the shape and dtype nav_plan works on (path: n_starts x max_path x 2 int32; outputs may be
        None); goals and starts stay host memory.  Returns the stats dict."""
        self._need_navplan("ssf_navplan_field")
        p, keep = self._navplan_params(True, width, height, goals, starts, params)
        addr = lambda t: None if t is None else C.c_void_p(int(t) if isinstance(t, int) else t.data_ptr())
        return self._navplan_field(p, addr(state), addr(dist2), dict(cost=addr(cost), frontier=addr(frontier), start_cost=addr(start_cost),
                                                                     start_status=addr(start_status), path_len=addr(path_len), path=addr(path)))

    def nav_plan_default_params(self):
        """ssf_navplan_default_params as a dict"""
        self._need_navplan("ssf_navplan_default_params")
        p = SsfNavPlanParams()
        self._ck(self.L.lib.ssf_navplan_default_params(self.h, C.byref(p)), "ssf_navplan_default_params")
        return {nm: getattr(p, nm) for nm, _ in p._fields_ if nm not in ("goals", "starts")}

    def nav_plan_from_map(self, views, goals=None, starts=None, grid=None, carve=None, plan=None, outputs=NAVPLAN_OUTPUT_NAMES):
        """Carve the navigation grid of the map along `views` (nav_grid_carve_device) into device tensors and plan on them
        (nav_plan_device) without the grid leaving the device.  grid: nav_grid's keywords; carve: the carve's parameters; plan: the
        plan's.  Returns nav_plan's dict, with 'grid_stats' (the carve's) beside 'stats'."""
        import torch
        self._need_navplan("ssf_navplan_field")
        self._need_navcarve("ssf_navgrid_carve")
        grid, plan = dict(grid or {}), dict(plan or {})
        gp, _ = self._navgrid_params(True, **grid)
        W, H = gp.width, gp.height
        if not (1 <= W <= 4096 and 1 <= H <= 4096):
            raise SsfError("the grid's size must be 1..4096 x 1..4096")
        dev = torch.device("cuda")
        state, dist2 = torch.empty((H, W), dtype=torch.int8, device=dev), torch.empty((H, W), dtype=torch.int32, device=dev)
        grid_stats = self.nav_grid_carve_device(views, state=state, dist2=dist2, carve=carve, **grid)
        g, s = self._cell_list(goals, "goals"), self._cell_list(starts, "starts")
        n, mp = len(s), int(plan.get("max_path", 0))
        kinds = dict(cost=((H, W), torch.int32), frontier=((H, W), torch.uint8), start_cost=((n,), torch.int32), start_status=((n,), torch.int32),
                     path_len=((n,), torch.int32), path=((n, max(min(mp, 1 << 20), 0), 2), torch.int32))
        want = set(outputs) | ({"path_len"} if "path" in outputs else set())
        t = {nm: torch.zeros(kinds[nm][0], dtype=kinds[nm][1], device=dev) for nm in NAVPLAN_OUTPUT_NAMES if nm in want}
        stats = self.nav_plan_device(state, dist2, W, H, g, s, **dict(t, **plan))
        out = {nm: a.cpu().numpy() for nm, a in t.items()}
        for nm in ("cost", "start_cost"):
            if nm in out:
                out[nm] = out[nm].view(np.uint32)
        if "path" in out:
            out["path"] = [out["path"][i, :out["path_len"][i]].copy() for i in range(n)]
        if "path_len" not in outputs:
            out.pop("path_len", None)
        out["stats"], out["grid_stats"] = stats, grid_stats
        return out

    def debug_navplan_set_round_batch(self, rounds):
        """test hook: the relaxation rounds per look at the flagged-tile count (0 = the default); results never depend on it"""
        self._need_navplan("ssf_debug_navplan_set_round_batch")
        self._ck(self.L.lib.ssf_debug_navplan_set_round_batch(self.h, int(rounds)), "ssf_debug_navplan_set_round_batch")

    def debug_navplan_last(self):
        """dict(rounds, tile_visits) of the last nav_plan of this handle"""
        self._need_navplan("ssf_debug_navplan_last")
        a, b = C.c_int64(0), C.c_int64(0)
        self._ck(self.L.lib.ssf_debug_navplan_last(self.h, C.byref(a), C.byref(b)), "ssf_debug_navplan_last")
        return dict(rounds=int(a.value), tile_visits=int(b.value))

    # ---- the frontier of the navigation grid as regions (include/ssf_navfrontier.h) --------------------
    def _need_navfrontier(self, symbol):
        if not self.L.has_navfrontier:
            raise SsfError("%s does not export %s: it groups no frontier (include/ssf_navfrontier.h: libssf_hip_explore.so, binding.load_explore)"
                           % (self.L.path, symbol))

    def _navfrontier_params(self, on_device, width, height, params):
        """SsfNavFrontierParams: the fields of ssf_navfrontier_params by name, each at ssf_navfrontier_default_params' value when
        missing"""
        p = SsfNavFrontierParams()
        self._ck(self.L.lib.ssf_navfrontier_default_params(self.h, C.byref(p)), "ssf_navfrontier_default_params")
        kinds = dict(p._fields_)
        for nm, val in params.items():
            if nm not in kinds or nm in ("width", "height", "on_device"):
                raise SsfError("unknown frontier parameter %r" % nm)
            setattr(p, nm, int(val))
        p.width, p.height, p.on_device = int(width), int(height), int(bool(on_device))
        return p

    def _navfrontier_regions(self, p, state, dist2, cost, region):
        """the call with a host table and order of max_regions records: (regions, order, stats), cut to regions_written"""
        n = min(max(p.max_regions, 0), NAVFRONTIER_MAX_REGIONS)
        regions, order = np.zeros(n, NAVFRONTIER_REGION_DTYPE), np.zeros(n, np.int32)
        st, out = SsfNavFrontierStats(), SsfNavFrontierOut(region, _ptr(regions), _ptr(order))
        self._ck(self.L.lib.ssf_navfrontier_regions(self.h, C.byref(p), state, dist2, cost, C.byref(out), C.byref(st)), "ssf_navfrontier_regions")
        stats = st.as_dict()
        k = stats["regions_written"]
        return regions[:k].copy(), order[:k].copy(), stats

    def nav_frontiers(self, state, dist2=None, cost=None, **params):
        """The frontier of a navigation grid grouped into regions (ssf_navfrontier_regions).  state H x W int8 and dist2 H x W int32
        as nav_grid / nav_grid_carve return them, cost H x W uint32 as nav_plan returns it (both may be None).  Returns a dict:
        'region' H x W int32 (table index, -1 no member, -2 not in the table), 'regions' (NAVFRONTIER_REGION_DTYPE records, in label
        order), 'order' (table indices, best first) and 'stats'.  params: connectivity, traversable_only, min_dist2, min_cells,
        reachable_only, max_regions, gain_radius, cost_weight, gain_weight, size_weight."""
        self._need_navfrontier("ssf_navfrontier_regions")
        state = np.ascontiguousarray(state, np.int8)
        if state.ndim != 2:
            raise SsfError("state is an H x W array, got shape %s" % (state.shape,))
        if dist2 is not None:
            dist2 = np.ascontiguousarray(dist2, np.int32)
        if cost is not None:
            cost = np.ascontiguousarray(cost, np.uint32)
        for nm, a in (("dist2", dist2), ("cost", cost)):
            if a is not None and a.shape != state.shape:
                raise SsfError("state and %s are H x W arrays of one shape, got %s and %s" % (nm, state.shape, a.shape))
        H, W = state.shape
        p = self._navfrontier_params(False, W, H, params)
        region = np.zeros((H, W), np.int32)
        regions, order, stats = self._navfrontier_regions(p, _ptr(state), _ptr(dist2), _ptr(cost), _ptr(region))
        return dict(region=region, regions=regions, order=order, stats=stats)

    def nav_frontiers_device(self, state, width, height, dist2=None, cost=None, region=None, **params):
        """ssf_navfrontier_regions on device memory: state, dist2, cost and region are contiguous torch tensors on the device or
        device addresses (int) of buffers of the shapes and dtypes nav_frontiers works on (dist2, cost and region may be None); the
        table and the order stay host memory.  Returns a dict of 'regions', 'order' and 'stats'."""
        self._need_navfrontier("ssf_navfrontier_regions")
        p = self._navfrontier_params(True, width, height, params)
        addr = lambda t: None if t is None else C.c_void_p(int(t) if isinstance(t, int) else t.data_ptr())
        regions, order, stats = self._navfrontier_regions(p, addr(state), addr(dist2), addr(cost), addr(region))
        return dict(regions=regions, order=order, stats=stats)

    def nav_frontiers_default_params(self):
        """ssf_navfrontier_default_params as a dict"""
        self._need_navfrontier("ssf_navfrontier_default_params")
        p = SsfNavFrontierParams()
        self._ck(self.L.lib.ssf_navfrontier_default_params(self.h, C.byref(p)), "ssf_navfrontier_default_params")
        return {nm: getattr(p, nm) for nm, _ in p._fields_}

    def nav_explore(self, state, dist2, robot_cell, plan=None, frontier=None):
        """Where to go next on a navigation grid, in three calls: (1) nav_plan with the robot's cell as the only goal: the field;
        (2) nav_frontiers with that field as `cost`; (3) nav_plan with the chosen region's representative as the only goal and the
        robot as the start: the path.  The chosen region is order[0], if it was reached.  plan: the plan's parameters (min_dist2,
        soft_dist2, near_penalty, allow_unknown, max_path; max_path defaults to width * height capped at 1 << 20); frontier:
        nav_frontiers' parameters (reachable_only defaults to 1).

        The field's cost is "from the cell to the robot": the cost of driving from the cell to the robot's cell.  With a clearance
        penalty it differs from the drive out, robot to cell, by pen[cell] - pen[robot], because a move pays the penalty of the cell
        it enters; rep_cost and the ranking use the field as it is, and 'cost' below is the drive out as step (3) computes it.

        Returns a dict: 'region', 'regions', 'order', 'stats' as nav_frontiers; 'chosen' (the table index, or -1 when no region was
        reached); 'goal' ((ix, iy) or None); 'cost' (u32), 'status' and 'path' ((len, 2) int32) of the drive to it, None / empty
        without a goal; 'field_stats' and 'path_stats' (the two plans' stats)."""
        self._need_navplan("ssf_navplan_field")
        self._need_navfrontier("ssf_navfrontier_regions")
        plan, frontier = dict(plan or {}), dict(frontier or {})
        for nm in ("goals_from_frontier",):
            if nm in plan:
                raise SsfError("nav_explore sets %s itself" % nm)
        state = np.ascontiguousarray(state, np.int8)
        if state.ndim != 2:
            raise SsfError("state is an H x W array, got shape %s" % (state.shape,))
        H, W = state.shape
        robot = self._cell_list([tuple(robot_cell)], "robot_cell")
        max_path = int(plan.pop("max_path", min(W * H, 1 << 20)))
        field = self.nav_plan(state, dist2, goals=robot, outputs=("cost",), **plan)
        frontier.setdefault("reachable_only", 1)
        out = self.nav_frontiers(state, dist2, field["cost"], **frontier)
        out.update(field_stats=field["stats"], chosen=-1, goal=None, cost=None, status=None, path=np.zeros((0, 2), np.int32), path_stats=None)
        if len(out["order"]) and out["regions"]["rep_cost"][out["order"][0]] != NAVPLAN_UNREACHED:
            c = int(out["order"][0])
            goal = (int(out["regions"]["rep_x"][c]), int(out["regions"]["rep_y"][c]))
            drive = self.nav_plan(state, dist2, goals=[goal], starts=robot, outputs=("start_cost", "start_status", "path"), max_path=max_path, **plan)
            out.update(chosen=c, goal=goal, cost=int(drive["start_cost"][0]), status=int(drive["start_status"][0]), path=drive["path"][0],
                       path_stats=drive["stats"])
        return out

    # ---- any-angle waypoints from the plan's cell paths (include/ssf_navpath.h) -----------------------
    def _need_navpath(self, symbol):
        if not self.L.has_navpath:
            raise SsfError("%s does not export %s: it refines no path (include/ssf_navpath.h: libssf_hip_drive.so, binding.load_drive)"
                           % (self.L.path, symbol))

    def _navpath_params(self, on_device, width, height, n_paths, max_path, params):
        """SsfNavPathParams: the fields of ssf_navpath_params by name, each at ssf_navpath_default_params' value when missing;
        max_waypoints defaults to max_path (no path has more waypoints than cells)"""
        p = SsfNavPathParams()
        self._ck(self.L.lib.ssf_navpath_default_params(self.h, C.byref(p)), "ssf_navpath_default_params")
        kinds = dict(p._fields_)
        for nm, val in params.items():
            if nm not in kinds or nm in ("width", "height", "n_paths", "max_path", "on_device"):
                raise SsfError("unknown waypoint parameter %r" % nm)
            setattr(p, nm, int(val))
        p.width, p.height, p.n_paths, p.max_path, p.on_device = int(width), int(height), int(n_paths), int(max_path), int(bool(on_device))
        if "max_waypoints" not in params:
            p.max_waypoints = p.max_path
        return p

    def _navpath_waypoints(self, p, state, dist2, path, path_len, ptrs):
        st = SsfNavPathStats()
        out = SsfNavPathOut(*[ptrs.get(nm) for nm in NAVPATH_OUTPUT_NAMES])
        self._ck(self.L.lib.ssf_navpath_waypoints(self.h, C.byref(p), state, dist2, path, path_len, C.byref(out), C.byref(st)), "ssf_navpath_waypoints")
        return st.as_dict()

    def nav_waypoints(self, state, dist2, path, path_len=None, outputs=NAVPATH_OUTPUT_NAMES, **params):
        """The cell paths of a plan reduced to any-angle waypoints (ssf_navpath_waypoints).  state H x W int8 and dist2 H x W int32
        as nav_grid / nav_grid_carve return them; path: n x max_path x 2 int32 with path_len (n), or a list of (len, 2) arrays as
        nav_plan returns it (path_len None).  Returns a dict of the requested outputs -- n_waypoints (n i32), status (n i32),
        waypoints: a list with one (n_waypoints, 4) int32 array per path, (ix, iy, index | NAVPATH_FORCED, seg_min), path_min
        (n i32) -- and 'stats'.  params: min_dist2, allow_unknown, los_dist2, keep_clearance, clearance_cap, lookahead,
        max_waypoints (default: max_path)."""
        self._need_navpath("ssf_navpath_waypoints")
        bad = [nm for nm in outputs if nm not in NAVPATH_OUTPUT_NAMES]
        if bad:
            raise SsfError("unknown waypoint outputs %s (known: %s)" % (bad, ", ".join(NAVPATH_OUTPUT_NAMES)))
        state, dist2 = np.ascontiguousarray(state, np.int8), np.ascontiguousarray(dist2, np.int32)
        if state.ndim != 2 or dist2.shape != state.shape:
            raise SsfError("state and dist2 are H x W arrays of one shape, got %s and %s" % (state.shape, dist2.shape))
        if path_len is None:
            cells = [self._cell_list(c, "a path's cells") for c in path]
            path_len = np.array([len(c) for c in cells], np.int32)
            path = np.zeros((len(cells), max(1, int(path_len.max()) if len(cells) else 1), 2), np.int32)
            for i, c in enumerate(cells):
                path[i, :len(c)] = c
        path, path_len = np.ascontiguousarray(path, np.int32), np.ascontiguousarray(path_len, np.int32)
        if path.ndim != 3 or path.shape[2] != 2 or path_len.shape != (path.shape[0],):
            raise SsfError("path is n x max_path x 2 and path_len n, got %s and %s" % (path.shape, path_len.shape))
        H, W = state.shape
        n, mp = path.shape[0], path.shape[1]
        p = self._navpath_params(False, W, H, n, mp, params)
        mw = min(max(p.max_waypoints, 0), 1 << 20)
        shapes = dict(n_waypoints=((n,), np.int32), status=((n,), np.int32), waypoints=((n, mw, 4), np.int32), path_min=((n,), np.int32))
        want = set(outputs)
        if "waypoints" in want:
            want.add("n_waypoints")                  # (the counts cut the lists)
        out = {nm: np.zeros(*shapes[nm]) for nm in NAVPATH_OUTPUT_NAMES if nm in want}
        stats = self._navpath_waypoints(p, _ptr(state), _ptr(dist2), _ptr(path), _ptr(path_len), {nm: _ptr(a) for nm, a in out.items()})
        if "waypoints" in out:
            out["waypoints"] = [out["waypoints"][i, :out["n_waypoints"][i]].copy() for i in range(n)]
        if "n_waypoints" not in outputs:
            out.pop("n_waypoints", None)
        out["stats"] = stats
        return out

    def nav_waypoints_device(self, state, dist2, width, height, path, path_len, n_paths, max_path, n_waypoints=None, status=None, waypoints=None,
                             path_min=None, **params):
        """ssf_navpath_waypoints on device memory: state, dist2, path, path_len and each output are a contiguous torch tensor on the
        device or the device address (int) of a buffer of the shape and dtype nav_waypoints works on (waypoints: n_paths x
        max_waypoints x 4 int32; outputs may be None).  Returns the stats dict."""
        self._need_navpath("ssf_navpath_waypoints")
        p = self._navpath_params(True, width, height, n_paths, max_path, params)
        addr = lambda t: None if t is None else C.c_void_p(int(t) if isinstance(t, int) else t.data_ptr())
        return self._navpath_waypoints(p, addr(state), addr(dist2), addr(path), addr(path_len),
                                       dict(n_waypoints=addr(n_waypoints), status=addr(status), waypoints=addr(waypoints), path_min=addr(path_min)))

    def nav_waypoints_default_params(self):
        """ssf_navpath_default_params as a dict"""
        self._need_navpath("ssf_navpath_default_params")
        p = SsfNavPathParams()
        self._ck(self.L.lib.ssf_navpath_default_params(self.h, C.byref(p)), "ssf_navpath_default_params")
        return {nm: getattr(p, nm) for nm, _ in p._fields_}

    def nav_plan_waypoints(self, state, dist2, goals=None, starts=None, plan=None, waypoints=None):
        """Plan and refine without the paths leaving the device: state and dist2 (host arrays) are uploaded once, nav_plan_device
        writes the field's paths into device tensors and nav_waypoints_device reads them there.  plan: the plan's parameters
        (max_path defaults to width * height capped at 1 << 20); waypoints: the waypoints' parameters (min_dist2 and allow_unknown
        default to the plan's; max_waypoints to 4096 or max_path, whichever is less).  Returns a dict: 'plan' (start_cost,
        start_status, path_len, path, stats, as nav_plan) and 'waypoints' (nav_waypoints' dict)."""
        import torch
        self._need_navplan("ssf_navplan_field")
        self._need_navpath("ssf_navpath_waypoints")
        plan, wq = dict(plan or {}), dict(waypoints or {})
        state, dist2 = np.ascontiguousarray(state, np.int8), np.ascontiguousarray(dist2, np.int32)
        if state.ndim != 2 or dist2.shape != state.shape:
            raise SsfError("state and dist2 are H x W arrays of one shape, got %s and %s" % (state.shape, dist2.shape))
        H, W = state.shape
        s = self._cell_list(starts, "starts")
        n = len(s)
        if n < 1:
            raise SsfError("nav_plan_waypoints needs a start")
        mp = int(plan.setdefault("max_path", min(W * H, 1 << 20)))
        for nm in ("min_dist2", "allow_unknown"):
            wq.setdefault(nm, plan.get(nm, 0))
        mw = int(wq.setdefault("max_waypoints", max(1, min(4096, mp))))
        dev = torch.device("cuda")
        d_state, d_dist2 = torch.from_numpy(state).to(dev), torch.from_numpy(dist2).to(dev)
        i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dev)
        t = dict(start_cost=i32(n), start_status=i32(n), path_len=i32(n), path=i32(n, max(mp, 1), 2))
        plan_stats = self.nav_plan_device(d_state, d_dist2, W, H, goals, s, **dict(t, **plan))
        o = dict(n_waypoints=i32(n), status=i32(n), waypoints=i32(n, max(mw, 1), 4), path_min=i32(n))
        wp_stats = self.nav_waypoints_device(d_state, d_dist2, W, H, t["path"], t["path_len"], n, mp, **dict(o, **wq))
        got = {nm: a.cpu().numpy() for nm, a in t.items()}
        got["start_cost"] = got["start_cost"].view(np.uint32)
        got["path"] = [got["path"][i, :got["path_len"][i]].copy() for i in range(n)]
        got["stats"] = plan_stats
        ref = {nm: a.cpu().numpy() for nm, a in o.items()}
        ref["waypoints"] = [ref["waypoints"][i, :ref["n_waypoints"][i]].copy() for i in range(n)]
        ref["stats"] = wp_stats
        return dict(plan=got, waypoints=ref)

    # ---- the live obstacle layer: the depth frame stamped onto a navigation grid (include/ssf_navlive.h) ----
    def _need_navlive(self, symbol):
        if not self.L.has_navlive:
            raise SsfError("%s does not export %s: it overlays no depth frame (include/ssf_navlive.h: libssf_hip_live.so, binding.load_live)"
                           % (self.L.path, symbol))

    # what the calls that put a depth frame onto a grid share (nav_live*, nav_memory*): params, host checks, frame staging
    def _frame_layer_defaults(self, struct, default_fn, as_dict=False):
        """`struct` as the library's `default_fn` (a symbol's name) fills it; as_dict: its fields but the poses, what nav_*_default_params return"""
        p = struct()
        self._ck(getattr(self.L.lib, default_fn)(self.h, C.byref(p)), default_fn)
        return {nm: getattr(p, nm) for nm, _ in p._fields_ if nm not in ("grid_pose", "cam_pose")} if as_dict else p

    def _frame_layer_params(self, struct, default_fn, what, on_device, frame_on_device, grid_pose=None, cam_pose=None, **kw):
        """(struct, the pose arrays it points into).  grid_pose: grid-to-map, what the grid's stats returned as 'pose' (None =
        nav_grid_default_pose now); cam_pose: camera-to-map (None = the handle's pose); the other keywords are fields of the struct by
        name, each at default_fn's value when missing; what: how an error calls them ('overlay', 'memory')."""
        p = self._frame_layer_defaults(struct, default_fn)
        keep = []
        for nm, pose in (("grid_pose", grid_pose), ("cam_pose", cam_pose)):
            if pose is not None:
                keep.append(self._pose12(pose, nm))
                setattr(p, nm, keep[-1].ctypes.data)
        kinds = dict(p._fields_)
        for nm, val in kw.items():
            if nm not in kinds or nm in ("grid_pose", "cam_pose", "on_device", "frame_on_device"):
                raise SsfError("unknown %s parameter %r" % (what, nm))
            if kinds[nm] is C.c_uint32 and not 0 <= int(val) <= 0xFFFFFFFF:
                raise SsfError("%s is a uint32, got %r" % (nm, val))
            setattr(p, nm, float(val) if kinds[nm] is C.c_float else int(val))
        p.on_device, p.frame_on_device = int(bool(on_device)), int(bool(frame_on_device))
        return p, keep

    def _frame_layer_host(self, who, make_params, depth, state, mask, kw):
        """The host arrays of `who` (nav_live, nav_memory) checked: state 2-D int8, which fixes width and height; depth of the camera's
        shape in the handle's input format; mask of depth's shape.  make_params(W, H) builds the call's params once the grid's size
        is known.  Returns (p, keep, depth, state, mask)."""
        state = np.ascontiguousarray(state, np.int8)
        if state.ndim != 2:
            raise SsfError("state is a height x width array, got shape %s" % (state.shape,))
        for nm in ("width", "height"):
            if nm in kw:
                raise SsfError("%s takes %s from state" % (who, nm))
        H, W = state.shape
        p, keep = make_params(W, H)
        cw, ch = (p.cam_width, p.cam_height) if p.cam_width else (self.W, self.H)
        depth = np.ascontiguousarray(depth, np.uint16 if self.depth_format == "u16" else np.float32)
        if depth.shape != (ch, cw):
            raise SsfError("depth is %d x %d in the handle's input format, got shape %s" % (ch, cw, depth.shape))
        if mask is not None:
            mask = np.ascontiguousarray(mask, np.uint8)
            if mask.shape != depth.shape:
                raise SsfError("mask and depth are images of one shape, got %s and %s" % (mask.shape, depth.shape))
        return p, keep, depth, state, mask

    def _frame_layer_device(self, depth, mask, frame_on_device):
        """(addr, depth, mask, keep) of a device call: addr(t) is the pointer of a tensor or a device address (None stays None);
        depth and mask go through it, or, with frame_on_device false, are host arrays (kept alive in `keep`) and their pointers."""
        addr = lambda t: None if t is None else C.c_void_p(int(t) if isinstance(t, int) else t.data_ptr())
        if frame_on_device:
            return addr, addr(depth), addr(mask), ()
        depth = np.ascontiguousarray(depth, np.uint16 if self.depth_format == "u16" else np.float32)
        mask = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        return addr, _ptr(depth), _ptr(mask), (depth, mask)

    def _navlive_params(self, on_device, frame_on_device, **kw):
        """(SsfNavLiveParams, the pose arrays it points into): _frame_layer_params over ssf_navlive_params"""
        return self._frame_layer_params(SsfNavLiveParams, "ssf_navlive_default_params", "overlay", on_device, frame_on_device, **kw)

    def _navlive_overlay(self, p, depth, mask, state_in, ptrs):
        st = SsfNavLiveStats()
        out = SsfNavLiveOut(*[ptrs.get(nm) for nm in NAVLIVE_OUTPUT_NAMES])
        self._ck(self.L.lib.ssf_navlive_overlay(self.h, C.byref(p), depth, mask, state_in, C.byref(out), C.byref(st)), "ssf_navlive_overlay")
        return st.as_dict()

    def nav_live(self, depth, state, mask=None, outputs=NAVLIVE_OUTPUT_NAMES, **kw):
        """The depth frame of the instant stamped onto a navigation grid (ssf_navlive_overlay), host arrays.  depth: H x W in the
        handle's input format (set_input_format); state: height x width int8 as nav_grid / nav_grid_carve or an earlier nav_live
        returned it (it fixes width and height); mask: H x W uint8 or None (with mask_mode 1 or 2: nav_motion_mask's output plugs in
        here).  Returns a dict of the requested outputs -- live_hits, live_seen (u32), state (i8), dist2 (i32), each height x
        width -- and 'stats'.  Keywords: _navlive_params."""
        self._need_navlive("ssf_navlive_overlay")
        bad = [nm for nm in outputs if nm not in NAVLIVE_OUTPUT_NAMES]
        if bad:
            raise SsfError("unknown overlay outputs %s (known: %s)" % (bad, ", ".join(NAVLIVE_OUTPUT_NAMES)))
        p, keep, depth, state, mask = self._frame_layer_host(
            "nav_live", lambda W, H: self._navlive_params(False, False, width=W, height=H, **kw), depth, state, mask, kw)
        out = {nm: np.zeros(state.shape, dt) for nm, dt in NAVLIVE_OUTPUTS if nm in outputs}
        stats = self._navlive_overlay(p, _ptr(depth), _ptr(mask), _ptr(state), {nm: _ptr(a) for nm, a in out.items()})
        out["stats"] = stats
        return out

    def nav_live_device(self, depth, state, width, height, mask=None, live_hits=None, live_seen=None, state_out=None, dist2=None,
                        frame_on_device=True, **kw):
        """ssf_navlive_overlay on device memory: state and each output are a contiguous torch tensor on the device or the device
        address (int) of a buffer of the shape and dtype nav_live works on (outputs may be None, not all; state_out may be `state`
        itself: the update in place); depth and mask likewise, or host arrays with frame_on_device=False.  Returns the stats dict."""
        self._need_navlive("ssf_navlive_overlay")
        p, keep = self._navlive_params(True, frame_on_device, width=width, height=height, **kw)
        addr, d, m, frame = self._frame_layer_device(depth, mask, frame_on_device)
        return self._navlive_overlay(p, d, m, addr(state), dict(live_hits=addr(live_hits), live_seen=addr(live_seen), state=addr(state_out),
                                                                dist2=addr(dist2)))

    def nav_live_default_params(self):
        """ssf_navlive_default_params as a dict"""
        self._need_navlive("ssf_navlive_default_params")
        return self._frame_layer_defaults(SsfNavLiveParams, "ssf_navlive_default_params", as_dict=True)

    def nav_live_plan(self, depth, state, goals, starts, waypoints=False, mask=None, live=None, plan=None, waypoint_params=None, _overlay=None):
        """Overlay, plan and (waypoints=True) refine without the grid leaving the device: state (host, height x width int8) and the
        depth frame (host array in the input format, or a device tensor) are uploaded once, nav_live_device writes the live state and
        dist2 into device tensors, nav_plan_device plans on them and nav_waypoints_device reads its paths there.  live: the overlay's
        keywords (_navlive_params); plan: the plan's parameters (max_path defaults to width * height capped at 1 << 20);
        waypoint_params: the waypoints' (defaults as nav_plan_waypoints).  Returns a dict: 'live' (state, dist2, stats), 'plan'
        (start_cost, start_status, path_len, path, stats, as nav_plan) and, with waypoints, 'waypoints' (nav_waypoints' dict)."""
        import torch
        self._need_navlive("ssf_navlive_overlay")
        self._need_navplan("ssf_navplan_field")
        if waypoints:
            self._need_navpath("ssf_navpath_waypoints")
        live, plan, wq = dict(live or {}), dict(plan or {}), dict(waypoint_params or {})
        state = np.ascontiguousarray(state, np.int8)
        if state.ndim != 2:
            raise SsfError("state is a height x width array, got shape %s" % (state.shape,))
        H, W = state.shape
        s = self._cell_list(starts, "starts")
        n = len(s)
        if n < 1:
            raise SsfError("nav_live_plan needs a start")
        dev = torch.device("cuda")
        on_dev = isinstance(depth, torch.Tensor)
        if not on_dev:
            depth = torch.from_numpy(np.ascontiguousarray(depth, np.uint16 if self.depth_format == "u16" else np.float32).view(
                np.int16 if self.depth_format == "u16" else np.float32)).to(dev)
        if mask is not None and not isinstance(mask, torch.Tensor):
            mask = torch.from_numpy(np.ascontiguousarray(mask, np.uint8)).to(dev)
        d_state = torch.from_numpy(state).to(dev)
        d_dist2 = torch.empty((H, W), dtype=torch.int32, device=dev)
        live_stats = (_overlay or self.nav_live_device)(depth, d_state, W, H, mask=mask, state_out=d_state, dist2=d_dist2, **live)      # (_overlay: nav_memory_plan's)
        mp = int(plan.setdefault("max_path", min(W * H, 1 << 20)))
        i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dev)
        t = dict(start_cost=i32(n), start_status=i32(n), path_len=i32(n), path=i32(n, max(mp, 1), 2))
        plan_stats = self.nav_plan_device(d_state, d_dist2, W, H, goals, s, **dict(t, **plan))
        got = {nm: a.cpu().numpy() for nm, a in t.items()}
        got["start_cost"] = got["start_cost"].view(np.uint32)
        got["path"] = [got["path"][i, :got["path_len"][i]].copy() for i in range(n)]
        got["stats"] = plan_stats
        res = dict(live=dict(state=d_state.cpu().numpy(), dist2=d_dist2.cpu().numpy(), stats=live_stats), plan=got)
        if waypoints:
            for nm in ("min_dist2", "allow_unknown"):
                wq.setdefault(nm, plan.get(nm, 0))
            mw = int(wq.setdefault("max_waypoints", max(1, min(4096, mp))))
            o = dict(n_waypoints=i32(n), status=i32(n), waypoints=i32(n, max(mw, 1), 4), path_min=i32(n))
            wp_stats = self.nav_waypoints_device(d_state, d_dist2, W, H, t["path"], t["path_len"], n, mp, **dict(o, **wq))
            ref = {nm: a.cpu().numpy() for nm, a in o.items()}
            ref["waypoints"] = [ref["waypoints"][i, :ref["n_waypoints"][i]].copy() for i in range(n)]
            ref["stats"] = wp_stats
            res["waypoints"] = ref
        return res

    # ---- the live layer with memory: height-sliced marks, ray clearing and decay (include/ssf_navmem.h) ----
    def _need_navmem(self, symbol):
        if not self.L.has_navmem:
            raise SsfError("%s does not export %s: its live layer has no memory (include/ssf_navmem.h: libssf_hip_mem.so, binding.load_mem)"
                           % (self.L.path, symbol))

    def _navmem_params(self, on_device, frame_on_device, **kw):
        """(SsfNavMemParams, the pose arrays it points into): _frame_layer_params over ssf_navmem_params"""
        return self._frame_layer_params(SsfNavMemParams, "ssf_navmem_default_params", "memory", on_device, frame_on_device, **kw)

    def _navmem_update(self, p, depth, mask, state_in, layer, ptrs):
        st = SsfNavMemStats()
        lay = SsfNavMemLayer(*layer) if layer is not None else None
        out = SsfNavMemOut(*[ptrs.get(nm) for nm in NAVMEM_OUTPUT_NAMES])
        self._ck(self.L.lib.ssf_navmem_update(self.h, C.byref(p), depth, mask, state_in, None if lay is None else C.byref(lay), C.byref(out),
                                              C.byref(st)), "ssf_navmem_update")
        return st.as_dict()

    def nav_memory(self, depth, state, memory=None, mask=None, tick=None, outputs=NAVMEM_OUTPUT_NAMES, **kw):
        """The depth frame stamped into the caller's sliced memory of the live layer (ssf_navmem_update), host arrays.  depth: H x W in
        the handle's input format; state: height x width int8, the STATIC grid of every frame (nav_grid's or nav_grid_carve's); memory:
        a LiveMemory of host arrays of that size -- read, updated in place and its tick advanced -- or None for a zero layer that is
        not kept; tick: this update's (None = memory.tick + 1, or 1).  Returns a dict of the requested outputs -- marks, mark_tick,
        seen_tick, live_hits, hit_bits, seen_bits (u32), state (i8), dist2 (i32), each height x width -- and 'stats'.  With a memory
        the three layer arrays returned ARE the memory's.  Keywords: _navmem_params."""
        self._need_navmem("ssf_navmem_update")
        bad = [nm for nm in outputs if nm not in NAVMEM_OUTPUT_NAMES]
        if bad:
            raise SsfError("unknown memory outputs %s (known: %s)" % (bad, ", ".join(NAVMEM_OUTPUT_NAMES)))
        def make_params(W, H):
            if memory is not None and (memory.device or (memory.height, memory.width) != (H, W)):
                raise SsfError("nav_memory takes a LiveMemory of host arrays of the state's size %d x %d" % (H, W))
            t = memory.next_tick(tick) if memory is not None else (1 if tick is None else int(tick))
            return self._navmem_params(False, False, width=W, height=H, tick=t, **kw)
        p, keep, depth, state, mask = self._frame_layer_host("nav_memory", make_params, depth, state, mask, kw)
        tick = p.tick
        out = {nm: np.zeros(state.shape, dt) for nm, dt in NAVMEM_OUTPUTS if nm in outputs}
        layer = None
        if memory is not None:
            layer = [_ptr(a) for a in memory.arrays()]
            out.update(zip(NAVMEM_LAYER_NAMES, memory.arrays()))          # the update in place, asked for or not
        stats = self._navmem_update(p, _ptr(depth), _ptr(mask), _ptr(state), layer, {nm: _ptr(a) for nm, a in out.items()})
        if memory is not None:
            memory.tick = tick
        out = {nm: a for nm, a in out.items() if nm in outputs}
        out["stats"] = stats
        return out

    def nav_memory_device(self, depth, state, width, height, memory=None, mask=None, layer_in=None, marks=None, mark_tick=None, seen_tick=None,
                          live_hits=None, hit_bits=None, seen_bits=None, state_out=None, dist2=None, frame_on_device=True, tick=None, **kw):
        """ssf_navmem_update on device memory: state and each output are a contiguous torch tensor on the device or the device address
        (int) of a buffer of the shape and dtype nav_memory works on (outputs may be None, not all; state_out may be `state` itself);
        depth and mask likewise, or host arrays with frame_on_device=False.  memory: a LiveMemory(device=True), read, updated in place
        and its tick advanced; or, without one, layer_in: None or three tensors / addresses (None = zero) and marks / mark_tick /
        seen_tick: where the layer goes (each may be its own input).  Returns the stats dict."""
        self._need_navmem("ssf_navmem_update")
        if memory is not None:
            if not memory.device or (memory.height, memory.width) != (int(height), int(width)):
                raise SsfError("nav_memory_device takes a LiveMemory(device=True) of the grid's size %d x %d" % (height, width))
            if layer_in is not None or marks is not None or mark_tick is not None or seen_tick is not None:
                raise SsfError("nav_memory_device takes a LiveMemory or the layer's arrays, not both")
            layer_in = memory.arrays()
            marks, mark_tick, seen_tick = layer_in
            tick = memory.next_tick(tick)
        elif tick is None:
            tick = 1
        p, keep = self._navmem_params(True, frame_on_device, width=width, height=height, tick=tick, **kw)
        addr, d, m, frame = self._frame_layer_device(depth, mask, frame_on_device)
        layer = None if layer_in is None else [addr(a) for a in layer_in]
        stats = self._navmem_update(p, d, m, addr(state), layer, dict(marks=addr(marks), mark_tick=addr(mark_tick), seen_tick=addr(seen_tick),
                                                                      live_hits=addr(live_hits), hit_bits=addr(hit_bits), seen_bits=addr(seen_bits),
                                                                      state=addr(state_out), dist2=addr(dist2)))
        if memory is not None:
            memory.tick = int(tick)
        return stats

    def nav_memory_default_params(self):
        """ssf_navmem_default_params as a dict"""
        self._need_navmem("ssf_navmem_default_params")
        return self._frame_layer_defaults(SsfNavMemParams, "ssf_navmem_default_params", as_dict=True)

    def _navmem_overlay(self, memory, tick):
        """nav_memory_device with `memory` in the place of nav_live_device in the chains below"""
        self._need_navmem("ssf_navmem_update")
        if not isinstance(memory, LiveMemory) or not memory.device:
            raise SsfError("the chain keeps its grid on the device: it takes a LiveMemory(device=True)")
        return lambda depth, state, W, H, **k: self.nav_memory_device(depth, state, W, H, memory=memory, tick=tick, **k)

    def nav_memory_plan(self, depth, state, memory, goals, starts, waypoints=False, mask=None, tick=None, live=None, plan=None, waypoint_params=None):
        """nav_live_plan with the memory in the overlay's place: update, plan and (waypoints=True) refine without the grid or the layer
        leaving the device.  state: the STATIC grid (host, height x width int8), uploaded afresh every call; memory: a
        LiveMemory(device=True), updated in place; live: the update's keywords (_navmem_params).  Returns nav_live_plan's dict ('live'
        holds the update's state, dist2 and stats)."""
        return self.nav_live_plan(depth, state, goals, starts, waypoints=waypoints, mask=mask, live=live, plan=plan, waypoint_params=waypoint_params,
                                  _overlay=self._navmem_overlay(memory, tick))

    def nav_memory_dyn_steer(self, depth, state, memory, goals, poses, tracker, steps_since=1, targets=None, tick=None, motion=None, live=None,
                             blobs=None, plan=None, steer=None):
        """nav_live_dyn_steer with the memory in the overlay's place: the moving pixels stay out of the stamp (mask_mode 2) but their rays
        still clear, so a mover's trail is not remembered and what it walked away from is cleared behind it.  memory: a
        LiveMemory(device=True), updated in place; live: the update's keywords (_navmem_params).  Returns nav_live_dyn_steer's dict."""
        return self.nav_live_dyn_steer(depth, state, goals, poses, tracker, steps_since=steps_since, targets=targets, motion=motion, live=live,
                                       blobs=blobs, plan=plan, steer=steer, _overlay=self._navmem_overlay(memory, tick))

    # ---- velocity commands on the navigation grid: rollouts scored on the device (include/ssf_navsteer.h) ----
    def _need_navsteer(self, symbol):
        if not self.L.has_navsteer:
            raise SsfError("%s does not export %s: it steers nothing (include/ssf_navsteer.h: libssf_hip_steer.so, binding.load_steer)"
                           % (self.L.path, symbol))

    def _navsteer_params(self, on_device, width, height, n_poses, params):
        """SsfNavSteerParams: the fields of ssf_navsteer_params by name, each at ssf_navsteer_default_params' value when missing"""
        p = SsfNavSteerParams()
        self._ck(self.L.lib.ssf_navsteer_default_params(self.h, C.byref(p)), "ssf_navsteer_default_params")
        kinds = dict(p._fields_)
        for nm, val in params.items():
            if nm not in kinds or nm in ("width", "height", "n_poses", "on_device"):
                raise SsfError("unknown steering parameter %r" % nm)
            setattr(p, nm, int(val))
        p.width, p.height, p.n_poses, p.on_device = int(width), int(height), int(n_poses), int(bool(on_device))
        return p

    def _navsteer_rollouts(self, p, state, dist2, cost, poses, targets, ptrs, n_headings=None):
        """the disc's rollouts over `state`, or with n_headings the footprint's over the mask given in its place"""
        st = SsfNavSteerStats()
        out = SsfNavSteerOut(*[ptrs.get(nm) for nm in NAVSTEER_OUTPUT_NAMES])
        if n_headings is None:
            self._ck(self.L.lib.ssf_navsteer_rollouts(self.h, C.byref(p), state, dist2, cost, poses, targets, C.byref(out), C.byref(st)),
                     "ssf_navsteer_rollouts")
        else:
            self._ck(self.L.lib.ssf_navfoot_rollouts(self.h, C.byref(p), int(n_headings), state, dist2, cost, poses, targets, C.byref(out),
                                                     C.byref(st)), "ssf_navfoot_rollouts")
        return st.as_dict()

    @staticmethod
    def _navsteer_shape(kind, tail, n, K, T):
        return (n,) + ((K,) if kind == "cand" else ()) + tuple(T + 1 if d == "T1" else d for d in tail)

    def nav_steer(self, state, dist2, poses, cost=None, targets=None, outputs=NAVSTEER_POSE_OUTPUTS, **params):
        """A lattice of (v, w) candidates rolled out from every pose over the grid, tested and scored (ssf_navsteer_rollouts), host
        arrays.  state H x W int8 and dist2 H x W int32 as the grid calls or nav_live return them; cost H x W uint32 as nav_plan
        returns it (None with cost_weight=0); poses n x 3 int32 (x, y, heading) in units (nav_steer_units); targets n x 2 int32 (None
        with target_weight 0).  Returns a dict of the requested outputs (NAVSTEER_OUTPUTS; best_traj: a list with one (best_len, 3)
        array per pose) and 'stats'.  params: the other fields of ssf_navsteer_params by name."""
        self._need_navsteer("ssf_navsteer_rollouts")
        return self._nav_steer_host(state, np.int8, "state", None, dist2, poses, cost, targets, outputs, params)

    def _nav_steer_host(self, state, grid_dtype, grid_name, n_headings, dist2, poses, cost, targets, outputs, params):
        """nav_steer's body, and nav_foot_steer's with the mask in the place of state"""
        bad = [nm for nm in outputs if nm not in NAVSTEER_OUTPUT_NAMES]
        if bad:
            raise SsfError("unknown steering outputs %s (known: %s)" % (bad, ", ".join(NAVSTEER_OUTPUT_NAMES)))
        state, dist2 = np.ascontiguousarray(state, grid_dtype), np.ascontiguousarray(dist2, np.int32)
        if state.ndim != 2 or dist2.shape != state.shape:
            raise SsfError("%s and dist2 are H x W arrays of one shape, got %s and %s" % (grid_name, state.shape, dist2.shape))
        H, W = state.shape
        poses = np.ascontiguousarray(poses, np.int32)
        if poses.ndim != 2 or poses.shape[1] != 3:
            raise SsfError("poses are n x 3 (x, y, heading) in units, got shape %s" % (poses.shape,))
        n = poses.shape[0]
        if cost is not None:
            cost = np.ascontiguousarray(cost, np.uint32)
            if cost.shape != state.shape:
                raise SsfError("cost is an H x W array like state, got %s" % (cost.shape,))
        if targets is not None:
            targets = np.ascontiguousarray(targets, np.int32)
            if targets.shape != (n, 2):
                raise SsfError("targets are n x 2 (x, y) in units, one per pose, got shape %s" % (targets.shape,))
        p = self._navsteer_params(False, W, H, n, params)
        K, T = max(p.n_v, 0) * max(p.n_w, 0), max(p.n_steps, 0)
        if not (0 < K <= 65536 and T <= 256 and n * K <= 1 << 24):
            K = T = 1                                # (the call refuses it: the arrays only have to exist)
        want = set(outputs)
        if "best_traj" in want:
            want.add("best_len")                     # (the counts cut the lists)
        out = {nm: np.zeros(self._navsteer_shape(kind, tail, n, K, T), dt) for nm, dt, kind, tail in NAVSTEER_OUTPUTS if nm in want}
        stats = self._navsteer_rollouts(p, _ptr(state), _ptr(dist2), _ptr(cost), _ptr(poses), _ptr(targets), {nm: _ptr(a) for nm, a in out.items()},
                                        n_headings)
        if "best_traj" in out:
            out["best_traj"] = [out["best_traj"][i, :out["best_len"][i]].copy() for i in range(n)]
        if "best_len" not in outputs:
            out.pop("best_len", None)
        out["stats"] = stats
        return out

    def nav_steer_device(self, state, dist2, width, height, poses, n_poses, cost=None, targets=None, best=None, best_cmd=None, best_score=None,
                         n_admissible=None, pose_status=None, best_len=None, best_traj=None, cand_free=None, cand_min_d=None, cand_end=None,
                         cand_end_cost=None, cand_score=None, **params):
        """ssf_navsteer_rollouts on device memory: state, dist2, cost, poses, targets and each output are a contiguous torch tensor on
        the device or the device address (int) of a buffer of the shape and dtype nav_steer works on (outputs may be None, not all):
        nav_live_device's state and dist2 and nav_plan_device's cost are read where they lie.  Returns the stats dict."""
        self._need_navsteer("ssf_navsteer_rollouts")
        p = self._navsteer_params(True, width, height, n_poses, params)
        addr = lambda t: None if t is None else C.c_void_p(int(t) if isinstance(t, int) else t.data_ptr())
        return self._navsteer_rollouts(p, addr(state), addr(dist2), addr(cost), addr(poses), addr(targets),
                                       dict(best=addr(best), best_cmd=addr(best_cmd), best_score=addr(best_score), n_admissible=addr(n_admissible),
                                            pose_status=addr(pose_status), best_len=addr(best_len), best_traj=addr(best_traj), cand_free=addr(cand_free),
                                            cand_min_d=addr(cand_min_d), cand_end=addr(cand_end), cand_end_cost=addr(cand_end_cost),
                                            cand_score=addr(cand_score)))

    def nav_steer_default_params(self):
        """ssf_navsteer_default_params as a dict"""
        self._need_navsteer("ssf_navsteer_default_params")
        p = SsfNavSteerParams()
        self._ck(self.L.lib.ssf_navsteer_default_params(self.h, C.byref(p)), "ssf_navsteer_default_params")
        return {nm: getattr(p, nm) for nm, _ in p._fields_}

    @staticmethod
    def nav_steer_window(v_now, w_now, v_limits, w_limits, accel, dt, res, n_v, n_w):
        """The integer lattice of a dynamic window (pure host arithmetic): the speeds (m/s) and turn rates (rad/s) reachable from
        (v_now, w_now) within one step of dt seconds under accel = (a_v m/s^2, a_w rad/s^2), cut to v_limits = (lo, hi) and
        w_limits = (lo, hi) and to the call's own |v| <= 1024, |w| <= 16384, in units per step: v = speed * dt * 1024 / res,
        w = rate * dt * 65536 / 2 pi.  The lattice starts at the window's lower end rounded up and its step is rounded down, so that
        no candidate lies outside the window; an axis whose window is narrower than its count keeps fewer candidates (a step of 0 and
        a count of 1 when it is narrower than one unit).  Returns dict(n_v, n_w, v_min, v_step, w_min, w_step): nav_steer's keywords."""
        if not (dt > 0 and res > 0 and n_v >= 1 and n_w >= 1):
            raise SsfError("nav_steer_window needs dt > 0, res > 0, n_v >= 1 and n_w >= 1")

        def axis(now, limits, a, scale, cap, n):
            lo, hi = max(float(limits[0]), now - a * dt), min(float(limits[1]), now + a * dt)
            if lo > hi:                              # (the current value lies outside the limits: the nearest limit)
                lo = hi = min(max(now, float(limits[0])), float(limits[1]))
            a0, a1 = max(int(np.ceil(lo * scale)), -cap), min(int(np.floor(hi * scale)), cap)
            if a0 > a1:                              # (narrower than one unit: the unit nearest to its middle)
                a0 = a1 = min(max(int(np.rint(0.5 * (lo + hi) * scale)), -cap), cap)
            n = min(int(n), a1 - a0 + 1)
            return n, a0, ((a1 - a0) // (n - 1) if n > 1 else 0)

        nv, v0, dv = axis(float(v_now), v_limits, float(accel[0]), dt * NAVSTEER_SUBUNITS / res, 1024, n_v)
        nw, w0, dw = axis(float(w_now), w_limits, float(accel[1]), dt * NAVSTEER_TURN / (2.0 * np.pi), 16384, n_w)
        return dict(n_v=nv, n_w=nw, v_min=v0, v_step=dv, w_min=w0, w_step=dw)

    @staticmethod
    def nav_steer_units(pose_xy_yaw, res):
        """Metric grid-frame poses (x m, y m, yaw rad; one or n x 3) in the call's units (pure host arithmetic): n x 3 int32
        (floor(x / res * 1024), floor(y / res * 1024), round(yaw / 2 pi * 65536) & 0xFFFF)"""
        a = np.atleast_2d(np.asarray(pose_xy_yaw, np.float64))
        if a.shape[1] != 3 or not res > 0:
            raise SsfError("nav_steer_units takes (x, y, yaw) rows and res > 0, got shape %s" % (a.shape,))
        out = np.zeros(a.shape, np.int64)
        out[:, :2] = np.floor(a[:, :2] / res * NAVSTEER_SUBUNITS)
        out[:, 2] = np.rint(a[:, 2] / (2.0 * np.pi) * NAVSTEER_TURN).astype(np.int64) & 0xFFFF
        return out.astype(np.int32)

    def nav_live_steer(self, depth, state, goals, poses, targets=None, mask=None, live=None, plan=None, steer=None):
        """Overlay, plan and steer with nothing but the command leaving the device: state (host, height x width int8) and the depth
        frame (host array in the input format, or a device tensor) are uploaded once, nav_live_device writes the live state and dist2
        into device tensors, nav_plan_device writes the cost-to-goal field of `goals` beside them and nav_steer_device reads all
        three there.  poses: n x 3 int32 in units; live, plan, steer: the three calls' keywords (steer's min_dist2 and allow_unknown
        default to the plan's).  Returns a dict: 'live' (stats), 'plan' (stats) and 'steer' (the per-pose outputs as nav_steer
        returns them, and stats)."""
        import torch
        self._need_navlive("ssf_navlive_overlay")
        self._need_navplan("ssf_navplan_field")
        self._need_navsteer("ssf_navsteer_rollouts")
        live, plan, sq = dict(live or {}), dict(plan or {}), dict(steer or {})
        state = np.ascontiguousarray(state, np.int8)
        if state.ndim != 2:
            raise SsfError("state is a height x width array, got shape %s" % (state.shape,))
        H, W = state.shape
        poses = np.ascontiguousarray(poses, np.int32)
        if poses.ndim != 2 or poses.shape[1] != 3 or poses.shape[0] < 1:
            raise SsfError("poses are n x 3 (x, y, heading) in units, n >= 1, got shape %s" % (poses.shape,))
        n = poses.shape[0]
        dev = torch.device("cuda")
        if not isinstance(depth, torch.Tensor):
            depth = torch.from_numpy(np.ascontiguousarray(depth, np.uint16 if self.depth_format == "u16" else np.float32).view(
                np.int16 if self.depth_format == "u16" else np.float32)).to(dev)
        if mask is not None and not isinstance(mask, torch.Tensor):
            mask = torch.from_numpy(np.ascontiguousarray(mask, np.uint8)).to(dev)
        d_state = torch.from_numpy(state).to(dev)
        d_dist2 = torch.empty((H, W), dtype=torch.int32, device=dev)
        d_cost = torch.empty((H, W), dtype=torch.int32, device=dev)       # (uint32 words)
        live_stats = self.nav_live_device(depth, d_state, W, H, mask=mask, state_out=d_state, dist2=d_dist2, **live)
        plan_stats = self.nav_plan_device(d_state, d_dist2, W, H, goals, None, cost=d_cost, **plan)
        for nm in ("min_dist2", "allow_unknown"):
            sq.setdefault(nm, plan.get(nm, 0))
        p = self._navsteer_params(True, W, H, n, sq)
        T = min(max(p.n_steps, 0), 256)
        d_poses = torch.from_numpy(poses).to(dev)
        d_targets = None if targets is None else torch.from_numpy(np.ascontiguousarray(targets, np.int32)).to(dev)
        o = {nm: torch.zeros(self._navsteer_shape(kind, tail, n, 1, T), dtype=torch.int64 if dt is np.int64 else torch.int32, device=dev)
             for nm, dt, kind, tail in NAVSTEER_OUTPUTS if kind == "pose"}
        steer_stats = self.nav_steer_device(d_state, d_dist2, W, H, d_poses, n, cost=d_cost, targets=d_targets, **dict(o, **sq))
        got = {nm: a.cpu().numpy() for nm, a in o.items()}
        got["best_traj"] = [got["best_traj"][i, :got["best_len"][i]].copy() for i in range(n)]
        got["stats"] = steer_stats
        return dict(live=dict(stats=live_stats), plan=dict(stats=plan_stats), steer=got)

    # ---- an oriented footprint on the navigation grid: heading layers and rollouts over them (include/ssf_navfoot.h) ----
    def _need_navfoot(self, symbol):
        if not self.L.has_navfoot:
            raise SsfError("%s does not export %s: it holds no footprint (include/ssf_navfoot.h: libssf_hip_foot.so, binding.load_foot)"
                           % (self.L.path, symbol))

    def _navfoot_params(self, on_device, width, height, params):
        p = SsfNavFootParams()
        self._ck(self.L.lib.ssf_navfoot_default_params(self.h, C.byref(p)), "ssf_navfoot_default_params")
        kinds = dict(p._fields_)
        for nm, val in params.items():
            if nm not in kinds or nm in ("width", "height", "on_device"):
                raise SsfError("unknown footprint parameter %r" % nm)
            setattr(p, nm, int(val))
        p.width, p.height, p.on_device = int(width), int(height), int(bool(on_device))
        return p

    def _navfoot_layers(self, p, state, free_mask, n_free):
        st = SsfNavFootStats()
        out = SsfNavFootOut(free_mask, n_free)
        self._ck(self.L.lib.ssf_navfoot_layers(self.h, C.byref(p), state, C.byref(out), C.byref(st)), "ssf_navfoot_layers")
        return st.as_dict()

    def nav_foot(self, state, outputs=("free_mask",), **params):
        """The heading layers of a rectangular footprint (ssf_navfoot_layers), host arrays.  state H x W int8 as the grid calls or
        nav_live return it.  params: the fields of ssf_navfoot_params by name (front, back, left, right, pad in sub-units:
        nav_foot_units, nav_foot_pad; n_headings; allow_unknown).  Returns a dict of the requested outputs ('free_mask' H x W uint32:
        bit b set iff the footprint at heading bin b centred on the cell stands on clear cells only; 'n_free' H x W uint8) and 'stats'."""
        self._need_navfoot("ssf_navfoot_layers")
        bad = [nm for nm in outputs if nm not in ("free_mask", "n_free")]
        if bad:
            raise SsfError("unknown footprint outputs %s (known: free_mask, n_free)" % (bad,))
        state = np.ascontiguousarray(state, np.int8)
        if state.ndim != 2:
            raise SsfError("state is an H x W array, got shape %s" % (state.shape,))
        H, W = state.shape
        p = self._navfoot_params(False, W, H, params)
        out = {}
        if "free_mask" in outputs:
            out["free_mask"] = np.zeros((H, W), np.uint32)
        if "n_free" in outputs:
            out["n_free"] = np.zeros((H, W), np.uint8)
        out["stats"] = self._navfoot_layers(p, _ptr(state), _ptr(out.get("free_mask")), _ptr(out.get("n_free")))
        return out

    def nav_foot_device(self, state, width, height, free_mask=None, n_free=None, **params):
        """ssf_navfoot_layers on device memory: state and each output are a contiguous torch tensor on the device or the device address
        (int) of a buffer of the shape and dtype nav_foot works on (free_mask: 4-byte words; outputs may be None, not both):
        nav_live_device's state is read where it lies.  Returns the stats dict."""
        self._need_navfoot("ssf_navfoot_layers")
        p = self._navfoot_params(True, width, height, params)
        addr = lambda t: None if t is None else C.c_void_p(int(t) if isinstance(t, int) else t.data_ptr())
        return self._navfoot_layers(p, addr(state), addr(free_mask), addr(n_free))

    def nav_foot_default_params(self):
        """ssf_navfoot_default_params as a dict"""
        self._need_navfoot("ssf_navfoot_default_params")
        p = SsfNavFootParams()
        self._ck(self.L.lib.ssf_navfoot_default_params(self.h, C.byref(p)), "ssf_navfoot_default_params")
        return {nm: getattr(p, nm) for nm, _ in p._fields_}

    @staticmethod
    def nav_foot_pad(front, back, left, right, n_headings):
        """The pad (sub-units, pure host arithmetic) that makes the layers conservative for any position in the cell a pose lies in and
        any heading in the bin its heading lies in: ceil(2 * 724.1 + rho * pi / n_headings), rho the distance of the farthest corner
        (include/ssf_navfoot.h step 1).  The call refuses a pad above 4096: a long body needs more headings."""
        if int(n_headings) not in NAVFOOT_HEADINGS or min(front, back, left, right) < 0:
            raise SsfError("nav_foot_pad takes sides >= 0 in sub-units and n_headings one of %s" % (NAVFOOT_HEADINGS,))
        rho = float(np.hypot(max(front, back), max(left, right)))
        return int(np.ceil(2 * 724.1 + rho * np.pi / int(n_headings)))

    @staticmethod
    def nav_foot_units(front_m, back_m, left_m, right_m, res):
        """A footprint in metres from the robot's centre in the call's sub-units (pure host arithmetic), each side rounded up:
        dict(front, back, left, right), nav_foot's keywords"""
        if not res > 0 or min(front_m, back_m, left_m, right_m) < 0:
            raise SsfError("nav_foot_units takes four sides >= 0 in metres and res > 0")
        return {nm: int(np.ceil(v / res * NAVSTEER_SUBUNITS)) for nm, v in (("front", front_m), ("back", back_m), ("left", left_m), ("right", right_m))}

    def nav_foot_steer(self, free_mask, dist2, poses, n_headings, cost=None, targets=None, outputs=NAVSTEER_POSE_OUTPUTS, **params):
        """nav_steer with the oriented footprint in the place of the disc (ssf_navfoot_rollouts), host arrays: free_mask H x W uint32 as
        nav_foot returns it for n_headings bins.  A cell is traversable for a step iff its mask holds every bin the heading sweeps in
        that step and dist2 >= min_dist2.  Everything else, the outputs included, is nav_steer's."""
        self._need_navfoot("ssf_navfoot_rollouts")
        return self._nav_steer_host(free_mask, np.uint32, "free_mask", n_headings, dist2, poses, cost, targets, outputs, params)

    def nav_foot_steer_device(self, free_mask, dist2, width, height, poses, n_poses, n_headings, cost=None, targets=None, best=None, best_cmd=None,
                              best_score=None, n_admissible=None, pose_status=None, best_len=None, best_traj=None, cand_free=None, cand_min_d=None,
                              cand_end=None, cand_end_cost=None, cand_score=None, **params):
        """ssf_navfoot_rollouts on device memory, as nav_steer_device: nav_foot_device's free_mask is read where it lies.  Returns the
        stats dict."""
        self._need_navfoot("ssf_navfoot_rollouts")
        p = self._navsteer_params(True, width, height, n_poses, params)
        addr = lambda t: None if t is None else C.c_void_p(int(t) if isinstance(t, int) else t.data_ptr())
        return self._navsteer_rollouts(p, addr(free_mask), addr(dist2), addr(cost), addr(poses), addr(targets),
                                       dict(best=addr(best), best_cmd=addr(best_cmd), best_score=addr(best_score), n_admissible=addr(n_admissible),
                                            pose_status=addr(pose_status), best_len=addr(best_len), best_traj=addr(best_traj), cand_free=addr(cand_free),
                                            cand_min_d=addr(cand_min_d), cand_end=addr(cand_end), cand_end_cost=addr(cand_end_cost),
                                            cand_score=addr(cand_score)), n_headings)

    def nav_live_foot_steer(self, depth, state, goals, poses, foot, targets=None, mask=None, live=None, plan=None, steer=None, keep_mask=False):
        """Overlay, plan, heading layers and rollouts with nothing but the command leaving the device: nav_live_steer with
        nav_foot_device between the plan and the rollouts.  foot: nav_foot's keywords (front, back, left, right, n_headings; pad
        defaults to nav_foot_pad's, allow_unknown to the plan's).  The plan is the disc's by its own min_dist2 (the inscribed radius).
        Returns a dict: 'live', 'plan' and 'foot' (stats; with keep_mask also 'free_mask', copied out) and 'steer' (the per-pose
        outputs as nav_steer returns them, and stats)."""
        import torch
        self._need_navlive("ssf_navlive_overlay")
        self._need_navplan("ssf_navplan_field")
        self._need_navfoot("ssf_navfoot_rollouts")
        live, plan, fq, sq = dict(live or {}), dict(plan or {}), dict(foot or {}), dict(steer or {})
        state = np.ascontiguousarray(state, np.int8)
        if state.ndim != 2:
            raise SsfError("state is a height x width array, got shape %s" % (state.shape,))
        H, W = state.shape
        poses = np.ascontiguousarray(poses, np.int32)
        if poses.ndim != 2 or poses.shape[1] != 3 or poses.shape[0] < 1:
            raise SsfError("poses are n x 3 (x, y, heading) in units, n >= 1, got shape %s" % (poses.shape,))
        n = poses.shape[0]
        fq.setdefault("n_headings", self.nav_foot_default_params()["n_headings"])
        fq.setdefault("allow_unknown", plan.get("allow_unknown", 0))
        fq.setdefault("pad", self.nav_foot_pad(fq.get("front", 0), fq.get("back", 0), fq.get("left", 0), fq.get("right", 0), fq["n_headings"]))
        dev = torch.device("cuda")
        if not isinstance(depth, torch.Tensor):
            depth = torch.from_numpy(np.ascontiguousarray(depth, np.uint16 if self.depth_format == "u16" else np.float32).view(
                np.int16 if self.depth_format == "u16" else np.float32)).to(dev)
        if mask is not None and not isinstance(mask, torch.Tensor):
            mask = torch.from_numpy(np.ascontiguousarray(mask, np.uint8)).to(dev)
        d_state = torch.from_numpy(state).to(dev)
        d_dist2 = torch.empty((H, W), dtype=torch.int32, device=dev)
        d_cost = torch.empty((H, W), dtype=torch.int32, device=dev)       # (uint32 words)
        d_mask = torch.empty((H, W), dtype=torch.int32, device=dev)       # (uint32 words)
        live_stats = self.nav_live_device(depth, d_state, W, H, mask=mask, state_out=d_state, dist2=d_dist2, **live)
        plan_stats = self.nav_plan_device(d_state, d_dist2, W, H, goals, None, cost=d_cost, **plan)
        foot_stats = self.nav_foot_device(d_state, W, H, free_mask=d_mask, **fq)
        for nm in ("min_dist2", "allow_unknown"):
            sq.setdefault(nm, plan.get(nm, 0))
        p = self._navsteer_params(True, W, H, n, sq)
        T = min(max(p.n_steps, 0), 256)
        d_poses = torch.from_numpy(poses).to(dev)
        d_targets = None if targets is None else torch.from_numpy(np.ascontiguousarray(targets, np.int32)).to(dev)
        o = {nm: torch.zeros(self._navsteer_shape(kind, tail, n, 1, T), dtype=torch.int64 if dt is np.int64 else torch.int32, device=dev)
             for nm, dt, kind, tail in NAVSTEER_OUTPUTS if kind == "pose"}
        steer_stats = self.nav_foot_steer_device(d_mask, d_dist2, W, H, d_poses, n, fq["n_headings"], cost=d_cost, targets=d_targets, **dict(o, **sq))
        got = {nm: a.cpu().numpy() for nm, a in o.items()}
        got["best_traj"] = [got["best_traj"][i, :got["best_len"][i]].copy() for i in range(n)]
        got["stats"] = steer_stats
        res = dict(live=dict(stats=live_stats), plan=dict(stats=plan_stats), foot=dict(stats=foot_stats), steer=got)
        if keep_mask:
            res["foot"]["free_mask"] = d_mask.cpu().numpy().view(np.uint32)
        return res

    # ---- plan over (x, y, heading): the cost-to-goal field over (cell, heading bin) and the state paths (include/ssf_navpose.h) ----
    def _need_navpose(self, symbol):
        if not self.L.has_navpose:
            raise SsfError("%s does not export %s: it plans over no headings (include/ssf_navpose.h: libssf_hip_pose.so, binding.load_pose)"
                           % (self.L.path, symbol))

    @staticmethod
    def _triple_list(a, what):
        if a is None or len(a) == 0:
            return np.zeros((0, 3), np.int32)
        a = np.asarray(a)
        if a.ndim != 2 or a.shape[1] != 3:
            raise SsfError("%s are n x 3, got shape %s" % (what, a.shape))
        return np.ascontiguousarray(a, np.int32)

    def _navpose_params(self, on_device, width, height, goals, starts, params):
        """(SsfNavPoseParams, the goal and start arrays it points into).  goals: n x 3 (ix, iy, bin; bin -1 = any); starts: n x 3 poses
        (x, y, heading) in units; host memory both; params: the other fields of ssf_navpose_params by name, each at
        ssf_navpose_default_params' value when missing."""
        p = SsfNavPoseParams()
        self._ck(self.L.lib.ssf_navpose_default_params(self.h, C.byref(p)), "ssf_navpose_default_params")
        g, s = self._triple_list(goals, "goals"), self._triple_list(starts, "starts")
        kinds = dict(p._fields_)
        for nm, val in params.items():
            if nm not in kinds or nm in ("width", "height", "goals", "n_goals", "starts", "n_starts", "on_device"):
                raise SsfError("unknown pose plan parameter %r" % nm)
            setattr(p, nm, int(val))
        p.width, p.height, p.on_device = int(width), int(height), int(bool(on_device))
        p.goals, p.n_goals = (g.ctypes.data if len(g) else None), len(g)
        p.starts, p.n_starts = (s.ctypes.data if len(s) else None), len(s)
        return p, (g, s)

    def _navpose_field(self, p, free_mask, dist2, ptrs):
        st = SsfNavPoseStats()
        out = SsfNavPoseOut(*[ptrs.get(nm) for nm in NAVPOSE_OUTPUT_NAMES])
        self._ck(self.L.lib.ssf_navpose_field(self.h, C.byref(p), free_mask, dist2, C.byref(out), C.byref(st)), "ssf_navpose_field")
        return st.as_dict()

    def nav_pose_plan(self, free_mask, dist2, goals, starts=None, outputs=NAVPOSE_OUTPUT_NAMES, **params):
        """The cost-to-goal field over (cell, heading bin) of an oriented footprint and the state paths down it (ssf_navpose_field),
        host arrays.  free_mask H x W uint32 as nav_foot returns it for n_headings bins, dist2 H x W int32; goals: n x 3 (ix, iy, bin),
        bin -1 = every bin the body fits at; starts: n x 3 poses (x, y, heading) in nav_steer's units.  Returns a dict of the requested
        outputs -- cost B x H x W u32 (0xFFFFFFFF: not reached), cell_cost H x W u32 (the minimum over the bins: nav_foot_steer's
        `cost`), cell_bin H x W u8 (255: none), start_cost, start_status, path_len, path: a list with one (len, 3) int32 array
        (ix, iy, bin) per start -- and 'stats'.  params: n_headings, min_dist2, soft_dist2, near_penalty, move_tol, allow_reverse,
        reverse_cost, turn_cost, max_path."""
        self._need_navpose("ssf_navpose_field")
        bad = [nm for nm in outputs if nm not in NAVPOSE_OUTPUT_NAMES]
        if bad:
            raise SsfError("unknown pose plan outputs %s (known: %s)" % (bad, ", ".join(NAVPOSE_OUTPUT_NAMES)))
        free_mask, dist2 = np.ascontiguousarray(free_mask, np.uint32), np.ascontiguousarray(dist2, np.int32)
        if free_mask.ndim != 2 or dist2.shape != free_mask.shape:
            raise SsfError("free_mask and dist2 are H x W arrays of one shape, got %s and %s" % (free_mask.shape, dist2.shape))
        H, W = free_mask.shape
        p, keep = self._navpose_params(False, W, H, goals, starts, params)
        n, mp = p.n_starts, max(p.max_path, 0)
        B = p.n_headings if p.n_headings in NAVFOOT_HEADINGS and H * W * p.n_headings <= NAVPOSE_MAX_STATES else 1     # (else the call refuses)
        shapes = dict(cost=((B, H, W), np.uint32), cell_cost=((H, W), np.uint32), cell_bin=((H, W), np.uint8), start_cost=((n,), np.uint32),
                      start_status=((n,), np.int32), path_len=((n,), np.int32), path=((n, min(mp, 1 << 20), 3), np.int32))
        want = set(outputs)
        if "path" in want:
            want.add("path_len")                     # (the lengths cut the paths)
        out = {nm: np.zeros(*shapes[nm]) for nm in NAVPOSE_OUTPUT_NAMES if nm in want}
        stats = self._navpose_field(p, _ptr(free_mask), _ptr(dist2), {nm: _ptr(a) for nm, a in out.items()})
        if "path" in out:
            out["path"] = [out["path"][i, :out["path_len"][i]].copy() for i in range(n)]
        if "path_len" not in outputs:
            out.pop("path_len", None)
        out["stats"] = stats
        return out

    def nav_pose_plan_device(self, free_mask, dist2, width, height, goals, starts=None, cost=None, cell_cost=None, cell_bin=None, start_cost=None,
                             start_status=None, path_len=None, path=None, **params):
        """ssf_navpose_field on device memory: free_mask, dist2 and each output are a contiguous torch tensor on the device or the
        device address (int) of a buffer of the shape and dtype nav_pose_plan works on (path: n_starts x max_path x 3 int32; outputs
        may be None, not all): nav_foot_device's free_mask is read where it lies, and cell_cost is nav_foot_steer_device's `cost`.
        goals and starts stay host memory.  Returns the stats dict."""
        self._need_navpose("ssf_navpose_field")
        p, keep = self._navpose_params(True, width, height, goals, starts, params)
        addr = lambda t: None if t is None else C.c_void_p(int(t) if isinstance(t, int) else t.data_ptr())
        return self._navpose_field(p, addr(free_mask), addr(dist2), dict(cost=addr(cost), cell_cost=addr(cell_cost), cell_bin=addr(cell_bin),
                                                                         start_cost=addr(start_cost), start_status=addr(start_status),
                                                                         path_len=addr(path_len), path=addr(path)))

    def nav_pose_default_params(self):
        """ssf_navpose_default_params as a dict"""
        self._need_navpose("ssf_navpose_default_params")
        p = SsfNavPoseParams()
        self._ck(self.L.lib.ssf_navpose_default_params(self.h, C.byref(p)), "ssf_navpose_default_params")
        return {nm: getattr(p, nm) for nm, _ in p._fields_ if nm not in ("goals", "starts")}

    def nav_live_pose_steer(self, depth, state, goals, poses, foot, targets=None, mask=None, live=None, pose=None, steer=None, keep_mask=False,
                            keep_cost=False):
        """Overlay, disc clearance, heading layers, the plan over (x, y, heading) and the rollouts on its cell_cost, with nothing but
        the command leaving the device: nav_live_foot_steer with nav_pose_plan_device in the place of the disc's plan.  goals: n x 3
        (ix, iy, bin), bin -1 = any; foot: nav_foot's keywords (pad defaults to nav_foot_pad's); pose: nav_pose_plan's parameters
        (n_headings is the footprint's).  Returns a dict: 'live', 'foot' and 'pose' (stats; with keep_mask 'free_mask' under 'foot',
        with keep_cost 'cell_cost' under 'pose', copied out) and 'steer' (the per-pose outputs as nav_steer returns them, and stats)."""
        import torch
        self._need_navlive("ssf_navlive_overlay")
        self._need_navfoot("ssf_navfoot_rollouts")
        self._need_navpose("ssf_navpose_field")
        live, pq, fq, sq = dict(live or {}), dict(pose or {}), dict(foot or {}), dict(steer or {})
        state = np.ascontiguousarray(state, np.int8)
        if state.ndim != 2:
            raise SsfError("state is a height x width array, got shape %s" % (state.shape,))
        H, W = state.shape
        poses = np.ascontiguousarray(poses, np.int32)
        if poses.ndim != 2 or poses.shape[1] != 3 or poses.shape[0] < 1:
            raise SsfError("poses are n x 3 (x, y, heading) in units, n >= 1, got shape %s" % (poses.shape,))
        n = poses.shape[0]
        fq.setdefault("n_headings", self.nav_foot_default_params()["n_headings"])
        if pq.setdefault("n_headings", fq["n_headings"]) != fq["n_headings"]:
            raise SsfError("the pose plan's n_headings is the footprint's (%d), got %d" % (fq["n_headings"], pq["n_headings"]))
        fq.setdefault("allow_unknown", sq.get("allow_unknown", 0))
        fq.setdefault("pad", self.nav_foot_pad(fq.get("front", 0), fq.get("back", 0), fq.get("left", 0), fq.get("right", 0), fq["n_headings"]))
        dev = torch.device("cuda")
        if not isinstance(depth, torch.Tensor):
            depth = torch.from_numpy(np.ascontiguousarray(depth, np.uint16 if self.depth_format == "u16" else np.float32).view(
                np.int16 if self.depth_format == "u16" else np.float32)).to(dev)
        if mask is not None and not isinstance(mask, torch.Tensor):
            mask = torch.from_numpy(np.ascontiguousarray(mask, np.uint8)).to(dev)
        d_state = torch.from_numpy(state).to(dev)
        d_dist2 = torch.empty((H, W), dtype=torch.int32, device=dev)
        d_cost = torch.empty((H, W), dtype=torch.int32, device=dev)       # (uint32 words)
        d_mask = torch.empty((H, W), dtype=torch.int32, device=dev)       # (uint32 words)
        live_stats = self.nav_live_device(depth, d_state, W, H, mask=mask, state_out=d_state, dist2=d_dist2, **live)
        foot_stats = self.nav_foot_device(d_state, W, H, free_mask=d_mask, **fq)
        pose_stats = self.nav_pose_plan_device(d_mask, d_dist2, W, H, goals, None, cell_cost=d_cost, **pq)
        sq.setdefault("min_dist2", pq.get("min_dist2", 0))
        sq.setdefault("allow_unknown", fq["allow_unknown"])
        p = self._navsteer_params(True, W, H, n, sq)
        T = min(max(p.n_steps, 0), 256)
        d_poses = torch.from_numpy(poses).to(dev)
        d_targets = None if targets is None else torch.from_numpy(np.ascontiguousarray(targets, np.int32)).to(dev)
        o = {nm: torch.zeros(self._navsteer_shape(kind, tail, n, 1, T), dtype=torch.int64 if dt is np.int64 else torch.int32, device=dev)
             for nm, dt, kind, tail in NAVSTEER_OUTPUTS if kind == "pose"}
        steer_stats = self.nav_foot_steer_device(d_mask, d_dist2, W, H, d_poses, n, fq["n_headings"], cost=d_cost, targets=d_targets, **dict(o, **sq))
        got = {nm: a.cpu().numpy() for nm, a in o.items()}
        got["best_traj"] = [got["best_traj"][i, :got["best_len"][i]].copy() for i in range(n)]
        got["stats"] = steer_stats
        res = dict(live=dict(stats=live_stats), foot=dict(stats=foot_stats), pose=dict(stats=pose_stats), steer=got)
        if keep_mask:
            res["foot"]["free_mask"] = d_mask.cpu().numpy().view(np.uint32)
        if keep_cost:
            res["pose"]["cell_cost"] = d_cost.cpu().numpy().view(np.uint32)
        return res

    # ---- steering among movers: rollouts tested against predicted movers, blobs of the moving pixels (include/ssf_navdyn.h) ----
    def _need_navdyn(self, symbol):
        if not self.L.has_navdyn:
            raise SsfError("%s does not export %s: it sees no movers (include/ssf_navdyn.h: libssf_hip_dyn.so, binding.load_dyn)"
                           % (self.L.path, symbol))

    def _navdyn_params(self, n_movers, params):
        """(SsfNavDynParams, the rest of `params`): mover_cap and mover_weight taken out of a steering call's keywords, each at
        ssf_navdyn_default_params' value when missing"""
        dp = SsfNavDynParams()
        self._ck(self.L.lib.ssf_navdyn_default_params(self.h, C.byref(dp)), "ssf_navdyn_default_params")
        rest = dict(params)
        for nm in ("mover_cap", "mover_weight"):
            if nm in rest:
                setattr(dp, nm, int(rest.pop(nm)))
        dp.n_movers = int(n_movers)
        return dp, rest

    def _navdyn_rollouts(self, p, dp, grid, dist2, cost, poses, targets, movers, ptrs, n_headings=None):
        """the disc's rollouts among movers over `grid` = state, or with n_headings the footprint's over the mask given in its place"""
        st, dst = SsfNavSteerStats(), SsfNavDynStats()
        out = SsfNavSteerOut(*[ptrs.get(nm) for nm in NAVSTEER_OUTPUT_NAMES])
        dout = SsfNavDynOut(*[ptrs.get(nm) for nm in NAVDYN_OUTPUT_NAMES])
        if n_headings is None:
            self._ck(self.L.lib.ssf_navdyn_rollouts(self.h, C.byref(p), C.byref(dp), grid, dist2, cost, poses, targets, movers, C.byref(out),
                                                    C.byref(dout), C.byref(st), C.byref(dst)), "ssf_navdyn_rollouts")
        else:
            self._ck(self.L.lib.ssf_navdyn_foot_rollouts(self.h, C.byref(p), C.byref(dp), int(n_headings), grid, dist2, cost, poses, targets, movers,
                                                         C.byref(out), C.byref(dout), C.byref(st), C.byref(dst)), "ssf_navdyn_foot_rollouts")
        return dict(st.as_dict(), **dst.as_dict())

    def _nav_dyn_steer_host(self, grid, grid_dtype, grid_name, n_headings, dist2, poses, movers, cost, targets, outputs, params):
        known = NAVSTEER_OUTPUTS + NAVDYN_OUTPUTS
        bad = [nm for nm in outputs if nm not in [o[0] for o in known]]
        if bad:
            raise SsfError("unknown steering outputs %s (known: %s)" % (bad, ", ".join(o[0] for o in known)))
        grid, dist2 = np.ascontiguousarray(grid, grid_dtype), np.ascontiguousarray(dist2, np.int32)
        if grid.ndim != 2 or dist2.shape != grid.shape:
            raise SsfError("%s and dist2 are H x W arrays of one shape, got %s and %s" % (grid_name, grid.shape, dist2.shape))
        H, W = grid.shape
        poses = np.ascontiguousarray(poses, np.int32)
        if poses.ndim != 2 or poses.shape[1] != 3:
            raise SsfError("poses are n x 3 (x, y, heading) in units, got shape %s" % (poses.shape,))
        n = poses.shape[0]
        if cost is not None:
            cost = np.ascontiguousarray(cost, np.uint32)
            if cost.shape != grid.shape:
                raise SsfError("cost is an H x W array like %s, got %s" % (grid_name, cost.shape))
        if targets is not None:
            targets = np.ascontiguousarray(targets, np.int32)
            if targets.shape != (n, 2):
                raise SsfError("targets are n x 2 (x, y) in units, one per pose, got shape %s" % (targets.shape,))
        movers = np.zeros((0, NAVDYN_MOVER_WORDS), np.int32) if movers is None else np.ascontiguousarray(movers, np.int32)
        if movers.ndim != 2 or movers.shape[1] != NAVDYN_MOVER_WORDS:
            raise SsfError("movers are m x 6 (x, y, vx, vy, r, grow) in units, got shape %s" % (movers.shape,))
        dp, rest = self._navdyn_params(movers.shape[0], params)
        p = self._navsteer_params(False, W, H, n, rest)
        K, T = max(p.n_v, 0) * max(p.n_w, 0), max(p.n_steps, 0)
        if not (0 < K <= 65536 and T <= 256 and n * K <= 1 << 24):
            K = T = 1                                # (the call refuses it: the arrays only have to exist)
        want = set(outputs)
        if "best_traj" in want:
            want.add("best_len")                     # (the counts cut the lists)
        out = {nm: np.zeros(self._navsteer_shape(kind, tail, n, K, T), dt) for nm, dt, kind, tail in known if nm in want}
        stats = self._navdyn_rollouts(p, dp, _ptr(grid), _ptr(dist2), _ptr(cost), _ptr(poses), _ptr(targets),
                                      _ptr(movers) if movers.shape[0] else None, {nm: _ptr(a) for nm, a in out.items()}, n_headings)
        if "best_traj" in out:
            out["best_traj"] = [out["best_traj"][i, :out["best_len"][i]].copy() for i in range(n)]
        if "best_len" not in outputs:
            out.pop("best_len", None)
        out["stats"] = stats
        return out

    def nav_dyn_steer(self, state, dist2, poses, movers=None, cost=None, targets=None, outputs=NAVSTEER_POSE_OUTPUTS + ("best_min_gap",), **params):
        """nav_steer among predicted movers (ssf_navdyn_rollouts), host arrays: movers m x 6 int32 (x, y, vx, vy, r, grow) in sub-units
        and sub-units per step (MoverTracker.update makes them; None or empty: none), one list for all poses.  A step is refused where
        it lies inside a mover's disc of that step, and the score gains mover_weight * the lack of gap below mover_cap.  Outputs:
        nav_steer's and cand_hit, cand_min_gap, best_min_gap; 'stats' gains hit_movers.  params: the fields of ssf_navsteer_params
        and mover_cap, mover_weight by name."""
        self._need_navdyn("ssf_navdyn_rollouts")
        return self._nav_dyn_steer_host(state, np.int8, "state", None, dist2, poses, movers, cost, targets, outputs, params)

    def nav_dyn_foot_steer(self, free_mask, dist2, poses, n_headings, movers=None, cost=None, targets=None,
                           outputs=NAVSTEER_POSE_OUTPUTS + ("best_min_gap",), **params):
        """nav_foot_steer among predicted movers (ssf_navdyn_foot_rollouts), host arrays: nav_dyn_steer with the oriented footprint's
        mask in the place of state.  A mover's r carries the footprint's circumscribed radius."""
        self._need_navdyn("ssf_navdyn_foot_rollouts")
        return self._nav_dyn_steer_host(free_mask, np.uint32, "free_mask", n_headings, dist2, poses, movers, cost, targets, outputs, params)

    def nav_dyn_steer_device(self, state, dist2, width, height, poses, n_poses, movers=None, n_movers=0, n_headings=None, cost=None, targets=None,
                             best=None, best_cmd=None, best_score=None, n_admissible=None, pose_status=None, best_len=None, best_traj=None,
                             cand_free=None, cand_min_d=None, cand_end=None, cand_end_cost=None, cand_score=None, cand_hit=None, cand_min_gap=None,
                             best_min_gap=None, **params):
        """ssf_navdyn_rollouts (with n_headings: ssf_navdyn_foot_rollouts, `state` then the footprint's mask) on device memory, as
        nav_steer_device: movers is a device tensor or address of n_movers x 6 int32, whose values the library does not check.
        Returns the stats dict."""
        self._need_navdyn("ssf_navdyn_rollouts")
        dp, rest = self._navdyn_params(n_movers, params)
        p = self._navsteer_params(True, width, height, n_poses, rest)
        addr = self._dev_addr
        return self._navdyn_rollouts(p, dp, addr(state), addr(dist2), addr(cost), addr(poses), addr(targets), addr(movers),
                                     dict(best=addr(best), best_cmd=addr(best_cmd), best_score=addr(best_score), n_admissible=addr(n_admissible),
                                          pose_status=addr(pose_status), best_len=addr(best_len), best_traj=addr(best_traj), cand_free=addr(cand_free),
                                          cand_min_d=addr(cand_min_d), cand_end=addr(cand_end), cand_end_cost=addr(cand_end_cost),
                                          cand_score=addr(cand_score), cand_hit=addr(cand_hit), cand_min_gap=addr(cand_min_gap),
                                          best_min_gap=addr(best_min_gap)), n_headings)

    def nav_dyn_default_params(self):
        """ssf_navdyn_default_params and ssf_navdyn_default_blob_params as one dict: 'steer' and 'blobs'"""
        self._need_navdyn("ssf_navdyn_default_params")
        dp, bp = SsfNavDynParams(), SsfNavDynBlobParams()
        self._ck(self.L.lib.ssf_navdyn_default_params(self.h, C.byref(dp)), "ssf_navdyn_default_params")
        self._ck(self.L.lib.ssf_navdyn_default_blob_params(self.h, C.byref(bp)), "ssf_navdyn_default_blob_params")
        return dict(steer={nm: getattr(dp, nm) for nm, _ in dp._fields_},
                    blobs={nm: getattr(bp, nm) for nm, _ in bp._fields_ if nm not in ("grid_pose", "cam_pose")})

    def _navdyn_blob_params(self, on_device, frame_on_device, grid_pose=None, cam_pose=None, **kw):
        """(SsfNavDynBlobParams, the pose arrays it points into), as _navlive_params"""
        p = SsfNavDynBlobParams()
        self._ck(self.L.lib.ssf_navdyn_default_blob_params(self.h, C.byref(p)), "ssf_navdyn_default_blob_params")
        keep = []
        for nm, pose in (("grid_pose", grid_pose), ("cam_pose", cam_pose)):
            if pose is not None:
                keep.append(self._pose12(pose, nm))
                setattr(p, nm, keep[-1].ctypes.data)
        kinds = dict(p._fields_)
        for nm, val in kw.items():
            if nm not in kinds or nm in ("grid_pose", "cam_pose", "on_device", "frame_on_device"):
                raise SsfError("unknown blob parameter %r" % nm)
            setattr(p, nm, float(val) if kinds[nm] is C.c_float else int(val))
        p.on_device, p.frame_on_device = int(bool(on_device)), int(bool(frame_on_device))
        return p, keep

    def nav_dyn_blobs(self, depth, mask, label, **kw):
        """The moving pixels of a depth frame as blobs in the grid frame (ssf_navdyn_blobs), host arrays: depth in the handle's input
        format, mask uint8 and label int32 as motion_mask returns them, all of the camera's size.  Returns dict(blobs: k x 8 int32 rows
        (label, n, cx, cy, r, ex, ey, 0) in sub-units, ordered by (-n, label), k = stats['blobs_written']; stats).  Keywords: the
        fields of ssf_navdyn_blob_params by name, grid_pose and cam_pose as nav_live."""
        self._need_navdyn("ssf_navdyn_blobs")
        p, keep = self._navdyn_blob_params(False, False, **kw)
        cw, ch = (p.cam_width, p.cam_height) if p.cam_width else (self.W, self.H)
        depth = np.ascontiguousarray(depth, np.uint16 if self.depth_format == "u16" else np.float32)
        mask, label = np.ascontiguousarray(mask, np.uint8), np.ascontiguousarray(label, np.int32)
        for nm, a in (("depth", depth), ("mask", mask), ("label", label)):
            if a.shape != (ch, cw):
                raise SsfError("%s is a %d x %d image, got shape %s" % (nm, ch, cw, a.shape))
        blobs = np.zeros((NAVDYN_MAX_BLOBS, NAVDYN_BLOB_WORDS), np.int32)
        st = SsfNavDynBlobStats()
        self._ck(self.L.lib.ssf_navdyn_blobs(self.h, C.byref(p), _ptr(depth), _ptr(mask), _ptr(label), _ptr(blobs), C.byref(st)), "ssf_navdyn_blobs")
        stats = st.as_dict()
        return dict(blobs=blobs[:stats["blobs_written"]].copy(), stats=stats)

    def nav_dyn_blobs_device(self, depth, mask, label, blobs=None, **kw):
        """ssf_navdyn_blobs on device images: depth, mask and label are device tensors or addresses (motion_mask_device's outputs are
        read where they lie).  blobs: None (the table comes back as nav_dyn_blobs returns it) or a device tensor or address of
        64 x 8 int32, written on the device.  Returns dict(blobs (None when written on the device), stats)."""
        self._need_navdyn("ssf_navdyn_blobs")
        p, keep = self._navdyn_blob_params(blobs is not None, True, **kw)
        host = np.zeros((NAVDYN_MAX_BLOBS, NAVDYN_BLOB_WORDS), np.int32) if blobs is None else None
        st = SsfNavDynBlobStats()
        self._ck(self.L.lib.ssf_navdyn_blobs(self.h, C.byref(p), self._dev_addr(depth), self._dev_addr(mask), self._dev_addr(label),
                                             _ptr(host) if blobs is None else self._dev_addr(blobs), C.byref(st)), "ssf_navdyn_blobs")
        stats = st.as_dict()
        return dict(blobs=None if host is None else host[:stats["blobs_written"]].copy(), stats=stats)

    def nav_live_dyn_steer(self, depth, state, goals, poses, tracker, steps_since=1, targets=None, motion=None, live=None, blobs=None, plan=None,
                           steer=None, _overlay=None):
        """Motion mask, overlay, blobs, tracker, plan and rollouts among the movers, with nothing but the blob table and the command
        leaving the device: nav_live_steer with the moving pixels taken OUT of the overlay (mask_mode 2: a mover is not stamped as a
        wall where it stands now) and handed to the rollouts as predicted discs instead.  depth: host array in the input format or a
        device tensor; tracker: a MoverTracker, which keeps the blob table from call to call; steps_since: the rollout steps since
        the previous call; motion: motion_mask's params; live, blobs, plan, steer: the four calls' keywords (blobs' grid and camera
        default to live's; steer's min_dist2 and allow_unknown to the plan's).  Returns a dict: 'motion', 'live', 'plan' (stats),
        'blobs' (the table and stats), 'movers' (m x 6) and 'steer' (the per-pose outputs as nav_dyn_steer returns them, and stats)."""
        import torch
        self._need_navlive("ssf_navlive_overlay")
        self._need_navplan("ssf_navplan_field")
        self._need_navdyn("ssf_navdyn_rollouts")
        live, bq, plan, sq = dict(live or {}), dict(blobs or {}), dict(plan or {}), dict(steer or {})
        state = np.ascontiguousarray(state, np.int8)
        if state.ndim != 2:
            raise SsfError("state is a height x width array, got shape %s" % (state.shape,))
        H, W = state.shape
        poses = np.ascontiguousarray(poses, np.int32)
        if poses.ndim != 2 or poses.shape[1] != 3 or poses.shape[0] < 1:
            raise SsfError("poses are n x 3 (x, y, heading) in units, n >= 1, got shape %s" % (poses.shape,))
        n = poses.shape[0]
        dev = torch.device("cuda")
        if not isinstance(depth, torch.Tensor):
            depth = torch.from_numpy(np.ascontiguousarray(depth, np.uint16 if self.depth_format == "u16" else np.float32).view(
                np.int16 if self.depth_format == "u16" else np.float32)).to(dev)
        d_mask = torch.empty((self.H, self.W), dtype=torch.uint8, device=dev)
        d_label = torch.empty((self.H, self.W), dtype=torch.int32, device=dev)
        motion_stats = self.motion_mask_device(depth, mask=d_mask, label=d_label, params=motion)
        d_state = torch.from_numpy(state).to(dev)
        d_dist2 = torch.empty((H, W), dtype=torch.int32, device=dev)
        d_cost = torch.empty((H, W), dtype=torch.int32, device=dev)       # (uint32 words)
        live_stats = (_overlay or self.nav_live_device)(depth, d_state, W, H, mask=d_mask, state_out=d_state, dist2=d_dist2, **dict(live, mask_mode=2))
        for nm in ("grid_pose", "cam_pose", "res", "floor_max", "z_max", "fx", "fy", "cx", "cy", "cam_width", "cam_height", "t_min", "t_max"):
            if nm in live:
                bq.setdefault(nm, live[nm])
        table = self.nav_dyn_blobs_device(depth, d_mask, d_label, width=W, height=H, **bq)
        movers = tracker.update(table["blobs"], steps_since)
        plan_stats = self.nav_plan_device(d_state, d_dist2, W, H, goals, None, cost=d_cost, **plan)
        for nm in ("min_dist2", "allow_unknown"):
            sq.setdefault(nm, plan.get(nm, 0))
        _, rest = self._navdyn_params(0, sq)
        T = min(max(self._navsteer_params(True, W, H, n, rest).n_steps, 0), 256)
        d_poses = torch.from_numpy(poses).to(dev)
        d_targets = None if targets is None else torch.from_numpy(np.ascontiguousarray(targets, np.int32)).to(dev)
        d_movers = torch.from_numpy(movers).to(dev) if movers.shape[0] else None
        o = {nm: torch.zeros(self._navsteer_shape(kind, tail, n, 1, T), dtype=torch.int64 if dt is np.int64 else torch.int32, device=dev)
             for nm, dt, kind, tail in NAVSTEER_OUTPUTS + NAVDYN_OUTPUTS if kind == "pose"}
        steer_stats = self.nav_dyn_steer_device(d_state, d_dist2, W, H, d_poses, n, movers=d_movers, n_movers=movers.shape[0], cost=d_cost,
                                                targets=d_targets, **dict(o, **sq))
        got = {nm: a.cpu().numpy() for nm, a in o.items()}
        got["best_traj"] = [got["best_traj"][i, :got["best_len"][i]].copy() for i in range(n)]
        got["stats"] = steer_stats
        return dict(motion=dict(stats=motion_stats), live=dict(stats=live_stats), plan=dict(stats=plan_stats), blobs=table, movers=movers, steer=got)

    # ---- rays cast through the model: the first disc each ray hits (include/ssf_raycast.h) ------------
    def _need_raycast(self, symbol):
        if not self.L.has_raycast:
            raise SsfError("%s does not export %s: it casts no rays (include/ssf_raycast.h, HIP product only)" % (self.L.path, symbol))

    def _raycast_params(self, on_device, pose=None, visible_only=False, **kw):
        """(SsfRaycastParams, the pose array it points into).  pose: 12 floats or a 3 x 4 [R | t] ray-frame-to-map (None = the
        handle's pose); the other keywords are fields of ssf_raycast_params (t_min, t_max, min_conf, splat_scale, cell,
        hash_bits), each at ssf_raycast_default_params' value when missing."""
        p = SsfRaycastParams()
        self._ck(self.L.lib.ssf_raycast_default_params(self.h, C.byref(p)), "ssf_raycast_default_params")
        keep = None
        if pose is not None:
            pose = np.asarray(pose, np.float32)
            if pose.shape == (3, 4):
                pose = np.concatenate([pose[:, :3].ravel(), pose[:, 3]])
            if pose.size != 12:
                raise SsfError("a ray pose is 12 floats (R row-major, then t) or 3 x 4 [R | t], got shape %s" % (pose.shape,))
            keep = np.ascontiguousarray(pose.ravel(), np.float32)
            p.pose = keep.ctypes.data
        kinds = dict(p._fields_)
        for nm, v in kw.items():
            if nm not in kinds or nm in ("pose", "on_device", "visible_only"):
                raise SsfError("unknown ray cast parameter %r" % nm)
            setattr(p, nm, float(v) if kinds[nm] is C.c_float else int(v))
        p.visible_only, p.on_device = int(bool(visible_only)), int(bool(on_device))
        return p, keep

    def _raycast(self, p, rays, n, ptrs):
        st = SsfRaycastStats()
        self._ck(self.L.lib.ssf_raycast(self.h, C.byref(p), rays, n, *([ptrs.get(nm) for nm in RAYCAST_OUTPUT_NAMES] + [C.byref(st)])),
                 "ssf_raycast")
        return st.as_dict()

    def raycast(self, rays, outputs=RAYCAST_OUTPUT_NAMES, pose=None, **kw):
        """The first disc of the model that each ray hits (ssf_raycast).  rays: n x 6 (origin, direction) in the pose's frame.
        Returns a dict of the requested arrays (t n f32, index n i32, point / normal / color n x 3 f32; a miss: 0, -1, 0) and
        'stats'.  Keywords: _raycast_params."""
        self._need_raycast("ssf_raycast")
        bad = [nm for nm in outputs if nm not in RAYCAST_OUTPUT_NAMES]
        if bad:
            raise SsfError("unknown ray cast outputs %s (known: %s)" % (bad, ", ".join(RAYCAST_OUTPUT_NAMES)))
        rays = np.ascontiguousarray(rays, np.float32)
        if rays.ndim != 2 or rays.shape[1] != 6:
            raise SsfError("rays are n x 6 floats (origin, direction), got shape %s" % (rays.shape,))
        n = len(rays)
        p, keep = self._raycast_params(False, pose=pose, **kw)
        out = {nm: np.empty((n,) + tail, dt) for nm, dt, tail in RAYCAST_OUTPUTS if nm in outputs}
        stats = self._raycast(p, _ptr(rays) if n else None, n, {nm: _ptr(a) for nm, a in out.items()})
        out["stats"] = stats
        return out

    def raycast_device(self, rays, n, t=None, index=None, point=None, normal=None, color=None, pose=None, **kw):
        """ssf_raycast on device memory: rays and each output are a contiguous torch tensor on the device or the device address (int)
        of a buffer of the shape and dtype raycast takes and returns (an output may be None).  Returns the stats dict."""
        self._need_raycast("ssf_raycast")
        p, keep = self._raycast_params(True, pose=pose, **kw)
        addr = lambda a: None if a is None else C.c_void_p(int(a) if isinstance(a, int) else a.data_ptr())
        return self._raycast(p, addr(rays), int(n), dict(t=addr(t), index=addr(index), point=addr(point), normal=addr(normal), color=addr(color)))

    def raycast_default_params(self):
        """ssf_raycast_default_params as a dict"""
        self._need_raycast("ssf_raycast_default_params")
        p = SsfRaycastParams()
        self._ck(self.L.lib.ssf_raycast_default_params(self.h, C.byref(p)), "ssf_raycast_default_params")
        return {nm: getattr(p, nm) for nm, _ in p._fields_ if nm != "pose"}

    # ---- the deformation graph's nodes and per-row binding (include/ssf_graph.h) ------------------
    def _need_graph(self, symbol):
        if not self.L.has_graph:
            raise SsfError("%s does not export %s: it does not build the deformation graph (include/ssf_graph.h, HIP product only)"
                           % (self.L.path, symbol))

    def graph_default_params(self):
        """ssf_graph_default_params as a dict"""
        self._need_graph("ssf_graph_default_params")
        p = SsfGraphParams()
        rc = self.L.lib.ssf_graph_default_params(C.byref(p))
        if rc != 0:
            raise SsfError("ssf_graph_default_params failed (%d)" % rc)
        return {nm: getattr(p, nm) for nm, _ in p._fields_}

    def graph_build(self, stride=50, look=20, min_conf=0.0):
        """Sample the nodes from the model and bind every row to them on the device (ssf_graph_build); returns n_nodes."""
        self._need_graph("ssf_graph_build")
        p = SsfGraphParams(int(stride), int(look), float(min_conf))
        m = C.c_int(0)
        self._ck(self.L.lib.ssf_graph_build(self.h, C.byref(p), C.byref(m)), "ssf_graph_build")
        return m.value

    def graph_info(self):
        """dict(n_nodes, n_rows, valid) of the resident graph"""
        self._need_graph("ssf_graph_info")
        m, n, v = C.c_int(0), C.c_int(0), C.c_int(0)
        self._ck(self.L.lib.ssf_graph_info(self.h, C.byref(m), C.byref(n), C.byref(v)), "ssf_graph_info")
        return {"n_nodes": m.value, "n_rows": n.value, "valid": bool(v.value)}

    def graph_nodes(self, capacity=None):
        """(positions m x 3 f32, t_init m i32, rows m i32): the node table in time order (ssf_graph_get_nodes)"""
        self._need_graph("ssf_graph_get_nodes")
        m = self.graph_info()["n_nodes"] if capacity is None else int(capacity)
        pos, t0, rows = np.empty((max(m, 0), 3), np.float32), np.empty(max(m, 0), np.int32), np.empty(max(m, 0), np.int32)
        self._ck(self.L.lib.ssf_graph_get_nodes(self.h, _ptr(pos), _ptr(t0), _ptr(rows), m), "ssf_graph_get_nodes")
        k = self.graph_info()["n_nodes"]
        return pos[:k], t0[:k], rows[:k]

    def graph_binding(self):
        """(weights4 n x 4 f32, idx4 n x 4 i32): the resident binding of every logical row (ssf_graph_get_binding)"""
        self._need_graph("ssf_graph_get_binding")
        n = self.graph_info()["n_rows"]
        w, i = np.empty((n, 4), np.float32), np.empty((n, 4), np.int32)
        self._ck(self.L.lib.ssf_graph_get_binding(self.h, _ptr(w), _ptr(i), 0), "ssf_graph_get_binding")
        return w, i

    def graph_binding_device(self, weights4, idx4):
        """ssf_graph_get_binding into device memory: the device addresses (int, or None) of n x 4 f32 / n x 4 i32 buffers"""
        self._need_graph("ssf_graph_get_binding")
        ptrs = [None if a is None else C.c_void_p(int(a)) for a in (weights4, idx4)]
        self._ck(self.L.lib.ssf_graph_get_binding(self.h, ptrs[0], ptrs[1], 1), "ssf_graph_get_binding")

    def graph_bind_points(self, points, t_init):
        """(weights4, idx4) of n caller points (n x 3 f32, birth stamps n i32) against the resident nodes (ssf_graph_bind_points)"""
        self._need_graph("ssf_graph_bind_points")
        pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        t0 = np.ascontiguousarray(t_init, np.int32).ravel()
        if len(t0) != len(pts):
            raise SsfError("graph_bind_points: %d points but %d stamps" % (len(pts), len(t0)))
        n = len(pts)
        w, i = np.empty((n, 4), np.float32), np.empty((n, 4), np.int32)
        self._ck(self.L.lib.ssf_graph_bind_points(self.h, _ptr(pts), _ptr(t0), n, _ptr(w), _ptr(i)), "ssf_graph_bind_points")
        return w, i

    def graph_apply(self, node_rot, node_trans):
        """Deform the model through the resident nodes and binding (ssf_graph_apply): node_rot m x 9 (or m x 3 x 3), node_trans m x 3"""
        self._need_graph("ssf_graph_apply")
        m = self.graph_info()["n_nodes"]
        R, t = np.ascontiguousarray(node_rot, np.float32), np.ascontiguousarray(node_trans, np.float32)
        if R.size != 9 * m or t.size != 3 * m:
            raise SsfError("graph_apply: the graph has %d nodes; got %d rotation and %d translation floats" % (m, R.size, t.size))
        self._ck(self.L.lib.ssf_graph_apply(self.h, _ptr(R), _ptr(t)), "ssf_graph_apply")

    # ---- the graph's optimisation (include/ssf_graph_solve.h) ----------------------------------------
    def _need_graph_solve(self, symbol):
        if not self.L.has_graph_solve:
            raise SsfError("%s does not export %s: it does not solve the deformation graph (include/ssf_graph_solve.h, HIP product only)"
                           % (self.L.path, symbol))

    def graph_solve_default_params(self):
        """ssf_graph_solve_default_params as a dict"""
        self._need_graph_solve("ssf_graph_solve_default_params")
        p = SsfGraphSolveParams()
        rc = self.L.lib.ssf_graph_solve_default_params(C.byref(p))
        if rc != 0:
            raise SsfError("ssf_graph_solve_default_params failed (%d)" % rc)
        return {nm: getattr(p, nm) for nm, _ in p._fields_}

    def graph_edges(self, capacity=None):
        """m x 4 i32: the four neighbours N(j) of every node (ssf_graph_get_edges)"""
        self._need_graph_solve("ssf_graph_get_edges")
        m = self.graph_info()["n_nodes"] if capacity is None else int(capacity)
        e = np.empty((max(m, 0), 4), np.int32)
        self._ck(self.L.lib.ssf_graph_get_edges(self.h, _ptr(e), m), "ssf_graph_get_edges")
        return e[:self.graph_info()["n_nodes"]]

    def graph_solve(self, src, t_init, dst, **params):
        """Solve the node transforms that take the points src (n x 3 f32, birth stamps t_init n i32) to dst (ssf_graph_solve);
        params override ssf_graph_solve_default_params.  Returns the result record as a dict; the transforms stay on the device
        (graph_transforms, graph_apply_solved)."""
        self._need_graph_solve("ssf_graph_solve")
        p = SsfGraphSolveParams()
        rc = self.L.lib.ssf_graph_solve_default_params(C.byref(p))
        if rc != 0:
            raise SsfError("ssf_graph_solve_default_params failed (%d)" % rc)
        for k, v in params.items():
            if k not in dict(p._fields_):
                raise SsfError("graph_solve: unknown parameter %s" % k)
            setattr(p, k, v)
        s, d = (np.ascontiguousarray(a, np.float32).reshape(-1, 3) for a in (src, dst))
        t0 = np.ascontiguousarray(t_init, np.int32).ravel()
        if len(t0) != len(s) or len(d) != len(s):
            raise SsfError("graph_solve: %d sources, %d stamps, %d targets" % (len(s), len(t0), len(d)))
        res = SsfGraphSolveResult()
        self._ck(self.L.lib.ssf_graph_solve(self.h, C.byref(p), _ptr(s), _ptr(t0), _ptr(d), len(s), C.byref(res)), "ssf_graph_solve")
        return res.as_dict()

    def graph_transforms(self, capacity=None):
        """(node_rotations m x 9 f32, node_translations m x 3 f32) of the last solve (ssf_graph_get_transforms)"""
        self._need_graph_solve("ssf_graph_get_transforms")
        m = self.graph_info()["n_nodes"] if capacity is None else int(capacity)
        R, t = np.empty((max(m, 0), 9), np.float32), np.empty((max(m, 0), 3), np.float32)
        self._ck(self.L.lib.ssf_graph_get_transforms(self.h, _ptr(R), _ptr(t), m), "ssf_graph_get_transforms")
        k = self.graph_info()["n_nodes"]
        return R[:k], t[:k]

    def graph_apply_solved(self):
        """Deform the model by the resident solved transforms (ssf_graph_apply_solved); the graph is stale afterwards"""
        self._need_graph_solve("ssf_graph_apply_solved")
        self._ck(self.L.lib.ssf_graph_apply_solved(self.h), "ssf_graph_apply_solved")

    # ---- whole frame -------------------------------------------------------------------------
    def process_frame(self, rgb, depth, prior_pose=None, dynamic_mask=None, pixel_mask=None, motion=None, odometry=None):
        """odometry: None, or True / a dict of ssf_odometry_params fields: the pose prior comes from the library's dense odometry
        against the frame before (ssf_process_frame_odometry, ssf_odometry.h; combines with motion, whose mask is then rendered at
        that prior; not with prior_pose or the masks).
        pixel_mask: H x W uint8 (non-zero = moving object), voted onto the frame's superpixels (ssf_dynamic.h);
        not together with dynamic_mask (one byte per superpixel).  motion: None, or True / a dict of ssf_motion_params fields:
        the pixel mask is detected on the device from this depth and the map (ssf_process_frame_motion, ssf_motion.h)."""
        rgb, depth = self._frame(rgb, depth)
        prior = None if prior_pose is None else np.ascontiguousarray(prior_pose, np.float32)
        if odometry is not None:
            if prior is not None or pixel_mask is not None or dynamic_mask is not None:
                raise SsfError("odometry makes the pose prior itself and combines only with motion: not with prior_pose, pixel_mask or dynamic_mask")
            return self._process_frame_odometry(_ptr(rgb), _ptr(depth), False, odometry, motion).as_dict()
        if motion is not None:
            if pixel_mask is not None or dynamic_mask is not None:
                raise SsfError("motion does not combine with pixel_mask or dynamic_mask: it makes the frame's pixel mask itself")
            return self._process_frame_motion(_ptr(rgb), _ptr(depth), False, prior, motion).as_dict()
        if pixel_mask is not None:
            self._need_pixmask("ssf_process_frame_pixmask")
            if dynamic_mask is not None:
                raise SsfError("pixel_mask and dynamic_mask do not combine: the pixel-mask calls take no per-superpixel mask")
            pm, keep = self._pixel_mask(pixel_mask)
            res = SsfFrameResult()
            self._ck(self.L.lib.ssf_process_frame_pixmask(self.h, _ptr(rgb), _ptr(depth), 0, _ptr(prior), pm, C.byref(res)),
                     "ssf_process_frame_pixmask")
            return res.as_dict()
        mask = None if dynamic_mask is None else np.ascontiguousarray(dynamic_mask, np.uint8)
        res = SsfFrameResult()
        self._ck(self.L.lib.ssf_process_frame(self.h, _ptr(rgb), _ptr(depth), _ptr(prior), _ptr(mask),
                                              C.byref(res)), "ssf_process_frame")
        return res.as_dict()

    def process_frame_device(self, d_rgb_ptr, d_depth_ptr, prior_pose=None, pixel_mask=None, motion=None, odometry=None):
        """pixel_mask: None or the device address of an H x W uint8 pixel mask (ssf_dynamic.h); motion, odometry: as process_frame"""
        prior = None if prior_pose is None else np.ascontiguousarray(prior_pose, np.float32)
        if odometry is not None:
            if prior is not None or pixel_mask is not None:
                raise SsfError("odometry makes the pose prior itself and combines only with motion: not with prior_pose or pixel_mask")
            return self._process_frame_odometry(C.c_void_p(d_rgb_ptr), C.c_void_p(d_depth_ptr), True, odometry, motion)
        if motion is not None:
            if pixel_mask is not None:
                raise SsfError("motion does not combine with pixel_mask: it makes the frame's pixel mask itself")
            return self._process_frame_motion(C.c_void_p(d_rgb_ptr), C.c_void_p(d_depth_ptr), True, prior, motion)
        res = SsfFrameResult()
        if pixel_mask is not None:
            self._need_pixmask("ssf_process_frame_pixmask")
            pm, _ = self._pixel_mask(pixel_mask, on_device=True)
            self._ck(self.L.lib.ssf_process_frame_pixmask(self.h, C.c_void_p(d_rgb_ptr), C.c_void_p(d_depth_ptr), 1, _ptr(prior), pm,
                                                          C.byref(res)), "ssf_process_frame_pixmask")
            return res
        self._ck(self.L.lib.ssf_process_frame_device(self.h, C.c_void_p(d_rgb_ptr), C.c_void_p(d_depth_ptr),
                                                     _ptr(prior), None, C.byref(res)),
                 "ssf_process_frame_device")
        return res

    # ---- pipelined form ----------------------------------------------------------------------
    def submit_frame(self, rgb, depth, dynamic_mask=None, on_device=False, pixel_mask=None):
        """Enqueue the extract stage of the next frame (asynchronous).  With on_device=True rgb and
        depth are device addresses that must stay valid until the frame has been processed.
        pixel_mask (ssf_dynamic.h): H x W uint8 host array, or a device address with on_device=True."""
        if on_device:
            rp, dp = C.c_void_p(rgb), C.c_void_p(depth)
        else:
            rgb, depth = self._frame(rgb, depth)
            rp, dp = _ptr(rgb), _ptr(depth)
        if pixel_mask is not None:
            self._need_pixmask("ssf_submit_frame_pixmask")
            if dynamic_mask is not None:
                raise SsfError("pixel_mask and dynamic_mask do not combine: the pixel-mask calls take no per-superpixel mask")
            pm, keep = self._pixel_mask(pixel_mask, on_device)
            self._ck(self.L.lib.ssf_submit_frame_pixmask(self.h, rp, dp, 1 if on_device else 0, pm), "ssf_submit_frame_pixmask")
            self._held.append((rgb, depth, keep))
            return
        mask = None if dynamic_mask is None else np.ascontiguousarray(dynamic_mask, np.uint8)
        self._ck(self.L.lib.ssf_submit_frame(self.h, rp, dp, 1 if on_device else 0, _ptr(mask)), "ssf_submit_frame")
        self._held.append((rgb, depth, mask))

    def submit_frame_tables(self, label, plane_depth, frame):
        """The next frame, extracted by ANOTHER rank (ssf_submit_frame_tables): its label map (H x W int32), plane-rendered depth
        (H x W float32) and frame supersurfels (the dict get_frame() returns) take the place of submit_frame's images."""
        label = np.ascontiguousarray(label, np.int32); plane_depth = np.ascontiguousarray(plane_depth, np.float32)
        assert label.shape == (self.H, self.W) and plane_depth.shape == (self.H, self.W) and len(frame["confidences"]) == self.S
        keep = [np.ascontiguousarray(frame[name], dt) for name, _, dt in SURFEL_FIELDS]
        st = SsfSurfels(*[a.ctypes.data_as(C.c_void_p) for a in keep])
        self._ck(self.L.lib.ssf_submit_frame_tables(self.h, _ptr(label), _ptr(plane_depth), C.byref(st), 0), "ssf_submit_frame_tables")

    def prepare_sequence(self, rgb_ptrs, depth_ptrs):
        """ctypes argument arrays of a sequence (built ahead, e.g. outside a timed region): (rgb, depth, results, n)"""
        n = len(rgb_ptrs)
        return (C.c_void_p * n)(*rgb_ptrs), (C.c_void_p * n)(*depth_ptrs), (SsfFrameResult * n)(), n

    def process_prepared(self, prepared, on_device=True, mask_ptrs=None):
        """ssf_process_sequence on arrays from prepare_sequence; returns the raw SsfFrameResult array (as_dict() each).
        mask_ptrs: None, or one pixel-mask address (or None / 0) per frame: ssf_process_sequence_pixmask."""
        pr, pd, res, n = prepared
        if mask_ptrs is None:
            self._ck(self.L.lib.ssf_process_sequence(self.h, pr, pd, n, 1 if on_device else 0, res), "ssf_process_sequence")
            return res
        self._need_pixmask("ssf_process_sequence_pixmask")
        if len(mask_ptrs) != n:
            raise SsfError("mask_ptrs has %d entries for %d frames" % (len(mask_ptrs), n))
        pm = (C.c_void_p * n)(*[int(q) if q else None for q in mask_ptrs])
        self._ck(self.L.lib.ssf_process_sequence_pixmask(self.h, pr, pd, pm, n, 1 if on_device else 0, res), "ssf_process_sequence_pixmask")
        return res

    def process_sequence(self, rgb_ptrs, depth_ptrs, on_device=True, mask_ptrs=None):
        """The whole submit-ahead / process-in-order loop in native code.  rgb_ptrs / depth_ptrs: raw addresses
        (device pointers when on_device, else addresses of contiguous host arrays).  mask_ptrs: None, or per frame the
        address of its H x W uint8 pixel mask (same kind as the frames) or None (ssf_dynamic.h).  Returns a list of result dicts."""
        return [r.as_dict() for r in self.process_prepared(self.prepare_sequence(rgb_ptrs, depth_ptrs), on_device, mask_ptrs)]

    def host_masks(self, masks):
        """Host pixel masks for process_sequence(mask_ptrs=...), checked like process_frame's: returns (mask_ptrs, keep) -- an
        entry None stays None; `keep` holds the arrays and must outlive the call."""
        keep = [None if m is None else self._pixel_mask(m)[1] for m in masks]
        return [None if m is None else m.ctypes.data for m in keep], keep

    def host_sequence(self, rgbs, depths):
        """Host frames for prepare_sequence / process_sequence(on_device=False), checked against the input format like
        process_frame's: returns (rgb_ptrs, depth_ptrs, keep) -- `keep` holds the arrays and must outlive the call."""
        keep = [self._frame(r, d) for r, d in zip(rgbs, depths)]
        return [a.ctypes.data for a, _ in keep], [b.ctypes.data for _, b in keep], keep

    def process_submitted(self, prior_pose=None):
        """ICP + association + fusion of the oldest submitted frame; returns its SsfFrameResult."""
        prior = None if prior_pose is None else np.ascontiguousarray(prior_pose, np.float32)
        res = SsfFrameResult()
        self._ck(self.L.lib.ssf_process_submitted(self.h, _ptr(prior), C.byref(res)), "ssf_process_submitted")
        if self._held:
            self._held.pop(0)
        return res

    def pending_frames(self):
        return int(self.L.lib.ssf_pending_frames(self.h))

    def can_submit(self):
        return bool(self.L.lib.ssf_can_submit(self.h))

    def pipeline_capacity(self):
        return int(self.L.lib.ssf_pipeline_capacity(self.h))

    # ---- stage seams -------------------------------------------------------------------------
    def stage_extract(self, rgb, depth, dynamic_mask=None, on_device=False, pixel_mask=None):
        if pixel_mask is not None:
            self._need_pixmask("ssf_stage_extract_pixmask")
            if dynamic_mask is not None:
                raise SsfError("pixel_mask and dynamic_mask do not combine: the pixel-mask calls take no per-superpixel mask")
            if on_device:
                rp, dp = C.c_void_p(rgb), C.c_void_p(depth)
            else:
                rgb, depth = self._frame(rgb, depth)
                rp, dp = _ptr(rgb), _ptr(depth)
            pm, keep = self._pixel_mask(pixel_mask, on_device)
            self._ck(self.L.lib.ssf_stage_extract_pixmask(self.h, rp, dp, 1 if on_device else 0, pm), "ssf_stage_extract_pixmask")
            return
        if on_device:
            rp, dp = C.c_void_p(rgb), C.c_void_p(depth)
        elif (self.color_format, self.depth_format) == ("rgb8", "f32"):
            rgb = np.ascontiguousarray(rgb, np.uint8)
            depth = np.ascontiguousarray(depth, np.float32)
            rp, dp = _ptr(rgb), _ptr(depth)
        else:
            rgb, depth = self._frame(rgb, depth)
            rp, dp = _ptr(rgb), _ptr(depth)
        mask = None if dynamic_mask is None else np.ascontiguousarray(dynamic_mask, np.uint8)
        self._ck(self.L.lib.ssf_stage_extract(self.h, rp, dp, 1 if on_device else 0, _ptr(mask)), "ssf_stage_extract")

    def debug_recentre(self):
        self._ck(self.L.lib.ssf_debug_recentre(self.h), "ssf_debug_recentre")

    def debug_recentre_count(self):
        return int(self.L.lib.ssf_debug_recentre_count(self.h))

    def set_max_passes(self, n):
        self._ck(self.L.lib.ssf_debug_set_max_passes(self.h, n), "ssf_debug_set_max_passes")

    def set_bin_min_rows(self, n):
        """visible rows from which a frame's tracking streams a tile-sorted copy of them (product default: 400 000; 0 = always, < 0 = never)"""
        self._ck(self.L.lib.ssf_debug_set_bin_min_rows(self.h, int(n)), "ssf_debug_set_bin_min_rows")

    def set_resident_icp_max_rows(self, n):
        """visible rows up to which a frame's ICP iterations and association run in one resident launch (product default and ceiling:
        262 144; 0 = never)"""
        if not self.L.has_track:
            raise SsfError("this library has no resident ICP launch (include/ssf_track.h: HIP product only)")
        self._ck(self.L.lib.ssf_debug_set_resident_icp_max_rows(self.h, int(n)), "ssf_debug_set_resident_icp_max_rows")

    def resident_icp_frames(self):
        """frames whose ICP iterations ran in a resident launch since the handle was created"""
        if not self.L.has_track:
            raise SsfError("this library has no resident ICP launch (include/ssf_track.h: HIP product only)")
        return int(self.L.lib.ssf_resident_icp_frames(self.h))

    def resident_icp_ahead_frames(self):
        """... and those of them whose launch started behind a first record made by the frame before"""
        if not self.L.has_track:
            raise SsfError("this library has no resident ICP launch (include/ssf_track.h: HIP product only)")
        return int(self.L.lib.ssf_resident_icp_ahead_frames(self.h))

    def tile_copy_frames(self):
        """frames whose tracking made the tile-sorted copy of the visible rows since the handle was created"""
        if not self.L.has_track:
            raise SsfError("this library has no tile-sorted copy (include/ssf_track.h: HIP product only)")
        return int(self.L.lib.ssf_tile_copy_frames(self.h))

    def debug_tile_copy(self, T12):
        """ssf_debug_tile_copy: the visible rows sorted by the tile they project to under T12 (12 floats: R row-major, then t).
        Returns dict(records: n_visible x 12 float32 (position, confidence | Lab, row index as integer bits | normal, 0), totals:
        uint32 rows per bin, ceil(W / 32) * ceil(H / 32) + 1 of them, lab_src: n_visible x 3 float32, the stored Lab in array order)"""
        if not self.L.has_track:
            raise SsfError("this library has no tile-sorted copy (include/ssf_track.h: HIP product only)")
        T12 = np.ascontiguousarray(T12, np.float32).reshape(-1)
        assert T12.size == 12, T12.size
        n = self.counts()["n_visible"]
        records, lab_src = np.zeros((max(n, 1), 12), np.float32)[:n], np.zeros((max(n, 1), 3), np.float32)[:n]
        totals = np.zeros(((self.W + 31) // 32) * ((self.H + 31) // 32) + 1, np.uint32)
        self._ck(self.L.lib.ssf_debug_tile_copy(self.h, _ptr(T12), _ptr(records), _ptr(totals), _ptr(lab_src)), "ssf_debug_tile_copy")
        return dict(records=records, totals=totals, lab_src=lab_src)

    def set_shard(self, id_offset, global_n_model, global_n_visible):
        self._ck(self.L.lib.ssf_stage_set_shard(self.h, id_offset, global_n_model, global_n_visible), "ssf_stage_set_shard")

    def icp_begin(self, prior_pose=None):
        prior = None if prior_pose is None else np.ascontiguousarray(prior_pose, np.float32)
        self._ck(self.L.lib.ssf_stage_icp_begin(self.h, _ptr(prior)), "ssf_stage_icp_begin")

    def icp_accumulate(self):
        sums = np.zeros(ICP_RECORD, np.int64)
        self._ck(self.L.lib.ssf_stage_icp_accumulate(self.h, _ptr(sums)), "ssf_stage_icp_accumulate")
        return sums

    def icp_update(self, sums):
        sums = np.ascontiguousarray(sums, np.int64)
        again = C.c_int(0)
        self._ck(self.L.lib.ssf_stage_icp_update(self.h, _ptr(sums), C.byref(again)), "ssf_stage_icp_update")
        return bool(again.value)

    def icp_end(self):
        valid = C.c_int(0)
        self._ck(self.L.lib.ssf_stage_icp_end(self.h, C.byref(valid)), "ssf_stage_icp_end")
        return bool(valid.value)

    def match(self):
        best = np.zeros(self.S, np.uint64)
        matched = np.zeros(self.S, np.uint8)
        self._ck(self.L.lib.ssf_stage_match(self.h, _ptr(best), _ptr(matched)), "ssf_stage_match")
        return best, matched

    def fuse(self, best, matched):
        best = np.ascontiguousarray(best, np.uint64)
        matched = np.ascontiguousarray(matched, np.uint8)
        res = SsfFrameResult()
        self._ck(self.L.lib.ssf_stage_fuse(self.h, _ptr(best), _ptr(matched), C.byref(res)), "ssf_stage_fuse")
        return res.as_dict()

    def fuse_begin(self, best, matched):
        """first half of the fuse stage; returns this shard's migrant table (S x MIGRANT_WORDS int32, see ssf.h)"""
        best = np.ascontiguousarray(best, np.uint64)
        matched = np.ascontiguousarray(matched, np.uint8)
        table = np.zeros((self.S, MIGRANT_WORDS), np.int32)
        self._ck(self.L.lib.ssf_stage_fuse_begin(self.h, _ptr(best), _ptr(matched), _ptr(table)), "ssf_stage_fuse_begin")
        return table

    def fuse_end(self, table=None):
        """second half: rows addressed to this rank in the (rank-reduced) table arrive, then classify + reorder"""
        table = None if table is None else np.ascontiguousarray(table, np.int32)
        res = SsfFrameResult()
        self._ck(self.L.lib.ssf_stage_fuse_end(self.h, _ptr(table), C.byref(res)), "ssf_stage_fuse_end")
        return res.as_dict()

    def fuse_begin_device(self, d_best_ptr, d_matched_ptr, d_table_ptr):
        self._ck(self.L.lib.ssf_stage_fuse_begin_device(self.h, C.c_void_p(d_best_ptr), C.c_void_p(d_matched_ptr), C.c_void_p(d_table_ptr)),
                 "ssf_stage_fuse_begin_device")

    def fuse_end_device(self, d_table_ptr):
        res = SsfFrameResult()
        self._ck(self.L.lib.ssf_stage_fuse_end_device(self.h, C.c_void_p(d_table_ptr), C.byref(res)), "ssf_stage_fuse_end_device")
        return res.as_dict()

    # ---- the fern-coded keyframe database (include/ssf_keyframes.h) ---------------------------------
    def _need_keyframes(self, symbol):
        if not self.L.has_keyframes:
            raise SsfError("%s does not export %s: it keeps no keyframe database (include/ssf_keyframes.h, HIP product only)"
                           % (self.L.path, symbol))

    def keyframes_default_params(self):
        """ssf_keyframes_default_params as a dict"""
        self._need_keyframes("ssf_keyframes_default_params")
        p = SsfKeyframesParams()
        rc = self.L.lib.ssf_keyframes_default_params(C.byref(p))
        if rc != 0:
            raise SsfError("ssf_keyframes_default_params failed (%d)" % rc)
        return p.as_dict()

    def keyframes_configure(self, **kw):
        """Allocate the database on the device and generate the fern table (ssf_keyframes_configure); keywords: the fields of
        ssf_keyframes_params (cell, n_ferns, seed, max_keyframes, min_gap, max_rows, new_ratio, loop_ratio)"""
        self._need_keyframes("ssf_keyframes_configure")
        p = SsfKeyframesParams()
        self.L.lib.ssf_keyframes_default_params(C.byref(p))
        for k, v in kw.items():
            if not hasattr(p, k):
                raise AttributeError("ssf_keyframes_params has no field %r" % k)
            setattr(p, k, v)
        self._ck(self.L.lib.ssf_keyframes_configure(self.h, C.byref(p)), "ssf_keyframes_configure")

    def keyframes_info(self):
        """dict(configured, n_keyframes, rows_used, params) (ssf_keyframes_info)"""
        self._need_keyframes("ssf_keyframes_info")
        c, n, r, p = C.c_int(0), C.c_int(0), C.c_int64(0), SsfKeyframesParams()
        self._ck(self.L.lib.ssf_keyframes_info(self.h, C.byref(c), C.byref(n), C.byref(r), C.byref(p)), "ssf_keyframes_info")
        return dict(configured=bool(c.value), n_keyframes=n.value, rows_used=r.value, params=p.as_dict())

    def _kf_n(self):
        return self.keyframes_info()["params"]["n_ferns"]

    def keyframes_set_ferns(self, ferns):
        """Replace the fern table: a FERN_DTYPE record array of n_ferns entries (ssf_keyframes_set_ferns)"""
        self._need_keyframes("ssf_keyframes_set_ferns")
        f = np.ascontiguousarray(ferns, FERN_DTYPE)
        self._ck(self.L.lib.ssf_keyframes_set_ferns(self.h, _ptr(f), len(f)), "ssf_keyframes_set_ferns")

    def keyframes_get_ferns(self):
        """The fern table in force as a FERN_DTYPE record array (ssf_keyframes_get_ferns)"""
        self._need_keyframes("ssf_keyframes_get_ferns")
        f = np.zeros(KEYFRAMES_MAX_FERNS, FERN_DTYPE)
        self._ck(self.L.lib.ssf_keyframes_get_ferns(self.h, _ptr(f), len(f)), "ssf_keyframes_get_ferns")
        return f[:self._kf_n()].copy()

    def keyframes_encode(self):
        """The current frame's codes, one byte per fern (ssf_keyframes_encode)"""
        self._need_keyframes("ssf_keyframes_encode")
        codes = np.zeros(KEYFRAMES_MAX_FERNS, np.uint8)
        self._ck(self.L.lib.ssf_keyframes_encode(self.h, _ptr(codes), len(codes)), "ssf_keyframes_encode")
        return codes[:self._kf_n()].copy()

    def keyframes_query(self, codes=None, stamp=0, min_gap=-1, k=KEYFRAMES_MAX_CANDIDATES):
        """Search the stored keyframes (ssf_keyframes_query): codes None = the current frame's (with the handle's stamp), else
        n_ferns bytes with `stamp`; min_gap < 0 = the configured one.  Returns the record as a dict."""
        self._need_keyframes("ssf_keyframes_query")
        if codes is not None:
            codes = np.ascontiguousarray(codes, np.uint8)
            if len(codes) != self._kf_n():
                raise SsfError("keyframes_query: %d codes, the database has %d ferns" % (len(codes), self._kf_n()))
        res = SsfKeyframeResult()
        self._ck(self.L.lib.ssf_keyframes_query(self.h, _ptr(codes), int(stamp), int(min_gap), int(k), C.byref(res)), "ssf_keyframes_query")
        return res.as_dict()

    def keyframes_add(self):
        """The current frame becomes a keyframe (ssf_keyframes_add); returns its id"""
        self._need_keyframes("ssf_keyframes_add")
        i = C.c_int(-1)
        self._ck(self.L.lib.ssf_keyframes_add(self.h, C.byref(i)), "ssf_keyframes_add")
        return i.value

    def keyframes_consider(self):
        """Encode the current frame, search, add it when the view is new (ssf_keyframes_consider); returns the record as a dict"""
        self._need_keyframes("ssf_keyframes_consider")
        res = SsfKeyframeResult()
        self._ck(self.L.lib.ssf_keyframes_consider(self.h, C.byref(res)), "ssf_keyframes_consider")
        return res.as_dict()

    def keyframes_put(self, codes, rows, pose, stamp):
        """A keyframe from host data (ssf_keyframes_put): codes n_ferns bytes, rows a dict of the SURFEL_FIELDS arrays (or None for
        no rows), pose 12 floats; returns its id"""
        self._need_keyframes("ssf_keyframes_put")
        codes = np.ascontiguousarray(codes, np.uint8)
        if len(codes) != self._kf_n():
            raise SsfError("keyframes_put: %d codes, the database has %d ferns" % (len(codes), self._kf_n()))
        pose = np.ascontiguousarray(pose, np.float32)
        if pose.size != 12:
            raise SsfError("keyframes_put: a pose is 12 floats")
        n, st, keep = 0, None, []
        if rows is not None and len(rows["confidences"]) > 0:
            n = len(rows["confidences"])
            keep = [np.ascontiguousarray(rows[name], dt) for name, _, dt in SURFEL_FIELDS]
            for a, (name, k, _) in zip(keep, SURFEL_FIELDS):
                if a.size != n * k:
                    raise SsfError("keyframes_put: rows[%r] has %d values for %d rows" % (name, a.size, n))
            st = C.byref(SsfSurfels(*[a.ctypes.data_as(C.c_void_p) for a in keep]))
        i = C.c_int(-1)
        self._ck(self.L.lib.ssf_keyframes_put(self.h, _ptr(codes), st, n, _ptr(pose), int(stamp), C.byref(i)), "ssf_keyframes_put")
        return i.value

    def keyframes_get(self, kf_id):
        """dict(rows (the SURFEL_FIELDS arrays), pose, stamp, codes) of one stored keyframe (ssf_keyframes_get)"""
        self._need_keyframes("ssf_keyframes_get")
        n, stamp = C.c_int(0), C.c_int(0)
        self._ck(self.L.lib.ssf_keyframes_get(self.h, int(kf_id), None, 0, C.byref(n), None, None, None), "ssf_keyframes_get")
        arrs, st = _alloc_surfels(n.value)
        pose, codes = np.zeros(12, np.float32), np.zeros(KEYFRAMES_MAX_FERNS, np.uint8)
        self._ck(self.L.lib.ssf_keyframes_get(self.h, int(kf_id), C.byref(st), n.value, C.byref(n), _ptr(pose), C.byref(stamp), _ptr(codes)),
                 "ssf_keyframes_get")
        return dict(rows=arrs, pose=pose, stamp=stamp.value, codes=codes[:self._kf_n()].copy())

    def keyframes_set_pose(self, kf_id, pose):
        """Move a stored keyframe's pose (ssf_keyframes_set_pose)"""
        self._need_keyframes("ssf_keyframes_set_pose")
        pose = np.ascontiguousarray(pose, np.float32)
        if pose.size != 12:
            raise SsfError("keyframes_set_pose: a pose is 12 floats")
        self._ck(self.L.lib.ssf_keyframes_set_pose(self.h, int(kf_id), _ptr(pose)), "ssf_keyframes_set_pose")

    def keyframes_align(self, kf_id, init_pose=None, use_conf=False):
        """align() with the stored rows of keyframe kf_id as sources, nothing row-sized crossing the bus (ssf_keyframes_align).
        Returns dict(rel_pose (12,), valid, iters, pairs)."""
        self._need_keyframes("ssf_keyframes_align")
        init = None if init_pose is None else np.ascontiguousarray(init_pose, np.float32)
        rel = np.zeros(12, np.float32)
        valid, iters, pairs = C.c_int(0), C.c_int(0), C.c_int(0)
        self._ck(self.L.lib.ssf_keyframes_align(self.h, int(kf_id), _ptr(init), 1 if use_conf else 0, _ptr(rel), C.byref(valid),
                                                C.byref(iters), C.byref(pairs)), "ssf_keyframes_align")
        return dict(rel_pose=rel, valid=bool(valid.value), iters=iters.value, pairs=pairs.value)

    def keyframes_clear(self):
        """Free the database (ssf_keyframes_clear); keyframes_configure may be called again"""
        self._need_keyframes("ssf_keyframes_clear")
        self._ck(self.L.lib.ssf_keyframes_clear(self.h), "ssf_keyframes_clear")

    # ---- loop closure: registration of a keyframe's supersurfels against the current frame ---------
    def align(self, source, init_pose=None):
        """source: dict with positions (n,3), colors (n,3), orientations (n,9) [, confidences (n,)].
        Returns dict(rel_pose (12,), valid, iters, pairs)."""
        pos = np.ascontiguousarray(source["positions"], np.float32)
        col = np.ascontiguousarray(source["colors"], np.float32)
        ori = np.ascontiguousarray(source["orientations"], np.float32)
        conf = source.get("confidences")
        conf = None if conf is None else np.ascontiguousarray(conf, np.float32)
        n = len(pos)
        st = SsfSurfels(_ptr(pos), _ptr(col), None, _ptr(ori), None, None, _ptr(conf))
        init = None if init_pose is None else np.ascontiguousarray(init_pose, np.float32)
        rel = np.zeros(12, np.float32)
        valid, iters, pairs = C.c_int(0), C.c_int(0), C.c_int(0)
        self._ck(self.L.lib.ssf_align(self.h, C.byref(st), n, _ptr(init), _ptr(rel), C.byref(valid), C.byref(iters),
                                      C.byref(pairs)), "ssf_align")
        return dict(rel_pose=rel, valid=bool(valid.value), iters=iters.value, pairs=pairs.value)

    def fern_codes(self, rgb, depth, fern_pos, fern_rgb, fern_depth):
        rgb = np.ascontiguousarray(rgb, np.uint8); depth = np.ascontiguousarray(depth, np.float32)
        fp = np.ascontiguousarray(fern_pos, np.uint32); fr = np.ascontiguousarray(fern_rgb, np.uint8)
        fd = np.ascontiguousarray(fern_depth, np.float32)
        n = len(fd)
        codes = np.zeros(n, np.uint8)
        self._ck(self.L.lib.ssf_fern_codes(self.h, _ptr(rgb), _ptr(depth), depth.shape[1], depth.shape[0], _ptr(fp), _ptr(fr),
                                           _ptr(fd), n, _ptr(codes)), "ssf_fern_codes")
        return codes

    # ---- multi-GPU, native RCCL ------------------------------------------------------------------
    def comm_deal_extract(self, mode=1):
        """After comm_attach, on every rank: batch j of the frame stream is extracted by rank j % nranks alone, which broadcasts
        its frames' tables (ssf_comm_deal_extract; mode 2 additionally re-imports on the extracting rank: a self-check)"""
        self._ck(self.L.lib.ssf_comm_deal_extract(self.h, int(mode)), "ssf_comm_deal_extract")

    def comm_attach(self, group=None):
        """Attach an RCCL communicator over the ranks of a torch.distributed group (which is only used
        to ship rank 0's unique id); afterwards process_frame / process_submitted exchange natively."""
        import torch
        import torch.distributed as dist
        ident, err = np.zeros(128, np.uint8), None
        if dist.get_rank(group) == 0:
            rc = self.L.lib.ssf_comm_unique_id(_ptr(ident))
            if rc != 0:
                err = "ssf_comm_unique_id failed (%d): %s" % (rc, self.L.lib.ssf_last_error(None).decode())
        obj = [None if err else ident.tobytes(), err]
        dist.broadcast_object_list(obj, src=0, group=group)      # every rank learns about a failure on rank 0
        if obj[0] is None:
            raise SsfError(obj[1])
        ident = np.frombuffer(obj[0], np.uint8).copy()
        self._ck(self.L.lib.ssf_comm_attach(self.h, _ptr(ident)), "ssf_comm_attach")

    def comm_info(self):
        """what exchange is attached and how many ranks it reports itself: dict(backend 'none' | 'rccl' | 'p2p', ranks, rank)"""
        b, n, r = C.c_int(), C.c_int(), C.c_int()
        self._ck(self.L.lib.ssf_comm_info(self.h, C.byref(b), C.byref(n), C.byref(r)), "ssf_comm_info")
        return dict(backend=("none", "rccl", "p2p")[b.value], ranks=n.value, rank=r.value)

    # peer-to-peer exchange (ssf_p2p_* in ssf.h): the ranks of one node trade their records through each other's HBM
    P2P_HANDLE_BYTES = 64

    def p2p_configure(self, all_ranks_on_this_device=False, timeout_s=30.0):
        """before p2p_export / p2p_region: plain device memory when every rank is a handle on this GPU (fine-grained
        otherwise), and the wall-clock bound of every in-kernel wait for a peer"""
        self._ck(self.L.lib.ssf_p2p_configure(self.h, 1 if all_ranks_on_this_device else 0, float(timeout_s)), "ssf_p2p_configure")

    def p2p_export(self):
        """64-byte IPC handle of this handle's exchange region (to be shipped to the other ranks)"""
        out = np.zeros(self.P2P_HANDLE_BYTES, np.uint8)
        self._ck(self.L.lib.ssf_p2p_export(self.h, _ptr(out)), "ssf_p2p_export")
        return out

    def p2p_attach(self, handles=None, group=None):
        """handles: nranks x 64 bytes in rank order; None: all-gathered over torch.distributed (group)"""
        if handles is None:
            import torch.distributed as dist
            mine = self.p2p_export().tobytes()
            got = [None] * dist.get_world_size(group)
            dist.all_gather_object(got, mine, group=group)
            handles = np.concatenate([np.frombuffer(b, np.uint8) for b in got])
        handles = np.ascontiguousarray(handles, np.uint8).reshape(-1)
        assert handles.size == self.P2P_HANDLE_BYTES * self.cfg.nranks
        self._ck(self.L.lib.ssf_p2p_attach(self.h, _ptr(handles)), "ssf_p2p_attach")

    def p2p_region(self):
        """(address, bytes) of this handle's exchange region: for ranks that live in one process"""
        reg, nb = C.c_void_p(), C.c_size_t()
        self._ck(self.L.lib.ssf_p2p_region(self.h, C.byref(reg), C.byref(nb)), "ssf_p2p_region")
        return reg.value, nb.value

    def p2p_attach_local(self, regions):
        arr = (C.c_void_p * len(regions))(*regions)
        self._ck(self.L.lib.ssf_p2p_attach_local(self.h, arr), "ssf_p2p_attach_local")

    def global_counts(self):
        out = np.zeros(5, np.int64)
        self._ck(self.L.lib.ssf_get_global_counts(self.h, _ptr(out)), "ssf_get_global_counts")
        return dict(zip(("n_model", "n_visible", "n_removed", "n_inserted", "n_updated"), (int(v) for v in out)))

    # device-resident variants: the arguments are raw addresses (torch tensor .data_ptr())
    def begin_submitted(self):
        self._ck(self.L.lib.ssf_stage_begin_submitted(self.h), "ssf_stage_begin_submitted")

    def icp_accumulate_device(self, d_sums_ptr):
        self._ck(self.L.lib.ssf_stage_icp_accumulate_device(self.h, C.c_void_p(d_sums_ptr)), "ssf_stage_icp_accumulate_device")

    def icp_fetch(self, d_sums_ptr):
        sums = np.zeros(ICP_RECORD, np.int64)
        self._ck(self.L.lib.ssf_stage_icp_fetch(self.h, C.c_void_p(d_sums_ptr), _ptr(sums)), "ssf_stage_icp_fetch")
        return sums

    def match_device(self, d_best_ptr, d_matched_ptr):
        self._ck(self.L.lib.ssf_stage_match_device(self.h, C.c_void_p(d_best_ptr), C.c_void_p(d_matched_ptr)),
                 "ssf_stage_match_device")

    def fuse_device(self, d_best_ptr, d_matched_ptr):
        res = SsfFrameResult()
        self._ck(self.L.lib.ssf_stage_fuse_device(self.h, C.c_void_p(d_best_ptr), C.c_void_p(d_matched_ptr), C.byref(res)),
                 "ssf_stage_fuse_device")
        return res.as_dict()

    # ---- read back ---------------------------------------------------------------------------
    def get_pose(self):
        p = np.zeros(12, np.float32)
        self._ck(self.L.lib.ssf_get_pose(self.h, _ptr(p)), "ssf_get_pose")
        return p

    def set_pose(self, p):
        p = np.ascontiguousarray(p, np.float32)
        self._ck(self.L.lib.ssf_set_pose(self.h, _ptr(p)), "ssf_set_pose")

    def counts(self):
        v = [C.c_int(0) for _ in range(4)]
        self._ck(self.L.lib.ssf_get_counts(self.h, *[C.byref(x) for x in v]), "ssf_get_counts")
        return dict(n_model=v[0].value, n_visible=v[1].value, stamp=v[2].value, n_superpixels=v[3].value)

    def get_model(self, first=0, count=None):
        if count is None:
            count = self.counts()["n_model"] - first
        arrs, st = _alloc_surfels(max(count, 0))
        if count > 0:
            self._ck(self.L.lib.ssf_get_model(self.h, first, count, C.byref(st)), "ssf_get_model")
        return arrs

    def get_frame(self):
        arrs, st = _alloc_surfels(self.S)
        self._ck(self.L.lib.ssf_get_frame(self.h, C.byref(st)), "ssf_get_frame")
        return arrs

    def set_model(self, arrs, n_visible, stamp):
        n = len(arrs["confidences"])
        keep = [np.ascontiguousarray(arrs[name], dt) for name, _, dt in SURFEL_FIELDS]
        st = SsfSurfels(*[a.ctypes.data_as(C.c_void_p) for a in keep])
        self._ck(self.L.lib.ssf_set_model(self.h, C.byref(st), n, n_visible, stamp), "ssf_set_model")

    def _map(self, fn, dtype, shape):
        out = np.zeros(shape, dtype)
        self._ck(getattr(self.L.lib, fn)(self.h, _ptr(out)), fn)
        return out

    def index_map(self):
        return self._map("ssf_get_index_map", np.int32, (self.H, self.W))

    def boundary_map(self):
        return self._map("ssf_get_boundary_map", np.int32, (self.H, self.W))

    def inlier_map(self):
        return self._map("ssf_get_inlier_map", np.uint8, (self.H, self.W))

    def plane_depth(self):
        return self._map("ssf_get_plane_depth", np.float32, (self.H, self.W))

    def preview_image(self):
        """computeSuperpixelSegIm: H x W x 3 uint8 (B, G, R), boundaries white"""
        return self._map("ssf_get_preview_image", np.uint8, (self.H, self.W, 3))

    def slanted_plane_image(self):
        """computeSlantedPlaneIm: the plane-rendered depth, H x W float32"""
        return self.plane_depth()

    def model_device(self):
        """ssf_get_model_device: (SsfSurfels of device pointers in the reference's layout, n_model)"""
        st, n = SsfSurfels(), C.c_int(0)
        self._ck(self.L.lib.ssf_get_model_device(self.h, C.byref(st), C.byref(n)), "ssf_get_model_device")
        return st, n.value

    def superpixels(self):
        return self._map("ssf_get_superpixels", np.float32, (self.S, 9))

    def export_model_txt(self, path):
        self._ck(self.L.lib.ssf_export_model_txt(self.h, path.encode()), "ssf_export_model_txt")

    def apply_deformation(self, node_pos, node_rot, node_trans, weights4, idx4):
        a = [np.ascontiguousarray(node_pos, np.float32), np.ascontiguousarray(node_rot, np.float32),
             np.ascontiguousarray(node_trans, np.float32), np.ascontiguousarray(weights4, np.float32),
             np.ascontiguousarray(idx4, np.int32)]
        self._ck(self.L.lib.ssf_apply_deformation(self.h, _ptr(a[0]), _ptr(a[1]), _ptr(a[2]), len(a[0]),
                                                  _ptr(a[3]), _ptr(a[4])), "ssf_apply_deformation")

    def rehome_begin(self, capacity=None):
        """rows that now belong to another rank's tile leave this shard -> (n, MIGRANT_WORDS) int32 records"""
        cap = self.counts()["n_model"] if capacity is None else int(capacity)
        table = np.zeros((max(cap, 1), MIGRANT_WORDS), np.int32)
        n = C.c_int(0)
        self._ck(self.L.lib.ssf_rehome_begin(self.h, _ptr(table), cap, C.byref(n)), "ssf_rehome_begin")
        return table[:n.value].copy()

    def rehome_end(self, table):
        """table: the records of all ranks in rank order (those addressed to this rank are appended).  Returns the number of
        arrivals a full shard had to turn away (lost to the map, like an arrival at a full shard inside a frame)"""
        table = np.ascontiguousarray(table, np.int32).reshape(-1, MIGRANT_WORDS)
        rc = self.L.lib.ssf_rehome_end(self.h, _ptr(table), len(table))
        if rc < 0:
            self._ck(rc, "ssf_rehome_end")
        return rc

    def bilateral_filter(self, depth):
        """the depth pre-filter alone: input in the handle's depth format, output H x W float32 metres"""
        depth = np.ascontiguousarray(depth, np.float32) if self.depth_format == "f32" else self._depth_array(depth)
        out = np.zeros(depth.shape, np.float32)
        self._ck(self.L.lib.ssf_bilateral_filter(self.h, _ptr(depth), _ptr(out), 0), "ssf_bilateral_filter")
        return out

    def kernel_times(self, max_k=64):
        names = (C.c_char_p * max_k)()
        ms = np.zeros(max_k, np.float64)
        calls = np.zeros(max_k, np.int64)
        n = self.L.lib.ssf_get_kernel_times(self.h, C.cast(names, C.c_void_p), _ptr(ms), _ptr(calls), max_k)
        return {names[i].decode(): (float(ms[i]), int(calls[i])) for i in range(max(n, 0))}

    def reset_kernel_times(self):
        self.L.lib.ssf_reset_kernel_times(self.h)

    def set_profile(self, level):
        """0: off, 2: stage_ms split only, 1: stage split + per-kernel hipEvent times"""
        self._ck(self.L.lib.ssf_set_profile(self.h, int(level)), "ssf_set_profile")
