/* ssf.hpp -- header-only C++ surface over the C ABI of ssf.h, with the method names of the reference's
 * supersurfel_fusion::SupersurfelFusion (core/include/supersurfel_fusion/supersurfel_fusion.hpp:40-143) for the
 * hot path: initialize / processFrame / getPose / getnbSupersurfels / getStamp / getModel / exportModel.
 * A node that owns a `supersurfel_fusion::SupersurfelFusion ssf;` member includes this header instead of the
 * reference's and links libssf_hip.so.  No OpenCV needed: processFrame takes raw pointers; the
 * cv::Mat overloads appear when <opencv2/core.hpp> has been included before this header.  setInputFormat (ssf_input.h,
 * libssf_hip.so only) lets processFrame take a sensor's frames as they come: BGR colour, uint16 depth counts.  processFrame with a
 * PixelMask (ssf_dynamic.h, libssf_hip.so only) takes a detector's per-pixel mask of moving objects.
 *
 * Sparse VO, MOD and loop closure stay with the caller; their outputs enter as `vo_pose` and `dynamic`.
 * Errors: the reference exits the process on a CUDA failure (cuda_error_check.h:30-66); this surface throws
 * std::runtime_error with the library's message. */
#ifndef SSF_HPP
#define SSF_HPP
#include <algorithm>
#include <array>
#include <cmath>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>
#include "ssf.h"
#include "ssf_input.h"
#include "ssf_dynamic.h"
#include "ssf_render.h"
#include "ssf_query.h"
#include "ssf_navgrid.h"
#include "ssf_navcarve.h"
#include "ssf_navplan.h"
#include "ssf_navfrontier.h"
#include "ssf_navpath.h"
#include "ssf_navlive.h"
#include "ssf_navsteer.h"
#include "ssf_navfoot.h"
#include "ssf_navpose.h"
#include "ssf_navdyn.h"
#include "ssf_navmem.h"
#include "ssf_navfloor.h"
#include "ssf_raycast.h"
#include "ssf_motion.h"
#include "ssf_odometry.h"
#include "ssf_graph.h"
#include "ssf_graph_solve.h"
#include "ssf_keyframes.h"

/* The reference's pose / matrix types (core/include/supersurfel_fusion/matrix_types.h:26-42), at GLOBAL scope as there,
 * so that the nodes' lines compile as they stand:
 *     Transform3 pose = ssf.getPose();
 *     tf::Matrix3x3(pose.R.rows[0].x, pose.R.rows[0].y, ... ), tf::Vector3(pose.t.x, pose.t.y, pose.t.z)
 * (node/supersurfel_fusion_node.cpp:87-91, node/supersurfel_fusion_rgbd_benchmark_node.cpp:616-620).  The reference gets
 * float3 from <cuda_runtime.h>; a translation unit that already has HIP's or CUDA's vector types keeps those (same three
 * floats x, y, z), any other gets the plain struct below.  SSF_NO_MATRIX_TYPES: the includer brings its own
 * matrix_types.h. */
#ifndef SSF_NO_MATRIX_TYPES
/* Include order: a translation unit that uses HIP's / CUDA's vector types includes THEIR header before this one (then
 * float3 / float2 / int2 below are theirs).  The other order is a compile error (redefinition of float3 in the vendor
 * header), never a silent mismatch: the three fallbacks have the vendor types' size and field order, asserted below. */
#if !defined(HIP_INCLUDE_HIP_AMD_DETAIL_HIP_VECTOR_TYPES_H) && !defined(__VECTOR_TYPES_H__) && !defined(SSF_HAVE_FLOAT3)
#define SSF_HAVE_FLOAT3
struct float3 { float x, y, z; };
struct float2 { float x, y; };
struct int2 { int x, y; };
#endif
static_assert(sizeof(float3) == 12 && sizeof(float2) == 8 && sizeof(int2) == 8, "ssf.hpp: float3 / float2 / int2 must be the packed vendor layouts");
#ifndef MATRIX_TYPES_HPP            /* the reference header's own guard: both may be included, in either order */
#define MATRIX_TYPES_HPP
struct Cov3 { float xx, xy, xz, yy, yz, zz; };                          /* matrix_types.h:26-31 */
struct Mat33 { float3 rows[3]; };                                       /* matrix_types.h:33-36 */
struct Transform3 { Mat33 R; float3 t; };                               /* matrix_types.h:38-42: camera-to-map */
#endif
#endif

namespace supersurfel_fusion {

struct CamParam { float fx, fy, cx, cy; int height, width; };          /* cam_param.hpp:27-31 */
using ::Transform3; using ::Mat33; using ::Cov3; using ::float3;       /* the reference's are global; both spellings work */

/* Transform3 <-> the C ABI's 12 floats (row-major R, then t) */
inline Transform3 transform3_from_rt(const float v[12]) {
    Transform3 p;
    for (int r = 0; r < 3; r++) { p.R.rows[r].x = v[3 * r]; p.R.rows[r].y = v[3 * r + 1]; p.R.rows[r].z = v[3 * r + 2]; }
    p.t.x = v[9]; p.t.y = v[10]; p.t.z = v[11];
    return p;
}
inline void transform3_to_rt(const Transform3& p, float v[12]) {
    for (int r = 0; r < 3; r++) { v[3 * r] = p.R.rows[r].x; v[3 * r + 1] = p.R.rows[r].y; v[3 * r + 2] = p.R.rows[r].z; }
    v[9] = p.t.x; v[10] = p.t.y; v[11] = p.t.z;
}

/* host copy of a supersurfel set in the reference's SoA layout (supersurfels.hpp:34-40) */
struct HostSupersurfels {
    std::vector<float> positions, colors, orientations, shapes, dims, confidences;
    std::vector<int32_t> stamps;
    int size = 0;
    void resize(int n) {
        size = n; const size_t m = (size_t)(n > 0 ? n : 1);
        positions.resize(3 * m); colors.resize(3 * m); stamps.resize(2 * m); orientations.resize(9 * m);
        shapes.resize(6 * m); dims.resize(2 * m); confidences.resize(m);
    }
    ssf_surfels view() {
        ssf_surfels v; v.positions = positions.data(); v.colors = colors.data(); v.stamps = stamps.data();
        v.orientations = orientations.data(); v.shapes = shapes.data(); v.dims = dims.data(); v.confidences = confidences.data();
        return v;
    }
};

/* ---- getModel() / getFrame() as the reference returns them: device-resident arrays the callers hand to thrust ----------------
 * The reference's Supersurfels (supersurfels.hpp:32-40) holds seven thrust::device_vectors and its nodes copy them out with
 *     thrust::host_vector<float3> positions(ssf.getModel().positions.begin(), ssf.getModel().positions.begin() + ssf.getnbSupersurfels());
 *     thrust::host_vector<Mat33> orientations(ssf.getFrame().orientations);
 * (node/supersurfel_fusion_node.cpp:306-310,423-427,688-690; ...benchmark_node.cpp:189-193,305-306).  A node built for AMD has
 * rocThrust (hipcc, /opt/rocm/include/thrust): when <thrust/...> was included before this header, Supersurfels is a VIEW of the
 * library's device arrays with the same seven member names -- each a DeviceArray<T>: begin() / end() as thrust::device_ptr<T>,
 * size(), and a conversion to thrust::host_vector<T> for the whole-array form -- and getModel() / getFrame() return
 * `const Supersurfels&` exactly as supersurfel_fusion.hpp:86-87: those lines compile as they stand (tests/cpp/node_model_copy.cpp,
 * compiled by hipcc against rocThrust).  The view covers the n valid rows (the reference's vectors have capacity
 * nb_supersurfels_max; its callers stop at getnbSupersurfels()); it is valid until the next call on the object.  Without
 * thrust (plain g++) getModel() / getFrame() hand back host copies (HostSupersurfels), also available as getModelHost() /
 * getFrameHost() in both builds.  SSF_NO_THRUST_VIEW: keep the host-copy form although thrust is there. */
#if defined(THRUST_VERSION) && !defined(SSF_NO_THRUST_VIEW)
#define SSF_THRUST_VIEW 1
}  /* namespace supersurfel_fusion */
#include <thrust/device_ptr.h>
#include <thrust/host_vector.h>
#include <thrust/copy.h>
namespace supersurfel_fusion {
#endif
/* DATA LAYOUT IS UNCONDITIONAL: DeviceArray<T> is a pointer and a count whether or not thrust is there -- only its
 * thrust-typed accessors depend on the include order -- and SupersurfelFusion always holds its two views, so
 * sizeof(SupersurfelFusion) is the same in every translation unit of a node (a .hip file with thrust and a main.cpp
 * without may share one object).  What DOES differ between the two forms is the return type of getModel() / getFrame();
 * the class therefore lives in an inline namespace named after the form (`thrust_view` / `host_copy`): code never spells
 * it, but a function that passes a SupersurfelFusion between translation units of different forms fails to LINK instead
 * of calling the wrong getModel(). */
/* (round 6: DeviceArray and Supersurfels live in the inline namespace too -- their member SETS differ between the forms, and two
 * definitions of one class name in one namespace would be an ODR violation even where the layout agrees) */
#ifdef SSF_THRUST_VIEW
inline namespace thrust_view {
#else
inline namespace host_copy {
#endif

template <typename T> struct DeviceArray {
    T* ptr = nullptr; size_t n = 0;
    size_t size() const { return n; }
    bool empty() const { return n == 0; }
    T* data() const { return ptr; }
#ifdef SSF_THRUST_VIEW
    typedef thrust::device_ptr<T> iterator;
    typedef thrust::device_ptr<T> const_iterator;
    iterator begin() const { return thrust::device_pointer_cast(ptr); }
    iterator end() const { return thrust::device_pointer_cast(ptr) + n; }
    operator thrust::host_vector<T>() const { thrust::host_vector<T> v(n); thrust::copy(begin(), end(), v.begin()); return v; }
#endif
};
struct Supersurfels {                                                    /* supersurfels.hpp:32-40, as views */
    DeviceArray<float3> positions, colors;
    DeviceArray<int2> stamps;
    DeviceArray<Mat33> orientations;
    DeviceArray<Cov3> shapes;
    DeviceArray<float2> dims;
    DeviceArray<float> confidences;
    void bind(const ssf_surfels& v, size_t n) {
        positions.ptr = reinterpret_cast<float3*>(v.positions); colors.ptr = reinterpret_cast<float3*>(v.colors);
        stamps.ptr = reinterpret_cast<int2*>(v.stamps); orientations.ptr = reinterpret_cast<Mat33*>(v.orientations);
        shapes.ptr = reinterpret_cast<Cov3*>(v.shapes); dims.ptr = reinterpret_cast<float2*>(v.dims); confidences.ptr = v.confidences;
        positions.n = colors.n = stamps.n = orientations.n = shapes.n = dims.n = confidences.n = n;
    }
};
static_assert(sizeof(DeviceArray<float3>) == sizeof(void*) + sizeof(size_t) && sizeof(Supersurfels) == 7 * sizeof(DeviceArray<float>),
              "ssf.hpp: the device views are (pointer, count) pairs in every translation unit");

/* a per-pixel mask of moving objects for processFrame (ssf_dynamic.h): H x W bytes, non-zero = dynamic; nullptr = none */
struct PixelMask {
    const uint8_t* data;
    explicit PixelMask(const uint8_t* d) : data(d) {}
};

/* detectMotion / processFrame(rgb, depth, MotionParams) (ssf_motion.h; exported by libssf_hip.so only): the geometric moving-object
 * detector.  The defaults are ssf_motion_default_params' (design choices, not tuned values); min_seeds 0 = max(1, W * H / 1024);
 * pose nullptr = the pose prior of the call, else the current pose */
struct MotionParams {
    const float* pose = nullptr;
    float min_conf = 0.f, splat_scale = 3.f, front_abs = 0.05f, front_quad = 0.01f, link_abs = 0.02f, link_rel = 0.01f;
    int min_seeds = 0, unknown_per_seed = 2;
};
/* the mask of detectMotion / getMotionMask, row-major H x W (1 = moving object), and its statistics */
struct MotionMask {
    int width = 0, height = 0;
    std::vector<uint8_t> mask;
    ssf_motion_stats stats{};
};

/* estimateOdometry / trackOdometry / processFrame(rgb, depth, OdometryParams) (ssf_odometry.h; exported by libssf_hip.so only): the
 * dense RGB-D odometry that makes a frame's pose prior.  The defaults are ssf_odometry_default_params' (design choices, not tuned
 * values); iters[l] belongs to pyramid level l, 0 = the full image */
struct OdometryParams {
    int levels = 4;
    int iters[SSF_ODO_MAX_LEVELS] = {4, 6, 8, 10, 10, 10};
    float r_max = 0.5f, huber = 0.2f, min_pixel_share = 0.05f, tol_rot = 1e-4f, tol_trans = 1e-4f, max_translation = 0.3f, max_rotation = 0.35f;
};
/* what estimateOdometry / trackOdometry / getOdometry return: rel = current camera -> reference camera, prior = the pose prior
 * (camera-to-map), both in getPose's 12-float layout; prior is meaningful when has_prior (trackOdometry with a valid estimate) */
struct OdometryEstimate {
    float rel[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
    float prior[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    bool has_prior = false;
    ssf_odometry_result result{};
};

/* renderModel (ssf_render.h; exported by libssf_hip.so only): the map drawn into a pinhole camera on the device.  Defaults: the
 * handle's camera (width 0), cfg.range_min / range_max (both 0), the reference node's marker size 3 */
struct RenderOptions {
    int width = 0, height = 0; float fx = 0.f, fy = 0.f, cx = 0.f, cy = 0.f;
    float z_min = 0.f, z_max = 0.f, min_conf = 0.f, splat_scale = 3.f;
    bool visible_only = false;
};
/* the images of renderModel, row-major H x W (x 3), and its statistics */
struct RenderedView {
    int width = 0, height = 0;
    std::vector<float> depth, color, normal;       /* depth 0 / colour 0 / normal 0 where no disc is hit */
    std::vector<int32_t> index;                    /* logical row index (getModelHost's order), -1 where no disc is hit */
    std::vector<uint8_t> rgb8;
    ssf_render_stats stats;
};

/* queryModel / countModel (ssf_query.h; exported by libssf_hip.so only): rows of the map selected on the device.  Defaults: every
 * live row (min_conf 0, any stamps, SSF_REGION_ALL); pose nullptr = the current pose; width 0 = the handle's camera; z_min = z_max
 * = 0 = cfg.range_min / range_max */
struct QueryParams {
    float min_conf = 0.f;
    int32_t t_init_min = -2147483647 - 1, t_init_max = 2147483647, t_last_min = -2147483647 - 1, t_last_max = 2147483647;
    bool visible_only = false;
    int region = SSF_REGION_ALL;                   /* ssf_region_kind */
    const Transform3* pose = nullptr;              /* frame-to-map: the sphere's centre (t) / the box's frame / the frustum's camera */
    float radius = 0.f;
    float half[3] = {0.f, 0.f, 0.f};
    int width = 0, height = 0; float fx = 0.f, fy = 0.f, cx = 0.f, cy = 0.f;
    float z_min = 0.f, z_max = 0.f;
};
/* the rows queryModel selects, in getModelHost()'s layout and order; index[j] = the row's position in getModelHost() */
struct QueryResult {
    HostSupersurfels rows;
    std::vector<int32_t> index;
    ssf_query_stats stats;
};

/* buildNavGrid (ssf_navgrid.h; exported by libssf_hip.so only): the floor-plane navigation grid of the map.  The members start at
 * ssf_navgrid_default_params' values (design choices, see the header); pose nullptr = floor-aligned about the camera with heights
 * measured from the first camera -- a node that knows how its camera is mounted passes its own frame and bands */
struct NavGridParams {
    const Transform3* pose = nullptr;              /* grid-to-map: x, y span the floor, z up */
    int width = 512, height = 512; float res = 0.05f;
    float z_min = -1.5f, z_max = 0.5f, floor_max = -0.8f, floor_cos = 0.8f, min_conf = 0.f;
    int32_t t_init_min = -2147483647 - 1, t_init_max = 2147483647, t_last_min = -2147483647 - 1, t_last_max = 2147483647;
    bool visible_only = false;
    float splat_scale = 2.f; int max_steps = 8, min_hits = 1, max_dist_cells = 40;
    bool unknown_is_obstacle = false;
    bool want_heights = true, want_hits = true, want_state = true, want_dist2 = true;      /* false: not produced (its vector stays empty) */
};
/* the grid buildNavGrid makes, row-major height x width (cell (ix, iy) at iy * width + ix), and its statistics; stats.pose is the
 * grid frame that was used */
struct NavGrid {
    int width = 0, height = 0; float res = 0.f;
    std::vector<float> zmin, zmax;                 /* +inf / -inf where nothing was seen */
    std::vector<uint32_t> hits;                    /* x 2: floor samples, obstacle samples */
    std::vector<int8_t> state;                     /* nav_msgs/OccupancyGrid's values: 100 occupied, 0 free, -1 unknown */
    std::vector<int32_t> dist2;                    /* squared distance in cells to the nearest obstacle cell, capped at max_dist_cells^2 */
    ssf_navgrid_stats stats;
};
/* fitFloor (ssf_navfloor.h; exported by libssf_hip_floor.so, linked INSTEAD of the other libraries -- a program that does not call
 * it links as before: the inline member leaves no reference behind): the floor plane of the map, fitted on the device, as the frame and
 * bands of a navigation grid.  The members start at ssf_navfloor_default_params' values; origin nullptr = the camera position. */
struct FloorParams {
    float3 up = float3{0.f, -1.f, 0.f};            /* up hint in the map frame (the first camera's y points down) */
    const float3* origin = nullptr;                /* positions are taken relative to it; the pose's multiples of res count from it */
    float tilt_cos = 0.8f, align_cos = 0.95f, height_res = 0.02f;
    int min_rows = 32, floor_share256 = 64, refine_iters = 3;
    float first_dist = 0.15f, inlier_dist = 0.05f, min_conf = 0.f;
    int32_t t_init_min = -2147483647 - 1, t_init_max = 2147483647, t_last_min = -2147483647 - 1, t_last_max = 2147483647;
    bool visible_only = false;
    int width = 512, height = 512; float res = 0.05f;      /* the grid the pose is centred and snapped for */
    float below = 0.5f, step = 0.2f, body_height = 1.5f;   /* the bands about the floor: z_min = -below, floor_max = step, z_max = body_height */
    bool want_histograms = false;
};
/* what fitFloor found: fit is the C result (status, plane, counts, rounds, pose, bands); pose is fit.pose as a Transform3 */
struct FloorFit {
    ssf_navfloor_fit_result fit;
    Transform3 pose;
    std::vector<uint32_t> dir_hist, height_hist;   /* with want_histograms: 31 x 31 and 2048 */
    bool ok() const { return fit.status == SSF_NAVFLOOR_OK; }
    /* the frame, the bands and the size of the fit into a grid's parameters; g.pose points into this object */
    void applyTo(NavGridParams& g) const {
        g.pose = &pose; g.z_min = fit.z_min; g.floor_max = fit.floor_max; g.z_max = fit.z_max;
        g.width = fit.width; g.height = fit.height; g.res = fit.res;
    }
};
/* buildNavGrid with views (ssf_navcarve.h; exported by libssf_hip_navcarve.so, linked INSTEAD of libssf_hip.so -- a program that
 * does not call it links against libssf_hip.so as before: the inline member leaves no reference behind): the grid with free space carved along camera rays.  The
 * members start at ssf_navcarve_default_params' values: width 0 = the configured camera and its intrinsics, t_min = t_max = 0 =
 * the configured depth range, ray_splat_scale 0 = the ray cast's 3.  A miss carves nothing unless carve_misses says so. */
struct CarveParams {
    float fx = 0.f, fy = 0.f, cx = 0.f, cy = 0.f; int width = 0, height = 0;
    int stride = 8;
    float t_min = 0.f, t_max = 0.f, ray_min_conf = 0.f, ray_splat_scale = 0.f, hit_margin_cells = 1.f;
    bool carve_misses = false; int min_seen = 1;
    bool want_seen = true;
};
/* a NavGrid whose state and dist2 are carved, with the ray entries per cell; stats (the base's) = carve.grid */
struct CarvedNavGrid : NavGrid {
    std::vector<uint32_t> seen;
    ssf_navcarve_stats carve;
};

/* planOnGrid (ssf_navplan.h; exported by libssf_hip_nav.so, linked INSTEAD of libssf_hip.so or libssf_hip_navcarve.so -- a program
 * that does not call it links as before: the inline member leaves no reference behind): the cost-to-goal field of a grid and the
 * cell paths down it.  The members start at ssf_navplan_default_params' values. */
struct PlanParams {
    int min_dist2 = 0;                             /* the robot's squared radius in cells */
    int soft_dist2 = 0, near_penalty = 0;          /* extra cost below a squared clearance; 0 = none */
    bool allow_unknown = false, goals_from_frontier = false;
    int max_path = 0;                              /* cells per path; 0 = no paths */
    bool want_cost = true, want_frontier = true;   /* false: not produced (its vector stays empty) */
};
typedef std::array<int32_t, 2> GridCell;           /* (ix, iy) */
/* what planOnGrid makes: the field and the frontier, row-major height x width; per start its cost, status (ssf_navplan.h step 7)
 * and the cells of its path */
struct NavPlan {
    int width = 0, height = 0;
    std::vector<uint32_t> cost;                    /* 0xFFFFFFFF = not reached */
    std::vector<uint8_t> frontier;
    std::vector<uint32_t> start_cost;
    std::vector<int32_t> start_status;
    std::vector<std::vector<GridCell> > paths;
    ssf_navplan_stats stats;
};

/* frontierRegions and exploreGoal (ssf_navfrontier.h; exported by libssf_hip_explore.so, linked INSTEAD of the other libraries -- a
 * program that calls neither links as before: the inline members leave no reference behind): the grid's frontier as regions, and
 * the region to drive to next.  The members start at ssf_navfrontier_default_params' values. */
struct FrontierParams {
    int connectivity = 8;                          /* 8 or 4 */
    bool traversable_only = false; int min_dist2 = 0;       /* members with dist2 >= min_dist2 only (the grid needs dist2) */
    int min_cells = 1;                             /* smaller regions are dropped */
    bool reachable_only = false;                   /* regions without a reached member are dropped (needs a cost field) */
    int max_regions = 4096, gain_radius = 0;
    int cost_weight = 1, gain_weight = 0, size_weight = 0;
    bool want_region = true;                       /* false: the map is not produced (its vector stays empty) */
};
/* what frontierRegions makes: the map (row-major height x width: table index, -1 no member, -2 not in the table), the table in
 * label order and the table indices best first */
struct FrontierRegions {
    int width = 0, height = 0;
    std::vector<int32_t> region;
    std::vector<ssf_navfrontier_region> regions;
    std::vector<int32_t> order;
    ssf_navfrontier_stats stats;
};
/* what exploreGoal makes: the regions ranked by the cost of reaching them from the robot, the chosen one (order[0]; -1 = none was
 * reached), its representative cell and the robot's path to it (drive.paths[0]) */
struct ExploreGoal {
    FrontierRegions frontier;
    int chosen = -1;
    GridCell goal;
    NavPlan drive;
};

/* refinePaths (ssf_navpath.h; exported by libssf_hip_drive.so, linked INSTEAD of the other libraries -- a program that does not call
 * it links as before: the inline member leaves no reference behind): the cell paths of a plan reduced to any-angle waypoints.  The
 * members start at ssf_navpath_default_params' values. */
struct WaypointParams {
    int min_dist2 = 0; bool allow_unknown = false;      /* the plan's: what the robot may stand on */
    int los_dist2 = 0;                                  /* every cell of a segment has at least this squared clearance */
    bool keep_clearance = false; int clearance_cap = 0; /* a segment keeps the clearance of the piece of path it replaces, up to the cap */
    int lookahead = 256;                                /* candidates per anchor, 1..4096 */
    int max_waypoints = 0;                              /* per path; 0 = as many as the longest path has cells */
};
struct Waypoint { int32_t ix, iy, index, seg_min; };    /* index: into the path, bit 30 (SSF_NAVPATH_FORCED) on a forced step */
/* what refinePaths makes: per path its waypoints, status (ssf_navpath.h step 6) and smallest seg_min (-1: no waypoint) */
struct NavWaypoints {
    std::vector<std::vector<Waypoint> > waypoints;
    std::vector<int32_t> status, path_min;
    ssf_navpath_stats stats;
};

/* overlayDepthFrame (ssf_navlive.h; exported by libssf_hip_live.so, linked INSTEAD of the other libraries -- a program that does not
 * call it links as before: the inline member leaves no reference behind): the depth frame of the instant stamped onto a grid.  The
 * members start at ssf_navlive_default_params' values: cam_pose nullptr = the tracked pose, width 0 = the configured camera and its
 * intrinsics, t_min = t_max = 0 = the configured depth range.  The grid's size, res and frame are the input grid's. */
struct LiveParams {
    const Transform3* cam_pose = nullptr;          /* camera-to-map of the depth frame */
    float fx = 0.f, fy = 0.f, cx = 0.f, cy = 0.f; int width = 0, height = 0;
    float t_min = 0.f, t_max = 0.f;
    float floor_max = -0.8f, z_max = 0.5f;         /* the band of the robot's body, as the grid was built with */
    int max_dist_cells = 40; bool unknown_is_obstacle = false;
    int mask_mode = 0;                             /* 0 no mask; 1 only pixels with mask != 0 stamp; 2 only pixels with mask == 0 */
    int min_hits = 4, stride = 4; float hit_margin_cells = 1.f; int min_seen = 1; bool open_unknown = true;
    bool want_hits = true, want_seen = true, want_dist2 = true;      /* false: not produced (its vector stays empty) */
};
/* a NavGrid whose state and dist2 hold the live layer, with the frame's points and ray entries per cell; stats.pose and the cell
 * counts of stats are the live grid's, zmin / zmax / hits stay empty */
struct LiveNavGrid : NavGrid {
    std::vector<uint32_t> live_hits, live_seen;
    ssf_navlive_stats live;
};
/* The caller's memory of the live layer (ssf_navmem.h; exported by libssf_hip_mem.so, linked INSTEAD of the other libraries -- a program
 * that does not call the overlayDepthFrame overloads that take one links as before): per cell the marked height slices of the body's
 * band, the tick of the last stamp and the tick at which the cell was last seen through.  The handle keeps nothing of it: the overloads
 * read it, write it back and record the call's tick and stats.  It sizes itself to the grid of the first call; a grid of another size
 * starts it afresh, and so does clear().  It lives in the grid's frame and does not scroll: keep the grid's pose, or clear it. */
struct LiveMemory {
    int slices = 16;                               /* 1..32 height slices of the band */
    uint32_t max_mark_age = 0, max_seen_age = 0;   /* ticks after which a mark / a seen-through cell expires; 0 = never */
    int width = 0, height = 0;
    std::vector<uint32_t> marks, mark_tick, seen_tick;
    uint32_t tick = 0;                             /* of the last update; 0 = none yet */
    ssf_navmem_stats stats = ssf_navmem_stats();   /* of the last update */
    std::vector<uint32_t> hit_bits, seen_bits;     /* the last frame's evidence per cell and slice */
    void clear() { width = height = 0; marks.clear(); mark_tick.clear(); seen_tick.clear(); hit_bits.clear(); seen_bits.clear(); tick = 0; }
};

/* steerOnGrid (ssf_navsteer.h; exported by libssf_hip_steer.so, linked INSTEAD of the other libraries -- a program that does not call
 * it links as before: the inline member leaves no reference behind): a lattice of (v, w) candidates rolled out over a grid from
 * every pose, and the best admissible one.  The members start at ssf_navsteer_default_params' values; units as in ssf_navsteer.h:
 * 1024 sub-units per cell, 65536 heading units per turn, per step. */
struct SteerParams {
    int min_dist2 = 0; bool allow_unknown = false;      /* the plan's: what the robot may stand on */
    int clearance_cap = 64;
    int n_v = 9, n_w = 33, v_min = 0, v_step = 64, w_min = -2048, w_step = 128;       /* the lattice (steerWindow makes one) */
    int n_steps = 32, min_free_steps = 2, brake_div = 128;
    int cost_weight = 1, target_weight = 0, clear_weight = 1, speed_weight = 1, turn_weight = 0;
    bool want_traj = true, want_candidates = false;     /* false: not produced (its vectors stay empty) */
};
struct SteerPose { int32_t x, y, heading; };            /* units */
struct SteerTarget { int32_t x, y; };
/* a metric grid-frame pose (x m, y m, yaw rad) in units */
inline SteerPose steerUnits(double x_m, double y_m, double yaw, float res) {
    SteerPose p;
    p.x = (int32_t)std::floor(x_m / (double)res * 1024.0); p.y = (int32_t)std::floor(y_m / (double)res * 1024.0);
    p.heading = (int32_t)((long long)std::floor(yaw / 6.283185307179586476925286766559 * 65536.0 + 0.5) & 0xFFFF);
    return p;
}
/* what steerOnGrid makes: per pose the winning candidate (-1: none), its command, score, the admissible count, the status
 * (ssf_navsteer.h step 8) and the winner's arc; with want_candidates the per-candidate arrays, n_poses x K */
struct NavSteer {
    int n_steps = 0, candidates = 0;                   /* K */
    std::vector<int32_t> best, v, w, n_admissible, status;
    std::vector<int64_t> score;
    std::vector<std::vector<SteerPose> > traj;
    std::vector<int32_t> cand_free, cand_min_d, cand_end;      /* cand_end x 3 */
    std::vector<uint32_t> cand_end_cost;
    std::vector<int64_t> cand_score;
    ssf_navsteer_stats stats;
};

/* footprintLayers and steerWithFootprint (ssf_navfoot.h; exported by libssf_hip_foot.so, linked INSTEAD of the other libraries -- a
 * program that calls neither links as before): a rectangular body from the robot's centre, in sub-units (1024 per cell; x forward,
 * +y left), and the heading bins its layers are made for.  pad < 0: footprintPad's value, which makes the layers conservative
 * for any position in a cell and any heading in a bin. */
struct FootprintParams {
    int front = 0, back = 0, left = 0, right = 0, pad = -1;
    int n_headings = 16;                                /* 1, 2, 4, 8, 16 or 32 */
    bool allow_unknown = false;                         /* the plan's */
    bool want_n_free = false;
};
/* a body in metres, each side rounded up to sub-units */
inline FootprintParams footprintUnits(double front_m, double back_m, double left_m, double right_m, float res) {
    FootprintParams f;
    f.front = (int)std::ceil(front_m / (double)res * 1024.0); f.back = (int)std::ceil(back_m / (double)res * 1024.0);
    f.left = (int)std::ceil(left_m / (double)res * 1024.0); f.right = (int)std::ceil(right_m / (double)res * 1024.0);
    return f;
}
/* what footprintLayers makes: per cell the bit mask of the heading bins at which the body centred there stands on clear cells only */
struct FootprintLayers {
    int width = 0, height = 0, n_headings = 0;
    std::vector<uint32_t> free_mask;
    std::vector<uint8_t> n_free;                        /* with want_n_free */
    ssf_navfoot_stats stats;
};

/* planPoses (ssf_navpose.h; exported by libssf_hip_pose.so, linked INSTEAD of the other libraries -- a program that does not call it
 * links as before): the cost-to-goal field over (cell, heading bin) of the body whose layers footprintLayers made, and the state
 * paths down it.  The members start at ssf_navpose_default_params' values; the heading bins are the layers'. */
struct PosePlanParams {
    int min_dist2 = 0;
    int soft_dist2 = 0, near_penalty = 0;              /* extra cost below a squared clearance; 0 = none */
    int move_tol = 64;                                  /* direction units between heading and move, 0..256 */
    bool allow_reverse = true;
    int reverse_cost = 10, turn_cost = 5;
    int max_path = 0;                                   /* states per path; 0 = no paths */
    bool want_cost = false, want_cells = true;          /* the field over the states; its projection onto the cells */
};
typedef std::array<int32_t, 3> PoseState;              /* (ix, iy, bin); as a goal, bin -1 = every bin the body fits at */
/* what planPoses makes: the field, layer-major n_headings x height x width; cell_cost (steerWithFootprint's cost term: costAsPlan)
 * and cell_bin, height x width; per start its cost, status (ssf_navpose.h step 9) and the states of its path */
struct PosePlan {
    int width = 0, height = 0, n_headings = 0;
    std::vector<uint32_t> cost;                         /* with want_cost; 0xFFFFFFFF = not reached */
    std::vector<uint32_t> cell_cost;
    std::vector<uint8_t> cell_bin;                      /* 255 = no bin reached */
    std::vector<uint32_t> start_cost;
    std::vector<int32_t> start_status;
    std::vector<std::vector<PoseState> > paths;
    ssf_navpose_stats stats;
    /* cell_cost as the plan steerWithFootprint scores against */
    NavPlan costAsPlan() const { NavPlan p; p.width = width; p.height = height; p.cost = cell_cost; p.stats = ssf_navplan_stats(); return p; }
};

/* steerAmongMovers, steerFootprintAmongMovers and moverBlobs (ssf_navdyn.h; exported by libssf_hip_dyn.so, linked INSTEAD of the other
 * libraries -- a program that calls none of them links as before): the rollouts refused where they meet a predicted mover and scored
 * by the gap they keep, and the moving pixels of a depth frame as blobs in the grid frame.  Units as in ssf_navdyn.h: sub-units
 * (1024 per cell) and sub-units per step. */
struct Mover { int32_t x, y, vx, vy, r, grow; };
struct MoverBlob { int32_t label, n, cx, cy, r, ex, ey, pad; };
struct MoverParams {
    int mover_cap = 4096, mover_weight = 1;             /* ssf_navdyn_default_params' values */
    bool want_candidates = false;                       /* cand_hit and cand_min_gap, n_poses x K */
};
/* what the two steering members make: a NavSteer (fillTwist and fillLocalPlan take it as it is) with the winner's smallest gap per pose
 * (-1: no winner) and, with want_candidates, the mover that ended each rollout (-1: none) and each rollout's smallest gap */
struct NavSteerAmongMovers : NavSteer {
    std::vector<int32_t> min_gap, cand_hit, cand_min_gap;
    ssf_navdyn_stats dyn;
};
struct MoverBlobParams {
    int min_points = 16, max_blobs = SSF_NAVDYN_MAX_BLOBS;
};
struct MoverBlobs {
    std::vector<MoverBlob> blobs;                       /* ordered by (-n, label) */
    ssf_navdyn_blob_stats stats;
};
/* From two successive blob tables to movers: host only, integer only (ssf_navdyn.h part C; binding.MoverTracker states the same rule).
 * gate: the largest centre distance of a match; inflate: added to every radius (the robot's own radius goes here); grow: the growth
 * of a matched mover per step; grow_unmatched: that of a blob without a predecessor, whose velocity is taken as 0. */
class MoverTracker {
public:
    explicit MoverTracker(int gate = 2048, int inflate = 0, int grow = 16, int grow_unmatched = 128)
        : gate_(gate), inflate_(inflate), grow_(grow), grow_unmatched_(grow_unmatched) {}
    void reset() { prev_.clear(); }
    /* steps_since >= 1: the rollout steps between the previous table and this one.  Every field is clamped to the call's bounds. */
    std::vector<Mover> update(const std::vector<MoverBlob>& blobs, int steps_since = 1) {
        if (steps_since < 1 || blobs.size() > (size_t)SSF_NAVDYN_MAX_BLOBS) throw std::invalid_argument("MoverTracker::update takes at most 64 blobs and steps_since >= 1");
        std::vector<bool> used(prev_.size(), false);
        std::vector<Mover> out(blobs.size());
        for (size_t i = 0; i < blobs.size(); i++) {
            const long long cx = blobs[i].cx, cy = blobs[i].cy;
            long long best_d2 = -1; size_t best = 0;
            for (size_t j = 0; j < prev_.size(); j++) {
                if (used[j]) continue;
                const long long dx = cx - prev_[j].cx, dy = cy - prev_[j].cy, d2 = dx * dx + dy * dy;
                if (d2 <= (long long)gate_ * gate_ && (best_d2 < 0 || d2 < best_d2)) { best_d2 = d2; best = j; }      /* (j grows: the smaller index wins a tie) */
            }
            long long vx = 0, vy = 0, grow = grow_unmatched_;
            if (best_d2 >= 0) {
                used[best] = true;
                vx = floor_div(cx - prev_[best].cx, steps_since); vy = floor_div(cy - prev_[best].cy, steps_since); grow = grow_;
            }
            Mover& m = out[i];
            m.x = clamp(cx, -(1 << 24), 1 << 24); m.y = clamp(cy, -(1 << 24), 1 << 24); m.vx = clamp(vx, -4096, 4096); m.vy = clamp(vy, -4096, 4096);
            m.r = clamp((long long)blobs[i].r + inflate_, 0, 1 << 20); m.grow = clamp(grow, 0, 4096);
        }
        prev_ = blobs;
        return out;
    }
private:
    static long long floor_div(long long a, long long b) { const long long q = a / b; return (a % b != 0 && ((a < 0) != (b < 0))) ? q - 1 : q; }
    static int32_t clamp(long long v, long long lo, long long hi) { return (int32_t)(v < lo ? lo : (v > hi ? hi : v)); }
    int gate_, inflate_, grow_, grow_unmatched_;
    std::vector<MoverBlob> prev_;
};

/* castRays (ssf_raycast.h; exported by libssf_hip.so only): the first disc of the map that each ray hits.  The members start at
 * ssf_raycast_default_params' values: pose nullptr = the tracked pose, t_min = t_max = 0 = the configured depth range, splat_scale
 * 0 = 3, cell 0 = 0.125 m, hash_bits 0 = chosen by the library */
struct RaycastParams {
    const Transform3* pose = nullptr;              /* ray-frame-to-map */
    float t_min = 0.f, t_max = 0.f, min_conf = 0.f, splat_scale = 0.f;
    bool visible_only = false;
    float cell = 0.f; int hash_bits = 0;
    bool want_t = true, want_index = true, want_point = true, want_normal = true, want_color = true;   /* false: its vector stays empty */
};
/* per ray: t (a multiple of the direction; 0 on a miss), index into getModelHost() (-1 on a miss), hit point, normal facing the
 * ray's origin and colour (all 0 on a miss), map frame */
struct RaycastResult {
    std::vector<float> t;
    std::vector<int32_t> index;
    std::vector<float3> point, normal, color;
    ssf_raycast_stats stats;
};

/* the deformation graph's binding (ssf_graph.h): four node indices and four weights per row, in getModelHost()'s row order */
struct GraphBinding {
    std::vector<float> weights4;
    std::vector<int32_t> idx4;
    size_t size() const { return idx4.size() / 4; }
};

/* one stored keyframe (ssf_keyframes.h): its rows, pose (12 floats, ssf_get_pose's layout), stamp and codes (one byte per fern) */
struct Keyframe {
    HostSupersurfels rows;
    float pose[12];
    int stamp = 0;
    std::vector<uint8_t> codes;
};
/* what ssf_align / ssf_keyframes_align report */
struct KeyframeAlignment { float rel_pose[12]; bool valid = false; int iters = 0, pairs = 0; };

class SupersurfelFusion {
public:
    SupersurfelFusion() = default;
    SupersurfelFusion(const SupersurfelFusion&) = delete;
    SupersurfelFusion& operator=(const SupersurfelFusion&) = delete;
    ~SupersurfelFusion() { if (h_) ssf_destroy(h_); }

    /* initialize(): supersurfel_fusion.hpp:46-74 -- the reference's complete parameter list, in its order and with its
     * defaults, so that the nodes' calls (node/supersurfel_fusion_node.cpp:256-284,
     * node/supersurfel_fusion_rgbd_benchmark_node.cpp: same 29 positional arguments) compile unchanged.  The 21
     * path-relevant arguments map 1:1 onto ssf_config; the last eight configure the reference's sparse VO (ORB
     * features), loop closure and MOD, which are outside this library (their outputs enter processFrame as `vo_pose`
     * and `dynamic`): accepted and ignored.  What this library adds -- pipelining, batching, the pre-filter switch --
     * is set by name BEFORE initialize (setPipeline / setDepthPrefilter below) or through initialize(const ssf_config&);
     * the defaults are the reference's behaviour: one frame in flight, processFrame filters the depth image first
     * (supersurfel_fusion.cu:180). */
    void initialize(const CamParam& cam, int cell_size = 16, float lambda_pos = 50.f, float lambda_bound = 1000.f,
                    float lambda_size = 10000.f, float lambda_disp = 1e6f, float thresh_disp = 1e-4f,
                    int seg_iter = 10, bool seg_use_ransac = true, int nb_samples = 16, int filter_iter = 4,
                    float filter_alpha = 0.1f, float filter_beta = 1.0f, float filter_threshold = 0.05f,
                    float range_min = 0.2f, float range_max = 5.0f, int delta_t = 20, float conf_thresh = 2500.f,
                    int nb_supersurfels_max = 50000, int icp_iter = 10, double icp_cov_thresh = 0.04,
                    int nb_features = 2000, float features_scale_factor = 1.2f, int features_nb_levels = 8,
                    int ini_th_fast = 20, int min_th_fast = 7, int untracked_threshold = 10,
                    bool enable_loop_closure = true, bool enable_mod = true) {
        (void)nb_features; (void)features_scale_factor; (void)features_nb_levels; (void)ini_th_fast; (void)min_th_fast;
        (void)untracked_threshold; (void)enable_loop_closure; (void)enable_mod;
        ssf_config c; ssf_default_config(&c);
        c.width = cam.width; c.height = cam.height; c.fx = cam.fx; c.fy = cam.fy; c.cx = cam.cx; c.cy = cam.cy;
        c.cell_size = cell_size; c.lambda_pos = lambda_pos; c.lambda_bound = lambda_bound; c.lambda_size = lambda_size;
        c.lambda_disp = lambda_disp; c.thresh_disp = thresh_disp; c.seg_iter = seg_iter; c.seg_use_ransac = seg_use_ransac ? 1 : 0;
        c.nb_samples = nb_samples; c.filter_iter = filter_iter; c.filter_alpha = filter_alpha; c.filter_beta = filter_beta;
        c.filter_threshold = filter_threshold; c.range_min = range_min; c.range_max = range_max; c.delta_t = delta_t;
        c.conf_thresh = conf_thresh; c.nb_supersurfels_max = nb_supersurfels_max; c.icp_iter = icp_iter;
        c.icp_cov_thresh = icp_cov_thresh; c.pipeline_depth = pipeline_depth_; c.extract_batch = extract_batch_;
        c.depth_prefilter = depth_prefilter_ ? 1 : 0;
        initialize(c);
    }
    /* library-specific knobs, by name; they take effect at the next initialize().  pipeline_depth / extract_batch: see
     * ssf_config (0 / 1 = the reference's one-frame-in-flight behaviour; 2 / 8 for replay through processSequence).
     * depth_prefilter false = the caller hands over the depth it wants segmented. */
    void setPipeline(int pipeline_depth, int extract_batch) { pipeline_depth_ = pipeline_depth; extract_batch_ = extract_batch; }
    void setDepthPrefilter(bool on) { depth_prefilter_ = on; }
    void initialize(const ssf_config& c) {
        if (h_) { ssf_destroy(h_); h_ = nullptr; }
        if (ssf_create(&c, &h_) != SSF_OK) { h_ = nullptr; throw std::runtime_error(ssf_last_error(nullptr)); }
        width_ = c.width; height_ = c.height; depth_u16_ = false;
    }
    /* raw sensor frames (ssf_input.h; exported by libssf_hip.so only): after initialize(), which resets the handle to RGB8 +
     * float metres.  color: SSF_COLOR_RGB8 / BGR8 / RGBA8 / BGRA8; depth: SSF_DEPTH_F32_METRES or SSF_DEPTH_U16_SCALED with
     * depth_scale metres per count (the node's depthScale, 0.0002 for TUM).  Then
     *     ssf.setInputFormat(SSF_COLOR_BGR8, SSF_DEPTH_U16_SCALED, depthScale);
     *     ssf.processFrame(rgb_ptr, depth_u16_ptr);              // or the cv::Mat overload with CV_8UC3 (BGR) + CV_16UC1
     * replace the node's cvtColor / convertTo. */
    void setInputFormat(ssf_color_format color, ssf_depth_format depth, double depth_scale = 1.0) {
        check(ssf_set_input_format(need(), color, depth, depth_scale));
        depth_u16_ = depth == SSF_DEPTH_U16_SCALED;
    }
    bool isInitialized() const { return h_ != nullptr; }

    /* processFrame(): supersurfel_fusion.hpp:75-76.  rgb: H x W x 3 bytes in RGB order, depth: H x W floats in
     * metres (0 = hole) -- what RGBDCallback / run() build (convertTo(CV_32FC1, depthScale)).  vo_pose: the sparse-VO
     * pose prior (supersurfel_fusion.cu:225-228; row-major R then t; nullptr = previous pose); dynamic: the MOD
     * mask, one byte per superpixel (motion_detection.cu:573-578; nullptr = none). */
    void processFrame(const uint8_t* rgb, const float* depth_m, const float* vo_pose = nullptr, const uint8_t* dynamic = nullptr) {
        if (depth_u16_) throw std::logic_error("processFrame: the input format is uint16 depth; pass the counts as const uint16_t*");
        check(ssf_process_frame(need(), rgb, depth_m, vo_pose, dynamic, &last_));
    }
    /* the same with H x W uint16 depth counts: needs setInputFormat(..., SSF_DEPTH_U16_SCALED, scale) first; rgb in the
     * colour format set there */
    void processFrame(const uint8_t* rgb, const uint16_t* depth_counts, const float* vo_pose = nullptr, const uint8_t* dynamic = nullptr) {
        if (!depth_u16_) throw std::logic_error("processFrame(uint16_t depth): call setInputFormat(..., SSF_DEPTH_U16_SCALED, scale) first");
        check(ssf_process_frame(need(), rgb, reinterpret_cast<const float*>(depth_counts), vo_pose, dynamic, &last_));
    }
    /* a per-pixel mask of moving objects (ssf_dynamic.h; exported by libssf_hip.so only): H x W bytes, non-zero = dynamic, e.g. a
     * detector's person boxes rasterised.  The superpixels of which at least half the pixels are masked get confidence -1, as
     * with the reference's MOD.  The mask is wrapped so that processFrame(rgb, depth, nullptr) stays the pose-prior overload:
     *     ssf.processFrame(rgb_ptr, depth_ptr, supersurfel_fusion::PixelMask(mask_ptr), vo_pose);
     * PixelMask(nullptr) = no mask. */
    void processFrame(const uint8_t* rgb, const float* depth_m, PixelMask pixel_mask, const float* vo_pose = nullptr) {
        if (depth_u16_) throw std::logic_error("processFrame: the input format is uint16 depth; pass the counts as const uint16_t*");
        check(ssf_process_frame_pixmask(need(), rgb, depth_m, 0, vo_pose, pixel_mask.data, &last_));
    }
    void processFrame(const uint8_t* rgb, const uint16_t* depth_counts, PixelMask pixel_mask, const float* vo_pose = nullptr) {
        if (!depth_u16_) throw std::logic_error("processFrame(uint16_t depth): call setInputFormat(..., SSF_DEPTH_U16_SCALED, scale) first");
        check(ssf_process_frame_pixmask(need(), rgb, depth_counts, 0, vo_pose, pixel_mask.data, &last_));
    }
    /* the dynamic superpixels of the last frame by its pixel mask (S bytes, 1 = dynamic; all 0 without a mask) */
    std::vector<uint8_t> getDynamicSuperpixels() {
        std::vector<uint8_t> v((size_t)getnbSuperpixels());
        check(ssf_get_dynamic_superpixels(need(), v.data(), nullptr));
        return v;
    }
    /* Moving objects from the depth frame and the map (ssf_motion.h; exported by libssf_hip.so only): pixels clearly in front of
     * a surface the map knows, grown over depth-continuous pixels the map says nothing about.  detectMotion only looks (no state
     * changes); processFrame(rgb, depth, MotionParams()) detects on the device and processes the frame with that pixel mask, which
     * getMotionMask() returns afterwards. */
    MotionMask detectMotion(const float* depth_m, const MotionParams& mp = MotionParams()) {
        if (depth_u16_) throw std::logic_error("detectMotion: the input format is uint16 depth; pass the counts as const uint16_t*");
        return detect_motion(depth_m, mp);
    }
    MotionMask detectMotion(const uint16_t* depth_counts, const MotionParams& mp = MotionParams()) {
        if (!depth_u16_) throw std::logic_error("detectMotion(uint16_t depth): call setInputFormat(..., SSF_DEPTH_U16_SCALED, scale) first");
        return detect_motion(depth_counts, mp);
    }
    MotionMask detectMotion(const std::vector<float>& depth_m, const MotionParams& mp = MotionParams()) {
        if (depth_m.size() != (size_t)width_ * (size_t)height_) throw std::invalid_argument("detectMotion: the depth image must be width x height");
        return detectMotion(depth_m.data(), mp);
    }
    void processFrame(const uint8_t* rgb, const float* depth_m, const MotionParams& mp, const float* vo_pose = nullptr) {
        if (depth_u16_) throw std::logic_error("processFrame: the input format is uint16 depth; pass the counts as const uint16_t*");
        const ssf_motion_params p = motion_params(mp);
        check(ssf_process_frame_motion(need(), rgb, depth_m, 0, vo_pose, &p, &last_));
    }
    void processFrame(const uint8_t* rgb, const uint16_t* depth_counts, const MotionParams& mp, const float* vo_pose = nullptr) {
        if (!depth_u16_) throw std::logic_error("processFrame(uint16_t depth): call setInputFormat(..., SSF_DEPTH_U16_SCALED, scale) first");
        const ssf_motion_params p = motion_params(mp);
        check(ssf_process_frame_motion(need(), rgb, depth_counts, 0, vo_pose, &p, &last_));
    }
    /* the mask of the last processFrame(rgb, depth, MotionParams) */
    MotionMask getMotionMask() {
        MotionMask m;
        m.width = width_; m.height = height_; m.mask.resize((size_t)width_ * (size_t)height_);
        check(ssf_get_motion_mask(need(), m.mask.data(), &m.stats));
        return m;
    }
    /* Dense RGB-D odometry, the pose prior of the library's own (ssf_odometry.h; exported by libssf_hip.so only).
     * setOdometryReference keeps a frame's pyramid (ref_mask: H x W, non-zero = ignore, or nullptr); estimateOdometry aligns a frame
     * to it (init: 12 floats current camera -> reference camera, or nullptr) and leaves it; trackOdometry also makes the frame the
     * next reference and returns the prior; processFrame(rgb, depth, OdometryParams()) tracks, then processes the frame with that
     * prior (the first frame, and a frame whose estimate is invalid, without one); getOdometry returns the last track. */
    void setOdometryReference(const uint8_t* rgb, const float* depth_m, const uint8_t* ref_mask = nullptr) {
        if (depth_u16_) throw std::logic_error("setOdometryReference: the input format is uint16 depth; pass the counts as const uint16_t*");
        check(ssf_odometry_set_reference(need(), rgb, depth_m, 0, ref_mask));
    }
    void setOdometryReference(const uint8_t* rgb, const uint16_t* depth_counts, const uint8_t* ref_mask = nullptr) {
        if (!depth_u16_) throw std::logic_error("setOdometryReference(uint16_t depth): call setInputFormat(..., SSF_DEPTH_U16_SCALED, scale) first");
        check(ssf_odometry_set_reference(need(), rgb, depth_counts, 0, ref_mask));
    }
    OdometryEstimate estimateOdometry(const uint8_t* rgb, const float* depth_m, const OdometryParams& op = OdometryParams(), const float* init = nullptr) {
        if (depth_u16_) throw std::logic_error("estimateOdometry: the input format is uint16 depth; pass the counts as const uint16_t*");
        return estimate_odometry(rgb, depth_m, op, init);
    }
    OdometryEstimate estimateOdometry(const uint8_t* rgb, const uint16_t* depth_counts, const OdometryParams& op = OdometryParams(), const float* init = nullptr) {
        if (!depth_u16_) throw std::logic_error("estimateOdometry(uint16_t depth): call setInputFormat(..., SSF_DEPTH_U16_SCALED, scale) first");
        return estimate_odometry(rgb, depth_counts, op, init);
    }
    OdometryEstimate trackOdometry(const uint8_t* rgb, const float* depth_m, const OdometryParams& op = OdometryParams()) {
        if (depth_u16_) throw std::logic_error("trackOdometry: the input format is uint16 depth; pass the counts as const uint16_t*");
        return track_odometry(rgb, depth_m, op);
    }
    OdometryEstimate trackOdometry(const uint8_t* rgb, const uint16_t* depth_counts, const OdometryParams& op = OdometryParams()) {
        if (!depth_u16_) throw std::logic_error("trackOdometry(uint16_t depth): call setInputFormat(..., SSF_DEPTH_U16_SCALED, scale) first");
        return track_odometry(rgb, depth_counts, op);
    }
    void processFrame(const uint8_t* rgb, const float* depth_m, const OdometryParams& op) {
        if (depth_u16_) throw std::logic_error("processFrame: the input format is uint16 depth; pass the counts as const uint16_t*");
        const ssf_odometry_params p = odometry_params(op);
        check(ssf_process_frame_odometry(need(), rgb, depth_m, 0, &p, nullptr, &last_));
    }
    void processFrame(const uint8_t* rgb, const uint16_t* depth_counts, const OdometryParams& op) {
        if (!depth_u16_) throw std::logic_error("processFrame(uint16_t depth): call setInputFormat(..., SSF_DEPTH_U16_SCALED, scale) first");
        const ssf_odometry_params p = odometry_params(op);
        check(ssf_process_frame_odometry(need(), rgb, depth_counts, 0, &p, nullptr, &last_));
    }
    /* ... with the moving-object detector on top: its mask is rendered at the odometry prior */
    void processFrame(const uint8_t* rgb, const float* depth_m, const OdometryParams& op, const MotionParams& mp) {
        if (depth_u16_) throw std::logic_error("processFrame: the input format is uint16 depth; pass the counts as const uint16_t*");
        const ssf_odometry_params p = odometry_params(op);
        const ssf_motion_params m = motion_params(mp);
        check(ssf_process_frame_odometry(need(), rgb, depth_m, 0, &p, &m, &last_));
    }
    OdometryEstimate getOdometry() {
        OdometryEstimate e;
        check(ssf_get_odometry(need(), e.rel, e.prior, &e.result));
        e.has_prior = e.result.valid != 0;
        return e;
    }
    /* replay of a recorded sequence (SupersurfelFusionRGBDBenchmarkNode::run): host images of n frames, results in
     * order; with pipeline_depth / extract_batch > 0 / 1 the extract stage runs ahead (bit-identical results) */
    std::vector<ssf_frame_result> processSequence(const std::vector<const uint8_t*>& rgb, const std::vector<const float*>& depth_m) {
        if (rgb.size() != depth_m.size()) throw std::invalid_argument("processSequence: rgb / depth counts differ");
        std::vector<const void*> r(rgb.begin(), rgb.end()), d(depth_m.begin(), depth_m.end());
        std::vector<ssf_frame_result> out(rgb.size());
        if (depth_u16_) throw std::logic_error("processSequence: the input format is uint16 depth; pass the counts as const uint16_t*");
        check(ssf_process_sequence(need(), r.data(), d.data(), (int)rgb.size(), 0, out.data()));
        if (!out.empty()) last_ = out.back();
        return out;
    }
    std::vector<ssf_frame_result> processSequence(const std::vector<const uint8_t*>& rgb, const std::vector<const uint16_t*>& depth_counts) {
        if (rgb.size() != depth_counts.size()) throw std::invalid_argument("processSequence: rgb / depth counts differ");
        if (!depth_u16_) throw std::logic_error("processSequence(uint16_t depth): call setInputFormat(..., SSF_DEPTH_U16_SCALED, scale) first");
        std::vector<const void*> r(rgb.begin(), rgb.end()), d(depth_counts.begin(), depth_counts.end());
        std::vector<ssf_frame_result> out(rgb.size());
        check(ssf_process_sequence(need(), r.data(), d.data(), (int)rgb.size(), 0, out.data()));
        if (!out.empty()) last_ = out.back();
        return out;
    }
#ifdef CV_VERSION
    /* the reference's own signatures (supersurfel_fusion.hpp:75-80); compiled against a cv::Mat test double by
     * tests/test_cpp_wrapper.py (tests/cpp/cv_double.hpp) since OpenCV is not in the build image */
    void processFrame(const cv::Mat& rgb_h, const cv::Mat& depth_h, const float* vo_pose = nullptr, const uint8_t* dynamic = nullptr) {
        const cv::Mat rgb = rgb_h.isContinuous() ? rgb_h : rgb_h.clone(), d = depth_h.isContinuous() ? depth_h : depth_h.clone();
#ifdef CV_16UC1
        /* the sensor's CV_16UC1 depth (and its colour, BGR from cv_bridge) as they come, once setInputFormat has said so */
        if (d.type() == CV_16UC1) { processFrame(rgb.ptr<uint8_t>(), d.ptr<uint16_t>(), vo_pose, dynamic); return; }
#endif
        processFrame(rgb.ptr<uint8_t>(), d.ptr<float>(), vo_pose, dynamic);
    }
#ifdef CV_8UC1
    /* ... with a CV_8UC1 pixel mask of the frame's size (non-zero = moving object; an empty Mat = no mask), e.g. the node's
     * YOLO person boxes drawn filled into a zero image */
    void processFrame(const cv::Mat& rgb_h, const cv::Mat& depth_h, const cv::Mat& pixel_mask, const float* vo_pose = nullptr) {
        if (pixel_mask.rows == 0 && pixel_mask.cols == 0) { processFrame(rgb_h, depth_h, vo_pose); return; }
        if (pixel_mask.type() != CV_8UC1 || pixel_mask.rows != height_ || pixel_mask.cols != width_)
            throw std::invalid_argument("processFrame: the pixel mask must be CV_8UC1 of the frame's size");
        const cv::Mat rgb = rgb_h.isContinuous() ? rgb_h : rgb_h.clone(), d = depth_h.isContinuous() ? depth_h : depth_h.clone();
        const cv::Mat m = pixel_mask.isContinuous() ? pixel_mask : pixel_mask.clone();
#ifdef CV_16UC1
        if (d.type() == CV_16UC1) { processFrame(rgb.ptr<uint8_t>(), d.ptr<uint16_t>(), PixelMask(m.ptr<uint8_t>()), vo_pose); return; }
#endif
        processFrame(rgb.ptr<uint8_t>(), d.ptr<float>(), PixelMask(m.ptr<uint8_t>()), vo_pose);
    }
    /* ... the detector on a CV_32FC1 (or, after setInputFormat, CV_16UC1) depth image: the mask as CV_8UC1, 1 = moving object */
    cv::Mat detectMotion(const cv::Mat& depth_h, const MotionParams& mp = MotionParams()) {
        if (depth_h.rows != height_ || depth_h.cols != width_) throw std::invalid_argument("detectMotion: the depth image must be of the frame's size");
        const cv::Mat d = depth_h.isContinuous() ? depth_h : depth_h.clone();
#ifdef CV_16UC1
        const MotionMask m = d.type() == CV_16UC1 ? detectMotion(d.ptr<uint16_t>(), mp) : detectMotion(d.ptr<float>(), mp);
#else
        const MotionMask m = detectMotion(d.ptr<float>(), mp);
#endif
        cv::Mat out;
        out.create(height_, width_, CV_8UC1);
        std::copy(m.mask.begin(), m.mask.end(), out.ptr<uint8_t>());
        return out;
    }
    void processFrame(const cv::Mat& rgb_h, const cv::Mat& depth_h, const MotionParams& mp, const float* vo_pose = nullptr) {
        if (rgb_h.rows != height_ || rgb_h.cols != width_ || depth_h.rows != height_ || depth_h.cols != width_)
            throw std::invalid_argument("processFrame: the colour and depth images must be of the frame's size");
        const cv::Mat rgb = rgb_h.isContinuous() ? rgb_h : rgb_h.clone(), d = depth_h.isContinuous() ? depth_h : depth_h.clone();
#ifdef CV_16UC1
        if (d.type() == CV_16UC1) { processFrame(rgb.ptr<uint8_t>(), d.ptr<uint16_t>(), mp, vo_pose); return; }
#endif
        processFrame(rgb.ptr<uint8_t>(), d.ptr<float>(), mp, vo_pose);
    }
#endif
#if defined(CV_8UC3) && defined(CV_32FC1)
    /* ... as images of the handle's camera: rgb CV_8UC3, depth CV_32FC1 (metres, 0 = nothing) */
    void renderModel(const Transform3& pose, cv::Mat& rgb, cv::Mat& depth) {
        ssf_render_params p;
        check(ssf_render_default_params(need(), &p));
        float v[12];
        transform3_to_rt(pose, v);
        p.pose = v;
        rgb.create(height_, width_, CV_8UC3);
        depth.create(height_, width_, CV_32FC1);
        check(ssf_render_model(need(), &p, depth.ptr<float>(), nullptr, rgb.ptr<uint8_t>(), nullptr, nullptr, nullptr));
    }
#endif
    void computeSuperpixelSegIm(cv::Mat& seg_im) {                     /* CV_8UC3, supersurfel_fusion.cu:635-640 */
        seg_im.create(height_, width_, CV_8UC3);
        check(ssf_get_preview_image(need(), seg_im.ptr<uint8_t>()));
    }
    void computeSlantedPlaneIm(cv::Mat& slanted_plane_im) {            /* CV_32FC1, supersurfel_fusion.cu:642-647 */
        slanted_plane_im.create(height_, width_, CV_32FC1);
        check(ssf_get_plane_depth(need(), slanted_plane_im.ptr<float>()));
    }
#endif
    /* The model drawn into a pinhole camera at `pose` (camera-to-map) on the device (ssf_render.h): every supersurfel is the
     * ellipse inscribed in the reference node's marker quad, the nearest one wins.  Replaces the node's getModelHost() copy-out
     * for its markers. */
    void renderModel(const Transform3& pose, RenderedView& out, const RenderOptions& o = RenderOptions()) {
        ssf_render_params p;
        check(ssf_render_default_params(need(), &p));
        float v[12];
        transform3_to_rt(pose, v);
        p.pose = v;
        if (o.width != 0) { p.width = o.width; p.height = o.height; p.fx = o.fx; p.fy = o.fy; p.cx = o.cx; p.cy = o.cy; }
        if (o.z_min != 0.f || o.z_max != 0.f) { p.z_min = o.z_min; p.z_max = o.z_max; }
        p.min_conf = o.min_conf; p.splat_scale = o.splat_scale; p.visible_only = o.visible_only ? 1 : 0; p.on_device = 0;
        const size_t n = (p.width >= 1 && p.height >= 1) ? (size_t)p.width * (size_t)p.height : 1;
        out.width = p.width; out.height = p.height;
        out.depth.resize(n); out.index.resize(n); out.rgb8.resize(3 * n); out.color.resize(3 * n); out.normal.resize(3 * n);
        check(ssf_render_model(need(), &p, out.depth.data(), out.index.data(), out.rgb8.data(), out.color.data(), out.normal.data(),
                               &out.stats));
    }
    /* Rows of the map selected on the device by region, age and confidence (ssf_query.h): how many there are and their bounding
     * box (countModel), or the rows themselves (queryModel) -- without the copy of the whole map that getModelHost() makes. */
    ssf_query_stats countModel(const QueryParams& q) {
        ssf_query_params p; float v[12];
        query_params(q, p, v);
        ssf_query_stats s;
        check(ssf_query_count(need(), &p, &s));
        return s;
    }
    void queryModel(const QueryParams& q, QueryResult& out) {
        ssf_query_params p; float v[12];
        query_params(q, p, v);
        check(ssf_query_count(need(), &p, &out.stats));
        for (int attempt = 0;; attempt++) {             /* sized from the count; repeated once should the call name another size */
            const int n = (int)out.stats.n_selected;
            out.rows.resize(n); out.index.resize((size_t)(n > 0 ? n : 1));
            ssf_surfels view = out.rows.view();
            const int rc = ssf_query_rows(need(), &p, &view, out.index.data(), n, &out.stats);
            if (rc == SSF_ERR_CAPACITY && attempt == 0) continue;
            check(rc);
            break;
        }
        out.rows.resize((int)out.stats.n_selected); out.index.resize((size_t)out.stats.n_selected);
    }
    /* extractLocalPointCloud (supersurfel_fusion.hpp; extractLocalPointCloud kernel, supersurfel_fusion_kernels.cu:490): the part of
     * the map within `radius` of the current pose's position, for a planner or a local visualiser -- positions, colours (sRGB
     * 0..255) and normals (orientation row 2) of the rows selected by a SSF_REGION_SPHERE query, in getModelHost()'s order. */
    void extractLocalPointCloud(float radius, std::vector<float3>& positions, std::vector<float3>& colors, std::vector<float3>& normals) {
        ssf_query_params p;
        check(ssf_query_default_params(need(), &p));
        p.region = SSF_REGION_SPHERE; p.radius = radius;
        ssf_query_stats s;
        check(ssf_query_count(need(), &p, &s));
        std::vector<float> ori;
        for (int attempt = 0;; attempt++) {
            const size_t n = (size_t)s.n_selected, m = n > 0 ? n : 1;
            positions.resize(m); colors.resize(m); ori.resize(9 * m);
            ssf_surfels view = {reinterpret_cast<float*>(positions.data()), reinterpret_cast<float*>(colors.data()), nullptr, ori.data(),
                                nullptr, nullptr, nullptr};
            const int rc = ssf_query_rows(need(), &p, &view, nullptr, (int)n, &s);
            if (rc == SSF_ERR_CAPACITY && attempt == 0) continue;
            check(rc);
            break;
        }
        const size_t n = (size_t)s.n_selected;
        positions.resize(n); colors.resize(n); normals.resize(n);
        for (size_t i = 0; i < n; i++) { normals[i].x = ori[9 * i + 6]; normals[i].y = ori[9 * i + 7]; normals[i].z = ori[9 * i + 8]; }
    }
    /* The floor-plane navigation grid of the map, built on the device (ssf_navgrid.h): per cell the height range, the floor and
     * obstacle hit counts, the occupancy state and the squared clearance -- without the copy of the whole map, the host
     * rasteriser and the host distance transform a node would otherwise need.  INTEGRATION.md section 2 has the publishing side. */
    void buildNavGrid(const NavGridParams& g, NavGrid& out) {
        ssf_navgrid_params p; float v[12];
        const ssf_navgrid_out o = navGridCall(g, p, v, out);
        check(ssf_navgrid_build(need(), &p, &o, &out.stats));
    }
    /* The same grid with free space carved along the rays of `views` (ssf_navcarve.h): n camera-to-map poses of 12 floats each
     * (R row-major, then t: transform3_to_rt), e.g. the node's trajectory so far.  out.seen counts, per cell, the rays that crossed
     * the band of the robot's body before their hit; out.state and out.dist2 are carved, and fillOccupancyGrid takes out as it is. */
    void buildNavGrid(const NavGridParams& g, const CarveParams& c, const float* views12, int n_views, CarvedNavGrid& out) {
        ssf_navgrid_params p; float v[12];
        ssf_navcarve_out o;
        o.grid = navGridCall(g, p, v, out);
        ssf_navcarve_params q;
        check(ssf_navcarve_default_params(need(), &q));
        q.views = views12; q.n_views = n_views;
        q.fx = c.fx; q.fy = c.fy; q.cx = c.cx; q.cy = c.cy; q.cam_width = c.width; q.cam_height = c.height; q.stride = c.stride;
        q.t_min = c.t_min; q.t_max = c.t_max; q.ray_min_conf = c.ray_min_conf; q.ray_splat_scale = c.ray_splat_scale;
        q.hit_margin_cells = c.hit_margin_cells; q.carve_misses = c.carve_misses ? 1 : 0; q.min_seen = c.min_seen;
        out.seen.resize(c.want_seen ? (size_t)(out.width >= 1 && out.height >= 1 ? (size_t)out.width * (size_t)out.height : 1) : 0);
        o.seen = c.want_seen ? out.seen.data() : nullptr;
        check(ssf_navgrid_carve(need(), &p, &q, &o, &out.carve));
        out.stats = out.carve.grid;
    }
    void buildNavGrid(const NavGridParams& g, const CarveParams& c, const std::vector<std::array<float, 12> >& views, CarvedNavGrid& out) {
        buildNavGrid(g, c, views.empty() ? nullptr : views[0].data(), (int)views.size(), out);
    }
    /* The floor plane of the map, fitted on the device (ssf_navfloor.h): the lowest large set of rows whose normals agree with the up
     * hint and whose heights agree.  A status other than SSF_NAVFLOOR_OK is no error: out.fit says how far the fit came. */
    void fitFloor(const FloorParams& f, FloorFit& out) {
        ssf_navfloor_params p;
        check(ssf_navfloor_default_params(need(), &p));
        float o[3];
        p.up[0] = f.up.x; p.up[1] = f.up.y; p.up[2] = f.up.z;
        if (f.origin) { o[0] = f.origin->x; o[1] = f.origin->y; o[2] = f.origin->z; p.origin = o; }
        p.tilt_cos = f.tilt_cos; p.align_cos = f.align_cos; p.height_res = f.height_res;
        p.min_rows = f.min_rows; p.floor_share256 = f.floor_share256; p.refine_iters = f.refine_iters;
        p.first_dist = f.first_dist; p.inlier_dist = f.inlier_dist; p.min_conf = f.min_conf;
        p.t_init_min = f.t_init_min; p.t_init_max = f.t_init_max; p.t_last_min = f.t_last_min; p.t_last_max = f.t_last_max;
        p.visible_only = f.visible_only ? 1 : 0;
        p.width = f.width; p.height = f.height; p.res = f.res; p.below = f.below; p.step = f.step; p.body_height = f.body_height;
        out.dir_hist.assign(f.want_histograms ? SSF_NAVFLOOR_DIR_BINS * SSF_NAVFLOOR_DIR_BINS : 0, 0u);
        out.height_hist.assign(f.want_histograms ? SSF_NAVFLOOR_HEIGHT_BINS : 0, 0u);
        const ssf_navfloor_out o2 = {f.want_histograms ? out.dir_hist.data() : nullptr, f.want_histograms ? out.height_hist.data() : nullptr};
        check(ssf_navfloor_fit(need(), &p, &o2, &out.fit));
        out.pose = transform3_from_rt(out.fit.pose);
    }
    /* The fit, then the grid in its frame and bands: g's pose, bands, size and res are replaced by the fit's (f's width, height and
     * res), everything else of g holds. */
    void buildNavGridOnFloor(const FloorParams& f, NavGridParams g, FloorFit& fit, NavGrid& out) {
        fitFloor(f, fit);
        fit.applyTo(g);
        buildNavGrid(g, out);
    }
private:
    /* the C parameters of a grid call (v: room for the pose), out's vectors sized, and the output pointers into them */
    ssf_navgrid_out navGridCall(const NavGridParams& g, ssf_navgrid_params& p, float* v, NavGrid& out) {
        check(ssf_navgrid_default_params(need(), &p));
        if (g.pose) { transform3_to_rt(*g.pose, v); p.pose = v; }
        p.width = g.width; p.height = g.height; p.res = g.res;
        p.z_min = g.z_min; p.z_max = g.z_max; p.floor_max = g.floor_max; p.floor_cos = g.floor_cos; p.min_conf = g.min_conf;
        p.t_init_min = g.t_init_min; p.t_init_max = g.t_init_max; p.t_last_min = g.t_last_min; p.t_last_max = g.t_last_max;
        p.visible_only = g.visible_only ? 1 : 0; p.splat_scale = g.splat_scale; p.max_steps = g.max_steps; p.min_hits = g.min_hits;
        p.max_dist_cells = g.max_dist_cells; p.unknown_is_obstacle = g.unknown_is_obstacle ? 1 : 0; p.on_device = 0;
        const size_t n = (p.width >= 1 && p.height >= 1) ? (size_t)p.width * (size_t)p.height : 1;
        out.width = p.width; out.height = p.height; out.res = p.res;
        out.zmin.resize(g.want_heights ? n : 0); out.zmax.resize(g.want_heights ? n : 0); out.hits.resize(g.want_hits ? 2 * n : 0);
        out.state.resize(g.want_state ? n : 0); out.dist2.resize(g.want_dist2 ? n : 0);
        const ssf_navgrid_out o = {g.want_heights ? out.zmin.data() : nullptr, g.want_heights ? out.zmax.data() : nullptr,
                                   g.want_hits ? out.hits.data() : nullptr, g.want_state ? out.state.data() : nullptr,
                                   g.want_dist2 ? out.dist2.data() : nullptr};
        return o;
    }
public:
    /* The fields of a nav_msgs::OccupancyGrid that the grid determines: data, info.resolution, info.width, info.height and
     * info.origin (the map-frame pose of cell (0, 0)'s corner: the grid frame's t, and its rotation as a quaternion).  header and
     * info.map_load_time are the node's.  Any message type with these members works (tests use a double). */
    template <typename OccupancyGridT> static void fillOccupancyGrid(const NavGrid& g, OccupancyGridT& msg) {
        if (g.state.size() != (size_t)g.width * (size_t)g.height) throw std::logic_error("fillOccupancyGrid: the grid has no state (want_state)");
        msg.info.resolution = g.res; msg.info.width = (unsigned)g.width; msg.info.height = (unsigned)g.height;
        msg.data.assign(g.state.begin(), g.state.end());
        const float* R = g.stats.pose;
        msg.info.origin.position.x = R[9]; msg.info.origin.position.y = R[10]; msg.info.origin.position.z = R[11];
        /* rotation matrix (row-major) -> unit quaternion, the branch with the largest divisor */
        const double m00 = R[0], m01 = R[1], m02 = R[2], m10 = R[3], m11 = R[4], m12 = R[5], m20 = R[6], m21 = R[7], m22 = R[8];
        const double tr = m00 + m11 + m22;
        double qw, qx, qy, qz;
        if (tr > 0.0) { const double s = 2.0 * std::sqrt(tr + 1.0); qw = 0.25 * s; qx = (m21 - m12) / s; qy = (m02 - m20) / s; qz = (m10 - m01) / s; }
        else if (m00 > m11 && m00 > m22) { const double s = 2.0 * std::sqrt(1.0 + m00 - m11 - m22); qw = (m21 - m12) / s; qx = 0.25 * s; qy = (m01 + m10) / s; qz = (m02 + m20) / s; }
        else if (m11 > m22) { const double s = 2.0 * std::sqrt(1.0 + m11 - m00 - m22); qw = (m02 - m20) / s; qx = (m01 + m10) / s; qy = 0.25 * s; qz = (m12 + m21) / s; }
        else { const double s = 2.0 * std::sqrt(1.0 + m22 - m00 - m11); qw = (m10 - m01) / s; qx = (m02 + m20) / s; qy = (m12 + m21) / s; qz = 0.25 * s; }
        msg.info.origin.orientation.x = qx; msg.info.origin.orientation.y = qy; msg.info.origin.orientation.z = qz; msg.info.origin.orientation.w = qw;
    }
    /* The depth frame of the instant stamped onto a grid that buildNavGrid made, plain or carved, or onto an earlier live grid
     * (ssf_navlive.h): cells in which the frame's points lie in the band of the robot's body become occupied, unknown cells the
     * sensor looked through become free, and dist2 is recomputed.  g needs its state and stats.pose (its frame); depth is width x
     * height of the camera in the input format (float metres, or after setInputFormat uint16 counts); mask: empty, or one byte per
     * pixel for q.mask_mode (detectMotion's mask plugs in).  fillOccupancyGrid and planOnGrid take out as it is. */
    void overlayDepthFrame(const NavGrid& g, const LiveParams& q, const std::vector<float>& depth_m, const std::vector<uint8_t>& mask, LiveNavGrid& out) {
        if (depth_u16_) throw std::logic_error("overlayDepthFrame: the input format is uint16 depth; pass the counts as std::vector<uint16_t>");
        overlay_depth(g, q, depth_m.data(), depth_m.size(), mask, out);
    }
    void overlayDepthFrame(const NavGrid& g, const LiveParams& q, const std::vector<uint16_t>& depth_counts, const std::vector<uint8_t>& mask,
                           LiveNavGrid& out) {
        if (!depth_u16_) throw std::logic_error("overlayDepthFrame(uint16_t depth): call setInputFormat(..., SSF_DEPTH_U16_SCALED, scale) first");
        overlay_depth(g, q, depth_counts.data(), depth_counts.size(), mask, out);
    }
#if defined(CV_VERSION) && defined(CV_32FC1) && defined(CV_8UC1)
    /* ... with the depth as CV_32FC1 (or, after setInputFormat, CV_16UC1) and the mask as CV_8UC1 (an empty Mat = no mask) */
    void overlayDepthFrame(const NavGrid& g, const LiveParams& q, const cv::Mat& depth_h, const cv::Mat& mask_h, LiveNavGrid& out) {
        with_depth_mats(depth_h, mask_h, [&](const void* d, size_t n, const std::vector<uint8_t>& mk) { overlay_depth(g, q, d, n, mk, out); });
    }
#endif
    /* ... into a layer that REMEMBERS (ssf_navmem.h): the frame marks height slices of the band in mem, the rays that see through a
     * slice clear it, marks and seen-through cells older than mem's ages expire, and out is g -- the STATIC grid of every frame, the
     * map's own, not an earlier out -- with the marked cells occupied and the seen-through cells opened.  tick: >= 1 and monotone (a
     * frame counter).  q.min_seen and q.want_seen have no part in it; out.live_hits holds the frame's points per cell, out.live_seen
     * stays empty (mem.seen_bits has the slices seen through), out.live the counts both calls share, mem.stats all of them. */
    void overlayDepthFrame(const NavGrid& g, const LiveParams& q, const std::vector<float>& depth_m, const std::vector<uint8_t>& mask, LiveMemory& mem,
                           uint32_t tick, LiveNavGrid& out) {
        if (depth_u16_) throw std::logic_error("overlayDepthFrame: the input format is uint16 depth; pass the counts as std::vector<uint16_t>");
        remember_depth(g, q, depth_m.data(), depth_m.size(), mask, mem, tick, out);
    }
    void overlayDepthFrame(const NavGrid& g, const LiveParams& q, const std::vector<uint16_t>& depth_counts, const std::vector<uint8_t>& mask,
                           LiveMemory& mem, uint32_t tick, LiveNavGrid& out) {
        if (!depth_u16_) throw std::logic_error("overlayDepthFrame(uint16_t depth): call setInputFormat(..., SSF_DEPTH_U16_SCALED, scale) first");
        remember_depth(g, q, depth_counts.data(), depth_counts.size(), mask, mem, tick, out);
    }
#if defined(CV_VERSION) && defined(CV_32FC1) && defined(CV_8UC1)
    void overlayDepthFrame(const NavGrid& g, const LiveParams& q, const cv::Mat& depth_h, const cv::Mat& mask_h, LiveMemory& mem, uint32_t tick,
                           LiveNavGrid& out) {
        with_depth_mats(depth_h, mask_h, [&](const void* d, size_t n, const std::vector<uint8_t>& mk) { remember_depth(g, q, d, n, mk, mem, tick, out); });
    }
private:
    /* the two overloads above: the images made continuous, their types checked against the input format, and f(depth as uint16_t* or
     * float*, its pixels, the mask's bytes or none) */
    template <class F> void with_depth_mats(const cv::Mat& depth_h, const cv::Mat& mask_h, F f) {
        const cv::Mat d = depth_h.isContinuous() ? depth_h : depth_h.clone(), m = mask_h.isContinuous() ? mask_h : mask_h.clone();
        const size_t n = (size_t)d.rows * (size_t)d.cols;
        const bool masked = m.rows != 0 || m.cols != 0;
        if (masked && (m.type() != CV_8UC1 || m.rows != d.rows || m.cols != d.cols)) throw std::invalid_argument("overlayDepthFrame: the mask must be CV_8UC1 of the depth image's size");
        std::vector<uint8_t> mk;
        if (masked) mk.assign(m.ptr<uint8_t>(), m.ptr<uint8_t>() + n);
#ifdef CV_16UC1
        if (d.type() == CV_16UC1) {
            if (!depth_u16_) throw std::logic_error("overlayDepthFrame(CV_16UC1 depth): call setInputFormat(..., SSF_DEPTH_U16_SCALED, scale) first");
            f(d.ptr<uint16_t>(), n, mk);
            return;
        }
#endif
        if (d.type() != CV_32FC1) throw std::invalid_argument("overlayDepthFrame: the depth image must be CV_32FC1 or CV_16UC1");
        if (depth_u16_) throw std::logic_error("overlayDepthFrame: the input format is uint16 depth; pass a CV_16UC1 image");
        f(d.ptr<float>(), n, mk);
    }
#endif
private:
    /* What overlay_depth and remember_depth share.  The checks: g has its state, depth and mask are images of q's camera; the cells */
    size_t check_depth_frame(const NavGrid& g, const LiveParams& q, size_t n_depth, const std::vector<uint8_t>& mask) const {
        const size_t n = (size_t)(g.width >= 1 && g.height >= 1 ? (size_t)g.width * (size_t)g.height : 0);
        if (n == 0 || g.state.size() != n) throw std::logic_error("overlayDepthFrame: the grid has no state (want_state)");
        const size_t npix = q.width > 0 ? (size_t)q.width * (size_t)(q.height > 0 ? q.height : 0) : (size_t)width_ * (size_t)height_;
        if (n_depth != npix) throw std::invalid_argument("overlayDepthFrame: the depth image must be width x height of the camera");
        if (!mask.empty() && mask.size() != npix) throw std::invalid_argument("overlayDepthFrame: the mask must be width x height of the camera");
        return n;
    }
    /* the fields that ssf_navlive_params and ssf_navmem_params share, host arrays; cam: 12 floats of the caller's for q.cam_pose */
    template <class P> static void fill_frame_params(P& p, const NavGrid& g, const LiveParams& q, float* cam) {
        if (q.cam_pose) { transform3_to_rt(*q.cam_pose, cam); p.cam_pose = cam; }
        p.grid_pose = g.stats.pose; p.width = g.width; p.height = g.height; p.res = g.res;
        p.floor_max = q.floor_max; p.z_max = q.z_max; p.max_dist_cells = q.max_dist_cells; p.unknown_is_obstacle = q.unknown_is_obstacle ? 1 : 0;
        p.fx = q.fx; p.fy = q.fy; p.cx = q.cx; p.cy = q.cy; p.cam_width = q.width; p.cam_height = q.height; p.t_min = q.t_min; p.t_max = q.t_max;
        p.mask_mode = q.mask_mode; p.min_hits = q.min_hits; p.stride = q.stride; p.hit_margin_cells = q.hit_margin_cells;
        p.open_unknown = q.open_unknown ? 1 : 0; p.on_device = 0; p.frame_on_device = 0;
    }
    /* out as either call leaves it: g's size, the call's arrays (live_seen: the caller's), its stats as the live grid's and the grid's */
    static void fill_live_grid(LiveNavGrid& out, const NavGrid& g, std::vector<int8_t>& state, std::vector<int32_t>& dist2, std::vector<uint32_t>& hits,
                               const ssf_navlive_stats& st) {
        out.width = g.width; out.height = g.height; out.res = g.res;
        out.zmin.clear(); out.zmax.clear(); out.hits.clear();
        out.state.swap(state); out.dist2.swap(dist2); out.live_hits.swap(hits);
        out.live = st;
        ssf_navgrid_stats gs = ssf_navgrid_stats();
        gs.cells_free = st.cells_free; gs.cells_occupied = st.cells_occupied; gs.cells_unknown = st.cells_unknown;
        std::copy(st.pose, st.pose + 12, gs.pose);
        out.stats = gs;
    }
    void remember_depth(const NavGrid& g, const LiveParams& q, const void* depth, size_t n_depth, const std::vector<uint8_t>& mask, LiveMemory& mem,
                        uint32_t tick, LiveNavGrid& out) {
        const size_t n = check_depth_frame(g, q, n_depth, mask);
        if (mem.width != g.width || mem.height != g.height || mem.marks.size() != n || mem.mark_tick.size() != n || mem.seen_tick.size() != n) {
            mem.clear();
            mem.width = g.width; mem.height = g.height;
            mem.marks.assign(n, 0u); mem.mark_tick.assign(n, 0u); mem.seen_tick.assign(n, 0u);
        }
        ssf_navmem_params p;
        check(ssf_navmem_default_params(need(), &p));
        float cam[12];
        fill_frame_params(p, g, q, cam);
        p.slices = mem.slices; p.tick = tick; p.max_mark_age = mem.max_mark_age; p.max_seen_age = mem.max_seen_age;
        std::vector<int8_t> state(n);                             /* (g may be out itself) */
        std::vector<uint32_t> hits(q.want_hits ? n : 0), hit_bits(n), seen_bits(n);
        std::vector<int32_t> dist2(q.want_dist2 ? n : 0);
        ssf_navmem_layer in;
        in.marks = mem.marks.data(); in.mark_tick = mem.mark_tick.data(); in.seen_tick = mem.seen_tick.data();
        ssf_navmem_out o;
        o.marks = mem.marks.data(); o.mark_tick = mem.mark_tick.data(); o.seen_tick = mem.seen_tick.data();      /* the update in place */
        o.live_hits = q.want_hits ? hits.data() : nullptr; o.hit_bits = hit_bits.data(); o.seen_bits = seen_bits.data();
        o.state = state.data(); o.dist2 = q.want_dist2 ? dist2.data() : nullptr;
        ssf_navmem_stats st;
        check(ssf_navmem_update(need(), &p, depth, mask.empty() ? nullptr : mask.data(), g.state.data(), &in, &o, &st));
        mem.tick = tick; mem.stats = st; mem.hit_bits.swap(hit_bits); mem.seen_bits.swap(seen_bits);
        ssf_navlive_stats ls = ssf_navlive_stats();
        ls.pixels_valid = st.pixels_valid; ls.pixels_stamping = st.pixels_stamping; ls.points_in_band = st.points_in_band; ls.rays = st.rays;
        ls.rays_carving = st.rays_carving; ls.ray_samples = st.ray_samples; ls.cells_opened = st.cells_opened; ls.cells_free = st.cells_free;
        ls.cells_occupied = st.cells_occupied; ls.cells_unknown = st.cells_unknown; ls.atomics = st.atomics;
        std::copy(st.pose, st.pose + 12, ls.pose);
        fill_live_grid(out, g, state, dist2, hits, ls);
        out.live_seen.clear();
    }
    void overlay_depth(const NavGrid& g, const LiveParams& q, const void* depth, size_t n_depth, const std::vector<uint8_t>& mask, LiveNavGrid& out) {
        const size_t n = check_depth_frame(g, q, n_depth, mask);
        ssf_navlive_params p;
        check(ssf_navlive_default_params(need(), &p));
        float cam[12];
        fill_frame_params(p, g, q, cam);
        p.min_seen = q.min_seen;
        std::vector<int8_t> state(n);                             /* (g may be out itself) */
        std::vector<uint32_t> hits(q.want_hits ? n : 0), seen(q.want_seen ? n : 0);
        std::vector<int32_t> dist2(q.want_dist2 ? n : 0);
        ssf_navlive_out o;
        o.live_hits = q.want_hits ? hits.data() : nullptr; o.live_seen = q.want_seen ? seen.data() : nullptr;
        o.state = state.data(); o.dist2 = q.want_dist2 ? dist2.data() : nullptr;
        ssf_navlive_stats st;
        check(ssf_navlive_overlay(need(), &p, depth, mask.empty() ? nullptr : mask.data(), g.state.data(), &o, &st));
        fill_live_grid(out, g, state, dist2, hits, st);
        out.live_seen.swap(seen);
    }
public:
    /* Plan on a grid that buildNavGrid made (ssf_navplan.h), plain or carved: the cost-to-goal field over the cells a robot of
     * squared radius q.min_dist2 can be in, for `goals` (and, with goals_from_frontier, the grid's frontier), and for every start
     * its cost, status and path.  The grid needs its state and dist2 (want_state, want_dist2). */
    void planOnGrid(const NavGrid& g, const PlanParams& q, const std::vector<GridCell>& goals, const std::vector<GridCell>& starts, NavPlan& out) {
        const size_t n = (size_t)(g.width >= 1 && g.height >= 1 ? (size_t)g.width * (size_t)g.height : 0);
        if (n == 0 || g.state.size() != n || g.dist2.size() != n) throw std::logic_error("planOnGrid: the grid has no state or no dist2 (want_state, want_dist2)");
        ssf_navplan_params p;
        check(ssf_navplan_default_params(need(), &p));
        p.width = g.width; p.height = g.height; p.min_dist2 = q.min_dist2; p.soft_dist2 = q.soft_dist2; p.near_penalty = q.near_penalty;
        p.allow_unknown = q.allow_unknown ? 1 : 0; p.goals_from_frontier = q.goals_from_frontier ? 1 : 0; p.max_path = q.max_path; p.on_device = 0;
        p.goals = goals.empty() ? nullptr : goals[0].data(); p.n_goals = (int)goals.size();
        p.starts = starts.empty() ? nullptr : starts[0].data(); p.n_starts = (int)starts.size();
        const size_t ns = starts.size(), mp = q.max_path > 0 ? (size_t)q.max_path : 0;
        out.width = g.width; out.height = g.height;
        out.cost.resize(q.want_cost ? n : 0); out.frontier.resize(q.want_frontier ? n : 0);
        out.start_cost.assign(ns, SSF_NAVPLAN_UNREACHED); out.start_status.assign(ns, 0);
        std::vector<int32_t> len(ns, 0), cells(ns * mp * 2);
        ssf_navplan_out o;
        o.cost = q.want_cost ? out.cost.data() : nullptr; o.frontier = q.want_frontier ? out.frontier.data() : nullptr;
        o.start_cost = ns ? out.start_cost.data() : nullptr; o.start_status = ns ? out.start_status.data() : nullptr;
        o.path_len = ns ? len.data() : nullptr; o.path = cells.empty() ? nullptr : cells.data();
        check(ssf_navplan_field(need(), &p, g.state.data(), g.dist2.data(), &o, &out.stats));
        out.paths.assign(ns, std::vector<GridCell>());
        for (size_t i = 0; i < ns && mp; i++) {
            out.paths[i].resize((size_t)len[i]);
            for (size_t k = 0; k < (size_t)len[i]; k++) { out.paths[i][k][0] = cells[(i * mp + k) * 2]; out.paths[i][k][1] = cells[(i * mp + k) * 2 + 1]; }
        }
    }
    /* The poses of a nav_msgs::Path from the path of start `start`: the centre of every cell, ((ix + 0.5) res, (iy + 0.5) res, 0) in
     * the grid frame, taken to the map frame by pose12 (grid-to-map, R row-major then t: NavGrid::stats.pose); the orientation is
     * the identity.  header and the poses' headers are the node's.  Any message type with poses[i].pose works (tests use a double). */
    template <typename PathT> static void fillPath(const NavPlan& plan, size_t start, const float pose12[12], float res, PathT& msg) {
        if (start >= plan.paths.size()) throw std::logic_error("fillPath: no such start");
        const std::vector<GridCell>& cells = plan.paths[start];
        msg.poses.resize(cells.size());
        for (size_t i = 0; i < cells.size(); i++) {
            const double x = ((double)cells[i][0] + 0.5) * (double)res, y = ((double)cells[i][1] + 0.5) * (double)res;
            msg.poses[i].pose.position.x = (double)pose12[0] * x + (double)pose12[1] * y + (double)pose12[9];
            msg.poses[i].pose.position.y = (double)pose12[3] * x + (double)pose12[4] * y + (double)pose12[10];
            msg.poses[i].pose.position.z = (double)pose12[6] * x + (double)pose12[7] * y + (double)pose12[11];
            msg.poses[i].pose.orientation.x = 0.0; msg.poses[i].pose.orientation.y = 0.0; msg.poses[i].pose.orientation.z = 0.0;
            msg.poses[i].pose.orientation.w = 1.0;
        }
    }
    /* The frontier of a grid that buildNavGrid made, plain or carved, as regions (ssf_navfrontier.h).  cost: the field of a
     * planOnGrid on the same grid (NavPlan::cost), or nullptr: then no region has a representative cost.  The grid needs its state,
     * and its dist2 with traversable_only. */
    void frontierRegions(const NavGrid& g, const FrontierParams& q, const std::vector<uint32_t>* cost, FrontierRegions& out) {
        const size_t n = (size_t)(g.width >= 1 && g.height >= 1 ? (size_t)g.width * (size_t)g.height : 0);
        if (n == 0 || g.state.size() != n) throw std::logic_error("frontierRegions: the grid has no state (want_state)");
        if (q.traversable_only && g.dist2.size() != n) throw std::logic_error("frontierRegions: traversable_only needs the grid's dist2 (want_dist2)");
        if (cost && cost->size() != n) throw std::logic_error("frontierRegions: the cost field is not the grid's size");
        ssf_navfrontier_params p;
        check(ssf_navfrontier_default_params(need(), &p));
        p.width = g.width; p.height = g.height; p.connectivity = q.connectivity; p.traversable_only = q.traversable_only ? 1 : 0;
        p.min_dist2 = q.min_dist2; p.min_cells = q.min_cells; p.reachable_only = q.reachable_only ? 1 : 0; p.max_regions = q.max_regions;
        p.gain_radius = q.gain_radius; p.cost_weight = q.cost_weight; p.gain_weight = q.gain_weight; p.size_weight = q.size_weight; p.on_device = 0;
        const size_t cap = q.max_regions >= 1 && q.max_regions <= 65536 ? (size_t)q.max_regions : 1;     /* (outside: the library refuses) */
        out.width = g.width; out.height = g.height;
        out.region.resize(q.want_region ? n : 0); out.regions.resize(cap); out.order.resize(cap);
        ssf_navfrontier_out o;
        o.region = q.want_region ? out.region.data() : nullptr; o.regions = out.regions.data(); o.order = out.order.data();
        check(ssf_navfrontier_regions(need(), &p, g.state.data(), g.dist2.size() == n ? g.dist2.data() : nullptr, cost ? cost->data() : nullptr, &o,
                                      &out.stats));
        out.regions.resize((size_t)out.stats.regions_written); out.order.resize((size_t)out.stats.regions_written);
    }
    /* Where to go next, in three calls: (1) planOnGrid with the robot's cell as the only goal: the field; (2) frontierRegions with
     * that field as the cost (reachable_only is switched on); (3) planOnGrid from the robot to the representative of order[0], with
     * plan.max_path cells at most (0: width * height, capped at 1 << 20).  The field's cost is "from the cell to the robot": with a
     * clearance penalty it differs from the drive out by pen[cell] - pen[robot]; the regions are ranked by the field as it is, and
     * drive.start_cost[0] is the drive out.  Without a reached region chosen is -1 and drive is empty. */
    void exploreGoal(const NavGrid& g, const GridCell& robot, PlanParams plan, FrontierParams frontier, ExploreGoal& out) {
        const std::vector<GridCell> at(1, robot), none;
        const int max_path = plan.max_path > 0 ? plan.max_path : (int)std::min<size_t>((size_t)g.width * (size_t)g.height, (size_t)1 << 20);
        plan.goals_from_frontier = false; plan.max_path = 0; plan.want_cost = true; plan.want_frontier = false;
        NavPlan field;
        planOnGrid(g, plan, at, none, field);
        frontier.reachable_only = true;
        frontierRegions(g, frontier, &field.cost, out.frontier);
        out.chosen = -1; out.goal[0] = -1; out.goal[1] = -1; out.drive = NavPlan();
        if (out.frontier.order.empty()) return;
        const ssf_navfrontier_region& r = out.frontier.regions[(size_t)out.frontier.order[0]];
        out.chosen = out.frontier.order[0]; out.goal[0] = r.rep_x; out.goal[1] = r.rep_y;
        plan.max_path = max_path; plan.want_cost = false;
        planOnGrid(g, plan, std::vector<GridCell>(1, out.goal), at, out.drive);
    }
    /* The pose of a geometry_msgs::PoseStamped from the chosen cell: its centre, ((ix + 0.5) res, (iy + 0.5) res, 0) in the grid
     * frame, taken to the map frame by pose12 (grid-to-map: NavGrid::stats.pose); the orientation is the identity.  header is the
     * node's.  Any message type with pose.position and pose.orientation works (tests use a double). */
    template <typename PoseStampedT> static void fillExploreGoal(const ExploreGoal& e, const float pose12[12], float res, PoseStampedT& msg) {
        if (e.chosen < 0) throw std::logic_error("fillExploreGoal: no region was chosen");
        const double x = ((double)e.goal[0] + 0.5) * (double)res, y = ((double)e.goal[1] + 0.5) * (double)res;
        msg.pose.position.x = (double)pose12[0] * x + (double)pose12[1] * y + (double)pose12[9];
        msg.pose.position.y = (double)pose12[3] * x + (double)pose12[4] * y + (double)pose12[10];
        msg.pose.position.z = (double)pose12[6] * x + (double)pose12[7] * y + (double)pose12[11];
        msg.pose.orientation.x = 0.0; msg.pose.orientation.y = 0.0; msg.pose.orientation.z = 0.0; msg.pose.orientation.w = 1.0;
    }
    /* The paths of a planOnGrid on the same grid reduced to waypoints (ssf_navpath.h): consecutive waypoints are joined by a straight
     * segment whose every cell is traversable with the asked clearance.  The grid needs its state and dist2. */
    void refinePaths(const NavGrid& g, const std::vector<std::vector<GridCell> >& paths, const WaypointParams& q, NavWaypoints& out) {
        const size_t n = (size_t)(g.width >= 1 && g.height >= 1 ? (size_t)g.width * (size_t)g.height : 0);
        if (n == 0 || g.state.size() != n || g.dist2.size() != n) throw std::logic_error("refinePaths: the grid has no state or no dist2 (want_state, want_dist2)");
        if (paths.empty()) throw std::logic_error("refinePaths: no path");
        size_t mp = 1;
        for (size_t i = 0; i < paths.size(); i++) mp = std::max(mp, paths[i].size());
        const size_t np = paths.size(), mw = q.max_waypoints > 0 ? (size_t)q.max_waypoints : mp;
        ssf_navpath_params p;
        check(ssf_navpath_default_params(need(), &p));
        p.width = g.width; p.height = g.height; p.min_dist2 = q.min_dist2; p.allow_unknown = q.allow_unknown ? 1 : 0; p.los_dist2 = q.los_dist2;
        p.keep_clearance = q.keep_clearance ? 1 : 0; p.clearance_cap = q.clearance_cap; p.lookahead = q.lookahead;
        p.n_paths = (int)std::min<size_t>(np, 1u << 30); p.max_path = (int)std::min<size_t>(mp, 1u << 30);        /* (too many: the library refuses) */
        p.max_waypoints = (int)std::min<size_t>(mw, 1u << 30); p.on_device = 0;
        const bool fits = np <= 4096 && mp <= ((size_t)1 << 20) && mw <= ((size_t)1 << 20);
        std::vector<int32_t> cells(fits ? np * mp * 2 : 2), len(np), count(np, 0), wp(fits ? np * mw * 4 : 4);
        for (size_t i = 0; i < np; i++) {
            len[i] = (int32_t)paths[i].size();
            for (size_t k = 0; fits && k < paths[i].size(); k++) { cells[(i * mp + k) * 2] = paths[i][k][0]; cells[(i * mp + k) * 2 + 1] = paths[i][k][1]; }
        }
        out.status.assign(np, 0); out.path_min.assign(np, -1);
        ssf_navpath_out o;
        o.n_waypoints = count.data(); o.status = out.status.data(); o.waypoints = wp.data(); o.path_min = out.path_min.data();
        check(ssf_navpath_waypoints(need(), &p, g.state.data(), g.dist2.data(), cells.data(), len.data(), &o, &out.stats));
        out.waypoints.assign(np, std::vector<Waypoint>());
        for (size_t i = 0; i < np; i++) {
            out.waypoints[i].resize((size_t)count[i]);
            for (size_t k = 0; k < (size_t)count[i]; k++) {
                const int32_t* w = &wp[(i * mw + k) * 4];
                Waypoint& d = out.waypoints[i][k];
                d.ix = w[0]; d.iy = w[1]; d.index = w[2]; d.seg_min = w[3];
            }
        }
    }
    /* The poses of a nav_msgs::Path from the waypoints of path i, one pose per waypoint: the position as fillPath makes it (the
     * cell's centre in the grid frame, taken to the map frame by pose12 = NavGrid::stats.pose); the orientation is the grid frame's
     * rotation times the yaw about the grid's z towards the next waypoint, and the last pose repeats the one before it (a path of
     * one waypoint has yaw 0).  header and the poses' headers are the node's. */
    template <typename PathT> static void fillWaypointPath(const NavWaypoints& wp, size_t i, const float pose12[12], float res, PathT& msg) {
        if (i >= wp.waypoints.size()) throw std::logic_error("fillWaypointPath: no such path");
        const std::vector<Waypoint>& w = wp.waypoints[i];
        const double m00 = pose12[0], m01 = pose12[1], m02 = pose12[2], m10 = pose12[3], m11 = pose12[4], m12 = pose12[5], m20 = pose12[6], m21 = pose12[7],
                     m22 = pose12[8];
        const double tr = m00 + m11 + m22;
        double qw, qx, qy, qz;
        if (tr > 0.0) { const double s = 2.0 * std::sqrt(1.0 + tr); qw = 0.25 * s; qx = (m21 - m12) / s; qy = (m02 - m20) / s; qz = (m10 - m01) / s; }
        else if (m00 > m11 && m00 > m22) { const double s = 2.0 * std::sqrt(1.0 + m00 - m11 - m22); qw = (m21 - m12) / s; qx = 0.25 * s; qy = (m01 + m10) / s; qz = (m02 + m20) / s; }
        else if (m11 > m22) { const double s = 2.0 * std::sqrt(1.0 + m11 - m00 - m22); qw = (m02 - m20) / s; qx = (m01 + m10) / s; qy = 0.25 * s; qz = (m12 + m21) / s; }
        else { const double s = 2.0 * std::sqrt(1.0 + m22 - m00 - m11); qw = (m10 - m01) / s; qx = (m02 + m20) / s; qy = (m12 + m21) / s; qz = 0.25 * s; }
        msg.poses.resize(w.size());
        double yaw = 0.0;
        for (size_t k = 0; k < w.size(); k++) {
            const double x = ((double)w[k].ix + 0.5) * (double)res, y = ((double)w[k].iy + 0.5) * (double)res;
            msg.poses[k].pose.position.x = m00 * x + m01 * y + (double)pose12[9];
            msg.poses[k].pose.position.y = m10 * x + m11 * y + (double)pose12[10];
            msg.poses[k].pose.position.z = m20 * x + m21 * y + (double)pose12[11];
            if (k + 1 < w.size()) yaw = std::atan2((double)(w[k + 1].iy - w[k].iy), (double)(w[k + 1].ix - w[k].ix));
            const double sz = std::sin(0.5 * yaw), cz = std::cos(0.5 * yaw);       /* q(R) * (0, 0, sz, cz) */
            msg.poses[k].pose.orientation.w = qw * cz - qz * sz; msg.poses[k].pose.orientation.x = qx * cz + qy * sz;
            msg.poses[k].pose.orientation.y = qy * cz - qx * sz; msg.poses[k].pose.orientation.z = qz * cz + qw * sz;
        }
    }
    /* Velocity commands on a grid (ssf_navsteer.h): from every pose the lattice of q is rolled out over g, and the best admissible
     * candidate comes back with its arc.  g: a grid that buildNavGrid or overlayDepthFrame made (state and dist2); plan: a planOnGrid
     * on the same grid whose cost field is the cost-to-goal term (nullptr with q.cost_weight 0); targets: one per pose, or empty with
     * q.target_weight 0. */
    void steerOnGrid(const NavGrid& g, const NavPlan* plan, const std::vector<SteerPose>& poses, const std::vector<SteerTarget>& targets,
                     const SteerParams& q, NavSteer& out) {
        const size_t n = (size_t)(g.width >= 1 && g.height >= 1 ? (size_t)g.width * (size_t)g.height : 0);
        if (n == 0 || g.state.size() != n || g.dist2.size() != n) throw std::logic_error("steerOnGrid: the grid has no state or no dist2 (want_state, want_dist2)");
        steer_run("steerOnGrid", g, plan, poses, targets, q, out, DiscRollouts(g.state.data()));
    }
    /* The pad (sub-units, pure host arithmetic) that makes the layers conservative for any position in the cell a pose lies in and any
     * heading in the bin its heading lies in: ceil(2 * 724.1 + rho * pi / n_headings), rho the distance of the farthest corner
     * (ssf_navfoot.h step 1).  The library refuses a pad above 4096: a long body needs more headings. */
    static int footprintPad(int front, int back, int left, int right, int n_headings) {
        if (front < 0 || back < 0 || left < 0 || right < 0 || n_headings < 1) throw std::invalid_argument("footprintPad needs sides >= 0 and n_headings >= 1");
        const double a = (double)std::max(front, back), b = (double)std::max(left, right);
        return (int)std::ceil(2.0 * 724.1 + std::sqrt(a * a + b * b) * 3.14159265358979323846 / (double)n_headings);
    }
    /* The heading layers of a body on a grid (ssf_navfoot.h step 2): g: a grid that buildNavGrid or overlayDepthFrame made (state). */
    void footprintLayers(const NavGrid& g, const FootprintParams& f, FootprintLayers& out) {
        const size_t n = (size_t)(g.width >= 1 && g.height >= 1 ? (size_t)g.width * (size_t)g.height : 0);
        if (n == 0 || g.state.size() != n) throw std::logic_error("footprintLayers: the grid has no state (want_state)");
        ssf_navfoot_params p;
        check(ssf_navfoot_default_params(need(), &p));
        p.width = g.width; p.height = g.height; p.allow_unknown = f.allow_unknown ? 1 : 0; p.n_headings = f.n_headings;
        p.front = f.front; p.back = f.back; p.left = f.left; p.right = f.right;
        p.pad = f.pad >= 0 ? f.pad : footprintPad(f.front, f.back, f.left, f.right, f.n_headings);
        p.on_device = 0;
        out.width = g.width; out.height = g.height; out.n_headings = f.n_headings;
        out.free_mask.assign(n, 0u); out.n_free.assign(f.want_n_free ? n : 0, 0);
        ssf_navfoot_out o;
        o.free_mask = out.free_mask.data(); o.n_free = f.want_n_free ? out.n_free.data() : nullptr;
        check(ssf_navfoot_layers(need(), &p, g.state.data(), &o, &out.stats));
    }
    /* steerOnGrid with the oriented body in the place of the disc (ssf_navfoot.h step 3): a cell is traversable for a step iff its
     * mask holds every bin the heading sweeps in that step and dist2 >= q.min_dist2.  layers: footprintLayers of the same grid.  The
     * result feeds fillTwist and fillLocalPlan as steerOnGrid's does. */
    void steerWithFootprint(const NavGrid& g, const FootprintLayers& layers, const NavPlan* plan, const std::vector<SteerPose>& poses,
                            const std::vector<SteerTarget>& targets, const SteerParams& q, NavSteer& out) {
        const size_t n = (size_t)(g.width >= 1 && g.height >= 1 ? (size_t)g.width * (size_t)g.height : 0);
        if (n == 0 || g.dist2.size() != n) throw std::logic_error("steerWithFootprint: the grid has no dist2 (want_dist2)");
        if (layers.width != g.width || layers.height != g.height || layers.free_mask.size() != n)
            throw std::logic_error("steerWithFootprint: the layers are not the grid's size (footprintLayers of the same grid)");
        steer_run("steerWithFootprint", g, plan, poses, targets, q, out, FootRollouts(layers.free_mask.data(), layers.n_headings));
    }
    /* steerOnGrid among predicted movers (ssf_navdyn.h part A): a step is refused where it lies inside a mover's disc of that step, and
     * the score gains m.mover_weight * the lack of gap below m.mover_cap.  movers: at most 64 (MoverTracker::update makes them), one
     * list for all poses; a mover's r carries the robot's own radius. */
    void steerAmongMovers(const NavGrid& g, const NavPlan* plan, const std::vector<SteerPose>& poses, const std::vector<SteerTarget>& targets,
                          const std::vector<Mover>& movers, const SteerParams& q, const MoverParams& m, NavSteerAmongMovers& out) {
        const size_t n = (size_t)(g.width >= 1 && g.height >= 1 ? (size_t)g.width * (size_t)g.height : 0);
        if (n == 0 || g.state.size() != n || g.dist2.size() != n) throw std::logic_error("steerAmongMovers: the grid has no state or no dist2 (want_state, want_dist2)");
        MoverCall mc(movers, m, q, poses.size(), out);
        steer_run("steerAmongMovers", g, plan, poses, targets, q, out, DynDiscRollouts(g.state.data(), mc));
    }
    /* steerWithFootprint among predicted movers: a mover's r carries the body's circumscribed radius. */
    void steerFootprintAmongMovers(const NavGrid& g, const FootprintLayers& layers, const NavPlan* plan, const std::vector<SteerPose>& poses,
                                   const std::vector<SteerTarget>& targets, const std::vector<Mover>& movers, const SteerParams& q, const MoverParams& m,
                                   NavSteerAmongMovers& out) {
        const size_t n = (size_t)(g.width >= 1 && g.height >= 1 ? (size_t)g.width * (size_t)g.height : 0);
        if (n == 0 || g.dist2.size() != n) throw std::logic_error("steerFootprintAmongMovers: the grid has no dist2 (want_dist2)");
        if (layers.width != g.width || layers.height != g.height || layers.free_mask.size() != n)
            throw std::logic_error("steerFootprintAmongMovers: the layers are not the grid's size (footprintLayers of the same grid)");
        MoverCall mc(movers, m, q, poses.size(), out);
        steer_run("steerFootprintAmongMovers", g, plan, poses, targets, q, out, DynFootRollouts(layers.free_mask.data(), layers.n_headings, mc));
    }
    /* The moving pixels of a depth frame as blobs in g's frame (ssf_navdyn.h part B).  depth in the handle's input format (float metres
     * or uint16 counts), mask and label as ssf_motion_mask writes them, all of the camera's size; q: the camera, the depth range and the
     * band, as overlayDepthFrame takes them (its other members are not read). */
    void moverBlobs(const NavGrid& g, const LiveParams& q, const void* depth, const std::vector<uint8_t>& mask, const std::vector<int32_t>& label,
                    const MoverBlobParams& b, MoverBlobs& out) {
        const size_t npix = q.width > 0 ? (size_t)q.width * (size_t)(q.height > 0 ? q.height : 0) : (size_t)width_ * (size_t)height_;
        if (!depth || mask.size() != npix || label.size() != npix) throw std::invalid_argument("moverBlobs: depth, mask and label must be width x height of the camera");
        ssf_navdyn_blob_params p;
        check(ssf_navdyn_default_blob_params(need(), &p));
        float cam[12];
        if (q.cam_pose) { transform3_to_rt(*q.cam_pose, cam); p.cam_pose = cam; }
        p.grid_pose = g.stats.pose; p.width = g.width; p.height = g.height; p.res = g.res; p.floor_max = q.floor_max; p.z_max = q.z_max;
        p.fx = q.fx; p.fy = q.fy; p.cx = q.cx; p.cy = q.cy; p.cam_width = q.width; p.cam_height = q.height; p.t_min = q.t_min; p.t_max = q.t_max;
        p.min_points = b.min_points; p.max_blobs = b.max_blobs; p.on_device = 0; p.frame_on_device = 0;
        static_assert(sizeof(MoverBlob) == SSF_NAVDYN_BLOB_WORDS * sizeof(int32_t), "a blob is eight int32");
        std::vector<MoverBlob> rows((size_t)SSF_NAVDYN_MAX_BLOBS);
        check(ssf_navdyn_blobs(need(), &p, depth, mask.data(), label.data(), &rows[0].label, &out.stats));
        rows.resize((size_t)out.stats.blobs_written);
        out.blobs.swap(rows);
    }
    /* Plan over (x, y, heading) for the body of `layers` (ssf_navpose.h): g: the grid the layers were made of (dist2); goals: states,
     * bin -1 = any; starts: poses in units, as steerWithFootprint takes them. */
    void planPoses(const NavGrid& g, const FootprintLayers& layers, const PosePlanParams& q, const std::vector<PoseState>& goals,
                   const std::vector<SteerPose>& starts, PosePlan& out) {
        pose_run(g, layers, q, goals, starts, out, PoseField());
    }
    /* The poses of a nav_msgs::Path from the path of start `start`, one per state: the cell's centre in the grid frame, taken to the
     * map frame by pose12 (grid-to-map: NavGrid::stats.pose); the orientation is the grid frame's rotation times the yaw of the
     * state's bin, bin * 2 pi / n_headings, about the grid's z (fillLocalPlan's arithmetic). */
    template <typename PathT> static void fillPosePath(const PosePlan& plan, size_t start, const float pose12[12], float res, PathT& msg) {
        if (start >= plan.paths.size()) throw std::logic_error("fillPosePath: no such start");
        if (plan.n_headings < 1) throw std::logic_error("fillPosePath: the plan has no heading bins");
        NavSteer arc;
        arc.traj.resize(1);
        const std::vector<PoseState>& st = plan.paths[start];
        arc.traj[0].resize(st.size());
        for (size_t k = 0; k < st.size(); k++) {
            arc.traj[0][k].x = st[k][0] * 1024 + 512; arc.traj[0][k].y = st[k][1] * 1024 + 512; arc.traj[0][k].heading = st[k][2] * (65536 / plan.n_headings);
        }
        fillLocalPlan(arc, 0, pose12, res, msg);
    }
    /* The integer lattice of a dynamic window (pure host arithmetic, no handle): the speeds (m/s) and turn rates (rad/s) reachable
     * from (v_now, w_now) within one step of dt seconds under (accel_v m/s^2, accel_w rad/s^2), cut to [v_lo, v_hi] and [w_lo, w_hi]
     * and to the call's own |v| <= 1024, |w| <= 16384, in units per step: v = speed * dt * 1024 / res, w = rate * dt * 65536 / 2 pi.
     * The lattice starts at the window's lower end rounded up and its step is rounded down, so that no candidate lies outside the
     * window; an axis whose window is narrower than its count keeps fewer candidates.  q's six lattice members are set. */
    static void steerWindow(double v_now, double w_now, double v_lo, double v_hi, double w_lo, double w_hi, double accel_v, double accel_w, double dt,
                            float res, int n_v, int n_w, SteerParams& q) {
        if (!(dt > 0.0) || !(res > 0.f) || n_v < 1 || n_w < 1) throw std::invalid_argument("steerWindow needs dt > 0, res > 0, n_v >= 1 and n_w >= 1");
        steer_axis(v_now, v_lo, v_hi, accel_v * dt, dt * 1024.0 / (double)res, 1024, n_v, q.n_v, q.v_min, q.v_step);
        steer_axis(w_now, w_lo, w_hi, accel_w * dt, dt * 65536.0 / 6.283185307179586476925286766559, 16384, n_w, q.n_w, q.w_min, q.w_step);
    }
    /* A geometry_msgs::Twist from the command of pose `pose`: linear.x = v * res / (1024 dt), angular.z = w * 2 pi / (65536 dt), the
     * other four components 0.  A pose without a winner gives the zero twist: stop.  Any message type with linear and angular works
     * (tests use a double). */
    template <typename TwistT> static void fillTwist(const NavSteer& s, size_t pose, float res, float dt, TwistT& msg) {
        if (pose >= s.best.size()) throw std::logic_error("fillTwist: no such pose");
        if (!(dt > 0.f)) throw std::invalid_argument("fillTwist: dt must be > 0");
        msg.linear.x = (double)s.v[pose] * (double)res / (1024.0 * (double)dt); msg.linear.y = 0.0; msg.linear.z = 0.0;
        msg.angular.x = 0.0; msg.angular.y = 0.0; msg.angular.z = (double)s.w[pose] * 6.283185307179586476925286766559 / (65536.0 * (double)dt);
    }
    /* The poses of a nav_msgs::Path from the winner's arc of pose `pose`, one per entry: the position (x / 1024 res, y / 1024 res, 0)
     * in the grid frame, taken to the map frame by pose12 (grid-to-map: NavGrid::stats.pose) as fillWaypointPath does; the
     * orientation is the grid frame's rotation times the yaw heading * 2 pi / 65536 about the grid's z. */
    template <typename PathT> static void fillLocalPlan(const NavSteer& s, size_t pose, const float pose12[12], float res, PathT& msg) {
        if (pose >= s.traj.size()) throw std::logic_error("fillLocalPlan: no such pose (want_traj)");
        const std::vector<SteerPose>& t = s.traj[pose];
        const double m00 = pose12[0], m01 = pose12[1], m02 = pose12[2], m10 = pose12[3], m11 = pose12[4], m12 = pose12[5], m20 = pose12[6], m21 = pose12[7],
                     m22 = pose12[8];
        const double tr = m00 + m11 + m22;
        double qw, qx, qy, qz;
        if (tr > 0.0) { const double k = 2.0 * std::sqrt(1.0 + tr); qw = 0.25 * k; qx = (m21 - m12) / k; qy = (m02 - m20) / k; qz = (m10 - m01) / k; }
        else if (m00 > m11 && m00 > m22) { const double k = 2.0 * std::sqrt(1.0 + m00 - m11 - m22); qw = (m21 - m12) / k; qx = 0.25 * k; qy = (m01 + m10) / k; qz = (m02 + m20) / k; }
        else if (m11 > m22) { const double k = 2.0 * std::sqrt(1.0 + m11 - m00 - m22); qw = (m02 - m20) / k; qx = (m01 + m10) / k; qy = 0.25 * k; qz = (m12 + m21) / k; }
        else { const double k = 2.0 * std::sqrt(1.0 + m22 - m00 - m11); qw = (m10 - m01) / k; qx = (m02 + m20) / k; qy = (m12 + m21) / k; qz = 0.25 * k; }
        msg.poses.resize(t.size());
        for (size_t k = 0; k < t.size(); k++) {
            const double x = (double)t[k].x / 1024.0 * (double)res, y = (double)t[k].y / 1024.0 * (double)res;
            msg.poses[k].pose.position.x = m00 * x + m01 * y + (double)pose12[9];
            msg.poses[k].pose.position.y = m10 * x + m11 * y + (double)pose12[10];
            msg.poses[k].pose.position.z = m20 * x + m21 * y + (double)pose12[11];
            const double yaw = (double)t[k].heading * 6.283185307179586476925286766559 / 65536.0;
            const double sz = std::sin(0.5 * yaw), cz = std::cos(0.5 * yaw);       /* q(R) * (0, 0, sz, cz) */
            msg.poses[k].pose.orientation.w = qw * cz - qz * sz; msg.poses[k].pose.orientation.x = qx * cz + qy * sz;
            msg.poses[k].pose.orientation.y = qy * cz - qx * sz; msg.poses[k].pose.orientation.z = qz * cz + qw * sz;
        }
    }
private:
    /* the rollouts' two entry points behind one signature: a program that calls only one of the public members references only that one */
    struct DiscRollouts {
        const int8_t* state;
        explicit DiscRollouts(const int8_t* s) : state(s) {}
        int operator()(ssf_handle* h, const ssf_navsteer_params* p, const int32_t* dist2, const uint32_t* cost, const int32_t* poses, const int32_t* targets,
                       const ssf_navsteer_out* o, ssf_navsteer_stats* st) const {
            return ssf_navsteer_rollouts(h, p, state, dist2, cost, poses, targets, o, st);
        }
    };
    struct FootRollouts {
        const uint32_t* mask; int n_headings;
        FootRollouts(const uint32_t* m, int b) : mask(m), n_headings(b) {}
        int operator()(ssf_handle* h, const ssf_navsteer_params* p, const int32_t* dist2, const uint32_t* cost, const int32_t* poses, const int32_t* targets,
                       const ssf_navsteer_out* o, ssf_navsteer_stats* st) const {
            return ssf_navfoot_rollouts(h, p, n_headings, mask, dist2, cost, poses, targets, o, st);
        }
    };
    /* what the movers add to a rollouts call: the params, the list, the outputs' vectors (sized as steer_run sizes its own) */
    struct MoverCall {
        ssf_navdyn_params dp; const int32_t* movers; ssf_navdyn_out o; ssf_navdyn_stats* stats;
        MoverCall(const std::vector<Mover>& mv, const MoverParams& m, const SteerParams& q, size_t np, NavSteerAmongMovers& out) {
            static_assert(sizeof(Mover) == SSF_NAVDYN_MOVER_WORDS * sizeof(int32_t), "a mover is six int32");
            dp.n_movers = (int)std::min<size_t>(mv.size(), 1u << 30); dp.mover_cap = m.mover_cap; dp.mover_weight = m.mover_weight;
            movers = mv.empty() ? nullptr : &mv[0].x;
            size_t K, T1;
            steer_sizes(q, np, K, T1);
            const size_t nk = m.want_candidates ? np * K : 0;
            out.min_gap.assign(np, -1); out.cand_hit.assign(nk, -1); out.cand_min_gap.assign(nk, -1);
            o.cand_hit = nk ? out.cand_hit.data() : nullptr; o.cand_min_gap = nk ? out.cand_min_gap.data() : nullptr;
            o.best_min_gap = np ? out.min_gap.data() : nullptr;
            out.dyn = ssf_navdyn_stats();
            stats = &out.dyn;
        }
    };
    struct DynDiscRollouts {
        const int8_t* state; const MoverCall& mc;
        DynDiscRollouts(const int8_t* s, const MoverCall& m) : state(s), mc(m) {}
        int operator()(ssf_handle* h, const ssf_navsteer_params* p, const int32_t* dist2, const uint32_t* cost, const int32_t* poses, const int32_t* targets,
                       const ssf_navsteer_out* o, ssf_navsteer_stats* st) const {
            return ssf_navdyn_rollouts(h, p, &mc.dp, state, dist2, cost, poses, targets, mc.movers, o, &mc.o, st, mc.stats);
        }
    };
    struct DynFootRollouts {
        const uint32_t* mask; int n_headings; const MoverCall& mc;
        DynFootRollouts(const uint32_t* m, int b, const MoverCall& c) : mask(m), n_headings(b), mc(c) {}
        int operator()(ssf_handle* h, const ssf_navsteer_params* p, const int32_t* dist2, const uint32_t* cost, const int32_t* poses, const int32_t* targets,
                       const ssf_navsteer_out* o, ssf_navsteer_stats* st) const {
            return ssf_navdyn_foot_rollouts(h, p, &mc.dp, n_headings, mask, dist2, cost, poses, targets, mc.movers, o, &mc.o, st, mc.stats);
        }
    };
    /* K and n_steps + 1 of a call, 1 each where the library refuses the lattice (its arrays only have to exist) */
    static void steer_sizes(const SteerParams& q, size_t np, size_t& K, size_t& T1) {
        const bool fits = q.n_v >= 1 && q.n_v <= 256 && q.n_w >= 1 && q.n_w <= 1024 && q.n_v * q.n_w <= 65536 && q.n_steps >= 1 && q.n_steps <= 256 &&
                          np <= 4096 && np * (size_t)(q.n_v * q.n_w) <= ((size_t)1 << 24);
        K = fits ? (size_t)(q.n_v * q.n_w) : 1; T1 = fits ? (size_t)q.n_steps + 1 : 1;
    }
    /* the pose plan's entry point behind a functor of its own: only a program that calls planPoses references it */
    struct PoseField {
        int operator()(ssf_handle* h, const ssf_navpose_params* p, const uint32_t* mask, const int32_t* dist2, const ssf_navpose_out* o,
                       ssf_navpose_stats* st) const {
            return ssf_navpose_field(h, p, mask, dist2, o, st);
        }
        int defaults(const ssf_handle* h, ssf_navpose_params* p) const { return ssf_navpose_default_params(h, p); }
    };
    template <typename Call>
    void pose_run(const NavGrid& g, const FootprintLayers& layers, const PosePlanParams& q, const std::vector<PoseState>& goals,
                  const std::vector<SteerPose>& starts, PosePlan& out, const Call& call) {
        const size_t n = (size_t)(g.width >= 1 && g.height >= 1 ? (size_t)g.width * (size_t)g.height : 0);
        if (n == 0 || g.dist2.size() != n) throw std::logic_error("planPoses: the grid has no dist2 (want_dist2)");
        if (layers.width != g.width || layers.height != g.height || layers.free_mask.size() != n)
            throw std::logic_error("planPoses: the layers are not the grid's size (footprintLayers of the same grid)");
        if (!q.want_cost && !q.want_cells && starts.empty()) throw std::logic_error("planPoses: nothing asked for");
        ssf_navpose_params p;
        check(call.defaults(need(), &p));
        p.width = g.width; p.height = g.height; p.n_headings = layers.n_headings; p.min_dist2 = q.min_dist2; p.soft_dist2 = q.soft_dist2;
        p.near_penalty = q.near_penalty; p.move_tol = q.move_tol; p.allow_reverse = q.allow_reverse ? 1 : 0; p.reverse_cost = q.reverse_cost;
        p.turn_cost = q.turn_cost; p.max_path = q.max_path; p.on_device = 0;
        p.goals = goals.empty() ? nullptr : goals[0].data(); p.n_goals = (int)std::min<size_t>(goals.size(), 1u << 30);
        static_assert(sizeof(SteerPose) == 3 * sizeof(int32_t), "a pose is three int32");
        p.starts = starts.empty() ? nullptr : &starts[0].x; p.n_starts = (int)std::min<size_t>(starts.size(), 1u << 30);
        const bool bins = layers.n_headings >= 1 && layers.n_headings <= SSF_NAVFOOT_MAX_HEADINGS && n * (size_t)layers.n_headings <= (size_t)SSF_NAVPOSE_MAX_STATES;
        const size_t ns = starts.size() <= 4096 ? starts.size() : 0, mp = q.max_path > 0 && q.max_path <= (1 << 20) ? (size_t)q.max_path : 0;
        out.width = g.width; out.height = g.height; out.n_headings = layers.n_headings;
        out.cost.resize(q.want_cost && bins ? n * (size_t)layers.n_headings : 0);        /* (a size the library refuses: nothing is written) */
        out.cell_cost.resize(q.want_cells ? n : 0); out.cell_bin.resize(q.want_cells ? n : 0);
        out.start_cost.assign(ns, SSF_NAVPOSE_UNREACHED); out.start_status.assign(ns, 0);
        std::vector<int32_t> len(ns, 0), states(ns * mp * 3);
        ssf_navpose_out o;
        o.cost = out.cost.empty() ? nullptr : out.cost.data();
        o.cell_cost = q.want_cells ? out.cell_cost.data() : nullptr; o.cell_bin = q.want_cells ? out.cell_bin.data() : nullptr;
        o.start_cost = ns ? out.start_cost.data() : nullptr; o.start_status = ns ? out.start_status.data() : nullptr;
        o.path_len = ns ? len.data() : nullptr; o.path = states.empty() ? nullptr : states.data();
        check(call(need(), &p, layers.free_mask.data(), g.dist2.data(), &o, &out.stats));
        out.paths.assign(ns, std::vector<PoseState>());
        for (size_t i = 0; i < ns && mp; i++) {
            out.paths[i].resize((size_t)len[i]);
            for (size_t k = 0; k < (size_t)len[i]; k++)
                for (int c = 0; c < 3; c++) out.paths[i][k][(size_t)c] = states[(i * mp + k) * 3 + (size_t)c];
        }
    }
    /* steerOnGrid's and steerWithFootprint's body: the params, the outputs' vectors, the call, the arcs */
    template <typename Call>
    void steer_run(const char* who, const NavGrid& g, const NavPlan* plan, const std::vector<SteerPose>& poses, const std::vector<SteerTarget>& targets,
                   const SteerParams& q, NavSteer& out, const Call& call) {
        const size_t n = (size_t)g.width * (size_t)g.height;
        if (plan && plan->cost.size() != n) throw std::logic_error(std::string(who) + ": the plan's cost field is not the grid's size (want_cost)");
        if (poses.empty()) throw std::logic_error(std::string(who) + ": no pose");
        if (!targets.empty() && targets.size() != poses.size()) throw std::logic_error(std::string(who) + ": one target per pose, or none");
        ssf_navsteer_params p;
        check(ssf_navsteer_default_params(need(), &p));
        p.width = g.width; p.height = g.height; p.min_dist2 = q.min_dist2; p.allow_unknown = q.allow_unknown ? 1 : 0; p.clearance_cap = q.clearance_cap;
        p.n_poses = (int)std::min<size_t>(poses.size(), 1u << 30);          /* (too many: the library refuses) */
        p.n_v = q.n_v; p.n_w = q.n_w; p.v_min = q.v_min; p.v_step = q.v_step; p.w_min = q.w_min; p.w_step = q.w_step; p.n_steps = q.n_steps;
        p.min_free_steps = q.min_free_steps; p.brake_div = q.brake_div; p.cost_weight = q.cost_weight; p.target_weight = q.target_weight;
        p.clear_weight = q.clear_weight; p.speed_weight = q.speed_weight; p.turn_weight = q.turn_weight; p.on_device = 0;
        const size_t np = poses.size();
        size_t K, T1;
        steer_sizes(q, np, K, T1);
        std::vector<int32_t> cmd(np * 2, 0), len(np, 0), traj(q.want_traj ? np * T1 * 3 : 0);
        out.n_steps = q.n_steps; out.candidates = (int)K;
        out.best.assign(np, -1); out.n_admissible.assign(np, 0); out.status.assign(np, 0); out.score.assign(np, -1);
        const size_t nk = q.want_candidates ? np * K : 0;
        out.cand_free.assign(nk, 0); out.cand_min_d.assign(nk, -1); out.cand_end.assign(nk * 3, 0); out.cand_end_cost.assign(nk, SSF_NAVSTEER_NO_COST);
        out.cand_score.assign(nk, -1);
        ssf_navsteer_out o;
        o.best = out.best.data(); o.best_cmd = cmd.data(); o.best_score = out.score.data(); o.n_admissible = out.n_admissible.data();
        o.pose_status = out.status.data(); o.best_len = len.data(); o.best_traj = q.want_traj ? traj.data() : nullptr;
        o.cand_free = nk ? out.cand_free.data() : nullptr; o.cand_min_d = nk ? out.cand_min_d.data() : nullptr; o.cand_end = nk ? out.cand_end.data() : nullptr;
        o.cand_end_cost = nk ? out.cand_end_cost.data() : nullptr; o.cand_score = nk ? out.cand_score.data() : nullptr;
        check(call(need(), &p, g.dist2.data(), plan ? plan->cost.data() : nullptr, &poses[0].x, targets.empty() ? nullptr : &targets[0].x, &o,
                   &out.stats));
        out.v.resize(np); out.w.resize(np); out.traj.assign(np, std::vector<SteerPose>());
        for (size_t i = 0; i < np; i++) {
            out.v[i] = cmd[2 * i]; out.w[i] = cmd[2 * i + 1];
            if (!q.want_traj) continue;
            out.traj[i].resize((size_t)len[i]);
            for (size_t k = 0; k < (size_t)len[i]; k++) {
                const int32_t* e = &traj[(i * T1 + k) * 3];
                out.traj[i][k].x = e[0]; out.traj[i][k].y = e[1]; out.traj[i][k].heading = e[2];
            }
        }
    }
    static void steer_axis(double now, double lo_limit, double hi_limit, double reach, double scale, int cap, int n, int& n_out, int& first, int& step) {
        double lo = std::max(lo_limit, now - reach), hi = std::min(hi_limit, now + reach);
        if (lo > hi) lo = hi = std::min(std::max(now, lo_limit), hi_limit);      /* (the current value lies outside the limits: the nearest limit) */
        int a0 = std::max((int)std::ceil(lo * scale), -cap), a1 = std::min((int)std::floor(hi * scale), cap);
        if (a0 > a1) a0 = a1 = std::min(std::max((int)std::floor(0.5 * (lo + hi) * scale + 0.5), -cap), cap);     /* (narrower than one unit) */
        n_out = std::min(n, a1 - a0 + 1); first = a0; step = n_out > 1 ? (a1 - a0) / (n_out - 1) : 0;
    }
public:
    /* Rays cast through the map on the device (ssf_raycast.h): rays6 holds n rays of six floats (origin, direction) in the frame of
     * r.pose.  The library keeps a spatial index of the map between calls and rebuilds it when the map has changed.  INTEGRATION.md
     * section 2 has the uses (a simulated lidar scan, line of sight, picking). */
    void castRays(const float* rays6, int n, const RaycastParams& r, RaycastResult& out) {
        ssf_raycast_params p; float v[12];
        check(ssf_raycast_default_params(need(), &p));
        if (r.pose) { transform3_to_rt(*r.pose, v); p.pose = v; }
        p.t_min = r.t_min; p.t_max = r.t_max; p.min_conf = r.min_conf; p.splat_scale = r.splat_scale;
        p.visible_only = r.visible_only ? 1 : 0; p.on_device = 0; p.cell = r.cell; p.hash_bits = r.hash_bits;
        const size_t m = n > 0 ? (size_t)n : 0;
        out.t.resize(r.want_t ? m : 0); out.index.resize(r.want_index ? m : 0); out.point.resize(r.want_point ? m : 0);
        out.normal.resize(r.want_normal ? m : 0); out.color.resize(r.want_color ? m : 0);
        std::vector<float> pt(r.want_point ? 3 * m : 0), nr(r.want_normal ? 3 * m : 0), cl(r.want_color ? 3 * m : 0);
        float dummy_t = 0.f;                           /* n == 0: the library still wants one output named */
        check(ssf_raycast(need(), &p, rays6, n, m == 0 ? &dummy_t : (r.want_t ? out.t.data() : nullptr), r.want_index ? out.index.data() : nullptr,
                          r.want_point ? pt.data() : nullptr, r.want_normal ? nr.data() : nullptr, r.want_color ? cl.data() : nullptr, &out.stats));
        for (size_t i = 0; i < pt.size() / 3; i++) { out.point[i].x = pt[3 * i]; out.point[i].y = pt[3 * i + 1]; out.point[i].z = pt[3 * i + 2]; }
        for (size_t i = 0; i < nr.size() / 3; i++) { out.normal[i].x = nr[3 * i]; out.normal[i].y = nr[3 * i + 1]; out.normal[i].z = nr[3 * i + 2]; }
        for (size_t i = 0; i < cl.size() / 3; i++) { out.color[i].x = cl[3 * i]; out.color[i].y = cl[3 * i + 1]; out.color[i].z = cl[3 * i + 2]; }
    }
    void castRays(const std::vector<float>& rays6, const RaycastParams& r, RaycastResult& out) {
        if (rays6.size() % 6 != 0) throw std::invalid_argument("castRays: rays6 holds six floats per ray");
        castRays(rays6.data(), (int)(rays6.size() / 6), r, out);
    }
    /* the first hit of every ray only: t per ray, 0 on a miss */
    std::vector<float> castRays(const std::vector<float>& rays6, const RaycastParams& r = RaycastParams()) {
        RaycastParams q = r; q.want_index = q.want_point = q.want_normal = q.want_color = false; q.want_t = true;
        RaycastResult out;
        castRays(rays6, q, out);
        return out.t;
    }
    /* A planar laser scan simulated from the map: n_beams unit rays in the x-y plane of `pose` (nullptr = the tracked pose; a node
     * passes its laser frame), beam i at angle_min + i * angle_increment about z, angle_increment = (angle_max - angle_min) /
     * (n_beams - 1).  Fills the members of a sensor_msgs::LaserScan that the scan determines: angle_min, angle_max, angle_increment,
     * range_min, range_max, ranges (metres; +inf where nothing is hit within [range_min, range_max], as REP 117) and an empty
     * intensities; time_increment and scan_time are set to 0, header is the node's.  Any message type with these members works. */
    template <typename ScanT> void laserScan(const Transform3* pose, float angle_min, float angle_max, int n_beams, float range_min, float range_max,
                                             ScanT& scan, const RaycastParams& r = RaycastParams()) {
        if (n_beams < 1) throw std::invalid_argument("laserScan: n_beams < 1");
        const float inc = n_beams > 1 ? (angle_max - angle_min) / (float)(n_beams - 1) : 0.f;
        std::vector<float> rays(6 * (size_t)n_beams, 0.f);
        for (int i = 0; i < n_beams; i++) {
            const float a = angle_min + (float)i * inc;
            rays[6 * (size_t)i + 3] = std::cos(a); rays[6 * (size_t)i + 4] = std::sin(a);
        }
        RaycastParams q = r;
        q.pose = pose; q.t_min = range_min; q.t_max = range_max;
        q.want_t = true; q.want_index = q.want_point = q.want_normal = q.want_color = false;
        RaycastResult out;
        castRays(rays, q, out);
        scan.angle_min = angle_min; scan.angle_max = angle_max; scan.angle_increment = inc; scan.time_increment = 0.f; scan.scan_time = 0.f;
        scan.range_min = range_min; scan.range_max = range_max;
        scan.ranges.assign(out.t.begin(), out.t.end());
        for (size_t i = 0; i < scan.ranges.size(); i++)
            if (!(scan.ranges[i] > 0.f)) scan.ranges[i] = std::numeric_limits<float>::infinity();
        scan.intensities.clear();
    }
    /* The deformation graph of a loop closure, built and kept on the device (ssf_graph.h; exported by libssf_hip.so only): every
     * stride-th confident row in birth order is a node, every row is bound to its four nearest nodes among the 2 * look born
     * around its own birth.  Returns the number of nodes.  INTEGRATION.md section 2 has the call sequence. */
    int buildDeformationGraph(int stride = 50, int look = 20, float min_conf = 0.f) {
        ssf_graph_params p;
        check(ssf_graph_default_params(&p));
        p.stride = stride; p.look = look; p.min_conf = min_conf;
        int m = 0;
        check(ssf_graph_build(need(), &p, &m));
        return m;
    }
    /* the reference's member name: the node positions in time order, for the caller's optimiser; t_init / rows (optional) get
     * the nodes' birth stamps and model rows */
    std::vector<float3> getNodesPositions(std::vector<int32_t>* t_init = nullptr, std::vector<int32_t>* rows = nullptr) {
        int m = 0;
        check(ssf_graph_info(need(), &m, nullptr, nullptr));
        std::vector<float3> pos((size_t)m);
        if (t_init) t_init->resize((size_t)m);
        if (rows) rows->resize((size_t)m);
        if (m > 0)
            check(ssf_graph_get_nodes(need(), reinterpret_cast<float*>(pos.data()), t_init ? t_init->data() : nullptr,
                                      rows ? rows->data() : nullptr, m));
        return pos;
    }
    GraphBinding getGraphBinding() {
        int n = 0;
        check(ssf_graph_info(need(), nullptr, &n, nullptr));
        GraphBinding b;
        b.weights4.resize(4 * (size_t)n); b.idx4.resize(4 * (size_t)n);
        check(ssf_graph_get_binding(need(), b.weights4.data(), b.idx4.data(), 0));
        return b;
    }
    /* the same rule for a loop closure's constraint points (their birth stamps in t_init) */
    GraphBinding bindPoints(const std::vector<float3>& points, const std::vector<int32_t>& t_init) {
        if (points.size() != t_init.size()) throw std::runtime_error("bindPoints: one birth stamp per point");
        GraphBinding b;
        b.weights4.resize(4 * points.size()); b.idx4.resize(4 * points.size());
        check(ssf_graph_bind_points(need(), reinterpret_cast<const float*>(points.data()), t_init.data(), (int)points.size(),
                                    b.weights4.data(), b.idx4.data()));
        return b;
    }
    /* deform the model with the optimised node transforms (one Mat33 and one translation per node, in node order) */
    void applyGraph(const std::vector<Mat33>& rotations, const std::vector<float3>& translations) {
        int m = 0;
        check(ssf_graph_info(need(), &m, nullptr, nullptr));
        if (rotations.size() != (size_t)m || translations.size() != (size_t)m)
            throw std::runtime_error("applyGraph: one rotation and one translation per node");
        check(ssf_graph_apply(need(), reinterpret_cast<const float*>(rotations.data()), reinterpret_cast<const float*>(translations.data())));
    }
    /* The graph's optimisation on the device (ssf_graph_solve.h; exported by libssf_hip.so only): node transforms that take the
     * constraint points src (birth stamps in t_init) to dst, a pin being dst == src.  The names follow the reference's
     * DeformationGraph (optimiseGraphSparse, applyGraphToModel) where it has the step.  The transforms stay on the device. */
    static ssf_graph_solve_params defaultGraphSolveParams() { ssf_graph_solve_params p; ssf_graph_solve_default_params(&p); return p; }
    ssf_graph_solve_result optimiseGraphSparse(const std::vector<float3>& src, const std::vector<int32_t>& t_init,
                                               const std::vector<float3>& dst,
                                               const ssf_graph_solve_params& p = defaultGraphSolveParams()) {
        if (src.size() != t_init.size() || src.size() != dst.size())
            throw std::runtime_error("optimiseGraphSparse: one birth stamp and one target per source point");
        ssf_graph_solve_result r;
        check(ssf_graph_solve(need(), &p, reinterpret_cast<const float*>(src.data()), t_init.data(),
                              reinterpret_cast<const float*>(dst.data()), (int)src.size(), &r));
        return r;
    }
    /* the four neighbours of every node, 4 per node in node order */
    std::vector<int32_t> getGraphEdges() {
        int m = 0;
        check(ssf_graph_info(need(), &m, nullptr, nullptr));
        std::vector<int32_t> e(4 * (size_t)m);
        check(ssf_graph_get_edges(need(), e.data(), m));
        return e;
    }
    /* the solved transforms, as applyGraph takes them */
    void getGraphTransforms(std::vector<Mat33>& rotations, std::vector<float3>& translations) {
        int m = 0;
        check(ssf_graph_info(need(), &m, nullptr, nullptr));
        rotations.resize((size_t)m); translations.resize((size_t)m);
        check(ssf_graph_get_transforms(need(), reinterpret_cast<float*>(rotations.data()), reinterpret_cast<float*>(translations.data()), m));
    }
    /* deform the model with the resident solved transforms (nothing is uploaded); the graph is stale afterwards */
    void applyGraphToModel() { check(ssf_graph_apply_solved(need())); }
    /* The keyframe database of loop detection, kept on the device (ssf_keyframes.h; exported by libssf_hip.so only):
     * configureKeyframes once, considerKeyframe after every frame, alignKeyframe for a loop candidate of its record.
     * INTEGRATION.md section 2 has the call sequence. */
    static ssf_keyframes_params defaultKeyframesParams() { ssf_keyframes_params p; ssf_keyframes_default_params(&p); return p; }
    void configureKeyframes(const ssf_keyframes_params& p) { check(ssf_keyframes_configure(need(), &p)); }
    void configureKeyframes() { configureKeyframes(defaultKeyframesParams()); }
    void clearKeyframes() { check(ssf_keyframes_clear(need())); }
    int nbKeyframes() { int n = 0; check(ssf_keyframes_info(need(), nullptr, &n, nullptr, nullptr)); return n; }
    void setFerns(const std::vector<ssf_fern>& ferns) { check(ssf_keyframes_set_ferns(need(), ferns.data(), (int)ferns.size())); }
    std::vector<ssf_fern> getFerns() {
        std::vector<ssf_fern> f((size_t)keyframeFerns());
        check(ssf_keyframes_get_ferns(need(), f.data(), (int)f.size()));
        return f;
    }
    /* the current frame's codes, one byte per fern */
    std::vector<uint8_t> encodeKeyframe() {
        std::vector<uint8_t> c((size_t)keyframeFerns());
        check(ssf_keyframes_encode(need(), c.data(), (int)c.size()));
        return c;
    }
    /* encode the current frame, search, add it when the view is new: the per-frame call */
    ssf_keyframe_result considerKeyframe() { ssf_keyframe_result r; check(ssf_keyframes_consider(need(), &r)); return r; }
    /* search only: the current frame's codes ... */
    ssf_keyframe_result queryKeyframes(int min_gap = -1, int k = SSF_KEYFRAMES_MAX_CANDIDATES) {
        ssf_keyframe_result r; check(ssf_keyframes_query(need(), nullptr, 0, min_gap, k, &r)); return r;
    }
    /* ... or the caller's, with the caller's stamp */
    ssf_keyframe_result queryKeyframes(const std::vector<uint8_t>& codes, int stamp, int min_gap = -1, int k = SSF_KEYFRAMES_MAX_CANDIDATES) {
        if (codes.size() != (size_t)keyframeFerns()) throw std::runtime_error("queryKeyframes: one code per fern");
        ssf_keyframe_result r; check(ssf_keyframes_query(need(), codes.data(), stamp, min_gap, k, &r)); return r;
    }
    int addKeyframe() { int id = -1; check(ssf_keyframes_add(need(), &id)); return id; }
    int putKeyframe(Keyframe& kf) {
        if (kf.codes.size() != (size_t)keyframeFerns()) throw std::runtime_error("putKeyframe: one code per fern");
        ssf_surfels v = kf.rows.view(); int id = -1;
        check(ssf_keyframes_put(need(), kf.codes.data(), &v, kf.rows.size, kf.pose, kf.stamp, &id));
        return id;
    }
    Keyframe getKeyframe(int id) {
        Keyframe kf; int n = 0;
        check(ssf_keyframes_get(need(), id, nullptr, 0, &n, nullptr, nullptr, nullptr));
        kf.rows.resize(n); kf.codes.resize((size_t)keyframeFerns());
        ssf_surfels v = kf.rows.view();
        check(ssf_keyframes_get(need(), id, &v, n, &n, kf.pose, &kf.stamp, kf.codes.data()));
        return kf;
    }
    void setKeyframePose(int id, const float* pose12) { check(ssf_keyframes_set_pose(need(), id, pose12)); }
    /* register stored keyframe id against the current frame (ssf_align's outputs); init_pose12 may be null */
    KeyframeAlignment alignKeyframe(int id, const float* init_pose12 = nullptr, bool use_conf = false) {
        KeyframeAlignment a; int valid = 0;
        check(ssf_keyframes_align(need(), id, init_pose12, use_conf ? 1 : 0, a.rel_pose, &valid, &a.iters, &a.pairs));
        a.valid = valid != 0;
        return a;
    }
    /* the same two images without OpenCV */
    std::vector<uint8_t> getSuperpixelSegIm() {
        std::vector<uint8_t> v((size_t)3 * width_ * height_);
        check(ssf_get_preview_image(need(), v.data()));
        return v;
    }
    std::vector<float> getSlantedPlaneIm() {
        std::vector<float> v((size_t)width_ * height_);
        check(ssf_get_plane_depth(need(), v.data()));
        return v;
    }
    int keyframeFerns() { ssf_keyframes_params p; check(ssf_keyframes_info(need(), nullptr, nullptr, nullptr, &p)); return p.n_ferns; }
    /* getPose(): supersurfel_fusion.hpp:89 -- `const Transform3&`, camera-to-map, valid until the next call on this
     * object (the reference returns a reference to its member; so does this, refreshed from the library) */
    const Transform3& getPose() const {
        float v[12];
        check(ssf_get_pose(need(), v));
        pose_ = transform3_from_rt(v);
        return pose_;
    }
    void setPose(const Transform3& p) {
        float v[12];
        transform3_to_rt(p, v);
        check(ssf_set_pose(need(), v));
    }
    int getnbSupersurfels() const { int n = 0; check(ssf_get_counts(need(), &n, nullptr, nullptr, nullptr)); return n; }
    int getnbVisible() const { int n = 0; check(ssf_get_counts(need(), nullptr, &n, nullptr, nullptr)); return n; }
    int getStamp() const { int s = 0; check(ssf_get_counts(need(), nullptr, nullptr, &s, nullptr)); return s; }
    int getnbSuperpixels() const { int s = 0; check(ssf_get_counts(need(), nullptr, nullptr, nullptr, &s)); return s; }
    /* getModel() / getFrame(): the reference returns device-resident thrust vectors and the node copies
     * [0, nbSupersurfels) to the host (supersurfel_fusion_node.cpp:306-310); here the copy comes back directly */
    HostSupersurfels getModelHost() {
        HostSupersurfels m; m.resize(getnbSupersurfels());
        ssf_surfels v = m.view();
        check(ssf_get_model(need(), 0, m.size, &v));
        return m;
    }
    HostSupersurfels getFrameHost() {
        HostSupersurfels m; m.resize(getnbSuperpixels());
        ssf_surfels v = m.view();
        check(ssf_get_frame(need(), &v));
        return m;
    }
#ifdef SSF_THRUST_VIEW
    /* supersurfel_fusion.hpp:86-87: `const Supersurfels&`, device-resident (views: see Supersurfels above) */
    const Supersurfels& getModel() {
        ssf_surfels v; int n = 0;
        check(ssf_get_model_device(need(), &v, &n));
        model_view_.bind(v, (size_t)n);
        return model_view_;
    }
    const Supersurfels& getFrame() {
        ssf_surfels v; int n = 0;
        check(ssf_get_frame_device(need(), &v, &n));
        frame_view_.bind(v, (size_t)n);
        return frame_view_;
    }
#else
    HostSupersurfels getModel() { return getModelHost(); }
    HostSupersurfels getFrame() { return getFrameHost(); }
#endif
    /* the device views under a name of their own, in both forms (data() / size() only without thrust) */
    const Supersurfels& getModelView() {
        ssf_surfels v; int n = 0;
        check(ssf_get_model_device(need(), &v, &n));
        model_view_.bind(v, (size_t)n);
        return model_view_;
    }
    const Supersurfels& getFrameView() {
        ssf_surfels v; int n = 0;
        check(ssf_get_frame_device(need(), &v, &n));
        frame_view_.bind(v, (size_t)n);
        return frame_view_;
    }
    /* getModel() as the reference returns it: device-resident arrays in the reference's layout (orientations =
     * packed Mat33), n rows, valid until the next call (supersurfel_fusion.hpp:87; the node copies
     * [0, nbSupersurfels) out array by array, supersurfel_fusion_node.cpp:306-310) */
    ssf_surfels getModelDevice(int* n = nullptr) { ssf_surfels v; check(ssf_get_model_device(need(), &v, n)); return v; }
    void exportModel(const std::string& file) { check(ssf_export_model_txt(need(), file.c_str())); }   /* supersurfel_fusion.cu:595-633 */
    /* TPS_RGBD::getIndexImage (TPS_RGBD.hpp:77): the label of every pixel */
    std::vector<int32_t> getIndexImage() {
        std::vector<int32_t> v((size_t)width_ * height_);
        check(ssf_get_index_map(need(), v.data()));
        return v;
    }
    const ssf_frame_result& lastResult() const { return last_; }
    ssf_handle* handle() { return h_; }

private:
    void query_params(const QueryParams& q, ssf_query_params& p, float v[12]) const {
        check(ssf_query_default_params(need(), &p));
        p.min_conf = q.min_conf; p.t_init_min = q.t_init_min; p.t_init_max = q.t_init_max; p.t_last_min = q.t_last_min; p.t_last_max = q.t_last_max;
        p.visible_only = q.visible_only ? 1 : 0; p.region = q.region;
        if (q.pose) { transform3_to_rt(*q.pose, v); p.pose = v; }
        p.radius = q.radius; p.half[0] = q.half[0]; p.half[1] = q.half[1]; p.half[2] = q.half[2];
        p.width = q.width; p.height = q.height; p.fx = q.fx; p.fy = q.fy; p.cx = q.cx; p.cy = q.cy; p.z_min = q.z_min; p.z_max = q.z_max;
        p.on_device = 0;
    }
    ssf_handle* need() const { if (!h_) throw std::logic_error("SupersurfelFusion: initialize() first"); return h_; }
    ssf_motion_params motion_params(const MotionParams& mp) {
        ssf_motion_params p;
        check(ssf_motion_default_params(need(), &p));
        p.pose = mp.pose; p.min_conf = mp.min_conf; p.splat_scale = mp.splat_scale;
        p.front_abs = mp.front_abs; p.front_quad = mp.front_quad; p.link_abs = mp.link_abs; p.link_rel = mp.link_rel;
        if (mp.min_seeds != 0) p.min_seeds = mp.min_seeds;
        p.unknown_per_seed = mp.unknown_per_seed; p.on_device = 0;
        return p;
    }
    ssf_odometry_params odometry_params(const OdometryParams& op) {
        ssf_odometry_params p;
        check(ssf_odometry_default_params(need(), &p));
        p.levels = op.levels;
        for (int l = 0; l < SSF_ODO_MAX_LEVELS; l++) p.iters[l] = op.iters[l];
        p.r_max = op.r_max; p.huber = op.huber; p.min_pixel_share = op.min_pixel_share; p.tol_rot = op.tol_rot; p.tol_trans = op.tol_trans;
        p.max_translation = op.max_translation; p.max_rotation = op.max_rotation;
        return p;
    }
    OdometryEstimate estimate_odometry(const uint8_t* rgb, const void* depth, const OdometryParams& op, const float* init) {
        const ssf_odometry_params p = odometry_params(op);
        OdometryEstimate e;
        check(ssf_odometry_estimate(need(), &p, rgb, depth, 0, init, e.rel, &e.result));
        return e;
    }
    OdometryEstimate track_odometry(const uint8_t* rgb, const void* depth, const OdometryParams& op) {
        const ssf_odometry_params p = odometry_params(op);
        OdometryEstimate e;
        check(ssf_odometry_track(need(), &p, rgb, depth, 0, e.prior, &e.result));
        e.has_prior = e.result.valid != 0;
        check(ssf_get_odometry(need(), e.rel, nullptr, nullptr));
        return e;
    }
    MotionMask detect_motion(const void* depth, const MotionParams& mp) {
        const ssf_motion_params p = motion_params(mp);
        MotionMask m;
        m.width = width_; m.height = height_; m.mask.resize((size_t)width_ * (size_t)height_);
        check(ssf_motion_mask(need(), &p, depth, m.mask.data(), nullptr, nullptr, nullptr, &m.stats));
        return m;
    }
    void check(int rc) const { if (rc != SSF_OK) throw std::runtime_error(std::string(ssf_last_error(h_))); }
    ssf_handle* h_ = nullptr;
    ssf_frame_result last_{};
    mutable Transform3 pose_{};
    Supersurfels model_view_, frame_view_;        /* always there (layout does not depend on the include order); bound by the thrust form's getModel() / getFrame() and by getModelView() / getFrameView() */
    int width_ = 0, height_ = 0;
    int pipeline_depth_ = 0, extract_batch_ = 1; bool depth_prefilter_ = true;
    bool depth_u16_ = false;                       /* setInputFormat: depth arrives as uint16 counts */
};

}  /* inline namespace thrust_view / host_copy */
}  /* namespace supersurfel_fusion */
#endif
