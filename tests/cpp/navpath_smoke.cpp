// The waypoints of include/ssf.hpp (WaypointParams, refinePaths, NavWaypoints, fillWaypointPath).  The grid is navplan_smoke.cpp's
// (70 x 45 from integer hashes of the cell number), so that tests/test_navpath_gpu.py plans and refines on the same arrays through
// the Python calls.  Prints the counts and the FNV-1a checksum of the waypoints, and fills the Path double from the first path that
// has more than one waypoint.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include "ssf.hpp"
#include "nav_msgs_path_double.hpp"

static uint64_t fnv1a(const void* p, size_t n, uint64_t h = 1469598103934665603ull) {
    const unsigned char* b = static_cast<const unsigned char*>(p);
    for (size_t i = 0; i < n; i++) { h ^= b[i]; h *= 1099511628211ull; }
    return h;
}

int main() {
    using namespace supersurfel_fusion;
    CamParam cam; cam.width = 160; cam.height = 128; cam.fx = 150.f; cam.fy = 150.f; cam.cx = 79.5f; cam.cy = 63.5f;
    try {
        SupersurfelFusion a;
        a.setDepthPrefilter(false);
        a.initialize(cam, 16, 10.f, 1000.f, 1000.f, 1e8f);
        NavGrid g;
        g.width = 70; g.height = 45; g.res = 0.25f;
        const size_t P = (size_t)g.width * g.height;
        g.state.resize(P); g.dist2.resize(P);
        for (size_t p = 0; p < P; p++) {
            const uint32_t u = ((uint32_t)p * 2654435761u) >> 16, v = ((uint32_t)p * 40503u + 977u) >> 5;
            g.state[p] = (int8_t)(u % 100u < 20u ? 100 : (u % 100u < 32u ? -1 : 0));
            g.dist2[p] = (int32_t)(v % 37u);
        }
        const float rt[12] = {0.f, 1.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, -1.f, -1.5f, 2.f, 0.25f};
        std::memcpy(g.stats.pose, rt, sizeof(rt));
        PlanParams q;
        q.min_dist2 = 1; q.allow_unknown = true; q.max_path = 200; q.want_cost = false; q.want_frontier = false;
        std::vector<GridCell> goals, starts;
        const int gl[4][2] = {{3, 3}, {66, 40}, {70, 2}, {35, 22}}, sl[5][2] = {{0, 0}, {69, 44}, {20, 30}, {-1, 4}, {50, 10}};
        for (int i = 0; i < 4; i++) { GridCell c; c[0] = gl[i][0]; c[1] = gl[i][1]; goals.push_back(c); }
        for (int i = 0; i < 5; i++) { GridCell c; c[0] = sl[i][0]; c[1] = sl[i][1]; starts.push_back(c); }
        NavPlan plan;
        a.planOnGrid(g, q, goals, starts, plan);
        WaypointParams w;
        w.min_dist2 = 1; w.allow_unknown = true; w.keep_clearance = true; w.clearance_cap = 9; w.lookahead = 40;
        NavWaypoints wp;
        a.refinePaths(g, plan.paths, w, wp);
        const ssf_navpath_stats& s = wp.stats;
        uint64_t h = 1469598103934665603ull;
        for (size_t i = 0; i < wp.waypoints.size(); i++)
            if (!wp.waypoints[i].empty()) h = fnv1a(&wp.waypoints[i][0], sizeof(Waypoint) * wp.waypoints[i].size(), h);
        std::printf("navpath ok=%lld bad=%lld truncated=%lld waypoints=%lld forced=%lld cells=%lld status=%016llx min=%016llx points=%016llx\n",
                    (long long)s.paths_ok, (long long)s.paths_bad, (long long)s.paths_truncated, (long long)s.waypoints, (long long)s.forced_steps,
                    (long long)s.cells_in, (unsigned long long)fnv1a(wp.status.data(), 4 * wp.status.size()),
                    (unsigned long long)fnv1a(wp.path_min.data(), 4 * wp.path_min.size()), (unsigned long long)h);
        if (wp.waypoints.size() != 5u || wp.status.size() != 5u || sizeof(Waypoint) != 16u) { std::printf("sizes\n"); return 2; }
        size_t first = 0;
        while (first < wp.waypoints.size() && wp.waypoints[first].size() < 2u) first++;
        if (first == wp.waypoints.size()) { std::printf("no path of two waypoints\n"); return 2; }
        const std::vector<Waypoint>& v = wp.waypoints[first];
        // positions through the grid frame as fillPath makes them
        nav_msgs::Path msg;
        SupersurfelFusion::fillWaypointPath(wp, first, g.stats.pose, g.res, msg);
        const double x = (v[0].ix + 0.5) * 0.25, y = (v[0].iy + 0.5) * 0.25;
        bool ok = msg.poses.size() == v.size() && msg.poses[0].pose.position.x == y - 1.5 && msg.poses[0].pose.position.y == x + 2.0 &&
                  msg.poses[0].pose.position.z == 0.25;
        // the yaw towards the next waypoint, in a grid frame that is the map frame; the last pose repeats the one before it
        const float id[12] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f};
        nav_msgs::Path flat;
        SupersurfelFusion::fillWaypointPath(wp, first, id, g.res, flat);
        const size_t n = v.size();
        for (size_t k = 0; k + 1 < n; k++) {
            const double yaw = std::atan2((double)(v[k + 1].iy - v[k].iy), (double)(v[k + 1].ix - v[k].ix));
            ok = ok && std::fabs(flat.poses[k].pose.orientation.z - std::sin(0.5 * yaw)) < 1e-12 &&
                 std::fabs(flat.poses[k].pose.orientation.w - std::cos(0.5 * yaw)) < 1e-12 && flat.poses[k].pose.orientation.x == 0.0 &&
                 flat.poses[k].pose.orientation.y == 0.0;
        }
        ok = ok && flat.poses[n - 1].pose.orientation.z == flat.poses[n - 2].pose.orientation.z &&
             flat.poses[n - 1].pose.orientation.w == flat.poses[n - 2].pose.orientation.w;
        // every orientation is a unit quaternion
        for (size_t k = 0; k < n; k++) {
            const double qx = msg.poses[k].pose.orientation.x, qy = msg.poses[k].pose.orientation.y, qz = msg.poses[k].pose.orientation.z,
                         qw = msg.poses[k].pose.orientation.w;
            ok = ok && std::fabs(qx * qx + qy * qy + qz * qz + qw * qw - 1.0) < 1e-12;
        }
        std::printf("path start=%d poses=%d ok=%d\n", (int)first, (int)msg.poses.size(), ok ? 1 : 0);
        if (!ok) return 2;
        // a grid without dist2 is refused before the library is asked
        NavGrid bare; bare.width = 4; bare.height = 4; bare.state.assign(16, 0);
        bool threw = false;
        try { a.refinePaths(bare, plan.paths, w, wp); } catch (const std::logic_error&) { threw = true; }
        if (!threw) { std::printf("no refusal\n"); return 2; }
    } catch (const std::exception& e) { std::printf("exception %s\n", e.what()); return 1; }
    return 0;
}
