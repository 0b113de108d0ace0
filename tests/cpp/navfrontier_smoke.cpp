// The frontier regions of include/ssf.hpp (FrontierParams, frontierRegions, exploreGoal, fillExploreGoal).  The grid is the one of
// navplan_smoke.cpp, written cell by cell from a formula (70 x 45), so that tests/test_navfrontier_gpu.py makes the same calls through
// Python.  Prints the regions' counts and the FNV-1a checksums of the map, the table and the order, then the chosen region with
// its path, and fills the PoseStamped double from it.
#include <cstdio>
#include <cstring>
#include <vector>
#include "ssf.hpp"
#include "geometry_msgs_pose_stamped_double.hpp"

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
        // the regions on their own: no cost field, every figure but the representative's cost
        FrontierParams f;
        f.min_cells = 2; f.gain_radius = 5; f.max_regions = 64;
        FrontierRegions fr;
        a.frontierRegions(g, f, nullptr, fr);
        const ssf_navfrontier_stats& s = fr.stats;
        std::printf("navfrontier %dx%d cells=%lld found=%lld small=%lld unreached=%lld kept=%lld written=%lld largest=%lld rays=%lld "
                    "region=%016llx table=%016llx order=%016llx\n",
                    fr.width, fr.height, (long long)s.frontier_cells, (long long)s.regions_found, (long long)s.regions_small,
                    (long long)s.regions_unreached, (long long)s.regions_kept, (long long)s.regions_written, (long long)s.largest_cells,
                    (long long)s.gain_rays, (unsigned long long)fnv1a(fr.region.data(), 4 * fr.region.size()),
                    (unsigned long long)fnv1a(fr.regions.data(), sizeof(ssf_navfrontier_region) * fr.regions.size()),
                    (unsigned long long)fnv1a(fr.order.data(), 4 * fr.order.size()));
        if (fr.region.size() != P || fr.regions.size() != (size_t)s.regions_written || fr.order.size() != fr.regions.size()) { std::printf("sizes\n"); return 2; }
        // where to go next from a free cell
        GridCell robot; robot[0] = 20; robot[1] = 30;
        while (g.state[(size_t)robot[1] * g.width + robot[0]] != 0) robot[0]++;
        PlanParams q;
        q.soft_dist2 = 30; q.near_penalty = 25;
        ExploreGoal e;
        a.exploreGoal(g, robot, q, f, e);
        if (e.chosen < 0 || e.drive.paths.size() != 1u || e.drive.paths[0].empty()) { std::printf("no goal\n"); return 2; }
        const ssf_navfrontier_region& r = e.frontier.regions[(size_t)e.chosen];
        std::printf("explore robot=%d,%d chosen=%d label=%d goal=%d,%d rep_cost=%u drive=%u status=%d cells=%d table=%016llx path=%016llx\n", robot[0], robot[1],
                    e.chosen, r.label, e.goal[0], e.goal[1], r.rep_cost, e.drive.start_cost[0], e.drive.start_status[0], (int)e.drive.paths[0].size(),
                    (unsigned long long)fnv1a(e.frontier.regions.data(), sizeof(ssf_navfrontier_region) * e.frontier.regions.size()),
                    (unsigned long long)fnv1a(e.drive.paths[0][0].data(), 8 * e.drive.paths[0].size()));
        const GridCell last = e.drive.paths[0].back();
        if (last[0] != e.goal[0] || last[1] != e.goal[1] || e.goal[0] != r.rep_x || e.goal[1] != r.rep_y) { std::printf("the path does not end at the goal\n"); return 2; }
        // the goal as a geometry_msgs/PoseStamped: the cell's centre through the grid frame
        geometry_msgs::PoseStamped msg;
        SupersurfelFusion::fillExploreGoal(e, g.stats.pose, g.res, msg);
        const double x = (e.goal[0] + 0.5) * 0.25, y = (e.goal[1] + 0.5) * 0.25;
        const bool ok = msg.pose.position.x == y - 1.5 && msg.pose.position.y == x + 2.0 && msg.pose.position.z == 0.25 && msg.pose.orientation.w == 1.0;
        std::printf("goal ok=%d\n", ok ? 1 : 0);
        if (!ok) return 2;
        // a grid without state is refused before the library is asked, and so is a goal that was not chosen
        NavGrid bare; bare.width = 4; bare.height = 4;
        int threw = 0;
        try { a.frontierRegions(bare, f, nullptr, fr); } catch (const std::logic_error&) { threw++; }
        try { SupersurfelFusion::fillExploreGoal(ExploreGoal(), g.stats.pose, g.res, msg); } catch (const std::logic_error&) { threw++; }
        if (threw != 2) { std::printf("no refusal\n"); return 2; }
    } catch (const std::exception& e) { std::printf("exception %s\n", e.what()); return 1; }
    return 0;
}
