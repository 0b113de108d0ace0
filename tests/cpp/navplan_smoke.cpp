// The plan on the navigation grid of include/ssf.hpp (PlanParams, planOnGrid, NavPlan, fillPath).  The grid is written here cell by
// cell from a formula (70 x 45: obstacles, unknown cells and clearances from integer hashes of the cell number), so that
// tests/test_navplan_gpu.py plans on the same arrays through the Python call.  Prints the plan's counts and the FNV-1a checksums of
// the cost field, the frontier and the paths' cells, and fills the Path double from the first path.
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
        q.min_dist2 = 2; q.soft_dist2 = 30; q.near_penalty = 25; q.goals_from_frontier = true; q.max_path = 64;
        std::vector<GridCell> goals, starts;
        const int gl[4][2] = {{3, 3}, {66, 40}, {70, 2}, {35, 22}}, sl[5][2] = {{0, 0}, {69, 44}, {20, 30}, {-1, 4}, {50, 10}};
        for (int i = 0; i < 4; i++) { GridCell c; c[0] = gl[i][0]; c[1] = gl[i][1]; goals.push_back(c); }
        for (int i = 0; i < 5; i++) { GridCell c; c[0] = sl[i][0]; c[1] = sl[i][1]; starts.push_back(c); }
        NavPlan plan;
        a.planOnGrid(g, q, goals, starts, plan);
        const ssf_navplan_stats& s = plan.stats;
        uint64_t hp = 1469598103934665603ull;
        long long cells = 0;
        for (size_t i = 0; i < plan.paths.size(); i++) {
            if (!plan.paths[i].empty()) hp = fnv1a(plan.paths[i][0].data(), 8 * plan.paths[i].size(), hp);
            cells += (long long)plan.paths[i].size();
        }
        std::printf("navplan %dx%d trav=%lld reached=%lld frontier=%lld fgoals=%lld used=%lld blocked=%lld outside=%lld max=%lld cells=%lld "
                    "cost=%016llx frontier=%016llx status=%016llx paths=%016llx\n",
                    plan.width, plan.height, (long long)s.cells_traversable, (long long)s.cells_reached, (long long)s.frontier_cells,
                    (long long)s.frontier_goals, (long long)s.goals_used, (long long)s.goals_blocked, (long long)s.goals_outside, (long long)s.max_cost,
                    cells, (unsigned long long)fnv1a(plan.cost.data(), 4 * plan.cost.size()),
                    (unsigned long long)fnv1a(plan.frontier.data(), plan.frontier.size()),
                    (unsigned long long)fnv1a(plan.start_status.data(), 4 * plan.start_status.size()), (unsigned long long)hp);
        if (plan.cost.size() != P || plan.paths.size() != 5u || plan.start_status[3] != 1) { std::printf("sizes\n"); return 2; }
        // the first start's path as a nav_msgs/Path: cell centres through the grid frame
        size_t first = 0;
        while (first < plan.paths.size() && plan.paths[first].empty()) first++;
        if (first == plan.paths.size()) { std::printf("no path\n"); return 2; }
        nav_msgs::Path msg;
        SupersurfelFusion::fillPath(plan, first, g.stats.pose, g.res, msg);
        const GridCell c0 = plan.paths[first][0];
        const double x = (c0[0] + 0.5) * 0.25, y = (c0[1] + 0.5) * 0.25;
        const bool ok = msg.poses.size() == plan.paths[first].size() && msg.poses[0].pose.position.x == y - 1.5 && msg.poses[0].pose.position.y == x + 2.0 &&
                        msg.poses[0].pose.position.z == 0.25 && msg.poses[0].pose.orientation.w == 1.0;
        std::printf("path start=%d poses=%d ok=%d\n", (int)first, (int)msg.poses.size(), ok ? 1 : 0);
        if (!ok) return 2;
        // a grid without dist2 is refused before the library is asked
        NavGrid bare; bare.width = 4; bare.height = 4; bare.state.assign(16, 0);
        bool threw = false;
        try { a.planOnGrid(bare, q, goals, starts, plan); } catch (const std::logic_error&) { threw = true; }
        if (!threw) { std::printf("no refusal\n"); return 2; }
    } catch (const std::exception& e) { std::printf("exception %s\n", e.what()); return 1; }
    return 0;
}
