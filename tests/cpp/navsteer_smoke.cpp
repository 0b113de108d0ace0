// The velocity commands of include/ssf.hpp (SteerParams, steerOnGrid, steerWindow, steerUnits, fillTwist, fillLocalPlan).  The grid
// comes from integer hashes of the cell number, so that tests/test_navsteer_gpu.py makes the same arrays and compares counts and
// FNV-1a checksums with the Python calls.  planOnGrid makes the cost field, steerOnGrid rolls a dynamic window's lattice out from
// six poses, and the winner of each goes into a geometry_msgs::Twist and a nav_msgs::Path (doubles).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include "ssf.hpp"
#include "nav_msgs_path_double.hpp"
#include "geometry_msgs_twist_double.hpp"

static uint64_t fnv1a(const void* p, size_t n, uint64_t h = 1469598103934665603ull) {
    const unsigned char* b = static_cast<const unsigned char*>(p);
    for (size_t i = 0; i < n; i++) { h ^= b[i]; h *= 1099511628211ull; }
    return h;
}

int main() {
    using namespace supersurfel_fusion;
    CamParam cam; cam.width = 160; cam.height = 128; cam.fx = 150.f; cam.fy = 150.f; cam.cx = 79.5f; cam.cy = 63.5f;
    try {
        // the window helper needs no handle: 0.3 m/s now, 0.5 m/s^2 and 2 rad/s^2 over 0.1 s, 0.05 m cells
        SteerParams q;
        SupersurfelFusion::steerWindow(0.3, 0.0, 0.0, 0.5, -1.0, 1.0, 0.5, 2.0, 0.1, 0.05f, 9, 33, q);
        std::printf("window n_v=%d n_w=%d v_min=%d v_step=%d w_min=%d w_step=%d\n", q.n_v, q.n_w, q.v_min, q.v_step, q.w_min, q.w_step);
        const SteerPose u = steerUnits(1.0, 2.0, -0.1, 0.05f);
        std::printf("units x=%d y=%d heading=%d\n", u.x, u.y, u.heading);

        SupersurfelFusion a;
        a.setDepthPrefilter(false);
        a.initialize(cam, 16, 10.f, 1000.f, 1000.f, 1e8f);
        NavGrid g;
        g.width = 70; g.height = 45; g.res = 0.05f;
        const size_t P = (size_t)g.width * g.height;
        g.state.resize(P); g.dist2.resize(P);
        for (size_t p = 0; p < P; p++) {
            const uint32_t h = ((uint32_t)p * 2654435761u) >> 16;
            g.state[p] = (int8_t)(h % 100u < 6u ? 100 : (h % 100u < 10u ? -1 : 0));
            g.dist2[p] = g.state[p] == 0 ? (int32_t)(1u + (h >> 7) % 40u) : 0;
        }
        const float rt[12] = {1.f, 0.f, 0.f, 0.f, 0.f, -1.f, 0.f, 1.f, 0.f, -1.2f, 0.f, -0.2f};
        g.stats = ssf_navgrid_stats();
        std::memcpy(g.stats.pose, rt, sizeof(rt));
        PlanParams pq;
        pq.want_frontier = false;
        NavPlan plan;
        std::vector<GridCell> goals(1), none;
        goals[0][0] = 60; goals[0][1] = 30;
        a.planOnGrid(g, pq, goals, none, plan);
        std::vector<SteerPose> poses;
        for (int k = 0; k < 6; k++) { SteerPose p; p.x = (5 + 11 * k) * 1024 + 300; p.y = (4 + 7 * k) * 1024 + 700; p.heading = 9000 * k; poses.push_back(p); }
        q = SteerParams();
        q.n_steps = 24; q.want_candidates = true;
        NavSteer s;
        a.steerOnGrid(g, &plan, poses, std::vector<SteerTarget>(), q, s);
        std::vector<int32_t> flat;
        for (size_t i = 0; i < s.traj.size(); i++)
            for (size_t k = 0; k < s.traj[i].size(); k++) { flat.push_back(s.traj[i][k].x); flat.push_back(s.traj[i][k].y); flat.push_back(s.traj[i][k].heading); }
        std::printf("navsteer ok=%lld blocked=%lld stuck=%lld admissible=%lld collided=%lld steps=%lld best=%016llx v=%016llx w=%016llx score=%016llx "
                    "traj=%016llx cand_score=%016llx cand_end=%016llx\n", (long long)s.stats.poses_ok, (long long)s.stats.poses_blocked,
                    (long long)s.stats.poses_stuck, (long long)s.stats.admissible, (long long)s.stats.collided, (long long)s.stats.steps_taken,
                    (unsigned long long)fnv1a(s.best.data(), 4 * s.best.size()), (unsigned long long)fnv1a(s.v.data(), 4 * s.v.size()),
                    (unsigned long long)fnv1a(s.w.data(), 4 * s.w.size()), (unsigned long long)fnv1a(s.score.data(), 8 * s.score.size()),
                    (unsigned long long)fnv1a(flat.data(), 4 * flat.size()), (unsigned long long)fnv1a(s.cand_score.data(), 8 * s.cand_score.size()),
                    (unsigned long long)fnv1a(s.cand_end.data(), 4 * s.cand_end.size()));
        // the messages of the first pose with a winner
        size_t win = 0;
        while (win < s.best.size() && s.best[win] < 0) win++;
        bool ok = win < s.best.size();
        if (ok) {
            const float dt = 0.1f;
            geometry_msgs::Twist tw;
            SupersurfelFusion::fillTwist(s, win, g.res, dt, tw);
            nav_msgs::Path path;
            SupersurfelFusion::fillLocalPlan(s, win, g.stats.pose, g.res, path);
            ok = std::fabs(tw.linear.x - (double)s.v[win] * (double)g.res / (1024.0 * (double)dt)) < 1e-12 && tw.linear.y == 0.0 && tw.angular.x == 0.0 &&
                 std::fabs(tw.angular.z - (double)s.w[win] * 6.283185307179586 / (65536.0 * (double)dt)) < 1e-12 && path.poses.size() == s.traj[win].size() &&
                 !path.poses.empty();
            // the grid's y is the map's z: the first pose's map position
            const double x = (double)s.traj[win][0].x / 1024.0 * 0.05f, y = (double)s.traj[win][0].y / 1024.0 * 0.05f;
            ok = ok && std::fabs(path.poses[0].pose.position.x - (x - 1.2f)) < 1e-6 && std::fabs(path.poses[0].pose.position.z - (y - 0.2f)) < 1e-6 &&
                 std::fabs(path.poses[0].pose.position.y) < 1e-9;
            std::printf("twist pose=%zu v=%d w=%d linear.x=%.9f angular.z=%.9f poses=%zu\n", win, s.v[win], s.w[win], tw.linear.x, tw.angular.z, path.poses.size());
        }
        std::printf("messages ok=%d\n", ok ? 1 : 0);
        return ok ? 0 : 1;
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 2;
    }
}
