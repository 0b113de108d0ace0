// The plan over (x, y, heading) of include/ssf.hpp (PosePlanParams, planPoses, fillPosePath, PosePlan::costAsPlan).  The grid comes
// from integer hashes of the cell number, as tests/cpp/navfoot_smoke.cpp's does, so that tests/test_navpose_gpu.py makes the same arrays
// and compares counts and FNV-1a checksums with the Python calls.  With --sizes it prints the structs' sizes and the move tables'
// checksums and touches no device.
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

int main(int argc, char** argv) {
    using namespace supersurfel_fusion;
    CamParam cam; cam.width = 160; cam.height = 128; cam.fx = 150.f; cam.fy = 150.f; cam.cx = 79.5f; cam.cy = 63.5f;
    try {
        // the move table needs no handle
        std::printf("sizes params=%zu out=%zu stats=%zu\n", sizeof(ssf_navpose_params), sizeof(ssf_navpose_out), sizeof(ssf_navpose_stats));
        bool tables = true;
        const int tols[3] = {0, 64, 256};
        for (int B = 1; B <= SSF_NAVFOOT_MAX_HEADINGS; B *= 2)
            for (int t = 0; t < 3; t++)
                for (int rev = 0; rev < 2; rev++) {
                    std::vector<int8_t> m((size_t)B * 8 + 1, 77);                       // one guard byte behind the table
                    const int rc = ssf_navpose_moves(B, tols[t], rev, m.data());
                    tables = tables && rc == SSF_OK && m[(size_t)B * 8] == 77;
                    std::printf("moves B=%d tol=%d rev=%d rc=%d sum=%016llx\n", B, tols[t], rev, rc, (unsigned long long)fnv1a(m.data(), (size_t)B * 8));
                }
        int8_t one[8];
        const bool refused = ssf_navpose_moves(3, 64, 1, one) != SSF_OK && ssf_navpose_moves(8, 257, 1, one) != SSF_OK && ssf_navpose_moves(8, -1, 1, one) != SSF_OK &&
                             ssf_navpose_moves(8, 64, 2, one) != SSF_OK && ssf_navpose_moves(8, 64, 1, nullptr) != SSF_OK;
        std::printf("moves refused=%d\n", refused ? 1 : 0);
        if (argc > 1 && std::strcmp(argv[1], "--sizes") == 0) return tables && refused ? 0 : 1;

        SupersurfelFusion a;
        a.setDepthPrefilter(false);
        a.initialize(cam, 16, 10.f, 1000.f, 1000.f, 1e8f);
        NavGrid g;
        g.width = 70; g.height = 45; g.res = 0.05f;
        const size_t P = (size_t)g.width * g.height;
        g.state.resize(P); g.dist2.resize(P);
        for (size_t p = 0; p < P; p++) {
            const uint32_t h = ((uint32_t)p * 2654435761u) >> 16;
            g.state[p] = (int8_t)(h % 100u < 3u ? 100 : (h % 100u < 5u ? -1 : 0));
            g.dist2[p] = g.state[p] == 0 ? (int32_t)(1u + (h >> 7) % 40u) : 0;
        }
        const float rt[12] = {1.f, 0.f, 0.f, 0.f, 0.f, -1.f, 0.f, 1.f, 0.f, -1.2f, 0.f, -0.2f};
        g.stats = ssf_navgrid_stats();
        std::memcpy(g.stats.pose, rt, sizeof(rt));
        FootprintParams f = footprintUnits(0.1, 0.05, 0.05, 0.05, 0.05f);
        f.pad = 0; f.n_headings = 16;
        FootprintLayers lay;
        a.footprintLayers(g, f, lay);
        std::vector<PoseState> goals(2);
        goals[0][0] = 60; goals[0][1] = 30; goals[0][2] = -1;
        goals[1][0] = 5; goals[1][1] = 40; goals[1][2] = 4;
        std::vector<SteerPose> poses;
        for (int k = 0; k < 6; k++) { SteerPose p; p.x = (5 + 11 * k) * 1024 + 300; p.y = (4 + 7 * k) * 1024 + 700; p.heading = 9000 * k; poses.push_back(p); }
        PosePlanParams q;
        q.max_path = 512; q.want_cost = true; q.soft_dist2 = 20; q.near_penalty = 8;
        PosePlan plan;
        a.planPoses(g, lay, q, goals, poses, plan);
        std::vector<int32_t> flat;
        for (size_t i = 0; i < plan.paths.size(); i++)
            for (size_t k = 0; k < plan.paths[i].size(); k++) for (size_t c = 0; c < 3; c++) flat.push_back(plan.paths[i][k][c]);
        std::printf("navpose traversable=%lld reached=%lld cells=%lld used=%lld blocked=%lld outside=%lld max=%lld cost=%016llx cell_cost=%016llx "
                    "cell_bin=%016llx start_cost=%016llx status=%016llx paths=%016llx\n", (long long)plan.stats.states_traversable,
                    (long long)plan.stats.states_reached, (long long)plan.stats.cells_reached, (long long)plan.stats.goals_used,
                    (long long)plan.stats.goals_blocked, (long long)plan.stats.goals_outside, (long long)plan.stats.max_cost,
                    (unsigned long long)fnv1a(plan.cost.data(), 4 * plan.cost.size()), (unsigned long long)fnv1a(plan.cell_cost.data(), 4 * plan.cell_cost.size()),
                    (unsigned long long)fnv1a(plan.cell_bin.data(), plan.cell_bin.size()), (unsigned long long)fnv1a(plan.start_cost.data(), 4 * plan.start_cost.size()),
                    (unsigned long long)fnv1a(plan.start_status.data(), 4 * plan.start_status.size()), (unsigned long long)fnv1a(flat.data(), 4 * flat.size()));
        // the projection is the rollouts' cost term
        SteerParams sq;
        sq.n_steps = 24;
        NavSteer s;
        const NavPlan as_plan = plan.costAsPlan();
        a.steerWithFootprint(g, lay, &as_plan, poses, std::vector<SteerTarget>(), sq, s);
        std::printf("posesteer ok=%lld best=%016llx\n", (long long)s.stats.poses_ok, (unsigned long long)fnv1a(s.best.data(), 4 * s.best.size()));
        // the message: one pose per state, at the cell's centre, turned by the bin
        size_t win = 0;
        while (win < plan.paths.size() && plan.paths[win].size() < 2) win++;
        bool ok = win < plan.paths.size();
        if (ok) {
            nav_msgs::Path path;
            SupersurfelFusion::fillPosePath(plan, win, g.stats.pose, g.res, path);
            const PoseState& s0 = plan.paths[win][0];
            const double x = (s0[0] + 0.5) * (double)g.res, y = (s0[1] + 0.5) * (double)g.res;
            ok = path.poses.size() == plan.paths[win].size() && std::fabs(path.poses[0].pose.position.x - (x - 1.2)) < 1e-6 &&
                 std::fabs(path.poses[0].pose.position.y - 0.0) < 1e-6 && std::fabs(path.poses[0].pose.position.z - (y - 0.2)) < 1e-6;
            double norm = 0.0;
            for (size_t k = 0; k < path.poses.size(); k++) {
                const double w = path.poses[k].pose.orientation.w, qx = path.poses[k].pose.orientation.x, qy = path.poses[k].pose.orientation.y,
                             qz = path.poses[k].pose.orientation.z;
                norm = std::max(norm, std::fabs(w * w + qx * qx + qy * qy + qz * qz - 1.0));
            }
            ok = ok && norm < 1e-9;
            std::printf("path start=%zu states=%zu\n", win, path.poses.size());
        }
        // the layers of another grid are refused before the library is asked
        bool threw = false;
        NavGrid other = g;
        other.width = 35; other.height = 90;
        try { a.planPoses(other, lay, q, goals, poses, plan); } catch (const std::logic_error&) { threw = true; }
        std::printf("messages ok=%d\n", ok && threw ? 1 : 0);
        return ok && threw ? 0 : 1;
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 2;
    }
}
