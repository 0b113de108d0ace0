// The oriented footprint of include/ssf.hpp (FootprintParams, footprintUnits, footprintPad, footprintLayers, steerWithFootprint).  The
// grid comes from integer hashes of the cell number, as tests/cpp/navsteer_smoke.cpp's does, so that tests/test_navfoot_gpu.py makes the
// same arrays and compares counts and FNV-1a checksums with the Python calls.  With --sizes it prints the structs' sizes and the host
// helpers' values and touches no device.
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

int main(int argc, char** argv) {
    using namespace supersurfel_fusion;
    CamParam cam; cam.width = 160; cam.height = 128; cam.fx = 150.f; cam.fy = 150.f; cam.cx = 79.5f; cam.cy = 63.5f;
    try {
        // the host helpers need no handle: a 0.15 m x 0.1 m body, its centre 0.05 m from the back, on 0.05 m cells
        FootprintParams f = footprintUnits(0.1, 0.05, 0.05, 0.05, 0.05f);
        std::printf("sizes params=%zu out=%zu stats=%zu\n", sizeof(ssf_navfoot_params), sizeof(ssf_navfoot_out), sizeof(ssf_navfoot_stats));
        std::printf("units front=%d back=%d left=%d right=%d pad16=%d pad32=%d\n", f.front, f.back, f.left, f.right,
                    SupersurfelFusion::footprintPad(f.front, f.back, f.left, f.right, 16), SupersurfelFusion::footprintPad(f.front, f.back, f.left, f.right, 32));
        int16_t spans[SSF_NAVFOOT_MAX_HEADINGS * SSF_NAVFOOT_ROWS * 2];
        int32_t reach = -1; int64_t cells = -1;
        const int rc = ssf_navfoot_spans(f.front, f.back, f.left, f.right, 0, 16, spans, &reach, &cells);
        std::printf("spans rc=%d reach=%d cells=%lld sum=%016llx\n", rc, (int)reach, (long long)cells, (unsigned long long)fnv1a(spans, sizeof(int16_t) * 16 * SSF_NAVFOOT_ROWS * 2));
        if (argc > 1 && std::strcmp(argv[1], "--sizes") == 0) return rc == SSF_OK ? 0 : 1;

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
        PlanParams pq;
        pq.want_frontier = false;
        NavPlan plan;
        std::vector<GridCell> goals(1), none;
        goals[0][0] = 60; goals[0][1] = 30;
        a.planOnGrid(g, pq, goals, none, plan);
        f.pad = 0; f.n_headings = 16; f.want_n_free = true;
        FootprintLayers lay;
        a.footprintLayers(g, f, lay);
        std::printf("navfoot clear=%lld all=%lld some=%lld none=%lld reach=%lld cells=%lld mask=%016llx n_free=%016llx\n", (long long)lay.stats.cells_clear,
                    (long long)lay.stats.cells_all, (long long)lay.stats.cells_some, (long long)lay.stats.cells_none, (long long)lay.stats.reach,
                    (long long)lay.stats.kernel_cells, (unsigned long long)fnv1a(lay.free_mask.data(), 4 * lay.free_mask.size()),
                    (unsigned long long)fnv1a(lay.n_free.data(), lay.n_free.size()));
        std::vector<SteerPose> poses;
        for (int k = 0; k < 6; k++) { SteerPose p; p.x = (5 + 11 * k) * 1024 + 300; p.y = (4 + 7 * k) * 1024 + 700; p.heading = 9000 * k; poses.push_back(p); }
        SteerParams q;
        q.n_steps = 24; q.want_candidates = true;
        NavSteer s;
        a.steerWithFootprint(g, lay, &plan, poses, std::vector<SteerTarget>(), q, s);
        std::vector<int32_t> flat;
        for (size_t i = 0; i < s.traj.size(); i++)
            for (size_t k = 0; k < s.traj[i].size(); k++) { flat.push_back(s.traj[i][k].x); flat.push_back(s.traj[i][k].y); flat.push_back(s.traj[i][k].heading); }
        std::printf("footsteer ok=%lld blocked=%lld stuck=%lld admissible=%lld collided=%lld steps=%lld best=%016llx v=%016llx w=%016llx score=%016llx "
                    "traj=%016llx cand_score=%016llx cand_end=%016llx\n", (long long)s.stats.poses_ok, (long long)s.stats.poses_blocked,
                    (long long)s.stats.poses_stuck, (long long)s.stats.admissible, (long long)s.stats.collided, (long long)s.stats.steps_taken,
                    (unsigned long long)fnv1a(s.best.data(), 4 * s.best.size()), (unsigned long long)fnv1a(s.v.data(), 4 * s.v.size()),
                    (unsigned long long)fnv1a(s.w.data(), 4 * s.w.size()), (unsigned long long)fnv1a(s.score.data(), 8 * s.score.size()),
                    (unsigned long long)fnv1a(flat.data(), 4 * flat.size()), (unsigned long long)fnv1a(s.cand_score.data(), 8 * s.cand_score.size()),
                    (unsigned long long)fnv1a(s.cand_end.data(), 4 * s.cand_end.size()));
        // the result feeds the disc's message helpers: the first pose with a winner
        size_t win = 0;
        while (win < s.best.size() && s.best[win] < 0) win++;
        bool ok = win < s.best.size();
        if (ok) {
            const float dt = 0.1f;
            geometry_msgs::Twist tw;
            SupersurfelFusion::fillTwist(s, win, g.res, dt, tw);
            nav_msgs::Path path;
            SupersurfelFusion::fillLocalPlan(s, win, g.stats.pose, g.res, path);
            ok = std::fabs(tw.linear.x - (double)s.v[win] * (double)g.res / (1024.0 * (double)dt)) < 1e-12 && path.poses.size() == s.traj[win].size() &&
                 !path.poses.empty();
            std::printf("twist pose=%zu v=%d w=%d poses=%zu\n", win, s.v[win], s.w[win], path.poses.size());
        }
        // the layers of another grid are refused before the library is asked
        bool threw = false;
        NavGrid other = g;
        other.width = 35; other.height = 90;
        try { a.steerWithFootprint(other, lay, &plan, poses, std::vector<SteerTarget>(), q, s); } catch (const std::logic_error&) { threw = true; }
        std::printf("messages ok=%d\n", ok && threw ? 1 : 0);
        return ok && threw ? 0 : 1;
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 2;
    }
}
