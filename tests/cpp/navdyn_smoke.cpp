// Steering among movers through include/ssf.hpp (Mover, MoverBlob, MoverTracker, steerAmongMovers, steerFootprintAmongMovers,
// moverBlobs).  With --tracker it runs the case list of tests/navdyn_ref.py (TRACKER_CASES: the same numbers) through supersurfel_fusion::MoverTracker
// and prints every mover list, touching no device: tests/test_navdyn.py compares it with the Python tracker.  Without an argument it
// steers on the grid of integer hashes that tests/cpp/navfoot_smoke.cpp uses and prints counts and FNV-1a checksums, which
// tests/test_navdyn_gpu.py compares with the Python calls on the same arrays.
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

using namespace supersurfel_fusion;

static MoverBlob blob(int label, int n, int cx, int cy, int r, int ex, int ey) {
    MoverBlob b; b.label = label; b.n = n; b.cx = cx; b.cy = cy; b.r = r; b.ex = ex; b.ey = ey; b.pad = 0;
    return b;
}
static void show(int k, int u, const std::vector<Mover>& m) {
    std::printf("case %d update %d:", k, u);
    for (size_t i = 0; i < m.size(); i++) std::printf(" (%d %d %d %d %d %d)", m[i].x, m[i].y, m[i].vx, m[i].vy, m[i].r, m[i].grow);
    std::printf("\n");
}
static void tracker_cases() {
    {
        MoverTracker t(2048, 300, 16, 128);
        show(0, 0, t.update(std::vector<MoverBlob>(1, blob(5, 40, 10000, 20000, 700, 500, 500)), 1));
        show(0, 1, t.update(std::vector<MoverBlob>(1, blob(9, 44, 10301, 19499, 650, 400, 500)), 2));
        show(0, 2, t.update(std::vector<MoverBlob>(1, blob(9, 44, 20000, 19499, 650, 400, 500)), 1));
    }
    {
        MoverTracker t(1000, 0, 5, 50);
        std::vector<MoverBlob> a, b;
        a.push_back(blob(1, 9, 0, 0, 10, 1, 1)); a.push_back(blob(2, 8, 600, 0, 10, 1, 1));
        b.push_back(blob(7, 9, 300, 0, 10, 1, 1)); b.push_back(blob(8, 9, 300, 1, 10, 1, 1)); b.push_back(blob(9, 9, 5000, 5000, 10, 1, 1));
        show(1, 0, t.update(a, 1));
        show(1, 1, t.update(b, 3));
    }
    {
        MoverTracker t(1 << 25, 1 << 20, 4096, 4096);
        show(2, 0, t.update(std::vector<MoverBlob>(1, blob(1, 1, -(1 << 23), 1 << 23, 1 << 20, 0, 0)), 1));
        show(2, 1, t.update(std::vector<MoverBlob>(1, blob(1, 1, 1 << 23, -(1 << 23), 1 << 20, 0, 0)), 1));
    }
}

int main(int argc, char** argv) {
    CamParam cam; cam.width = 160; cam.height = 128; cam.fx = 150.f; cam.fy = 150.f; cam.cx = 79.5f; cam.cy = 63.5f;
    try {
        std::printf("sizes params=%zu out=%zu stats=%zu blob_params=%zu blob_stats=%zu mover=%zu blob=%zu\n", sizeof(ssf_navdyn_params), sizeof(ssf_navdyn_out),
                    sizeof(ssf_navdyn_stats), sizeof(ssf_navdyn_blob_params), sizeof(ssf_navdyn_blob_stats), sizeof(Mover), sizeof(MoverBlob));
        if (argc > 1 && std::strcmp(argv[1], "--tracker") == 0) { tracker_cases(); return 0; }

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
        std::vector<SteerPose> poses;
        for (int k = 0; k < 6; k++) { SteerPose p; p.x = (5 + 11 * k) * 1024 + 300; p.y = (4 + 7 * k) * 1024 + 700; p.heading = 9000 * k; poses.push_back(p); }
        // the movers: two blobs seen twice, two steps apart, through the tracker
        MoverTracker tracker(4096, 400, 16, 128);
        std::vector<MoverBlob> t0, t1;
        t0.push_back(blob(3, 50, 20 * 1024, 14 * 1024, 600, 400, 400)); t0.push_back(blob(8, 30, 44 * 1024, 30 * 1024, 500, 300, 400));
        t1.push_back(blob(3, 52, 20 * 1024 - 600, 14 * 1024 - 300, 600, 400, 400)); t1.push_back(blob(9, 31, 44 * 1024 - 500, 30 * 1024 + 400, 500, 300, 400));
        tracker.update(t0, 1);
        const std::vector<Mover> movers = tracker.update(t1, 2);
        show(9, 0, movers);
        SteerParams q;
        q.n_steps = 24; q.want_candidates = true;
        MoverParams m;
        m.mover_cap = 3000; m.mover_weight = 5; m.want_candidates = true;
        NavSteerAmongMovers s;
        a.steerAmongMovers(g, &plan, poses, std::vector<SteerTarget>(), movers, q, m, s);
        std::vector<int32_t> flat;
        for (size_t i = 0; i < s.traj.size(); i++)
            for (size_t k = 0; k < s.traj[i].size(); k++) { flat.push_back(s.traj[i][k].x); flat.push_back(s.traj[i][k].y); flat.push_back(s.traj[i][k].heading); }
        std::printf("dynsteer ok=%lld admissible=%lld collided=%lld steps=%lld hit=%lld best=%016llx score=%016llx traj=%016llx cand_score=%016llx "
                    "min_gap=%016llx cand_hit=%016llx cand_min_gap=%016llx\n", (long long)s.stats.poses_ok, (long long)s.stats.admissible,
                    (long long)s.stats.collided, (long long)s.stats.steps_taken, (long long)s.dyn.hit_movers,
                    (unsigned long long)fnv1a(s.best.data(), 4 * s.best.size()), (unsigned long long)fnv1a(s.score.data(), 8 * s.score.size()),
                    (unsigned long long)fnv1a(flat.data(), 4 * flat.size()), (unsigned long long)fnv1a(s.cand_score.data(), 8 * s.cand_score.size()),
                    (unsigned long long)fnv1a(s.min_gap.data(), 4 * s.min_gap.size()), (unsigned long long)fnv1a(s.cand_hit.data(), 4 * s.cand_hit.size()),
                    (unsigned long long)fnv1a(s.cand_min_gap.data(), 4 * s.cand_min_gap.size()));
        // the same with the oriented body
        FootprintParams f = footprintUnits(0.1, 0.05, 0.05, 0.05, 0.05f);
        f.pad = 0; f.n_headings = 16;
        FootprintLayers lay;
        a.footprintLayers(g, f, lay);
        NavSteerAmongMovers sf;
        a.steerFootprintAmongMovers(g, lay, &plan, poses, std::vector<SteerTarget>(), movers, q, m, sf);
        std::printf("dynfoot ok=%lld admissible=%lld hit=%lld best=%016llx score=%016llx min_gap=%016llx cand_hit=%016llx\n", (long long)sf.stats.poses_ok,
                    (long long)sf.stats.admissible, (long long)sf.dyn.hit_movers, (unsigned long long)fnv1a(sf.best.data(), 4 * sf.best.size()),
                    (unsigned long long)fnv1a(sf.score.data(), 8 * sf.score.size()), (unsigned long long)fnv1a(sf.min_gap.data(), 4 * sf.min_gap.size()),
                    (unsigned long long)fnv1a(sf.cand_hit.data(), 4 * sf.cand_hit.size()));
        // the blobs of a flat wall one metre ahead, its left half labelled 7 and its right half labelled 80
        std::vector<float> depth((size_t)cam.width * cam.height, 1.0f);
        std::vector<uint8_t> mask(depth.size(), 1);
        std::vector<int32_t> label(depth.size());
        for (int v = 0; v < cam.height; v++)
            for (int u = 0; u < cam.width; u++) label[(size_t)v * cam.width + u] = u < 80 ? 7 : 80;
        LiveParams lq;
        lq.floor_max = -10.f; lq.z_max = 10.f;
        MoverBlobs mb;
        a.moverBlobs(g, lq, depth.data(), mask, label, MoverBlobParams(), mb);
        std::printf("blobs member=%lld band=%lld labels=%lld kept=%lld written=%lld rows=%016llx\n", (long long)mb.stats.pixels_member,
                    (long long)mb.stats.points_in_band, (long long)mb.stats.labels_seen, (long long)mb.stats.blobs_kept, (long long)mb.stats.blobs_written,
                    (unsigned long long)fnv1a(mb.blobs.empty() ? nullptr : &mb.blobs[0].label, sizeof(MoverBlob) * mb.blobs.size()));
        // the result feeds the disc's message helpers unchanged: the first pose with a winner
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
        }
        std::printf("messages ok=%d\n", ok ? 1 : 0);
        return ok ? 0 : 1;
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 2;
    }
}
