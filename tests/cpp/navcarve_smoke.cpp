// The carved navigation grid of include/ssf.hpp (CarveParams, buildNavGrid with views, CarvedNavGrid).  The frames and the grid of
// navgrid_smoke.cpp; the views are the six camera poses the frames were tracked at.  Prints the carve's counts and the FNV-1a
// checksums of the carved state, dist2 and seen (tests/test_navcarve_gpu.py compares them with the Python call on the same map),
// checks that no views give buildNavGrid's grid, and fills the OccupancyGrid double from the carved grid.
#include <array>
#include <cstdio>
#include <cstring>
#include <vector>
#include "ssf.hpp"
#include "nav_msgs_double.hpp"

static uint64_t fnv1a(const void* p, size_t n) {
    uint64_t h = 1469598103934665603ull;
    const unsigned char* b = static_cast<const unsigned char*>(p);
    for (size_t i = 0; i < n; i++) { h ^= b[i]; h *= 1099511628211ull; }
    return h;
}

int main() {
    using namespace supersurfel_fusion;
    const int W = 160, H = 128;
    const size_t P = (size_t)W * H;
    CamParam cam; cam.width = W; cam.height = H; cam.fx = 150.f; cam.fy = 150.f; cam.cx = 79.5f; cam.cy = 63.5f;
    std::vector<uint8_t> rgb(3 * P);
    std::vector<float> depth(P);
    try {
        SupersurfelFusion a;
        a.setDepthPrefilter(false);
        a.initialize(cam, 16, 10.f, 1000.f, 1000.f, 1e8f);
        std::vector<std::array<float, 12> > views;
        for (int k = 0; k < 6; k++) {
            for (size_t i = 0; i < P; i++) {
                const int x = (int)(i % W) + 2 * k, y = (int)(i / W);
                rgb[3 * i] = (uint8_t)(x * 255 / (W + 16)); rgb[3 * i + 1] = (uint8_t)(y * 255 / H); rgb[3 * i + 2] = (uint8_t)((x ^ y) & 255);
                depth[i] = 1.0f + 0.004f * (float)x;
            }
            a.processFrame(rgb.data(), depth.data());
            std::array<float, 12> v;
            if (ssf_get_pose(a.handle(), v.data()) != SSF_OK) { std::printf("no pose\n"); return 2; }
            views.push_back(v);
        }
        const float rt[12] = {0.f, 1.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, -1.f, -1.6f, -1.6f, 0.f};
        const Transform3 frame = transform3_from_rt(rt);
        NavGridParams g;
        g.pose = &frame; g.width = 64; g.height = 64; g.res = 0.05f;
        g.z_min = -2.0f; g.floor_max = -1.3f; g.z_max = 0.0f; g.max_dist_cells = 12;
        CarveParams c;
        c.stride = 4; c.hit_margin_cells = 2.f;
        CarvedNavGrid grid;
        a.buildNavGrid(g, c, views, grid);
        const ssf_navcarve_stats& s = grid.carve;
        std::printf("navcarve %dx%d rays=%lld hit=%lld invalid=%lld carving=%lld samples=%lld entries=%lld seen=%lld carved=%lld free=%lld "
                    "occupied=%lld unknown=%lld state=%016llx dist2=%016llx seen=%016llx\n",
                    grid.width, grid.height, (long long)s.rays, (long long)s.rays_hit, (long long)s.rays_invalid, (long long)s.rays_carving,
                    (long long)s.ray_samples, (long long)s.ray_entries, (long long)s.cells_seen, (long long)s.cells_carved,
                    (long long)grid.stats.cells_free, (long long)grid.stats.cells_occupied, (long long)grid.stats.cells_unknown,
                    (unsigned long long)fnv1a(grid.state.data(), grid.state.size()), (unsigned long long)fnv1a(grid.dist2.data(), 4 * grid.dist2.size()),
                    (unsigned long long)fnv1a(grid.seen.data(), 4 * grid.seen.size()));
        if (grid.seen.size() != 64u * 64u || s.rays != 6 * 40 * 32) { std::printf("sizes\n"); return 2; }
        nav_msgs::OccupancyGrid msg;
        SupersurfelFusion::fillOccupancyGrid(grid, msg);
        if (msg.data.size() != grid.state.size() || std::memcmp(msg.data.data(), grid.state.data(), grid.state.size()) != 0) { std::printf("data differs\n"); return 2; }
        // no views: the grid of buildNavGrid
        NavGrid plain;
        a.buildNavGrid(g, plain);
        CarvedNavGrid none;
        a.buildNavGrid(g, c, nullptr, 0, none);
        const bool same = none.state == plain.state && none.dist2 == plain.dist2 && none.hits == plain.hits &&
                          std::memcmp(none.zmin.data(), plain.zmin.data(), 4 * plain.zmin.size()) == 0 && none.carve.rays == 0 && none.carve.cells_carved == 0;
        std::printf("no_views same=%d seen_sum=%llu\n", same ? 1 : 0, (unsigned long long)fnv1a(none.seen.data(), 4 * none.seen.size()));
        if (!same) return 2;
        for (size_t i = 0; i < none.seen.size(); i++) if (none.seen[i] != 0u) return 2;
    } catch (const std::exception& e) { std::printf("exception %s\n", e.what()); return 1; }
    return 0;
}
