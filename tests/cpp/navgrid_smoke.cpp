// The navigation-grid surface of include/ssf.hpp (NavGridParams, buildNavGrid, fillOccupancyGrid).  The frames of query_smoke.cpp:
// a tilted plane seen by a camera that steps sideways.  The grid's frame takes the camera's viewing direction as "down", so the
// plane is the floor and its near part, above floor_max, the obstacle.  Prints the grid's counts and the FNV-1a checksums of the
// state and dist2 bytes (tests/test_navgrid_gpu.py compares them with the Python call on the same map), then fills the
// OccupancyGrid double.
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
        for (int k = 0; k < 6; k++) {
            for (size_t i = 0; i < P; i++) {
                const int x = (int)(i % W) + 2 * k, y = (int)(i / W);
                rgb[3 * i] = (uint8_t)(x * 255 / (W + 16)); rgb[3 * i + 1] = (uint8_t)(y * 255 / H); rgb[3 * i + 2] = (uint8_t)((x ^ y) & 255);
                depth[i] = 1.0f + 0.004f * (float)x;
            }
            a.processFrame(rgb.data(), depth.data());
        }
        // grid x = map y, grid y = map x, grid z = -map z; 3.2 m x 3.2 m about the first camera's axis
        const float rt[12] = {0.f, 1.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, -1.f, -1.6f, -1.6f, 0.f};
        const Transform3 frame = transform3_from_rt(rt);
        NavGridParams g;
        g.pose = &frame; g.width = 64; g.height = 64; g.res = 0.05f;
        g.z_min = -2.0f; g.floor_max = -1.3f; g.z_max = 0.0f; g.max_dist_cells = 12;
        NavGrid grid;
        a.buildNavGrid(g, grid);
        const ssf_navgrid_stats& s = grid.stats;
        std::printf("navgrid %dx%d rows=%lld samples=%lld in_grid=%lld free=%lld occupied=%lld unknown=%lld state=%016llx dist2=%016llx hits=%016llx\n",
                    grid.width, grid.height, (long long)s.rows_used, (long long)s.samples, (long long)s.samples_in_grid, (long long)s.cells_free,
                    (long long)s.cells_occupied, (long long)s.cells_unknown, (unsigned long long)fnv1a(grid.state.data(), grid.state.size()),
                    (unsigned long long)fnv1a(grid.dist2.data(), 4 * grid.dist2.size()), (unsigned long long)fnv1a(grid.hits.data(), 4 * grid.hits.size()));
        if (s.cells_free + s.cells_occupied + s.cells_unknown != 64 * 64) { std::printf("the cells do not add up\n"); return 2; }
        if (grid.zmin.size() != 64u * 64u || grid.hits.size() != 2u * 64u * 64u) { std::printf("sizes\n"); return 2; }
        nav_msgs::OccupancyGrid msg;
        SupersurfelFusion::fillOccupancyGrid(grid, msg);
        std::printf("occupancy %ux%u res=%.3f origin=(%.2f %.2f %.2f) q=(%.4f %.4f %.4f %.4f) data=%zu\n", msg.info.width, msg.info.height,
                    (double)msg.info.resolution, msg.info.origin.position.x, msg.info.origin.position.y, msg.info.origin.position.z,
                    msg.info.origin.orientation.x, msg.info.origin.orientation.y, msg.info.origin.orientation.z, msg.info.origin.orientation.w,
                    msg.data.size());
        if (msg.data.size() != grid.state.size() || std::memcmp(msg.data.data(), grid.state.data(), grid.state.size()) != 0) { std::printf("data differs\n"); return 2; }
        // dist2 alone, and the default frame
        NavGridParams d;
        d.width = 32; d.height = 48; d.want_heights = d.want_hits = d.want_state = false;
        NavGrid only;
        a.buildNavGrid(d, only);
        std::printf("dist2_alone %zu state=%zu zmin=%zu t=(%.2f %.2f %.2f)\n", only.dist2.size(), only.state.size(), only.zmin.size(),
                    (double)only.stats.pose[9], (double)only.stats.pose[10], (double)only.stats.pose[11]);
        if (only.dist2.size() != 32u * 48u || !only.state.empty()) return 2;
    } catch (const std::exception& e) { std::printf("exception %s\n", e.what()); return 1; }
    return 0;
}
