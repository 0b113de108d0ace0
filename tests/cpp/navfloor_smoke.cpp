// The floor-fit surface of include/ssf.hpp (FloorParams, FloorFit, fitFloor, buildNavGridOnFloor).  The frames of navgrid_smoke.cpp: a
// tilted plane seen by a camera that steps sideways.  The up hint is the direction towards the camera, so the plane is the floor, about
// 31 degrees off the hint.  Prints the fit's status and counts and the FNV-1a checksums of its sums, plane and pose, then the counts and
// checksums of the grid built in the fitted frame (tests/test_navfloor_gpu.py compares them with the Python calls on the same map).
#include <cstdio>
#include <cstring>
#include <vector>
#include "ssf.hpp"

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
        FloorParams f;
        f.up = float3{0.f, 0.f, -1.f};
        f.min_rows = 8; f.width = 64; f.height = 48; f.res = 0.05f; f.below = 0.3f; f.step = 0.1f; f.body_height = 1.0f;
        f.want_histograms = true;
        FloorFit fit;
        NavGridParams g;
        g.max_dist_cells = 12;
        NavGrid grid;
        a.buildNavGridOnFloor(f, g, fit, grid);
        const ssf_navfloor_fit_result& r = fit.fit;
        std::printf("navfloor status=%d rounds=%d rows=%lld candidates=%lld direction=%lld aligned=%lld out=%lld height_rows=%lld bin=(%d %d %d) "
                    "inliers=(%lld %lld %lld) sums=%016llx plane=%016llx pose=%016llx dir_hist=%016llx height_hist=%016llx\n", r.status, r.rounds,
                    (long long)r.rows_used, (long long)r.candidates, (long long)r.direction_rows, (long long)r.aligned, (long long)r.height_out_of_range,
                    (long long)r.height_rows, r.dir_bin[0], r.dir_bin[1], r.height_bin, (long long)r.inliers[0], (long long)r.inliers[1],
                    (long long)r.inliers[2], (unsigned long long)fnv1a(r.sums, sizeof(r.sums)), (unsigned long long)fnv1a(r.normal, 16),
                    (unsigned long long)fnv1a(r.pose, sizeof(r.pose)), (unsigned long long)fnv1a(fit.dir_hist.data(), 4 * fit.dir_hist.size()),
                    (unsigned long long)fnv1a(fit.height_hist.data(), 4 * fit.height_hist.size()));
        const ssf_navgrid_stats& s = grid.stats;
        std::printf("floorgrid %dx%d rows=%lld in_grid=%lld free=%lld occupied=%lld unknown=%lld state=%016llx dist2=%016llx\n", grid.width, grid.height,
                    (long long)s.rows_used, (long long)s.samples_in_grid, (long long)s.cells_free, (long long)s.cells_occupied, (long long)s.cells_unknown,
                    (unsigned long long)fnv1a(grid.state.data(), grid.state.size()), (unsigned long long)fnv1a(grid.dist2.data(), 4 * grid.dist2.size()));
        if (!fit.ok()) { std::printf("no floor\n"); return 2; }
        if (std::memcmp(s.pose, r.pose, sizeof(r.pose)) != 0) { std::printf("the grid was not built in the fitted frame\n"); return 2; }
        if (grid.width != 64 || grid.height != 48 || fit.dir_hist.size() != 31u * 31u || fit.height_hist.size() != 2048u) { std::printf("sizes\n"); return 2; }
        // applyTo on its own, without histograms
        FloorParams f2 = f;
        f2.want_histograms = false;
        FloorFit again;
        a.fitFloor(f2, again);
        NavGridParams g2;
        again.applyTo(g2);
        if (g2.pose != &again.pose || g2.z_min != -0.3f || g2.floor_max != 0.1f || g2.z_max != 1.0f || g2.width != 64 || g2.height != 48 || !again.dir_hist.empty() ||
            std::memcmp(&again.fit, &fit.fit, sizeof(fit.fit)) != 0) { std::printf("applyTo\n"); return 2; }
        std::printf("apply ok\n");
    } catch (const std::exception& e) { std::printf("exception %s\n", e.what()); return 1; }
    return 0;
}
