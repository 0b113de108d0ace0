// The ray-cast surface of include/ssf.hpp (RaycastParams, castRays, laserScan).  The frames of navgrid_smoke.cpp: a tilted plane
// seen by a camera that steps sideways.  Casts a 16 x 13 bundle of rays from the tracked pose and prints the counts and the FNV-1a
// checksums of the outputs (tests/test_raycast_gpu.py compares them with the Python call on the same map), then fills the
// LaserScan double from a fan that sees the plane in front and nothing behind.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include "ssf.hpp"
#include "sensor_msgs_double.hpp"

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
        // a 16 x 13 bundle through every tenth pixel, directions (qx, qy, 1) (not unit: t is the depth along the camera's axis)
        std::vector<float> rays;
        for (int v = 4; v < H; v += 10)
            for (int u = 5; u < W; u += 10) {
                const float r6[6] = {0.f, 0.f, 0.f, ((float)u - cam.cx) / cam.fx, ((float)v - cam.cy) / cam.fy, 1.f};
                rays.insert(rays.end(), r6, r6 + 6);
            }
        RaycastParams q;
        q.t_min = 0.25f; q.t_max = 4.0f;
        RaycastResult res;
        a.castRays(rays, q, res);
        const ssf_raycast_stats& s = res.stats;
        std::printf("raycast rays=%lld hit=%lld invalid=%lld rows=%lld oversize=%lld t=%016llx index=%016llx point=%016llx normal=%016llx color=%016llx\n",
                    (long long)s.rays, (long long)s.rays_hit, (long long)s.rays_invalid, (long long)s.rows_indexed, (long long)s.rows_oversize,
                    (unsigned long long)fnv1a(res.t.data(), 4 * res.t.size()), (unsigned long long)fnv1a(res.index.data(), 4 * res.index.size()),
                    (unsigned long long)fnv1a(res.point.data(), 12 * res.point.size()), (unsigned long long)fnv1a(res.normal.data(), 12 * res.normal.size()),
                    (unsigned long long)fnv1a(res.color.data(), 12 * res.color.size()));
        if (res.t.size() != rays.size() / 6 || res.point.size() != res.t.size() || s.rays != (long long)res.t.size()) { std::printf("sizes\n"); return 2; }
        if (s.rays_hit <= 0 || s.rays_hit >= s.rays + 1) { std::printf("no ray hit\n"); return 2; }
        const std::vector<float> t_only = a.castRays(rays, q);
        if (t_only.size() != res.t.size() || std::memcmp(t_only.data(), res.t.data(), 4 * t_only.size()) != 0) { std::printf("t alone differs\n"); return 2; }
        // a fan of 9 beams over the full circle in the camera's x-z plane: laser x = camera z (forward), laser y = camera x, laser z = camera y
        const Transform3 cam_pose = a.getPose();
        float c[12]; transform3_to_rt(cam_pose, c);
        const float l[12] = {c[2], c[0], c[1], c[5], c[3], c[4], c[8], c[6], c[7], c[9], c[10], c[11]};
        const Transform3 laser = transform3_from_rt(l);
        sensor_msgs::LaserScan scan;
        scan.intensities.push_back(1.f);
        a.laserScan(&laser, -3.14159265f, 3.14159265f, 9, 0.25f, 4.0f, scan);
        int n_inf = 0, n_hit = 0;
        for (size_t i = 0; i < scan.ranges.size(); i++) {
            if (std::isinf(scan.ranges[i]) && scan.ranges[i] > 0.f) n_inf++;
            else if (scan.ranges[i] >= scan.range_min && scan.ranges[i] <= scan.range_max) n_hit++;
        }
        std::printf("scan beams=%zu hit=%d inf=%d inc=%.6f min=%.2f max=%.2f forward=%.3f intensities=%zu\n", scan.ranges.size(), n_hit, n_inf,
                    (double)scan.angle_increment, (double)scan.range_min, (double)scan.range_max, (double)scan.ranges[4], scan.intensities.size());
        if (n_hit + n_inf != 9 || n_hit < 1 || n_inf < 1 || std::isinf(scan.ranges[4])) { std::printf("the scan is wrong\n"); return 2; }
    } catch (const std::exception& e) { std::printf("exception %s\n", e.what()); return 1; }
    return 0;
}
