// The motion surface of include/ssf.hpp (detectMotion on pointers, a std::vector and a cv::Mat; processFrame with MotionParams;
// getMotionMask) against the cv::Mat test double that knows CV_8UC1.  Synthetic frames: a tilted plane, then the same plane with
// a box half a metre in front of it.  Prints the masked pixels of every call.
#include <cstdio>
#include <cstring>
#include <vector>
#include "cv_double_mask.hpp"
#include "ssf.hpp"

int main() {
    using namespace supersurfel_fusion;
    const int W = 160, H = 128;
    const size_t P = (size_t)W * H;
    CamParam cam; cam.width = W; cam.height = H; cam.fx = 150.f; cam.fy = 150.f; cam.cx = 79.5f; cam.cy = 63.5f;
    std::vector<uint8_t> rgb(3 * P);
    std::vector<float> depth(P), boxed(P);
    for (size_t i = 0; i < P; i++) {
        const int x = (int)(i % W), y = (int)(i / W);
        rgb[3 * i] = (uint8_t)(x * 255 / W); rgb[3 * i + 1] = (uint8_t)(y * 255 / H); rgb[3 * i + 2] = (uint8_t)((x ^ y) & 255);
        depth[i] = 1.5f + 0.002f * (float)x;
        boxed[i] = (x >= 60 && x < 100 && y >= 40 && y < 80) ? 1.0f : depth[i];
    }
    try {
        SupersurfelFusion a;
        a.setDepthPrefilter(false);
        a.initialize(cam, 16, 10.f, 1000.f, 1000.f, 1e8f);
        a.processFrame(rgb.data(), depth.data(), MotionParams());
        std::printf("frame0 masked=%lld\n", (long long)a.getMotionMask().stats.pixels_masked);
        MotionMask m = a.detectMotion(boxed.data());
        std::printf("detect masked=%lld seeds=%lld\n", (long long)m.stats.pixels_masked, (long long)m.stats.n_seed);
        MotionParams mp; mp.min_seeds = 4; mp.front_abs = 0.1f;
        m = a.detectMotion(boxed, mp);
        std::printf("vector masked=%lld\n", (long long)m.stats.pixels_masked);
        cv::Mat d(H, W, CV_32FC1);
        std::memcpy(d.ptr<float>(), boxed.data(), 4 * P);
        cv::Mat mm = a.detectMotion(d);
        size_t hit = 0;
        for (size_t i = 0; i < P; i++) hit += mm.ptr<uint8_t>()[i];
        std::printf("mat masked=%zu type=%d\n", hit, mm.type());
        a.processFrame(rgb.data(), boxed.data(), mp);
        std::printf("frame1 masked=%lld n=%d\n", (long long)a.getMotionMask().stats.pixels_masked, a.lastResult().n_model);
        cv::Mat c(H, W, CV_8UC3);
        std::memcpy(c.ptr<uint8_t>(), rgb.data(), 3 * P);
        a.processFrame(c, d, MotionParams());
        std::printf("frame2 masked=%lld\n", (long long)a.getMotionMask().stats.pixels_masked);
    } catch (const std::exception& e) { std::printf("exception %s\n", e.what()); return 1; }
    return 0;
}
