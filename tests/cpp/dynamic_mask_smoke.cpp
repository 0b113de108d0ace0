// The pixel-mask surface of include/ssf.hpp (processFrame with a PixelMask, float and uint16 depth, the cv::Mat overload with a
// CV_8UC1 mask, getDynamicSuperpixels) against the cv::Mat test double that knows CV_8UC1.  Synthetic frames: a tilted plane,
// the left half of the image masked.  Prints the number of dynamic superpixels and the model size of every frame.
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
    std::vector<uint8_t> rgb(3 * P), mask(P, 0);
    std::vector<float> depth(P);
    std::vector<uint16_t> d16(P);
    for (size_t i = 0; i < P; i++) {
        const int x = (int)(i % W), y = (int)(i / W);
        rgb[3 * i] = (uint8_t)(x * 255 / W); rgb[3 * i + 1] = (uint8_t)(y * 255 / H); rgb[3 * i + 2] = (uint8_t)((x ^ y) & 255);
        depth[i] = 1.0f + 0.002f * (float)x; d16[i] = (uint16_t)(depth[i] * 5000.f);
        mask[i] = x < W / 2 ? 255 : 0;
    }
    try {
        SupersurfelFusion a;
        a.setDepthPrefilter(false);
        a.initialize(cam, 16, 10.f, 1000.f, 1000.f, 1e8f);
        a.processFrame(rgb.data(), depth.data(), PixelMask(mask.data()));
        std::vector<uint8_t> dyn = a.getDynamicSuperpixels();
        int n = 0;
        for (uint8_t v : dyn) n += v;
        std::printf("frame0 dynamic=%d n=%d\n", n, a.lastResult().n_model);
        a.processFrame(rgb.data(), depth.data(), PixelMask(nullptr));
        std::printf("frame1 n=%d\n", a.lastResult().n_model);
        a.setInputFormat(SSF_COLOR_RGB8, SSF_DEPTH_U16_SCALED, 0.0002);
        cv::Mat c(H, W, CV_8UC3), d(H, W, CV_16UC1), m(H, W, CV_8UC1);
        std::memcpy(c.ptr<uint8_t>(), rgb.data(), 3 * P); std::memcpy(d.ptr<uint16_t>(), d16.data(), 2 * P);
        std::memcpy(m.ptr<uint8_t>(), mask.data(), P);
        a.processFrame(c, d, m);
        std::printf("frame2 n=%d\n", a.lastResult().n_model);
        a.processFrame(rgb.data(), d16.data(), PixelMask(mask.data()), nullptr);
        std::printf("frame3 n=%d\n", a.lastResult().n_model);
    } catch (const std::exception& e) { std::printf("exception %s\n", e.what()); return 1; }
    return 0;
}
