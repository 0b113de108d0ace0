// The render surface of include/ssf.hpp (renderModel into a RenderedView with RenderOptions, and the cv::Mat overload: CV_8UC3
// colour, CV_32FC1 depth) against the cv::Mat test double.  Synthetic frames: a tilted plane.  Prints the filled pixels of every
// render.
#include <cstdio>
#include <vector>
#include "cv_double.hpp"
#include "ssf.hpp"

int main() {
    using namespace supersurfel_fusion;
    const int W = 160, H = 128;
    const size_t P = (size_t)W * H;
    CamParam cam; cam.width = W; cam.height = H; cam.fx = 150.f; cam.fy = 150.f; cam.cx = 79.5f; cam.cy = 63.5f;
    std::vector<uint8_t> rgb(3 * P);
    std::vector<float> depth(P);
    for (size_t i = 0; i < P; i++) {
        const int x = (int)(i % W), y = (int)(i / W);
        rgb[3 * i] = (uint8_t)(x * 255 / W); rgb[3 * i + 1] = (uint8_t)(y * 255 / H); rgb[3 * i + 2] = (uint8_t)((x ^ y) & 255);
        depth[i] = 1.0f + 0.002f * (float)x;
    }
    try {
        SupersurfelFusion a;
        a.setDepthPrefilter(false);
        a.initialize(cam, 16, 10.f, 1000.f, 1000.f, 1e8f);
        a.processFrame(rgb.data(), depth.data());
        RenderedView view;
        a.renderModel(a.getPose(), view);
        std::printf("render %dx%d filled=%lld rows=%lld\n", view.width, view.height, (long long)view.stats.pixels_filled,
                    (long long)view.stats.rows_shown);
        RenderOptions o; o.width = 64; o.height = 48; o.fx = 60.f; o.fy = 60.f; o.cx = 31.5f; o.cy = 23.5f; o.visible_only = true;
        a.renderModel(a.getPose(), view, o);
        std::printf("small filled=%lld\n", (long long)view.stats.pixels_filled);
        cv::Mat c, d;
        a.renderModel(a.getPose(), c, d);
        size_t hit = 0;
        for (size_t i = 0; i < P; i++) hit += d.ptr<float>()[i] > 0.f ? 1 : 0;
        std::printf("mat filled=%zu type=%d\n", hit, c.type());
    } catch (const std::exception& e) { std::printf("exception %s\n", e.what()); return 1; }
    return 0;
}
