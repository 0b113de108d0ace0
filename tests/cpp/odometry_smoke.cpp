// The odometry surface of include/ssf.hpp (setOdometryReference, estimateOdometry, trackOdometry, processFrame with
// OdometryParams -- alone and with MotionParams --, getOdometry).  Synthetic frames: a textured tilted plane, shifted by one pixel
// per frame.  Prints the verdict and the translation of every estimate.
#include <cstdio>
#include <vector>
#include "ssf.hpp"

int main() {
    using namespace supersurfel_fusion;
    const int W = 160, H = 128, N = 4;
    const size_t P = (size_t)W * H;
    CamParam cam; cam.width = W; cam.height = H; cam.fx = 150.f; cam.fy = 150.f; cam.cx = 79.5f; cam.cy = 63.5f;
    std::vector<std::vector<uint8_t> > rgb(N, std::vector<uint8_t>(3 * P));
    std::vector<std::vector<float> > depth(N, std::vector<float>(P));
    for (int k = 0; k < N; k++)
        for (size_t i = 0; i < P; i++) {
            const int x = (int)(i % W) + k, y = (int)(i / W);
            const uint8_t v = (uint8_t)(128 + 60 * (((x / 8) + (y / 8)) & 1) + (x * 5 + y * 3) % 40);
            rgb[k][3 * i] = v; rgb[k][3 * i + 1] = (uint8_t)(v / 2 + 40); rgb[k][3 * i + 2] = (uint8_t)(255 - v);
            depth[k][i] = 1.5f + 0.002f * (float)x;
        }
    try {
        SupersurfelFusion a;
        a.setDepthPrefilter(false);
        a.initialize(cam, 16, 10.f, 1000.f, 1000.f, 1e8f);
        a.setOdometryReference(rgb[0].data(), depth[0].data());
        OdometryParams op; op.levels = 3; op.iters[0] = 3;
        OdometryEstimate e = a.estimateOdometry(rgb[1].data(), depth[1].data(), op);
        std::printf("estimate valid=%d reason=%d tx=%.4f pixels=%lld\n", e.result.valid, e.result.reason, e.rel[9], (long long)e.result.pixels);
        e = a.estimateOdometry(rgb[1].data(), depth[1].data(), op, e.rel);
        std::printf("estimate(init) valid=%d iters0=%d\n", e.result.valid, e.result.iters[0]);
        e = a.trackOdometry(rgb[1].data(), depth[1].data(), op);
        std::printf("track valid=%d reason=%d has_prior=%d tx=%.4f\n", e.result.valid, e.result.reason, (int)e.has_prior, e.prior[9]);
        SupersurfelFusion b;
        b.setDepthPrefilter(false);
        b.initialize(cam, 16, 10.f, 1000.f, 1000.f, 1e8f);
        for (int k = 0; k < N; k++) {
            if (k < 2) b.processFrame(rgb[k].data(), depth[k].data(), op);
            else b.processFrame(rgb[k].data(), depth[k].data(), op, MotionParams());
            std::printf("frame%d n=%d", k, b.lastResult().n_model);
            if (k > 0) { e = b.getOdometry(); std::printf(" valid=%d has_prior=%d", e.result.valid, (int)e.has_prior); }
            std::printf("\n");
        }
    } catch (const std::exception& ex) { std::printf("exception %s\n", ex.what()); return 1; }
    return 0;
}
