// The raw-frame surface of include/ssf.hpp (setInputFormat, processFrame with uint16 depth -- pointer and cv::Mat CV_16UC1
// overloads -- and processSequence with uint16 depth) against the cv::Mat test double that knows CV_16UC1.  Frames: BGR8 colour
// + uint16 depth counts.  Prints the pose bits of every frame, which tests/test_input_formats_gpu.py compares with the float
// RGB path of the Python binding.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "cv_double_u16.hpp"
#include "ssf.hpp"

static void print_pose(int k, const ssf_frame_result& r) {
    std::printf("frame%d", k);
    for (int i = 0; i < 12; i++) { unsigned int u; std::memcpy(&u, &r.pose[i], 4); std::printf(" %08x", u); }
    std::printf(" n=%d\n", r.n_model);
}

int main(int argc, char** argv) {
    if (argc < 10) return 2;
    const int W = std::atoi(argv[1]), H = std::atoi(argv[2]), n = std::atoi(argv[3]);
    std::FILE* f = std::fopen(argv[4], "rb");
    if (!f) return 3;
    const double scale = std::atof(argv[9]);
    using namespace supersurfel_fusion;
    CamParam cam; cam.width = W; cam.height = H;
    cam.fx = (float)std::atof(argv[5]); cam.fy = (float)std::atof(argv[6]); cam.cx = (float)std::atof(argv[7]); cam.cy = (float)std::atof(argv[8]);
    const size_t P = (size_t)W * H;
    std::vector<std::vector<uint8_t>> rgb(n, std::vector<uint8_t>(3 * P));
    std::vector<std::vector<uint16_t>> depth(n, std::vector<uint16_t>(P));
    for (int k = 0; k < n; k++)
        if (std::fread(rgb[k].data(), 1, 3 * P, f) != 3 * P || std::fread(depth[k].data(), 2, P, f) != P) return 4;
    std::fclose(f);
    try {
        SupersurfelFusion a, b;
        a.setDepthPrefilter(false); b.setDepthPrefilter(false); b.setPipeline(2, 4);
        a.initialize(cam, 16, 10.f, 1000.f, 1000.f, 1e8f);
        b.initialize(cam, 16, 10.f, 1000.f, 1000.f, 1e8f);
        a.setInputFormat(SSF_COLOR_BGR8, SSF_DEPTH_U16_SCALED, scale);
        b.setInputFormat(SSF_COLOR_BGR8, SSF_DEPTH_U16_SCALED, scale);
        try { a.processFrame(rgb[0].data(), reinterpret_cast<const float*>(depth[0].data())); std::printf("float_refused 0\n"); }
        catch (const std::logic_error&) { std::printf("float_refused 1\n"); }
        for (int k = 0; k < n; k++) {
            if (k % 2 == 0) {
                cv::Mat c(H, W, CV_8UC3), d(H, W, CV_16UC1);
                std::memcpy(c.ptr<uint8_t>(), rgb[k].data(), 3 * P); std::memcpy(d.ptr<uint16_t>(), depth[k].data(), 2 * P);
                if (k == 2) d.pretendStrided();
                a.processFrame(c, d);
            } else {
                a.processFrame(rgb[k].data(), depth[k].data());
            }
            print_pose(k, a.lastResult());
        }
        std::vector<const uint8_t*> rp; std::vector<const uint16_t*> dp;
        for (int k = 0; k < n; k++) { rp.push_back(rgb[k].data()); dp.push_back(depth[k].data()); }
        const std::vector<ssf_frame_result> seq = b.processSequence(rp, dp);
        for (int k = 0; k < n; k++) print_pose(100 + k, seq[k]);
    } catch (const std::exception& e) { std::printf("exception %s\n", e.what()); return 1; }
    return 0;
}
