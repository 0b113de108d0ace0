// The keyframe surface of include/ssf.hpp (configureKeyframes, considerKeyframe, queryKeyframes, getKeyframe, putKeyframe,
// alignKeyframe, ...) on frames read from a file: keyframes_smoke W H n frames.bin fx fy cx cy.  After every frame one line of the
// consider record; at the end an FNV-1a hash of the fern table, of keyframe 0 (rows, codes) and the verdict of aligning it against
// the last frame.  The GPU test repeats the calls through the Python binding and compares the lines.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "ssf.hpp"

static unsigned long long fnv(const void* p, size_t bytes, unsigned long long h = 1469598103934665603ull) {
    const unsigned char* b = static_cast<const unsigned char*>(p);
    for (size_t i = 0; i < bytes; i++) { h ^= b[i]; h *= 1099511628211ull; }
    return h;
}

int main(int argc, char** argv) {
    using namespace supersurfel_fusion;
    if (argc < 9) { std::printf("usage: keyframes_smoke W H n frames.bin fx fy cx cy\n"); return 2; }
    const int W = std::atoi(argv[1]), H = std::atoi(argv[2]), n = std::atoi(argv[3]);
    const size_t P = (size_t)W * H;
    CamParam cam; cam.width = W; cam.height = H;
    cam.fx = (float)std::atof(argv[5]); cam.fy = (float)std::atof(argv[6]); cam.cx = (float)std::atof(argv[7]); cam.cy = (float)std::atof(argv[8]);
    std::FILE* f = std::fopen(argv[4], "rb");
    if (!f) { std::printf("cannot open %s\n", argv[4]); return 2; }
    try {
        SupersurfelFusion a;
        a.initialize(cam, 16, 10.f, 1000.f, 1000.f, 1e8f);
        ssf_keyframes_params p = SupersurfelFusion::defaultKeyframesParams();
        p.min_gap = 2; p.max_keyframes = 16;
        a.configureKeyframes(p);
        const std::vector<ssf_fern> ferns = a.getFerns();
        std::printf("ferns %zu %016llx\n", ferns.size(), fnv(ferns.data(), sizeof(ssf_fern) * ferns.size()));
        std::vector<uint8_t> rgb(3 * P);
        std::vector<float> depth(P);
        for (int k = 0; k < n; k++) {
            if (std::fread(rgb.data(), 1, 3 * P, f) != 3 * P || std::fread(depth.data(), 4, P, f) != P) { std::printf("short read\n"); return 2; }
            a.processFrame(rgb.data(), depth.data());
            const ssf_keyframe_result r = a.considerKeyframe();
            std::printf("frame %d added=%d id=%d full=%d min=%d n=%d cand=%d", k, r.added, r.id, r.full, r.min_diff_all, r.n_keyframes, r.n_candidates);
            for (int j = 0; j < r.n_candidates; j++) std::printf(" (%d %d %d %d)", r.candidates[j].id, r.candidates[j].diff, r.candidates[j].stamp, r.candidates[j].loop);
            std::printf("\n");
        }
        std::fclose(f);
        const std::vector<uint8_t> codes = a.encodeKeyframe();
        const ssf_keyframe_result q = a.queryKeyframes(codes, 1000, 0, 3);
        std::printf("query min=%d cand=%d first=%d\n", q.min_diff_all, q.n_candidates, q.n_candidates ? q.candidates[0].id : -1);
        Keyframe kf = a.getKeyframe(0);
        std::printf("keyframe0 rows=%d stamp=%d %016llx\n", kf.rows.size, kf.stamp,
                    fnv(kf.codes.data(), kf.codes.size(), fnv(kf.rows.orientations.data(), 36 * (size_t)kf.rows.size,
                                                              fnv(kf.rows.positions.data(), 12 * (size_t)kf.rows.size))));
        const KeyframeAlignment al = a.alignKeyframe(0);
        std::printf("align valid=%d iters=%d pairs=%d %016llx\n", al.valid ? 1 : 0, al.iters, al.pairs, fnv(al.rel_pose, sizeof(al.rel_pose)));
        kf.stamp = 77;
        const int id = a.putKeyframe(kf);
        a.setKeyframePose(id, kf.pose);
        std::printf("put id=%d n=%d\n", id, a.nbKeyframes());
        a.clearKeyframes();
        bool refused = false;
        try { a.considerKeyframe(); } catch (const std::runtime_error&) { refused = true; }
        std::printf("refused_after_clear %d\n", refused ? 1 : 0);
    } catch (const std::exception& e) { std::printf("exception %s\n", e.what()); return 1; }
    return 0;
}
