// The query surface of include/ssf.hpp (countModel, queryModel, extractLocalPointCloud).  Synthetic frames: a tilted plane seen by a
// camera that steps sideways.  Prints the row count of a radius-1.5 m local cloud of the 6-frame map and the FNV-1a checksum of
// its positions' bytes (tests/test_query_gpu.py compares both with the Python query of the same map).
#include <cstdio>
#include <cstring>
#include <vector>
#include "ssf.hpp"

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
        std::vector<float3> pos, col, nrm;
        a.extractLocalPointCloud(1.5f, pos, col, nrm);
        uint64_t fnv = 1469598103934665603ull;
        const unsigned char* b = reinterpret_cast<const unsigned char*>(pos.data());
        for (size_t i = 0; i < 12 * pos.size(); i++) { fnv ^= b[i]; fnv *= 1099511628211ull; }
        std::printf("local_cloud rows=%zu fnv=%016llx colors=%zu normals=%zu\n", pos.size(), (unsigned long long)fnv, col.size(), nrm.size());
        QueryParams q;
        q.region = SSF_REGION_SPHERE; q.radius = 1.5f;
        const ssf_query_stats s = a.countModel(q);
        std::printf("count scanned=%lld selected=%lld visible=%lld model=%d\n", (long long)s.n_scanned, (long long)s.n_selected,
                    (long long)s.n_selected_visible, a.getnbSupersurfels());
        QueryResult r;
        a.queryModel(q, r);
        std::printf("query rows=%zu index=%zu first=%d\n", (size_t)r.rows.size, r.index.size(), r.index.empty() ? -1 : r.index[0]);
        if ((size_t)r.rows.size != pos.size() || (size_t)s.n_selected != pos.size()) { std::printf("mismatch\n"); return 2; }
        if (!pos.empty() && std::memcmp(r.rows.positions.data(), pos.data(), 12 * pos.size()) != 0) { std::printf("positions differ\n"); return 2; }
    } catch (const std::exception& e) { std::printf("exception %s\n", e.what()); return 1; }
    return 0;
}
