// The deformation-graph surface of include/ssf.hpp (buildDeformationGraph, getNodesPositions, getGraphBinding, bindPoints,
// applyGraph) on frames read from a file: graph_smoke W H n frames.bin fx fy cx cy.  Prints the sizes and an FNV-1a hash of the
// node table, the binding, the binding of the nodes as caller points and the deformed model's positions; the GPU test repeats
// the calls through the Python binding and compares the lines.
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
    if (argc < 9) { std::printf("usage: graph_smoke W H n frames.bin fx fy cx cy\n"); return 2; }
    const int W = std::atoi(argv[1]), H = std::atoi(argv[2]), n = std::atoi(argv[3]);
    const size_t P = (size_t)W * H;
    CamParam cam; cam.width = W; cam.height = H;
    cam.fx = (float)std::atof(argv[5]); cam.fy = (float)std::atof(argv[6]); cam.cx = (float)std::atof(argv[7]); cam.cy = (float)std::atof(argv[8]);
    std::FILE* f = std::fopen(argv[4], "rb");
    if (!f) { std::printf("cannot open %s\n", argv[4]); return 2; }
    try {
        SupersurfelFusion a;
        a.initialize(cam, 16, 10.f, 1000.f, 1000.f, 1e8f);
        std::vector<uint8_t> rgb(3 * P);
        std::vector<float> depth(P);
        for (int k = 0; k < n; k++) {
            if (std::fread(rgb.data(), 1, 3 * P, f) != 3 * P || std::fread(depth.data(), 4, P, f) != P) { std::printf("short read\n"); return 2; }
            a.processFrame(rgb.data(), depth.data());
        }
        std::fclose(f);
        const int m = a.buildDeformationGraph(8, 5, 0.f);
        std::vector<int32_t> t0, rows;
        const std::vector<float3> g = a.getNodesPositions(&t0, &rows);
        std::printf("graph nodes=%d rows=%d\n", m, a.getnbSupersurfels());
        std::printf("nodes %016llx\n", fnv(rows.data(), 4 * rows.size(), fnv(t0.data(), 4 * t0.size(), fnv(g.data(), 12 * g.size()))));
        const GraphBinding b = a.getGraphBinding();
        std::printf("binding %zu %016llx\n", b.size(), fnv(b.idx4.data(), 4 * b.idx4.size(), fnv(b.weights4.data(), 4 * b.weights4.size())));
        const GraphBinding c = a.bindPoints(g, t0);
        std::printf("points %zu %016llx\n", c.size(), fnv(c.idx4.data(), 4 * c.idx4.size(), fnv(c.weights4.data(), 4 * c.weights4.size())));
        std::vector<Mat33> R((size_t)m);
        std::vector<float3> t((size_t)m);
        for (int k = 0; k < m; k++) {
            Mat33 I = {{{1.f, 0.f, 0.f}, {0.f, 1.f, 0.f}, {0.f, 0.f, 1.f}}};
            R[(size_t)k] = I;
            t[(size_t)k].x = 0.001f * (float)(k % 5); t[(size_t)k].y = 0.f; t[(size_t)k].z = -0.002f * (float)(k % 3);
        }
        a.applyGraph(R, t);
        const HostSupersurfels model = a.getModelHost();
        std::printf("model %d %016llx\n", model.size, fnv(model.positions.data(), 12 * (size_t)model.size));
        bool stale = false;
        try { a.getGraphBinding(); } catch (const std::runtime_error&) { stale = true; }
        std::printf("stale_after_apply %d\n", stale ? 1 : 0);
    } catch (const std::exception& e) { std::printf("exception %s\n", e.what()); return 1; }
    return 0;
}
