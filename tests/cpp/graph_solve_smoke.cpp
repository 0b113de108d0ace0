// The graph-optimisation surface of include/ssf.hpp (getGraphEdges, optimiseGraphSparse, getGraphTransforms, applyGraphToModel)
// on frames read from a file: graph_solve_smoke W H n frames.bin fx fy cx cy.  The constraints are the node positions themselves:
// the earlier half pinned, the later half shifted; solved twice, once through ssf_graph_solve itself with no result record.
// Prints sizes, the result record and FNV-1a hashes; the GPU test repeats the calls through the Python binding and compares
// the lines.
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
    if (argc < 9) { std::printf("usage: graph_solve_smoke W H n frames.bin fx fy cx cy\n"); return 2; }
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
        std::vector<int32_t> t0;
        const std::vector<float3> g = a.getNodesPositions(&t0, nullptr);
        const std::vector<int32_t> e = a.getGraphEdges();
        std::printf("graph nodes=%d edges %016llx\n", m, fnv(e.data(), 4 * e.size()));
        std::vector<float3> dst = g;
        for (int k = m / 2; k < m; k++) { dst[(size_t)k].x += 0.01f; dst[(size_t)k].z -= 0.02f; }
        ssf_graph_solve_params p = SupersurfelFusion::defaultGraphSolveParams();
        p.max_outer = 3;
        // first the C entry point without a result record, the stop rule read after every iteration; its line is printed last
        ssf_graph_solve_params p1 = p;
        p1.inner_check = 1;
        if (ssf_graph_solve(a.handle(), &p1, reinterpret_cast<const float*>(g.data()), t0.data(), reinterpret_cast<const float*>(dst.data()),
                            m, nullptr) != SSF_OK) { std::printf("ssf_graph_solve without a result record failed\n"); return 1; }
        std::vector<Mat33> R1; std::vector<float3> t1;
        a.getGraphTransforms(R1, t1);
        const unsigned long long every_1 = fnv(t1.data(), 12 * t1.size(), fnv(R1.data(), 36 * R1.size()));
        const ssf_graph_solve_result r = a.optimiseGraphSparse(g, t0, dst, p);
        std::printf("solve outer=%d inner=%d,%d,%d end=%d energy %016llx\n", r.outer, r.inner[0], r.inner[1], r.inner[2], r.inner_end,
                    fnv(&r.e_before, 5 * sizeof(double)));
        std::vector<Mat33> R; std::vector<float3> t;
        a.getGraphTransforms(R, t);
        std::printf("transforms %016llx\n", fnv(t.data(), 12 * t.size(), fnv(R.data(), 36 * R.size())));
        a.applyGraphToModel();
        const HostSupersurfels model = a.getModelHost();
        std::printf("model %d %016llx\n", model.size, fnv(model.positions.data(), 12 * (size_t)model.size));
        bool stale = false;
        try { a.getGraphTransforms(R, t); } catch (const std::runtime_error&) { stale = true; }
        std::printf("stale_after_apply %d\n", stale ? 1 : 0);
        std::printf("no_record_check_every_1 transforms %016llx\n", every_1);
    } catch (const std::exception& e) { std::printf("exception %s\n", e.what()); return 1; }
    return 0;
}
