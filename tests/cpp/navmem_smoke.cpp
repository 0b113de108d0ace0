// The live layer with memory of include/ssf.hpp (LiveMemory and the overlayDepthFrame overloads that take one).  The depth image, the mask
// and the grid are navlive_smoke.cpp's integer hashes, every float of them exact, so that tests/test_navmem_gpu.py makes the same arrays
// and compares counts and FNV-1a checksums with the Python calls.  Three calls: float depth in a std::vector at tick 1, the same as
// cv::Mat (a double) with a CV_8UC1 mask under mask_mode 2 at tick 4 into the same memory with ages, and uint16 counts after
// setInputFormat into a memory of 5 slices.  The result goes through fillOccupancyGrid and planOnGrid as it is.
#include <cstdio>
#include <cstring>
#include <vector>
#include "cv_double_mask.hpp"
#include "ssf.hpp"
#include "nav_msgs_double.hpp"

static uint64_t fnv1a(const void* p, size_t n, uint64_t h = 1469598103934665603ull) {
    const unsigned char* b = static_cast<const unsigned char*>(p);
    for (size_t i = 0; i < n; i++) { h ^= b[i]; h *= 1099511628211ull; }
    return h;
}
static void report(const char* what, const supersurfel_fusion::LiveNavGrid& g, const supersurfel_fusion::LiveMemory& m) {
    const ssf_navmem_stats& s = m.stats;
    std::printf("%s tick=%u valid=%lld points=%lld samples=%lld marked=%lld cleared=%lld expired=%lld remembered=%lld opened=%lld state=%016llx "
                "dist2=%016llx hits=%016llx marks=%016llx mark_tick=%016llx seen_tick=%016llx seen_bits=%016llx\n", what, (unsigned)m.tick,
                (long long)s.pixels_valid, (long long)s.points_in_band, (long long)s.ray_samples, (long long)s.cells_marked, (long long)s.cells_cleared,
                (long long)s.cells_expired, (long long)s.cells_remembered, (long long)s.cells_opened,
                (unsigned long long)fnv1a(g.state.data(), g.state.size()), (unsigned long long)fnv1a(g.dist2.data(), 4 * g.dist2.size()),
                (unsigned long long)fnv1a(g.live_hits.data(), 4 * g.live_hits.size()), (unsigned long long)fnv1a(m.marks.data(), 4 * m.marks.size()),
                (unsigned long long)fnv1a(m.mark_tick.data(), 4 * m.mark_tick.size()), (unsigned long long)fnv1a(m.seen_tick.data(), 4 * m.seen_tick.size()),
                (unsigned long long)fnv1a(m.seen_bits.data(), 4 * m.seen_bits.size()));
}

int main() {
    using namespace supersurfel_fusion;
    CamParam cam; cam.width = 160; cam.height = 128; cam.fx = 150.f; cam.fy = 150.f; cam.cx = 79.5f; cam.cy = 63.5f;
    const size_t npix = (size_t)cam.width * cam.height;
    try {
        SupersurfelFusion a;
        a.setDepthPrefilter(false);
        a.initialize(cam, 16, 10.f, 1000.f, 1000.f, 1e8f);
        NavGrid g;
        g.width = 48; g.height = 40; g.res = 0.05f;
        const size_t P = (size_t)g.width * g.height;
        g.state.resize(P);
        for (size_t p = 0; p < P; p++) {
            const uint32_t u = ((uint32_t)p * 2654435761u) >> 16;
            g.state[p] = (int8_t)(u % 100u < 5u ? 100 : (u % 100u < 75u ? -1 : 0));
        }
        const float rt[12] = {1.f, 0.f, 0.f, 0.f, 0.f, -1.f, 0.f, 1.f, 0.f, -1.2f, 0.f, -0.2f};
        g.stats = ssf_navgrid_stats();
        std::memcpy(g.stats.pose, rt, sizeof(rt));
        std::vector<float> depth(npix);
        std::vector<uint16_t> counts(npix);
        std::vector<uint8_t> mask(npix), none;
        for (size_t p = 0; p < npix; p++) {
            const uint32_t k = (((uint32_t)p * 2654435761u) >> 12) % 1024u;
            depth[p] = p % 97u == 0u ? 0.f : 0.5f + (float)k * 0.0009765625f;
            counts[p] = p % 97u == 0u ? (uint16_t)0 : (uint16_t)(500u + k);
            mask[p] = (uint8_t)(p % 3u == 0u ? 255 : 0);
        }
        LiveParams q;
        q.max_dist_cells = 8;
        LiveMemory mem;
        LiveNavGrid live;
        a.overlayDepthFrame(g, q, depth, none, mem, 1u, live);
        report("navmem", live, mem);
        if (live.state.size() != P || live.dist2.size() != P || live.live_hits.size() != P || mem.marks.size() != P || mem.seen_bits.size() != P ||
            mem.width != 48 || mem.tick != 1u) { std::printf("sizes\n"); return 2; }
        nav_msgs::OccupancyGrid msg;
        SupersurfelFusion::fillOccupancyGrid(live, msg);
        bool ok = msg.data.size() == P && msg.info.width == 48u && msg.info.height == 40u && msg.info.origin.position.x == (double)-1.2f &&
                  std::memcmp(msg.data.data(), live.state.data(), P) == 0;
        PlanParams pq; pq.allow_unknown = true; pq.max_path = 200; pq.want_cost = false; pq.want_frontier = false;
        std::vector<GridCell> goals(1), starts(1);
        goals[0][0] = 24; goals[0][1] = 4; starts[0][0] = 24; starts[0][1] = 4;
        NavPlan plan;
        a.planOnGrid(live, pq, goals, starts, plan);
        ok = ok && plan.start_status.size() == 1u;
        std::printf("grid ok=%d\n", ok ? 1 : 0);
        if (!ok) return 2;
        // the same frame as images three ticks later, every third pixel kept from stamping, the marks allowed two ticks: the cells that
        // only those pixels held up expire or are seen through
        cv::Mat d(cam.height, cam.width, CV_32FC1), m(cam.height, cam.width, CV_8UC1);
        std::memcpy(d.ptr<float>(), depth.data(), 4 * npix);
        std::memcpy(m.ptr<uint8_t>(), mask.data(), npix);
        d.pretendStrided();
        q.mask_mode = 2; q.min_hits = 30;
        mem.max_mark_age = 2u; mem.max_seen_age = 2u;
        LiveNavGrid masked;
        a.overlayDepthFrame(g, q, d, m, mem, 4u, masked);
        report("masked", masked, mem);
        q.mask_mode = 0; q.min_hits = 4;
        // refusals: before the library is asked, and the library's own (the tick)
        int threw = 0;
        LiveMemory scratch;
        try { a.overlayDepthFrame(g, q, counts, none, scratch, 1u, live); } catch (const std::logic_error&) { threw++; }
        try { std::vector<float> small(5); a.overlayDepthFrame(g, q, small, none, scratch, 1u, live); } catch (const std::invalid_argument&) { threw++; }
        try { NavGrid bare; bare.width = 4; bare.height = 4; a.overlayDepthFrame(bare, q, depth, none, scratch, 1u, live); } catch (const std::logic_error&) { threw++; }
        try { a.overlayDepthFrame(g, q, depth, none, scratch, 0u, live); } catch (const std::exception&) { threw++; }
        if (threw != 4) { std::printf("no refusal %d\n", threw); return 2; }
        // uint16 counts of a millimetre into a memory of five slices
        a.setInputFormat(SSF_COLOR_RGB8, SSF_DEPTH_U16_SCALED, 0.001);
        LiveMemory five;
        five.slices = 5;
        LiveNavGrid u16;
        a.overlayDepthFrame(g, q, counts, none, five, 7u, u16);
        report("u16", u16, five);
        five.clear();
        if (five.width != 0 || !five.marks.empty() || five.tick != 0u) { std::printf("clear\n"); return 2; }
    } catch (const std::exception& e) { std::printf("exception %s\n", e.what()); return 1; }
    return 0;
}
