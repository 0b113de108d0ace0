// The live obstacle layer of include/ssf.hpp (LiveParams, overlayDepthFrame, LiveNavGrid).  The depth image, the mask and the grid
// come from integer hashes of the pixel / cell number, every float of them exact, so that tests/test_navlive_gpu.py makes the same
// arrays and compares counts and FNV-1a checksums with the Python calls.  Three calls: float depth in a std::vector, the same as
// cv::Mat (a double) with a CV_8UC1 mask under mask_mode 2, and uint16 counts after setInputFormat.  The result goes through
// fillOccupancyGrid and planOnGrid as it is.
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
static void report(const char* what, const supersurfel_fusion::LiveNavGrid& g) {
    const ssf_navlive_stats& s = g.live;
    std::printf("%s valid=%lld stamping=%lld points=%lld rays=%lld entries=%lld stamped=%lld opened=%lld state=%016llx dist2=%016llx hits=%016llx "
                "seen=%016llx\n", what, (long long)s.pixels_valid, (long long)s.pixels_stamping, (long long)s.points_in_band, (long long)s.rays,
                (long long)s.ray_entries, (long long)s.cells_stamped, (long long)s.cells_opened, (unsigned long long)fnv1a(g.state.data(), g.state.size()),
                (unsigned long long)fnv1a(g.dist2.data(), 4 * g.dist2.size()), (unsigned long long)fnv1a(g.live_hits.data(), 4 * g.live_hits.size()),
                (unsigned long long)fnv1a(g.live_seen.data(), 4 * g.live_seen.size()));
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
        // the floor frame (grid y = map z, grid z = -map y) with the camera, at the map's origin, inside the grid
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
        LiveNavGrid live;
        a.overlayDepthFrame(g, q, depth, none, live);
        report("navlive", live);
        if (live.state.size() != P || live.dist2.size() != P || live.live_hits.size() != P || live.live_seen.size() != P) { std::printf("sizes\n"); return 2; }
        nav_msgs::OccupancyGrid msg;
        SupersurfelFusion::fillOccupancyGrid(live, msg);
        bool ok = msg.data.size() == P && msg.info.width == 48u && msg.info.height == 40u && msg.info.origin.position.x == (double)-1.2f &&
                  msg.info.origin.position.z == (double)-0.2f && std::memcmp(msg.data.data(), live.state.data(), P) == 0;
        // the live grid plans as it is
        PlanParams pq; pq.allow_unknown = true; pq.max_path = 200; pq.want_cost = false; pq.want_frontier = false;
        std::vector<GridCell> goals(1), starts(1);
        goals[0][0] = 24; goals[0][1] = 4; starts[0][0] = 24; starts[0][1] = 4;
        NavPlan plan;
        a.planOnGrid(live, pq, goals, starts, plan);
        ok = ok && plan.start_status.size() == 1u;
        std::printf("grid ok=%d\n", ok ? 1 : 0);
        if (!ok) return 2;
        // the same frame as images, the mask keeping every third pixel from stamping; fed back: the live grid as the next input
        cv::Mat d(cam.height, cam.width, CV_32FC1), m(cam.height, cam.width, CV_8UC1);
        std::memcpy(d.ptr<float>(), depth.data(), 4 * npix);
        std::memcpy(m.ptr<uint8_t>(), mask.data(), npix);
        d.pretendStrided();
        q.mask_mode = 2;
        LiveNavGrid masked;
        a.overlayDepthFrame(g, q, d, m, masked);
        report("masked", masked);
        LiveNavGrid again;
        q.mask_mode = 0;
        a.overlayDepthFrame(live, q, d, cv::Mat(), again);
        if (again.state != live.state || again.dist2 != live.dist2 || again.live.cells_stamped != 0 || again.live.cells_opened != 0) {
            std::printf("fed back: not a fixed point\n"); return 2;
        }
        // refusals before the library is asked
        int threw = 0;
        try { a.overlayDepthFrame(g, q, counts, none, live); } catch (const std::logic_error&) { threw++; }
        try { std::vector<float> small(5); a.overlayDepthFrame(g, q, small, none, live); } catch (const std::invalid_argument&) { threw++; }
        try { NavGrid bare; bare.width = 4; bare.height = 4; a.overlayDepthFrame(bare, q, depth, none, live); } catch (const std::logic_error&) { threw++; }
        if (threw != 3) { std::printf("no refusal\n"); return 2; }
        // uint16 counts of a millimetre
        a.setInputFormat(SSF_COLOR_RGB8, SSF_DEPTH_U16_SCALED, 0.001);
        LiveNavGrid u16;
        a.overlayDepthFrame(g, q, counts, none, u16);
        report("u16", u16);
    } catch (const std::exception& e) { std::printf("exception %s\n", e.what()); return 1; }
    return 0;
}
