// navfloor_solve_check.cpp -- the host steps of ssf_navfloor_fit as the library compiles them (csrc/ssf_navfloor_solve.hpp, and nothing
// else of the library), driven by lines on stdin and answered in integers and the bit patterns of floats, for tests/test_navfloor.py
// to compare with the numpy restatement.  Compile with -ffp-contract=off, as the library is.
//   round <min_rows> <ten int64> <n: 3 hex> <a: 3 hex> <b: 3 hex> <d: hex>        -> status [n_new: 3 hex, d_new, rms]
//   dir <961 counts>                                                              -> ia ib rows | none
//   height <min_rows> <floor_share256> <2048 counts>                              -> j* rows d0(height_res 0.02) | none
//   pose <up: 3 hex> <normal: 3 hex> <d> <o: 3 hex> <pc: 3 hex> <W> <H> <res> <S: 3 int64> <tilt_cos>
//                                                                                 -> u, a, b, n0, scale, camera_height, pose: 26 hex
#include "ssf_navfloor_solve.hpp"

#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

namespace nf = ssf_navfloor;

static float get_f(std::istream& in) {
    std::string w;
    in >> w;
    const uint32_t u = (uint32_t)std::stoul(w, nullptr, 16);
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}
static void get3(std::istream& in, float* v) { for (int k = 0; k < 3; k++) v[k] = get_f(in); }
static void put(float f, bool& first) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    std::printf("%s%08x", first ? "" : " ", u);
    first = false;
}
static void put3(const float* v, bool& first) { for (int k = 0; k < 3; k++) put(v[k], first); }

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string what;
        if (!(in >> what)) continue;
        bool first = true;
        if (what == "round") {
            int min_rows;
            int64_t s[10];
            float n[3], a[3], b[3], n_new[3], d_new = 0.0f, rms = 0.0f;
            in >> min_rows;
            for (int k = 0; k < 10; k++) { long long v; in >> v; s[k] = v; }
            get3(in, n); get3(in, a); get3(in, b);
            const float d = get_f(in);
            const int status = nf::refine_round(s, min_rows, n, a, b, d, n_new, &d_new, &rms);
            std::printf("%d", status);
            first = false;
            if (status == nf::OK) { put3(n_new, first); put(d_new, first); put(rms, first); }
        } else if (what == "dir") {
            std::vector<uint32_t> hist(nf::DIR_BINS * nf::DIR_BINS);
            for (auto& v : hist) in >> v;
            int ia, ib;
            uint64_t rows;
            if (nf::direction_winner(hist.data(), &ia, &ib, &rows)) std::printf("%d %d %llu", ia, ib, (unsigned long long)rows);
            else std::printf("none");
        } else if (what == "height") {
            int min_rows, share, j;
            uint64_t rows;
            in >> min_rows >> share;
            std::vector<uint32_t> hist(nf::HEIGHT_BINS);
            for (auto& v : hist) in >> v;
            if (nf::height_winner(hist.data(), min_rows, share, &j, &rows)) {
                std::printf("%d %llu", j, (unsigned long long)rows);
                first = false;
                put(nf::height_of_bin(j, 0.02f), first);
            } else std::printf("none");
        } else if (what == "pose") {
            float up[3], normal[3], o[3], pc[3], u[3], a[3], b[3], n0[3], pose[12];
            get3(in, up); get3(in, normal);
            const float d = get_f(in);
            get3(in, o); get3(in, pc);
            int W, H;
            in >> W >> H;
            const float res = get_f(in);
            int64_t S[3];
            for (int k = 0; k < 3; k++) { long long v; in >> v; S[k] = v; }
            const float tilt_cos = get_f(in);
            if (!nf::unit_up(up, u) || !nf::hint_frame(u, a, b) || !nf::direction_normal(S, n0) || !nf::grid_pose(normal, d, o, pc, a, b, W, H, res, pose)) {
                std::printf("failed\n");
                continue;
            }
            put3(u, first); put3(a, first); put3(b, first); put3(n0, first);
            put(nf::vote_scale(tilt_cos), first); put(nf::camera_height(pc, normal, d), first);
            for (int k = 0; k < 12; k++) put(pose[k], first);
        } else {
            std::fprintf(stderr, "unknown line: %s\n", what.c_str());
            return 1;
        }
        std::printf("\n");
    }
    return 0;
}
