// ssf_navfloor_solve.hpp -- the host steps of ssf_navfloor_fit (include/ssf_navfloor.h): the hint frame, the winners of the two
// histograms, the 128-bit centring and the 2 x 2 solve of a round, the pose.  Free of HIP, so that a stand-alone C++ program can
// compile and check it on the CPU (tests/cpp/navfloor_solve_check.cpp); it must be compiled with -ffp-contract=off, as the library
// is: every line below is one f64 (or, where the header says so, f32) operation in the header's order.
#pragma once
#include <cmath>
#include <cstdint>

namespace ssf_navfloor {

enum { OK = 0, NO_FLOOR = 1, DEGENERATE = 2, DIR_BINS = 31, HEIGHT_BINS = 2048 };

inline double dot3(const double* v, const double* w) { return (v[0] * w[0] + v[1] * w[1]) + v[2] * w[2]; }
inline float dot3f(const float* v, const float* w) { return (v[0] * w[0] + v[1] * w[1]) + v[2] * w[2]; }

// step 0: u = the hint normalised; false: not finite or zero
inline bool unit_up(const float* up, float* u) {
    const double U[3] = {(double)up[0], (double)up[1], (double)up[2]};
    const double L = std::sqrt(dot3(U, U));
    if (!std::isfinite(L) || !(L > 0.0)) return false;
    for (int k = 0; k < 3; k++) u[k] = (float)(U[k] / L);
    return true;
}
// step 0: frame(n, v) = (x, y, n); false: it does not exist
inline bool frame(const float* n, const float* v, float* x, float* y) {
    const double N[3] = {(double)n[0], (double)n[1], (double)n[2]}, V[3] = {(double)v[0], (double)v[1], (double)v[2]};
    const double t = dot3(V, N);
    const double W[3] = {V[0] - t * N[0], V[1] - t * N[1], V[2] - t * N[2]};
    const double L = std::sqrt(dot3(W, W));
    if (!(L > 0.0)) return false;
    const double X[3] = {W[0] / L, W[1] / L, W[2] / L};
    const double Y[3] = {N[1] * X[2] - N[2] * X[1], N[2] * X[0] - N[0] * X[2], N[0] * X[1] - N[1] * X[0]};
    for (int k = 0; k < 3; k++) { x[k] = (float)X[k]; y[k] = (float)Y[k]; }
    return true;
}
// step 0: the hint frame (a, b, u)
inline bool hint_frame(const float* u, float* a, float* b) {
    int e = 0;
    for (int k = 1; k < 3; k++) if (std::fabs(u[k]) < std::fabs(u[e])) e = k;
    float ax[3] = {0.0f, 0.0f, 0.0f};
    ax[e] = 1.0f;
    return frame(u, ax, a, b);
}
// step 2: the scale of the direction vote
inline float vote_scale(float tilt_cos) { return 15.0f / sqrtf(1.0f - tilt_cos * tilt_cos); }

// step 2: the winner of the direction histogram; false: it is empty
inline bool direction_winner(const uint32_t* hist, int* ia0, int* ib0, uint64_t* rows) {
    uint64_t best = 0;
    int at = -1;
    for (int ib = 0; ib < DIR_BINS; ib++)
        for (int ia = 0; ia < DIR_BINS; ia++) {
            uint64_t w = 0;
            for (int y = ib - 1; y <= ib + 1; y++)
                for (int x = ia - 1; x <= ia + 1; x++)
                    if (y >= 0 && y < DIR_BINS && x >= 0 && x < DIR_BINS) w += hist[y * DIR_BINS + x];
            if (w > best) { best = w; at = ib * DIR_BINS + ia; }
        }
    if (at < 0) return false;
    *ia0 = at % DIR_BINS; *ib0 = at / DIR_BINS; *rows = best;
    return true;
}
// step 2: n0 of the three quantised sums
inline bool direction_normal(const int64_t* S, float* n0) {
    const double D[3] = {(double)S[0], (double)S[1], (double)S[2]};
    const double L = std::sqrt(dot3(D, D));
    if (!(L > 0.0)) return false;
    for (int k = 0; k < 3; k++) n0[k] = (float)(D[k] / L);
    return true;
}
// step 3: j* and W(j*); false: no bin is large enough
inline bool height_winner(const uint32_t* hist, int min_rows, int floor_share256, int* jstar, uint64_t* rows) {
    auto W = [&](int j) {
        uint64_t w = hist[j];
        if (j > 0) w += hist[j - 1];
        if (j + 1 < HEIGHT_BINS) w += hist[j + 1];
        return w;
    };
    uint64_t wmax = 0;
    for (int j = 0; j < HEIGHT_BINS; j++) { const uint64_t w = W(j); if (w > wmax) wmax = w; }
    int j0 = -1;
    for (int j = 0; j < HEIGHT_BINS && j0 < 0; j++) {
        const uint64_t w = W(j);
        if (w >= (uint64_t)min_rows && w * 256u >= (uint64_t)floor_share256 * wmax) j0 = j;
    }
    if (j0 < 0) return false;
    int js = j0;
    for (int j = j0 + 1; j <= j0 + 4 && j < HEIGHT_BINS; j++) if (W(j) > W(js)) js = j;
    *jstar = js; *rows = W(js);
    return true;
}
inline float height_of_bin(int j, float height_res) { return ((float)(j - 1024) + 0.5f) * height_res; }

// step 4: one round's host part.  s: the ten words; (n, a, b, d): the round's frame and offset.  OK: the new plane and the rms
inline int refine_round(const int64_t* s, int min_rows, const float* n, const float* a, const float* b, float d, float* n_new, float* d_new, float* rms) {
    typedef __int128 i128;
    const i128 N = s[0], Sx = s[1], Sy = s[2], Sz = s[3];
    if (s[0] < (int64_t)min_rows) return NO_FLOOR;
    const double Cxx = (double)(N * s[4] - Sx * Sx), Cxy = (double)(N * s[5] - Sx * Sy), Cyy = (double)(N * s[6] - Sy * Sy);
    const double Cxz = (double)(N * s[7] - Sx * Sz), Cyz = (double)(N * s[8] - Sy * Sz), Czz = (double)(N * s[9] - Sz * Sz);
    const double det = Cxx * Cyy - Cxy * Cxy;
    if (!(det > 0.0)) return DEGENERATE;
    const double alpha = (Cxz * Cyy - Cyz * Cxy) / det;
    const double beta = (Cyz * Cxx - Cxz * Cxy) / det;
    const double gamma = (((double)s[3] - alpha * (double)s[1]) - beta * (double)s[2]) / (double)s[0];
    double V[3];
    for (int k = 0; k < 3; k++) V[k] = ((double)n[k] - alpha * (double)a[k]) - beta * (double)b[k];
    const double L = std::sqrt(dot3(V, V));
    if (!(L > 0.0) || !std::isfinite(L)) return DEGENERATE;
    for (int k = 0; k < 3; k++) n_new[k] = (float)(V[k] / L);
    *d_new = (float)(((double)d + gamma * 0.0009765625) / L);
    double r = (Czz - alpha * Cxz) - beta * Cyz;
    if (!(r > 0.0)) r = 0.0;
    *rms = (float)(std::sqrt(r / ((double)s[0] * (double)s[0])) * 0.0009765625);
    return OK;
}

// step 5: the camera's height above the plane, pc = camera - origin
inline float camera_height(const float* pc, const float* normal, float d) {
    const double P[3] = {(double)pc[0], (double)pc[1], (double)pc[2]}, N[3] = {(double)normal[0], (double)normal[1], (double)normal[2]};
    return (float)(dot3(P, N) - (double)d);
}
// step 5: the grid frame of the plane (normal, d) about the camera's foot point
inline bool grid_pose(const float* normal, float d, const float* o, const float* pc, const float* a, const float* b, int width, int height, float res,
                      float* pose) {
    float x[3], y[3];
    if (!frame(normal, a, x, y) && !frame(normal, b, x, y)) return false;
    const float gx = dot3f(pc, x), gy = dot3f(pc, y);
    const float sx = (floorf(gx / res) - (float)(width / 2)) * res, sy = (floorf(gy / res) - (float)(height / 2)) * res;
    for (int i = 0; i < 3; i++) {
        pose[3 * i] = x[i] + 0.0f; pose[3 * i + 1] = y[i] + 0.0f; pose[3 * i + 2] = normal[i] + 0.0f;
        pose[9 + i] = (float)((((double)o[i] + (double)sx * (double)x[i]) + (double)sy * (double)y[i]) + (double)d * (double)normal[i]);
    }
    return true;
}

}  // namespace ssf_navfloor
