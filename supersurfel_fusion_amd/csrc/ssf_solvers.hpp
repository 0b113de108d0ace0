// ssf_solvers.hpp -- the host solvers of the ICP and align loops: dependency-free counterparts of the reference's Eigen calls
// (LDLT with diagonal pivoting as Eigen::LDLT, partial-pivot LU inverse, Shoemake quaternion re-normalisation, Rodrigues rotation;
// pinned against the reference's vendored Eigen by tests/test_solvers.py through the ssf_dbg_* hooks of ssf_testing.hip).  Plain
// C++ without a HIP type (g++ -std=c++17 compiles it on its own); ssf_host.hip (icp_update, icp_end, align_loop) includes it too.
#pragma once
#include <cfloat>
#include <cmath>
#include <cstring>
#include <utility>

#pragma GCC visibility push(hidden)       // (shared by the library's own files, no part of what it exports)
namespace ssf {
inline void sym6_ldlt_solve(const double* A, const double* b, double* x) {
    const int n = 6;
    double L[36]; int piv[6]; double w[6];
    std::memcpy(L, A, sizeof(L));
    bool all_zero = false;
    for (int k = 0; k < n; k++) {
        int p = k; double pm = std::fabs(L[k * n + k]);
        for (int i = k + 1; i < n; i++) if (std::fabs(L[i * n + i]) > pm) { pm = std::fabs(L[i * n + i]); p = i; }
        piv[k] = p;
        if (p != k) {                       // symmetric row/column exchange on the lower triangle
            for (int j = 0; j < k; j++) std::swap(L[k * n + j], L[p * n + j]);
            for (int i = p + 1; i < n; i++) std::swap(L[i * n + k], L[i * n + p]);
            std::swap(L[k * n + k], L[p * n + p]);
            for (int i = k + 1; i < p; i++) std::swap(L[i * n + k], L[p * n + i]);
        }
        if (k > 0) {
            for (int j = 0; j < k; j++) w[j] = L[j * n + j] * L[k * n + j];
            double s = 0.0;
            for (int j = 0; j < k; j++) s += L[k * n + j] * w[j];
            L[k * n + k] -= s;
            for (int i = k + 1; i < n; i++) {
                double s2 = 0.0;
                for (int j = 0; j < k; j++) s2 += L[i * n + j] * w[j];
                L[i * n + k] -= s2;
            }
        }
        const double d = L[k * n + k];
        const bool ok = std::fabs(d) > 0.0;
        if (k == 0 && !ok) { for (int j = 0; j < n; j++) piv[j] = j; all_zero = true; break; }
        if (ok) for (int i = k + 1; i < n; i++) L[i * n + k] /= d;
    }
    double y[6];
    for (int i = 0; i < n; i++) y[i] = b[i];
    for (int k = 0; k < n; k++) std::swap(y[k], y[piv[k]]);
    if (!all_zero) for (int i = 0; i < n; i++) for (int j = 0; j < i; j++) y[i] -= L[i * n + j] * y[j];
    for (int i = 0; i < n; i++) { const double d = L[i * n + i]; y[i] = (std::fabs(d) > DBL_MIN) ? y[i] / d : 0.0; }
    if (!all_zero) for (int i = n - 1; i >= 0; i--) for (int j = i + 1; j < n; j++) y[i] -= L[j * n + i] * y[j];
    for (int k = n - 1; k >= 0; k--) std::swap(y[k], y[piv[k]]);
    for (int i = 0; i < n; i++) x[i] = y[i];
}

inline void mat6_inverse_lu(const double* A, double* Ainv) {
    const int n = 6;
    double U[36]; int perm[6];
    std::memcpy(U, A, sizeof(U));
    for (int i = 0; i < n; i++) perm[i] = i;
    for (int k = 0; k < n; k++) {
        int p = k; double pm = std::fabs(U[k * n + k]);
        for (int i = k + 1; i < n; i++) if (std::fabs(U[i * n + k]) > pm) { pm = std::fabs(U[i * n + k]); p = i; }
        if (p != k) { for (int j = 0; j < n; j++) std::swap(U[k * n + j], U[p * n + j]); std::swap(perm[k], perm[p]); }
        for (int i = k + 1; i < n; i++) {
            U[i * n + k] /= U[k * n + k];
            for (int j = k + 1; j < n; j++) U[i * n + j] -= U[i * n + k] * U[k * n + j];
        }
    }
    for (int c = 0; c < n; c++) {
        double y[6];
        for (int i = 0; i < n; i++) y[i] = (perm[i] == c) ? 1.0 : 0.0;
        for (int i = 0; i < n; i++) for (int j = 0; j < i; j++) y[i] -= U[i * n + j] * y[j];
        for (int i = n - 1; i >= 0; i--) { for (int j = i + 1; j < n; j++) y[i] -= U[i * n + j] * y[j]; y[i] /= U[i * n + i]; }
        for (int i = 0; i < n; i++) Ainv[i * n + c] = y[i];
    }
}

template <typename T>
inline void renormalise_rotation(T* R) {       // Quaternion(R).normalized().toRotationMatrix()
    T q[4];
    T t = (R[0] + R[4]) + R[8];
    if (t > T(0)) {
        t = std::sqrt(t + T(1.0)); q[3] = T(0.5) * t; t = T(0.5) / t;
        q[0] = (R[7] - R[5]) * t; q[1] = (R[2] - R[6]) * t; q[2] = (R[3] - R[1]) * t;
    } else {
        int i = 0;
        if (R[4] > R[0]) i = 1;
        if (R[8] > R[i * 4]) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        t = std::sqrt(((R[i * 4] - R[j * 4]) - R[k * 4]) + T(1.0));
        q[i] = T(0.5) * t; t = T(0.5) / t;
        q[3] = (R[k * 3 + j] - R[j * 3 + k]) * t;
        q[j] = (R[j * 3 + i] + R[i * 3 + j]) * t;
        q[k] = (R[k * 3 + i] + R[i * 3 + k]) * t;
    }
    const T z = ((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3];
    if (z > T(0)) { const T nrm = std::sqrt(z); for (int a = 0; a < 4; a++) q[a] = q[a] / nrm; }
    const T tx = T(2) * q[0], ty = T(2) * q[1], tz = T(2) * q[2];
    const T twx = tx * q[3], twy = ty * q[3], twz = tz * q[3];
    const T txx = tx * q[0], txy = ty * q[0], txz = tz * q[0];
    const T tyy = ty * q[1], tyz = tz * q[1], tzz = tz * q[2];
    R[0] = T(1) - (tyy + tzz); R[1] = txy - twz; R[2] = txz + twy;
    R[3] = txy + twz; R[4] = T(1) - (txx + tzz); R[5] = tyz - twx;
    R[6] = txz - twy; R[7] = tyz + twx; R[8] = T(1) - (txx + tyy);
}

inline void rodrigues(double angle, const double* ax, double* R) {     // AngleAxisd::toRotationMatrix
    const double s = std::sin(angle), c = std::cos(angle);
    const double sx = s * ax[0], sy = s * ax[1], sz = s * ax[2];
    const double ox = (1.0 - c) * ax[0], oy = (1.0 - c) * ax[1], oz = (1.0 - c) * ax[2];
    double m;
    m = ox * ax[1]; R[1] = m - sz; R[3] = m + sz;
    m = ox * ax[2]; R[2] = m + sy; R[6] = m - sy;
    m = oy * ax[2]; R[5] = m - sx; R[7] = m + sx;
    R[0] = ox * ax[0] + c; R[4] = oy * ax[1] + c; R[8] = oz * ax[2] + c;
}

// one Gauss-Newton increment from the solved 6-vector: tf_iter (4x4, row-major)
inline void gn_increment(const double* X, double* tf_iter) {
    double tran[3] = {X[3], X[4], X[5]}, axis[3] = {X[0], X[1], X[2]};
    const double nrm = std::sqrt((axis[0] * axis[0] + axis[1] * axis[1]) + axis[2] * axis[2]);
    const double angle = 0.5 * std::atan(nrm);
    double Rr[9];
    if (nrm == 0.0) { for (int i = 0; i < 9; i++) Rr[i] = (i % 4 == 0) ? 1.0 : 0.0; }
    else { for (int i = 0; i < 3; i++) axis[i] /= nrm; rodrigues(angle, axis, Rr); }
    const double ca = std::cos(angle);
    for (int i = 0; i < 3; i++) tran[i] *= ca;
    for (int i = 0; i < 16; i++) tf_iter[i] = 0.0;
    double R9[9];
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) R9[i * 3 + j] = (Rr[i * 3] * Rr[j] + Rr[i * 3 + 1] * Rr[3 + j]) + Rr[i * 3 + 2] * Rr[6 + j];
        tf_iter[i * 4 + 3] = (Rr[i * 3] * tran[0] + Rr[i * 3 + 1] * tran[1]) + Rr[i * 3 + 2] * tran[2];
    }
    renormalise_rotation<double>(R9);
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) tf_iter[i * 4 + j] = R9[i * 3 + j];
    tf_iter[15] = 1.0;
}

// host step of one align iteration (DenseRegistration::align, dense_registration.cu:168-210): as gn_increment, with
// the translation un-scaled and the increment conjugated by the centroid translations:
// T(ct) * Rot * T(tran) * Rot * T(-cs), Eigen Isometry products left to right
inline void align_increment(const double* JtJ, const double* Jtr, float scale, const float* cs, const float* ct, double* tf_iter) {
    double X[6];
    sym6_ldlt_solve(JtJ, Jtr, X);
    double tran[3] = {X[3], X[4], X[5]}, axis[3] = {X[0], X[1], X[2]};
    const double nrm = std::sqrt((axis[0] * axis[0] + axis[1] * axis[1]) + axis[2] * axis[2]);
    const double angle = 0.5 * std::atan(nrm);
    double Rr[9];
    if (nrm == 0.0) { for (int i = 0; i < 9; i++) Rr[i] = (i % 4 == 0) ? 1.0 : 0.0; }
    else { for (int i = 0; i < 3; i++) axis[i] /= nrm; rodrigues(angle, axis, Rr); }
    const double ca = std::cos(angle);
    for (int i = 0; i < 3; i++) { tran[i] /= (double)scale; tran[i] *= ca; }
    double RR[9], t2[3], t4[3];
    for (int i = 0; i < 3; i++) {
        t2[i] = ((Rr[i * 3] * tran[0] + Rr[i * 3 + 1] * tran[1]) + Rr[i * 3 + 2] * tran[2]) + (double)ct[i];
        for (int j = 0; j < 3; j++) RR[i * 3 + j] = (Rr[i * 3] * Rr[j] + Rr[i * 3 + 1] * Rr[3 + j]) + Rr[i * 3 + 2] * Rr[6 + j];
    }
    const double ncs[3] = {-1.0 * (double)cs[0], -1.0 * (double)cs[1], -1.0 * (double)cs[2]};
    for (int i = 0; i < 3; i++) t4[i] = ((RR[i * 3] * ncs[0] + RR[i * 3 + 1] * ncs[1]) + RR[i * 3 + 2] * ncs[2]) + t2[i];
    renormalise_rotation<double>(RR);
    for (int i = 0; i < 16; i++) tf_iter[i] = 0.0;
    for (int i = 0; i < 3; i++) { for (int j = 0; j < 3; j++) tf_iter[i * 4 + j] = RR[i * 3 + j]; tf_iter[i * 4 + 3] = t4[i]; }
    tf_iter[15] = 1.0;
}

inline void mat4_lmul(const double* a, double* b) {      // b <- a * b
    double r[16];
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++)
            r[i * 4 + j] = ((a[i * 4] * b[j] + a[i * 4 + 1] * b[4 + j]) + a[i * 4 + 2] * b[8 + j]) + a[i * 4 + 3] * b[12 + j];
    std::memcpy(b, r, sizeof(r));
}
}  // namespace ssf
#pragma GCC visibility pop
