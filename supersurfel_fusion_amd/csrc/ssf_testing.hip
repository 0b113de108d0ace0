// ssf_testing.hip -- the test hooks of include/ssf_testing.h: the host solvers (ssf_solvers.hpp) and the kernels' per-element
// arithmetic (ssf_math.hpp) evaluated on the host, so they can be pinned on a CPU box.  Nothing here touches the handle or the device.
#include <hip/hip_runtime.h>          // (ssf_math.hpp's SSF_HD under hipcc)
#include "ssf_math.hpp"
#include "ssf_solvers.hpp"
#include "../../include/ssf_testing.h"

using namespace ssf;

static M3 m3_from9(const float* a) { return m3(v3(a[0], a[1], a[2]), v3(a[3], a[4], a[5]), v3(a[6], a[7], a[8])); }
static void m3_to9(const M3& m, float* o) { o[0] = m.r0.x; o[1] = m.r0.y; o[2] = m.r0.z; o[3] = m.r1.x; o[4] = m.r1.y; o[5] = m.r1.z; o[6] = m.r2.x; o[7] = m.r2.y; o[8] = m.r2.z; }
static void sym_to6(const Sym3& s, float* o) { o[0] = s.xx; o[1] = s.xy; o[2] = s.xz; o[3] = s.yy; o[4] = s.yz; o[5] = s.zz; }

extern "C" {
int ssf_dbg_ldlt_solve6(const double* A, const double* b, double* x) { sym6_ldlt_solve(A, b, x); return 0; }
int ssf_dbg_lu_inverse6(const double* A, double* Ainv) { mat6_inverse_lu(A, Ainv); return 0; }
int ssf_dbg_renormalise_d(double* R9) { renormalise_rotation<double>(R9); return 0; }
int ssf_dbg_renormalise_f(float* R9) { renormalise_rotation<float>(R9); return 0; }
int ssf_dbg_gn_increment(const double* X6, double* tf16) { gn_increment(X6, tf16); return 0; }
int ssf_dbg_align_increment(const double* JtJ, const double* Jtr, float scale, const float* cs, const float* ct, double* tf16) {
    align_increment(JtJ, Jtr, scale, cs, ct, tf16); return 0;
}

int ssf_dbg_rgb_to_lab(const float* c, float* o) { V3 r = rgb_to_lab(v3(c[0], c[1], c[2])); o[0] = r.x; o[1] = r.y; o[2] = r.z; return 0; }
int ssf_dbg_lab_to_rgb(const float* c, float* o) { V3 r = lab_to_rgb(v3(c[0], c[1], c[2])); o[0] = r.x; o[1] = r.y; o[2] = r.z; return 0; }
int ssf_dbg_sym_inverse(const float* c, float* o) {
    Sym3 out; const bool ok = sym_inverse(sym3(c[0], c[1], c[2], c[3], c[4], c[5]), out);
    o[0] = out.xx; o[1] = out.xy; o[2] = out.xz; o[3] = out.yy; o[4] = out.yz; o[5] = out.zz; return ok ? 1 : 0;
}
int ssf_dbg_principal_frame(const float* c, float* vecs, float* vals) {
    M3 m; V3 v; principal_frame(sym3(c[0], c[1], c[2], c[3], c[4], c[5]), m, v);
    m3_to9(m, vecs); vals[0] = v.x; vals[1] = v.y; vals[2] = v.z; return 0;
}
// img9: a 3 x 3 label patch, row-major; returns 1 when the centre pixel is a bridge (its label may not change)
int ssf_dbg_connectivity_guard(const int32_t* g) { return guard_unchangeable(guard_ring(g[4], g[0], g[1], g[2], g[5], g[8], g[7], g[6], g[3])) ? 1 : 0; }
int ssf_dbg_plane_solve(const float* r, float* th) {
    float a = 0, b = 0, c = 0;
    const bool ok = plane_solve(a, b, c, r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7], r[8], r[9], r[10], r[11]);
    th[0] = a; th[1] = b; th[2] = c; return ok ? 1 : 0;
}
int ssf_dbg_sym_square(const float* c, float* o) { sym_to6(sym_square(sym3(c[0], c[1], c[2], c[3], c[4], c[5])), o); return 0; }
int ssf_dbg_sym_mulv(const float* c, const float* v, float* o) { V3 r = sym_mul(sym3(c[0], c[1], c[2], c[3], c[4], c[5]), v3(v[0], v[1], v[2])); o[0] = r.x; o[1] = r.y; o[2] = r.z; return 0; }
int ssf_dbg_mult_abat(const float* R9, const float* c, float* o) { sym_to6(rot_sym(m3_from9(R9), sym3(c[0], c[1], c[2], c[3], c[4], c[5])), o); return 0; }
int ssf_dbg_m3_mul(const float* A9, const float* B9, float* o) { m3_to9(m3_mul(m3_from9(A9), m3_from9(B9)), o); return 0; }
int ssf_dbg_m3_mulv(const float* A9, const float* v, float* o) { V3 r = m3_mulv(m3_from9(A9), v3(v[0], v[1], v[2])); o[0] = r.x; o[1] = r.y; o[2] = r.z; return 0; }
int ssf_dbg_row_mul(const float* v, const float* A9, float* o) { V3 r = row_mul(v3(v[0], v[1], v[2]), m3_from9(A9)); o[0] = r.x; o[1] = r.y; o[2] = r.z; return 0; }
int ssf_dbg_rot_to_quat(const float* R9, float* q4) { rot_to_quat(m3_from9(R9), q4); return 0; }
int ssf_dbg_quat_to_rot(const float* q4, float* R9) { m3_to9(quat_to_rot_quirk(q4), R9); return 0; }
}  // extern "C"
