// oracle_mathbatch.cpp -- TEST INFRASTRUCTURE (CPU oracle): the per-element arithmetic of oracle_math.h looped over n elements,
// under the operation numbers and element layouts of supersurfel_fusion_amd/csrc/probe/ssf_math_ops.h.  It is the reference of
// tests/test_math_device_gpu.py, which runs the product's ssf_math.hpp on the device under the same numbers and asks for 0 bits of
// difference.  Every operation below is the PLAIN one: where oracle_math.h has no counterpart of a product helper (the rewritten
// divisions div3_u64 / div3_exact / div_inrange) the reference is the operation it replaces -- b / 3, x / 3.0, n / d.
// The fixed-point scales and limits are restated here as powers of two, not taken from the product's headers.
//
// This file alone is compiled with OpenMP (oracle/Makefile): the loop over elements is split among threads, each element is
// computed by one thread exactly as in the sequential loop, so no bit depends on the thread count.
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "oracle.h"
#include "../supersurfel_fusion_amd/csrc/probe/ssf_math_ops.h"

using namespace orc;

namespace {

inline float w2f(uint32_t w) { float f; std::memcpy(&f, &w, 4); return f; }
inline uint32_t f2w(float f) { uint32_t w; std::memcpy(&w, &f, 4); return w; }
inline uint64_t w2u(const uint32_t* w) { return (uint64_t)w[0] | ((uint64_t)w[1] << 32); }
inline double w2d(const uint32_t* w) { uint64_t b = w2u(w); double d; std::memcpy(&d, &b, 8); return d; }
inline void u2w(uint64_t b, uint32_t* w) { w[0] = (uint32_t)b; w[1] = (uint32_t)(b >> 32); }
inline void d2w(double d, uint32_t* w) { uint64_t b; std::memcpy(&b, &d, 8); u2w(b, w); }
inline f3 w2v(const uint32_t* w) { return mk3(w2f(w[0]), w2f(w[1]), w2f(w[2])); }
inline void v2w(f3 v, uint32_t* w) { w[0] = f2w(v.x); w[1] = f2w(v.y); w[2] = f2w(v.z); }
inline Cov3 w2c(const uint32_t* w) { return mkcov(w2f(w[0]), w2f(w[1]), w2f(w[2]), w2f(w[3]), w2f(w[4]), w2f(w[5])); }
inline void c2w(const Cov3& c, uint32_t* w) { w[0] = f2w(c.xx); w[1] = f2w(c.xy); w[2] = f2w(c.xz); w[3] = f2w(c.yy); w[4] = f2w(c.yz); w[5] = f2w(c.zz); }
inline Mat33 w2m(const uint32_t* w) { Mat33 m; for (int r = 0; r < 3; r++) m.r[r] = w2v(w + 3 * r); return m; }
inline void m2w(const Mat33& m, uint32_t* w) { for (int r = 0; r < 3; r++) v2w(m.r[r], w + 3 * r); }

inline double pow2(int e) { return std::ldexp(1.0, e); }

#define OP(name) inline void op_##name(const uint32_t* in, uint32_t* out)
#define FX64_OP(name, scale_bits, lim_bits) OP(name) { u2w((uint64_t)fx_quant(w2d(in), pow2(scale_bits), pow2(lim_bits)), out); }
FX64_OP(fx64_disp, 30, 52)
FX64_OP(fx64_mom, 24, 40)
FX64_OP(fx64_icp_r, 44, 62)
FX64_OP(fx64_align_pos, 24, 52)
FX64_OP(fx64_align_d2, 30, 52)
FX64_OP(fx64_odo_a, 10, 40)
FX64_OP(fx64_odo_b, 24, 40)
FX64_OP(fx64_odo_c, 36, 40)
OP(fx32r) { out[0] = (uint32_t)fx_quant32r(w2f(in[0])); }
OP(fx32_s20) { out[0] = (uint32_t)fx_quant32(w2f(in[0]), 1048576.0f); }
OP(fx32_s24) { out[0] = (uint32_t)fx_quant32(w2f(in[0]), 16777216.0f); }
// round_half_away under the range rule its callers keep: -1 when v cannot be a pixel coordinate (|v| >= 2^23 or NaN)
OP(pixel_round) { const float v = w2f(in[0]); out[0] = (uint32_t)(!(std::fabs(v) < 8388608.0f) ? -1 : round_half_away(v)); }
OP(div3_u64) { u2w(w2u(in) / 3, out); }
OP(div3_exact) { d2w(w2d(in) / 3.0, out); }
OP(div_inrange) { d2w(w2d(in) / w2d(in + 2), out); }
OP(cbrt_spec) { d2w(spec_cbrt(w2d(in)), out); }
OP(root5_spec) { d2w(spec_root5(w2d(in)), out); }
OP(pow24_spec) { out[0] = f2w(spec_pow24(w2f(in[0]))); }
OP(pow_inv24_spec) { out[0] = f2w(spec_pow_inv24(w2f(in[0]))); }
OP(cbrtf_spec) { out[0] = f2w(spec_cbrtf(w2f(in[0]))); }
OP(exp_neg_spec) { out[0] = f2w(spec_exp_neg(w2f(in[0]))); }
// the three scalar pieces of rgbToLab / labToRgb (vector_math.cuh:566-585, 543-564), as oracle_math.h writes them inline
OP(srgb_expand) { const float r = w2f(in[0]); out[0] = f2w((r > 0.04045f) ? spec_pow24(fdiv(r + 0.055f, 1.055f)) : fdiv(r, 12.92f)); }
OP(srgb_compress) { const float r = w2f(in[0]); out[0] = f2w((r > 0.0031308f) ? (1.055f * spec_pow_inv24(r) - 0.055f) : 12.92f * r); }
OP(lab_f) { const float x = w2f(in[0]); out[0] = f2w((x > 0.008856f) ? spec_cbrtf(x) : 7.787f * x + 16.0f / 116.0f); }
OP(rgb_to_lab) { v2w(rgbToLab(w2v(in)), out); }
OP(lab_to_rgb) { v2w(labToRgb(w2v(in)), out); }
OP(rgb8_to_lab) { v2w(rgbToLab(mk3((float)(in[0] & 255u), (float)((in[0] >> 8) & 255u), (float)((in[0] >> 16) & 255u))), out); }
OP(rng_draw) { uint32_t counter = in[3]; out[0] = rng_u32(w2u(in), in[2], counter); out[1] = counter; }
OP(rng_unit) { out[0] = f2w(rng_uniform(in[0])); }
OP(len3) { out[0] = f2w(length(w2v(in))); }
OP(unit3) { v2w(normalize(w2v(in)), out); }
OP(sym_inverse) { Cov3 inv; out[0] = inverse(w2c(in), inv) ? 1u : 0u; c2w(inv, out + 1); }
OP(principal_frame) { Mat33 vecs; f3 vals; eigenDecomposition(w2c(in), vecs, vals, 10); m2w(vecs, out); v2w(vals, out + 9); }
OP(plane_solve) {
    float a = 0, b = 0, c = 0;
    out[0] = solvePlaneEquations(a, b, c, w2f(in[0]), w2f(in[1]), w2f(in[2]), w2f(in[3]), w2f(in[4]), w2f(in[5]), w2f(in[6]), w2f(in[7]),
                                 w2f(in[8]), w2f(in[9]), w2f(in[10]), w2f(in[11])) ? 1u : 0u;
    out[1] = f2w(a); out[2] = f2w(b); out[3] = f2w(c);
}
OP(guard) {
    const int ring[8] = {(int)in[0], (int)in[1], (int)in[2], (int)in[5], (int)in[8], (int)in[7], (int)in[6], (int)in[3]};
    out[0] = ring_unchangeable((int)in[4], ring) ? 1u : 0u;
}
OP(sym_square) { c2w(square(w2c(in)), out); }
OP(sym_mul) { v2w(w2c(in) * w2v(in + 6), out); }
OP(rot_sym) { c2w(mult_ABAt(w2m(in), w2c(in + 9)), out); }
OP(m3_mul) { m2w(w2m(in) * w2m(in + 9), out); }
OP(m3_mulv) { v2w(w2m(in) * w2v(in + 9), out); }
OP(row_mul) { v2w(transpose(w2m(in + 3)) * w2v(in), out); }               // float3 * Mat33, matrix_math.cuh:491-496
OP(rot_to_quat) { float q[4]; rot_to_quat(w2m(in), q); for (int j = 0; j < 4; j++) out[j] = f2w(q[j]); }
OP(quat_to_rot_quirk) { float q[4]; for (int j = 0; j < 4; j++) q[j] = w2f(in[j]); m2w(quat_to_rot(q), out); }

}  // namespace

extern "C" {
// operation `op` (ssf_math_ops.h) on n elements; 0, or -1 for an unknown operation
int ssf_oracle_mathbatch(int op, const void* in_, void* out_, size_t n) {
    const uint32_t* in = (const uint32_t*)in_; uint32_t* out = (uint32_t*)out_;
    const long long N = (long long)n;
    switch (op) {
#define SSF_MATHOP(id, name, IW, OW)                                                             \
    case id: {                                                                                   \
        _Pragma("omp parallel for schedule(static)")                                             \
        for (long long i = 0; i < N; i++) op_##name(in + (size_t)i * IW, out + (size_t)i * OW);  \
        return 0;                                                                                \
    }
        SSF_MATHOPS(SSF_MATHOP)
#undef SSF_MATHOP
    default: return -1;
    }
}
int ssf_oracle_mathbatch_num_ops(void) { return SSF_MATHOP_COUNT; }
}  // extern "C"
