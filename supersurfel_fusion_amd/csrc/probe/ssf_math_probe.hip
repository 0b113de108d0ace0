// ssf_math_probe.hip -- TEST INFRASTRUCTURE: the per-element arithmetic of ssf_math.hpp evaluated ON THE DEVICE, one element per
// thread, so that the branches only the GPU compiles (#if defined(__HIP_DEVICE_COMPILE__): fx64, fx32r, div_inrange, div3_u64) can
// be compared with the CPU checker element by element (tests/test_math_device_gpu.py).  Built with the product's FLAGS into
// variants/mathprobe/libssf_mathprobe.so; not an object of libssf_hip.so, which gains no symbol and no code from it.
//
// One kernel per operation of ssf_math_ops.h: thread i reads element i, calls the helper, writes element i.  fx64 is instantiated
// with each (scale, limit) pair a kernel passes, as compile-time constants: the device code emitted depends on the limit.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include "../ssf_math.hpp"
#include "../../../include/ssf.h"
#include "../../../include/ssf_odometry.h"
#include "ssf_math_ops.h"

using namespace ssf;

#define PROBE_HD __host__ __device__ __forceinline__

// 2^40, the odometry's clamp (SSF_ODO_LIM of ssf_odometry.hip, SSF_ODO_CLAMP_BITS of ssf_odometry.h)
#define PROBE_ODO_LIM 1099511627776.0
static_assert(SSF_ODO_CLAMP_BITS == 40, "the odometry clamp moved: update PROBE_ODO_LIM");
// the ICP residual word's pair as k_icp writes it (ssf_track_fuse.hip: emit(27, fx64(..., 17592186044416.0, 4611686018427387904.0)))
#define PROBE_ICP_R_LIM 4611686018427387904.0
static_assert(SSF_ICP_SCALE_R == 17592186044416.0, "the ICP residual scale moved");

PROBE_HD float w2f(uint32_t w) { float f; memcpy(&f, &w, 4); return f; }
PROBE_HD uint32_t f2w(float f) { uint32_t w; memcpy(&w, &f, 4); return w; }
PROBE_HD uint64_t w2u(const uint32_t* w) { return (uint64_t)w[0] | ((uint64_t)w[1] << 32); }
PROBE_HD double w2d(const uint32_t* w) { return bits_to_f64(w2u(w)); }
PROBE_HD void u2w(uint64_t b, uint32_t* w) { w[0] = (uint32_t)b; w[1] = (uint32_t)(b >> 32); }
PROBE_HD void d2w(double d, uint32_t* w) { u2w(f64_to_bits(d), w); }
PROBE_HD V3 w2v(const uint32_t* w) { return v3(w2f(w[0]), w2f(w[1]), w2f(w[2])); }
PROBE_HD void v2w(V3 v, uint32_t* w) { w[0] = f2w(v.x); w[1] = f2w(v.y); w[2] = f2w(v.z); }
PROBE_HD Sym3 w2s(const uint32_t* w) { return sym3(w2f(w[0]), w2f(w[1]), w2f(w[2]), w2f(w[3]), w2f(w[4]), w2f(w[5])); }
PROBE_HD void s2w(Sym3 s, uint32_t* w) { w[0] = f2w(s.xx); w[1] = f2w(s.xy); w[2] = f2w(s.xz); w[3] = f2w(s.yy); w[4] = f2w(s.yz); w[5] = f2w(s.zz); }
PROBE_HD M3 w2m(const uint32_t* w) { return m3(w2v(w), w2v(w + 3), w2v(w + 6)); }
PROBE_HD void m2w(M3 m, uint32_t* w) { v2w(m.r0, w); v2w(m.r1, w + 3); v2w(m.r2, w + 6); }

// ---- the operations: in -> out, both as 32-bit words (layouts: ssf_math_ops.h); `lut` is the host-built gamma table ---------------
#define OP(name) PROBE_HD void op_##name(const uint32_t* in, uint32_t* out, const float* lut)
#define FX64_OP(name, scale, lim) OP(name) { u2w((uint64_t)fx64(w2d(in), scale, lim), out); }
FX64_OP(fx64_disp, SSF_DISP_SCALE, SSF_DISP_LIM)
FX64_OP(fx64_mom, SSF_MOM_SCALE, SSF_MOM_LIM)
FX64_OP(fx64_icp_r, SSF_ICP_SCALE_R, PROBE_ICP_R_LIM)
FX64_OP(fx64_align_pos, SSF_ALIGN_SCALE_POS, SSF_ALIGN_LIM)
FX64_OP(fx64_align_d2, SSF_ALIGN_SCALE_D2, SSF_ALIGN_LIM)
FX64_OP(fx64_odo_a, (double)(1ll << SSF_ODO_S_A), PROBE_ODO_LIM)
FX64_OP(fx64_odo_b, (double)(1ll << SSF_ODO_S_B), PROBE_ODO_LIM)
FX64_OP(fx64_odo_c, (double)(1ll << SSF_ODO_S_C), PROBE_ODO_LIM)
OP(fx32r) { out[0] = (uint32_t)fx32r(w2f(in[0])); }
OP(fx32_s20) { out[0] = (uint32_t)fx32(w2f(in[0]), 1048576.0f); }
OP(fx32_s24) { out[0] = (uint32_t)fx32(w2f(in[0]), 16777216.0f); }
OP(pixel_round) { out[0] = (uint32_t)pixel_round(w2f(in[0])); }
OP(div3_u64) { u2w(div3_u64(w2u(in)), out); }
OP(div3_exact) { d2w(div3_exact(w2d(in)), out); }
OP(div_inrange) { d2w(div_inrange(w2d(in), w2d(in + 2)), out); }
OP(cbrt_spec) { d2w(cbrt_spec(w2d(in)), out); }
OP(root5_spec) { d2w(root5_spec(w2d(in)), out); }
OP(pow24_spec) { out[0] = f2w(pow24_spec(w2f(in[0]))); }
OP(pow_inv24_spec) { out[0] = f2w(pow_inv24_spec(w2f(in[0]))); }
OP(cbrtf_spec) { out[0] = f2w(cbrtf_spec(w2f(in[0]))); }
OP(exp_neg_spec) { out[0] = f2w(exp_neg_spec(w2f(in[0]))); }
OP(srgb_expand) { out[0] = f2w(srgb_expand(w2f(in[0]))); }
OP(srgb_compress) { out[0] = f2w(srgb_compress(w2f(in[0]))); }
OP(lab_f) { out[0] = f2w(lab_f(w2f(in[0]))); }
OP(rgb_to_lab) { v2w(rgb_to_lab(w2v(in)), out); }
OP(lab_to_rgb) { v2w(lab_to_rgb(w2v(in)), out); }
OP(rgb8_to_lab) { v2w(rgb8_to_lab(lut, in[0] & 255u, (in[0] >> 8) & 255u, (in[0] >> 16) & 255u), out); }
OP(rng_draw) { uint32_t counter = in[3]; out[0] = rng_draw(w2u(in), in[2], counter); out[1] = counter; }
OP(rng_unit) { out[0] = f2w(rng_unit(in[0])); }
OP(len3) { out[0] = f2w(len3(w2v(in))); }
OP(unit3) { v2w(unit3(w2v(in)), out); }
OP(sym_inverse) { Sym3 inv; out[0] = sym_inverse(w2s(in), inv) ? 1u : 0u; s2w(inv, out + 1); }
OP(principal_frame) { M3 vecs; V3 vals; principal_frame(w2s(in), vecs, vals); m2w(vecs, out); v2w(vals, out + 9); }
OP(plane_solve) {
    float a = 0, b = 0, c = 0;
    out[0] = plane_solve(a, b, c, w2f(in[0]), w2f(in[1]), w2f(in[2]), w2f(in[3]), w2f(in[4]), w2f(in[5]), w2f(in[6]), w2f(in[7]),
                         w2f(in[8]), w2f(in[9]), w2f(in[10]), w2f(in[11])) ? 1u : 0u;
    out[1] = f2w(a); out[2] = f2w(b); out[3] = f2w(c);
}
// 3 x 3 label patch, row-major (the ring walks NW, N, NE, E, SE, S, SW, W)
OP(guard) {
    out[0] = guard_unchangeable(guard_ring((int)in[4], (int)in[0], (int)in[1], (int)in[2], (int)in[5], (int)in[8], (int)in[7], (int)in[6], (int)in[3])) ? 1u : 0u;
}
OP(sym_square) { s2w(sym_square(w2s(in)), out); }
OP(sym_mul) { v2w(sym_mul(w2s(in), w2v(in + 6)), out); }
OP(rot_sym) { s2w(rot_sym(w2m(in), w2s(in + 9)), out); }
OP(m3_mul) { m2w(m3_mul(w2m(in), w2m(in + 9)), out); }
OP(m3_mulv) { v2w(m3_mulv(w2m(in), w2v(in + 9)), out); }
OP(row_mul) { v2w(row_mul(w2v(in), w2m(in + 3)), out); }
OP(rot_to_quat) { float q[4]; rot_to_quat(w2m(in), q); for (int j = 0; j < 4; j++) out[j] = f2w(q[j]); }
OP(quat_to_rot_quirk) { float q[4]; for (int j = 0; j < 4; j++) q[j] = w2f(in[j]); m2w(quat_to_rot_quirk(q), out); }

// ---- one element-wise kernel per operation; the same loop on the host (the host branches: the CPU tests' third party) -----------
#define SSF_MATHOP(id, name, IW, OW)                                                                                              \
    __global__ __launch_bounds__(256) void k_probe_##name(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, size_t n, \
                                                          const float* __restrict__ lut) {                                       \
        const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;                                                                \
        if (i >= n) return;                                                                                                      \
        uint32_t a[IW], r[OW];                                                                                                   \
        _Pragma("unroll") for (int j = 0; j < IW; j++) a[j] = in[i * IW + j];                                                    \
        op_##name(a, r, lut);                                                                                                    \
        _Pragma("unroll") for (int j = 0; j < OW; j++) out[i * OW + j] = r[j];                                                   \
    }                                                                                                                            \
    static void host_##name(const uint32_t* in, uint32_t* out, size_t n, const float* lut) {                                     \
        for (size_t i = 0; i < n; i++) op_##name(in + i * IW, out + i * OW, lut);                                                \
    }
SSF_MATHOPS(SSF_MATHOP)
#undef SSF_MATHOP

struct ProbeOp {
    int id; const char* name; int in_words, out_words;
    void (*kernel)(const uint32_t*, uint32_t*, size_t, const float*);
    void (*host)(const uint32_t*, uint32_t*, size_t, const float*);
};
#define SSF_MATHOP(id, name, IW, OW) {id, #name, IW, OW, k_probe_##name, host_##name},
static const ProbeOp g_ops[] = {SSF_MATHOPS(SSF_MATHOP)};
#undef SSF_MATHOP
static_assert(sizeof(g_ops) / sizeof(g_ops[0]) == SSF_MATHOP_COUNT, "SSF_MATHOP_COUNT does not match the list");

static const ProbeOp* find_op(int op) {
    for (const ProbeOp& o : g_ops) if (o.id == op) return &o;
    return nullptr;
}
// the gamma table as ssf_host.hip builds it: srgb_expand itself, on the host
static void build_lut(float* lut) { for (int c8 = 0; c8 < 256; c8++) lut[c8] = srgb_expand((float)c8 / 255.0f); }

extern "C" {
int ssf_mathprobe_num_ops(void) { return SSF_MATHOP_COUNT; }
// the k-th entry of the list (k = 0 .. num_ops - 1): its operation number, name and element sizes in 32-bit words
int ssf_mathprobe_op_info(int k, int* id, const char** name, int* in_words, int* out_words) {
    if (k < 0 || k >= SSF_MATHOP_COUNT) return -1;
    *id = g_ops[k].id; *name = g_ops[k].name; *in_words = g_ops[k].in_words; *out_words = g_ops[k].out_words;
    return 0;
}
void ssf_mathprobe_expand_lut(float* lut256) { build_lut(lut256); }

// operation `op` on n host elements ON THE DEVICE: allocate, copy in, launch, copy out, free.  Returns the HIP error code (0 = ok),
// -1 for an unknown operation.
int ssf_mathprobe_eval(int op, const void* in, void* out, size_t n) {
    const ProbeOp* o = find_op(op);
    if (!o) return -1;
    if (n == 0) return 0;
    if ((n + 255u) / 256u > 0x7FFFFFFFu) return -2;                 // (the grid is one block per 256 elements)
    const size_t ib = n * (size_t)o->in_words * 4u, ob = n * (size_t)o->out_words * 4u;
    uint32_t *din = nullptr, *dout = nullptr; float* dlut = nullptr;
    float lut[256]; build_lut(lut);
    hipError_t e = hipMalloc((void**)&din, ib);
    if (e == hipSuccess) e = hipMalloc((void**)&dout, ob);
    if (e == hipSuccess) e = hipMalloc((void**)&dlut, sizeof(lut));
    if (e == hipSuccess) e = hipMemcpy(din, in, ib, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dlut, lut, sizeof(lut), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(o->kernel, dim3((unsigned)((n + 255u) / 256u)), dim3(256), 0, 0, din, dout, n, dlut);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(out, dout, ob, hipMemcpyDeviceToHost);
    if (din) (void)hipFree(din);
    if (dout) (void)hipFree(dout);
    if (dlut) (void)hipFree(dlut);
    return (int)e;
}
// the same operation through the HOST branches of ssf_math.hpp (no device call): what the ssf_dbg_* hooks of the product evaluate
int ssf_mathprobe_eval_host(int op, const void* in, void* out, size_t n) {
    const ProbeOp* o = find_op(op);
    if (!o) return -1;
    float lut[256]; build_lut(lut);
    o->host((const uint32_t*)in, (uint32_t*)out, n, lut);
    return 0;
}
}  // extern "C"
