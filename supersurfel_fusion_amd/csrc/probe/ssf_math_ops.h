/*
 * ssf_math_ops.h -- the operation numbers of the element-wise arithmetic evaluators (TEST INFRASTRUCTURE).
 *
 * One list, three readers: the device evaluator (ssf_math_probe.hip -> variants/mathprobe/libssf_mathprobe.so), the CPU
 * checker's batch entry, and tests/test_math_device_gpu.py / tests/test_math.py (which parse the SSF_MATHOP lines below).
 *
 * SSF_MATHOP(number, name, in_words, out_words): an element is in_words 32-bit words in, out_words 32-bit words out,
 * elements packed one after the other.  A double / int64 / uint64 takes two words (little endian, as in memory), a float /
 * int32 / uint32 one.  Matrices are 9 floats row-major, symmetric matrices 6 floats (xx xy xz yy yz zz), quaternions
 * (x, y, z, w).  Layouts that are not obvious from the name:
 *   fx64_*            double v -> int64; scale and limit are the compile-time constants of the kernel named in the comment
 *   fx32_s20 / _s24   fx32(v, 2^20) / fx32(v, 2^24): the two scales of the ICP normal equations
 *   div_inrange       (double n, double d) -> double
 *   rgb8_to_lab       one word r | g << 8 | b << 16 -> 3 floats, through the 256-entry host-built gamma table
 *   rng_draw          (seed lo, seed hi, stream, counter) -> (draw, counter afterwards)
 *   sym_inverse       cov6 -> (invertible 0 / 1, inv6)            plane_solve   rows12 -> (accepted 0 / 1, theta3)
 *   principal_frame   cov6 -> (vecs9, vals3)                      guard         3 x 3 int32 label patch -> 0 / 1
 *   sym_mul           (cov6, v3) -> v3        rot_sym  (R9, cov6) -> cov6        m3_mul   (A9, B9) -> 9
 *   m3_mulv           (A9, v3) -> v3          row_mul  (v3, A9) -> v3
 */
#ifndef SSF_MATH_OPS_H
#define SSF_MATH_OPS_H

#define SSF_MATHOPS(SSF_MATHOP) \
    SSF_MATHOP(0, fx64_disp, 2, 2)          /* 2^30, limit 2^52: disparity sums (extract, relabelling pass) */ \
    SSF_MATHOP(1, fx64_mom, 2, 2)           /* 2^24, limit 2^40: k_render_moments */ \
    SSF_MATHOP(2, fx64_icp_r, 2, 2)         /* 2^44, limit 2^62: the ICP residual word */ \
    SSF_MATHOP(3, fx64_align_pos, 2, 2)     /* 2^24, limit 2^52: loop-closure centroids */ \
    SSF_MATHOP(4, fx64_align_d2, 2, 2)      /* 2^30, limit 2^52: loop-closure scale */ \
    SSF_MATHOP(5, fx64_odo_a, 2, 2)         /* 2^10, limit 2^40: odometry normal matrix */ \
    SSF_MATHOP(6, fx64_odo_b, 2, 2)         /* 2^24, limit 2^40: odometry right-hand side */ \
    SSF_MATHOP(7, fx64_odo_c, 2, 2)         /* 2^36, limit 2^40: odometry residual */ \
    SSF_MATHOP(8, fx32r, 1, 1) \
    SSF_MATHOP(9, fx32_s20, 1, 1) \
    SSF_MATHOP(10, fx32_s24, 1, 1) \
    SSF_MATHOP(11, pixel_round, 1, 1) \
    SSF_MATHOP(12, div3_u64, 2, 2) \
    SSF_MATHOP(13, div3_exact, 2, 2) \
    SSF_MATHOP(14, div_inrange, 4, 2) \
    SSF_MATHOP(15, cbrt_spec, 2, 2) \
    SSF_MATHOP(16, root5_spec, 2, 2) \
    SSF_MATHOP(17, pow24_spec, 1, 1) \
    SSF_MATHOP(18, pow_inv24_spec, 1, 1) \
    SSF_MATHOP(19, cbrtf_spec, 1, 1) \
    SSF_MATHOP(20, exp_neg_spec, 1, 1) \
    SSF_MATHOP(21, srgb_expand, 1, 1) \
    SSF_MATHOP(22, srgb_compress, 1, 1) \
    SSF_MATHOP(23, lab_f, 1, 1) \
    SSF_MATHOP(24, rgb_to_lab, 3, 3) \
    SSF_MATHOP(25, lab_to_rgb, 3, 3) \
    SSF_MATHOP(26, rgb8_to_lab, 1, 3) \
    SSF_MATHOP(27, rng_draw, 4, 2) \
    SSF_MATHOP(28, rng_unit, 1, 1) \
    SSF_MATHOP(29, len3, 3, 1) \
    SSF_MATHOP(30, unit3, 3, 3) \
    SSF_MATHOP(31, sym_inverse, 6, 7) \
    SSF_MATHOP(32, principal_frame, 6, 12) \
    SSF_MATHOP(33, plane_solve, 12, 4) \
    SSF_MATHOP(34, guard, 9, 1) \
    SSF_MATHOP(35, sym_square, 6, 6) \
    SSF_MATHOP(36, sym_mul, 9, 3) \
    SSF_MATHOP(37, rot_sym, 15, 6) \
    SSF_MATHOP(38, m3_mul, 18, 9) \
    SSF_MATHOP(39, m3_mulv, 12, 3) \
    SSF_MATHOP(40, row_mul, 12, 3) \
    SSF_MATHOP(41, rot_to_quat, 9, 4) \
    SSF_MATHOP(42, quat_to_rot_quirk, 4, 9)

#define SSF_MATHOP_COUNT 43

#endif
