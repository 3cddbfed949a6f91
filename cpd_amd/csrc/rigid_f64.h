// rigid_f64.h -- the float64 pose product of points_rigid_transform (precompute_ppscore.py:36-45,
// outline_utils.py:328-338), shared by ppscore.hip and mfcf.hip. Both files are built with -ffp-contract=off; the only fused
// multiply-adds are the explicit ones below, which are the reference's.
#pragma once
#include "common.h"

namespace {

// One points_rigid_transform product (l.36-45): the np.mat product is a dgemm whose inner loop accumulates over k with fused
// multiply-adds, acc = m0*x; acc = fma(m1, y, acc); acc = fma(m2, z, acc); acc + m3 (the last step multiplies by the exact 1
// of the homogeneous column). The unfused (m0*x + m1*y) + m2*z + m3 of roi_pool.hip's rigid3 differs from it by one float64
// ulp on some rows, which survives the rounding to float32 where the sum cancels to almost zero (DESIGN 5m has the counts).
// These are explicit fma() calls; the file is still built with -ffp-contract=off, so nothing else is ever fused.
__device__ __forceinline__ float pp_row(const double *m, double x, double y, double z) {
    return (float)__dadd_rn(__fma_rn(m[2], z, __fma_rn(m[1], y, __dmul_rn(m[0], x))), m[3]);
}
__device__ __forceinline__ void pp_rigid3(const double *m, float x, float y, float z, float &ox, float &oy, float &oz) {
    const double dx = x, dy = y, dz = z;
    ox = pp_row(m, dx, dy, dz);
    oy = pp_row(m + 4, dx, dy, dz);
    oz = pp_row(m + 8, dx, dy, dz);
}

}  // namespace
