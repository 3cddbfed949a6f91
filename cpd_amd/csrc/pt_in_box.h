// pt_in_box.h -- the reference's CPU in-box test and its box staging, shared by roi_pool.hip (cpd_points_in_boxes_mask,
// cpd_crop_boxes) and augment.hip (cpd_augment_scene). Every file that includes it is compiled with -ffp-contract=off.
#pragma once
#include "common.h"

// check_pt_in_box3d_cpu (roiaware_pool3d.cpp:128-140): |z - cz| > dz / 2.0 rejects; the rectangle test compares
// fabs(local) with d / 2.0 + MARGIN in DOUBLE (MARGIN = (float)1e-2 promoted), local coordinates from fp32
// lidar_to_local_coords_cpu (cos / sin of -rz, no contraction).
__device__ __forceinline__ bool pt_in_box_cpu(float x, float y, float z, const float *q, float ca, float sa) {
    // q = cx, cy, cz, dx, dy, dz; ca / sa = cos / sin(-rz)
    if ((double)fabsf(z - q[2]) > (double)q[5] / 2.0) return false;
    const float sx = x - q[0], sy = y - q[1];
    const float lx = __fadd_rn(__fmul_rn(sx, ca), __fmul_rn(sy, -sa));
    const float ly = __fadd_rn(__fmul_rn(sx, sa), __fmul_rn(sy, ca));
    const double margin = (double)1e-2f;
    return (double)fabsf(lx) < (double)q[3] / 2.0 + margin && (double)fabsf(ly) < (double)q[4] / 2.0 + margin;
}

// Box j of a chunk staged for pt_in_box_cpu, CPD_BOX_LDS_FLOATS floats per box: [0..5] = centre and size, [6] / [7] = cos / sin(-rz);
// the rest is the caller's. The host libm's cosf / sinf are correctly rounded in all but rare cases; so is the double routine
// rounded to float.
#define CPD_BOX_LDS_FLOATS 12
#define CPD_BOX_LDS_CHUNK 512        // boxes staged at a time
__device__ __forceinline__ void stage_box_cpu(float *sbox, int j, const float *bq) {
    for (int q = 0; q < 6; ++q) sbox[12 * j + q] = bq[q];
    sbox[12 * j + 6] = (float)cos((double)(-bq[6]));
    sbox[12 * j + 7] = (float)sin((double)(-bq[6]));
}
