// aug_ops.h -- the per-point op list of the augmentors (CPD_AUG_* of include/cpd_hip.h) and its arithmetic, shared by augment.hip
// (cpd_augment_scene) and tta.hip (cpd_tta_views): ONE device function, so that a view made by either is the same bits. Every
// file that includes it is compiled with -ffp-contract=off; the rotation is the one place where a fused multiply-add is written,
// explicitly: torch's CPU float32 matmul of [1, N, 3] x [1, 3, 3] evaluates fma(y, R[1][j], fl(x * R[0][j])) for all but tiny N.
#pragma once
#include "common.h"

struct AugOps {
    int n;
    int kind[CPD_AUG_MAX_OPS];
    float c[CPD_AUG_MAX_OPS], s[CPD_AUG_MAX_OPS];     // ROT: the host's float32 cos / sin
    float f[CPD_AUG_MAX_OPS];                         // SCALE: the factor rounded to float32
};

// HOST op_kind [n_ops] / op_param [n_ops][2] -> ops; CPD_ERR_ARG for an unknown kind (the caller has checked n_ops and the pointers)
static inline int aug_ops_fill(AugOps &ops, const int32_t *op_kind, const double *op_param, int n_ops) {
    for (int q = 0; q < n_ops; ++q) {
        if (op_kind[q] < CPD_AUG_FLIP_X || op_kind[q] > CPD_AUG_SCALE) return CPD_ERR_ARG;
        ops.kind[q] = op_kind[q];
        ops.c[q] = (float)op_param[2 * q];
        ops.s[q] = (float)op_param[2 * q + 1];
        ops.f[q] = (float)op_param[2 * q];
    }
    ops.n = n_ops;
    return CPD_OK;
}

__device__ __forceinline__ void aug_apply(const AugOps &ops, float &x, float &y, float &z) {
    for (int q = 0; q < ops.n; ++q) {
        switch (ops.kind[q]) {
        case CPD_AUG_FLIP_X: y = -y; break;
        case CPD_AUG_FLIP_Y: x = -x; break;
        case CPD_AUG_ROT: {
            const float cs = ops.c[q], sn = ops.s[q];
            const float nx = __fmaf_rn(y, -sn, __fmul_rn(x, cs));
            const float ny = __fmaf_rn(y, cs, __fmul_rn(x, sn));
            x = nx; y = ny;
            break;
        }
        default: {                                   // CPD_AUG_SCALE: points[:, :3] *= Python float, a float32 product
            const float f = ops.f[q];
            x = __fmul_rn(x, f); y = __fmul_rn(y, f); z = __fmul_rn(z, f);
        }
        }
    }
}
