// tta_rules.h -- the rules of cpd_tta_collect (tta.hip): which candidate slot of the views' result blocks enters a (frame, class)
// segment, the key the segment is sorted by, and TestAugmentor.backward's arithmetic on a box (cpd/datasets/augmentor/
// test_augmentor.py), op by op in the host path's number formats (numpy >= 2: a Python float against a float32 array is a float32
// operation). __host__ __device__ like wbf_rules.h: the kernel and cpd_tta_collect_cpu (the host build of the same text, which the
// CPU tests hold to TestAugmentor.backward and wbf.build_segment_table) share it. Compile WITHOUT fp contraction.
#pragma once
#include "common.h"

#define TTA_HD __host__ __device__ __forceinline__

// the reversed op queue of one view as it acts on boxes
struct TtaBack {
    int n;
    int kind[CPD_AUG_MAX_OPS];
    float c[CPD_AUG_MAX_OPS], s[CPD_AUG_MAX_OPS];     // ROT: float32 cos / sin of -WORLD_ROT (the host's, from torch)
    float d[CPD_AUG_MAX_OPS];                         // ROT: float32(-WORLD_ROT); SCALE: float32(WORLD_SCALE)
};
struct TtaBackAll {
    TtaBack v[CPD_TTA_MAX_VIEWS];
};

// merge_detections.py:195-198: the class's boxes at or above its floor (float32 comparison; NaN: dropped); rows past the view's
// count are padding
TTA_HD bool tta_keep(int row, int count, long long label, float score, int cls, float floor) {
    return row < count && label == (long long)cls + 1 && score >= floor;
}

// np.argsort(-scores, kind="stable") as ONE ascending 64-bit key: the float32 -score mapped to an unsigned integer of the same
// order (-0.0 and 0.0 compare equal in numpy: both map to 0.0), then the candidate position
TTA_HD unsigned long long tta_sort_key(float score, unsigned int position) {
    float k = -score;
    if (k == 0.f) k = 0.f;
    unsigned int u;
    __builtin_memcpy(&u, &k, sizeof(u));
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((unsigned long long)u << 32) | position;
}
TTA_HD unsigned int tta_key_position(unsigned long long key) { return (unsigned int)(key & 0xffffffffull); }

// correctly rounded float32 quotient whatever the compiler makes of a float division (53 >= 2 * 24 + 2 bits)
TTA_HD float tta_div(float x, float y) { return (float)((double)x / (double)y); }

// TestAugmentor.backward on one box [7], the reversed queue in order:
//   world_scaling   boxes[:, 0:6] /= WORLD_SCALE                     float32 quotients by float32(scale)
//   world_rotation  rotate_points_along_z(boxes[:, 0:3], -WORLD_ROT); boxes[:, 6] += -WORLD_ROT
//                   x' = fl(fl(x c) + fl(y (-s))), y' = fl(fl(x s) + fl(y c)), z as it is (torch's host matmul may associate and
//                   fuse the two-term products differently: a few units in the last place of max(|x|, |y|))
//   world_flip      x: col 1 and col 6 = -(v + 0); y: col 0 = -(v + 0), col 6 = -(v + float32(pi))     (random_flip_with_param)
TTA_HD void tta_backward(const TtaBack &b, float *box) {
    for (int q = 0; q < b.n; ++q) {
        switch (b.kind[q]) {
        case CPD_AUG_FLIP_X:
            box[1] = -(box[1] + 0.f);
            box[6] = -(box[6] + 0.f);
            break;
        case CPD_AUG_FLIP_Y:
            box[0] = -(box[0] + 0.f);
            box[6] = -(box[6] + 3.141592653589793f);
            break;
        case CPD_AUG_ROT: {
            const float cs = b.c[q], sn = b.s[q], x = box[0], y = box[1];
            const float xc = x * cs, ys = y * (-sn), xs = x * sn, yc = y * cs;
            box[0] = xc + ys;
            box[1] = xs + yc;
            box[6] = box[6] + b.d[q];
            break;
        }
        default:
            for (int k = 0; k < 6; ++k) box[k] = tta_div(box[k], b.d[q]);
        }
    }
}
