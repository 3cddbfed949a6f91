// tta.hip -- test-time augmentation around an engine step, with no host wait and nothing read back:
//   * cpd_tta_views   = TestAugmentor.forward (cpd/datasets/augmentor/test_augmentor.py) of every view of a TEST_AUGMENTOR list on
//                       a packed batch in ONE launch: a point is read once and written once per view. The op arithmetic is
//                       cpd_augment_scene's own device function (aug_ops.h), so a view is the bits TestAugmentor.forward makes.
//   * cpd_tta_collect = TestAugmentor.backward on the views' result blocks + DetectionsMerger's per-class score floor and sort
//                       (cpd/datasets/kitti/kitti_object_eval_python/merge_detections.py:195-207): the floored, sorted,
//                       back-transformed segment table cpd_wbf_cluster / cpd_nms_batch take. One workgroup per (frame, class):
//                       ordered compaction of the kept candidate slots into LDS (wave ballot + prefix), a bitonic sort of 64-bit
//                       (score, position) keys in LDS, then the rows. Workgroups never talk to each other and every loop is
//                       bounded by V * K.
//   * cpd_tta_collect_cpu = the same rules (tta_rules.h) on the calling thread.
// Compiled with -ffp-contract=off like augment.hip (csrc/Makefile).
#include <algorithm>
#include <vector>

#include "aug_ops.h"
#include "tta_rules.h"

namespace {

#define TTA_BLOCK 1024
#define TTA_REG_COLS 5                   // columns 3 .. 3 + TTA_REG_COLS - 1 of a point stay in registers between the views

struct TtaViews {
    int n;
    AugOps ops[CPD_TTA_MAX_VIEWS];
};

__global__ void __launch_bounds__(256) tta_views_kernel(const float *__restrict__ points, long long n_total, int c, TtaViews vw,
                                                        float *__restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_total) return;
    const float *p = points + (size_t)i * c;
    const float x0 = p[0], y0 = p[1], z0 = p[2];
    float rest[TTA_REG_COLS];
#pragma unroll
    for (int q = 0; q < TTA_REG_COLS; ++q) rest[q] = 3 + q < c ? p[3 + q] : 0.f;
    for (int v = 0; v < vw.n; ++v) {
        float x = x0, y = y0, z = z0;
        aug_apply(vw.ops[v], x, y, z);
        float *o = out + ((size_t)v * (size_t)n_total + (size_t)i) * c;
        o[0] = x; o[1] = y; o[2] = z;
#pragma unroll
        for (int q = 0; q < TTA_REG_COLS; ++q)
            if (3 + q < c) o[3 + q] = rest[q];
        for (int q = 3 + TTA_REG_COLS; q < c; ++q) o[q] = p[q];
    }
}

struct TtaClasses {
    int n;
    float floor[CPD_TTA_MAX_CLASSES], iou[CPD_TTA_MAX_CLASSES];
    int mode[CPD_TTA_MAX_CLASSES];
};

struct TtaIn {
    const float *boxes;        // [V * B][K][7]
    const float *scores;       // [V * B][K]
    const int64_t *labels;     // [V * B][K], 1-based
    const int32_t *counts;     // [V * B]
    int n_views, batch, cap;
};
struct TtaOut {
    float *boxes, *scores;     // [S * V * K][7], [S * V * K]
    int32_t *src;              // [S * V * K] candidate position view * K + row
    int32_t *start, *count, *count_wbf, *count_nms, *mode;   // [S]
    float *thresh;             // [S][2]
};

// what does not depend on the rows: the segment's fixed start, its threshold pair and mode
TTA_HD void tta_segment_header(const TtaOut &o, const TtaClasses &cl, int seg, int c, long long vk) {
    o.start[seg] = (int32_t)((long long)seg * vk);
    o.thresh[2 * seg] = cl.iou[c];
    o.thresh[2 * seg + 1] = 0.f;
    o.mode[seg] = cl.mode[c];
}
// the counts: the segment's, and the same split by consumer (cpd_wbf_cluster reads count_wbf, cpd_nms_batch count_nms); a segment
// above CPD_WBF_MAX_SEGMENT is refused with cpd_wbf_cluster's -1
TTA_HD void tta_segment_counts(const TtaOut &o, const TtaClasses &cl, int seg, int c, int count) {
    const bool refused = count > CPD_WBF_MAX_SEGMENT, nms = cl.mode[c] < 0;
    o.count[seg] = refused ? -1 : count;
    o.count_wbf[seg] = refused ? -1 : (nms ? 0 : count);
    o.count_nms[seg] = (refused || !nms) ? 0 : count;
}
// sorted row r of a segment <- candidate position `pos` of frame f
TTA_HD void tta_write_row(const TtaIn &in, const TtaOut &o, const TtaBackAll &back, int f, size_t dst, unsigned int pos) {
    const int v = (int)(pos / (unsigned int)in.cap), row = (int)(pos % (unsigned int)in.cap);
    const size_t at = ((size_t)v * in.batch + f) * in.cap + row;
    float box[7];
    for (int k = 0; k < 7; ++k) box[k] = in.boxes[7 * at + k];
    tta_backward(back.v[v], box);
    for (int k = 0; k < 7; ++k) o.boxes[7 * dst + k] = box[k];
    o.scores[dst] = in.scores[at];
    o.src[dst] = (int32_t)pos;
}

__global__ void __launch_bounds__(TTA_BLOCK) tta_collect_kernel(TtaIn in, TtaBackAll back, TtaClasses cl, TtaOut o) {
    __shared__ unsigned long long s_key[CPD_WBF_MAX_SEGMENT];
    __shared__ int s_wave[TTA_BLOCK / 64];
    const int seg = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int f = seg / cl.n, c = seg % cl.n;
    const long long vk = (long long)in.n_views * in.cap;
    const float floor = cl.floor[c];
    // 1. the kept slots, compacted in candidate order
    int total = 0;                                               // block-uniform
    for (long long base = 0; base < vk; base += TTA_BLOCK) {
        const long long p = base + tid;
        bool keep = false;
        float score = 0.f;
        if (p < vk) {
            const int v = (int)(p / in.cap), row = (int)(p % in.cap);
            const size_t blk = (size_t)v * in.batch + f;
            const int n_rows = in.counts[blk];
            if (row < n_rows) {                                  // (padding rows are not read: stale allocator bytes)
                score = in.scores[blk * in.cap + row];
                keep = tta_keep(row, n_rows, in.labels[blk * in.cap + row], score, c, floor);
            }
        }
        const unsigned long long vote = __ballot(keep);
        if (lane == 0) s_wave[wave] = __popcll(vote);
        __syncthreads();
        int before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < TTA_BLOCK / 64; ++w) {
            const int t = s_wave[w];
            before += w < wave ? t : 0;
            all += t;
        }
        if (keep) {
            const int dst = total + before + __popcll(vote & ((1ull << lane) - 1ull));
            if (dst < CPD_WBF_MAX_SEGMENT) s_key[dst] = tta_sort_key(score, (unsigned int)p);
        }
        total += all;
        __syncthreads();                                         // s_wave is rewritten by the next turn
    }
    if (tid == 0) {
        tta_segment_header(o, cl, seg, c, vk);
        tta_segment_counts(o, cl, seg, c, total);
    }
    if (total == 0 || total > CPD_WBF_MAX_SEGMENT) return;
    // 2. ascending bitonic sort of the keys, padded to a power of two with the largest key
    int n2 = 1;
    while (n2 < total) n2 <<= 1;
    for (int i = total + tid; i < n2; i += TTA_BLOCK) s_key[i] = ~0ull;
    __syncthreads();
    for (int k = 2; k <= n2; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (n2 >> 1); t += TTA_BLOCK) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), ij = i | j;
                const unsigned long long a = s_key[i], b = s_key[ij];
                if (((i & k) == 0) == (a > b)) {
                    s_key[i] = b;
                    s_key[ij] = a;
                }
            }
            __syncthreads();
        }
    }
    // 3. the rows
    const size_t first = (size_t)seg * (size_t)vk;
    for (int r = tid; r < total; r += TTA_BLOCK) tta_write_row(in, o, back, f, first + r, tta_key_position(s_key[r]));
}

// HOST kind [V][MAX_OPS] / param [V][MAX_OPS][3] / n [V] -> back
int tta_back_fill(TtaBackAll &back, const int32_t *kind, const double *param, const int32_t *n_back, int n_views) {
    for (int v = 0; v < n_views; ++v) {
        if (n_back[v] < 0 || n_back[v] > CPD_AUG_MAX_OPS) return CPD_ERR_ARG;
        TtaBack &b = back.v[v];
        b.n = n_back[v];
        for (int q = 0; q < b.n; ++q) {
            const int kd = kind[v * CPD_AUG_MAX_OPS + q];
            const double *pp = param + 3 * ((size_t)v * CPD_AUG_MAX_OPS + q);
            if (kd < CPD_AUG_FLIP_X || kd > CPD_AUG_SCALE) return CPD_ERR_ARG;
            if (kd == CPD_AUG_SCALE && (float)pp[0] == 0.f) return CPD_ERR_ARG;
            b.kind[q] = kd;
            b.c[q] = (float)pp[0];
            b.s[q] = (float)pp[1];
            b.d[q] = kd == CPD_AUG_ROT ? (float)pp[2] : (float)pp[0];
        }
    }
    return CPD_OK;
}

int tta_collect_args(const float *boxes, const float *scores, const int64_t *labels, const int32_t *counts, int n_views, int batch, int cap,
                     const int32_t *back_kind, const double *back_param, const int32_t *n_back, const float *cls_floor,
                     const float *cls_iou, const int32_t *cls_mode, int n_class, float *out_boxes, float *out_scores, int32_t *out_src,
                     int32_t *seg_start, int32_t *seg_count, int32_t *seg_count_wbf, int32_t *seg_count_nms, float *seg_thresh,
                     int32_t *seg_mode, TtaIn &in, TtaBackAll &back, TtaClasses &cl, TtaOut &o) {
    if (n_views < 1 || n_views > CPD_TTA_MAX_VIEWS || batch < 0 || cap < 0 || n_class < 0 || n_class > CPD_TTA_MAX_CLASSES) return CPD_ERR_ARG;
    if (!back_kind || !back_param || !n_back || (n_class > 0 && (!cls_floor || !cls_iou || !cls_mode))) return CPD_ERR_ARG;
    const long long n_seg = (long long)batch * n_class, vk = (long long)n_views * cap;
    if (n_seg * vk >= (1ll << 31) || vk >= (1ll << 31) || (long long)n_views * batch >= (1ll << 31)) return CPD_ERR_ARG;
    if (n_seg > 0 && (!counts || !seg_start || !seg_count || !seg_count_wbf || !seg_count_nms || !seg_thresh || !seg_mode)) return CPD_ERR_ARG;
    if (n_seg * vk > 0 && (!boxes || !scores || !labels || !out_boxes || !out_scores || !out_src)) return CPD_ERR_ARG;
    const int rc = tta_back_fill(back, back_kind, back_param, n_back, n_views);
    if (rc != CPD_OK) return rc;
    cl.n = n_class;
    for (int c = 0; c < n_class; ++c) {
        cl.floor[c] = cls_floor[c];
        cl.iou[c] = cls_iou[c];
        cl.mode[c] = cls_mode[c];
    }
    in = TtaIn{boxes, scores, labels, counts, n_views, batch, cap};
    o = TtaOut{out_boxes, out_scores, out_src, seg_start, seg_count, seg_count_wbf, seg_count_nms, seg_mode, seg_thresh};
    return CPD_OK;
}

}  // namespace

extern "C" int cpd_tta_views(const float *points, long long n_total, int c, const int64_t *frame_offsets, int batch, const int32_t *op_kind,
                             const double *op_param, const int32_t *n_ops, int n_views, float *out, cpd_stream_t stream) {
    if (n_total < 0 || c < 3 || batch < 0 || n_views < 1 || n_views > CPD_TTA_MAX_VIEWS || !frame_offsets || !op_kind || !op_param || !n_ops)
        return CPD_ERR_ARG;
    if ((long long)n_views * n_total >= (1ll << 31)) return CPD_ERR_ARG;
    if (frame_offsets[0] != 0 || frame_offsets[batch] != n_total) return CPD_ERR_ARG;
    for (int f = 0; f < batch; ++f)
        if (frame_offsets[f + 1] < frame_offsets[f]) return CPD_ERR_ARG;
    TtaViews vw{};
    vw.n = n_views;
    for (int v = 0; v < n_views; ++v) {
        if (n_ops[v] < 0 || n_ops[v] > CPD_AUG_MAX_OPS) return CPD_ERR_ARG;
        if (aug_ops_fill(vw.ops[v], op_kind + (size_t)v * CPD_AUG_MAX_OPS, op_param + 2 * (size_t)v * CPD_AUG_MAX_OPS, n_ops[v]) != CPD_OK)
            return CPD_ERR_ARG;
    }
    if (n_total == 0) return CPD_OK;
    if (!points || !out) return CPD_ERR_ARG;
    tta_views_kernel<<<cpd_div_up(n_total, 256), 256, 0, cpd_s(stream)>>>(points, n_total, c, vw, out);
    return cpd_check_launch();
}

extern "C" int cpd_tta_collect(const float *boxes, const float *scores, const int64_t *labels, const int32_t *counts, int n_views, int batch,
                               int cap, const int32_t *back_kind, const double *back_param, const int32_t *n_back, const float *cls_floor,
                               const float *cls_iou, const int32_t *cls_mode, int n_class, float *out_boxes, float *out_scores,
                               int32_t *out_src, int32_t *seg_start, int32_t *seg_count, int32_t *seg_count_wbf, int32_t *seg_count_nms,
                               float *seg_thresh, int32_t *seg_mode, cpd_stream_t stream) {
    TtaIn in;
    TtaBackAll back{};
    TtaClasses cl{};
    TtaOut o;
    const int rc = tta_collect_args(boxes, scores, labels, counts, n_views, batch, cap, back_kind, back_param, n_back, cls_floor, cls_iou,
                                    cls_mode, n_class, out_boxes, out_scores, out_src, seg_start, seg_count, seg_count_wbf, seg_count_nms,
                                    seg_thresh, seg_mode, in, back, cl, o);
    if (rc != CPD_OK) return rc;
    if (batch * n_class == 0) return CPD_OK;
    tta_collect_kernel<<<batch * n_class, TTA_BLOCK, 0, cpd_s(stream)>>>(in, back, cl, o);
    return cpd_check_launch();
}

extern "C" int cpd_tta_collect_cpu(const float *boxes, const float *scores, const int64_t *labels, const int32_t *counts, int n_views, int batch,
                                   int cap, const int32_t *back_kind, const double *back_param, const int32_t *n_back, const float *cls_floor,
                                   const float *cls_iou, const int32_t *cls_mode, int n_class, float *out_boxes, float *out_scores,
                                   int32_t *out_src, int32_t *seg_start, int32_t *seg_count, int32_t *seg_count_wbf, int32_t *seg_count_nms,
                                   float *seg_thresh, int32_t *seg_mode) {
    TtaIn in;
    TtaBackAll back{};
    TtaClasses cl{};
    TtaOut o;
    const int rc = tta_collect_args(boxes, scores, labels, counts, n_views, batch, cap, back_kind, back_param, n_back, cls_floor, cls_iou,
                                    cls_mode, n_class, out_boxes, out_scores, out_src, seg_start, seg_count, seg_count_wbf, seg_count_nms,
                                    seg_thresh, seg_mode, in, back, cl, o);
    if (rc != CPD_OK) return rc;
    const long long vk = (long long)n_views * cap;
    std::vector<unsigned long long> keys;
    for (int seg = 0; seg < batch * n_class; ++seg) {
        const int f = seg / n_class, c = seg % n_class;
        keys.clear();
        for (long long p = 0; p < vk; ++p) {
            const int v = (int)(p / cap), row = (int)(p % cap);
            const size_t blk = (size_t)v * batch + f;
            if (row >= counts[blk]) continue;
            const float score = scores[blk * cap + row];
            if (tta_keep(row, counts[blk], labels[blk * cap + row], score, c, cl.floor[c])) keys.push_back(tta_sort_key(score, (unsigned int)p));
        }
        tta_segment_header(o, cl, seg, c, vk);
        tta_segment_counts(o, cl, seg, c, (int)keys.size());
        if (keys.size() > CPD_WBF_MAX_SEGMENT) continue;
        std::sort(keys.begin(), keys.end());                     // (the keys are distinct: the position is part of them)
        for (size_t r = 0; r < keys.size(); ++r) tta_write_row(in, o, back, f, (size_t)seg * (size_t)vk + r, tta_key_position(keys[r]));
    }
    return CPD_OK;
}
