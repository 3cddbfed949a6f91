// roi_targets.hip -- the RoI head's proposal-target layer on the device, for gfx950.
//
// Replaces the per-frame / per-class Python loops of ProposalTargetLayer (cpd/models/roi_heads/target_assigner/
// proposal_target_layer.py:32-427: forward, sample_rois_for_rcnn, subsample_rois' pools, get_max_iou_with_same_class) and the torch
// chain of RoIHeadTemplate.assign_targets (cpd/models/roi_heads/roi_head_template.py:116-146) by two launches:
//
//   roi_targets_classify_kernel  one workgroup of RT_THREADS per frame. It trims the frame's ground truth with recall_kernel's rule,
//       then takes the kept rows 64 at a time: lane = ground-truth row (its BoxG stays in registers), the waves deal the RoIs out, and
//       a butterfly over the lanes yields the row's maximum of iou3d_g (box_geom.h: the bits of a cpd_boxes_iou3d entry) and the LOWEST
//       row that attains it; any number of rows and RoIs. Then thread = RoI: the three sampling pools come out as ascending index
//       lists by ballot + prefix over the waves: no atomic decides a position.
//   roi_targets_gather_kernel    one thread per sampled slot: the host's pick (pool, position) -> RoI index -> every gathered row
//       and every target derived from it (reg_valid_mask, rcnn_cls_labels for all five CLS_SCORE_TYPEs, the canonical gt_of_rois).
//
// The random numbers stay on the host (equal seeds give the reference's samples): between the two launches the host reads the
// pools' lengths back, draws, and uploads the pick table.
//
// This file is compiled with the flags of iou3d_nms.hip, so that box_overlap_g rounds here as it does there. The target arithmetic of
// the gather kernel must round as torch's fp32 kernels do, one operation at a time: everything below the classify kernel is compiled
// with contraction off (the pragma further down; HIP's __f*_rn are plain operators and would contract); the two products of the
// rotation fuse by explicit fmaf.
#include <math.h>

#include "box_geom.h"
#include "common.h"

namespace {

enum { RT_THREADS = 512, RT_WAVES = RT_THREADS / 64, RT_MAX_CLASSES = CPD_ROI_TARGETS_MAX_CLASSES };

// pool thresholds as float (torch compares the fp32 overlaps with the scalar cast to fp32). n == 0: scalar thresholds in [0];
// n > 0: per-class lists, entry c for an assigned ground truth of class c + 1.
struct RtPools {
    float fg[RT_MAX_CLASSES];    // min(REG_FG_THRESH, CLS_FG_THRESH)
    float reg[RT_MAX_CLASSES];   // REG_FG_THRESH
    float lo;                    // CLS_BG_THRESH_LO
    int n;
};

// the pieces of the workspace: five [batch][n] arrays of 4-byte words, each piece 256-byte aligned
struct RtWs {
    float *overlaps;
    int32_t *assign;
    int32_t *lists;              // piece 2, 3, 4 = fg, hard, easy: pool p of frame b at lists + p * stride + b * n
    size_t stride;               // words between two pools' pieces
};
static RtWs rt_carve(void *ws, int batch, int n, size_t *total) {     // (RtWs is a kernel argument: the total stays out of it)
    const size_t piece = (size_t)batch * n * 4;
    Carve c;
    RtWs w;
    w.overlaps = ws_at<float>(ws, c.take(piece));
    w.assign = ws_at<int32_t>(ws, c.take(piece));
    const size_t fg = c.take(piece), hard = c.take(piece);
    c.take(piece);                                                    // easy
    w.lists = ws_at<int32_t>(ws, fg);
    w.stride = (hard - fg) / 4;
    *total = c.o;
    return w;
}

// torch.max(dim=1) between two candidates (value, row; row < 0: none): is `a` the one to keep? A NaN wins, then the larger value,
// then the lower row.
__device__ __forceinline__ bool rt_better(float av, int ai, float bv, int bi) {
    if (ai < 0) return false;
    if (bi < 0) return true;
    const bool an = av != av, bn = bv != bv;
    if (an || bn) return an && (!bn || ai < bi);
    return av > bv || (av == bv && ai < bi);
}

__global__ void __launch_bounds__(RT_THREADS) roi_targets_classify_kernel(
        const float *__restrict__ rois, const long long *__restrict__ roi_labels, int n, const float *__restrict__ gt, int m, int gt_ld,
        int by_class, RtPools th, RtWs ws, int32_t *__restrict__ counts) {
    __shared__ int s_last;
    __shared__ int s_wave[3][RT_WAVES];
    __shared__ int s_base[3];
    __shared__ RtPools s_th;                                  // (indexed by the lane in phase 2)
    const int frame = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const float *g = gt + (size_t)frame * m * gt_ld;
    // rows 0 .. k of the frame count, k the last row whose fp32 sum over all columns is not zero (recall_kernel's rule for the same
    // reference idiom, proposal_target_layer.py:221-225)
    if (tid == 0) s_last = 0;
    if (tid < 3) s_base[tid] = 0;
    if (tid == 64) s_th = th;
    __syncthreads();
    for (int r = tid; r < m; r += RT_THREADS) {
        float sum = 0.f;
#pragma unroll 1
        for (int c = 0; c < gt_ld; ++c) sum += g[(size_t)r * gt_ld + c];
        if (!(sum == 0.f)) atomicMax(&s_last, r);
    }
    __syncthreads();
    const int rows = s_last + 1;
    const float *frame_rois = rois + (size_t)frame * n * 7;
    const long long *frame_labels = roi_labels + (size_t)frame * n;
    float *best_of = ws.overlaps + (size_t)frame * n;
    int32_t *row_of = ws.assign + (size_t)frame * n;
    // phase 1, pairwise_kernel's loop: lane = ground-truth row (its BoxG set up once and kept in registers), the waves deal the RoIs
    // out and set each one up from a wave-uniform address (scalar loads). The overlap is the float cpd_boxes_iou3d stores: iou3d_g
    // keeps its own operations from contracting (box_geom.h) and box_overlap_g is compiled with the same flags in the same roles.
    // A butterfly leaves the RoI's best in every lane; lane 0 keeps it.
#pragma unroll 1
    for (int t0 = 0; t0 < rows; t0 += 64) {
        const int col = t0 + lane;
        const bool colok = col < rows;
        const float *brow = g + (size_t)(colok ? col : 0) * gt_ld;
        BoxG B;
        box_setup(brow, B);
        const long long cls = (long long)brow[gt_ld - 1];     // `.long()` truncates
#pragma unroll 1
        for (int row = wave; row < n; row += RT_WAVES) {
            BoxG A;
            box_setup(frame_rois + 7 * (size_t)row, A);
            float v = iou3d_g(A, B);
            int at = colok && (!by_class || cls == frame_labels[row]) ? col : -1;
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) {
                const float ov = __shfl_xor(v, d, 64);
                const int oat = __shfl_xor(at, d, 64);
                if (rt_better(ov, oat, v, at)) {
                    v = ov;
                    at = oat;
                }
            }
            if (lane == 0 && (t0 == 0 || rt_better(v, at, best_of[row], row_of[row]))) {   // (a RoI stays with one wave: program order)
                best_of[row] = v;
                row_of[row] = at;
            }
        }
    }
    __syncthreads();
    // phase 2, thread = RoI: no row of its class -> overlap 0 and row 0; the pools; the stable compaction
    const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll 1
    for (int base = 0; base < n; base += RT_THREADS) {
        const int r = base + tid;
        const bool ok = r < n;
        int arg = ok ? row_of[r] : 0;
        const float best = ok && arg >= 0 ? best_of[r] : 0.f;
        arg = arg < 0 ? 0 : arg;
        bool in_fg = false, in_hard = false;
        const bool in_easy = best < s_th.lo;
        if (s_th.n == 0) {
            in_fg = best >= s_th.fg[0];
            in_hard = best < s_th.reg[0] && best >= s_th.lo;
        } else {
            // entry c serves class c + 1, when the assigned row's class is exactly that integer
            const float cls = g[(size_t)arg * gt_ld + gt_ld - 1];
            const int c = (int)cls - 1;
            if (c >= 0 && c < s_th.n && cls == (float)(c + 1)) {
                in_fg = best >= s_th.fg[c];
                in_hard = best < s_th.reg[c] && best >= s_th.lo;
            }
        }
        if (ok) {
            best_of[r] = best;
            row_of[r] = arg;
        }
        // a RoI's position = RoIs of earlier chunks + earlier waves + lower lanes that are in the pool
        const unsigned long long b0 = __ballot(ok && in_fg), b1 = __ballot(ok && in_hard), b2 = __ballot(ok && in_easy);
        if (lane == 0) {
            s_wave[0][wave] = __popcll(b0);
            s_wave[1][wave] = __popcll(b1);
            s_wave[2][wave] = __popcll(b2);
        }
        __syncthreads();
        int o0 = s_base[0], o1 = s_base[1], o2 = s_base[2];
#pragma unroll
        for (int w = 0; w < RT_WAVES; ++w) {
            o0 += w < wave ? s_wave[0][w] : 0;
            o1 += w < wave ? s_wave[1][w] : 0;
            o2 += w < wave ? s_wave[2][w] : 0;
        }
        int32_t *lst = ws.lists + (size_t)frame * n;
        if (ok && in_fg) lst[o0 + __popcll(b0 & below)] = r;
        if (ok && in_hard) lst[ws.stride + o1 + __popcll(b1 & below)] = r;
        if (ok && in_easy) lst[2 * ws.stride + o2 + __popcll(b2 & below)] = r;
        __syncthreads();
        if (tid < 3) {
            int t = s_base[tid];
            for (int w = 0; w < RT_WAVES; ++w) t += s_wave[tid][w];
            s_base[tid] = t;
        }
        __syncthreads();
    }
    if (tid < 3) counts[frame * 4 + tid] = s_base[tid];
    if (tid == 3) counts[frame * 4 + 3] = rows;
}

// ---- the gather kernel's arithmetic: torch's fp32 kernels, one rounding per operation ----
#pragma clang fp contract(off)
#define RT_TWO_PI ((float)6.283185307179586)       // float(2 * np.pi)
#define RT_PI ((float)3.141592653589793)
#define RT_HALF_PI ((float)1.5707963267948966)     // float(np.pi * 0.5) = float(np.pi / 2)
#define RT_THREE_HALF_PI ((float)4.71238898038469) // float(np.pi * 1.5)

__device__ __forceinline__ float rt_remainder(float a, float b) {          // torch.remainder: fmod, then the divisor's sign
    float r = fmodf(a, b);
    if (r != 0.f && ((b < 0.f) != (r < 0.f))) r = __fadd_rn(r, b);
    return r;
}
__device__ __forceinline__ float rt_limit(float a) {                       // bbloss.limit (bbloss.py:4-11)
    a = rt_remainder(a, RT_TWO_PI);
    a = a > RT_PI ? __fsub_rn(a, RT_TWO_PI) : a;
    return a < -RT_PI ? __fadd_rn(a, RT_TWO_PI) : a;
}

struct RtScore {
    int kind;                           // CPD_ROI_SCORE_*
    int n_cls;                          // entries of the lists below (1 for the scalar kinds)
    float reg_fg[RT_MAX_CLASSES], cls_fg[RT_MAX_CLASSES], cls_bg[RT_MAX_CLASSES];
    float cls_inv_span[RT_MAX_CLASSES]; // float(1 / (fg - bg)), formed in double
    float hard_thresh[RT_MAX_CLASSES];
    int hard_every[RT_MAX_CLASSES];     // 0: no hard sampling for this class
    int hard_offset[RT_MAX_CLASSES];
    float dir_min, dir_max, dir_inv_span;   // DIRECTION_MIN / MAX and float(1 / (max - min)), formed in double
};
struct RtExtras {
    const float *in[3];
    float *out[3];
};

// torch divides a device tensor by a host scalar as a product with the scalar's reciprocal, formed in double and cast to float:
// the callers pass that reciprocal
#define RT_INV_PI ((float)0.3183098861837907)     // float(1 / np.pi)

__device__ __forceinline__ float rt_soft_label(float iou, float fg_t, float bg_t, float inv_span) {     // l.100-107 / 162-172
    const bool fg = iou > fg_t, bg = iou < bg_t;
    if (!fg && !bg) return __fmul_rn(__fsub_rn(iou, bg_t), inv_span);
    return fg ? 1.f : 0.f;
}

__global__ void __launch_bounds__(256) roi_targets_gather_kernel(
        const float *__restrict__ rois, const long long *__restrict__ roi_labels, const float *__restrict__ roi_scores, int n,
        const float *__restrict__ gt, int m, int gt_ld, RtExtras ex, const int32_t *__restrict__ picks, int per_image, RtWs ws,
        const int32_t *__restrict__ counts, RtScore sc, float *__restrict__ out_rois, long long *__restrict__ out_labels,
        float *__restrict__ out_scores, float *__restrict__ out_iou, float *__restrict__ out_src, float *__restrict__ out_gt,
        long long *__restrict__ out_reg_valid, void *__restrict__ out_cls_labels) {
    const int slot = blockIdx.x * blockDim.x + threadIdx.x;
    const int frame = blockIdx.y;
    if (slot >= per_image) return;
    const size_t o = (size_t)frame * per_image + slot;
    const int pool = picks[2 * o], pos = picks[2 * o + 1];
    int r = 0;                                              // (a pick outside its pool reads RoI 0: nothing out of bounds)
    if (pool >= 0 && pool < 3 && pos >= 0 && pos < counts[frame * 4 + pool]) r = ws.lists[pool * ws.stride + (size_t)frame * n + pos];
    r = r < 0 || r >= n ? 0 : r;
    const size_t ri = (size_t)frame * n + r;
    int a = ws.assign[ri];
    a = a < 0 || a >= m ? 0 : a;
    const float iou = ws.overlaps[ri];
    const float *roi = rois + ri * 7;
    const float *src = gt + ((size_t)frame * m + a) * gt_ld;
    float *o_roi = out_rois + o * 7, *o_src = out_src + o * gt_ld, *o_gt = out_gt ? out_gt + o * gt_ld : nullptr;
    float q[7];
#pragma unroll
    for (int c = 0; c < 7; ++c) o_roi[c] = q[c] = roi[c];
    for (int c = 0; c < gt_ld; ++c) o_src[c] = src[c];
    out_labels[o] = roi_labels[ri];
    out_scores[o] = roi_scores[ri];
    out_iou[o] = iou;
#pragma unroll
    for (int k = 0; k < 3; ++k)
        if (ex.in[k]) ex.out[k][o] = ex.in[k][(size_t)frame * m + a];

    // reg_valid_mask and rcnn_cls_labels (proposal_target_layer.py:57-196)
    const float gt_cls = src[gt_ld - 1];
    const bool per_class = sc.kind == CPD_ROI_SCORE_ROI_IOU_X || sc.kind == CPD_ROI_SCORE_ROI_IOUD_X;
    const bool directed = sc.kind == CPD_ROI_SCORE_ROI_IOUD || sc.kind == CPD_ROI_SCORE_ROI_IOUD_X;
    float dw = 1.f;
    if (directed) {
        const float d = fabsf(__fsub_rn(rt_limit(q[6]), rt_limit(src[6])));
        const float w = __fsub_rn(1.f, __fmul_rn(fminf(d, __fsub_rn(RT_TWO_PI, d)), RT_INV_PI));
        dw = __fmul_rn(__fsub_rn(fminf(fmaxf(w, sc.dir_min), sc.dir_max), sc.dir_min), sc.dir_inv_span);
    }
    long long valid = 0;
    float lab = 0.f;
    if (per_class) {
#pragma unroll
        for (int c = 0; c < RT_MAX_CLASSES; ++c) {
            if (c >= sc.n_cls || !(gt_cls == (float)(c + 1))) continue;
            valid += iou > sc.reg_fg[c] ? 1 : 0;
            // ENABLE_HARD_SAMPLING switches whole BATCH rows on: rows offset, offset + every, ... (l.66-72)
            const bool on = sc.hard_every[c] > 0 && frame >= sc.hard_offset[c] && (frame - sc.hard_offset[c]) % sc.hard_every[c] == 0;
            valid += (on && iou < sc.reg_fg[c] && iou > sc.hard_thresh[c]) ? 1 : 0;
            lab = rt_soft_label(iou, sc.cls_fg[c], sc.cls_bg[c], sc.cls_inv_span[c]);
            if (directed) lab = __fmul_rn(lab, dw);
        }
    } else {
        valid = iou > sc.reg_fg[0] ? 1 : 0;
        if (sc.kind == CPD_ROI_SCORE_CLS) {
            lab = (iou > sc.cls_bg[0] && iou < sc.cls_fg[0]) ? -1.f : (iou > sc.cls_fg[0] ? 1.f : 0.f);
        } else {
            lab = rt_soft_label(iou, sc.cls_fg[0], sc.cls_bg[0], sc.cls_inv_span[0]);
            if (directed) lab = __fmul_rn(lab, dw);
        }
    }
    out_reg_valid[o] = valid;
    if (sc.kind == CPD_ROI_SCORE_CLS) static_cast<long long *>(out_cls_labels)[o] = (long long)lab;
    else static_cast<float *>(out_cls_labels)[o] = lab;
    if (!o_gt) return;

    // the ground truth in the RoI's canonical frame (roi_head_template.py:124-145)
    const float ry = rt_remainder(q[6], RT_TWO_PI);
    const float x = __fsub_rn(src[0], q[0]), y = __fsub_rn(src[1], q[1]), z = __fsub_rn(src[2], q[2]);
    const float ca = cosf(-ry), sa = sinf(-ry);            // rotate_points_along_z(gt, -ry): [x y z] x [[c, s, 0], [-s, c, 0], [0, 0, 1]]
    o_gt[0] = fmaf(y, -sa, __fmul_rn(x, ca));
    o_gt[1] = fmaf(y, ca, __fmul_rn(x, sa));
    o_gt[2] = z;
    float h = rt_remainder(__fsub_rn(src[6], ry), RT_TWO_PI);
    if (h > RT_HALF_PI && h < RT_THREE_HALF_PI) h = rt_remainder(__fadd_rn(h, RT_PI), RT_TWO_PI);     // the opposite-facing half turn
    h = h > RT_PI ? __fsub_rn(h, RT_TWO_PI) : h;
    h = fminf(fmaxf(h, -RT_HALF_PI), RT_HALF_PI);
    for (int c = 3; c < gt_ld; ++c) o_gt[c] = c == 6 ? h : src[c];
}

}  // namespace

extern "C" size_t cpd_roi_targets_workspace_bytes(int batch, int n) {
    if (batch <= 0 || n <= 0) return 0;
    size_t total;
    rt_carve(nullptr, batch, n, &total);
    return total;
}

extern "C" int cpd_roi_targets_classify(const float *rois, const int64_t *roi_labels, int batch, int n, const float *gt_boxes, int m, int gt_ld,
                                        int by_class, const float *fg_thresh, const float *reg_thresh, int n_thresh, float bg_thresh_lo,
                                        int32_t *counts, void *ws, size_t ws_bytes, cpd_stream_t stream) {
    if (batch <= 0 || batch > 65535 || n <= 0 || m <= 0 || gt_ld < 7 || !rois || !roi_labels || !gt_boxes || !fg_thresh || !reg_thresh || !counts ||
        n_thresh < 0)
        return CPD_ERR_ARG;
    if (n_thresh > RT_MAX_CLASSES) return CPD_ERR_UNSUPPORTED;
    size_t need;
    const RtWs pieces = rt_carve(ws, batch, n, &need);
    if (!ws || ws_bytes < need) return CPD_ERR_WORKSPACE;
    RtPools th = {};
    for (int c = 0; c < (n_thresh ? n_thresh : 1); ++c) {
        th.fg[c] = fg_thresh[c];
        th.reg[c] = reg_thresh[c];
    }
    th.lo = bg_thresh_lo;
    th.n = n_thresh;
    roi_targets_classify_kernel<<<batch, RT_THREADS, 0, cpd_s(stream)>>>(rois, reinterpret_cast<const long long *>(roi_labels), n, gt_boxes, m,
                                                                         gt_ld, by_class != 0, th, pieces, counts);
    cpd_launch_log_note("roi_targets_classify_kernel");
    return cpd_check_launch();
}

extern "C" int cpd_roi_targets_gather(const float *rois, const int64_t *roi_labels, const float *roi_scores, int batch, int n,
                                      const float *gt_boxes, int m, int gt_ld, const float *const extras_in[3], const int32_t *picks,
                                      int per_image, const int32_t *counts, const void *ws, size_t ws_bytes, int score_type, int n_cls,
                                      const float *reg_fg_thresh, const float *cls_fg_thresh, const float *cls_bg_thresh,
                                      const float *cls_inv_span, const float *hard_thresh, const int32_t *hard_every,
                                      const int32_t *hard_offset, const float direction[3], float *out_rois, int64_t *out_roi_labels,
                                      float *out_roi_scores, float *out_gt_iou, float *out_gt_src, float *out_gt_canonical,
                                      int64_t *out_reg_valid, void *out_cls_labels, float *const extras_out[3], cpd_stream_t stream) {
    if (batch <= 0 || batch > 65535 || n <= 0 || m <= 0 || gt_ld < 7 || per_image <= 0 || !rois || !roi_labels || !roi_scores || !gt_boxes ||
        !picks || !counts || !reg_fg_thresh || !cls_fg_thresh || !cls_bg_thresh || !cls_inv_span || !out_rois || !out_roi_labels ||
        !out_roi_scores || !out_gt_iou || !out_gt_src || !out_reg_valid || !out_cls_labels || n_cls < 1)
        return CPD_ERR_ARG;
    if (score_type < CPD_ROI_SCORE_CLS || score_type > CPD_ROI_SCORE_ROI_IOUD_X) return CPD_ERR_ARG;
    const bool directed = score_type == CPD_ROI_SCORE_ROI_IOUD || score_type == CPD_ROI_SCORE_ROI_IOUD_X;
    const bool per_class = score_type == CPD_ROI_SCORE_ROI_IOU_X || score_type == CPD_ROI_SCORE_ROI_IOUD_X;
    if ((directed && !direction) || (!per_class && n_cls != 1)) return CPD_ERR_ARG;
    if (n_cls > RT_MAX_CLASSES) return CPD_ERR_UNSUPPORTED;
    size_t need;
    const RtWs pieces = rt_carve(const_cast<void *>(ws), batch, n, &need);
    if (!ws || ws_bytes < need) return CPD_ERR_WORKSPACE;
    RtScore sc = {};
    sc.kind = score_type;
    sc.n_cls = n_cls;
    for (int c = 0; c < n_cls; ++c) {
        sc.reg_fg[c] = reg_fg_thresh[c];
        sc.cls_fg[c] = cls_fg_thresh[c];
        sc.cls_bg[c] = cls_bg_thresh[c];
        sc.cls_inv_span[c] = cls_inv_span[c];
        const bool hard = per_class && hard_thresh && hard_every && hard_offset && hard_every[c] > 0;
        sc.hard_thresh[c] = hard ? hard_thresh[c] : 0.f;
        sc.hard_every[c] = hard ? hard_every[c] : 0;
        sc.hard_offset[c] = hard ? hard_offset[c] : 0;
    }
    if (directed) {
        sc.dir_min = direction[0];
        sc.dir_max = direction[1];
        sc.dir_inv_span = direction[2];
    }
    RtExtras ex = {};
    for (int k = 0; k < 3; ++k) {
        ex.in[k] = extras_in ? extras_in[k] : nullptr;
        ex.out[k] = extras_out ? extras_out[k] : nullptr;
        if (ex.in[k] && !ex.out[k]) return CPD_ERR_ARG;
    }
    dim3 grid(cpd_div_up(per_image, 256), batch);
    roi_targets_gather_kernel<<<grid, 256, 0, cpd_s(stream)>>>(
        rois, reinterpret_cast<const long long *>(roi_labels), roi_scores, n, gt_boxes, m, gt_ld, ex, picks, per_image,
        pieces, counts, sc, out_rois, reinterpret_cast<long long *>(out_roi_labels), out_roi_scores,
        out_gt_iou, out_gt_src, out_gt_canonical, reinterpret_cast<long long *>(out_reg_valid), out_cls_labels);
    cpd_launch_log_note("roi_targets_gather_kernel");
    return cpd_check_launch();
}
