// kitti_eval.hip -- the hot loops of the KITTI-protocol 3D detection evaluation
// (cpd/datasets/kitti/kitti_object_eval_python/eval.py + rotate_iou.py) without their JIT compiler:
//   1. cpd_kitti_overlaps: every frame's dt x gt overlap block (image IoU, BEV rotated IoU, 3-D IoU) in one launch;
//   2. cpd_kitti_match_scores: compute_statistics_jit(compute_fp=False) for every (sweep, frame) -> matched scores in gt order;
//   3. cpd_kitti_match_pr: compute_statistics_jit(compute_fp=True) for every (sweep, frame, threshold), then the frame-order
//      reduction of fused_compute_statistics into pr[sweep][threshold].
// A "sweep" is one (class, difficulty, min_overlap) of eval_class; all sweeps of one metric share a launch.
//
// Work split: one lane per (sweep, frame) in both matching passes. The greedy matching is serial over a frame's gts (a gt's
// pick depends on the detections earlier gts took), frames hold tens of boxes, and a KITTI-size set gives tens of thousands
// of (sweep, frame) pairs -- enough lanes to fill the part without splitting one frame's scan across a wave. Pass 2 loops its
// (at most 41) thresholds inside the lane, reusing the lane's assigned-detection flags; per-(frame, threshold) results go to a
// workspace and a second kernel sums them over frames in frame order (one lane per (sweep, threshold)): no float atomics,
// so every call gives the same bits.
//
// The rotated overlap restates rotate_iou.py:17-260 (NOT the polygon code of box_geom.h, whose algorithm differs) with
// the jitted CUDA typing: float32 corners, intersections and sort keys; accurate sinf / cosf; the triangle-fan area divides
// a float32 cross product by the float64 literal 2.0, so the area and the criterion arithmetic are float64 and the value is
// rounded to float32 on store. The reference's intersection buffer holds 8 points and the jitted code does not bound-check it; here
// points past the 8th are dropped, so no input writes past the buffer. Built with -ffp-contract=off (no fused multiply-add).
#include <math.h>

#include "common.h"

namespace {

constexpr int KE_THREADS = 256;
constexpr int KE_MAX_PTS = 8;      // rotate_iou.py:235 intersection_corners = 16 floats
constexpr int KE_MAX_THR = 41;     // N_SAMPLE_PTS (eval.py:461)
constexpr double KE_NO_DETECTION = -10000000.0;

// ---- rotate_iou.py --------------------------------------------------------------------------------------------------

// trangle_area (l.17-20): float32 cross product, "/ 2.0" promotes to float64
__device__ __forceinline__ double ke_tri_area(const float *a, const float *b, const float *c) {
    const float v = (a[0] - c[0]) * (b[1] - c[1]) - (a[1] - c[1]) * (b[0] - c[0]);
    return (double)v / 2.0;
}

// area (l.23-30): triangle fan from point 0, float64 accumulation
__device__ __forceinline__ double ke_area(const float *pts, int n) {
    double a = 0.0;
    for (int i = 0; i < n - 2; ++i) a += fabs(ke_tri_area(pts, pts + 2 * i + 2, pts + 2 * i + 4));
    return a;
}

// sort_vertex_in_convex_polygon (l.33-70): insertion sort by the pseudo-angle key
__device__ __forceinline__ void ke_sort_vertices(float *pts, int n) {
    if (n <= 0) return;
    float cx = 0.f, cy = 0.f;
    for (int i = 0; i < n; ++i) {
        cx += pts[2 * i];
        cy += pts[2 * i + 1];
    }
    cx = (float)((double)cx / (double)n);   // float32 /= int32: float64 division, float32 store
    cy = (float)((double)cy / (double)n);
    float vs[KE_MAX_PTS];
    for (int i = 0; i < n; ++i) {
        float v0 = pts[2 * i] - cx, v1 = pts[2 * i + 1] - cy;
        const float d = sqrtf(v0 * v0 + v1 * v1);
        v0 = v0 / d;
        v1 = v1 / d;
        if (v1 < 0.f) v0 = (float)(-2.0 - (double)v0);
        vs[i] = v0;
    }
    for (int i = 1; i < n; ++i) {
        if (vs[i - 1] > vs[i]) {
            const float temp = vs[i], tx = pts[2 * i], ty = pts[2 * i + 1];
            int j = i;
            while (j > 0 && vs[j - 1] > temp) {
                vs[j] = vs[j - 1];
                pts[2 * j] = pts[2 * j - 2];
                pts[2 * j + 1] = pts[2 * j - 1];
                --j;
            }
            vs[j] = temp;
            pts[2 * j] = tx;
            pts[2 * j + 1] = ty;
        }
    }
}

// line_segment_intersection (l.73-116; the non-_v1 form quadrilateral_intersection calls)
__device__ __forceinline__ bool ke_segment_intersection(const float *p1, const float *p2, int i, int j, float *out) {
    const float A0 = p1[2 * i], A1 = p1[2 * i + 1];
    const float B0 = p1[2 * ((i + 1) % 4)], B1 = p1[2 * ((i + 1) % 4) + 1];
    const float C0 = p2[2 * j], C1 = p2[2 * j + 1];
    const float D0 = p2[2 * ((j + 1) % 4)], D1 = p2[2 * ((j + 1) % 4) + 1];
    const float BA0 = B0 - A0, BA1 = B1 - A1;
    const float DA0 = D0 - A0, CA0 = C0 - A0;
    const float DA1 = D1 - A1, CA1 = C1 - A1;
    const bool acd = DA1 * CA0 > CA1 * DA0;
    const bool bcd = (D1 - B1) * (C0 - B0) > (C1 - B1) * (D0 - B0);
    if (acd != bcd) {
        const bool abc = CA1 * BA0 > BA1 * CA0;
        const bool abd = DA1 * BA0 > BA1 * DA0;
        if (abc != abd) {
            const float DC0 = D0 - C0, DC1 = D1 - C1;
            const float ABBA = A0 * B1 - B0 * A1;
            const float CDDC = C0 * D1 - D0 * C1;
            const float DH = BA1 * DC0 - BA0 * DC1;
            const float Dx = ABBA * DC0 - BA0 * CDDC;
            const float Dy = ABBA * DC1 - BA1 * CDDC;
            out[0] = Dx / DH;
            out[1] = Dy / DH;
            return true;
        }
    }
    return false;
}

// point_in_quadrilateral (l.161-177)
__device__ __forceinline__ bool ke_point_in_quad(float px, float py, const float *c) {
    const float ab0 = c[2] - c[0], ab1 = c[3] - c[1];
    const float ad0 = c[6] - c[0], ad1 = c[7] - c[1];
    const float ap0 = px - c[0], ap1 = py - c[1];
    const float abab = ab0 * ab0 + ab1 * ab1;
    const float abap = ab0 * ap0 + ab1 * ap1;
    const float adad = ad0 * ad0 + ad1 * ad1;
    const float adap = ad0 * ap0 + ad1 * ap1;
    return abab >= abap && abap >= 0.f && adad >= adap && adap >= 0.f;
}

__device__ __forceinline__ void ke_push(float *pts, int &n, float x, float y) {
    if (n < KE_MAX_PTS) {           // the reference's buffer bound; it would write past it
        pts[2 * n] = x;
        pts[2 * n + 1] = y;
        ++n;
    }
}

// quadrilateral_intersection (l.180-201)
__device__ __forceinline__ int ke_quad_intersection(const float *p1, const float *p2, float *pts) {
    int n = 0;
    for (int i = 0; i < 4; ++i) {
        if (ke_point_in_quad(p1[2 * i], p1[2 * i + 1], p2)) ke_push(pts, n, p1[2 * i], p1[2 * i + 1]);
        if (ke_point_in_quad(p2[2 * i], p2[2 * i + 1], p1)) ke_push(pts, n, p2[2 * i], p2[2 * i + 1]);
    }
    float t[2];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j)
            if (ke_segment_intersection(p1, p2, i, j, t)) ke_push(pts, n, t[0], t[1]);
    return n;
}

// rbbox_to_corners (l.204-228)
__device__ __forceinline__ void ke_corners(const float *b, float *c) {
    const float a_cos = cosf(b[4]), a_sin = sinf(b[4]);
    const float hx = -b[2] / 2.f, hy = -b[3] / 2.f;   // exact halving, as the jitted float64 "/ 2" then float32 store
    const float cxs[4] = {hx, hx, -hx, -hx};
    const float cys[4] = {hy, -hy, -hy, hy};
    for (int i = 0; i < 4; ++i) {
        c[2 * i] = a_cos * cxs[i] + a_sin * cys[i] + b[0];
        c[2 * i + 1] = -a_sin * cxs[i] + a_cos * cys[i] + b[1];
    }
}

// devRotateIoUEval(rbox1, rbox2, criterion) (l.248-260); float64 result, rounded to float32 by the caller
__device__ __forceinline__ double ke_rotate_iou(const float *rbox1, const float *rbox2, int criterion) {
    const float area1 = rbox1[2] * rbox1[3];
    const float area2 = rbox2[2] * rbox2[3];
    float c1[8], c2[8], pts[2 * KE_MAX_PTS];
    ke_corners(rbox1, c1);
    ke_corners(rbox2, c2);
    const int n = ke_quad_intersection(c1, c2, pts);
    ke_sort_vertices(pts, n);
    const double inter = ke_area(pts, n);
    if (criterion == -1) return inter / ((double)(area1 + area2) - inter);
    if (criterion == 0) return inter / (double)area1;
    if (criterion == 1) return inter / (double)area2;
    return inter;
}

// ---- eval.py --------------------------------------------------------------------------------------------------------

// image_box_overlap (eval.py:91-117) for one (boxes[n], query_boxes[k]) pair, float64
__device__ __forceinline__ double ke_image_overlap(const double *b, const double *q, int criterion) {
    const double qarea = (q[2] - q[0]) * (q[3] - q[1]);
    const double iw = fmin(b[2], q[2]) - fmax(b[0], q[0]);
    if (iw > 0.0) {
        const double ih = fmin(b[3], q[3]) - fmax(b[1], q[1]);
        if (ih > 0.0) {
            double ua;
            if (criterion == -1) ua = (b[2] - b[0]) * (b[3] - b[1]) + qarea - iw * ih;
            else if (criterion == 0) ua = (b[2] - b[0]) * (b[3] - b[1]);
            else if (criterion == 1) ua = qarea;
            else ua = 1.0;
            return iw * ih / ua;
        }
    }
    return 0.0;
}

// frame of packed pair p: the last f with pair_off[f] <= p (empty frames share an offset with the next one)
__device__ __forceinline__ int ke_frame_of(const int64_t *off, int n_frames, int64_t p) {
    int lo = 0, hi = n_frames;            // invariant: off[lo] <= p < off[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= p) lo = mid;
        else hi = mid;
    }
    return lo;
}

struct KeOverlapArgs {
    const void *dt, *gt;
    const int32_t *dt_off, *gt_off;
    const int64_t *pair_off;
    int n_frames, metric, criterion;
    int64_t n_pairs;
    double *out;
};

// one lane per packed (frame, dt row j, gt column i), grid-stride: out[pair_off[f] + j * n_gt + i] = overlaps[f][j, i] of
// calculate_iou_partly(dt_annos, gt_annos, metric) (eval.py:485), i.e. boxes = dt, query_boxes = gt
__device__ __forceinline__ void ke_overlap_one(const KeOverlapArgs &a, int64_t p) {
    const int f = ke_frame_of(a.pair_off, a.n_frames, p);
    const int64_t r = p - a.pair_off[f];
    const int ng = a.gt_off[f + 1] - a.gt_off[f];
    const int j = a.dt_off[f] + (int)(r / ng), i = a.gt_off[f] + (int)(r % ng);
    double v;
    if (a.metric == 0) {                                          // image_box_overlap(dt bbox, gt bbox, criterion)
        v = ke_image_overlap(static_cast<const double *>(a.dt) + 4 * (int64_t)j,
                             static_cast<const double *>(a.gt) + 4 * (int64_t)i, a.criterion);
    } else if (a.metric == 1) {                                   // rotate_iou_gpu_eval(dt bev, gt bev, criterion), float32
        const float *b = static_cast<const float *>(a.dt) + 5 * (int64_t)j;
        const float *q = static_cast<const float *>(a.gt) + 5 * (int64_t)i;
        v = (double)(float)ke_rotate_iou(q, b, a.criterion);      // launcher order: devRotateIoUEval(query, box)
    } else {                                                      // d3_box_overlap (eval.py:121-155)
        const double *b = static_cast<const double *>(a.dt) + 7 * (int64_t)j;
        const double *q = static_cast<const double *>(a.gt) + 7 * (int64_t)i;
        const float bb[5] = {(float)b[0], (float)b[2], (float)b[3], (float)b[5], (float)b[6]};
        const float qb[5] = {(float)q[0], (float)q[2], (float)q[3], (float)q[5], (float)q[6]};
        float rinc = (float)ke_rotate_iou(qb, bb, 2);            // BEV intersection area, float32 array
        if (rinc > 0.f) {
            const double iw = fmin(b[1], q[1]) - fmax(b[1] - b[4], q[1] - q[4]);
            if (iw > 0.0) {
                const double area1 = b[3] * b[4] * b[5];
                const double area2 = q[3] * q[4] * q[5];
                const double inc = iw * (double)rinc;
                double ua;
                if (a.criterion == -1) ua = area1 + area2 - inc;
                else if (a.criterion == 0) ua = area1;
                else if (a.criterion == 1) ua = area2;
                else ua = inc;
                rinc = (float)(inc / ua);                          // float64 arithmetic stored into the float32 rinc
            } else {
                rinc = 0.f;
            }
        }
        v = (double)rinc;
    }
    a.out[p] = v;
}

__global__ void __launch_bounds__(KE_THREADS) kitti_overlaps_kernel(KeOverlapArgs a) {
    for (int64_t p = (int64_t)blockIdx.x * KE_THREADS + threadIdx.x; p < a.n_pairs; p += (int64_t)gridDim.x * KE_THREADS)
        ke_overlap_one(a, p);
}

struct KeMatchArgs {
    const double *overlaps;
    const int64_t *pair_off;
    const int32_t *dt_off, *gt_off, *dc_off;
    const int8_t *ig_gt, *ig_dt;       // [n_cd][total_gt], [n_cd][total_dt]: clean_data's ignored_gt / ignored_det
    const double *dt_score, *dt_alpha, *gt_alpha, *dt_bbox, *dc_bbox;
    const int32_t *sweep_cd;           // [n_sweeps] row of ig_gt / ig_dt
    const double *sweep_min_overlap;   // [n_sweeps]
    const double *thresholds;          // [n_sweeps][41]
    const int32_t *n_thresholds;       // [n_sweeps]
    int n_frames, n_sweeps, total_gt, total_dt, metric, compute_aos;
    uint8_t *assigned;                 // workspace [n_sweeps][total_dt]
    double *scores;                    // pass 1: [n_sweeps][total_gt]
    int8_t *matched;                   // pass 1: [n_sweeps][total_gt]
    int32_t *counts;                   // pass 2 workspace: [n_sweeps][41][n_frames][3] tp, fp, fn
    double *sims;                      // pass 2 workspace: [n_sweeps][41][n_frames] similarity (-1: none)
};

// compute_statistics_jit with compute_fp=False (eval.py:158-259) for one (sweep, frame): scores[s][g] = dt score of the
// detection matched to gt g where the reference appends it to `thresholds` (matched = 1), in gt order
__global__ void __launch_bounds__(KE_THREADS) kitti_match_scores_kernel(KeMatchArgs a) {
    const int64_t idx = (int64_t)blockIdx.x * KE_THREADS + threadIdx.x;
    if (idx >= (int64_t)a.n_sweeps * a.n_frames) return;
    const int s = (int)(idx / a.n_frames), f = (int)(idx % a.n_frames);
    const int cd = a.sweep_cd[s];
    const double min_overlap = a.sweep_min_overlap[s];
    const int d0 = a.dt_off[f], nd = a.dt_off[f + 1] - d0, g0 = a.gt_off[f], ng = a.gt_off[f + 1] - g0;
    const double *ov = a.overlaps + a.pair_off[f];
    const int8_t *igg = a.ig_gt + (int64_t)cd * a.total_gt + g0;
    const int8_t *igd = a.ig_dt + (int64_t)cd * a.total_dt + d0;
    const double *score = a.dt_score + d0;
    uint8_t *asg = a.assigned + (int64_t)s * a.total_dt + d0;
    double *out = a.scores + (int64_t)s * a.total_gt + g0;
    int8_t *hit = a.matched + (int64_t)s * a.total_gt + g0;
    for (int j = 0; j < nd; ++j) asg[j] = 0;
    for (int i = 0; i < ng; ++i) {
        hit[i] = 0;
        out[i] = 0.0;
        if (igg[i] == -1) continue;
        int det = -1;
        double valid = KE_NO_DETECTION;
        for (int j = 0; j < nd; ++j) {
            if (igd[j] == -1 || asg[j]) continue;
            const double o = ov[(int64_t)j * ng + i];
            if (o > min_overlap && score[j] > valid) {       // strict: the lowest j wins a score tie
                det = j;
                valid = score[j];
            }
        }
        if (valid == KE_NO_DETECTION) continue;              // fn (igg 0) or nothing
        if (igg[i] == 1 || igd[det] == 1) {
            asg[det] = 1;
        } else {
            out[i] = score[det];
            hit[i] = 1;
            asg[det] = 1;
        }
    }
}

// compute_statistics_jit with compute_fp=True for one (sweep, frame) and each of the sweep's thresholds, as
// fused_compute_statistics (eval.py:275-337) calls it; tp / fp / fn / similarity per (sweep, threshold, frame)
__global__ void __launch_bounds__(KE_THREADS) kitti_match_pr_kernel(KeMatchArgs a) {
    const int64_t idx = (int64_t)blockIdx.x * KE_THREADS + threadIdx.x;
    if (idx >= (int64_t)a.n_sweeps * a.n_frames) return;
    const int s = (int)(idx / a.n_frames), f = (int)(idx % a.n_frames);
    const int cd = a.sweep_cd[s];
    const double min_overlap = a.sweep_min_overlap[s];
    const int d0 = a.dt_off[f], nd = a.dt_off[f + 1] - d0, g0 = a.gt_off[f], ng = a.gt_off[f + 1] - g0;
    const int c0 = a.dc_off[f], nc = a.dc_off[f + 1] - c0;
    const double *ov = a.overlaps + a.pair_off[f];
    const int8_t *igg = a.ig_gt + (int64_t)cd * a.total_gt + g0;
    const int8_t *igd = a.ig_dt + (int64_t)cd * a.total_dt + d0;
    const double *score = a.dt_score + d0;
    uint8_t *asg = a.assigned + (int64_t)s * a.total_dt + d0;
    const int nt = min(a.n_thresholds[s], KE_MAX_THR);
    for (int t = 0; t < nt; ++t) {
        const double thresh = a.thresholds[s * KE_MAX_THR + t];
        for (int j = 0; j < nd; ++j) asg[j] = 0;
        int tp = 0, fp = 0, fn = 0;
        double sim_sum = 0.0;                                // the jitted np.sum: a sequential sum from 0 (the fp zeros add nothing)
        for (int i = 0; i < ng; ++i) {
            if (igg[i] == -1) continue;
            int det = -1;
            double valid = KE_NO_DETECTION, max_overlap = 0.0;
            bool assigned_ignored_det = false;
            for (int j = 0; j < nd; ++j) {
                if (igd[j] == -1 || asg[j] || score[j] < thresh) continue;
                const double o = ov[(int64_t)j * ng + i];
                if (o > min_overlap && (o > max_overlap || assigned_ignored_det) && igd[j] == 0) {
                    max_overlap = o;                         // strict: the lowest j wins an overlap tie
                    det = j;
                    valid = 1.0;
                    assigned_ignored_det = false;
                } else if (o > min_overlap && valid == KE_NO_DETECTION && igd[j] == 1) {
                    det = j;
                    valid = 1.0;
                    assigned_ignored_det = true;
                }
            }
            if (valid == KE_NO_DETECTION && igg[i] == 0) {
                ++fn;
            } else if (valid != KE_NO_DETECTION && (igg[i] == 1 || igd[det] == 1)) {
                asg[det] = 1;
            } else if (valid != KE_NO_DETECTION) {
                ++tp;
                if (a.compute_aos) sim_sum += (1.0 + cos(a.gt_alpha[g0 + i] - a.dt_alpha[d0 + det])) / 2.0;
                asg[det] = 1;
            }
        }
        for (int j = 0; j < nd; ++j)
            if (!(asg[j] || igd[j] == -1 || igd[j] == 1 || score[j] < thresh)) ++fp;
        int nstuff = 0;
        if (a.metric == 0) {                                  // don't-care suppression: image_box_overlap(dt, dc, 0)
            for (int i = 0; i < nc; ++i) {
                for (int j = 0; j < nd; ++j) {
                    if (asg[j] || igd[j] == -1 || igd[j] == 1 || score[j] < thresh) continue;
                    if (ke_image_overlap(a.dt_bbox + 4 * (int64_t)(d0 + j), a.dc_bbox + 4 * (int64_t)(c0 + i), 0) > min_overlap) {
                        asg[j] = 1;
                        ++nstuff;
                    }
                }
            }
        }
        fp -= nstuff;
        double sim = 0.0;
        if (a.compute_aos) sim = (tp > 0 || fp > 0) ? sim_sum : -1.0;
        const int64_t o = ((int64_t)s * KE_MAX_THR + t) * a.n_frames + f;   // [sweep][threshold][frame]
        a.counts[3 * o] = tp;
        a.counts[3 * o + 1] = fp;
        a.counts[3 * o + 2] = fn;
        a.sims[o] = sim;
    }
}

// pr[s][t] = sum over frames, in frame order, of the per-frame results (fused_compute_statistics' "pr[t, k] +=");
// one lane per (sweep, threshold); rows past the sweep's threshold count are zero. The workspace is [sweep][threshold][frame]:
// each lane streams its own contiguous row, so one cache line serves several frame steps of the lane's serial loop (measured
// faster than a [sweep][frame][threshold] layout, whose neighbouring-lane reads cost every lane a new line per frame)
__global__ void __launch_bounds__(KE_THREADS) kitti_pr_reduce_kernel(const int32_t *__restrict__ counts, const double *__restrict__ sims,
                                                                     const int32_t *__restrict__ n_thresholds, int n_sweeps,
                                                                     int n_frames, int64_t *__restrict__ pr_counts,
                                                                     double *__restrict__ pr_sim) {
    const int idx = blockIdx.x * KE_THREADS + threadIdx.x;
    if (idx >= n_sweeps * KE_MAX_THR) return;
    const int s = idx / KE_MAX_THR, t = idx % KE_MAX_THR;
    int64_t tp = 0, fp = 0, fn = 0;
    double sim = 0.0;
    if (t < min(n_thresholds[s], KE_MAX_THR)) {
        for (int f = 0; f < n_frames; ++f) {
            const int64_t o = (int64_t)idx * n_frames + f;
            const int32_t *c = counts + 3 * o;
            tp += c[0];
            fp += c[1];
            fn += c[2];
            const double v = sims[o];
            if (v != -1.0) sim += v;
        }
    }
    pr_counts[3 * idx] = tp;
    pr_counts[3 * idx + 1] = fp;
    pr_counts[3 * idx + 2] = fn;
    pr_sim[idx] = sim;
}

int ke_fill_match(KeMatchArgs &a, const double *overlaps, const int64_t *pair_off, const int32_t *dt_off, const int32_t *gt_off,
                  int n_frames, const int8_t *ig_gt, const int8_t *ig_dt, const double *dt_score, const int32_t *sweep_cd,
                  const double *sweep_min_overlap, int n_sweeps, int total_gt, int total_dt) {
    if (n_frames <= 0 || n_sweeps <= 0 || total_gt < 0 || total_dt < 0 || !pair_off || !dt_off || !gt_off || !sweep_cd ||
        !sweep_min_overlap)
        return CPD_ERR_ARG;
    if ((total_gt > 0 && !ig_gt) || (total_dt > 0 && (!ig_dt || !dt_score)) || (total_gt > 0 && total_dt > 0 && !overlaps))
        return CPD_ERR_ARG;
    if ((int64_t)n_sweeps * n_frames >= ((int64_t)1 << 31)) return CPD_ERR_UNSUPPORTED;
    a = KeMatchArgs{};
    a.overlaps = overlaps; a.pair_off = pair_off; a.dt_off = dt_off; a.gt_off = gt_off;
    a.ig_gt = ig_gt; a.ig_dt = ig_dt; a.dt_score = dt_score;
    a.sweep_cd = sweep_cd; a.sweep_min_overlap = sweep_min_overlap;
    a.n_frames = n_frames; a.n_sweeps = n_sweeps; a.total_gt = total_gt; a.total_dt = total_dt;
    return CPD_OK;
}

}  // namespace

extern "C" int cpd_kitti_overlaps(int metric, int criterion, const void *dt_boxes, const void *gt_boxes, const int32_t *dt_off,
                                  const int32_t *gt_off, const int64_t *pair_off, int n_frames, int64_t n_pairs, double *out,
                                  cpd_stream_t st) {
    if (metric < 0 || metric > 2 || n_frames <= 0 || n_pairs < 0 || !dt_off || !gt_off || !pair_off) return CPD_ERR_ARG;
    if (n_pairs == 0) return CPD_OK;
    if (!dt_boxes || !gt_boxes || !out) return CPD_ERR_ARG;
    if (n_pairs > ((int64_t)1 << 40)) return CPD_ERR_UNSUPPORTED;
    KeOverlapArgs a;
    a.dt = dt_boxes; a.gt = gt_boxes; a.dt_off = dt_off; a.gt_off = gt_off; a.pair_off = pair_off;
    a.n_frames = n_frames; a.metric = metric; a.criterion = criterion; a.n_pairs = n_pairs; a.out = out;
    cpd_launch_log_note("kitti_overlaps_kernel");
    const int64_t blocks = (n_pairs + KE_THREADS - 1) / KE_THREADS;   // capped: the kernel strides over the rest
    kitti_overlaps_kernel<<<(unsigned)(blocks < 65536 ? blocks : 65536), KE_THREADS, 0, cpd_s(st)>>>(a);
    return cpd_check_launch();
}

// The PR pass keeps per (sweep, threshold, frame) row three counts and one similarity sum, then one `assigned` byte per
// (sweep, detection). pr_frames = 0 (the score pass, which has no such rows) leaves `assigned` alone, at offset 0.
struct KeLayout { size_t counts, sims, assigned, total; };
static KeLayout ke_layout(int n_sweeps, int pr_frames, int total_dt) {
    const size_t rows = (size_t)n_sweeps * KE_MAX_THR * pr_frames;
    Carve c;
    KeLayout l;
    l.counts = c.take(rows * 3 * sizeof(int32_t));
    l.sims = c.take(rows * sizeof(double));
    l.assigned = c.take((size_t)n_sweeps * total_dt);
    l.total = c.o;
    return l;
}

extern "C" size_t cpd_kitti_match_workspace_bytes(int n_sweeps, int n_frames, int total_dt) {
    if (n_sweeps <= 0 || n_frames <= 0 || total_dt < 0) return 0;
    return ke_layout(n_sweeps, n_frames, total_dt).total;
}

extern "C" int cpd_kitti_match_scores(const double *overlaps, const int64_t *pair_off, const int32_t *dt_off, const int32_t *gt_off,
                                      int n_frames, const int8_t *ig_gt, const int8_t *ig_dt, const double *dt_score,
                                      const int32_t *sweep_cd, const double *sweep_min_overlap, int n_sweeps, int total_gt,
                                      int total_dt, double *scores, int8_t *matched, void *workspace, size_t workspace_bytes,
                                      cpd_stream_t st) {
    KeMatchArgs a;
    const int rc = ke_fill_match(a, overlaps, pair_off, dt_off, gt_off, n_frames, ig_gt, ig_dt, dt_score, sweep_cd,
                                 sweep_min_overlap, n_sweeps, total_gt, total_dt);
    if (rc != CPD_OK) return rc;
    if (total_gt > 0 && (!scores || !matched)) return CPD_ERR_ARG;
    const KeLayout l = ke_layout(n_sweeps, 0, total_dt);
    if (l.total > 0 && (!workspace || workspace_bytes < l.total)) return CPD_ERR_WORKSPACE;
    a.assigned = ws_at<uint8_t>(workspace, l.assigned);
    a.scores = scores;
    a.matched = matched;
    const int64_t lanes = (int64_t)n_sweeps * n_frames;
    cpd_launch_log_note("kitti_match_scores_kernel");
    kitti_match_scores_kernel<<<(unsigned)((lanes + KE_THREADS - 1) / KE_THREADS), KE_THREADS, 0, cpd_s(st)>>>(a);
    return cpd_check_launch();
}

extern "C" int cpd_kitti_match_pr(const double *overlaps, const int64_t *pair_off, const int32_t *dt_off, const int32_t *gt_off,
                                  const int32_t *dc_off, int n_frames, const int8_t *ig_gt, const int8_t *ig_dt,
                                  const double *dt_score, const double *dt_alpha, const double *gt_alpha, const double *dt_bbox,
                                  const double *dc_bbox, int metric, int compute_aos, const int32_t *sweep_cd,
                                  const double *sweep_min_overlap, const double *thresholds, const int32_t *n_thresholds,
                                  int n_sweeps, int total_gt, int total_dt, int64_t *pr_counts, double *pr_sim, void *workspace,
                                  size_t workspace_bytes, cpd_stream_t st) {
    KeMatchArgs a;
    const int rc = ke_fill_match(a, overlaps, pair_off, dt_off, gt_off, n_frames, ig_gt, ig_dt, dt_score, sweep_cd,
                                 sweep_min_overlap, n_sweeps, total_gt, total_dt);
    if (rc != CPD_OK) return rc;
    if (!dc_off || !thresholds || !n_thresholds || !pr_counts || !pr_sim || metric < 0 || metric > 2) return CPD_ERR_ARG;
    if (total_dt > 0 && (!dt_alpha || !dt_bbox)) return CPD_ERR_ARG;
    if (total_gt > 0 && !gt_alpha) return CPD_ERR_ARG;
    const KeLayout l = ke_layout(n_sweeps, n_frames, total_dt);
    if (!workspace || workspace_bytes < l.total) return CPD_ERR_WORKSPACE;
    a.counts = ws_at<int32_t>(workspace, l.counts);
    a.sims = ws_at<double>(workspace, l.sims);
    a.assigned = ws_at<uint8_t>(workspace, l.assigned);
    a.dc_off = dc_off; a.dt_alpha = dt_alpha; a.gt_alpha = gt_alpha; a.dt_bbox = dt_bbox; a.dc_bbox = dc_bbox;
    a.thresholds = thresholds; a.n_thresholds = n_thresholds; a.metric = metric; a.compute_aos = compute_aos ? 1 : 0;
    const int64_t lanes = (int64_t)n_sweeps * n_frames;
    cpd_launch_log_note("kitti_match_pr_kernel");
    kitti_match_pr_kernel<<<(unsigned)((lanes + KE_THREADS - 1) / KE_THREADS), KE_THREADS, 0, cpd_s(st)>>>(a);
    int e = cpd_check_launch();
    if (e != CPD_OK) return e;
    cpd_launch_log_note("kitti_pr_reduce_kernel");
    kitti_pr_reduce_kernel<<<(unsigned)cpd_div_up((long long)n_sweeps * KE_MAX_THR, KE_THREADS), KE_THREADS, 0, cpd_s(st)>>>(
        a.counts, a.sims, n_thresholds, n_sweeps, n_frames, pr_counts, pr_sim);
    return cpd_check_launch();
}
