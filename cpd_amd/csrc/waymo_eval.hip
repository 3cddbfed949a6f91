// waymo_eval.hip -- the hot loops of the Waymo-protocol detection metrics (AP / APH), as cpd_amd/waymo_eval.py defines them
// (a drop-in for cpd/datasets/waymo_unsupervised/waymo_eval.py, whose metric op lives in a library outside the reference tree):
//   1. cpd_waymo_iou: the float64 rotated 3-D IoU block (prediction rows x ground-truth columns) of every (frame, type)
//      problem of a chunk of frames, packed, in one launch; cpd_waymo_iou_bev: the same block for the BEV protocol
//      (waymo_eval2d.py, box_type TYPE_2D: five-column rows, the rectangles' IoU with no z term);
//   2. cpd_waymo_match: for every problem, the maximum-weight matching at each of the 101 score cut-offs and its counts
//      (tp / fn per level, fp, heading accuracy), then an ordered reduction over frames.
//
// IoU: one lane per packed pair. Box A's corners are taken into box B's frame (one rotation by the heading difference), where
// B is the axis-aligned rectangle [-dx/2, dx/2] x [-dy/2, dy/2]; A is clipped against B's four half-planes (Sutherland-Hodgman,
// at most 8 vertices) and the shoelace area is multiplied by the overlap of the z intervals. All float64 from the float32 inputs.
// Clipping is used (not a sum of clipped boundary segments) because it stays continuous when edges coincide: identical boxes
// clip to the box itself. box_geom.h's polygon code carries the NMS op's 1e-2 margin test and is not used here.
//
// Matching: one wavefront (a 64-thread workgroup) per problem; lanes go across ground-truth columns. Predictions are ranked by
// descending score (stable: ties by index) and inserted one row at a time into a successive-shortest-augmenting-path assignment
// (the row-by-row Hungarian / Jonker-Volgenant scheme) with float64 row and column potentials. Cost of a cell is -IoU when
// IoU >= the type's threshold; other cells cannot match. Every row also owns a private zero-cost column ("unmatched"), so the
// assignment after each insertion is the maximum-weight matching of the rows inserted so far. A row that ends on its private
// column is never part of a later augmenting path (a path reaches a row only through the real column it holds), so only the
// rows that hold a real column keep a potential: ucol[j] is the potential of the row on column j. After the last row with
// score >= c_k the matching is optimal for cut-off k and its counts are emitted; all 101 cut-offs cost one assignment solve.
// Every loop has a trip count bounded by the problem's row or column count: a search runs at most n_gt + 1 scans (each scan
// but the last marks one more matched column as visited), a path walk at most n_gt + 1 steps. NaN cells never reach the
// >= test, infinite cells are not edges, NaN scores belong to no subset: malformed input costs time, never a hang.
//
// Potentials (minv, v, ucol), predecessors (way), the column -> row map and the visited flags live in LDS, sized by the chunk's
// largest column count; the IoU block is read from global memory. Per-problem results go to a workspace laid out
// [type][cut-off][frame]; a second kernel (one lane per (type, cut-off)) adds them in frame order into int64 counts and float64
// heading sums -- no floating-point atomics, and with `accumulate` the sums continue from the previous chunk's, so chunked and
// unchunked runs add the same terms in the same order. Built with -ffp-contract=off: the values are compared with thresholds.
#include <limits.h>
#include <math.h>

#include "common.h"

namespace {

constexpr int WM_THREADS = 256;       // IoU and reduce kernels
constexpr int WM_TYPES = CPD_WAYMO_TYPES;
constexpr int WM_CUTOFFS = CPD_WAYMO_CUTOFFS;
constexpr int WM_MAX_PTS = 8;         // a rectangle clipped by four half-planes has at most 8 vertices
constexpr double WM_PI = 3.14159265358979323846;

// ---- IoU ------------------------------------------------------------------------------------------------------------

// the part of a convex polygon with sgn * coordinate[axis] <= lim; vertex i of a buffer is element i * S
template <int S>
__device__ __forceinline__ int wm_clip(const double *ix, const double *iy, int n, int axis, double sgn, double lim, double *ox,
                                       double *oy) {
    int m = 0;
    for (int i = 0; i < n; ++i) {
        const int k = (i + 1 == n) ? 0 : i + 1;
        const double px = ix[i * S], py = iy[i * S], qx = ix[k * S], qy = iy[k * S];
        const double fp = lim - sgn * (axis ? py : px), fq = lim - sgn * (axis ? qy : qx);
        const bool pin = fp >= 0.0, qin = fq >= 0.0;
        if (pin && m < WM_MAX_PTS) {
            ox[m * S] = px;
            oy[m * S] = py;
            ++m;
        }
        if (pin != qin && m < WM_MAX_PTS) {          // fp and fq differ in sign, so fp - fq is not zero
            const double t = fp / (fp - fq);
            ox[m * S] = px + t * (qx - px);
            oy[m * S] = py + t * (qy - py);
            ++m;
        }
    }
    return m;
}

// area of the intersection of rectangle A (centre, full sizes, heading) with rectangle B: A's corners go into B's frame, where
// B is [-dx/2, dx/2] x [-dy/2, dy/2], and are clipped by its four half-planes; 0 when no circle of A reaches B's or fewer than
// 3 vertices remain. px, py, qx, qy: the caller's four buffers of WM_MAX_PTS vertices, vertex i at element i * S.
template <int S>
__device__ __forceinline__ double wm_rect_overlap(double ax, double ay, double adx, double ady, double ah, double bx, double by,
                                                  double bdx, double bdy, double bh, double *px, double *py, double *qx,
                                                  double *qy) {
    const double hxa = adx / 2.0, hya = ady / 2.0, hxb = bdx / 2.0, hyb = bdy / 2.0;
    const double tx = ax - bx, ty = ay - by;
    // no circle of A reaches B's: nothing to clip
    const double reach = sqrt(hxa * hxa + hya * hya) + sqrt(hxb * hxb + hyb * hyb);
    if (tx * tx + ty * ty > reach * reach) return 0.0;
    const double cb = cos(bh), sb = sin(bh);
    const double lx = cb * tx + sb * ty, ly = cb * ty - sb * tx;      // A's centre in B's frame
    const double d = ah - bh, c = cos(d), s = sin(d);
    const double sxs[4] = {1.0, -1.0, -1.0, 1.0}, sys[4] = {1.0, 1.0, -1.0, -1.0};
    for (int i = 0; i < 4; ++i) {
        const double ex = sxs[i] * hxa, ey = sys[i] * hya;
        px[i * S] = lx + (c * ex - s * ey);
        py[i * S] = ly + (s * ex + c * ey);
    }
    int n = wm_clip<S>(px, py, 4, 0, 1.0, hxb, qx, qy);
    n = wm_clip<S>(qx, qy, n, 0, -1.0, hxb, px, py);
    n = wm_clip<S>(px, py, n, 1, 1.0, hyb, qx, qy);
    n = wm_clip<S>(qx, qy, n, 1, -1.0, hyb, px, py);
    if (n < 3) return 0.0;
    double twice = 0.0;
    for (int i = 0; i < n; ++i) {
        const int k = (i + 1 == n) ? 0 : i + 1;
        twice += px[i * S] * py[k * S] - px[k * S] * py[i * S];
    }
    return fabs(twice) / 2.0;
}

// rows (cx, cy, cz, dx, dy, dz, heading) float32; 0 for an empty intersection, a non-positive union or any non-finite value
__device__ __forceinline__ double wm_iou(const float *pa, const float *pb) {
    double a[7], b[7];
    bool finite = true;
    for (int i = 0; i < 7; ++i) {
        a[i] = (double)pa[i];
        b[i] = (double)pb[i];
        finite = finite && isfinite(a[i]) && isfinite(b[i]);
    }
    if (!finite) return 0.0;
    const double zlo = fmax(a[2] - a[5] / 2.0, b[2] - b[5] / 2.0), zhi = fmin(a[2] + a[5] / 2.0, b[2] + b[5] / 2.0);
    const double h = zhi - zlo;
    if (!(h > 0.0)) return 0.0;
    double px[WM_MAX_PTS], py[WM_MAX_PTS], qx[WM_MAX_PTS], qy[WM_MAX_PTS];
    const double inter = wm_rect_overlap<1>(a[0], a[1], a[3], a[4], a[6], b[0], b[1], b[3], b[4], b[6], px, py, qx, qy) * h;
    const double uni = a[3] * a[4] * a[5] + b[3] * b[4] * b[5] - inter;
    if (!(inter > 0.0) || !(uni > 0.0)) return 0.0;
    const double v = inter / uni;
    return isfinite(v) ? v : 0.0;
}

// rows (cx, cy, dx, dy, heading) float32, the boxes of box_type TYPE_2D: the rectangles' intersection over their union, no z
// term. 0 for an empty intersection, a non-positive union, a size that is not positive (two negative ones would pass for a
// box), and any value that is not finite or not below WM_BEV_LIMIT in magnitude (2^29: a float32 that large holds neither a
// position in metres nor a direction, its ulp is 32). The four vertex buffers are the block's LDS, one column per lane, so
// the vertex counts that index them cost no scratch: WM_THREADS * 4 * WM_MAX_PTS doubles, 64 KiB.
constexpr double WM_BEV_LIMIT = 0x1.0p+29;
__device__ __forceinline__ double wm_iou_bev(const float *pa, const float *pb) {
    double a[5], b[5];
    bool ok = true;
    for (int i = 0; i < 5; ++i) {
        a[i] = (double)pa[i];
        b[i] = (double)pb[i];
        ok = ok && fabs(a[i]) < WM_BEV_LIMIT && fabs(b[i]) < WM_BEV_LIMIT;      // false for NaN and the infinities too
    }
    if (!ok || !(a[2] > 0.0 && a[3] > 0.0 && b[2] > 0.0 && b[3] > 0.0)) return 0.0;
    __shared__ double poly[4][WM_MAX_PTS][WM_THREADS];
    double *mine = &poly[0][0][threadIdx.x];
    constexpr int BUF = WM_MAX_PTS * WM_THREADS;
    const double inter = wm_rect_overlap<WM_THREADS>(a[0], a[1], a[2], a[3], a[4], b[0], b[1], b[2], b[3], b[4], mine, mine + BUF,
                                                     mine + 2 * BUF, mine + 3 * BUF);
    const double uni = a[2] * a[3] + b[2] * b[3] - inter;
    if (!(inter > 0.0) || !(uni > 0.0)) return 0.0;
    const double v = inter / uni;
    return isfinite(v) ? v : 0.0;
}

struct WmIouArgs {
    const float *pd, *gt;
    const int32_t *pd_off, *gt_off;
    const int64_t *pair_off;
    int n_problems;
    int64_t n_pairs;
    double *out;
};

// one lane per packed (problem, prediction row, ground-truth column), grid-stride; STRIDE floats per row, PAIR their IoU
template <int STRIDE, double (*PAIR)(const float *, const float *)>
__device__ __forceinline__ void wm_iou_lanes(const WmIouArgs &a) {
    for (int64_t p = (int64_t)blockIdx.x * WM_THREADS + threadIdx.x; p < a.n_pairs; p += (int64_t)gridDim.x * WM_THREADS) {
        int lo = 0, hi = a.n_problems;              // pair_off[lo] <= p < pair_off[hi]; empty problems share an offset
        for (int it = 0; it < 32 && hi - lo > 1; ++it) {
            const int mid = (lo + hi) >> 1;
            if (a.pair_off[mid] <= p) lo = mid;
            else hi = mid;
        }
        const int64_t r = p - a.pair_off[lo];
        const int ng = a.gt_off[lo + 1] - a.gt_off[lo];
        const int i = a.pd_off[lo] + (int)(r / ng), j = a.gt_off[lo] + (int)(r % ng);
        a.out[p] = PAIR(a.pd + STRIDE * (int64_t)i, a.gt + STRIDE * (int64_t)j);
    }
}
__global__ void __launch_bounds__(WM_THREADS) waymo_iou_kernel(WmIouArgs a) { wm_iou_lanes<7, wm_iou>(a); }
__global__ void __launch_bounds__(WM_THREADS) waymo_iou_bev_kernel(WmIouArgs a) { wm_iou_lanes<5, wm_iou_bev>(a); }

// ---- matching -------------------------------------------------------------------------------------------------------

struct WmMatchArgs {
    const double *iou;
    const int64_t *pair_off;
    const int32_t *pd_off, *gt_off;
    const float *score;
    const uint8_t *difficulty;
    const float *pd_heading, *gt_heading;
    double thr[WM_TYPES];
    int n_frames, max_pd, max_gt, cap;
    int32_t *order;      // workspace [total_pd]: a problem's rows by descending score
    int32_t *pcounts;    // workspace [type][cut-off][frame][5]: tp1, tp2, fn1, fn2, fp
    double *pha;         // workspace [type][cut-off][frame][2]
    int32_t *flag;       // workspace: set when a problem exceeds the maxima the LDS was sized for
};

__device__ __forceinline__ int wm_uni(int x) { return __builtin_amdgcn_readfirstlane(x); }

// total order of the scores: NaN sorts last (it is in no subset), -0 with +0
__device__ __forceinline__ float wm_score(float s) { return (s == s) ? s + 0.0f : -INFINITY; }

// smallest value over the wave and, among equals, its lowest column; every lane gets the result
__device__ __forceinline__ void wm_wave_argmin(double &b, int &j) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const double ob = __shfl_xor(b, d, 64);
        const int oj = __shfl_xor(j, d, 64);
        if (ob < b || (ob == b && oj < j)) {
            b = ob;
            j = oj;
        }
    }
}
__device__ __forceinline__ int wm_wave_sum(int v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
__device__ __forceinline__ double wm_wave_sum(double v) {      // a + b == b + a: every lane gets the same bits
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// 1 - |wrap(pd - gt)| / pi, wrap to [-pi, pi]
__device__ __forceinline__ double wm_heading_accuracy(float pd, float gt) {
    const double t = 1.0 - fabs(remainder((double)pd - (double)gt, 2.0 * WM_PI)) / WM_PI;
    return (t >= 0.0) ? t : 0.0;        // also NaN -> 0
}

__global__ void __launch_bounds__(64) waymo_match_kernel(WmMatchArgs a) {
    extern __shared__ double wm_lds[];
    const int q = blockIdx.x, lane = threadIdx.x;
    const int cap = a.cap;
    double *minv = wm_lds, *v = minv + cap, *ucol = v + cap;
    int32_t *way = reinterpret_cast<int32_t *>(ucol + cap), *prow = way + cap;
    uint8_t *used = reinterpret_cast<uint8_t *>(prow + cap);

    const int p0 = a.pd_off[q], R = a.pd_off[q + 1] - p0, g0 = a.gt_off[q], C = a.gt_off[q + 1] - g0;
    const int f = q / WM_TYPES, t = q % WM_TYPES;
    if (R < 0 || C < 0 || R > a.max_pd || C > a.max_gt) {      // the host passed maxima smaller than its own offsets
        if (lane == 0) *a.flag = 1;
        return;
    }
    const double thr = a.thr[t];
    const double *W = a.iou + a.pair_off[q];
    const float *score = a.score + p0;
    int32_t *order = a.order + p0;

    for (int j = lane; j < C; j += 64) {
        v[j] = 0.0;
        ucol[j] = 0.0;
        prow[j] = -1;
    }
    // rank sort: order[rank] = row, rank = rows that come before it (higher score, or equal score and lower index)
    for (int i = lane; i < R; i += 64) {
        const uint32_t ki = float_key(wm_score(score[i]));
        int rank = 0;
        for (int j = 0; j < R; ++j) {
            const uint32_t kj = float_key(wm_score(score[j]));
            rank += (kj > ki || (kj == ki && j < i)) ? 1 : 0;
        }
        order[rank] = i;
    }
    __syncthreads();

    int pos = 0, nmatched = 0;
    int tp1 = 0, tp2 = 0, fn1 = 0, fn2 = 0;
    double ha1 = 0.0, ha2 = 0.0;
    for (int k = WM_CUTOFFS - 1; k >= 0; --k) {
        const float ck = (k == WM_CUTOFFS - 1) ? 1.0f : (float)((double)k * 0.01);
        int grew = 0;
        for (; pos < R; ++pos) {
            const int r = wm_uni(order[pos]);
            if (!wm_uni(wm_score(score[r]) >= ck ? 1 : 0)) break;
            grew = 1;
            // ---- insert row r: shortest augmenting path from r over the columns
            for (int j = lane; j < C; j += 64) {
                minv[j] = INFINITY;
                used[j] = 0;
            }
            double u_root = 0.0, cur_u = 0.0, dmin = INFINITY;
            int dcol = -1, cur_col = -1, cur_row = r;
            int end_col = -1, gained = 0;
            for (int it = 0; it <= C; ++it) {
                if (-cur_u < dmin) {                 // the scanned row's private column
                    dmin = -cur_u;
                    dcol = cur_col;
                }
                const double *wr = W + (int64_t)cur_row * C;
                double best = INFINITY;
                int bestj = INT_MAX;
                for (int j = lane; j < C; j += 64) {
                    if (used[j]) continue;
                    const double w = wr[j];
                    double m = minv[j];
                    if (w >= thr && w < INFINITY) {
                        const double c = -w - cur_u - v[j];
                        if (c < m) {
                            m = c;
                            minv[j] = c;
                            way[j] = cur_col;
                        }
                    }
                    if (m < best) {
                        best = m;
                        bestj = j;
                    }
                }
                wm_wave_argmin(best, bestj);
                const int to_col = wm_uni(best < dmin ? 1 : 0);
                const double delta = to_col ? best : dmin;
                u_root += delta;
                for (int j = lane; j < C; j += 64) {
                    if (used[j]) {
                        ucol[j] += delta;
                        v[j] -= delta;
                    } else {
                        minv[j] -= delta;
                    }
                }
                dmin -= delta;
                if (!to_col) {                        // a row of the tree leaves for its private column (dcol -1: r itself)
                    end_col = dcol;
                    break;
                }
                const int j1 = wm_uni(bestj);
                const int held = wm_uni(prow[j1]);    // prow changes only between searches (barrier below)
                if (held < 0) {                       // a free column ends the path
                    end_col = j1;
                    gained = 1;
                    break;
                }
                if (lane == (j1 & 63)) used[j1] = 1;
                __syncthreads();
                cur_col = j1;
                cur_row = held;
                cur_u = ucol[j1];
            }
            end_col = wm_uni(end_col);
            __syncthreads();
            if (end_col >= 0 && lane == 0) {          // shift the rows along the path; r takes the path's first column
                int j = end_col;
                for (int step = 0; step <= C; ++step) {
                    const int jp = way[j];
                    if (jp < 0) {
                        prow[j] = r;
                        ucol[j] = u_root;
                        break;
                    }
                    prow[j] = prow[jp];
                    ucol[j] = ucol[jp];
                    j = jp;
                }
            }
            __syncthreads();
            nmatched += wm_uni(gained);
        }
        if (grew || k == WM_CUTOFFS - 1) {            // otherwise the subset is the previous cut-off's: repeat its counts
            int a1 = 0, a2 = 0, b1 = 0, b2 = 0;
            double h1 = 0.0, h2 = 0.0;
            for (int j = lane; j < C; j += 64) {
                const int d = a.difficulty[g0 + j];
                const int l1 = d == 1, l2 = (d == 1 || d == 2);
                const int held = prow[j];
                if (held >= 0) {
                    a1 += l1;
                    a2 += l2;
                    if (l2) {
                        const double term = wm_heading_accuracy(a.pd_heading[p0 + held], a.gt_heading[g0 + j]);
                        h2 += term;
                        if (l1) h1 += term;
                    }
                } else {
                    b1 += l1;
                    b2 += l2;
                }
            }
            tp1 = wm_wave_sum(a1);
            tp2 = wm_wave_sum(a2);
            fn1 = wm_wave_sum(b1);
            fn2 = wm_wave_sum(b2);
            ha1 = wm_wave_sum(h1);
            ha2 = wm_wave_sum(h2);
        }
        if (lane == 0) {
            const int64_t o = ((int64_t)t * WM_CUTOFFS + k) * a.n_frames + f;
            int32_t *c = a.pcounts + 5 * o;
            c[0] = tp1;
            c[1] = tp2;
            c[2] = fn1;
            c[3] = fn2;
            c[4] = pos - nmatched;
            a.pha[2 * o] = ha1;
            a.pha[2 * o + 1] = ha2;
        }
    }
}

// counts[type][level][cut-off][tp, fp, fn] and ha[type][level][cut-off]: the per-problem results added in frame order, one lane
// per (type, cut-off); with `accumulate` they continue from the values already there
__global__ void __launch_bounds__(WM_THREADS) waymo_reduce_kernel(const int32_t *__restrict__ pcounts, const double *__restrict__ pha,
                                                                  const int32_t *__restrict__ flag, int n_frames, int accumulate,
                                                                  int64_t *__restrict__ counts, double *__restrict__ ha) {
    const int idx = blockIdx.x * WM_THREADS + threadIdx.x;
    if (idx >= WM_TYPES * WM_CUTOFFS) return;
    const int t = idx / WM_CUTOFFS, k = idx % WM_CUTOFFS;
    int64_t *c1 = counts + ((int64_t)(t * 2 + 0) * WM_CUTOFFS + k) * 3, *c2 = counts + ((int64_t)(t * 2 + 1) * WM_CUTOFFS + k) * 3;
    double *h1 = ha + (t * 2 + 0) * WM_CUTOFFS + k, *h2 = ha + (t * 2 + 1) * WM_CUTOFFS + k;
    if (*flag) {                                      // a problem was skipped: poison the result, the host raises
        for (int i = 0; i < 3; ++i) c1[i] = c2[i] = -1;
        *h1 = *h2 = NAN;
        return;
    }
    int64_t tp1 = 0, tp2 = 0, fn1 = 0, fn2 = 0, fp = 0, fp2 = 0;
    double s1 = 0.0, s2 = 0.0;
    if (accumulate) {
        tp1 = c1[0], fp = c1[1], fn1 = c1[2];
        tp2 = c2[0], fp2 = c2[1], fn2 = c2[2];
        s1 = *h1, s2 = *h2;
    }
    for (int f = 0; f < n_frames; ++f) {
        const int64_t o = (int64_t)idx * n_frames + f;
        const int32_t *c = pcounts + 5 * o;
        tp1 += c[0];
        tp2 += c[1];
        fn1 += c[2];
        fn2 += c[3];
        fp += c[4];
        fp2 += c[4];
        s1 += pha[2 * o];
        s2 += pha[2 * o + 1];
    }
    c1[0] = tp1, c1[1] = fp, c1[2] = fn1;
    c2[0] = tp2, c2[1] = fp2, c2[2] = fn2;
    *h1 = s1;
    *h2 = s2;
}

struct WmLayout {
    size_t order, pcounts, pha, flag, total;
};
WmLayout wm_layout(int n_problems, int total_pd) {
    Carve c;
    WmLayout l;
    const size_t rows = (size_t)(n_problems / WM_TYPES) * WM_TYPES * WM_CUTOFFS;
    l.order = c.take((size_t)total_pd * sizeof(int32_t));
    l.pcounts = c.take(rows * 5 * sizeof(int32_t));
    l.pha = c.take(rows * 2 * sizeof(double));
    l.flag = c.take(sizeof(int32_t));
    l.total = c.o;
    return l;
}

}  // namespace

// the two IoU entry points differ in the kernel alone
static int wm_launch_iou(void (*kernel)(WmIouArgs), const char *label, const float *pd_boxes, const float *gt_boxes,
                         const int32_t *pd_off, const int32_t *gt_off, const int64_t *pair_off, int n_problems, int64_t n_pairs,
                         double *out, cpd_stream_t st) {
    if (n_problems <= 0 || n_pairs < 0 || !pd_off || !gt_off || !pair_off) return CPD_ERR_ARG;
    if (n_pairs == 0) return CPD_OK;
    if (!pd_boxes || !gt_boxes || !out) return CPD_ERR_ARG;
    if (n_pairs > ((int64_t)1 << 40)) return CPD_ERR_UNSUPPORTED;
    WmIouArgs a;
    a.pd = pd_boxes; a.gt = gt_boxes; a.pd_off = pd_off; a.gt_off = gt_off; a.pair_off = pair_off;
    a.n_problems = n_problems; a.n_pairs = n_pairs; a.out = out;
    cpd_launch_log_note(label);
    const int64_t blocks = (n_pairs + WM_THREADS - 1) / WM_THREADS;     // capped: the kernel strides over the rest
    kernel<<<(unsigned)(blocks < 65536 ? blocks : 65536), WM_THREADS, 0, cpd_s(st)>>>(a);
    return cpd_check_launch();
}

extern "C" int cpd_waymo_iou(const float *pd_boxes, const float *gt_boxes, const int32_t *pd_off, const int32_t *gt_off,
                             const int64_t *pair_off, int n_problems, int64_t n_pairs, double *out, cpd_stream_t st) {
    return wm_launch_iou(waymo_iou_kernel, "waymo_iou_kernel", pd_boxes, gt_boxes, pd_off, gt_off, pair_off, n_problems, n_pairs,
                         out, st);
}

extern "C" int cpd_waymo_iou_bev(const float *pd_boxes, const float *gt_boxes, const int32_t *pd_off, const int32_t *gt_off,
                                 const int64_t *pair_off, int n_problems, int64_t n_pairs, double *out, cpd_stream_t st) {
    return wm_launch_iou(waymo_iou_bev_kernel, "waymo_iou_bev_kernel", pd_boxes, gt_boxes, pd_off, gt_off, pair_off, n_problems,
                         n_pairs, out, st);
}

extern "C" size_t cpd_waymo_match_workspace_bytes(int n_problems, int total_pd) {
    if (n_problems <= 0 || n_problems % WM_TYPES != 0 || total_pd < 0) return 0;
    return wm_layout(n_problems, total_pd).total;
}

extern "C" int cpd_waymo_match(const double *iou, const int64_t *pair_off, const int32_t *pd_off, const int32_t *gt_off,
                               int n_problems, int total_pd, int total_gt, const float *pd_score, const uint8_t *gt_difficulty,
                               const float *pd_heading, const float *gt_heading, const double *iou_thresholds, int max_pd,
                               int max_gt, int accumulate, int64_t *counts, double *ha, void *workspace, size_t workspace_bytes,
                               cpd_stream_t st) {
    if (n_problems <= 0 || n_problems % WM_TYPES != 0 || total_pd < 0 || total_gt < 0 || max_pd < 0 || max_gt < 0) return CPD_ERR_ARG;
    if (!pair_off || !pd_off || !gt_off || !iou_thresholds || !counts || !ha) return CPD_ERR_ARG;
    if ((total_pd > 0 && (!pd_score || !pd_heading)) || (total_gt > 0 && (!gt_difficulty || !gt_heading))) return CPD_ERR_ARG;
    if (total_pd > 0 && total_gt > 0 && !iou) return CPD_ERR_ARG;
    if (max_pd > total_pd || max_gt > total_gt) return CPD_ERR_ARG;
    if (max_pd > CPD_WAYMO_MAX_PD || max_gt > CPD_WAYMO_MAX_GT) return CPD_ERR_UNSUPPORTED;
    const WmLayout l = wm_layout(n_problems, total_pd);
    if (!workspace || workspace_bytes < l.total) return CPD_ERR_WORKSPACE;
    WmMatchArgs a;
    a.iou = iou; a.pair_off = pair_off; a.pd_off = pd_off; a.gt_off = gt_off;
    a.score = pd_score; a.difficulty = gt_difficulty; a.pd_heading = pd_heading; a.gt_heading = gt_heading;
    for (int t = 0; t < WM_TYPES; ++t) a.thr[t] = iou_thresholds[t];
    a.n_frames = n_problems / WM_TYPES; a.max_pd = max_pd; a.max_gt = max_gt;
    a.cap = (max_gt + 63) / 64 * 64;
    if (a.cap == 0) a.cap = 64;
    a.order = ws_at<int32_t>(workspace, l.order);
    a.pcounts = ws_at<int32_t>(workspace, l.pcounts);
    a.pha = ws_at<double>(workspace, l.pha);
    a.flag = ws_at<int32_t>(workspace, l.flag);
    CPD_HIP_TRY(hipMemsetAsync(a.flag, 0, sizeof(int32_t), cpd_s(st)));
    // minv, v, ucol (float64), way, prow (int32), used (bytes) per column: 33 KiB at the 1024-column cap
    const size_t lds = (size_t)a.cap * (3 * sizeof(double) + 2 * sizeof(int32_t) + 1);
    cpd_launch_log_note("waymo_match_kernel");
    waymo_match_kernel<<<(unsigned)n_problems, 64, lds, cpd_s(st)>>>(a);
    int e = cpd_check_launch();
    if (e != CPD_OK) return e;
    cpd_launch_log_note("waymo_reduce_kernel");
    waymo_reduce_kernel<<<(unsigned)cpd_div_up(WM_TYPES * WM_CUTOFFS, WM_THREADS), WM_THREADS, 0, cpd_s(st)>>>(
        a.pcounts, a.pha, a.flag, a.n_frames, accumulate ? 1 : 0, counts, ha);
    return cpd_check_launch();
}
