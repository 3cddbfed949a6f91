// oyster.hip -- the numeric work that is the OYSTER pseudo-label generator's own (cpd/unsupervised_core/oyster.py:89-115 and
// outline_utils.py corner_align, l.94-123): the size consensus of a track and the corner alignment of each of its boxes, for
// every qualifying track of a sequence in one launch, one workgroup per track:
//   1. dis = sqrt((x*x + y*y) + z*z) per row; a row's rank is the number of rows that sort before it (smaller dis, ties to the
//      lower row; NaN last) -- counted against LDS tiles of OY_TILE distances, any track length;
//   2. the rows of rank < top hand their l and w to LDS slots at their rank (windows of OY_SEL ranks, any top) and one thread
//      adds them in rank order: np.mean(axis=0) adds rows one after another;
//   3. per row the four candidate centres (+-l_off/2, +-w_off/2) go through the box's float32 pose in float64, the one of
//      greatest norm of (x', y', z', 1) wins, the first on ties, and l, w take the offsets.
// No reduction whose order depends on the schedule: the same bits on every launch.
// Built with -ffp-contract=off: the sums of squares, the products with the float32 pose entries and l + (mean_l - l) are
// numpy's expressions op by op.
#include <math.h>

#include "common.h"

namespace {

constexpr int OY_THREADS = 256;
constexpr int OY_TILE = 1024;     // distances staged per counting step
constexpr int OY_SEL = 256;       // ranks collected per summing step

struct AlignArgs {
    const double *boxes;
    const int32_t *off, *top;
    int n_rows;
    double *out;
};

__device__ __forceinline__ double oy_dis(const double *b) { return sqrt((b[0] * b[0] + b[1] * b[1]) + b[2] * b[2]); }

// argsort's order: ascending, NaN last, ties to the lower row
__device__ __forceinline__ bool oy_before(double dj, int j, double di, int i) {
    if (di != di) return dj == dj || j < i;
    return dj < di || (dj == di && j < i);
}

__global__ void __launch_bounds__(OY_THREADS) oy_align_kernel(AlignArgs a) {
    __shared__ double s_dis[OY_TILE];
    __shared__ double s_l[OY_SEL], s_w[OY_SEL];
    __shared__ double s_mean[2];
    const int tid = threadIdx.x;
    const int o0 = a.off[blockIdx.x], o1 = a.off[blockIdx.x + 1];
    if (o0 < 0 || o1 > a.n_rows || o1 <= o0) return;         // an empty track, or offsets outside the rows: nothing is touched
    const int n = o1 - o0;
    const double *box = a.boxes + (size_t)o0 * 7;
    int top = a.top[blockIdx.x];
    top = top < 1 ? 1 : (top > n ? n : top);                  // new_objects_sort[0:top_len] of a shorter track is all of it

    double sum_l = 0.0, sum_w = 0.0;                          // thread 0's
    for (int r0 = 0; r0 < top; r0 += OY_SEL) {
        const int r1 = min(r0 + OY_SEL, top);
        for (int i0 = 0; i0 < n; i0 += OY_THREADS) {
            const int i = i0 + tid;
            const double di = i < n ? oy_dis(box + 7 * (size_t)i) : 0.0;
            int rank = 0;
            for (int j0 = 0; j0 < n; j0 += OY_TILE) {
                const int m = min(OY_TILE, n - j0);
                __syncthreads();
                for (int j = tid; j < m; j += OY_THREADS) s_dis[j] = oy_dis(box + 7 * (size_t)(j0 + j));
                __syncthreads();
                if (i < n)
                    for (int j = 0; j < m; ++j) rank += oy_before(s_dis[j], j0 + j, di, i) ? 1 : 0;
            }
            if (i < n && rank >= r0 && rank < r1) {           // the ranks are a permutation: every slot below is written once
                s_l[rank - r0] = box[7 * (size_t)i + 3];
                s_w[rank - r0] = box[7 * (size_t)i + 4];
            }
        }
        __syncthreads();
        if (tid == 0)
            for (int r = 0; r < r1 - r0; ++r) sum_l += s_l[r], sum_w += s_w[r];
        __syncthreads();
    }
    if (tid == 0) s_mean[0] = sum_l / (double)top, s_mean[1] = sum_w / (double)top;
    __syncthreads();
    const double mean_l = s_mean[0], mean_w = s_mean[1];

    for (int i = tid; i < n; i += OY_THREADS) {
        const double *b = box + 7 * (size_t)i;
        double *o = a.out + 7 * (size_t)(o0 + i);
        const double l = b[3], w = b[4], yaw = b[6];
        const double l_off = mean_l - l, w_off = mean_w - w;
        // trans_mat is float32: its entries are rounded, the products and sums with the float64 corners are not
        const double c = (double)(float)cos(yaw), s = (double)(float)sin(yaw);
        const double tx = (double)(float)b[0], ty = (double)(float)b[1], tz = (double)(float)b[2];
        const double hx = l_off / 2, hy = w_off / 2;
        double best = 0.0, bx = 0.0, by = 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {                         // (+, +), (-, -), (+, -), (-, +)
            const double cx = (k == 0 || k == 2) ? hx : -hx, cy = (k == 0 || k == 3) ? hy : -hy;
            const double px = (cx * c + cy * (-s)) + tx, py = (cx * s + cy * c) + ty;
            const double d = sqrt(((px * px + py * py) + tz * tz) + 1.0);
            // np.argmax: the first of the greatest; a NaN counts as the greatest
            if (k == 0 || (best == best && (d > best || d != d))) best = d, bx = px, by = py;
        }
        o[0] = bx, o[1] = by, o[2] = tz;
        o[3] = l + l_off, o[4] = w + w_off, o[5] = b[5], o[6] = yaw;
    }
}

}  // namespace

extern "C" {

int cpd_oyster_align_tracks(const double *boxes, const int32_t *track_off, const int32_t *track_top, int n_tracks, int n_rows,
                            double *out, cpd_stream_t stream) {
    if (n_tracks < 0 || n_rows < 0) return CPD_ERR_ARG;
    if (n_tracks == 0 || n_rows == 0) return CPD_OK;
    if (!boxes || !track_off || !track_top || !out) return CPD_ERR_ARG;
    AlignArgs a;
    a.boxes = boxes, a.off = track_off, a.top = track_top, a.n_rows = n_rows, a.out = out;
    oy_align_kernel<<<n_tracks, OY_THREADS, 0, cpd_s(stream)>>>(a);
    return cpd_check_launch();
}

}  // extern "C"
