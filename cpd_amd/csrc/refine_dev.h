// refine_dev.h -- device code of density_guided_drift (outline_utils.py:41-92) and correct_orientation (l.127-326) shared by
// cproto_refine.hip (C_PROTO's refine_box_size: the chosen cluster is a contiguous run of rows) and mfcf.hip (box_fit_DGD: the
// cluster is the rows of a frame with one DBSCAN label above a height cut). A cluster type C gives
//   c.n      the rows to walk, c.count the rows among them that belong to the cluster,
//   c.row(i, x, y, z)  false where row i does not belong.
// One RF_THREADS workgroup per cluster re-reads the rows on every pass. Minima, maxima and integer counts are the only
// reductions over rows (wave shuffles, then LDS), the per-bin extreme row is an integer LDS atomic on an order-preserving key
// followed by an atomicMin on the row index (ties: the lowest row, numpy's first occurrence), and the at most seven picked
// rows per half are added by one thread in bin order: no float atomics, the same bits for any launch geometry.
// Both files are built with -ffp-contract=off: no fused multiply-add anywhere in this code.
#pragma once
#include <math.h>

#include "common.h"

namespace {

constexpr int RF_THREADS = 256;
constexpr int RF_PARTS = 7;             // correct_orientation's parts
constexpr int RF_NO_ROW = 0x7fffffff;

struct Cluster {
    const float *xyz;     // the segment's rows
    int n, count;
    __device__ __forceinline__ bool row(int i, double &x, double &y, double &z) const {
        x = xyz[3 * (size_t)i], y = xyz[3 * (size_t)i + 1], z = xyz[3 * (size_t)i + 2];
        return true;
    }
};

struct Stats {
    double min_x, max_x, min_y, max_y;
    int pos_x, pos_y;     // rows with X > 0, Y > 0
};

// the box-frame coordinates of row i: the reference's cloud @ trans_mat_i.T, written out and unfused
template <class C>
__device__ __forceinline__ bool rf_xy(const C &c, int i, const double *m, double &X, double &Y) {
    double x, y, z;
    if (!c.row(i, x, y, z)) return false;
    X = ((x * m[0] + y * m[1]) + z * m[2]) + m[3];
    Y = ((x * m[4] + y * m[5]) + z * m[6]) + m[7];
    return true;
}

// min / max of X and Y and the counts of positive X and Y over the cluster, the same in every thread. smd: 16 doubles,
// smi: 8 ints of LDS, free again on return.
template <class C>
__device__ __forceinline__ Stats rf_stats(const C &c, const double *m, double *smd, int *smi) {
    Stats t = {INFINITY, -INFINITY, INFINITY, -INFINITY, 0, 0};
    for (int i = threadIdx.x; i < c.n; i += RF_THREADS) {
        double X, Y;
        if (!rf_xy(c, i, m, X, Y)) continue;
        t.min_x = fmin(t.min_x, X), t.max_x = fmax(t.max_x, X);
        t.min_y = fmin(t.min_y, Y), t.max_y = fmax(t.max_y, Y);
        t.pos_x += X > 0 ? 1 : 0, t.pos_y += Y > 0 ? 1 : 0;
    }
    for (int d = 32; d; d >>= 1) {
        t.min_x = fmin(t.min_x, __shfl_xor(t.min_x, d, 64)), t.max_x = fmax(t.max_x, __shfl_xor(t.max_x, d, 64));
        t.min_y = fmin(t.min_y, __shfl_xor(t.min_y, d, 64)), t.max_y = fmax(t.max_y, __shfl_xor(t.max_y, d, 64));
        t.pos_x += __shfl_xor(t.pos_x, d, 64), t.pos_y += __shfl_xor(t.pos_y, d, 64);
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) {
        smd[4 * w] = t.min_x, smd[4 * w + 1] = t.max_x, smd[4 * w + 2] = t.min_y, smd[4 * w + 3] = t.max_y;
        smi[2 * w] = t.pos_x, smi[2 * w + 1] = t.pos_y;
    }
    __syncthreads();
    t = {smd[0], smd[1], smd[2], smd[3], smi[0], smi[1]};
    for (int k = 1; k < RF_THREADS / 64; ++k) {
        t.min_x = fmin(t.min_x, smd[4 * k]), t.max_x = fmax(t.max_x, smd[4 * k + 1]);
        t.min_y = fmin(t.min_y, smd[4 * k + 2]), t.max_y = fmax(t.max_y, smd[4 * k + 3]);
        t.pos_x += smi[2 * k], t.pos_y += smi[2 * k + 1];
    }
    __syncthreads();
    return t;
}

// density_guided_drift's new centre from the cluster's extent in the box frame (one thread)
__device__ __forceinline__ void rf_drift_box(const double *b, const Stats &t, int n, double *out) {
    // the reference's float32 trans_mat: cos yaw, sin yaw, x, y rounded to float32
    const double c = (double)(float)cos(b[6]), s = (double)(float)sin(b[6]);
    const double x = (double)(float)b[0], y = (double)(float)b[1];
    const double l = b[3], w = b[4];
    const double cx = 2 * (long long)t.pos_x > n ? -(l / 2 - t.max_x) : -(-l / 2 - t.min_x);
    const double cy = 2 * (long long)t.pos_y > n ? -(w / 2 - t.max_y) : -(-w / 2 - t.min_y);
    out[0] = (cx * c + cy * (-s)) + x;
    out[1] = (cx * s + cy * c) + y;
    for (int k = 2; k < 7; ++k) out[k] = b[k];
}

__device__ __forceinline__ unsigned long long rf_dkey(double v) {      // order-preserving key of a double, -0.0 as 0.0
    if (v == 0.0) v = 0.0;
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    return (u & 0x8000000000000000ull) ? ~u : (u | 0x8000000000000000ull);
}

// the bin of coordinate u: 0..6 the top half's (mid + i*delta, mid + (i+1)*delta], 7..13 the bottom half's
// (lo + i*delta, lo + (i+1)*delta], -1 none (u == mid, u == lo, or past the last bound)
__device__ __forceinline__ int rf_bin(double u, double lo, double mid, double delta) {
    if (u > mid) {
        for (int i = 0; i < RF_PARTS; ++i)
            if (u > mid + i * delta && u <= mid + (i + 1) * delta) return i;
    } else if (u < mid) {
        for (int i = 0; i < RF_PARTS; ++i)
            if (u > lo + i * delta && u <= lo + (i + 1) * delta) return RF_PARTS + i;
    }
    return -1;
}

// the closed-form inverse (rows 0 and 1) of the float32 trans_mat of a box at (bx, by) with heading yaw, as the host forms it
// (cproto.inverse_box_rows): float64 over the float32 entries, rounded to float32
__device__ __forceinline__ void rf_inverse_rows(double bx, double by, double yaw, float *mo) {
    const double cs = (double)(float)cos(yaw), sn = (double)(float)sin(yaw);
    const double x = (double)(float)bx, y = (double)(float)by;
    const double d = cs * cs + sn * sn;
    mo[0] = (float)(cs / d), mo[1] = (float)(sn / d), mo[2] = 0.0f, mo[3] = (float)(-(cs * x + sn * y) / d);
    mo[4] = (float)(-sn / d), mo[5] = (float)(cs / d), mo[6] = 0.0f, mo[7] = (float)((sn * x - cs * y) / d);
}

struct Orient {
    double yaw;
    bool by_x, take_max, turned;
};

// correct_orientation on a cluster whose Stats are t: the new heading and the branches taken, valid in thread 0 only (every
// thread of the workgroup must call it). bkey: 14 unsigned long long, brow: 14 ints of LDS.
template <class C>
__device__ __forceinline__ Orient rf_orient(const C &c, const double *b, const double *m, const Stats &t,
                                            unsigned long long *bkey, int *brow) {
    Orient o;
    o.by_x = ((t.max_x - t.min_x) / b[3]) * 2 > ((t.max_y - t.min_y) / b[4]);
    const bool by_x = o.by_x;
    const double lo = by_x ? t.min_x : t.min_y, hi = by_x ? t.max_x : t.max_y;
    const double mid = (hi - lo) / 2. + lo;
    const double delta = (hi - mid) / RF_PARTS;
    o.take_max = 2 * (long long)(by_x ? t.pos_y : t.pos_x) > c.count;
    const bool take_max = o.take_max;
    o.yaw = b[6], o.turned = false;
    if (threadIdx.x < 2 * RF_PARTS) bkey[threadIdx.x] = 0ull, brow[threadIdx.x] = RF_NO_ROW;
    __syncthreads();
    for (int pass = 0; pass < 2; ++pass) {      // the extreme key of every bin, then the lowest row that holds it
        for (int i = threadIdx.x; i < c.n; i += RF_THREADS) {
            double X, Y;
            if (!rf_xy(c, i, m, X, Y)) continue;
            const int bin = rf_bin(by_x ? X : Y, lo, mid, delta);
            if (bin < 0) continue;
            const unsigned long long k = rf_dkey(by_x ? Y : X);
            const unsigned long long key = take_max ? k : ~k;
            if (pass == 0) atomicMax(&bkey[bin], key);
            else if (key == bkey[bin]) atomicMin(&brow[bin], i);
        }
        __syncthreads();
    }
    if (threadIdx.x != 0) return o;
    double sum[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
    int picked[2] = {0, 0};
    for (int half = 0; half < 2; ++half)
        for (int i = 0; i < RF_PARTS; ++i) {
            const int r = brow[half * RF_PARTS + i];
            if (r == RF_NO_ROW) continue;
            double X, Y;
            rf_xy(c, r, m, X, Y);
            sum[half][0] = picked[half] ? sum[half][0] + X : X;
            sum[half][1] = picked[half] ? sum[half][1] + Y : Y;
            ++picked[half];
        }
    o.turned = picked[0] > 0 && picked[1] > 0;
    if (o.turned) {
        const double dX = sum[0][0] / picked[0] - sum[1][0] / picked[1];
        const double dY = sum[0][1] / picked[0] - sum[1][1] / picked[1];
        o.yaw += by_x ? atan(dY / dX) : atan(dX / dY);
    }
    return o;
}

}  // namespace
