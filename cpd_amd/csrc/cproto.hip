// cproto.hip -- the first stage of CPD's C_PROTO refiner (cpd/unsupervised_core/c_proto_refine.py:65-195
// compute_css_score_and_raw_proto; outline_utils.py smooth_points l.391-396, compute_confidence l.398-436) for a batch of
// SEGMENTS, one segment = one (frame, box) pair of a chunk of frames:
//   1. cpd_cproto_crop_count / cpd_cproto_crop_fill : the radius crop sqrt(dx*dx + dy*dy) < max(l, w) in float64, rows kept
//      in input order and in the input dtype (count, scan, fill);
//   2. cpd_cproto_filter : smooth_points (neighbours within 0.2 m, self included, count > 3) by an LDS-tiled all-pairs count,
//      z_min / new_box, and the height window z > T(z_min + 0.2), z < z_max with T in the frame's dtype;
//   (ground removal and DBSCAN: cpd_outline_ground / cpd_outline_dbscan of outline.hip, a segment as a "frame")
//   3. cpd_cproto_score : the first largest valid cluster, its rows in the box frame (float64, unfused) and per `parts` the
//      number of cells holding more than one row, by the reference's own bound expressions.
// Every per-segment compaction is ordered: the four waves of a workgroup own contiguous quarters of the segment and place
// their rows by ballot ranks, so rows keep their order and every call gives the same bits. Integer atomics only.
// Built with -ffp-contract=off: no fused multiply-add anywhere in this file.
#include <math.h>

#include "common.h"

namespace {

constexpr int CP_THREADS = 256;
constexpr int CP_MAX_PARTS = 4;       // len(MLOParts)
constexpr int CP_MAX_PART = 16;       // largest MLOParts value
constexpr int CP_MAX_SEGMENTS = 1022; // + the tail segment = cpd_outline_dbscan's 1023 frames

__device__ __forceinline__ void cp_store3(void *p, int is_half, long long r, float x, float y, float z) {
    if (is_half) {
        _Float16 *q = static_cast<_Float16 *>(p) + r * 3;
        q[0] = (_Float16)x, q[1] = (_Float16)y, q[2] = (_Float16)z;
    } else {
        float *q = static_cast<float *>(p) + r * 3;
        q[0] = x, q[1] = y, q[2] = z;
    }
}

__device__ __forceinline__ int cp_wave_sum(int v) {
    for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// Ordered compaction of the items 0..n-1 of one segment by one workgroup of four waves: wave w owns the contiguous quarter
// [w * q, (w + 1) * q), counts its kept items, and after one barrier places them at (kept items of the waves before it) + its
// own ballot rank. emit(i, pos) is called for every kept item; returns the segment's kept count. pred is evaluated twice.
// sm4: four ints of LDS. With count_only no item is emitted.
template <class Pred, class Emit>
__device__ __forceinline__ int cp_compact(int n, int *sm4, bool count_only, Pred pred, Emit emit) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int q = ((n + 3) / 4 + 63) / 64 * 64;
    const int b0 = min(n, w * q), b1 = min(n, (w + 1) * q);
    int c = 0;
    for (int i = b0 + lane; i < b1; i += 64) c += pred(i) ? 1 : 0;
    c = cp_wave_sum(c);
    if (lane == 0) sm4[w] = c;
    __syncthreads();
    int base = 0, total = 0;
    for (int k = 0; k < 4; ++k) {
        if (k < w) base += sm4[k];
        total += sm4[k];
    }
    if (!count_only) {
        const unsigned long long lt = (1ull << lane) - 1ull;
        for (int i0 = b0; i0 < b1; i0 += 64) {
            const int i = i0 + lane;
            const bool k = i < b1 && pred(i);
            const unsigned long long m = __ballot(k);
            if (k) emit(i, base + __popcll(m & lt));
            base += __popcll(m);
        }
    }
    __syncthreads();
    return total;
}

// counts [n] -> offsets [n + 1] (one workgroup); extra_last: one more entry off[n + 1] = that value (or none when < 0)
__global__ void __launch_bounds__(1024) cp_offsets_kernel(const int32_t *counts, int n, int32_t *off, int extra_last) {
    __shared__ uint32_t sm[17];
    uint32_t carry = 0;
    for (int base = 0; base < n; base += 1024) {
        const int i = base + threadIdx.x;
        const uint32_t v = i < n ? (uint32_t)counts[i] : 0u;
        uint32_t tot;
        const uint32_t ex = block_excl_scan(v, sm, &tot);
        if (i < n) off[i] = (int32_t)(carry + ex);
        carry += tot;
    }
    if (threadIdx.x == 0) {
        off[n] = (int32_t)carry;
        if (extra_last >= 0) off[n + 1] = extra_last;
    }
}

// ---- 1. radius crop (c_proto_refine.py:120-123) ---------------------------------------------------------------------------

struct CropArgs {
    const void *points;
    int is_half, stride, n_frames, n_segments, row_cap;
    const int32_t *frame_off, *seg_frame;
    const double *boxes;
    int32_t *counts;          // [S]
    const int32_t *seg_off;   // [S + 1]
    void *out_rows;
    int32_t *out_src;
};

struct CropTest {
    const void *points;
    int is_half, stride;
    long long base;
    double bx, by, rad;
    __device__ __forceinline__ bool operator()(int i) const {
        float x, y, z;
        load_xyz(points, is_half, stride, base + i, x, y, z);
        const double dx = (double)x - bx, dy = (double)y - by;
        return sqrt(dx * dx + dy * dy) < rad;
    }
};
__device__ __forceinline__ bool cp_crop_setup(const CropArgs &a, int s, CropTest &t, int &n) {
    const int f = a.seg_frame[s];
    n = 0;
    if (f < 0 || f >= a.n_frames) return false;
    const double *b = a.boxes + (size_t)s * 7;
    t.points = a.points, t.is_half = a.is_half, t.stride = a.stride;
    t.base = a.frame_off[f];
    t.bx = b[0], t.by = b[1], t.rad = fmax(b[3], b[4]);
    n = a.frame_off[f + 1] - a.frame_off[f];
    return n > 0;
}

__global__ void __launch_bounds__(CP_THREADS) cp_crop_count_kernel(CropArgs a) {
    __shared__ int sm4[4];
    const int s = blockIdx.x;
    CropTest t;
    int n;
    cp_crop_setup(a, s, t, n);
    const int total = cp_compact(n, sm4, true, t, [](int, int) {});
    if (threadIdx.x == 0) a.counts[s] = total;
}

__global__ void __launch_bounds__(CP_THREADS) cp_crop_fill_kernel(CropArgs a) {
    __shared__ int sm4[4];
    const int s = blockIdx.x;
    CropTest t;
    int n;
    cp_crop_setup(a, s, t, n);
    const int o0 = a.seg_off[s], room = min(a.seg_off[s + 1], a.row_cap) - o0;
    cp_compact(n, sm4, false, t, [&](int i, int pos) {
        if (pos >= room) return;   // the offsets are this test's own counts: never taken
        float x, y, z;
        load_xyz(a.points, a.is_half, a.stride, t.base + i, x, y, z);
        cp_store3(a.out_rows, a.is_half, o0 + pos, x, y, z);
        a.out_src[o0 + pos] = i;
    });
}

// ---- 2. smooth_points + z_min / new_box + height window (outline_utils.py:391-396, c_proto_refine.py:125-147) -----------------

struct FilterArgs {
    const void *rows;         // [n_rows][3] of the dtype
    int is_half, n_segments, n_rows;
    const int32_t *seg_off, *crop_src;
    const double *boxes;
    double rad2;
    uint8_t *mask;            // [n_rows] density mask
    double *z_min, *new_box;
    int32_t *had;
    float *thr;               // [S] T(z_min + 0.2) as a float
    int32_t *counts;          // [S]
    int32_t *filt_off;        // [S + 2]
    void *filt_rows;
    int32_t *filt_src;
};

// neighbours within rad of every row, among the rows of its own segment: a workgroup owns 256 consecutive rows and walks
// the rows of the segments they belong to through LDS in tiles of 256
__global__ void __launch_bounds__(CP_THREADS) cp_density_kernel(FilterArgs a) {
    __shared__ float tx[CP_THREADS], ty[CP_THREADS], tz[CP_THREADS];
    const int i = blockIdx.x * CP_THREADS + threadIdx.x;
    const int first = blockIdx.x * CP_THREADS, last = min(first + CP_THREADS, a.n_rows) - 1;
    const int j0 = a.seg_off[segment_of(a.seg_off, a.n_segments, first)];
    const int j1 = a.seg_off[segment_of(a.seg_off, a.n_segments, last) + 1];
    int s0 = 0, s1 = 0;
    double x = 0.0, y = 0.0, z = 0.0;
    if (i < a.n_rows) {
        const int s = segment_of(a.seg_off, a.n_segments, i);
        s0 = a.seg_off[s], s1 = a.seg_off[s + 1];
        float fx, fy, fz;
        load_xyz(a.rows, a.is_half, 3, i, fx, fy, fz);
        x = fx, y = fy, z = fz;
    }
    int cnt = 0;
    for (int t0 = j0; t0 < j1; t0 += CP_THREADS) {
        const int j = t0 + threadIdx.x;
        if (j < j1) load_xyz(a.rows, a.is_half, 3, j, tx[threadIdx.x], ty[threadIdx.x], tz[threadIdx.x]);
        __syncthreads();
        const int k0 = max(t0, s0) - t0, k1 = min(min(t0 + CP_THREADS, j1), s1) - t0;
        for (int k = k0; k < k1; ++k) {
            const double dx = x - (double)tx[k], dy = y - (double)ty[k], dz = z - (double)tz[k];
            cnt += ((dx * dx + dy * dy) + dz * dz <= a.rad2) ? 1 : 0;
        }
        __syncthreads();
    }
    if (i < a.n_rows) a.mask[i] = cnt > 3 ? 1 : 0;
}

struct WindowTest {
    const void *rows;
    const uint8_t *mask;
    int is_half;
    long long base;
    float thr;
    double z_max;
    __device__ __forceinline__ bool operator()(int i) const {
        if (!mask[base + i]) return false;
        float x, y, z;
        load_xyz(rows, is_half, 3, base + i, x, y, z);
        return z > thr && (double)z < z_max;
    }
};

// one workgroup per segment: z_min over the dense rows, new_box, the window threshold and the window count
__global__ void __launch_bounds__(CP_THREADS) cp_zmin_kernel(FilterArgs a) {
    __shared__ int sm4[4];
    __shared__ uint32_t s_key;
    __shared__ int s_kept;
    const int s = blockIdx.x;
    const int o0 = a.seg_off[s], n = a.seg_off[s + 1] - o0;
    if (threadIdx.x == 0) s_key = 0xffffffffu, s_kept = 0;
    __syncthreads();
    uint32_t key = 0xffffffffu;
    int kept = 0;
    for (int i = threadIdx.x; i < n; i += CP_THREADS) {
        if (!a.mask[o0 + i]) continue;
        float x, y, z;
        load_xyz(a.rows, a.is_half, 3, o0 + i, x, y, z);
        key = min(key, float_key(z));
        ++kept;
    }
    if (kept) {
        atomicMin(&s_key, key);
        atomicAdd(&s_kept, kept);
    }
    __syncthreads();
    const bool had = s_kept > 0;
    const double *b = a.boxes + (size_t)s * 7;
    const float zf = had ? float_unkey(s_key) : 0.0f;
    const double z_min = had ? (double)zf : b[2] - b[5] / 2;
    const double z_max = b[2] + b[5] / 2;
    // z_min + 0.2 as numpy 2 evaluates it: the Python float becomes the scalar's dtype, the sum is rounded to it
    const float thr = a.is_half ? round_half(zf + round_half(0.2f)) : zf + 0.2f;
    if (threadIdx.x == 0) {
        double h = z_max - z_min;
        double zc = h / 2 + z_min;
        if (h < 1.3) {
            // the reference assigns the Python float 1.3: with z_min a scalar of the frame's dtype, h/2 + z_min is then
            // the sum in that dtype (numpy 2); without dense rows z_min is a float64 and so is the sum
            h = 1.3;
            zc = !had ? 1.3 / 2 + z_min : (double)(a.is_half ? round_half(round_half(0.65f) + zf) : 0.65f + zf);
        }
        double *nb = a.new_box + (size_t)s * 7;
        nb[0] = b[0], nb[1] = b[1], nb[2] = zc, nb[3] = b[3], nb[4] = b[4], nb[5] = h, nb[6] = b[6];
        a.z_min[s] = z_min;
        a.had[s] = had ? 1 : 0;
        a.thr[s] = thr;
    }
    WindowTest t = {a.rows, a.mask, a.is_half, o0, thr, z_max};
    const int total = cp_compact(had ? n : 0, sm4, true, t, [](int, int) {});
    if (threadIdx.x == 0) a.counts[s] = total;
}

// workgroup s < S: the window rows of segment s, order kept; workgroup S: the rows past the last segment are zeroed (they
// form one more, empty, segment for the ground kernel, whose row count is the crop's)
__global__ void __launch_bounds__(CP_THREADS) cp_window_fill_kernel(FilterArgs a) {
    __shared__ int sm4[4];
    const int s = blockIdx.x;
    if (s == a.n_segments) {
        for (int r = a.filt_off[s] + threadIdx.x; r < a.n_rows; r += CP_THREADS) {
            cp_store3(a.filt_rows, a.is_half, r, 0.0f, 0.0f, 0.0f);
            a.filt_src[r] = -1;
        }
        return;
    }
    const int o0 = a.seg_off[s], n = a.seg_off[s + 1] - o0;
    const double *b = a.boxes + (size_t)s * 7;
    WindowTest t = {a.rows, a.mask, a.is_half, o0, a.thr[s], b[2] + b[5] / 2};
    const int f0 = a.filt_off[s], room = min(a.filt_off[s + 1], a.n_rows) - f0;
    cp_compact(a.had[s] ? n : 0, sm4, false, t, [&](int i, int pos) {
        if (pos >= room) return;
        float x, y, z;
        load_xyz(a.rows, a.is_half, 3, o0 + i, x, y, z);
        cp_store3(a.filt_rows, a.is_half, f0 + pos, x, y, z);
        a.filt_src[f0 + pos] = a.crop_src[o0 + i];
    });
}

struct FilterLayout {
    size_t thr, counts, total;
};
FilterLayout filter_layout(int n_segments) {
    FilterLayout L;
    Carve c;
    L.thr = c.take((size_t)n_segments * 4);
    L.counts = c.take((size_t)n_segments * 4);
    L.total = c.o;
    return L;
}

// ---- 3. largest valid cluster + occupancy counts (outline_utils.py:789-807, 398-436; c_proto_refine.py:151-159) -------------

struct ScoreArgs {
    const float *xyz;            // [n_rows][3] non-ground rows (cpd_outline_ground's out_xyz)
    const int32_t *ng_src;       // row within the segment's filtered slice
    const int32_t *off;          // [S + 2] (the filter's offsets)
    const int32_t *count, *labels, *n_clusters, *had, *filt_src;
    const float *m;              // [S][8] rows 0 and 1 of the inverse box transform, float32
    const double *new_box;
    int n_segments, n_rows, n_parts, cluster_min_points, min_rows;
    int parts[CP_MAX_PARTS];
    double discard_max_height;
    int32_t *csize;              // [n_rows] per cluster slot (segment start + label)
    uint32_t *czmax;             // [n_rows]
    int32_t *occ, *best_label, *best_count, *out_off;
    float *out_xyz;
    int32_t *out_src;
};

__global__ void __launch_bounds__(CP_THREADS) cp_cluster_stats_kernel(ScoreArgs a) {
    const int i = blockIdx.x * CP_THREADS + threadIdx.x;
    if (i >= a.n_rows) return;
    const int s = segment_of(a.off, a.n_segments + 1, i);
    if (s >= a.n_segments || i - a.off[s] >= a.count[s]) return;
    const int l = a.labels[i];
    if (l < 0 || l >= a.n_clusters[s] || a.off[s] + l >= a.off[s + 1]) return;
    atomicAdd(a.csize + a.off[s] + l, 1);
    atomicMax(a.czmax + a.off[s] + l, float_key(a.xyz[3 * (size_t)i + 2]));
}

// one workgroup per segment: the first valid cluster of strictly greatest size, then the cell counts of its rows
__global__ void __launch_bounds__(CP_THREADS) cp_best_occ_kernel(ScoreArgs a) {
    __shared__ unsigned long long s_best;
    __shared__ int cells[CP_MAX_PART * CP_MAX_PART];
    __shared__ int s_occ;
    const int s = blockIdx.x;
    const int o0 = a.off[s], n = a.count[s];
    if (threadIdx.x == 0) s_best = 0ull;
    __syncthreads();
    if (a.had[s] && n > a.min_rows) {
        const int nc = min(a.n_clusters[s], a.off[s + 1] - o0);
        unsigned long long best = 0ull;
        for (int l = threadIdx.x; l < nc; l += CP_THREADS) {
            const int sz = a.csize[o0 + l];
            if (sz > a.cluster_min_points && (double)float_unkey(a.czmax[o0 + l]) < a.discard_max_height) {
                // greatest size first, lowest label among equals
                const unsigned long long k = ((unsigned long long)(uint32_t)sz << 32) | (0xffffffffu - (uint32_t)l);
                best = best > k ? best : k;
            }
        }
        if (best) atomicMax(&s_best, best);
    }
    __syncthreads();
    const unsigned long long best = s_best;
    const int label = best ? (int)(0xffffffffu - (uint32_t)(best & 0xffffffffu)) : -1;
    const int size = (int)(best >> 32);
    if (threadIdx.x == 0) a.best_label[s] = label, a.best_count[s] = size;
    const double *nb = a.new_box + (size_t)s * 7;
    const double bl = nb[3], bw = nb[4];
    const float *mf = a.m + (size_t)s * 8;
    const double m00 = mf[0], m01 = mf[1], m02 = mf[2], m03 = mf[3], m10 = mf[4], m11 = mf[5], m12 = mf[6], m13 = mf[7];
    for (int p = 0; p < a.n_parts; ++p) {
        const int parts = a.parts[p];
        for (int c = threadIdx.x; c < CP_MAX_PART * CP_MAX_PART; c += CP_THREADS) cells[c] = 0;
        if (threadIdx.x == 0) s_occ = 0;
        __syncthreads();
        if (label >= 0) {
            const double dl = bl / parts, dw = bw / parts;
            for (int i = threadIdx.x; i < n; i += CP_THREADS) {
                if (a.labels[o0 + i] != label) continue;
                const double x = a.xyz[3 * (size_t)(o0 + i)], y = a.xyz[3 * (size_t)(o0 + i) + 1], z = a.xyz[3 * (size_t)(o0 + i) + 2];
                const double X = ((x * m00 + y * m01) + z * m02) + m03;
                const double Y = ((x * m10 + y * m11) + z * m12) + m13;
                int ci = -1, cj = -1;
                for (int k = 0; k < parts; ++k) {   // the reference's bounds, evaluated as it writes them
                    if (-bl / 2 + k * dl <= X && X < -bl / 2 + (k + 1) * dl) ci = k;
                    if (-bw / 2 + k * dw <= Y && Y < -bw / 2 + (k + 1) * dw) cj = k;
                }
                if (ci >= 0 && cj >= 0) atomicAdd(&cells[ci * CP_MAX_PART + cj], 1);
            }
        }
        __syncthreads();
        int c = 0;
        for (int k = threadIdx.x; k < CP_MAX_PART * CP_MAX_PART; k += CP_THREADS) c += cells[k] > 1 ? 1 : 0;
        if (c) atomicAdd(&s_occ, c);
        __syncthreads();
        if (threadIdx.x == 0) a.occ[(size_t)s * a.n_parts + p] = s_occ;
        __syncthreads();
    }
}

__global__ void __launch_bounds__(CP_THREADS) cp_best_fill_kernel(ScoreArgs a) {
    __shared__ int sm4[4];
    const int s = blockIdx.x;
    const int o0 = a.off[s], label = a.best_label[s];
    const int n = label >= 0 ? a.count[s] : 0;
    const int f0 = a.out_off[s], room = min(a.out_off[s + 1], a.n_rows) - f0;
    const int32_t *labels = a.labels;
    cp_compact(n, sm4, false, [=](int i) { return labels[o0 + i] == label; }, [&](int i, int pos) {
        if (pos >= room) return;
        for (int k = 0; k < 3; ++k) a.out_xyz[3 * (size_t)(f0 + pos) + k] = a.xyz[3 * (size_t)(o0 + i) + k];
        const int r = a.ng_src[o0 + i];
        a.out_src[f0 + pos] = (r >= 0 && o0 + r < a.off[s + 1]) ? a.filt_src[o0 + r] : -1;
    });
}

// per_seg: one word per segment that the size query has always counted; no kernel touches it. The launcher clears the two
// per-row pieces in front of it, [0, per_seg).
struct ScoreLayout {
    size_t csize, czmax, per_seg, total;
};
ScoreLayout score_layout(int n_segments, long long n_rows) {
    ScoreLayout L;
    Carve c;
    L.csize = c.take((size_t)n_rows * 4);
    L.czmax = c.take((size_t)n_rows * 4);
    L.per_seg = c.take((size_t)n_segments * 4);
    L.total = c.o;
    return L;
}

int crop_args(CropArgs &a, const void *points, int is_half, int row_stride, const int32_t *frame_off, int n_frames,
              const double *boxes, const int32_t *seg_frame, int n_segments) {
    if (n_segments < 0 || n_segments > CP_MAX_SEGMENTS || n_frames <= 0 || row_stride < 3 || (is_half != 0 && is_half != 1))
        return CPD_ERR_ARG;
    if (!frame_off || (n_segments > 0 && (!points || !boxes || !seg_frame))) return CPD_ERR_ARG;
    a.points = points, a.is_half = is_half, a.stride = row_stride, a.n_frames = n_frames, a.n_segments = n_segments;
    a.frame_off = frame_off, a.seg_frame = seg_frame, a.boxes = boxes;
    a.row_cap = 0, a.counts = nullptr, a.seg_off = nullptr, a.out_rows = nullptr, a.out_src = nullptr;
    return CPD_OK;
}

}  // namespace

extern "C" {

size_t cpd_cproto_crop_workspace_bytes(int n_segments) {
    if (n_segments < 0) return 0;
    return cpd_align((size_t)(n_segments > 0 ? n_segments : 1) * 4);
}

int cpd_cproto_crop_count(const void *points, int is_half, int row_stride, const int32_t *frame_off, int n_frames,
                          const double *boxes, const int32_t *seg_frame, int n_segments, int32_t *seg_off, void *workspace,
                          size_t workspace_bytes, cpd_stream_t stream) {
    CropArgs a;
    const int rc = crop_args(a, points, is_half, row_stride, frame_off, n_frames, boxes, seg_frame, n_segments);
    if (rc != CPD_OK) return rc;
    if (!seg_off) return CPD_ERR_ARG;
    if (!workspace || workspace_bytes < cpd_cproto_crop_workspace_bytes(n_segments)) return CPD_ERR_WORKSPACE;
    hipStream_t st = cpd_s(stream);
    a.counts = static_cast<int32_t *>(workspace);
    if (n_segments > 0) cp_crop_count_kernel<<<n_segments, CP_THREADS, 0, st>>>(a);
    cp_offsets_kernel<<<1, 1024, 0, st>>>(a.counts, n_segments, seg_off, -1);
    return cpd_check_launch();
}

int cpd_cproto_crop_fill(const void *points, int is_half, int row_stride, const int32_t *frame_off, int n_frames,
                         const double *boxes, const int32_t *seg_frame, int n_segments, const int32_t *seg_off, int n_rows,
                         void *out_rows, int32_t *out_src, cpd_stream_t stream) {
    CropArgs a;
    const int rc = crop_args(a, points, is_half, row_stride, frame_off, n_frames, boxes, seg_frame, n_segments);
    if (rc != CPD_OK) return rc;
    if (!seg_off || n_rows < 0 || (n_rows > 0 && (!out_rows || !out_src))) return CPD_ERR_ARG;
    if (n_segments == 0 || n_rows == 0) return CPD_OK;
    a.seg_off = seg_off, a.row_cap = n_rows, a.out_rows = out_rows, a.out_src = out_src;
    cp_crop_fill_kernel<<<n_segments, CP_THREADS, 0, cpd_s(stream)>>>(a);
    return cpd_check_launch();
}

size_t cpd_cproto_filter_workspace_bytes(int n_segments, int n_rows) {
    if (n_segments < 0 || n_rows < 0) return 0;
    return filter_layout(n_segments > 0 ? n_segments : 1).total;
}

int cpd_cproto_filter(const void *rows, int is_half, const int32_t *seg_off, const int32_t *crop_src, const double *boxes,
                      int n_segments, int n_rows, double radius, uint8_t *dens_mask, double *z_min, double *new_box,
                      int32_t *had_points, void *filt_rows, int32_t *filt_src, int32_t *filt_off, void *workspace,
                      size_t workspace_bytes, cpd_stream_t stream) {
    if (n_segments < 0 || n_segments > CP_MAX_SEGMENTS || n_rows < 0 || (is_half != 0 && is_half != 1) || !(radius > 0.0))
        return CPD_ERR_ARG;
    if (!seg_off || !filt_off) return CPD_ERR_ARG;
    if (n_segments > 0 && (!boxes || !z_min || !new_box || !had_points)) return CPD_ERR_ARG;
    if (n_rows > 0 && (!rows || !crop_src || !dens_mask || !filt_rows || !filt_src)) return CPD_ERR_ARG;
    const FilterLayout L = filter_layout(n_segments > 0 ? n_segments : 1);
    if (!workspace || workspace_bytes < L.total) return CPD_ERR_WORKSPACE;
    hipStream_t st = cpd_s(stream);
    FilterArgs a;
    a.rows = rows, a.is_half = is_half, a.n_segments = n_segments, a.n_rows = n_rows, a.seg_off = seg_off;
    a.crop_src = crop_src, a.boxes = boxes, a.rad2 = radius * radius, a.mask = dens_mask, a.z_min = z_min;
    a.new_box = new_box, a.had = had_points, a.thr = ws_at<float>(workspace, L.thr), a.counts = ws_at<int32_t>(workspace, L.counts);
    a.filt_off = filt_off, a.filt_rows = filt_rows, a.filt_src = filt_src;
    if (n_segments > 0 && n_rows > 0) cp_density_kernel<<<cpd_div_up(n_rows, CP_THREADS), CP_THREADS, 0, st>>>(a);
    if (n_segments > 0) cp_zmin_kernel<<<n_segments, CP_THREADS, 0, st>>>(a);
    cp_offsets_kernel<<<1, 1024, 0, st>>>(a.counts, n_segments, filt_off, n_rows);
    cp_window_fill_kernel<<<n_segments + 1, CP_THREADS, 0, st>>>(a);
    return cpd_check_launch();
}

size_t cpd_cproto_score_workspace_bytes(int n_segments, int n_rows) {
    if (n_segments < 0 || n_rows < 0) return 0;
    return score_layout(n_segments > 0 ? n_segments : 1, n_rows > 0 ? n_rows : 1).total;
}

int cpd_cproto_score(const float *ng_xyz, const int32_t *ng_src, const int32_t *filt_off, const int32_t *ng_count,
                     const int32_t *labels, const int32_t *n_clusters, const int32_t *had_points, const int32_t *filt_src,
                     const float *m, const double *new_box, int n_segments, int n_rows, const int32_t *parts, int n_parts,
                     int min_rows, int cluster_min_points, double discard_max_height, int32_t *occ, int32_t *best_label,
                     int32_t *best_count, int32_t *out_off, float *out_xyz, int32_t *out_src, void *workspace,
                     size_t workspace_bytes, cpd_stream_t stream) {
    if (n_segments < 0 || n_segments > CP_MAX_SEGMENTS || n_rows < 0 || !parts || !out_off) return CPD_ERR_ARG;
    if (n_parts < 1 || n_parts > CP_MAX_PARTS) return CPD_ERR_UNSUPPORTED;
    for (int p = 0; p < n_parts; ++p)
        if (parts[p] < 1 || parts[p] > CP_MAX_PART) return CPD_ERR_UNSUPPORTED;
    if (n_segments > 0 && (!filt_off || !ng_count || !n_clusters || !had_points || !m || !new_box || !occ || !best_label ||
                           !best_count))
        return CPD_ERR_ARG;
    if (n_rows > 0 && (!ng_xyz || !ng_src || !labels || !filt_src || !out_xyz || !out_src)) return CPD_ERR_ARG;
    const ScoreLayout L = score_layout(n_segments > 0 ? n_segments : 1, n_rows > 0 ? n_rows : 1);
    if (!workspace || workspace_bytes < L.total) return CPD_ERR_WORKSPACE;
    hipStream_t st = cpd_s(stream);
    ScoreArgs a;
    a.xyz = ng_xyz, a.ng_src = ng_src, a.off = filt_off, a.count = ng_count, a.labels = labels, a.n_clusters = n_clusters;
    a.had = had_points, a.filt_src = filt_src, a.m = m, a.new_box = new_box, a.n_segments = n_segments, a.n_rows = n_rows;
    a.n_parts = n_parts, a.min_rows = min_rows, a.cluster_min_points = cluster_min_points, a.discard_max_height = discard_max_height;
    for (int p = 0; p < CP_MAX_PARTS; ++p) a.parts[p] = p < n_parts ? parts[p] : 1;
    a.csize = ws_at<int32_t>(workspace, L.csize), a.czmax = ws_at<uint32_t>(workspace, L.czmax);
    a.occ = occ, a.best_label = best_label, a.best_count = best_count, a.out_off = out_off, a.out_xyz = out_xyz;
    a.out_src = out_src;
    CPD_HIP_TRY(hipMemsetAsync(workspace, 0, L.per_seg, st));   // sizes 0, max z keys below every float
    if (n_segments > 0 && n_rows > 0) cp_cluster_stats_kernel<<<cpd_div_up(n_rows, CP_THREADS), CP_THREADS, 0, st>>>(a);
    if (n_segments > 0) cp_best_occ_kernel<<<n_segments, CP_THREADS, 0, st>>>(a);
    cp_offsets_kernel<<<1, 1024, 0, st>>>(best_count, n_segments, out_off, -1);
    if (n_segments > 0 && n_rows > 0) cp_best_fill_kernel<<<n_segments, CP_THREADS, 0, st>>>(a);
    return cpd_check_launch();
}

}  // extern "C"
