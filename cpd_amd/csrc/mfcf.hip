// mfcf.hip -- the per-frame half of CPD's MFCF pseudo-label generator (cpd/unsupervised_core/mfcf.py:46-80) for a chunk of
// current frames; ground removal, DBSCAN and box_fit between steps 2 and 3 are outline.hip's:
//   1. cpd_mfcf_gather : every sweep of a frame's window goes sweep -> world -> current frame (rigid_f64.h, the products of
//      ppscore.hip) and the rows with PP score H > thresh are kept in loop order, then the current sweep's own rows as they are
//      (mfcf.py:53-72): one ordered scan per current frame over (window rows, current rows);
//   2. cpd_mfcf_voxel_sample : voxel_sampling (outline_utils.py:368-389): per frame the minima, per row the cell
//      (x - min) // 0.1 with numpy's float32 floor_divide, a hash table per frame with the first and the last row of every
//      cell (integer atomicMin / atomicMax), then one scan over the rows that are the first of their cell: the cell's output
//      row is point[last], at the rank of first -- a dict's insertion order with overwritten values;
//   3. cpd_mfcf_fit_dgd : box_fit_DGD's tail (l.881-883) on cpd_outline_boxes' boxes: density_guided_drift, then
//      correct_orientation, then correct_heading (l.444-485), each on the inverse transform of the box the step before left;
//      one workgroup per box over the rows of its frame that carry its cluster's label and lie above min z + 0.2. The drift
//      and orientation passes are refine_dev.h's (shared with cproto_refine.hip).
// Every reduction is an integer or a min / max: the same bits on every launch.
// Built with -ffp-contract=off: the cell quotient and the bin / slab bounds are numpy's expressions op by op; the only fused
// multiply-adds are the explicit ones of the pose product.
#include <math.h>

#include "common.h"
#include "refine_dev.h"
#include "rigid_f64.h"

namespace {

constexpr int MF_MAX_WINDOW = 16;
constexpr int MF_HEAD_PARTS = 10;       // correct_heading's parts
constexpr unsigned long long MF_EMPTY = ~0ull;
constexpr int MF_CELL_BITS = 21;        // per axis: 2^21 cells of 0.1 m

// ---- 1. gather (mfcf.py:53-72) -------------------------------------------------------------------------------------------

struct GatherKeep {                      // what the keep test reads
    const uint16_t *h[MF_MAX_WINDOW];    // float16 bits, one array per window sweep
    int32_t off[MF_MAX_WINDOW + 2];      // row offsets of the window sweeps, then of the current sweep's raw rows
    int n_win;
    float thresh;                        // the threshold as numpy rounds it against a float16 array
};
struct GatherRows {
    const void *pts[MF_MAX_WINDOW + 1];  // the window sweeps, then the current sweep
    int32_t stride[MF_MAX_WINDOW + 1], half[MF_MAX_WINDOW + 1];
    double pose[MF_MAX_WINDOW][12];
    double cur_inv[12];
    float *out;                          // the frame's slice
};

__device__ __forceinline__ int mf_segment(const GatherKeep &k, int i) {
    int t = 0;
    while (t < k.n_win && i >= k.off[t + 1]) ++t;
    return t;
}
// numpy's all_H > thresh on float16: both sides are float16 values, compared exactly as floats; NaN is not greater
__device__ __forceinline__ bool mf_keep(const GatherKeep &k, int i) {
    const int t = mf_segment(k, i);
    if (t == k.n_win) return true;       // the current sweep's own rows
    const uint16_t bits = k.h[t][i - k.off[t]];
    _Float16 hf;
    __builtin_memcpy(&hf, &bits, 2);
    return (float)hf > k.thresh;
}

// ---- 2. voxel_sampling (outline_utils.py:368-389) -----------------------------------------------------------------------

struct VoxelArgs {
    const float *pts;            // [n_points][3]
    const int32_t *off, *count;  // [n_frames + 1], [n_frames]: frame f = rows off[f] .. off[f] + count[f]
    int n_frames, n_points;
    uint32_t *fmin;              // [n_frames][3] order-preserving keys of the minima
    unsigned long long *keys;    // [2 * n_points] frame f's table is slots 2 * off[f] .. 2 * off[f + 1]
    int32_t *first, *last;       // [2 * n_points]
    int32_t *slot;               // [n_points]
    int32_t *err;
    float *out;                  // [n_points][3]
    int32_t *out_src;            // [n_points] the row within its frame (may be null)
    int32_t *out_off;            // [n_frames + 2]
};

// the frame whose slice holds row i (the last frame that starts at or before it), -1 past its count
__device__ __forceinline__ int mf_frame_of(const VoxelArgs &a, int i) {
    int f = 0;
    while (f + 1 < a.n_frames && i >= a.off[f + 1]) ++f;
    return (i >= a.off[f] && i - a.off[f] < a.count[f] && i < a.off[f + 1]) ? f : -1;
}

__global__ void __launch_bounds__(256) vs_min_kernel(VoxelArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int f = i < a.n_points ? mf_frame_of(a, i) : -1;
    uint32_t k[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu};
    if (f >= 0)
        for (int d = 0; d < 3; ++d) k[d] = float_key(a.pts[3 * (size_t)i + d]);
    // a wave of one frame reduces first (the common case); a wave that straddles frames sends every lane's keys
    const int f0 = __shfl(f, 0, 64);
    if (__all(f == f0 || f < 0)) {
        for (int s = 32; s; s >>= 1)
            for (int d = 0; d < 3; ++d) k[d] = min(k[d], (uint32_t)__shfl_xor((int)k[d], s, 64));
        if ((threadIdx.x & 63) == 0 && f0 >= 0)
            for (int d = 0; d < 3; ++d) atomicMin(a.fmin + 3 * f0 + d, k[d]);
    } else if (f >= 0) {
        for (int d = 0; d < 3; ++d) atomicMin(a.fmin + 3 * f + d, k[d]);
    }
}

// numpy's float32 floor_divide (npy_divmodf) for a >= 0, b > 0: the quotient of the fmod-reduced numerator, floored, with
// the half-ulp correction
__device__ __forceinline__ float mf_floor_divide(float a, float b) {
    const float mod = fmodf(a, b);
    const float div = __fdiv_rn(__fsub_rn(a, mod), b);
    if (div == 0.0f) return 0.0f;
    float fl = floorf(div);
    if (__fsub_rn(div, fl) > 0.5f) fl = __fadd_rn(fl, 1.0f);
    return fl;
}

__global__ void __launch_bounds__(256) vs_insert_kernel(VoxelArgs a, float res) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n_points) return;
    a.slot[i] = -1;
    const int f = mf_frame_of(a, i);
    if (f < 0) return;
    if (a.off[f + 1] > a.n_points) {            // a slice that runs past the buffer: its table would too
        atomicOr(a.err, 2);
        return;
    }
    unsigned long long key = 0;
    for (int d = 0; d < 3; ++d) {
        const float c = mf_floor_divide(__fsub_rn(a.pts[3 * (size_t)i + d], float_unkey(a.fmin[3 * f + d])), res);
        if (!(c >= 0.0f && c < (float)(1 << MF_CELL_BITS))) {   // NaN, or a cloud wider than the key
            atomicOr(a.err, 1);
            return;
        }
        key = (key << MF_CELL_BITS) | (unsigned long long)c;
    }
    const unsigned long long base = 2ull * (unsigned long long)a.off[f];
    const unsigned long long size = 2ull * (unsigned long long)(a.off[f + 1] - a.off[f]);   // >= 2 slots per row: never full
    unsigned long long s = mix64(key) % size;
    for (;;) {
        const unsigned long long prev = atomicCAS(a.keys + base + s, MF_EMPTY, key);
        if (prev == MF_EMPTY || prev == key) break;
        s = s + 1 == size ? 0 : s + 1;
    }
    const int g = (int)(base + s);
    a.slot[i] = g;
    atomicMin(a.first + g, i);
    atomicMax(a.last + g, i);
}

__global__ void __launch_bounds__(256) vs_tail_kernel(VoxelArgs a) {   // frames that start at the end of the buffer, the padding frame
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f < a.n_frames && a.off[f] >= a.n_points) a.out_off[f] = a.out_off[a.n_frames];
    if (f == a.n_frames) a.out_off[a.n_frames + 1] = a.n_points;
}

struct VoxelLayout {
    size_t fmin, keys, first, last, slot, scan, total;
};
VoxelLayout vs_layout(int n_frames, long long n_points) {
    VoxelLayout L;
    Carve c;
    L.fmin = c.take((size_t)n_frames * 12);
    L.keys = c.take((size_t)n_points * 16);
    L.last = c.take((size_t)n_points * 8);
    L.first = c.take((size_t)n_points * 8);
    L.slot = c.take((size_t)n_points * 4);
    L.scan = c.take((size_t)scan_num_blocks(n_points) * 4);
    L.total = c.o;
    return L;
}

// ---- 3. box_fit_DGD's tail (outline_utils.py:881-883, 444-485) -----------------------------------------------------------

// the rows of a frame with one DBSCAN label above the height cut, as a refine_dev.h cluster
struct LabelCluster {
    const float *xyz;
    const int32_t *labels;
    int n, count, label;
    double cut;
    __device__ __forceinline__ bool row(int i, double &x, double &y, double &z) const {
        if (labels[i] != label) return false;
        z = xyz[3 * (size_t)i + 2];
        if (!(z > cut)) return false;
        x = xyz[3 * (size_t)i], y = xyz[3 * (size_t)i + 1];
        return true;
    }
};

struct DgdArgs {
    const float *xyz;
    const int32_t *off, *count, *labels;
    const double *boxes;         // cpd_outline_boxes' out: [n_frames] counts, then [box_cap][8]
    int n_frames, n_points, box_cap, steps;
    double *out;                 // [box_cap][7]
    int32_t *bits;               // [box_cap]
    int32_t *n_out;              // [1]
};

__global__ void __launch_bounds__(RF_THREADS) mf_dgd_kernel(DgdArgs a) {
    __shared__ double smd[16];
    __shared__ int smi[8];
    __shared__ unsigned long long bkey[2 * RF_PARTS];
    __shared__ int brow[2 * RF_PARTS];
    __shared__ unsigned long long slab[MF_HEAD_PARTS];
    __shared__ double sbox[7];
    __shared__ uint32_t szmin;
    __shared__ int scount;
    // the frame of box blockIdx.x: the boxes lie frame by frame, counts first
    int f = -1, total = 0;
    for (int g = 0; g < a.n_frames; ++g) {
        const int c = (int)a.boxes[g];
        if (f < 0 && (int)blockIdx.x < total + c) f = g;
        total += c;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) *a.n_out = total < a.box_cap ? total : a.box_cap;
    if (f < 0) return;
    const double *b0 = a.boxes + a.n_frames + (size_t)blockIdx.x * 8;
    double *out = a.out + (size_t)blockIdx.x * 7;
    const int o0 = min(max(a.off[f], 0), a.n_points);
    LabelCluster c;
    c.xyz = a.xyz + 3 * (size_t)o0, c.labels = a.labels + o0;
    c.n = min(max(a.count[f], 0), a.n_points - o0), c.label = (int)b0[7], c.count = 0, c.cut = -INFINITY;
    // pass 0: the cluster's least z (box_fit's filter is z > min z + 0.2), then the rows above it
    if (threadIdx.x == 0) szmin = 0xffffffffu, scount = 0;
    __syncthreads();
    uint32_t zk = 0xffffffffu;
    for (int i = threadIdx.x; i < c.n; i += RF_THREADS)
        if (c.labels[i] == c.label) zk = min(zk, float_key(c.xyz[3 * (size_t)i + 2]));
    for (int s = 32; s; s >>= 1) zk = min(zk, (uint32_t)__shfl_xor((int)zk, s, 64));
    if ((threadIdx.x & 63) == 0) atomicMin(&szmin, zk);
    __syncthreads();
    c.cut = szmin == 0xffffffffu ? INFINITY : (a.steps & 8) ? -INFINITY : (double)float_unkey(szmin) + 0.2;
    int cnt = 0;
    for (int i = threadIdx.x; i < c.n; i += RF_THREADS) {
        double x, y, z;
        cnt += c.row(i, x, y, z) ? 1 : 0;
    }
    for (int s = 32; s; s >>= 1) cnt += __shfl_xor(cnt, s, 64);
    if ((threadIdx.x & 63) == 0) atomicAdd(&scount, cnt);
    __syncthreads();
    c.count = scount;
    if (c.count == 0) {                      // not expected: a box comes from at least three rows
        if (threadIdx.x < 7) out[threadIdx.x] = b0[threadIdx.x];
        if (threadIdx.x == 0) a.bits[blockIdx.x] = 0;
        return;
    }
    double b[7], m[8];
    float mf[8];
    int bits = 0;
    for (int k = 0; k < 7; ++k) b[k] = b0[k];
    if (a.steps & 1) {                       // density_guided_drift
        rf_inverse_rows(b[0], b[1], b[6], mf);
        for (int k = 0; k < 8; ++k) m[k] = mf[k];
        const Stats t = rf_stats(c, m, smd, smi);
        if (threadIdx.x == 0) {
            rf_drift_box(b, t, c.count, sbox);
            bits |= (2 * (long long)t.pos_x > c.count ? 1 : 0) | (2 * (long long)t.pos_y > c.count ? 2 : 0);
        }
        __syncthreads();
        for (int k = 0; k < 7; ++k) b[k] = sbox[k];
        __syncthreads();
    }
    if (a.steps & 2) {                       // correct_orientation
        rf_inverse_rows(b[0], b[1], b[6], mf);
        for (int k = 0; k < 8; ++k) m[k] = mf[k];
        const Stats t = rf_stats(c, m, smd, smi);
        const Orient o = rf_orient(c, b, m, t, bkey, brow);
        if (threadIdx.x == 0) {
            sbox[6] = o.yaw;
            bits |= (o.by_x ? 4 : 0) | (o.take_max ? 8 : 0) | (o.turned ? 16 : 0);
        }
        __syncthreads();
        b[6] = sbox[6];
        __syncthreads();
    }
    if (!(a.steps & 4)) {
        if (threadIdx.x == 0) {
            for (int k = 0; k < 7; ++k) out[k] = b[k];
            a.bits[blockIdx.x] = bits;
        }
        return;
    }
    if (threadIdx.x < MF_HEAD_PARTS) slab[threadIdx.x] = 0ull;
    __syncthreads();
    // correct_heading: per slab of X the greatest box-frame z, Z = ((x*0 + y*0) + z*1) + (-z_box) with z_box in float32
    rf_inverse_rows(b[0], b[1], b[6], mf);
    for (int k = 0; k < 8; ++k) m[k] = mf[k];
    const double l = b[3], delta_l = l / MF_HEAD_PARTS, mz = -(double)(float)b[2];
    for (int i = threadIdx.x; i < c.n; i += RF_THREADS) {
        double x, y, z;
        if (!c.row(i, x, y, z)) continue;
        const double X = ((x * m[0] + y * m[1]) + z * m[2]) + m[3];
        const double Z = ((x * 0.0 + y * 0.0) + z * 1.0) + mz;
        for (int p = 0; p < MF_HEAD_PARTS; ++p)
            if (-l / 2 + p * delta_l <= X && X < -l / 2 + (p + 1) * delta_l) atomicMax(&slab[p], rf_dkey(Z));
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    double sum_min = 0.0, sum_max = 0.0;
    int n_min = 0, n_max = 0;
    for (int p = 0; p < MF_HEAD_PARTS; ++p) {
        if (slab[p] == 0ull) continue;
        const unsigned long long k = slab[p];
        const double zmax = __longlong_as_double((long long)((k & 0x8000000000000000ull) ? (k & 0x7fffffffffffffffull) : ~k));
        if (-l / 2 + p * delta_l < 0) sum_min += zmax, ++n_min;
        if (-l / 2 + (p + 1) * delta_l > 0) sum_max += zmax, ++n_max;
    }
    const double mean_min = n_min ? sum_min / n_min : 0.0, mean_max = n_max ? sum_max / n_max : 0.0;
    if (mean_min < mean_max) b[6] += M_PI, bits |= 32;
    for (int k = 0; k < 7; ++k) out[k] = b[k];
    a.bits[blockIdx.x] = bits;
}

}  // namespace

extern "C" {

size_t cpd_mfcf_gather_workspace_bytes(int max_rows) {
    if (max_rows < 0) return 0;
    return cpd_align((size_t)scan_num_blocks(max_rows) * 4);
}

int cpd_mfcf_gather(const void *const *sweep_pts, const void *const *sweep_h, const int32_t *sweep_rows,
                    const int32_t *sweep_stride, const int32_t *sweep_dtype, const double *sweep_pose, int n_sweeps,
                    const int32_t *win_sweep, const int32_t *win_count, const int32_t *cur_sweep, const double *cur_pose_inv,
                    const int32_t *out_off, int n_frames, float thresh, float *out, int32_t *out_count, void *workspace,
                    size_t workspace_bytes, cpd_stream_t stream) {
    if (n_sweeps < 0 || n_frames < 0) return CPD_ERR_ARG;
    if (n_frames == 0) return CPD_OK;
    if (!sweep_pts || !sweep_h || !sweep_rows || !sweep_stride || !sweep_dtype || !sweep_pose || !win_sweep || !win_count ||
        !cur_sweep || !cur_pose_inv || !out_off || !out || !out_count || out_off[0] != 0)
        return CPD_ERR_ARG;
    for (int s = 0; s < n_sweeps; ++s)
        if (sweep_rows[s] < 0 || sweep_stride[s] < 3 || (sweep_dtype[s] != 0 && sweep_dtype[s] != 1) ||
            (sweep_rows[s] > 0 && (!sweep_pts[s] || !sweep_h[s])))
            return CPD_ERR_ARG;
    long long max_rows = 0;
    for (int f = 0; f < n_frames; ++f) {
        if (win_count[f] > MF_MAX_WINDOW) return CPD_ERR_UNSUPPORTED;
        if (win_count[f] < 0 || cur_sweep[f] < 0 || cur_sweep[f] >= n_sweeps) return CPD_ERR_ARG;
        long long rows = sweep_rows[cur_sweep[f]];
        for (int w = 0; w < win_count[f]; ++w) {
            const int s = win_sweep[f * MF_MAX_WINDOW + w];
            if (s < 0 || s >= n_sweeps) return CPD_ERR_ARG;
            rows += sweep_rows[s];
        }
        if (rows > 0x7fffffff || (long long)out_off[f + 1] - out_off[f] < rows) return CPD_ERR_ARG;
        max_rows = rows > max_rows ? rows : max_rows;
    }
    if (!workspace || workspace_bytes < cpd_mfcf_gather_workspace_bytes((int)max_rows)) return CPD_ERR_WORKSPACE;
    hipStream_t st = cpd_s(stream);
    for (int f = 0; f < n_frames; ++f) {
        GatherKeep k;
        GatherRows r;
        k.n_win = win_count[f], k.thresh = thresh, k.off[0] = 0;
        // segments 0 .. n_win - 1: the window's sweeps in loop order; segment n_win: the current sweep's raw rows
        for (int w = 0; w <= MF_MAX_WINDOW; ++w) {
            const bool used = w <= k.n_win;
            const int s = w < k.n_win ? win_sweep[f * MF_MAX_WINDOW + w] : cur_sweep[f];
            r.pts[w] = used ? sweep_pts[s] : nullptr, r.stride[w] = used ? sweep_stride[s] : 3, r.half[w] = used ? sweep_dtype[s] : 0;
            k.off[w + 1] = k.off[w] + (used ? sweep_rows[s] : 0);
            if (w == MF_MAX_WINDOW) break;
            k.h[w] = w < k.n_win ? static_cast<const uint16_t *>(sweep_h[s]) : nullptr;
            for (int e = 0; e < 12; ++e) r.pose[w][e] = w < k.n_win ? sweep_pose[(size_t)s * 16 + e] : 0.0;
        }
        const int n_virt = k.off[k.n_win + 1];
        for (int e = 0; e < 12; ++e) r.cur_inv[e] = cur_pose_inv[(size_t)f * 16 + e];
        r.out = out + 3 * (size_t)out_off[f];
        if (n_virt == 0) {
            CPD_HIP_TRY(hipMemsetAsync(out_count + f, 0, 4, st));
            continue;
        }
        const int rc = device_scan(
            (long long)n_virt, [=] __device__(long long i) { return mf_keep(k, (int)i) ? 1u : 0u; },
            [=] __device__(long long i, uint32_t v, uint32_t pre) {
                if (!v) return;
                const int t = mf_segment(k, (int)i);
                float x, y, z;
                load_xyz(r.pts[t], r.half[t], r.stride[t], (int)i - k.off[t], x, y, z);
                if (t < k.n_win) {
                    float wx, wy, wz;
                    pp_rigid3(r.pose[t], x, y, z, wx, wy, wz);
                    pp_rigid3(r.cur_inv, wx, wy, wz, x, y, z);
                }
                float *o = r.out + 3 * (size_t)pre;
                o[0] = x, o[1] = y, o[2] = z;
            },
            static_cast<uint32_t *>(workspace), out_count + f, -1, st);
        if (rc != CPD_OK) return rc;
    }
    return cpd_check_launch();
}

size_t cpd_mfcf_voxel_sample_workspace_bytes(int n_frames, int n_points) {
    if (n_frames <= 0 || n_points < 0) return 0;
    return vs_layout(n_frames, n_points).total;
}

int cpd_mfcf_voxel_sample(const float *points, const int32_t *frame_off, const int32_t *frame_count, int n_frames, int n_points,
                          float res, float *out, int32_t *out_src, int32_t *out_off, int32_t *err, void *workspace,
                          size_t workspace_bytes, cpd_stream_t stream) {
    if (n_frames <= 0 || n_points < 0 || !frame_off || !frame_count || !out_off || !err || !(res > 0.0f)) return CPD_ERR_ARG;
    if (n_points > 0 && (!points || !out)) return CPD_ERR_ARG;
    const VoxelLayout L = vs_layout(n_frames, n_points);
    if (!workspace || workspace_bytes < L.total) return CPD_ERR_WORKSPACE;
    hipStream_t st = cpd_s(stream);
    VoxelArgs a;
    a.pts = points, a.off = frame_off, a.count = frame_count, a.n_frames = n_frames, a.n_points = n_points;
    a.fmin = ws_at<uint32_t>(workspace, L.fmin), a.keys = ws_at<unsigned long long>(workspace, L.keys);
    a.first = ws_at<int32_t>(workspace, L.first), a.last = ws_at<int32_t>(workspace, L.last), a.slot = ws_at<int32_t>(workspace, L.slot);
    a.err = err, a.out = out, a.out_src = out_src, a.out_off = out_off;
    // fmin keys and table keys start at all ones; keys and last are adjacent (last = -1: below every row), first = 0x7f7f7f7f
    CPD_HIP_TRY(hipMemsetAsync(a.fmin, 0xff, L.first, st));
    CPD_HIP_TRY(hipMemsetAsync(a.first, 0x7f, (size_t)n_points * 8, st));
    CPD_HIP_TRY(hipMemsetAsync(out_off, 0, ((size_t)n_frames + 2) * 4, st));
    if (n_points == 0) return cpd_check_launch();
    CPD_HIP_TRY(hipMemsetAsync(out, 0, (size_t)n_points * 12, st));
    const unsigned blocks = (unsigned)cpd_div_up(n_points, 256);
    vs_min_kernel<<<blocks, 256, 0, st>>>(a);
    vs_insert_kernel<<<blocks, 256, 0, st>>>(a, res);
    const VoxelArgs ac = a;
    const int rc = device_scan(
        (long long)n_points,
        [=] __device__(long long i) { return (ac.slot[i] >= 0 && ac.first[ac.slot[i]] == (int32_t)i) ? 1u : 0u; },
        [=] __device__(long long i, uint32_t v, uint32_t pre) {
            // the frames that start at row i (empty ones share their start with the next) begin at rank pre
            for (int f = 0; f < ac.n_frames; ++f)
                if (ac.off[f] == (int32_t)i) ac.out_off[f] = (int32_t)pre;
            if (!v) return;
            const int32_t src = ac.last[ac.slot[i]];
            const float *p = ac.pts + 3 * (size_t)src;
            float *o = ac.out + 3 * (size_t)pre;
            o[0] = p[0], o[1] = p[1], o[2] = p[2];
            if (ac.out_src) {
                int f = 0;
                while (f + 1 < ac.n_frames && src >= ac.off[f + 1]) ++f;
                ac.out_src[pre] = src - ac.off[f];
            }
        },
        ws_at<uint32_t>(workspace, L.scan), out_off + n_frames, -1, st);
    if (rc != CPD_OK) return rc;
    vs_tail_kernel<<<cpd_div_up(n_frames + 1, 256), 256, 0, st>>>(a);
    return cpd_check_launch();
}

int cpd_mfcf_fit_dgd(const float *xyz, const int32_t *frame_off, const int32_t *frame_count, int n_frames, int n_points,
                     const int32_t *labels, const double *boxes, int box_cap, int steps, double *out, int32_t *bits,
                     int32_t *n_out, cpd_stream_t stream) {
    if (n_frames <= 0 || n_points < 0 || box_cap < 0 || !frame_off || !frame_count || !boxes || !n_out) return CPD_ERR_ARG;
    if (steps < 0 || steps > 15) return CPD_ERR_ARG;
    if (box_cap > 0 && (!out || !bits)) return CPD_ERR_ARG;
    if (n_points > 0 && (!xyz || !labels)) return CPD_ERR_ARG;
    hipStream_t st = cpd_s(stream);
    CPD_HIP_TRY(hipMemsetAsync(n_out, 0, 4, st));
    if (box_cap == 0 || n_points == 0) return cpd_check_launch();
    DgdArgs a;
    a.xyz = xyz, a.off = frame_off, a.count = frame_count, a.labels = labels, a.boxes = boxes, a.n_frames = n_frames;
    a.n_points = n_points, a.box_cap = box_cap, a.steps = steps, a.out = out, a.bits = bits, a.n_out = n_out;
    mf_dgd_kernel<<<box_cap, RF_THREADS, 0, st>>>(a);
    return cpd_check_launch();
}

}  // extern "C"
