// outline.hip -- CPD's DBSCAN pseudo-label generator (cpd/unsupervised_core/outline_utils.py OutlineFitter, ground_removal.py
// Processor / Segmentation) for a batch of frames per launch sequence:
//   1. cpd_outline_ground : remove_ground -- projection in the input dtype, per-(frame, segment, bin) min z, one lane per
//      (frame, segment) for the serial line fit in float64, per-point labelling over the +-7 neighbouring segment positions,
//      distance bands, and a stable per-frame compaction into the canonical order (bands; high points in input order, then
//      low non-ground points by segment, input order within a segment);
//   2. cpd_outline_dbscan : sklearn DBSCAN(eps, min_samples) labels -- the hashed uniform grid of hash_grid.h with side eps,
//      neighbour counts (float64 d^2 <= eps^2), union-find over core-core pairs that hooks the larger root under the smaller
//      (the root of a component is its lowest index whatever the schedule), border label = lowest cluster among adjacent
//      cores, cluster number = rank of the root;
//   3. cpd_outline_boxes : clustering's filter + box_fit -- low-point cut, 2-D convex hull by gift wrapping (one wave per
//      cluster, exact float64 orientation tests), one lane per hull-edge angle for minimum_bounding_rectangle_distance's
//      score, the box and box_fit's adjustments and filter.
// Frames are CSR ranges of rows; integer atomics only (counts, min / max of order-preserving keys), so every call gives the
// same bits. Built with -ffp-contract=off: no fused multiply-add anywhere in this file.
#include <math.h>

#include "common.h"
#include "hash_grid.h"

namespace {

constexpr int OL_NBIN = 150;          // Processor(n_bins=150)
constexpr int OL_NSEG = 152;          // segment index range of the projection: 0..150 can occur (floor at 2 pi / step)
constexpr int OL_NCELL = OL_NSEG * OL_NBIN;
constexpr int OL_SEARCH = 7;          // largest k with k * 2 pi / 150 < line_search_angle 0.3
constexpr int OL_MAX_BANDS = 6;
constexpr int OL_NBUCKET = OL_MAX_BANDS * (OL_NSEG + 1);
constexpr int OL_ORDER_THREADS = 512;

// ---- 1. ground removal ------------------------------------------------------------------------------------------------

struct GroundArgs {
    const void *points;
    int is_half, stride, n_frames, n_points;
    const int32_t *off;
    float c_pi, c_seg_step, c_rmin, c_bin_step, c_high;   // the Python constants rounded to the input dtype (NEP 50)
    double sensor_height;
    int n_bands;
    double thr[OL_MAX_BANDS], dist[OL_MAX_BANDS + 1];
    int32_t *code;        // [n_points] -2 high, -1 dropped, else seg * OL_NBIN + bin
    uint32_t *minz;       // [n_frames][OL_NCELL] min z keys
    double2 *cover;       // [n_frames][OL_NCELL] (m, b) of the last line covering (seg, bin); m = NaN: none
    double2 *runs;        // [n_frames][OL_NCELL] per segment the (bin, min z) list
    int32_t *seg_pos;     // [n_frames][OL_NSEG] position in seg_list or -1
    int32_t *pos_seg;     // [n_frames][OL_NSEG]
    int32_t *n_pos;       // [n_frames]
    int32_t *bucket;      // [n_points]
    int32_t *bcount;      // [n_frames][OL_NBUCKET]
    int32_t *err;
    float *out_xyz;
    int32_t *out_src, *out_count;
};

// Processor.project_5D + filter_out_range (ground_removal.py:124-159); the high / low split of remove_ground (outline_utils.py:544-546)
__global__ void __launch_bounds__(256) ol_project_kernel(GroundArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n_points) return;
    float x, y, z;
    load_xyz(a.points, a.is_half, a.stride, i, x, y, z);
    if (z >= a.c_high) {   // ground_max_threshold
        a.code[i] = -2;
        return;
    }
    float q_seg, q_bin;
    if (a.is_half) {   // numpy float16 ufuncs: compute in float32, round to float16 after every op
        const float ang = round_half(atan2f(y, x));
        q_seg = round_half(round_half(ang + a.c_pi) / a.c_seg_step);
        const float r = round_half(sqrtf(round_half(round_half(x * x) + round_half(y * y))));
        q_bin = round_half(round_half(r - a.c_rmin) / a.c_bin_step);
    } else {
        q_seg = (atan2f(y, x) + a.c_pi) / a.c_seg_step;
        q_bin = (sqrtf(x * x + y * y) - a.c_rmin) / a.c_bin_step;
    }
    const float fb = floorf(q_bin), fs = floorf(q_seg);
    if (!(fb >= 1.0f && fb <= 149.0f)) {      // 0.3 < bin < 150 on the integer bin (NaN / overflow: dropped too)
        a.code[i] = -1;
        return;
    }
    if (!(fs >= 0.0f && fs < (float)OL_NSEG)) {
        a.code[i] = -1;
        atomicOr(a.err, 1);
        return;
    }
    const int seg = (int)fs, bin = (int)fb;
    a.code[i] = seg * OL_NBIN + bin;
    const int f = segment_of(a.off, a.n_frames, i);
    atomicMin(a.minz + (size_t)f * OL_NCELL + seg * OL_NBIN + bin, float_key(z));
}

// least squares z = m * bin + b over runs[r0..r1] by running sums in list order (tests/ref_outline.py fit_line)
struct OlSums {
    double sx, sy, sxx, sxy;
};
__device__ __forceinline__ void ol_add(OlSums &s, double2 p) {
    s.sx = s.sx + p.x;
    s.sy = s.sy + p.y;
    s.sxx = s.sxx + p.x * p.x;
    s.sxy = s.sxy + p.x * p.y;
}
__device__ __forceinline__ void ol_solve(const OlSums &s, int cnt, double &m, double &b) {
    const double n = (double)cnt;
    m = (n * s.sxy - s.sx * s.sy) / (n * s.sxx - s.sx * s.sx);
    b = (s.sy - m * s.sx) / n;
}
__device__ __forceinline__ OlSums ol_sums(const double2 *run, int r0, int r1) {
    OlSums s = {0.0, 0.0, 0.0, 0.0};
    for (int k = r0; k <= r1; ++k) ol_add(s, run[k]);
    return s;
}

// Segmentation.get_min_z + fitSegmentLines (ground_removal.py:180-242): one lane per (frame, segment); seg_list positions.
__global__ void __launch_bounds__(256) ol_fit_kernel(GroundArgs a) {
    __shared__ uint32_t sm[17];
    const int f = blockIdx.x, seg = threadIdx.x;
    const uint32_t *mz = a.minz + (size_t)f * OL_NCELL;
    double2 *run = a.runs + (size_t)f * OL_NCELL + (size_t)seg * OL_NBIN;
    double2 *cov = a.cover + (size_t)f * OL_NCELL + (size_t)seg * OL_NBIN;
    int n = 0;
    if (seg < OL_NSEG) {
        for (int b = 0; b < OL_NBIN; ++b) {
            cov[b] = make_double2(__longlong_as_double(0x7ff8000000000000ll), 0.0);
            const uint32_t k = mz[seg * OL_NBIN + b];
            if (k != 0xffffffffu) run[n++] = make_double2((double)b, (double)float_unkey(k));
        }
    }
    uint32_t tot;
    const uint32_t pos = block_excl_scan(n > 0 ? 1u : 0u, sm, &tot);
    if (seg < OL_NSEG) {
        a.seg_pos[f * OL_NSEG + seg] = n > 0 ? (int)pos : -1;
        if (n > 0) a.pos_seg[f * OL_NSEG + pos] = seg;
    }
    if (seg == 0) a.n_pos[f] = (int)tot;
    if (n == 0) return;
    // the reference's control flow; the current run is run[r0..r1] (always contiguous in the list)
    int r0 = 0, r1 = 0, i = 1;
    bool long_line = false;
    double ground = a.sensor_height;
    OlSums s = ol_sums(run, 0, 0);
    while (i < n) {
        const double2 cur = run[i], lst = run[r1];
        if (cur.x - lst.x > 8.0) long_line = true;                   // long_threshold
        if (r1 - r0 + 1 < 2) {
            if (cur.x - lst.x < 8.0 && fabs(lst.y - ground) < 0.5) { // max_start_height
                r1 = i;
                ol_add(s, cur);
            } else {
                r0 = r1 = i;
                s = ol_sums(run, i, i);
            }
        } else {
            OlSums s2 = s;
            ol_add(s2, cur);
            double m, b;
            ol_solve(s2, i - r0 + 1, m, b);
            double mse = 0.0;
            for (int k = r0; k <= i; ++k) {
                const double r = (m * run[k].x + b) - run[k].y;
                mse = fmax(mse, r * r);
            }
            if (mse > 0.1 || m > 2.0 || long_line) {                  // max_error, max_slope
                if (r1 - r0 + 1 >= 3) {
                    double m2, b2;
                    ol_solve(s, r1 - r0 + 1, m2, b2);
                    for (int k = (int)run[r0].x; k <= (int)run[r1].x; ++k) cov[k] = make_double2(m2, b2);
                    ground = m2 * run[r1].x + b2;
                }
                long_line = false;
                r0 = r1;
                s = ol_sums(run, r1, r1);
                --i;
            } else {
                r1 = i;
                s = s2;
            }
        }
        ++i;
    }
    if (r1 - r0 + 1 > 2) {
        double m, b;
        ol_solve(s, r1 - r0 + 1, m, b);
        for (int k = (int)run[r0].x; k <= (int)run[r1].x; ++k) cov[k] = make_double2(m, b);
    }
}

// Segment_Vel (ground_removal.py:85-116) + the distance bands of remove_ground (outline_utils.py:556-574): bucket per point
__global__ void __launch_bounds__(256) ol_label_kernel(GroundArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n_points) return;
    const int c = a.code[i];
    int bucket = -1;
    if (c != -1) {
        const int f = segment_of(a.off, a.n_frames, i);
        float x, y, z;
        load_xyz(a.points, a.is_half, a.stride, i, x, y, z);
        int cls = 0;
        bool keep = true;
        if (c >= 0) {
            const int seg = c / OL_NBIN, bin = c - seg * OL_NBIN;
            const int np_ = a.n_pos[f], p = a.seg_pos[f * OL_NSEG + seg];
            const double db = (double)bin, dz = (double)z;
            for (int o = -OL_SEARCH; o <= OL_SEARCH && keep; ++o) {
                const int q = ((p + o) % np_ + np_) % np_;
                const int s2 = a.pos_seg[f * OL_NSEG + q];
                const double2 mb = a.cover[(size_t)f * OL_NCELL + s2 * OL_NBIN + bin];
                if (mb.x == mb.x) {
                    const double d = fabs((mb.x * db + mb.y) - dz);
                    if (d > 0.0 && d <= 0.1) keep = false;             // a non-zero term: ground
                }
            }
            cls = 1 + seg;
        }
        if (keep) {
            const double X = x, Y = y, Z = z;
            const double d = sqrt((X * X + Y * Y) + Z * Z);
            const int k = a.n_bands;
            for (int band = 0; band < k; ++band) {
                bool in;
                if (band == 0) in = d < a.dist[1];
                else if (band == k - 1) in = d > a.dist[band];
                else in = d < a.dist[band + 1] && d > a.dist[band];
                if (in) {
                    if (Z > a.thr[band]) bucket = band * (OL_NSEG + 1) + cls;
                    break;
                }
            }
            if (bucket >= 0) atomicAdd(a.bcount + (size_t)f * OL_NBUCKET + bucket, 1);
        }
    }
    a.bucket[i] = bucket;
}

// stable counting sort of a frame's kept points by bucket, in index order: one workgroup per frame
__global__ void __launch_bounds__(OL_ORDER_THREADS) ol_order_kernel(GroundArgs a) {
    constexpr int NW = OL_ORDER_THREADS / 64;
    __shared__ int run[OL_NBUCKET];
    __shared__ int wcnt[NW][OL_NBUCKET];
    __shared__ uint32_t sm[17];
    const int f = blockIdx.x, t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int32_t *bc = a.bcount + (size_t)f * OL_NBUCKET;
    uint32_t carry = 0;
    for (int b0 = 0; b0 < OL_NBUCKET; b0 += OL_ORDER_THREADS) {
        const int b = b0 + t;
        const uint32_t v = b < OL_NBUCKET ? (uint32_t)bc[b] : 0u;
        uint32_t tot;
        const uint32_t ex = block_excl_scan(v, sm, &tot);
        if (b < OL_NBUCKET) run[b] = (int)(carry + ex);
        carry += tot;
    }
    for (int b = t; b < NW * OL_NBUCKET; b += OL_ORDER_THREADS) (&wcnt[0][0])[b] = 0;
    __syncthreads();
    const int base = a.off[f], end = a.off[f + 1];
    const unsigned long long lt = (1ull << lane) - 1ull;
    for (int c0 = base; c0 < end; c0 += OL_ORDER_THREADS) {
        const int i = c0 + t;
        const int b = i < end ? a.bucket[i] : -1;
        unsigned long long active = __ballot(b >= 0);
        int rank = 0;
        while (active) {
            const int leader = __ffsll((long long)active) - 1;
            const int lb = __shfl(b, leader, 64);
            const unsigned long long m = __ballot(b == lb) & active;
            if (b == lb) rank = __popcll(m & lt);
            if (lane == leader) wcnt[w][lb] = __popcll(m);
            active &= ~m;
        }
        __syncthreads();
        if (b >= 0) {
            int pos = run[b] + rank;
            for (int w2 = 0; w2 < w; ++w2) pos += wcnt[w2][b];
            float x, y, z;
            load_xyz(a.points, a.is_half, a.stride, i, x, y, z);
            float *o = a.out_xyz + (size_t)(base + pos) * 3;
            o[0] = x, o[1] = y, o[2] = z;
            a.out_src[base + pos] = i - base;
        }
        __syncthreads();
        for (int bb = t; bb < OL_NBUCKET; bb += OL_ORDER_THREADS) {
            int s = 0;
            for (int w2 = 0; w2 < NW; ++w2) {
                s += wcnt[w2][bb];
                wcnt[w2][bb] = 0;
            }
            run[bb] += s;
        }
        __syncthreads();
    }
    if (t == 0) a.out_count[f] = (int)carry;
}

struct GroundLayout {
    size_t code, minz, cover, runs, seg_pos, pos_seg, n_pos, bucket, bcount, err, total;
};
GroundLayout ground_layout(int n_frames, long long n_points) {
    GroundLayout L;
    Carve c;
    L.minz = c.take((size_t)n_frames * OL_NCELL * 4);
    L.bcount = c.take((size_t)n_frames * OL_NBUCKET * 4);
    L.err = c.take(4);
    L.code = c.take((size_t)n_points * 4);
    L.cover = c.take((size_t)n_frames * OL_NCELL * 16);
    L.runs = c.take((size_t)n_frames * OL_NCELL * 16);
    L.seg_pos = c.take((size_t)n_frames * OL_NSEG * 4);
    L.pos_seg = c.take((size_t)n_frames * OL_NSEG * 4);
    L.n_pos = c.take((size_t)n_frames * 4);
    L.bucket = c.take((size_t)n_points * 4);
    L.total = c.o;
    return L;
}

// ---- 2. DBSCAN --------------------------------------------------------------------------------------------------------

struct DbArgs {
    const float *xyz;
    const int32_t *off, *count;
    int n_frames, n_points, min_samples;
    HashGrid grid;              // side eps, tag = frame, members (x, y, z, index bits)
    int32_t *parent;            // [n_points]; -1 = not core (or padding)
    int32_t *gpre;              // [n_points + 1] exclusive prefix of root flags
    uint32_t *scan_ws;
    int32_t *labels, *n_clusters;
};

__device__ __forceinline__ bool db_valid(const DbArgs &a, int i, int &f) {
    f = segment_of(a.off, a.n_frames, i);
    return i - a.off[f] < a.count[f];
}
// the grid's source: the rows within their frame's count, tagged with the frame, w = the row's index bits
struct DbSrc {
    DbArgs a;
    __device__ __forceinline__ bool operator()(int i, int &f, float &x, float &y, float &z, float &w) const {
        if (!db_valid(a, i, f)) return false;
        x = a.xyz[3 * (size_t)i], y = a.xyz[3 * (size_t)i + 1], z = a.xyz[3 * (size_t)i + 2];
        w = __int_as_float(i);
        return true;
    }
};

// visit every point within eps of point i (itself included); fn(j, q) returns false to stop
template <class Fn>
__device__ __forceinline__ void db_for_neighbours(const DbArgs &a, int i, int f, Fn fn) {
    grid_for_near(a.grid, f, a.xyz[3 * (size_t)i], a.xyz[3 * (size_t)i + 1], a.xyz[3 * (size_t)i + 2],
                  [&](float4 q) { return fn(__float_as_int(q.w), q); });
}

__global__ void __launch_bounds__(256) db_core_kernel(DbArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n_points) return;
    int f, n = 0;
    if (db_valid(a, i, f)) {
        const int need = a.min_samples;
        db_for_neighbours(a, i, f, [&](int, float4) { return ++n < need; });
    }
    a.parent[i] = (n > 0 && n >= a.min_samples) ? i : -1;
}

__device__ __forceinline__ int db_find(int32_t *parent, int x) {
    for (;;) {
        const int p = __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (p == x) return x;
        const int gp = __hip_atomic_load(parent + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (gp != p) atomicMin(parent + x, gp);   // path halving (parents only ever decrease)
        x = gp;
    }
}
__device__ __forceinline__ void db_union(int32_t *parent, int u, int v) {
    for (;;) {
        u = db_find(parent, u);
        v = db_find(parent, v);
        if (u == v) return;
        if (u < v) {
            const int t = u;
            u = v;
            v = t;
        }
        const int old = atomicCAS(parent + u, u, v);   // hook the larger root under the smaller
        if (old == u) return;
        u = old;
    }
}

__global__ void __launch_bounds__(256) db_union_kernel(DbArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n_points || a.parent[i] < 0) return;
    int f = segment_of(a.off, a.n_frames, i);
    db_for_neighbours(a, i, f, [&](int j, float4) {
        if (j < i && __hip_atomic_load(a.parent + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= 0) db_union(a.parent, i, j);
        return true;
    });
}

__global__ void __launch_bounds__(256) db_root_kernel(DbArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n_points || a.parent[i] < 0) return;
    a.parent[i] = db_find(a.parent, i);
}

__global__ void __launch_bounds__(256) db_label_kernel(DbArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n_points) return;
    int f;
    if (!db_valid(a, i, f)) {
        a.labels[i] = -1;
        return;
    }
    const int base = a.gpre[a.off[f]];
    int lab = -1;
    if (a.parent[i] >= 0) {
        lab = a.gpre[a.parent[i]] - base;
    } else {
        int best = INT_MAX;
        db_for_neighbours(a, i, f, [&](int j, float4) {
            const int r = a.parent[j];
            if (r >= 0 && r < best) best = r;
            return true;
        });
        if (best != INT_MAX) lab = a.gpre[best] - base;
    }
    a.labels[i] = lab;
    if (i == a.off[f]) a.n_clusters[f] = a.gpre[a.off[f + 1]] - base;
}

struct DbLayout {
    GridLayout grid;
    size_t parent, gpre, total;
};
DbLayout db_layout(long long n_points) {
    DbLayout L;
    Carve c;
    L.grid = grid_carve(c, n_points);   // its scan words serve the root scan over the n_points <= slots / 2 rows too
    L.parent = c.take((size_t)n_points * 4);
    L.gpre = c.take(((size_t)n_points + 1) * 4);
    L.total = c.o;
    return L;
}

// ---- 3. boxes ---------------------------------------------------------------------------------------------------------

struct BoxArgs {
    const float *xyz;
    const int32_t *off, *count, *labels, *n_clusters;
    int n_frames, n_points, apply_filter, box_cap;
    int cluster_min_points;
    double discard_max_height, min_box_volume, min_box_height, max_box_volume, max_box_len, thr0, dist1;
    int32_t *csize, *cstart, *cursor;    // [n_points] per cluster slot (frame start + label)
    uint32_t *czmax, *czmin;
    int32_t *members;                    // [n_points] point index, cluster order
    double2 *hull;                       // [n_points] per cluster its hull, at its member offset
    int32_t *kept;                       // [n_points] kept cluster slots, slot order
    int32_t *n_kept, *fcount;
    double *kbox;                        // [n_points][8] per kept cluster: box + valid flag
    uint32_t *scan_ws;
    double *out;                         // [n_frames] box counts, then [box_cap][8] (box, cluster number)
};

__device__ __forceinline__ bool bx_slot(const BoxArgs &a, int i, int &slot) {
    const int f = segment_of(a.off, a.n_frames, i);
    if (i - a.off[f] >= a.count[f]) return false;
    const int l = a.labels[i];
    if (l < 0 || l >= a.n_clusters[f]) return false;
    slot = a.off[f] + l;
    return slot < a.off[f + 1];
}

__global__ void __launch_bounds__(256) bx_stats_kernel(BoxArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n_points) return;
    int s;
    if (!bx_slot(a, i, s)) return;
    const float z = a.xyz[3 * (size_t)i + 2];
    atomicAdd(a.csize + s, 1);
    atomicMax(a.czmax + s, float_key(z));
    atomicMin(a.czmin + s, float_key(z));
}

__global__ void __launch_bounds__(256) bx_fill_kernel(BoxArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n_points) return;
    int s;
    if (!bx_slot(a, i, s)) return;
    a.members[atomicAdd(a.cursor + s, 1)] = i;
}

__device__ __forceinline__ bool bx_kept(const BoxArgs &a, int s) {
    if (a.csize[s] == 0) return false;
    if (!a.apply_filter) return true;
    return a.csize[s] > a.cluster_min_points && (double)float_unkey(a.czmax[s]) < a.discard_max_height;
}

// r better than q as the next counter-clockwise hull vertex after p (every point lies left of p -> best, or on it nearer)
__device__ __forceinline__ bool bx_better(double px, double py, double qx, double qy, double rx, double ry) {
    const double c = (qx - px) * (ry - py) - (qy - py) * (rx - px);
    if (c < 0.0) return true;
    if (c > 0.0) return false;
    const double dq = (qx - px) * (qx - px) + (qy - py) * (qy - py), dr = (rx - px) * (rx - px) + (ry - py) * (ry - py);
    return dr > dq;
}

__device__ __forceinline__ double bx_wmin(double v) {
    for (int d = 32; d; d >>= 1) v = fmin(v, __shfl_xor(v, d, 64));
    return v;
}
__device__ __forceinline__ double bx_wmax(double v) {
    for (int d = 32; d; d >>= 1) v = fmax(v, __shfl_xor(v, d, 64));
    return v;
}

__device__ __forceinline__ void bx_rot(double ang, double r[4]) {   // [[cos a, cos(a - pi/2)], [cos(a + pi/2), cos a]]
    const double pi2 = M_PI / 2.;
    r[0] = cos(ang), r[1] = cos(ang - pi2), r[2] = cos(ang + pi2), r[3] = cos(ang);
}
__device__ __forceinline__ void bx_extent(const double2 *h, int nh, const double r[4], double e[4]) {
    double mnx = INFINITY, mxx = -INFINITY, mny = INFINITY, mxy = -INFINITY;
    for (int v = 0; v < nh; ++v) {
        const double X = r[0] * h[v].x + r[1] * h[v].y, Y = r[2] * h[v].x + r[3] * h[v].y;
        mnx = fmin(mnx, X), mxx = fmax(mxx, X), mny = fmin(mny, Y), mxy = fmax(mxy, Y);
    }
    e[0] = mnx, e[1] = mxx, e[2] = mny, e[3] = mxy;
}

// get_obj + minimum_bounding_rectangle_distance + box_fit's adjustments (outline_utils.py:609-701, 761-787, 809-846):
// one wave per kept cluster
__global__ void __launch_bounds__(256) bx_fit_kernel(BoxArgs a) {
    const int lane = threadIdx.x & 63;
    const int nwaves = gridDim.x * (blockDim.x >> 6);
    const int K = *a.n_kept;
    for (int k = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); k < K; k += nwaves) {
        const int s = a.kept[k];
        const int m0 = a.cstart[s], mn = a.csize[s];
        const double cut = (double)float_unkey(a.czmin[s]) + 0.2;
        // pass 1: filtered count, z range, start vertex = lexicographic min of (y, x)
        int cnt = 0;
        double zlo = INFINITY, zhi = -INFINITY, sx = INFINITY, sy = INFINITY;
        for (int t = lane; t < mn; t += 64) {
            const int i = a.members[m0 + t];
            const double X = a.xyz[3 * (size_t)i], Y = a.xyz[3 * (size_t)i + 1], Z = a.xyz[3 * (size_t)i + 2];
            if (!(Z > cut)) continue;
            ++cnt;
            zlo = fmin(zlo, Z), zhi = fmax(zhi, Z);
            if (Y < sx || (Y == sx && X < sy)) sx = Y, sy = X;
        }
        for (int d = 32; d; d >>= 1) {
            cnt += __shfl_xor(cnt, d, 64);
            zlo = fmin(zlo, __shfl_xor(zlo, d, 64));
            zhi = fmax(zhi, __shfl_xor(zhi, d, 64));
            const double ox = __shfl_xor(sx, d, 64), oy = __shfl_xor(sy, d, 64);
            if (ox < sx || (ox == sx && oy < sy)) sx = ox, sy = oy;
        }
        double *kb = a.kbox + (size_t)k * 8;
        bool ok = cnt >= 3;
        // pass 2: gift wrapping, counter-clockwise from the start vertex; collinear points are not vertices
        double2 *hull = a.hull + m0;
        int nh = 0;
        double px = sx, py = sy;
        while (ok) {
            if (nh >= cnt) {   // cannot happen with exact orientation tests; never write past the cluster's range
                ok = false;
                break;
            }
            if (lane == 0) hull[nh] = make_double2(px, py);
            ++nh;
            bool have = false;
            double bx = 0.0, by = 0.0;
            for (int t = lane; t < mn; t += 64) {
                const int i = a.members[m0 + t];
                const double X = a.xyz[3 * (size_t)i], Y = a.xyz[3 * (size_t)i + 1], Z = a.xyz[3 * (size_t)i + 2];
                if (!(Z > cut) || (Y == px && X == py)) continue;
                if (!have || bx_better(px, py, bx, by, Y, X)) bx = Y, by = X, have = true;
            }
            for (int d = 32; d; d >>= 1) {
                const int oh = __shfl_xor((int)have, d, 64);
                const double ox = __shfl_xor(bx, d, 64), oy = __shfl_xor(by, d, 64);
                if (oh && (!have || bx_better(px, py, bx, by, ox, oy) ||
                           (!bx_better(px, py, ox, oy, bx, by) && (ox < bx || (ox == bx && oy < by)))))
                    bx = ox, by = oy, have = true;
            }
            have = __shfl((int)have, 0, 64) != 0;   // one answer for the wave
            bx = __shfl(bx, 0, 64);
            by = __shfl(by, 0, 64);
            if (!have) {
                ok = false;
                break;
            }
            if (bx == sx && by == sy) break;
            px = bx, py = by;
        }
        ok = ok && nh >= 3;
        __builtin_amdgcn_wave_barrier();
        __threadfence_block();
        if (!ok) {
            if (lane == 0) kb[7] = 0.0;
            continue;
        }
        // one lane per hull edge: angle, area and distance scores
        const double pi2 = M_PI / 2.;
        double best_s = INFINITY, best_a = 0.0;
        double amin = INFINITY, amax = -INFINITY, vmin = INFINITY, vmax = -INFINITY;
        for (int pass = 0; pass < 2; ++pass) {
            for (int e0 = 0; e0 < nh; e0 += 64) {
                const int e = e0 + lane;
                double ang = 0.0, area = 0.0, val = 0.0;
                const bool act = e < nh;
                if (act) {
                    const double2 h0 = hull[e], h1 = hull[e + 1 < nh ? e + 1 : 0];
                    double md = fmod(atan2(h1.y - h0.y, h1.x - h0.x), pi2);   // np.mod: the sign of the divisor
                    if (md != 0.0 && md < 0.0) md += pi2;
                    ang = fabs(md);
                    double r[4], ex[4];
                    bx_rot(ang, r);
                    bx_extent(hull, nh, r, ex);
                    area = (ex[1] - ex[0]) * (ex[3] - ex[2]) * 0.5;
                    double sum = 0.0;
                    for (int v = 0; v < nh; ++v) {
                        const double X = r[0] * hull[v].x + r[1] * hull[v].y, Y = r[2] * hull[v].x + r[3] * hull[v].y;
                        sum += fmin(fmin(fabs(X - ex[0]), fabs(Y - ex[3])), fmin(fabs(X - ex[1]), fabs(Y - ex[2])));
                    }
                    val = sum / nh * 0.5;
                }
                if (pass == 0) {
                    if (act) amin = fmin(amin, area), amax = fmax(amax, area), vmin = fmin(vmin, val), vmax = fmax(vmax, val);
                } else if (act) {
                    const double sc = (val - vmin) / (vmax - vmin + 0.0001) + (area - amin) / (amax - amin + 0.0001);
                    if (sc < best_s || (sc == best_s && ang < best_a)) best_s = sc, best_a = ang;
                }
            }
            if (pass == 0) amin = bx_wmin(amin), amax = bx_wmax(amax), vmin = bx_wmin(vmin), vmax = bx_wmax(vmax);
        }
        for (int d = 32; d; d >>= 1) {
            const double os = __shfl_xor(best_s, d, 64), oa = __shfl_xor(best_a, d, 64);
            if (os < best_s || (os == best_s && oa < best_a)) best_s = os, best_a = oa;
        }
        if (lane == 0) {
            double r[4], ex[4];
            bx_rot(best_a, r);
            bx_extent(hull, nh, r, ex);
            const double x1 = ex[1], x2 = ex[0], y1 = ex[3], y2 = ex[2];
            // rval[j] = [u, v] @ r
            const double c0x = x1 * r[0] + y2 * r[2], c0y = x1 * r[1] + y2 * r[3];
            const double c1x = x2 * r[0] + y2 * r[2], c1y = x2 * r[1] + y2 * r[3];
            const double c2x = x2 * r[0] + y1 * r[2], c2y = x2 * r[1] + y1 * r[3];
            const double c3x = x1 * r[0] + y1 * r[2], c3y = x1 * r[1] + y1 * r[3];
            const double l = sqrt((c0x - c1x) * (c0x - c1x) + (c0y - c1y) * (c0y - c1y));
            const double w = sqrt((c0x - c3x) * (c0x - c3x) + (c0y - c3y) * (c0y - c3y));
            const double cx = (c0x + c2x) / 2, cy = (c0y + c2y) / 2;
            const double h = zhi - zlo;
            double b[7] = {cy, cx, zhi - h / 2, w, l, h, -best_a};
            b[2] -= 0.2 / 2;
            b[5] += 0.2;
            const double vl = b[3] * b[4] * b[5];
            const double len = fmax(b[3], b[4]);
            if (sqrt((b[0] * b[0] + b[1] * b[1]) + b[2] * b[2]) < a.dist1) {
                b[2] -= a.thr0 / 2;
                b[5] += a.thr0;
            }
            const bool keep = vl > a.min_box_volume && b[5] > a.min_box_height && vl < a.max_box_volume && len < a.max_box_len;
            if (keep && b[3] < b[4]) {
                const double t = b[3];
                b[3] = b[4];
                b[4] = t;
                b[6] += M_PI / 2;
            }
            for (int j = 0; j < 7; ++j) kb[j] = b[j];
            kb[7] = keep ? 1.0 : 0.0;
        }
    }
}

__global__ void __launch_bounds__(256) bx_counts_kernel(const int32_t *fcount, int n_frames, double *out) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f < n_frames) out[f] = (double)fcount[f];
}

struct BoxLayout {
    size_t csize, cstart, cursor, czmax, czmin, members, hull, kept, n_kept, fcount, kbox, scan, total;
};
BoxLayout bx_layout(int n_frames, long long n_points) {
    BoxLayout L;
    Carve c;
    L.csize = c.take((size_t)n_points * 4);
    L.czmax = c.take((size_t)n_points * 4);
    L.n_kept = c.take(4);
    L.fcount = c.take((size_t)n_frames * 4);
    L.czmin = c.take((size_t)n_points * 4);
    L.cstart = c.take((size_t)n_points * 4);
    L.cursor = c.take((size_t)n_points * 4);
    L.members = c.take((size_t)n_points * 4);
    L.hull = c.take((size_t)n_points * 16);
    L.kept = c.take((size_t)n_points * 4);
    L.kbox = c.take((size_t)n_points * 64);
    L.scan = c.take((size_t)scan_num_blocks(n_points) * 4);
    L.total = c.o;
    return L;
}

}  // namespace

extern "C" {

size_t cpd_outline_ground_workspace_bytes(int n_frames, int n_points) {
    if (n_frames <= 0 || n_points < 0) return 0;
    return ground_layout(n_frames, n_points).total;
}

int cpd_outline_ground(const void *points, int is_half, int row_stride, const int32_t *frame_off, int n_frames, int n_points,
                       const float consts[5], double sensor_height, const double *thr, const double *dist, int n_bands,
                       float *out_xyz, int32_t *out_src, int32_t *out_count, int32_t *err, void *workspace,
                       size_t workspace_bytes, cpd_stream_t stream) {
    if (n_frames <= 0 || n_points < 0 || row_stride < 3 || !frame_off || !consts || !thr || !dist || !out_count || !err)
        return CPD_ERR_ARG;
    if (n_bands < 1 || n_bands > OL_MAX_BANDS || (is_half != 0 && is_half != 1)) return CPD_ERR_ARG;
    if (n_points > 0 && (!points || !out_xyz || !out_src)) return CPD_ERR_ARG;
    const GroundLayout L = ground_layout(n_frames, n_points);
    if (!workspace || workspace_bytes < L.total) return CPD_ERR_WORKSPACE;
    hipStream_t st = cpd_s(stream);
    GroundArgs a;
    a.points = points, a.is_half = is_half, a.stride = row_stride, a.n_frames = n_frames, a.n_points = n_points;
    a.off = frame_off;
    a.c_pi = consts[0], a.c_seg_step = consts[1], a.c_rmin = consts[2], a.c_bin_step = consts[3], a.c_high = consts[4];
    a.sensor_height = sensor_height, a.n_bands = n_bands;
    for (int i = 0; i < OL_MAX_BANDS; ++i) a.thr[i] = i < n_bands ? thr[i] : 0.0;
    for (int i = 0; i <= OL_MAX_BANDS; ++i) a.dist[i] = dist[i];
    a.code = ws_at<int32_t>(workspace, L.code), a.minz = ws_at<uint32_t>(workspace, L.minz);
    a.cover = ws_at<double2>(workspace, L.cover), a.runs = ws_at<double2>(workspace, L.runs);
    a.seg_pos = ws_at<int32_t>(workspace, L.seg_pos), a.pos_seg = ws_at<int32_t>(workspace, L.pos_seg);
    a.n_pos = ws_at<int32_t>(workspace, L.n_pos), a.bucket = ws_at<int32_t>(workspace, L.bucket);
    a.bcount = ws_at<int32_t>(workspace, L.bcount), a.err = err;
    a.out_xyz = out_xyz, a.out_src = out_src, a.out_count = out_count;
    CPD_HIP_TRY(hipMemsetAsync(a.minz, 0xff, (size_t)n_frames * OL_NCELL * 4, st));
    CPD_HIP_TRY(hipMemsetAsync(a.bcount, 0, (size_t)n_frames * OL_NBUCKET * 4, st));
    const unsigned blocks = (unsigned)cpd_div_up(n_points, 256);
    if (n_points > 0) ol_project_kernel<<<blocks, 256, 0, st>>>(a);
    ol_fit_kernel<<<n_frames, 256, 0, st>>>(a);
    if (n_points > 0) ol_label_kernel<<<blocks, 256, 0, st>>>(a);
    ol_order_kernel<<<n_frames, OL_ORDER_THREADS, 0, st>>>(a);
    return cpd_check_launch();
}

size_t cpd_outline_dbscan_workspace_bytes(int n_frames, int n_points) {
    if (n_frames <= 0 || n_points < 0) return 0;
    return db_layout(n_points).total;
}

int cpd_outline_dbscan(const float *xyz, const int32_t *frame_off, const int32_t *frame_count, int n_frames, int n_points,
                       double eps, int min_samples, int32_t *labels, int32_t *n_clusters, void *workspace,
                       size_t workspace_bytes, cpd_stream_t stream) {
    if (n_frames <= 0 || n_frames > 1023 || n_points < 0 || !frame_off || !frame_count || !n_clusters || !(eps > 0.0))
        return CPD_ERR_ARG;
    if (n_points > 0 && (!xyz || !labels)) return CPD_ERR_ARG;
    const DbLayout L = db_layout(n_points);
    if (!workspace || workspace_bytes < L.total) return CPD_ERR_WORKSPACE;
    hipStream_t st = cpd_s(stream);
    DbArgs a;
    a.xyz = xyz, a.off = frame_off, a.count = frame_count, a.n_frames = n_frames, a.n_points = n_points;
    a.min_samples = min_samples, a.grid = L.grid.view(workspace, eps, eps * eps);
    a.parent = ws_at<int32_t>(workspace, L.parent), a.gpre = ws_at<int32_t>(workspace, L.gpre);
    a.scan_ws = ws_at<uint32_t>(workspace, L.grid.scan), a.labels = labels, a.n_clusters = n_clusters;
    // frames with no rows still need n_clusters = 0 (the labelling kernel writes it from a frame's first row)
    CPD_HIP_TRY(hipMemsetAsync(n_clusters, 0, (size_t)n_frames * 4, st));
    int rc = grid_build(a.grid, n_points, DbSrc{a}, a.scan_ws, st);
    if (rc != CPD_OK || n_points == 0) return rc;
    const unsigned blocks = (unsigned)cpd_div_up(n_points, 256);
    db_core_kernel<<<blocks, 256, 0, st>>>(a);
    db_union_kernel<<<blocks, 256, 0, st>>>(a);
    db_root_kernel<<<blocks, 256, 0, st>>>(a);
    const int32_t *parent = a.parent;
    int32_t *gpre = a.gpre;
    rc = device_scan(
        (long long)n_points, [=] __device__(long long i) { return parent[i] == (int32_t)i ? 1u : 0u; },
        [=] __device__(long long i, uint32_t, uint32_t pre) { gpre[i] = (int32_t)pre; }, a.scan_ws, gpre + n_points, -1, st);
    if (rc != CPD_OK) return rc;
    db_label_kernel<<<blocks, 256, 0, st>>>(a);
    return cpd_check_launch();
}

size_t cpd_outline_boxes_workspace_bytes(int n_frames, int n_points) {
    if (n_frames <= 0 || n_points < 0) return 0;
    return bx_layout(n_frames, n_points).total;
}

int cpd_outline_boxes(const float *xyz, const int32_t *frame_off, const int32_t *frame_count, int n_frames, int n_points,
                      const int32_t *labels, const int32_t *n_clusters, int apply_cluster_filter, const double params[8],
                      int box_cap, double *out, void *workspace, size_t workspace_bytes, cpd_stream_t stream) {
    if (n_frames <= 0 || n_points < 0 || !frame_off || !frame_count || !n_clusters || !params || !out || box_cap < 0)
        return CPD_ERR_ARG;
    if (n_points > 0 && (!xyz || !labels)) return CPD_ERR_ARG;
    const BoxLayout L = bx_layout(n_frames, n_points);
    if (!workspace || workspace_bytes < L.total) return CPD_ERR_WORKSPACE;
    hipStream_t st = cpd_s(stream);
    BoxArgs a;
    a.xyz = xyz, a.off = frame_off, a.count = frame_count, a.labels = labels, a.n_clusters = n_clusters;
    a.n_frames = n_frames, a.n_points = n_points, a.apply_filter = apply_cluster_filter, a.box_cap = box_cap;
    a.cluster_min_points = (int)params[0], a.discard_max_height = params[1], a.min_box_volume = params[2];
    a.min_box_height = params[3], a.max_box_volume = params[4], a.max_box_len = params[5], a.thr0 = params[6];
    a.dist1 = params[7];
    a.csize = ws_at<int32_t>(workspace, L.csize), a.cstart = ws_at<int32_t>(workspace, L.cstart);
    a.cursor = ws_at<int32_t>(workspace, L.cursor), a.czmax = ws_at<uint32_t>(workspace, L.czmax);
    a.czmin = ws_at<uint32_t>(workspace, L.czmin), a.members = ws_at<int32_t>(workspace, L.members);
    a.hull = ws_at<double2>(workspace, L.hull), a.kept = ws_at<int32_t>(workspace, L.kept), a.n_kept = ws_at<int32_t>(workspace, L.n_kept);
    a.fcount = ws_at<int32_t>(workspace, L.fcount);
    a.kbox = ws_at<double>(workspace, L.kbox), a.scan_ws = ws_at<uint32_t>(workspace, L.scan), a.out = out;
    // csize, czmax (key 0 = below every float), n_kept and fcount are adjacent: one clear; czmin keys start at all ones
    CPD_HIP_TRY(hipMemsetAsync(a.csize, 0, L.czmin, st));
    CPD_HIP_TRY(hipMemsetAsync(a.czmin, 0xff, (size_t)n_points * 4, st));
    CPD_HIP_TRY(hipMemsetAsync(out, 0, ((size_t)n_frames + (size_t)box_cap * 8) * 8, st));
    if (n_points == 0) return CPD_OK;
    const unsigned blocks = (unsigned)cpd_div_up(n_points, 256);
    bx_stats_kernel<<<blocks, 256, 0, st>>>(a);
    const int32_t *csize = a.csize;
    int32_t *cstart = a.cstart, *cursor = a.cursor;
    int rc = device_scan(
        (long long)n_points, [=] __device__(long long i) { return (uint32_t)csize[i]; },
        [=] __device__(long long i, uint32_t, uint32_t pre) { cstart[i] = (int32_t)pre, cursor[i] = (int32_t)pre; }, a.scan_ws,
        nullptr, -1, st);
    if (rc != CPD_OK) return rc;
    bx_fill_kernel<<<blocks, 256, 0, st>>>(a);
    const BoxArgs ac = a;
    int32_t *kept = a.kept;
    rc = device_scan(
        (long long)n_points, [=] __device__(long long i) { return bx_kept(ac, (int)i) ? 1u : 0u; },
        [=] __device__(long long i, uint32_t v, uint32_t pre) {
            if (v) kept[pre] = (int32_t)i;
        },
        a.scan_ws, a.n_kept, -1, st);
    if (rc != CPD_OK) return rc;
    bx_fit_kernel<<<1024, 256, 0, st>>>(a);
    // compaction of the fitted boxes in slot order (= frame, cluster number) into out
    const int32_t *n_kept = a.n_kept;
    const double *kbox = a.kbox;
    const int32_t *off = a.off;
    int32_t *fcount = a.fcount;
    const int nf = n_frames, cap = box_cap;
    rc = device_scan(
        (long long)n_points, [=] __device__(long long k) { return (k < *n_kept && kbox[k * 8 + 7] != 0.0) ? 1u : 0u; },
        [=] __device__(long long k, uint32_t v, uint32_t pre) {
            if (!v) return;
            const int s = kept[k];
            const int f = segment_of(off, nf, s);
            atomicAdd(fcount + f, 1);
            if ((int)pre < cap) {
                double *o = out + nf + (size_t)pre * 8;
                for (int j = 0; j < 7; ++j) o[j] = kbox[k * 8 + j];
                o[7] = (double)(s - off[f]);
            }
        },
        a.scan_ws, nullptr, -1, st);
    if (rc != CPD_OK) return rc;
    bx_counts_kernel<<<cpd_div_up(n_frames, 256), 256, 0, st>>>(fcount, n_frames, out);
    return cpd_check_launch();
}

}  // extern "C"
