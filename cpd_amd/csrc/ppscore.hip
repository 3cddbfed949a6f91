// ppscore.hip -- CPD's PP-score precompute (cpd/unsupervised_core/precompute_ppscore.py) for ONE current frame against its
// T <= 16 traversals per call:
//   a. every traversal point goes sweep -> world (its own pose) -> current frame (inverse of the current pose): two float64
//      products in the accumulation order of the reference's np.mat product (pp_row below), each rounded to float32 (the
//      rounding in world coordinates is the reference's and is kept);
//   b. one hashed uniform grid of side r over all traversals, tagged by traversal (hash_grid.h, shared with outline.hip's
//      DBSCAN);
//   c. one lane per (query point, traversal) walks the 27 cells (grid_for_near) and counts the members with float64
//      (dx*dx + dy*dy) + dz*dz <= r*r (cKDTree.query_ball_point(..., return_length=True): inclusive); lanes of a wave are
//      consecutive query rows of one traversal, which in scan order walk the same cells. Queries are the RAW rows of the
//      current frame, not transformed (that is what the reference does);
//   d. compute_ephe_score: P = c / (sum c + 1e-8), H = sum -P log(P + 1e-8) / log(T) in float64, stored as float16 bits;
//      T < 2 gives NaN (the reference divides by log(1) = 0).
// Integer atomics only (slot claims, counts, cursors): the order of a cell's members varies from call to call, the counts
// do not. Built with -ffp-contract=off: the compiler fuses nothing; the only fused multiply-adds are the explicit ones of
// the pose product, which are the reference's.
#include <math.h>

#include "common.h"
#include "hash_grid.h"
#include "rigid_f64.h"   // pp_row, pp_rigid3: shared with mfcf.hip

namespace {

constexpr int PP_MAX_TRAV = 16;

struct PpArgs {
    const void *query, *ref;
    int n_query, query_stride, query_half;
    int n_ref, ref_stride, ref_half;
    int n_trav, has_pose;
    int32_t off[PP_MAX_TRAV + 1];
    double pose[PP_MAX_TRAV][12];   // rows 0..2 of the 4x4 sweep -> world matrices
    double cur_inv[12];             // rows 0..2 of inverse(current pose)
    double log_t;
    HashGrid grid;                  // side r over all traversals, tag = traversal, members (x, y, z, 0)
    int32_t *counts;                // [n_query][n_trav]
    uint16_t *h;                    // [n_query] float16 bits
};

// traversal point i in the current frame's coordinates, and its traversal
__device__ __forceinline__ int pp_ref_point(const PpArgs &a, int i, float &x, float &y, float &z) {
    int t = 0;
    while (t + 1 < a.n_trav && i >= a.off[t + 1]) ++t;
    load_xyz(a.ref, a.ref_half, a.ref_stride, i, x, y, z);
    if (a.has_pose) {
        float wx, wy, wz;
        pp_rigid3(a.pose[t], x, y, z, wx, wy, wz);
        pp_rigid3(a.cur_inv, wx, wy, wz, x, y, z);
    }
    return t;
}

// the grid's source: every traversal point, tagged with its traversal
struct PpSrc {
    PpArgs a;
    __device__ __forceinline__ bool operator()(int i, int &tag, float &x, float &y, float &z, float &w) const {
        tag = pp_ref_point(a, i, x, y, z);
        w = 0.f;
        return true;
    }
};

__global__ void __launch_bounds__(256) pp_count_kernel(PpArgs a) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    const int t = blockIdx.y;
    if (q >= a.n_query) return;
    int n = 0;
    if (a.off[t + 1] > a.off[t]) {
        float x, y, z;
        load_xyz(a.query, a.query_half, a.query_stride, q, x, y, z);
        grid_for_near(a.grid, t, x, y, z, [&](float4) {
            ++n;
            return true;
        });
    }
    a.counts[(size_t)q * a.n_trav + t] = n;
}

// float64 -> float16 with ONE rounding (numpy's astype(np.float16)): the float32 step rounds to odd, which keeps the sticky
// information the final round-to-nearest-even needs (float32 carries more than two bits beyond float16's precision)
__device__ __forceinline__ uint16_t pp_half_bits(double d) {
    float f = (float)d;
    if ((double)f != d) {
        uint32_t u = __float_as_uint(f);
        if (fabs((double)f) > fabs(d)) u -= 1;   // back towards zero (f != 0 here)
        f = __uint_as_float(u | 1u);
    }
    const _Float16 hf = (_Float16)f;
    uint16_t b;
    __builtin_memcpy(&b, &hf, 2);
    return b;
}

// compute_ephe_score (precompute_ppscore.py:16-21); the sum over traversals runs in traversal order
__global__ void __launch_bounds__(256) pp_score_kernel(PpArgs a) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= a.n_query) return;
    if (a.n_trav < 2) {
        a.h[q] = 0x7e00;
        return;
    }
    const int32_t *c = a.counts + (size_t)q * a.n_trav;
    long long total = 0;
    for (int t = 0; t < a.n_trav; ++t) total += c[t];
    const double den = (double)total + 1e-8;
    double hsum = 0.0;
    for (int t = 0; t < a.n_trav; ++t) {
        const double p = (double)c[t] / den;
        const double term = (-p) * log(p + 1e-8);
        hsum = t == 0 ? term : hsum + term;
    }
    a.h[q] = pp_half_bits(hsum / a.log_t);
}

struct PpLayout {
    GridLayout grid;
    size_t counts, total;
};
PpLayout pp_layout(long long n_query, long long n_ref, int n_trav) {
    PpLayout L;
    Carve c;
    L.grid = grid_carve(c, n_ref);
    L.counts = c.take((size_t)n_query * (size_t)(n_trav > 0 ? n_trav : 1) * 4);
    L.total = c.o;
    return L;
}

}  // namespace

extern "C" {

size_t cpd_ppscore_workspace_bytes(int n_query, int n_ref_total, int n_trav) {
    if (n_query < 0 || n_ref_total < 0 || n_trav < 0 || n_trav > PP_MAX_TRAV) return 0;
    return pp_layout(n_query, n_ref_total, n_trav).total;
}

int cpd_ppscore(const void *query, int n_query, int query_stride, int query_dtype, const void *ref, const int32_t *trav_offsets,
                int n_trav, int ref_stride, int ref_dtype, const double *poses, const double *cur_pose_inv, double radius,
                int32_t *counts, uint16_t *h, void *workspace, size_t workspace_bytes, cpd_stream_t stream) {
    if (n_trav > PP_MAX_TRAV) return CPD_ERR_UNSUPPORTED;
    if (n_query < 0 || n_trav < 0 || !trav_offsets || !(radius > 0.0) || !(radius * radius < INFINITY)) return CPD_ERR_ARG;
    if ((query_dtype != 0 && query_dtype != 1) || (ref_dtype != 0 && ref_dtype != 1)) return CPD_ERR_ARG;
    if (query_stride < 3 || ref_stride < 3 || (poses == nullptr) != (cur_pose_inv == nullptr)) return CPD_ERR_ARG;
    if (trav_offsets[0] != 0) return CPD_ERR_ARG;
    for (int t = 0; t < n_trav; ++t)
        if (trav_offsets[t + 1] < trav_offsets[t]) return CPD_ERR_ARG;
    const int n_ref = trav_offsets[n_trav];
    if ((n_query > 0 && !query) || (n_ref > 0 && !ref)) return CPD_ERR_ARG;
    const PpLayout L = pp_layout(n_query, n_ref, n_trav);
    if (!workspace || workspace_bytes < L.total) return CPD_ERR_WORKSPACE;
    hipStream_t st = cpd_s(stream);
    PpArgs a;
    a.query = query, a.ref = ref, a.n_query = n_query, a.query_stride = query_stride, a.query_half = query_dtype;
    a.n_ref = n_ref, a.ref_stride = ref_stride, a.ref_half = ref_dtype, a.n_trav = n_trav, a.has_pose = poses != nullptr;
    for (int t = 0; t <= PP_MAX_TRAV; ++t) a.off[t] = trav_offsets[t < n_trav ? t : n_trav];
    for (int t = 0; t < PP_MAX_TRAV; ++t)
        for (int k = 0; k < 12; ++k) a.pose[t][k] = (poses && t < n_trav) ? poses[(size_t)t * 16 + k] : 0.0;
    for (int k = 0; k < 12; ++k) a.cur_inv[k] = cur_pose_inv ? cur_pose_inv[k] : 0.0;
    a.log_t = log((double)(n_trav > 0 ? n_trav : 1));
    a.grid = L.grid.view(workspace, radius, radius * radius);
    a.counts = counts ? counts : ws_at<int32_t>(workspace, L.counts);
    a.h = h;
    if (n_query == 0 || (n_trav == 0 && !h)) return CPD_OK;
    if (n_trav > 0) {
        const int rc = grid_build(a.grid, n_ref, PpSrc{a}, ws_at<uint32_t>(workspace, L.grid.scan), st);
        if (rc != CPD_OK) return rc;
        pp_count_kernel<<<dim3((unsigned)cpd_div_up(n_query, 256), (unsigned)n_trav), 256, 0, st>>>(a);
    }
    if (h) pp_score_kernel<<<(unsigned)cpd_div_up(n_query, 256), 256, 0, st>>>(a);
    return cpd_check_launch();
}

}  // extern "C"
