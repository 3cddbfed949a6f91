// augment.hip -- the training-time augmentor's point work:
//   * cpd_augment_scene       = DataBaseSampler.add_sampled_boxes_to_scene (database_sampler.py:359-416: paste the sampled
//                               objects, remove the scene points inside the enlarged sampled boxes), then the AUG_CONFIG_LIST
//                               transforms (augmentor_utils.py:8-105), then mask_points_by_range (common_utils.py:60-63) --
//                               one flag pass, one scan / emit; nothing intermediate is written
//   * cpd_group_points_by_box = the point work of create_track_groundtruth_database (waymo_unsupervised_dataset.py:711-725):
//                               rows grouped by ascending box id, order kept inside a box, centred on the box
// This file is compiled with -ffp-contract=off (csrc/Makefile): the paste offset and the centring are float64 operations
// rounded once, the scaling is one float32 product by the factor rounded to float32 (np.random.uniform and a yaml number are
// Python floats: numpy multiplies a float32 array by them in float32), the in-box test is the reference's fp32 / double expression (pt_in_box.h). The rotation is the one
// place where a fused multiply-add is written, explicitly: torch's CPU float32 matmul of [1, N, 3] x [1, 3, 3] evaluates
// fma(y, R[1][j], fl(x * R[0][j])) for all but tiny N. The op list and its arithmetic live in aug_ops.h, which tta.hip shares.
#include "aug_ops.h"
#include "pt_in_box.h"

namespace {

struct AugRows {
    const float *scene;
    int n, c;
    const float *obj_base;
    int c_obj, k_obj;
    long long m;                         // object rows: virtual rows [0, m) are objects, [m, m + n) the scene
    const int32_t *seg_off;              // [k_obj + 1] exclusive prefix of the segment counts (device)
    const long long *seg_start;          // [k_obj] first row of the segment in obj_base
    const double *seg_centre;            // [k_obj][3]
    AugOps ops;
    int has_range;
    float x0, y0, x1, y1;

    // virtual row i -> its source row and its coordinates before the ops
    __device__ __forceinline__ const float *load(long long i, float &x, float &y, float &z) const {
        if (i < m) {
            const int sgm = segment_of(seg_off, k_obj, (int)i);
            const float *p = obj_base + (size_t)(seg_start[sgm] + (i - seg_off[sgm])) * c_obj;
            const double *ctr = seg_centre + 3 * (size_t)sgm;
            x = (float)((double)p[0] + ctr[0]);          // obj_points[:, :3] += info['box3d_lidar'][:3]: float32 + float64
            y = (float)((double)p[1] + ctr[1]);
            z = (float)((double)p[2] + ctr[2]);
            return p;
        }
        const float *p = scene + (size_t)(i - m) * c;
        x = p[0]; y = p[1]; z = p[2];
        return p;
    }
    __device__ __forceinline__ void apply(float &x, float &y, float &z) const { aug_apply(ops, x, y, z); }     // (aug_ops.h)
    __device__ __forceinline__ bool in_range(float x, float y) const {      // false for NaN, as numpy's comparisons are
        return !has_range || (x >= x0 && x <= x1 && y >= y0 && y <= y1);
    }
};

// keep[i] = 1 when virtual row i survives: a scene row lies in no box; the row, after the ops, lies in the range.
__global__ void __launch_bounds__(256) augment_flags_kernel(AugRows r, const float *__restrict__ boxes, int k,
                                                            uint8_t *__restrict__ keep) {
    __shared__ float sbox[CPD_BOX_LDS_CHUNK * CPD_BOX_LDS_FLOATS];
    const long long total = r.m + r.n;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = i < total;
    float x = 0.f, y = 0.f, z = 0.f;
    if (live) r.load(i, x, y, z);
    bool hit = false;
    const bool block_has_scene = (long long)(blockIdx.x + 1) * blockDim.x > r.m;      // block-uniform
    if (block_has_scene) {
        for (int k0 = 0; k0 < k; k0 += CPD_BOX_LDS_CHUNK) {
            const int nk = min(CPD_BOX_LDS_CHUNK, k - k0);
            __syncthreads();
            for (int j = threadIdx.x; j < nk; j += blockDim.x) stage_box_cpu(sbox, j, boxes + 7 * (size_t)(k0 + j));
            __syncthreads();
            if (live && i >= r.m && !hit) {
                for (int j = 0; j < nk; ++j) {
                    const float *bq = sbox + CPD_BOX_LDS_FLOATS * j;
                    if (pt_in_box_cpu(x, y, z, bq, bq[6], bq[7])) { hit = true; break; }
                }
            }
        }
    }
    if (!live) return;
    r.apply(x, y, z);
    keep[i] = (!hit && r.in_range(x, y)) ? 1 : 0;
}

struct KeepFlagFn {
    const uint8_t *keep;
    __device__ uint32_t operator()(long long i) const { return keep[i]; }
};
struct AugEmitFn {        // stable compaction; the transform is recomputed here
    AugRows r;
    float *out;
    __device__ void operator()(long long i, uint32_t flag, uint32_t prefix) const {
        if (!flag) return;
        float x, y, z;
        const float *p = r.load(i, x, y, z);
        r.apply(x, y, z);
        float *o = out + (size_t)prefix * r.c;
        o[0] = x; o[1] = y; o[2] = z;
        for (int q = 3; q < r.c; ++q) o[q] = p[q];
    }
};

struct AugTable {                        // the pasted segments, host-built, one copy per call
    double centre[3 * 512];
    long long start[512];
    int32_t off[513];
};
struct AugLayout { size_t keep, scan, table, total; };
AugLayout augment_layout(long long total, int k_obj) {
    Carve cv;
    AugLayout l;
    l.keep = cv.take((size_t)(total > 0 ? total : 1));
    l.scan = cv.take((size_t)scan_num_blocks(total) * 4 + 16);
    (void)k_obj;
    l.table = cv.take(sizeof(AugTable));
    l.total = cv.o;
    return l;
}

// ---- cpd_group_points_by_box ---------------------------------------------------------------------------------------------
// A block owns GROUP_TILE consecutive rows, each of its 4 waves a contiguous quarter (the scan's layout, common.h).
#define GROUP_TILE 2048
#define GROUP_MAX_BOXES 1024

// counts[b * nb + block] = rows of `block` whose box is b: box-major, so ONE exclusive scan over the table gives every
// (box, block) pair its first output row and offsets[b] at (b, block 0).
__global__ void __launch_bounds__(256) group_count_kernel(const int32_t *__restrict__ box_idx, int n, int k, int nb,
                                                          uint32_t *__restrict__ counts) {
    __shared__ uint32_t hist[GROUP_MAX_BOXES];
    for (int b = threadIdx.x; b < k; b += blockDim.x) hist[b] = 0;
    __syncthreads();
    const long long base = (long long)blockIdx.x * GROUP_TILE;
    for (int t = threadIdx.x; t < GROUP_TILE; t += blockDim.x) {
        const long long i = base + t;
        if (i >= n) break;
        const int32_t b = box_idx[i];
        if (b >= 0 && b < k) atomicAdd(&hist[b], 1u);
    }
    __syncthreads();
    for (int b = threadIdx.x; b < k; b += blockDim.x) counts[(size_t)b * nb + blockIdx.x] = hist[b];
}

struct CountFn {
    const uint32_t *counts;
    __device__ uint32_t operator()(long long i) const { return counts[i]; }
};
struct GroupStartFn {     // first[b * nb + block] = exclusive prefix; offsets[b] = the prefix at block 0
    uint32_t *first;
    int32_t *offsets;
    int nb;
    __device__ void operator()(long long i, uint32_t, uint32_t prefix) const {
        first[i] = prefix;
        if (i % nb == 0) offsets[i / nb] = (int32_t)prefix;
    }
};

// The scatter. Rank of a row inside its block = rows of the same box in earlier waves of the block (a per-wave LDS histogram,
// prefixed in wave order) + rows of the same box earlier in this wave (its 64-row steps in order; inside a step, the lanes of
// one box found by ballot, their rank a popcount of the lower lanes) -- stable, no atomics on the ranks.
__global__ void __launch_bounds__(256) group_scatter_kernel(const float *__restrict__ pts, const int32_t *__restrict__ box_idx,
                                                            int n, int c, int k, int nb, const uint32_t *__restrict__ first,
                                                            const double *__restrict__ centre, float *__restrict__ out) {
    __shared__ uint32_t whist[4][GROUP_MAX_BOXES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int j = threadIdx.x; j < 4 * GROUP_MAX_BOXES; j += blockDim.x) (&whist[0][0])[j] = 0;
    __syncthreads();
    const long long wbase = (long long)blockIdx.x * GROUP_TILE + (long long)wave * (GROUP_TILE / 4);
    for (int s = 0; s < GROUP_TILE / 4; s += 64) {
        const long long i = wbase + s + lane;
        if (i < n) {
            const int32_t b = box_idx[i];
            if (b >= 0 && b < k) atomicAdd(&whist[wave][b], 1u);
        }
    }
    __syncthreads();
    for (int b = threadIdx.x; b < k; b += blockDim.x) {
        uint32_t at = first[(size_t)b * nb + blockIdx.x];
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const uint32_t t = whist[w][b];
            whist[w][b] = at;
            at += t;
        }
    }
    __syncthreads();
    volatile uint32_t *next = whist[wave];                 // this wave's running output row per box; no other wave touches it
    for (int s = 0; s < GROUP_TILE / 4; s += 64) {
        const long long i = wbase + s + lane;
        int32_t b = -1;
        if (i < n) {
            b = box_idx[i];
            if (b >= k) b = -1;
        }
        bool pending = b >= 0;
        uint32_t dst = 0;
        unsigned long long todo = __ballot(pending);
        while (todo) {                                     // one turn per distinct box among the wave's 64 rows
            const int leader = __ffsll((long long)todo) - 1;
            const int32_t lb = __shfl(b, leader, 64);
            const unsigned long long same = __ballot(pending && b == lb);
            if (pending && b == lb) {
                const uint32_t at = next[b];
                const int rank = __popcll(same & ((1ull << lane) - 1ull));
                dst = at + rank;
                __builtin_amdgcn_wave_barrier();           // every lane of the box has read `at` before the leader moves it
                if (lane == leader) next[b] = at + (uint32_t)__popcll(same);
                pending = false;
            }
            todo &= ~same;
        }
        if (b >= 0) {
            const float *p = pts + (size_t)i * c;
            const double *ctr = centre + 3 * (size_t)b;
            float *o = out + (size_t)dst * c;
            o[0] = (float)((double)p[0] - ctr[0]);         // gt_points[:, :3] -= gt_boxes[i, :3]: float32 - float64
            o[1] = (float)((double)p[1] - ctr[1]);
            o[2] = (float)((double)p[2] - ctr[2]);
            for (int q = 3; q < c; ++q) o[q] = p[q];
        }
    }
}

struct GroupLayout { size_t counts, first, scan, centre, total; };
GroupLayout group_layout(int n, int k) {
    const long long nb = n > 0 ? ((long long)n + GROUP_TILE - 1) / GROUP_TILE : 1;
    const long long cells = nb * (k > 0 ? k : 1);
    Carve cv;
    GroupLayout l;
    l.counts = cv.take((size_t)cells * 4);
    l.first = cv.take((size_t)cells * 4);
    l.scan = cv.take((size_t)scan_num_blocks(cells) * 4 + 16);
    l.centre = cv.take((size_t)(k > 0 ? k : 1) * 24);
    l.total = cv.o;
    return l;
}

}  // namespace

extern "C" size_t cpd_augment_scene_workspace_bytes(int n, int m, int k_obj) {
    if (n < 0 || m < 0 || k_obj < 0) return 0;
    return augment_layout((long long)n + m, k_obj).total;
}

extern "C" int cpd_augment_scene(const float *scene, int n, int c, const float *obj_base, long long obj_rows, int c_obj,
                                 const int64_t *obj_start, const int32_t *obj_count, const double *obj_centre, int k_obj, const float *boxes, int k,
                                 const int32_t *op_kind, const double *op_param, int n_ops, const float *range_xyz, float *out,
                                 int32_t *n_out, void *workspace, size_t workspace_bytes, cpd_stream_t st) {
    if (n < 0 || c < 3 || k_obj < 0 || k < 0 || n_ops < 0 || !n_out || !workspace || (n > 0 && !scene) || (k > 0 && !boxes) ||
        (k_obj > 0 && (!obj_start || !obj_count || !obj_centre || c_obj < c)) || (n_ops > 0 && (!op_kind || !op_param)))
        return CPD_ERR_ARG;
    if (k > 512 || k_obj > 512 || n_ops > CPD_AUG_MAX_OPS) return CPD_ERR_UNSUPPORTED;
    long long m = 0;
    for (int s = 0; s < k_obj; ++s) {
        if (obj_count[s] < 0 || obj_start[s] < 0) return CPD_ERR_ARG;
        m += obj_count[s];
    }
    const long long total = m + n;
    if (total >= (1ll << 31)) return CPD_ERR_UNSUPPORTED;
    for (int s = 0; s < k_obj; ++s)
        if (obj_start[s] + obj_count[s] > obj_rows) return CPD_ERR_ARG;
    if ((m > 0 && !obj_base) || (total > 0 && !out)) return CPD_ERR_ARG;
    AugRows r{};
    if (aug_ops_fill(r.ops, op_kind, op_param, n_ops) != CPD_OK) return CPD_ERR_ARG;
    const AugLayout l = augment_layout(total, k_obj);
    if (workspace_bytes < l.total) return CPD_ERR_WORKSPACE;
    hipStream_t s = cpd_s(st);
    if (total == 0) {
        CPD_HIP_TRY(hipMemsetAsync(n_out, 0, 4, s));
        return CPD_OK;
    }
    if (k_obj > 0) {
        // The segment table (at most 512 x 36 bytes: too large for kernel arguments) goes up in ONE copy, on the call's stream so
        // that it is ordered after whatever still reads this workspace. `table` is pageable host memory that dies with this
        // call: for a pageable source hipMemcpyAsync does not return before the source has been read (the HIP runtime makes the
        // host wait for such a copy, as the HIP API documents for non-pinned memory), which is what is relied on here.
        AugTable table;
        table.off[0] = 0;
        for (int q = 0; q < k_obj; ++q) {
            table.off[q + 1] = table.off[q] + obj_count[q];
            table.start[q] = obj_start[q];
            for (int d = 0; d < 3; ++d) table.centre[3 * q + d] = obj_centre[3 * q + d];
        }
        CPD_HIP_TRY(hipMemcpyAsync(ws_at<AugTable>(workspace, l.table), &table, sizeof(AugTable), hipMemcpyHostToDevice, s));
    }
    r.scene = scene; r.n = n; r.c = c;
    r.obj_base = obj_base; r.c_obj = c_obj; r.k_obj = k_obj; r.m = m;
    const AugTable *dtable = ws_at<AugTable>(workspace, l.table);
    r.seg_off = dtable->off;
    r.seg_start = dtable->start;
    r.seg_centre = dtable->centre;
    r.has_range = range_xyz ? 1 : 0;
    if (range_xyz) { r.x0 = range_xyz[0]; r.y0 = range_xyz[1]; r.x1 = range_xyz[3]; r.y1 = range_xyz[4]; }
    uint8_t *keep = ws_at<uint8_t>(workspace, l.keep);
    augment_flags_kernel<<<cpd_div_up(total, 256), 256, 0, s>>>(r, boxes, k, keep);
    const int rc = cpd_check_launch();
    if (rc != CPD_OK) return rc;
    return device_scan(total, KeepFlagFn{keep}, AugEmitFn{r, out}, ws_at<uint32_t>(workspace, l.scan), n_out, -1, s);
}

extern "C" size_t cpd_group_points_by_box_workspace_bytes(int n, int k) {
    if (n < 0 || k < 0 || k > GROUP_MAX_BOXES) return 0;
    return group_layout(n, k).total;
}

extern "C" int cpd_group_points_by_box(const float *points, int n, int c, const int32_t *box_idx, int k, const double *centre,
                                       float *out, int32_t *offsets, void *workspace, size_t workspace_bytes, cpd_stream_t st) {
    if (n < 0 || c < 3 || k < 0 || !offsets || !workspace || (k > 0 && !centre) || (n > 0 && (!points || !box_idx || !out)))
        return CPD_ERR_ARG;
    if (k > GROUP_MAX_BOXES) return CPD_ERR_UNSUPPORTED;
    const GroupLayout l = group_layout(n, k);
    if (workspace_bytes < l.total) return CPD_ERR_WORKSPACE;
    hipStream_t s = cpd_s(st);
    if (n == 0 || k == 0) {
        CPD_HIP_TRY(hipMemsetAsync(offsets, 0, (size_t)(k + 1) * 4, s));
        return CPD_OK;
    }
    const int nb = (int)(((long long)n + GROUP_TILE - 1) / GROUP_TILE);      // <= 2^20 for any int n
    const long long cells = (long long)nb * k;                               // <= 2^30 with k <= 1024
    uint32_t *counts = ws_at<uint32_t>(workspace, l.counts), *first = ws_at<uint32_t>(workspace, l.first);
    double *dcentre = ws_at<double>(workspace, l.centre);
    CPD_HIP_TRY(hipMemcpyAsync(dcentre, centre, (size_t)k * 24, hipMemcpyHostToDevice, s));   // (pageable source: see cpd_augment_scene)
    group_count_kernel<<<nb, 256, 0, s>>>(box_idx, n, k, nb, counts);
    int rc = cpd_check_launch();
    if (rc != CPD_OK) return rc;
    rc = device_scan(cells, CountFn{counts}, GroupStartFn{first, offsets, nb}, ws_at<uint32_t>(workspace, l.scan), offsets + k, -1, s);
    if (rc != CPD_OK) return rc;
    group_scatter_kernel<<<nb, 256, 0, s>>>(points, box_idx, n, c, k, nb, first, dcentre, out);
    return cpd_check_launch();
}
