// cproto_refine.hip -- the second stage of CPD's C_PROTO refiner (cpd/unsupervised_core/c_proto_refine.py:332-475
// refine_box_size) on the SEGMENTS of cproto.hip, one segment = one (frame, box) pair:
//   1. cpd_refine_fit_size : the prototype size fit (l.410-436) on cpd_cproto_filter's new_box, between the filter and the score;
//   2. cpd_refine_orient_drift : correct_orientation (outline_utils.py:127-326) and density_guided_drift (l.41-92) on the chosen
//      clusters cpd_cproto_score leaves: box_drift = drift(box), box_orient = orient(box), box_orient_drift = drift(orient(box)).
// One 256-thread workgroup per segment re-reads the cluster's rows on every pass; the passes themselves are refine_dev.h's
// (shared with mfcf.hip): no float atomics, the same bits for any launch geometry.
// Built with -ffp-contract=off: no fused multiply-add anywhere in this file.
#include <math.h>

#include "common.h"
#include "refine_dev.h"   // the cluster passes, shared with mfcf.hip

namespace {

constexpr int RF_MAX_SEGMENTS = 1022;   // cproto.hip CP_MAX_SEGMENTS
constexpr int RF_MAX_CAP = 64;          // high-quality prototypes per class

// ---- 1. prototype size fit (c_proto_refine.py:410-436) ------------------------------------------------------------------------

struct FitArgs {
    double *new_box;            // [S][7], l and w of Vehicle rows overwritten
    const int32_t *seg_cls;     // [S] 0 Vehicle, 1 Pedestrian, 2 Cyclist
    const double *basic_whl;    // [S][3], a NaN row where the box's own id is no basic prototype
    const double *hq_whl;       // [3][cap][3]
    int32_t *fit_index;         // [S]
    int n_segments, cap;
    int hq_count[3];
    double predefined[9];
};

__global__ void __launch_bounds__(RF_THREADS) rf_fit_kernel(FitArgs a) {
    const int s = blockIdx.x * RF_THREADS + threadIdx.x;
    if (s >= a.n_segments) return;
    const int c = a.seg_cls[s];
    if (c < 0 || c > 2) {
        a.fit_index[s] = -1;
        return;
    }
    double *nb = a.new_box + (size_t)s * 7;
    const double *own = a.basic_whl + (size_t)s * 3;
    const int count = c == 0 ? a.hq_count[0] : c == 1 ? a.hq_count[1] : a.hq_count[2];
    double fl, fw;
    int idx;
    if (own[0] == own[0]) {                 // not NaN: the box's own basic prototype
        fl = own[0], fw = own[1], idx = -2;
    } else if (count == 0) {
        fl = c == 0 ? a.predefined[0] : c == 1 ? a.predefined[3] : a.predefined[6];
        fw = c == 0 ? a.predefined[1] : c == 1 ? a.predefined[4] : a.predefined[7];
        idx = -1;
    } else {                                // np.argmin(np.abs(proto_whl[:, 2] - h)): the first minimum
        const double *q = a.hq_whl + (size_t)c * a.cap * 3;
        const double h = nb[5];
        double best = fabs(q[2] - h);
        idx = 0;
        for (int k = 1; k < count; ++k) {
            const double d = fabs(q[3 * k + 2] - h);
            if (d < best) best = d, idx = k;
        }
        fl = q[3 * idx], fw = q[3 * idx + 1];
    }
    if (c == 0) nb[3] = fl, nb[4] = fw;
    a.fit_index[s] = idx;
}

// ---- 2. correct_orientation and density_guided_drift (outline_utils.py:127-326, 41-92) ----------------------------------------

struct RefineArgs {
    const float *xyz;           // [n_rows][3] the chosen clusters' rows (cpd_cproto_score's out_xyz)
    const int32_t *off;         // [S + 1]
    const int32_t *best_label;  // [S]
    const double *box;          // [S][7]
    const float *m;             // [S][8] rows 0 and 1 of the inverse box transform
    int n_segments, n_rows;
    double *out;                // [S][7]
    float *m_out;               // [S][8] (orientation only): the inverse rows of the re-oriented box
};

__device__ __forceinline__ Cluster rf_cluster(const RefineArgs &a, int s) {
    const int o0 = min(max(a.off[s], 0), a.n_rows), o1 = min(max(a.off[s + 1], o0), a.n_rows);
    Cluster c;
    c.xyz = a.xyz + 3 * (size_t)o0;
    c.n = c.count = a.best_label[s] >= 0 ? o1 - o0 : 0;
    return c;
}

__global__ void __launch_bounds__(RF_THREADS) rf_drift_kernel(RefineArgs a) {
    __shared__ double smd[16];
    __shared__ int smi[8];
    const int s = blockIdx.x;
    const Cluster c = rf_cluster(a, s);
    const double *b = a.box + (size_t)s * 7;
    double *out = a.out + (size_t)s * 7;
    if (c.n == 0) {
        if (threadIdx.x < 7) out[threadIdx.x] = b[threadIdx.x];
        return;
    }
    double m[8];
    for (int k = 0; k < 8; ++k) m[k] = a.m[(size_t)s * 8 + k];
    const Stats t = rf_stats(c, m, smd, smi);
    if (threadIdx.x == 0) rf_drift_box(b, t, c.n, out);
}

__global__ void __launch_bounds__(RF_THREADS) rf_orient_kernel(RefineArgs a) {
    __shared__ double smd[16];
    __shared__ int smi[8];
    __shared__ unsigned long long bkey[2 * RF_PARTS];
    __shared__ int brow[2 * RF_PARTS];
    const int s = blockIdx.x;
    const Cluster c = rf_cluster(a, s);
    const double *b = a.box + (size_t)s * 7;
    double *out = a.out + (size_t)s * 7;
    float *mo = a.m_out + (size_t)s * 8;
    if (c.n == 0) {
        if (threadIdx.x < 7) out[threadIdx.x] = b[threadIdx.x];
        if (threadIdx.x < 8) mo[threadIdx.x] = a.m[(size_t)s * 8 + threadIdx.x];
        return;
    }
    double m[8];
    for (int k = 0; k < 8; ++k) m[k] = a.m[(size_t)s * 8 + k];
    const Stats t = rf_stats(c, m, smd, smi);
    const Orient o = rf_orient(c, b, m, t, bkey, brow);
    if (threadIdx.x != 0) return;
    for (int k = 0; k < 6; ++k) out[k] = b[k];
    out[6] = o.yaw;
    if (!o.turned) {
        for (int k = 0; k < 8; ++k) mo[k] = a.m[(size_t)s * 8 + k];
        return;
    }
    // the closed-form inverse of the re-oriented box's float32 trans_mat, as the host forms the first one
    rf_inverse_rows(b[0], b[1], o.yaw, mo);
}

}  // namespace

extern "C" {

int cpd_refine_fit_size(double *new_box, const int32_t *seg_cls, const double *basic_whl, int n_segments, const double *hq_whl,
                        const int32_t *hq_count, int cap, const double *predefined, int32_t *fit_index, cpd_stream_t stream) {
    if (n_segments < 0 || n_segments > RF_MAX_SEGMENTS || !hq_count || !predefined) return CPD_ERR_ARG;
    if (cap < 1 || cap > RF_MAX_CAP) return CPD_ERR_UNSUPPORTED;
    for (int c = 0; c < 3; ++c)
        if (hq_count[c] < 0 || hq_count[c] > cap) return CPD_ERR_ARG;
    if (n_segments > 0 && (!new_box || !seg_cls || !basic_whl || !fit_index)) return CPD_ERR_ARG;
    if ((hq_count[0] || hq_count[1] || hq_count[2]) && !hq_whl) return CPD_ERR_ARG;
    if (n_segments == 0) return CPD_OK;
    FitArgs a;
    a.new_box = new_box, a.seg_cls = seg_cls, a.basic_whl = basic_whl, a.hq_whl = hq_whl, a.fit_index = fit_index;
    a.n_segments = n_segments, a.cap = cap;
    for (int c = 0; c < 3; ++c) a.hq_count[c] = hq_count[c];
    for (int k = 0; k < 9; ++k) a.predefined[k] = predefined[k];
    rf_fit_kernel<<<cpd_div_up(n_segments, RF_THREADS), RF_THREADS, 0, cpd_s(stream)>>>(a);
    return cpd_check_launch();
}

size_t cpd_refine_orient_drift_workspace_bytes(int n_segments) {
    if (n_segments < 0) return 0;
    return cpd_align((size_t)(n_segments > 0 ? n_segments : 1) * 8 * sizeof(float));
}

int cpd_refine_orient_drift(const float *out_xyz, const int32_t *out_off, const int32_t *best_label, const double *new_box,
                            const float *m, int n_segments, int n_rows, double *box_drift, double *box_orient_drift,
                            double *box_orient, void *workspace, size_t workspace_bytes, cpd_stream_t stream) {
    if (n_segments < 0 || n_segments > RF_MAX_SEGMENTS || n_rows < 0) return CPD_ERR_ARG;
    if (n_segments > 0 && (!out_off || !best_label || !new_box || !m || !box_drift || !box_orient_drift || !box_orient))
        return CPD_ERR_ARG;
    if (n_rows > 0 && !out_xyz) return CPD_ERR_ARG;
    if (!workspace || workspace_bytes < cpd_refine_orient_drift_workspace_bytes(n_segments)) return CPD_ERR_WORKSPACE;
    if (n_segments == 0) return CPD_OK;
    hipStream_t st = cpd_s(stream);
    RefineArgs a;
    a.xyz = out_xyz, a.off = out_off, a.best_label = best_label, a.box = new_box, a.m = m, a.n_segments = n_segments;
    a.n_rows = n_rows, a.out = box_drift, a.m_out = nullptr;
    rf_drift_kernel<<<n_segments, RF_THREADS, 0, st>>>(a);
    a.out = box_orient, a.m_out = static_cast<float *>(workspace);
    rf_orient_kernel<<<n_segments, RF_THREADS, 0, st>>>(a);
    a.box = box_orient, a.m = static_cast<const float *>(workspace), a.out = box_orient_drift, a.m_out = nullptr;
    rf_drift_kernel<<<n_segments, RF_THREADS, 0, st>>>(a);
    return cpd_check_launch();
}

}  // extern "C"
