// wbf.hip -- weighted box fusion of test-time-augmentation views (cpd_wbf_cluster): DetectionsMerger.compute_WBF
// (cpd/datasets/kitti/kitti_object_eval_python/merge_detections.py:110-181) and model_nms_utils.compute_WBF
// (cpd/models/model_utils/model_nms_utils.py:14-113).
//
// The clustering is serial in the boxes (every decision depends on the clusters so far, and in mean mode the cluster boxes move) and
// wide in the clusters; frames and classes are independent. So: one workgroup per segment, the boxes one at a time, lanes over the
// clusters, a block reduction for (max IoU, lowest index), one thread for the rule (wbf_rules.h), a barrier. Workgroups never talk to
// each other and every loop is bounded by the segment's count.
// Cluster state is a structure of arrays [WBF_NF][clusters]: the first CPD_WBF_LDS_CLUSTERS clusters of a segment in LDS (51200 B),
// the rest in the workspace at the segment's own rows (a segment of c boxes opens at most c clusters, and segments do not overlap).
#include "wbf_rules.h"

namespace {

struct WbfState {
    float *lds;      // [WBF_NF][CPD_WBF_LDS_CLUSTERS]
    float *spill;    // [WBF_NF][pitch], already offset to the segment's first row
    size_t pitch;
    __device__ __forceinline__ float &f(int field, int k) {
        return k < CPD_WBF_LDS_CLUSTERS ? lds[field * CPD_WBF_LDS_CLUSTERS + k] : spill[(size_t)field * pitch + (k - CPD_WBF_LDS_CLUSTERS)];
    }
};

__device__ __forceinline__ void better(float &v, int &k, float ov, int ok) {   // larger IoU; equal IoUs: the lower index (np.argmax)
    if (ov > v || (ov == v && ok < k)) {
        v = ov;
        k = ok;
    }
}

__global__ void __launch_bounds__(CPD_WBF_BLOCK)
wbf_kernel(const float *__restrict__ boxes, const float *__restrict__ scores, int n, const int32_t *__restrict__ seg_start,
           const int32_t *__restrict__ seg_count, const float *__restrict__ seg_thresh, const int32_t *__restrict__ seg_mode,
           float *__restrict__ out_boxes, float *__restrict__ out_scores, int32_t *__restrict__ out_count, int32_t *__restrict__ cluster_of,
           float *ws_state, int32_t *ws_next) {
    __shared__ float s_state[WBF_NF * CPD_WBF_LDS_CLUSTERS];
    __shared__ float s_v[CPD_WBF_BLOCK / 64];
    __shared__ int s_k[CPD_WBF_BLOCK / 64];
    __shared__ int s_clusters, s_single;
    const int seg = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int start = seg_start[seg], count = seg_count[seg];
    if (start < 0 || count < 0 || count > CPD_WBF_MAX_SEGMENT || (long long)start + count > n) {
        if (tid == 0) out_count[seg] = -1;
        return;
    }
    if (count == 0) {
        if (tid == 0) out_count[seg] = 0;
        return;
    }
    WbfSeg sg;
    sg.boxes = boxes + 7 * (size_t)start;
    sg.scores = scores + start;
    sg.next = ws_next + start;
    sg.cluster_of = cluster_of + start;
    sg.out_boxes = out_boxes + 7 * (size_t)start;
    sg.out_scores = out_scores + start;
    sg.count = count;
    sg.mode = wbf_mode(seg_mode[seg]);
    sg.thr = seg_thresh[2 * seg];
    sg.thr2 = seg_thresh[2 * seg + 1];
    WbfState st = {s_state, ws_state + start, (size_t)n};
    if (tid == 0) {
        s_clusters = 0;
        s_single = 0;
    }
    __syncthreads();
    for (int i = 0; i < count; ++i) {
        const int n_clusters = s_clusters;
        float box[7];
#pragma unroll
        for (int c = 0; c < 7; ++c) box[c] = sg.boxes[7 * (size_t)i + c];
        box[6] = wbf_heading(sg.mode, box[6]);
        BoxG A;
        box_setup(box, A);
        const float ra = 0.5f * sqrtf(box[3] * box[3] + box[4] * box[4]);
        float v = -1.f;
        int kbest = 0x7fffffff;
        for (int k = tid; k < n_clusters; k += CPD_WBF_BLOCK) better(v, kbest, wbf_iou(st, k, A, ra), k);
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const float ov = __shfl_xor(v, off, 64);
            const int ok = __shfl_xor(kbest, off, 64);
            better(v, kbest, ov, ok);
        }
        if (lane == 0) {
            s_v[wave] = v;
            s_k[wave] = kbest;
        }
        __syncthreads();
        if (tid == 0) {
#pragma unroll
            for (int w = 1; w < CPD_WBF_BLOCK / 64; ++w) better(v, kbest, s_v[w], s_k[w]);
            int nc = n_clusters, ns = s_single;
            wbf_apply(st, sg, i, box, sg.scores[i], v, kbest, nc, ns);
            s_clusters = nc;
            s_single = ns;
        }
        __syncthreads();
    }
    const int n_clusters = s_clusters, n_single = s_single;
    for (int k = tid; k < n_clusters; k += CPD_WBF_BLOCK) {
        float box[7], score;
        wbf_finish(st, sg, k, box, score);
        float *o = sg.out_boxes + 7 * (size_t)(n_single + k);
#pragma unroll
        for (int c = 0; c < 7; ++c) o[c] = box[c];
        sg.out_scores[n_single + k] = score;
    }
    if (tid == 0) out_count[seg] = n_single + n_clusters;
}

struct WbfLayout {
    size_t state, next, total;
    explicit WbfLayout(int n) {
        Carve c;
        state = c.take((size_t)WBF_NF * sizeof(float) * (size_t)(n > 0 ? n : 1));
        next = c.take(sizeof(int32_t) * (size_t)(n > 0 ? n : 1));
        total = c.o;
    }
};

// ---- the same rules on the host (cpd_wbf_cluster_cpu): one box after the other, a segment's clusters in one allocation ----
struct WbfHostState {
    float *a;
    size_t pitch;
    float &f(int field, int k) { return a[(size_t)field * pitch + k]; }
};

}  // namespace

extern "C" int cpd_wbf_cluster_cpu(const float *boxes, const float *scores, int n, const int32_t *seg_start, const int32_t *seg_count,
                                   const float *seg_thresh, const int32_t *seg_mode, int n_seg, float *out_boxes, float *out_scores,
                                   int32_t *out_count, int32_t *cluster_of) {
    if (n < 0 || n_seg < 0 || (n > 0 && (!boxes || !scores || !out_boxes || !out_scores || !cluster_of))) return CPD_ERR_ARG;
    if (n_seg == 0) return CPD_OK;
    if (!seg_start || !seg_count || !seg_thresh || !seg_mode || !out_count) return CPD_ERR_ARG;
    for (int seg = 0; seg < n_seg; ++seg) {
        const int start = seg_start[seg], count = seg_count[seg];
        if (start < 0 || count < 0 || count > CPD_WBF_MAX_SEGMENT || (long long)start + count > n) {
            out_count[seg] = -1;
            continue;
        }
        float *state = static_cast<float *>(malloc(sizeof(float) * WBF_NF * (size_t)(count + 1)));
        int32_t *next = static_cast<int32_t *>(malloc(sizeof(int32_t) * (size_t)(count + 1)));
        if (!state || !next) {
            free(state);
            free(next);
            return CPD_ERR_WORKSPACE;
        }
        WbfHostState st = {state, (size_t)count + 1};
        WbfSeg sg;
        sg.boxes = boxes + 7 * (size_t)start;
        sg.scores = scores + start;
        sg.next = next;
        sg.cluster_of = cluster_of + start;
        sg.out_boxes = out_boxes + 7 * (size_t)start;
        sg.out_scores = out_scores + start;
        sg.count = count;
        sg.mode = wbf_mode(seg_mode[seg]);
        sg.thr = seg_thresh[2 * seg];
        sg.thr2 = seg_thresh[2 * seg + 1];
        int n_clusters = 0, n_single = 0;
        for (int i = 0; i < count; ++i) {
            float box[7];
            for (int c = 0; c < 7; ++c) box[c] = sg.boxes[7 * (size_t)i + c];
            box[6] = wbf_heading(sg.mode, box[6]);
            BoxG A;
            box_setup(box, A);
            const float ra = 0.5f * sqrtf(box[3] * box[3] + box[4] * box[4]);
            float v = -1.f;
            int kbest = 0x7fffffff;
            for (int k = 0; k < n_clusters; ++k) {
                const float x = wbf_iou(st, k, A, ra);
                if (x > v) {
                    v = x;
                    kbest = k;
                }
            }
            wbf_apply(st, sg, i, box, sg.scores[i], v, kbest, n_clusters, n_single);
        }
        for (int k = 0; k < n_clusters; ++k) {
            float box[7], score;
            wbf_finish(st, sg, k, box, score);
            for (int c = 0; c < 7; ++c) sg.out_boxes[7 * (size_t)(n_single + k) + c] = box[c];
            sg.out_scores[n_single + k] = score;
        }
        out_count[seg] = n_single + n_clusters;
        free(state);
        free(next);
    }
    return CPD_OK;
}

extern "C" size_t cpd_wbf_workspace_bytes(int n) { return WbfLayout(n).total; }

extern "C" int cpd_wbf_cluster(const float *boxes, const float *scores, int n, const int32_t *seg_start, const int32_t *seg_count,
                               const float *seg_thresh, const int32_t *seg_mode, int n_seg, float *out_boxes, float *out_scores,
                               int32_t *out_count, int32_t *cluster_of, void *workspace, size_t workspace_bytes, cpd_stream_t stream) {
    if (n < 0 || n_seg < 0 || (n > 0 && (!boxes || !scores || !out_boxes || !out_scores || !cluster_of))) return CPD_ERR_ARG;
    if (n_seg == 0) return CPD_OK;
    if (!seg_start || !seg_count || !seg_thresh || !seg_mode || !out_count) return CPD_ERR_ARG;
    const WbfLayout lay(n);
    if (!workspace || workspace_bytes < lay.total) return CPD_ERR_WORKSPACE;
    wbf_kernel<<<n_seg, CPD_WBF_BLOCK, 0, cpd_s(stream)>>>(boxes, scores, n, seg_start, seg_count, seg_thresh, seg_mode, out_boxes, out_scores,
                                                          out_count, cluster_of, ws_at<float>(workspace, lay.state),
                                                          ws_at<int32_t>(workspace, lay.next));
    return cpd_check_launch();
}
