// wbf_rules.h -- the serial half of weighted box fusion (wbf.hip): heading folds, the join / open / emit / drop rules, the cluster
// updates and the output expressions of DetectionsMerger.compute_WBF (cpd/datasets/kitti/kitti_object_eval_python/
// merge_detections.py:110-181) and model_nms_utils.compute_WBF (cpd/models/model_utils/model_nms_utils.py:5-113), op by op in the
// reference's number formats (numpy >= 2 scalar rules: a float32 scalar stays float32 against a Python number). __host__ __device__
// like box_geom.h, and written against a state accessor `St` (float &f(field, cluster)): the kernel's keeps a cluster in LDS or in
// the workspace, cpd_wbf_cluster_cpu's (the host build of the same text, which the CPU tests hold to the golden) in host memory. Compile WITHOUT fp contraction.
#pragma once
#include "box_geom.h"

#define WBF_HD __host__ __device__ __forceinline__

// per-cluster fields (structure of arrays: lanes read one field of consecutive clusters)
enum {
    WF_BOX = 0,      // 0..6 the cluster's box (mean mode: moves with every join; heading: the first member's)
    WF_CS = 7, WF_SN = 8, WF_NCS = 9, WF_NSN = 10,
    WF_CORN = 11,    // 11..18 corners x0 y0 .. x3 y3 (box_setup)
    WF_RAD = 19,     // half diagonal (centre-distance pre-test)
    WF_SSUM = 20,    // float32 sum of the member scores in joining order
    WF_SMAX = 21,
    WF_COUNT = 22, WF_HEAD = 23, WF_TAIL = 24,   // int32 bit patterns: members, first / last member (segment-local box index)
    WBF_NF = 25
};
enum { WBF_DROPPED = -1, WBF_SINGLE = -2 };
enum { WBF_DO_OPEN = 0, WBF_DO_JOIN = 1, WBF_DO_EMIT = 2, WBF_DO_DROP = 3 };

struct WbfSeg {
    const float *boxes;    // the segment's first row
    const float *scores;
    int32_t *next;         // [count] member chains
    int32_t *cluster_of;   // [count]
    float *out_boxes;      // the segment's first output row
    float *out_scores;
    int count, mode;
    float thr, thr2;
};

// correctly rounded float32 quotient whatever the compiler makes of a float division (53 >= 2 * 24 + 2 bits)
WBF_HD float wbf_div(float x, float y) { return (float)((double)x / (double)y); }

// common_utils.limit_period(val, 0.5, 2 pi) in torch float32 (common_utils.py:17-20)
WBF_HD float wbf_limit_period(float v) {
    const float period = 6.283185307179586f;
    return v - floorf(wbf_div(v, period) + 0.5f) * period;
}
// model_nms_utils.limit (l.5-12) on one float32: numpy's remainder (fmod, moved to the divisor's sign), then the two folds
WBF_HD float wbf_limit(float a) {
    const float two_pi = 6.283185307179586f, pi = 3.141592653589793f;
    float m = fmodf(a, two_pi);
    if (m != 0.f) {
        if (m < 0.f) m = m + two_pi;
    } else {
        m = 0.f;
    }
    if (m > pi) m = m - two_pi;
    if (m < -pi) m = m + two_pi;
    return m;
}
// the mode word with unknown bits dropped; CPD_WBF_NO_RETAIN means something in the model variant only
WBF_HD int wbf_mode(int m) {
    m &= CPD_WBF_MAX | CPD_WBF_MODEL | CPD_WBF_NO_RETAIN;
    return (m & CPD_WBF_MODEL) ? m : (m & CPD_WBF_MAX);
}
WBF_HD float wbf_heading(int mode, float h) { return (mode & CPD_WBF_MODEL) ? wbf_limit(h) : wbf_limit_period(h); }

// the int32 fields travel as bit patterns of the float words
template <class St>
WBF_HD int wbf_get_int(St &st, int field, int k) {
    const float f = st.f(field, k);
    int v;
    __builtin_memcpy(&v, &f, sizeof(v));
    return v;
}
template <class St>
WBF_HD void wbf_set_int(St &st, int field, int k, int v) {
    float f;
    __builtin_memcpy(&f, &v, sizeof(f));
    st.f(field, k) = f;
}

template <class St>
WBF_HD void wbf_store_geom(St &st, int k, const float *box) {
    BoxG g;
    box_setup(box, g);
#pragma unroll
    for (int c = 0; c < 7; ++c) st.f(WF_BOX + c, k) = g.b[c];
    st.f(WF_CS, k) = g.cs;
    st.f(WF_SN, k) = g.sn;
    st.f(WF_NCS, k) = g.ncs;
    st.f(WF_NSN, k) = g.nsn;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        st.f(WF_CORN + 2 * c, k) = g.c[c].x;
        st.f(WF_CORN + 2 * c + 1, k) = g.c[c].y;
    }
    st.f(WF_RAD, k) = 0.5f * sqrtf(box[3] * box[3] + box[4] * box[4]);
}
template <class St>
WBF_HD void wbf_load_geom(St &st, int k, BoxG &g) {
#pragma unroll
    for (int c = 0; c < 7; ++c) g.b[c] = st.f(WF_BOX + c, k);
    g.cs = st.f(WF_CS, k);
    g.sn = st.f(WF_SN, k);
    g.ncs = st.f(WF_NCS, k);
    g.nsn = st.f(WF_NSN, k);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        g.c[c].x = st.f(WF_CORN + 2 * c, k);
        g.c[c].y = st.f(WF_CORN + 2 * c + 1, k);
    }
    g.c[4] = g.c[0];
}

// IoU of box A (half diagonal ra) with cluster k. Boxes whose centres lie further apart than both half diagonals plus a slack that
// covers the corner test's 1e-2 margin share no crossing and no corner: the reference's overlap is exactly 0 there.
template <class St>
WBF_HD float wbf_iou(St &st, int k, const BoxG &A, float ra) {
    const float dx = st.f(WF_BOX + 0, k) - A.b[0], dy = st.f(WF_BOX + 1, k) - A.b[1];
    const float reach = ra + st.f(WF_RAD, k) + 0.1f;
    if (dx * dx + dy * dy > reach * reach) return 0.f;
    BoxG B;
    wbf_load_geom(st, k, B);
    return iou_bev_g(A, B);
}

// model_nms_utils.py:58-74 in order; merge_detections.py:144 for the evaluation-side variant
WBF_HD int wbf_decide(int mode, float v, float score, float thr, float thr2) {
    if (!(mode & CPD_WBF_MODEL)) return v > thr ? WBF_DO_JOIN : WBF_DO_OPEN;
    const bool retain = !(mode & CPD_WBF_NO_RETAIN);
    if (v >= thr) return WBF_DO_JOIN;
    if (thr2 <= v && v < thr && score > 0.4f && retain) return WBF_DO_EMIT;
    if (0.03f <= v && v < thr2 && retain) return WBF_DO_DROP;
    if (!retain && 0.03f <= v && v < thr) return WBF_DO_DROP;
    return WBF_DO_OPEN;
}

// One box's turn, by ONE thread: `box` with its heading already folded, `v` / `kbest` the largest IoU against the n_clusters clusters
// so far and the lowest cluster index that attains it (ignored for the first box).
template <class St>
WBF_HD void wbf_apply(St &st, const WbfSeg &sg, int i, const float *box, float score, float v, int kbest, int &n_clusters, int &n_single) {
    int what = n_clusters == 0 ? WBF_DO_OPEN : wbf_decide(sg.mode, v, score, sg.thr, sg.thr2);
    if (what == WBF_DO_JOIN && (unsigned)kbest >= (unsigned)n_clusters) what = WBF_DO_OPEN;   // (every IoU NaN under a negative threshold)
    if (what == WBF_DO_OPEN) {
        const int k = n_clusters++;
        wbf_store_geom(st, k, box);
        st.f(WF_SSUM, k) = score;
        st.f(WF_SMAX, k) = score;
        wbf_set_int(st, WF_COUNT, k, 1);
        wbf_set_int(st, WF_HEAD, k, i);
        wbf_set_int(st, WF_TAIL, k, i);
        sg.next[i] = -1;
        sg.cluster_of[i] = k;
        return;
    }
    if (what == WBF_DO_EMIT) {                                   // l.62-64: out on its own, ahead of every cluster
        float *o = sg.out_boxes + 7 * (size_t)n_single;
#pragma unroll
        for (int c = 0; c < 7; ++c) o[c] = box[c];
        sg.out_scores[n_single] = 0.4f + 0.2f * wbf_div(score - 0.4f, 0.6f);
        ++n_single;
        sg.cluster_of[i] = WBF_SINGLE;
        return;
    }
    if (what == WBF_DO_DROP) {
        sg.cluster_of[i] = WBF_DROPPED;
        return;
    }
    const int k = kbest;
    sg.next[wbf_get_int(st, WF_TAIL, k)] = i;
    sg.next[i] = -1;
    wbf_set_int(st, WF_TAIL, k, i);
    wbf_set_int(st, WF_COUNT, k, wbf_get_int(st, WF_COUNT, k) + 1);
    const float ssum = st.f(WF_SSUM, k) + score;
    st.f(WF_SSUM, k) = ssum;
    if (score > st.f(WF_SMAX, k)) st.f(WF_SMAX, k) = score;
    sg.cluster_of[i] = k;
    if (sg.mode != 0) return;                                    // max / model: the cluster's box stays its first member's
    // merge_detections.py:148-157. The list's first element is the merged row itself, so the sum starts from the box as merged so far.
    const int head = wbf_get_int(st, WF_HEAD, k);
    const float s0 = sg.scores[head];
    double acc[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        acc[c] = 0.0;
        acc[c] += (double)(st.f(WF_BOX + c, k) * s0);
    }
    int j = sg.next[head];
    for (int guard = 0; j >= 0 && guard < sg.count; ++guard) {
        const float sj = sg.scores[j];
        const float *row = sg.boxes + 7 * (size_t)j;
#pragma unroll
        for (int c = 0; c < 6; ++c) acc[c] += (double)(row[c] * sj);
        j = sg.next[j];
    }
    float nb[7];
#pragma unroll
    for (int c = 0; c < 6; ++c) nb[c] = (float)(acc[c] / (double)ssum);
    nb[6] = st.f(WF_BOX + 6, k);
    wbf_store_geom(st, k, nb);
}

// ---- the model variant's heading mean (model_nms_utils.py:92-99) ----
// the residuals of a cluster's members that pass |res| < 1.5, in joining order
struct WbfResiduals {
    const WbfSeg *sg;
    float h0;
    int j, left;
    WBF_HD bool advance(float &r) {                              // the next residual of the chain, filtered or not
        if (j < 0 || left <= 0) return false;
        const float a = wbf_limit(wbf_limit(sg->boxes[7 * (size_t)j + 6]));   // l.28 on the rows, l.93 on the list
        r = wbf_limit(a - h0);
        j = sg->next[j];
        --left;
        return true;
    }
    WBF_HD float nextv() {
        float r = 0.f;
        while (advance(r))
            if (fabsf(r) < 1.5f) return r;
        return 0.f;
    }
};
// ndarray.sum of `n` float32 values taken from `it` in order: numpy's pairwise sum (eight running sums per block of up to 128
// values; beyond, halves split at a multiple of eight), with the recursion unrolled onto a small stack.
template <class It>
WBF_HD float wbf_np_block_sum(It &it, int n) {
    if (n < 8) {
        float s = 0.f;
        for (int i = 0; i < n; ++i) s = i == 0 ? it.nextv() : s + it.nextv();
        return s;
    }
    float r[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) r[q] = it.nextv();
    int i = 8;
    for (; i < n - (n % 8); i += 8) {
#pragma unroll
        for (int q = 0; q < 8; ++q) r[q] = r[q] + it.nextv();
    }
    float s = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) s = s + it.nextv();
    return s;
}
template <class It>
WBF_HD float wbf_np_sum(It &it, int n) {
    int size[20], phase[20];
    float left[20];
    int sp = 0;
    size[0] = n;
    phase[0] = 0;
    float ret = 0.f;
    while (sp >= 0) {
        const int m = size[sp];
        if (m <= 128) {
            ret = wbf_np_block_sum(it, m);
            --sp;
            continue;
        }
        int half = m / 2;
        half -= half % 8;
        if (phase[sp] == 0) {
            phase[sp] = 1;
            size[sp + 1] = half;
            phase[sp + 1] = 0;
            ++sp;
        } else if (phase[sp] == 1) {
            left[sp] = ret;
            phase[sp] = 2;
            size[sp + 1] = m - half;
            phase[sp + 1] = 0;
            ++sp;
        } else {
            ret = left[sp] + ret;
            --sp;
        }
    }
    return ret;
}

// Output row of cluster k (by any one thread; clusters are independent here): box [7] and score.
template <class St>
WBF_HD void wbf_finish(St &st, const WbfSeg &sg, int k, float *box, float &score) {
#pragma unroll
    for (int c = 0; c < 7; ++c) box[c] = st.f(WF_BOX + c, k);
    const int count = wbf_get_int(st, WF_COUNT, k);
    if (sg.mode & CPD_WBF_MAX) {
        score = st.f(WF_SMAX, k);
        return;
    }
    score = wbf_div(st.f(WF_SSUM, k), (float)count);             // l.169-174 / l.85-88
    if (!(sg.mode & CPD_WBF_MODEL)) return;
    // model_nms_utils.py:79-99: unweighted float64 mean of the members' [0:6], heading = the first heading + mean residual
    const int head = wbf_get_int(st, WF_HEAD, k);
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    int j = head;
    for (int guard = 0; j >= 0 && guard < sg.count; ++guard) {
        const float *row = sg.boxes + 7 * (size_t)j;
#pragma unroll
        for (int c = 0; c < 6; ++c) acc[c] += (double)row[c];
        j = sg.next[j];
    }
#pragma unroll
    for (int c = 0; c < 6; ++c) box[c] = (float)(acc[c] / (double)count);
    WbfResiduals it = {&sg, box[6], head, count};
    int m = 0;
    float r;
    while (it.advance(r)) m += fabsf(r) < 1.5f ? 1 : 0;
    WbfResiduals it2 = {&sg, box[6], head, count};
    const float sum = wbf_np_sum(it2, m);
    box[6] = box[6] + wbf_div(sum, (float)m);                    // (no residual left: 0 / 0, numpy's nan)
}
