// rcnn_loss.hip -- RoIHeadTemplate.get_loss of the anchor-head VoxelRCNN (cpd/models/roi_heads/roi_head_template.py:148-267) fused
// with its gradient: binary cross entropy on sigmoid(rcnn_cls), WeightedSmoothL1Loss on the ResidualCoder targets of the canonical
// ground truth, the corner regularisation (loss_utils.py:210-233) and bbloss.bb_loss (bbloss.py:4-48).
//
// One workgroup of 256 lanes (four waves) does the whole loss in one launch, with no workspace and no host read-back:
//   1. integer counts of the valid (label >= 0) and foreground (reg_valid_mask > 0) rows -- the three normalisers;
//   2. every lane walks rows tid, tid + 256, ...: the row's loss terms (accumulated in double) and d(total)/d(rcnn_cls, rcnn_reg);
//   3. a fixed-order tree over the lanes' partials -> losses[6].
// No atomics anywhere: the sums run in the same order on every call, so two calls agree bit for bit.
// The arithmetic follows torch's operation by operation (forward formulas and autograd's derivative rules: BCE's -100 clamp on
// the logs and the 1e-12 floor of its backward, half / half gradients at min / max ties, zero gradient of abs at 0, clamp_min
// passing the gradient at the bound, torch.remainder for `%`). Accurate sinf / cosf / expf / logf, no fast-math forms.
// The second kernel, rcnn_proto_loss_kernel (further down), is VoxelRCNNProtoHead.get_loss -- the same per-row blocks on two branches
// plus proto_loss's bb_loss and cosine-similarity terms -- in the same shape.
#include "common.h"

namespace {

constexpr int RL_THREADS = 256;
constexpr float RL_PI = 3.14159265358979323846f;          // float32(np.pi), what torch adds / compares in float32
constexpr float RL_TWO_PI = 6.28318530717958647692f;      // float32(2 * np.pi)

struct RlParams {
    const float *cls, *reg, *rois, *gt, *gt_src, *mask, *labels;
    int n, ld_gt, ld_src, corner_reg;
    float cw[7], cls_weight, reg_weight, corner_weight;
    float *d_cls, *d_reg, *losses;
};

__device__ __forceinline__ float sgnf(float x) { return x > 0.f ? 1.f : (x < 0.f ? -1.f : 0.f); }

// torch.minimum / torch.maximum backward: the share of the gradient that goes to `a` (1, 0, or 1/2 at a tie)
__device__ __forceinline__ float min_share(float a, float b) { return a < b ? 1.f : (a == b ? 0.5f : 0.f); }
__device__ __forceinline__ float max_share(float a, float b) { return a > b ? 1.f : (a == b ? 0.5f : 0.f); }

// torch.remainder(x, 2 pi) for float32: fmod, plus the divisor when the remainder's sign differs from the divisor's
__device__ __forceinline__ float remainder_2pi(float x) {
    const float m = fmodf(x, RL_TWO_PI);
    return m < 0.f ? m + RL_TWO_PI : m;
}
// bbloss.limit: x % 2pi, then the part above pi moved down by 2pi (the `< -pi` branch cannot fire after a remainder by +2pi).
// d limit / dx = 1 everywhere (remainder and the masked shifts pass the gradient through).
__device__ __forceinline__ float limit_angle(float x) {
    float a = remainder_2pi(x);
    if (a > RL_PI) a = a - RL_TWO_PI;
    if (a < -RL_PI) a = a + RL_TWO_PI;
    return a;
}

// one axis of bbloss.compute_iou: iou = clamp_min(min(hi) - max(lo), 0) / clamp_min(max(hi) - min(lo), 0); returns iou and
// d iou / d (pred centre, pred size) given the upstream gradient g
__device__ __forceinline__ float axis_iou(float x, float w, float y, float l, float g, float *gx, float *gw) {
    const float hi1 = x + w * 0.5f, lo1 = x - w * 0.5f, hi2 = y + l * 0.5f, lo2 = y - l * 0.5f;
    const float mn = fminf(hi1, hi2), mx = fmaxf(lo1, lo2);
    const float ov = mn - mx, inter = fmaxf(ov, 0.f);
    const float Mx = fmaxf(hi1, hi2), Mn = fminf(lo1, lo2);
    const float sp = Mx - Mn, span = fmaxf(sp, 0.f);
    const float iou = inter / span;
    const float g_inter = g / span;
    const float g_span = -g * inter / (span * span);
    const float g_ov = ov >= 0.f ? g_inter : 0.f;          // clamp_min: gradient where x >= bound
    const float g_sp = sp >= 0.f ? g_span : 0.f;
    const float g_hi1 = g_ov * min_share(hi1, hi2) + g_sp * max_share(hi1, hi2);
    const float g_lo1 = -g_ov * max_share(lo1, lo2) - g_sp * min_share(lo1, lo2);
    *gx = g_hi1 + g_lo1;
    *gw = (g_hi1 - g_lo1) * 0.5f;
    return iou;
}

__device__ __forceinline__ float rl_box_corner(int k, int axis) {     // box_utils.boxes_to_corners_3d template / 2
    const float t[8][3] = {{1, 1, -1}, {1, -1, -1}, {-1, -1, -1}, {-1, 1, -1}, {1, 1, 1}, {1, -1, 1}, {-1, -1, 1}, {-1, 1, 1}};
    return t[k][axis] * 0.5f;
}

// the 8 corners of a box (x, y, z, dx, dy, dz, heading): local = size * template, rotated about z by the heading, plus the centre
__device__ __forceinline__ void corners(const float b[7], float c, float s, float out[8][3]) {
    for (int k = 0; k < 8; ++k) {
        const float lx = b[3] * rl_box_corner(k, 0), ly = b[4] * rl_box_corner(k, 1), lz = b[5] * rl_box_corner(k, 2);
        out[k][0] = lx * c - ly * s + b[0];
        out[k][1] = lx * s + ly * c + b[1];
        out[k][2] = lz + b[2];
    }
}

// ---- the per-row blocks, shared by rcnn_loss_kernel and rcnn_proto_loss_kernel -------------------------------------------------
// classification: F.binary_cross_entropy(sigmoid(x), y) of one valid row; *g_cls = d / dx with the upstream gradient `scale`
__device__ __forceinline__ float bce_row(float x, float y, float scale, float *g_cls) {
    const float pr = 1.f / (1.f + expf(-x));
    const float bce = (y - 1.f) * fmaxf(log1pf(-pr), -100.f) - y * fmaxf(logf(pr), -100.f);
    const float g = scale * (pr - y) / fmaxf((1.f - pr) * pr, 1e-12f);    // binary_cross_entropy_backward
    *g_cls = g * (1.f - pr) * pr;                                         // sigmoid_backward
    return bce;
}

// the canonical gt as the losses read it: encode_torch clamps its sizes IN PLACE (clamp_min 1e-5), so bb_loss sees them clamped too
__device__ __forceinline__ void clamped_gt(const float *gt, float g7[7]) {
    g7[0] = gt[0]; g7[1] = gt[1]; g7[2] = gt[2];
    g7[3] = fmaxf(gt[3], 1e-5f); g7[4] = fmaxf(gt[4], 1e-5f); g7[5] = fmaxf(gt[5], 1e-5f);
    g7[6] = gt[6];
}

// regression: smooth-L1 (beta 1/9, code weights) against ResidualCoder.encode of the canonical gt, the RoI with xyz and heading zeroed
// as the anchor (sizes clamp_min 1e-5). Adds the 7 terms to *l_reg and, with the upstream gradient reg_scale, d / d r to gr.
__device__ __forceinline__ void reg_row(const float *r, const float *roi, const float g7[7], const float cw[7], float reg_scale,
                                        double *l_reg, float gr[7]) {
    const float beta = 1.0f / 9.0f;
    const float adx = fmaxf(roi[3], 1e-5f), ady = fmaxf(roi[4], 1e-5f), adz = fmaxf(roi[5], 1e-5f);
    const float adiag = sqrtf(adx * adx + ady * ady);
    const float t[7] = {g7[0] / adiag, g7[1] / adiag, g7[2] / adz, logf(g7[3] / adx), logf(g7[4] / ady), logf(g7[5] / adz), g7[6]};
    for (int k = 0; k < 7; ++k) {
        const bool nan_t = t[k] != t[k];                 // NaN target -> replaced by the prediction: zero diff, zero gradient
        const float diff = (nan_t ? 0.f : r[k] - t[k]) * cw[k];
        const float n = fabsf(diff);
        *l_reg += (double)(n < beta ? 0.5f * (n * n) / beta : n - 0.5f * beta);
        const float gn = n < beta ? reg_scale / beta * 0.5f * 2.f * n : reg_scale;
        gr[k] += nan_t ? 0.f : gn * sgnf(diff) * cw[k];
    }
}

// ResidualCoder.decode of r against the RoI with xyz and heading zeroed (sizes NOT clamped: decode_torch takes them as they are)
struct RlDecoded { float pb[7], diag, e3, e4, e5; };
__device__ __forceinline__ RlDecoded decode_local(const float *r, const float *roi) {
    RlDecoded d;
    d.diag = sqrtf(roi[3] * roi[3] + roi[4] * roi[4]);
    d.e3 = expf(r[3]); d.e4 = expf(r[4]); d.e5 = expf(r[5]);
    d.pb[0] = r[0] * d.diag; d.pb[1] = r[1] * d.diag; d.pb[2] = r[2] * roi[5];
    d.pb[3] = d.e3 * roi[3]; d.pb[4] = d.e4 * roi[4]; d.pb[5] = d.e5 * roi[5];
    d.pb[6] = r[6];
    return d;
}

// bbloss.bb_loss(pb, tg) of one row; adds d / d r (through the decode `d`) to gr with the upstream gradient g_up on the row's
// (1 - iou + angle + dist2) term, i.e. g_up already holds the 1.5
__device__ __forceinline__ float bb_row(const RlDecoded &d, const float *roi, const float tg[7], float g_up, float gr[7]) {
    const float *pb = d.pb;
    // forward: the three axis IoUs first (their gradients need the others' values)
    float gdum0, gdum1;
    const float ix = axis_iou(pb[0], pb[3], tg[0], tg[3], 0.f, &gdum0, &gdum1);
    const float iy = axis_iou(pb[1], pb[4], tg[1], tg[4], 0.f, &gdum0, &gdum1);
    const float iz = axis_iou(pb[2], pb[5], tg[2], tg[5], 0.f, &gdum0, &gdum1);
    const float da = limit_angle(pb[6]) - limit_angle(tg[6]);
    const float sda = sinf(da);
    const float ia = 1.f - fabsf(sda);
    const float iou = ix * iy * iz * ia;
    const float de = pb[6] - tg[6];
    const float cde = cosf(de);
    const float af = 1.25f * (1.f - fabsf(cde));
    const float c0 = tg[0] - pb[0], c1 = tg[1] - pb[1], c2 = tg[2] - pb[2];
    const float d2 = c0 * c0 + c1 * c1 + c2 * c2;
    // backward
    const float g_iou = -g_up;
    float gpb[7];
    axis_iou(pb[0], pb[3], tg[0], tg[3], g_iou * ia * iz * iy, &gpb[0], &gpb[3]);
    axis_iou(pb[1], pb[4], tg[1], tg[4], g_iou * ia * iz * ix, &gpb[1], &gpb[4]);
    axis_iou(pb[2], pb[5], tg[2], tg[5], g_iou * ia * iy * ix, &gpb[2], &gpb[5]);
    const float g_ia = g_iou * iz * iy * ix;
    gpb[6] = -g_ia * sgnf(sda) * cosf(da)                           // d(1 - |sin(da)|)
             + 1.25f * g_up * sgnf(cde) * sinf(de);                   // d 1.25 (1 - |cos(de)|)
    gpb[0] += -2.f * c0 * g_up;                                       // d (g - p)^2 / dp
    gpb[1] += -2.f * c1 * g_up;
    gpb[2] += -2.f * c2 * g_up;
    gr[0] += gpb[0] * d.diag; gr[1] += gpb[1] * d.diag; gr[2] += gpb[2] * roi[5];
    gr[3] += gpb[3] * roi[3] * d.e3; gr[4] += gpb[4] * roi[4] * d.e4; gr[5] += gpb[5] * roi[5] * d.e5;
    gr[6] += gpb[6];
    return (1.f - iou + af + d2) * 1.5f;
}

// corner regularisation of one row: decode against the RoI with only xyz zeroed (heading kept), rotate by the RoI heading, add the
// RoI centre; smooth-L1 (beta 1) of the corner distances to the source gt or its pi-flipped copy, whichever is nearer, mean over the
// 8 corners. corner_scale = the upstream gradient on one corner's term; adds d / d r to gr.
__device__ __forceinline__ float corner_row(const float *r, const RlDecoded &d, const float *roi, const float *gs, float corner_scale,
                                            float gr[7]) {
    const float dx = roi[3], dy = roi[4], dz = roi[5];
    const float rc = cosf(roi[6]), rs = sinf(roi[6]);
    const float lx = r[0] * d.diag, ly = r[1] * d.diag;
    float P[7] = {lx * rc - ly * rs + roi[0], lx * rs + ly * rc + roi[1], r[2] * dz + roi[2], d.e3 * dx, d.e4 * dy, d.e5 * dz,
                  r[6] + roi[6]};
    const float G[7] = {gs[0], gs[1], gs[2], gs[3], gs[4], gs[5], gs[6]};
    const float F[7] = {gs[0], gs[1], gs[2], gs[3], gs[4], gs[5], gs[6] + RL_PI};
    const float ph_c = cosf(P[6]), ph_s = sinf(P[6]);
    float pc[8][3], gc[8][3], fc[8][3];
    corners(P, ph_c, ph_s, pc);
    corners(G, cosf(G[6]), sinf(G[6]), gc);
    corners(F, cosf(F[6]), sinf(F[6]), fc);
    float gP[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float row = 0.f;
    for (int k = 0; k < 8; ++k) {
        const float a0 = pc[k][0] - gc[k][0], a1 = pc[k][1] - gc[k][1], a2 = pc[k][2] - gc[k][2];
        const float b0 = pc[k][0] - fc[k][0], b1 = pc[k][1] - fc[k][1], b2 = pc[k][2] - fc[k][2];
        const float da_ = sqrtf(a0 * a0 + a1 * a1 + a2 * a2), db_ = sqrtf(b0 * b0 + b1 * b1 + b2 * b2);
        const float m = fminf(da_, db_);
        row += m < 1.f ? 0.5f * (m * m) : m - 0.5f;
        const float gm = corner_scale * (m < 1.f ? m : 1.f) * sgnf(m);
        const float ga = gm * min_share(da_, db_), gb = gm * min_share(db_, da_);
        const float qa = da_ > 0.f ? ga / da_ : 0.f, qb = db_ > 0.f ? gb / db_ : 0.f;   // norm backward (0 at a zero norm)
        const float gcx = qa * a0 + qb * b0, gcy = qa * a1 + qb * b1, gcz = qa * a2 + qb * b2;
        // corner k = R(heading) (size * template) + centre
        const float tx = rl_box_corner(k, 0), ty = rl_box_corner(k, 1), tz = rl_box_corner(k, 2);
        const float clx = P[3] * tx, cly = P[4] * ty;
        gP[0] += gcx; gP[1] += gcy; gP[2] += gcz;
        gP[3] += (gcx * ph_c + gcy * ph_s) * tx;
        gP[4] += (-gcx * ph_s + gcy * ph_c) * ty;
        gP[5] += gcz * tz;
        gP[6] += gcx * (-clx * ph_s - cly * ph_c) + gcy * (clx * ph_c - cly * ph_s);
    }
    // back through the rotation by the RoI heading (a constant) and the decode
    const float glx = gP[0] * rc + gP[1] * rs, gly = -gP[0] * rs + gP[1] * rc;
    gr[0] += glx * d.diag; gr[1] += gly * d.diag; gr[2] += gP[2] * dz;
    gr[3] += gP[3] * dx * d.e3; gr[4] += gP[4] * dy * d.e4; gr[5] += gP[5] * dz * d.e5;
    gr[6] += gP[6];
    return row / 8.f;
}

__global__ void __launch_bounds__(RL_THREADS) rcnn_loss_kernel(RlParams p) {
    __shared__ int sc[2][RL_THREADS];
    __shared__ double sl[4][RL_THREADS];
    const int tid = threadIdx.x;
    // ---- 1. normalisers (integer sums: exact)
    int n_valid = 0, n_fg = 0;
    for (int i = tid; i < p.n; i += RL_THREADS) {
        n_valid += p.labels[i] >= 0.f ? 1 : 0;
        n_fg += p.mask[i] > 0.f ? 1 : 0;
    }
    sc[0][tid] = n_valid; sc[1][tid] = n_fg;
    __syncthreads();
    for (int s = RL_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) { sc[0][tid] += sc[0][tid + s]; sc[1][tid] += sc[1][tid + s]; }
        __syncthreads();
    }
    const int valid = sc[0][0], fg = sc[1][0];
    const float cls_scale = p.cls_weight / fmaxf((float)valid, 1.f);             // torch.clamp(valid.sum(), min=1.0)
    const float reg_scale = p.reg_weight / (float)(fg > 1 ? fg : 1);             // / max(fg_sum, 1)
    const bool corner_on = p.corner_reg && fg > 0;
    const float corner_scale = corner_on ? p.corner_weight / (float)fg / 8.f : 0.f;   // mean over 8 corners, mean over fg rows
    const float bb_scale = 1.5f / (float)(fg + 1);                               // (1 - iou + ...) * 1.5, sum / (fg + 1)

    double l_cls = 0.0, l_reg = 0.0, l_corner = 0.0, l_bb = 0.0;
    for (int i = tid; i < p.n; i += RL_THREADS) {
        const float y = p.labels[i];                                             // rows with y < 0 are ignored
        float g_cls = 0.f;
        if (y >= 0.f) l_cls += (double)bce_row(p.cls[i], y, cls_scale, &g_cls);
        p.d_cls[i] = g_cls;
        float gr[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (p.mask[i] > 0.f) {
            const float *r = p.reg + (size_t)i * 7, *roi = p.rois + (size_t)i * 7;
            float g7[7];
            clamped_gt(p.gt + (size_t)i * p.ld_gt, g7);
            reg_row(r, roi, g7, p.cw, reg_scale, &l_reg, gr);
            const RlDecoded d = decode_local(r, roi);
            l_bb += (double)bb_row(d, roi, g7, bb_scale, gr);
            if (corner_on) l_corner += (double)corner_row(r, d, roi, p.gt_src + (size_t)i * p.ld_src, corner_scale, gr);
        }
        for (int k = 0; k < 7; ++k) p.d_reg[(size_t)i * 7 + k] = gr[k];
    }
    // ---- 3. fixed-order reduction of the lanes' partial sums
    sl[0][tid] = l_cls; sl[1][tid] = l_reg; sl[2][tid] = l_corner; sl[3][tid] = l_bb;
    __syncthreads();
    for (int s = RL_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s)
            for (int q = 0; q < 4; ++q) sl[q][tid] += sl[q][tid + s];
        __syncthreads();
    }
    if (tid == 0) {
        const float lc = (float)(sl[0][0] / (double)fmaxf((float)valid, 1.f)) * p.cls_weight;
        const float lr = (float)(sl[1][0] / (double)(fg > 1 ? fg : 1)) * p.reg_weight;
        const float lk = corner_on ? (float)(sl[2][0] / (double)fg) * p.corner_weight : 0.f;
        const float lb = fg > 0 ? (float)(sl[3][0] / (double)(fg + 1)) : 0.f;
        p.losses[0] = lc + lr + lk + lb;
        p.losses[1] = lc;
        p.losses[2] = lr;
        p.losses[3] = lk;
        p.losses[4] = lb;
        p.losses[5] = (float)fg;
    }
}

// ---- VoxelRCNNProtoHead.get_loss (voxel_rcnn_head.py:388-579) ----------------------------------------------------------------
// The detection branch (0) and the prototype branch (1) share one set of target rows. Branch j: css-weighted BCE, smooth-L1 and the
// corner term over the rows with mask * css > 0; proto_loss: css-weighted bb_loss of branch 0's decoded boxes against the canonical
// gt (b0) and against branch 1's decoded boxes as constants (b1, ramped twice), and the css-weighted cosine similarity of the shared
// features (feat1 a constant).
//   total = cls0 + reg0 + corner0 + proto_weight (0.5 cls1 + 0.5 (reg1 + corner1) + b0 + b1 + feat)
// Same shape as rcnn_loss_kernel (one workgroup, lane-per-row scalar terms, fixed-order sums); the feature pass runs wave-per-row,
// lanes over channels, its dot products reduced by a butterfly over the wave.
struct PlParams {
    const float *cls[2], *reg[2], *feat[2];
    const float *rois, *gt, *gt_src, *mask, *labels, *css;
    int n, feat_dim, ld_gt, ld_src, corner_reg;
    float cw[7], cls_weight, reg_weight, corner_weight, proto_weight, ramp;
    float *d_cls[2], *d_reg[2], *d_feat0, *losses;
};

constexpr int PL_TERMS = 9;         // cls0 reg0 corner0 cls1 reg1 corner1 b0 b1 feat

__device__ __forceinline__ double wave_sum(double v) {       // butterfly: every lane ends with the same sum, in the same order every call
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ void __launch_bounds__(RL_THREADS) rcnn_proto_loss_kernel(PlParams p) {
    __shared__ int sc[3][RL_THREADS];
    __shared__ double sl[PL_TERMS][RL_THREADS];
    const int tid = threadIdx.x;
    // ---- 1. normalisers: #valid, #(mask > 0), #(mask * css > 0) (integer sums: exact) and the float sum of valid * css
    int n_valid = 0, n_fgp = 0, n_fgc = 0;
    double s_valid = 0.0;
    for (int i = tid; i < p.n; i += RL_THREADS) {
        const float m = p.mask[i], c = p.css[i];
        const bool v = p.labels[i] >= 0.f;
        n_valid += v ? 1 : 0;
        n_fgp += m > 0.f ? 1 : 0;
        n_fgc += m * c > 0.f ? 1 : 0;
        s_valid += v ? (double)c : 0.0;
    }
    sc[0][tid] = n_valid; sc[1][tid] = n_fgp; sc[2][tid] = n_fgc; sl[0][tid] = s_valid;
    __syncthreads();
    for (int s = RL_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) {
            for (int q = 0; q < 3; ++q) sc[q][tid] += sc[q][tid + s];
            sl[0][tid] += sl[0][tid + s];
        }
        __syncthreads();
    }
    const int valid = sc[0][0], fgp = sc[1][0], fgc = sc[2][0];
    const float sv = fmaxf((float)sl[0][0], 1.f);                                // torch.clamp((valid * css).sum(), min=1.0)
    __syncthreads();                                                             // sl is written again below
    const float w = p.ramp, half_pw = 0.5f * p.proto_weight;
    const float cls_scale = p.cls_weight / fmaxf((float)valid, 1.f);             // the css weights the numerator only
    const float reg_scale = p.reg_weight / (float)(fgc > 1 ? fgc : 1);
    const bool corner_on = p.corner_reg && fgc > 0;
    const float corner_scale = corner_on ? p.corner_weight / (float)fgc / 8.f : 0.f;
    const float b0_scale = p.proto_weight * 1.5f / (float)(fgp + 1);
    const float b1_scale = b0_scale * w * w;                                     // b_loss1 *= w, then b_loss1 * w
    const float feat_scale = -p.proto_weight * w / sv;                           // feat = w * sum(-cos * weight) / sv

    double acc[PL_TERMS];
    for (int q = 0; q < PL_TERMS; ++q) acc[q] = 0.0;
    // ---- 2. the scalar terms, lane per row
    for (int i = tid; i < p.n; i += RL_THREADS) {
        const float y = p.labels[i], c = p.css[i], m = p.mask[i];
        for (int j = 0; j < 2; ++j) {
            float g_cls = 0.f;
            if (y >= 0.f) acc[3 * j] += (double)(bce_row(p.cls[j][i], y, (j ? half_pw : 1.f) * cls_scale * c, &g_cls) * c);
            p.d_cls[j][i] = g_cls;
        }
        float gr0[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, gr1[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        const bool row_fgc = m * c > 0.f, row_fgp = m > 0.f;
        if (row_fgc || row_fgp) {
            const float *r0 = p.reg[0] + (size_t)i * 7, *r1 = p.reg[1] + (size_t)i * 7, *roi = p.rois + (size_t)i * 7;
            const float *gs = p.gt_src + (size_t)i * p.ld_src;
            float g7[7];
            clamped_gt(p.gt + (size_t)i * p.ld_gt, g7);
            const RlDecoded d0 = decode_local(r0, roi), d1 = decode_local(r1, roi);
            if (row_fgc) {
                reg_row(r0, roi, g7, p.cw, reg_scale, &acc[1], gr0);
                reg_row(r1, roi, g7, p.cw, half_pw * reg_scale, &acc[4], gr1);
                if (corner_on) {
                    acc[2] += (double)corner_row(r0, d0, roi, gs, corner_scale, gr0);
                    acc[5] += (double)corner_row(r1, d1, roi, gs, half_pw * corner_scale, gr1);
                }
            }
            if (row_fgp) {
                acc[6] += (double)(bb_row(d0, roi, g7, b0_scale * c, gr0) * c);
                acc[7] += (double)(bb_row(d0, roi, d1.pb, b1_scale * c, gr0) * c);
            }
        }
        for (int k = 0; k < 7; ++k) {
            p.d_reg[0][(size_t)i * 7 + k] = gr0[k];
            p.d_reg[1][(size_t)i * 7 + k] = gr1[k];
        }
    }
    // ---- 3. the feature term, wave per row: cos = sum (x / max(|x|, 1e-8)) (y / max(|y|, 1e-8)). torch clamps the norms outside the
    // graph, so d cos / dx = yn / cx - cos / cx * x / |x| below the bound too (the norm's gradient is 0 at a zero vector)
    const int lane = tid & 63, wave = tid >> 6;
    for (int i = wave; i < p.n; i += RL_THREADS / 64) {
        const float wt = p.labels[i] >= 0.f ? p.css[i] : 0.f;
        const float *x = p.feat[0] + (size_t)i * p.feat_dim, *y = p.feat[1] + (size_t)i * p.feat_dim;
        float *dx = p.d_feat0 + (size_t)i * p.feat_dim;
        if (wt == 0.f) {                                                         // wave-uniform
            for (int ch = lane; ch < p.feat_dim; ch += 64) dx[ch] = 0.f;
            continue;
        }
        double xx = 0.0, yy = 0.0, xy = 0.0;
        for (int ch = lane; ch < p.feat_dim; ch += 64) {
            const double a = (double)x[ch], b = (double)y[ch];
            xx += a * a; yy += b * b; xy += a * b;
        }
        xx = wave_sum(xx); yy = wave_sum(yy); xy = wave_sum(xy);
        const float nx = (float)sqrt(xx), ny = (float)sqrt(yy);
        const float cx = fmaxf(nx, 1e-8f), cy = fmaxf(ny, 1e-8f);
        const float cosv = (float)(xy / ((double)cx * (double)cy));
        if (lane == 0) acc[8] += (double)(-cosv * wt);
        const float g = feat_scale * wt;                                         // d total / d cos of this row
        const float g_cx = -g * cosv / cx;                                       // through x / cx
        const float g_nx = nx > 0.f ? g_cx / nx : 0.f;                           // through |x|
        for (int ch = lane; ch < p.feat_dim; ch += 64) dx[ch] = g * (y[ch] / cy) / cx + g_nx * x[ch];
    }
    // ---- 4. fixed-order reduction of the lanes' partial sums
    for (int q = 0; q < PL_TERMS; ++q) sl[q][tid] = acc[q];
    __syncthreads();
    for (int s = RL_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s)
            for (int q = 0; q < PL_TERMS; ++q) sl[q][tid] += sl[q][tid + s];
        __syncthreads();
    }
    if (tid == 0) {
        float t[PL_TERMS];
        for (int j = 0; j < 2; ++j) {
            t[3 * j] = (float)(sl[3 * j][0] / (double)fmaxf((float)valid, 1.f)) * p.cls_weight;
            t[3 * j + 1] = (float)(sl[3 * j + 1][0] / (double)(fgc > 1 ? fgc : 1)) * p.reg_weight;
            t[3 * j + 2] = corner_on ? (float)(sl[3 * j + 2][0] / (double)fgc) * p.corner_weight : 0.f;
        }
        t[6] = fgp > 0 ? (float)(sl[6][0] / (double)(fgp + 1)) : 0.f;
        t[7] = fgp > 0 ? (float)(sl[7][0] / (double)(fgp + 1)) * w * w : 0.f;
        t[8] = (float)(sl[8][0] / (double)sv) * w;
        const float proto = 0.5f * t[3] + 0.5f * (t[4] + t[5]) + (t[6] + t[7] + t[8]);
        p.losses[0] = t[0] + (t[1] + t[2]) + proto * p.proto_weight;
        for (int q = 0; q < PL_TERMS; ++q) p.losses[1 + q] = t[q];
        p.losses[10] = (float)fgc;
        p.losses[11] = (float)fgp;
    }
}

}  // namespace

extern "C" int cpd_rcnn_loss(const float *rcnn_cls, const float *rcnn_reg, const float *rois, const float *gt_of_rois, int ld_gt,
                             const float *gt_of_rois_src, int ld_src, const float *reg_valid_mask, const float *rcnn_cls_labels, int n,
                             const float code_weights[7], float cls_weight, float reg_weight, float corner_weight,
                             int corner_regularization, float *d_cls, float *d_reg, float *losses, cpd_stream_t st) {
    if (!losses || !code_weights || n < 0) return CPD_ERR_ARG;
    if (n > 0 && (!rcnn_cls || !rcnn_reg || !rois || !gt_of_rois || !gt_of_rois_src || !reg_valid_mask || !rcnn_cls_labels || !d_cls ||
                  !d_reg || ld_gt < 7 || ld_src < 7))
        return CPD_ERR_ARG;
    RlParams p;
    p.cls = rcnn_cls; p.reg = rcnn_reg; p.rois = rois; p.gt = gt_of_rois; p.gt_src = gt_of_rois_src; p.mask = reg_valid_mask;
    p.labels = rcnn_cls_labels;
    p.n = n; p.ld_gt = ld_gt; p.ld_src = ld_src; p.corner_reg = corner_regularization ? 1 : 0;
    for (int k = 0; k < 7; ++k) p.cw[k] = code_weights[k];
    p.cls_weight = cls_weight; p.reg_weight = reg_weight; p.corner_weight = corner_weight;
    p.d_cls = d_cls; p.d_reg = d_reg; p.losses = losses;
    cpd_launch_log_note("rcnn_loss_kernel");
    rcnn_loss_kernel<<<1, RL_THREADS, 0, cpd_s(st)>>>(p);       // n = 0: the counts are 0 and the kernel writes zero losses
    return cpd_check_launch();
}

extern "C" int cpd_rcnn_proto_loss(const float *cls0, const float *reg0, const float *feat0, const float *cls1, const float *reg1,
                                   const float *feat1, int feat_dim, const float *rois, const float *gt_of_rois, int ld_gt,
                                   const float *gt_of_rois_src, int ld_src, const float *reg_valid_mask, const float *rcnn_cls_labels,
                                   const float *css_score, int n, const float code_weights[7], float cls_weight, float reg_weight,
                                   float corner_weight, float proto_weight, float ramp_weight, int corner_regularization, float *d_cls0,
                                   float *d_reg0, float *d_feat0, float *d_cls1, float *d_reg1, float *losses, cpd_stream_t st) {
    if (!losses || !code_weights || n < 0 || feat_dim < 1) return CPD_ERR_ARG;
    if (n > 0 && (!cls0 || !reg0 || !feat0 || !cls1 || !reg1 || !feat1 || !rois || !gt_of_rois || !gt_of_rois_src || !reg_valid_mask ||
                  !rcnn_cls_labels || !css_score || !d_cls0 || !d_reg0 || !d_feat0 || !d_cls1 || !d_reg1 || ld_gt < 7 || ld_src < 7))
        return CPD_ERR_ARG;
    PlParams p;
    p.cls[0] = cls0; p.reg[0] = reg0; p.feat[0] = feat0; p.cls[1] = cls1; p.reg[1] = reg1; p.feat[1] = feat1;
    p.rois = rois; p.gt = gt_of_rois; p.gt_src = gt_of_rois_src; p.mask = reg_valid_mask; p.labels = rcnn_cls_labels; p.css = css_score;
    p.n = n; p.feat_dim = feat_dim; p.ld_gt = ld_gt; p.ld_src = ld_src; p.corner_reg = corner_regularization ? 1 : 0;
    for (int k = 0; k < 7; ++k) p.cw[k] = code_weights[k];
    p.cls_weight = cls_weight; p.reg_weight = reg_weight; p.corner_weight = corner_weight; p.proto_weight = proto_weight;
    p.ramp = ramp_weight;
    p.d_cls[0] = d_cls0; p.d_reg[0] = d_reg0; p.d_cls[1] = d_cls1; p.d_reg[1] = d_reg1; p.d_feat0 = d_feat0; p.losses = losses;
    cpd_launch_log_note("rcnn_proto_loss_kernel");
    rcnn_proto_loss_kernel<<<1, RL_THREADS, 0, cpd_s(st)>>>(p);  // n = 0: the counts are 0 and the kernel writes zero losses
    return cpd_check_launch();
}
