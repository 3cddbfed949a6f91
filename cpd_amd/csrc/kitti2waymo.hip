// kitti2waymo.hip -- the two device stages of the KITTI transfer evaluation (Kitti2WaymoDataset): the FOV crop in front of the
// voxelizer and the camera-frame export behind the detector. See include/cpd_hip.h for the contracts. Built with -ffp-contract=off:
// every keep / drop decision is numpy's float32 expression op by op.
#include "common.h"

namespace {

struct K2wFrame {     // CPD_K2W_FRAME_WORDS words
    float m[12];      // np.dot(V2C.T, R0.T) [4][3]
    float p[12];      // P2 [3][4]
    int32_t h, w;     // image_shape
};
static_assert(sizeof(K2wFrame) == 4 * CPD_K2W_FRAME_WORDS, "frame record layout");

constexpr int kRounds = CPD_K2W_TILE / CPD_K2W_BLOCK;
constexpr int kWaves = CPD_K2W_BLOCK / CPD_WAVE;

// Calibration.lidar_to_rect: [x y z 1] . M, left to right (1 * M[3][j] is exact)
__device__ __forceinline__ void lidar_to_rect(const K2wFrame &f, float x, float y, float z, float &rx, float &ry, float &rz) {
    rx = ((x * f.m[0] + y * f.m[3]) + z * f.m[6]) + f.m[9];
    ry = ((x * f.m[1] + y * f.m[4]) + z * f.m[7]) + f.m[10];
    rz = ((x * f.m[2] + y * f.m[5]) + z * f.m[8]) + f.m[11];
}
// Calibration.rect_to_img: [rect 1] . P2^T; the image point is divided by the RECTIFIED z
__device__ __forceinline__ void rect_to_img(const K2wFrame &f, float rx, float ry, float rz, float &u, float &v, float &depth) {
    const float h0 = ((rx * f.p[0] + ry * f.p[1]) + rz * f.p[2]) + f.p[3];
    const float h1 = ((rx * f.p[4] + ry * f.p[5]) + rz * f.p[6]) + f.p[7];
    const float h2 = ((rx * f.p[8] + ry * f.p[9]) + rz * f.p[10]) + f.p[11];
    u = h0 / rz;
    v = h1 / rz;
    depth = h2 - f.p[11];
}
__device__ __forceinline__ bool fov_keep(const K2wFrame &f, float x, float y, float z) {
    float rx, ry, rz, u, v, depth;
    lidar_to_rect(f, x, y, z, rx, ry, rz);
    rect_to_img(f, rx, ry, rz, u, v, depth);
    return u >= 0.f && u < (float)f.w && v >= 0.f && v < (float)f.h && depth >= 0.f;     // NaN: false
}

__device__ __forceinline__ void load_point(const float *__restrict__ points, int ld, int vec_in, long long row, float &x, float &y, float &z) {
    if (vec_in) {
        const float4 q = reinterpret_cast<const float4 *>(points)[row];
        x = q.x, y = q.y, z = q.z;
    } else {
        const float *q = points + row * ld;
        x = q[0], y = q[1], z = q[2];
    }
}

// frame bounds of block (tile blockIdx.x, frame blockIdx.y); false: the frame is refused or the tile lies beyond it
__device__ __forceinline__ bool fov_tile(const int32_t *__restrict__ frame_start, int n, int max_len, int &start, int &len, bool &refused) {
    start = frame_start[blockIdx.y];
    len = frame_start[blockIdx.y + 1] - start;
    refused = start < 0 || len < 0 || (long long)start + len > n || len > max_len;
    return !refused && (long long)blockIdx.x * CPD_K2W_TILE < len;
}

// the lanes' keep flags of the tile: bit k of the result is round k (point tile * TILE + k * BLOCK + thread), whose coordinates
// stay in px / py / pz [k] (constant indices after unrolling: registers; dead in the count pass)
__device__ __forceinline__ uint32_t fov_flags(const float *__restrict__ points, int ld, int vec_in, const K2wFrame &f, int start, int len,
                                              float (&px)[kRounds], float (&py)[kRounds], float (&pz)[kRounds]) {
    uint32_t bits = 0;
#pragma unroll
    for (int k = 0; k < kRounds; ++k) {
        const int i = blockIdx.x * CPD_K2W_TILE + k * CPD_K2W_BLOCK + threadIdx.x;
        px[k] = py[k] = pz[k] = 0.f;
        if (i < len) {
            load_point(points, ld, vec_in, (long long)start + i, px[k], py[k], pz[k]);
            bits |= fov_keep(f, px[k], py[k], pz[k]) ? (1u << k) : 0u;
        }
    }
    return bits;
}

__global__ void __launch_bounds__(CPD_K2W_BLOCK) fov_count_kernel(const float *__restrict__ points, int n, int ld, int vec_in,
                                                                  const int32_t *__restrict__ frame_start, int max_len,
                                                                  const K2wFrame *__restrict__ frames, uint32_t *__restrict__ tile_count) {
    __shared__ uint32_t sm[kWaves];
    int start, len;
    bool refused;
    if (!fov_tile(frame_start, n, max_len, start, len, refused)) return;
    const K2wFrame &f = frames[blockIdx.y];
    float px[kRounds], py[kRounds], pz[kRounds];
    const uint32_t bits = fov_flags(points, ld, vec_in, f, start, len, px, py, pz);
    uint32_t c = 0;
#pragma unroll
    for (int k = 0; k < kRounds; ++k) c += __popcll(__ballot((bits >> k) & 1u));
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (int w = 0; w < kWaves; ++w) t += sm[w];
        tile_count[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = t;
    }
}

__global__ void __launch_bounds__(CPD_K2W_BLOCK) fov_scatter_kernel(const float *__restrict__ points, int n, int ld, int vec_in,
                                                                    const int32_t *__restrict__ frame_start, int max_len,
                                                                    const K2wFrame *__restrict__ frames, const uint32_t *__restrict__ tile_count,
                                                                    double z_shift, int nfo, int vec_out, float *__restrict__ out,
                                                                    int32_t *__restrict__ out_index, int32_t *__restrict__ out_count) {
    __shared__ uint32_t sm_tot[kRounds * kWaves];
    __shared__ uint32_t sm_base;
    int start, len;
    bool refused;
    if (!fov_tile(frame_start, n, max_len, start, len, refused)) {
        if (blockIdx.x == 0 && threadIdx.x == 0) out_count[blockIdx.y] = refused ? -1 : 0;     // refused, or an empty frame
        return;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // kept points of the frame's earlier tiles (integer sum: any order gives the same value)
    if (wave == 0) {
        uint32_t acc = 0;
        for (int j = lane; j < (int)blockIdx.x; j += 64) acc += tile_count[(size_t)blockIdx.y * gridDim.x + j];
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) acc += __shfl_xor(acc, d, 64);
        if (lane == 0) sm_base = acc;
    }
    const K2wFrame &f = frames[blockIdx.y];
    float px[kRounds], py[kRounds], pz[kRounds];
    const uint32_t bits = fov_flags(points, ld, vec_in, f, start, len, px, py, pz);
    uint32_t before[kRounds];      // kept lanes below this one in its wave, per round
#pragma unroll
    for (int k = 0; k < kRounds; ++k) {
        const unsigned long long b = __ballot((bits >> k) & 1u);
        before[k] = __popcll(b & ((1ull << lane) - 1ull));
        if (lane == 0) sm_tot[k * kWaves + wave] = __popcll(b);
    }
    __syncthreads();
    uint32_t run = sm_base;        // kept points before round k of this tile
#pragma unroll
    for (int k = 0; k < kRounds; ++k) {
        uint32_t lower_waves = 0, round_total = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            const uint32_t t = sm_tot[k * kWaves + w];
            lower_waves += w < wave ? t : 0u;
            round_total += t;
        }
        if ((bits >> k) & 1u) {
            const int i = blockIdx.x * CPD_K2W_TILE + k * CPD_K2W_BLOCK + threadIdx.x;
            const float zs = (float)((double)pz[k] + z_shift);
            const long long row = (long long)start + run + lower_waves + before[k];      // < start + len: at most len points are kept
            if (vec_out) {
                reinterpret_cast<float4 *>(out)[row] = make_float4(px[k], py[k], zs, 0.f);
            } else {
                float *o = out + row * nfo;
                o[0] = px[k], o[1] = py[k], o[2] = zs;
                for (int c = 3; c < nfo; ++c) o[c] = 0.f;
            }
            if (out_index) out_index[row] = i;
        }
        run += round_total;
    }
    if ((int)blockIdx.x == (len - 1) / CPD_K2W_TILE && threadIdx.x == 0) out_count[blockIdx.y] = (int32_t)run;   // the frame's last tile
}

// np.min / np.max / np.clip keep a NaN
__device__ __forceinline__ float np_min(float m, float v) { return (v < m || v != v) ? v : m; }
__device__ __forceinline__ float np_max(float m, float v) { return (v > m || v != v) ? v : m; }
__device__ __forceinline__ float np_clip(float v, float lo, float hi) { return v != v ? v : fminf(fmaxf(v, lo), hi); }

__global__ void __launch_bounds__(CPD_K2W_BLOCK) export_kernel(const float *__restrict__ boxes, const float *__restrict__ scores,
                                                               const int32_t *__restrict__ labels, int n,
                                                               const int32_t *__restrict__ seg_start, const K2wFrame *__restrict__ frames,
                                                               int mode, float *__restrict__ out_boxes, float *__restrict__ out_scores,
                                                               int32_t *__restrict__ out_labels, float *__restrict__ out_camera,
                                                               float *__restrict__ out_alpha, float *__restrict__ out_bbox,
                                                               int32_t *__restrict__ out_count) {
    __shared__ uint32_t sm[17];
    const int start = seg_start[blockIdx.x], len = seg_start[blockIdx.x + 1] - start;
    if (start < 0 || len < 0 || (long long)start + len > n) {
        if (threadIdx.x == 0) out_count[blockIdx.x] = -1;
        return;
    }
    const K2wFrame &f = frames[blockIdx.x];
    const bool predict = mode == CPD_K2W_PREDICT;
    // mask_car.sum() != 0 (kitti2waymo_dataset.py:279-281)
    int any = 0;
    if (predict)
        for (int i = threadIdx.x; i < len; i += CPD_K2W_BLOCK) any |= labels[start + i] != 0;
    const bool shrink = predict && __syncthreads_or(any);
    uint32_t run = 0;
    for (int c0 = 0; c0 < len; c0 += CPD_K2W_BLOCK) {      // uniform trip count: the scan below holds barriers
        const int i = c0 + threadIdx.x;
        const bool active = i < len;
        float x = 0.f, y = 0.f, z = 0.f, l = 0.f, w = 0.f, h = 0.f, r = 0.f, score = 0.f;
        int32_t lab = 0;
        bool keep = active;
        if (active) {
            const float *b = boxes + (long long)(start + i) * 7;
            x = b[0], y = b[1], z = b[2], l = b[3], w = b[4], h = b[5], r = b[6];
            if (scores) score = scores[start + i];
            if (labels) lab = labels[start + i];
        }
        if (active && predict) {
            z = z - 1.55f;
            if (shrink) {
                if (lab != 0) {
                    z = z + 0.1f;
                    l = l - 0.2f;
                    w = w - 0.2f;
                    h = h - 0.1f;
                }
                keep = l < 5.f;
            }
            if (keep && lab == 1) {     // l.296-331
                const float cs = cosf(r), sn = sinf(r);
                const float dis0 = sqrtf((x * x + y * y) + z * z);
                double half_d;
                if (dis0 > 60.f) {
                    half_d = (0.1 + 1.0 * (0.4 - 0.1)) / 2;                     // Python floats from here on
                } else {
                    const float weight = dis0 / 60.f;
                    const float new_d = 0.1f + weight * (float)(0.4 - 0.1);      // float32 scalars (numpy >= 2)
                    half_d = (double)(new_d / 2.f);
                }
                const double x1 = half_d * (double)cs + (double)x, y1 = half_d * (double)sn + (double)y;
                const double x2 = -half_d * (double)cs + (double)x, y2 = -half_d * (double)sn + (double)y;
                const double zz = (double)z * (double)z;
                const double dis1 = sqrt(((x1 * x1 + y1 * y1) + zz) + 1.0);      // the norm takes the homogeneous 1 along
                const double dis2 = sqrt(((x2 * x2 + y2 * y2) + zz) + 1.0);
                if (dis1 < dis2) {
                    x = (float)x1, y = (float)y1;
                } else {
                    x = (float)x2, y = (float)y2;
                }
            }
        }
        uint32_t tot;
        const uint32_t pos = run + block_excl_scan(keep ? 1u : 0u, sm, &tot);
        run += tot;
        if (!keep) continue;
        // boxes3d_lidar_to_kitti_camera (in place: the returned boxes_lidar is bottom-centred)
        z = z - h / 2.f;
        float cx, cy, cz;
        lidar_to_rect(f, x, y, z, cx, cy, cz);
        const float ry = -r - 1.5707963267948966f;
        // boxes3d_to_corners3d_kitti_camera + rect_to_img + min / max
        const float cr = cosf(ry), sr = sinf(ry);
        const float hl = l / 2.f, hw = w / 2.f;
        float u0 = 0.f, v0 = 0.f, u1 = 0.f, v1 = 0.f;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const float xc = ((k >> 1) & 1) ? -hl : hl;
            const float zc = (((k + 1) >> 1) & 1) ? -hw : hw;
            const float yc = k >= 4 ? -h : 0.f;
            const float px = cx + ((xc * cr + yc * 0.f) + zc * sr);
            const float py = cy + ((xc * 0.f + yc * 1.f) + zc * 0.f);
            const float pz = cz + ((xc * -sr + yc * 0.f) + zc * cr);
            float u, v, depth;
            rect_to_img(f, px, py, pz, u, v, depth);
            if (k == 0) {
                u0 = u1 = u, v0 = v1 = v;
            } else {
                u0 = np_min(u0, u), v0 = np_min(v0, v), u1 = np_max(u1, u), v1 = np_max(v1, v);
            }
        }
        const float wmax = (float)(f.w - 1), hmax = (float)(f.h - 1);
        const long long row = (long long)start + pos;       // pos < len
        float *ob = out_boxes + row * 7;
        ob[0] = x, ob[1] = y, ob[2] = z, ob[3] = l, ob[4] = w, ob[5] = h, ob[6] = r;
        out_scores[row] = score;
        out_labels[row] = lab;
        float *oc = out_camera + row * 7;
        oc[0] = cx, oc[1] = cy, oc[2] = cz, oc[3] = l, oc[4] = h, oc[5] = w, oc[6] = ry;
        out_alpha[row] = -atan2f(-y, x) + ry;
        float *bb = out_bbox + row * 4;
        bb[0] = np_clip(u0, 0.f, wmax), bb[1] = np_clip(v0, 0.f, hmax), bb[2] = np_clip(u1, 0.f, wmax), bb[3] = np_clip(v1, 0.f, hmax);
    }
    if (threadIdx.x == 0) out_count[blockIdx.x] = (int32_t)run;
}

static inline int fov_tiles(int max_len) { return max_len <= 0 ? 1 : cpd_div_up(max_len, CPD_K2W_TILE); }

}  // namespace

extern "C" size_t cpd_kitti_fov_workspace_bytes(int batch, int max_len) {
    if (batch < 0 || max_len < 0) return 0;
    return cpd_align((size_t)batch * fov_tiles(max_len) * sizeof(uint32_t));
}

extern "C" int cpd_kitti_fov_points(const float *points, int n, int ld, const int32_t *frame_start, int batch, int max_len,
                                    const void *frames, double z_shift, int n_feat_out, float *out, int32_t *out_index,
                                    int32_t *out_count, void *workspace, size_t workspace_bytes, cpd_stream_t stream) {
    if (n < 0 || batch < 0 || ld < 3 || n_feat_out < 3 || max_len < 0 || max_len > n || (n > 0 && (!points || !out))) return CPD_ERR_ARG;
    if (batch == 0) return CPD_OK;
    if (batch > 65535 || !frame_start || !frames || !out_count) return CPD_ERR_ARG;
    if (!workspace || workspace_bytes < cpd_kitti_fov_workspace_bytes(batch, max_len)) return CPD_ERR_WORKSPACE;
    const int vec_in = ld == 4 && ((uintptr_t)points & 15) == 0, vec_out = n_feat_out == 4 && ((uintptr_t)out & 15) == 0;
    const dim3 grid(fov_tiles(max_len), batch);
    const K2wFrame *fr = static_cast<const K2wFrame *>(frames);
    uint32_t *tile_count = static_cast<uint32_t *>(workspace);
    fov_count_kernel<<<grid, CPD_K2W_BLOCK, 0, cpd_s(stream)>>>(points, n, ld, vec_in, frame_start, max_len, fr, tile_count);
    fov_scatter_kernel<<<grid, CPD_K2W_BLOCK, 0, cpd_s(stream)>>>(points, n, ld, vec_in, frame_start, max_len, fr, tile_count, z_shift,
                                                                 n_feat_out, vec_out, out, out_index, out_count);
    return cpd_check_launch();
}

extern "C" int cpd_kitti_export(const float *boxes, const float *scores, const int32_t *labels, int n, const int32_t *seg_start, int batch,
                                const void *frames, int mode, float *out_boxes, float *out_scores, int32_t *out_labels, float *out_camera,
                                float *out_alpha, float *out_bbox, int32_t *out_count, cpd_stream_t stream) {
    if (n < 0 || batch < 0 || (mode != CPD_K2W_PREDICT && mode != CPD_K2W_CAMERA)) return CPD_ERR_ARG;
    if (n > 0 && (!boxes || !out_boxes || !out_scores || !out_labels || !out_camera || !out_alpha || !out_bbox)) return CPD_ERR_ARG;
    if (mode == CPD_K2W_PREDICT && n > 0 && (!scores || !labels)) return CPD_ERR_ARG;
    if (batch == 0) return CPD_OK;
    if (!seg_start || !frames || !out_count) return CPD_ERR_ARG;
    export_kernel<<<batch, CPD_K2W_BLOCK, 0, cpd_s(stream)>>>(boxes, scores, labels, n, seg_start, static_cast<const K2wFrame *>(frames), mode,
                                                            out_boxes, out_scores, out_labels, out_camera, out_alpha, out_bbox, out_count);
    return cpd_check_launch();
}
