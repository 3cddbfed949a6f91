// decode.hip -- CenterHead box decode for gfx950.
//
// Replaces, for one sample, CenterHead.generate_predicted_boxes (center_head.py:252-303) ->
// centernet_utils._topk (centernet_utils.py:136-151) + decode_bbox_from_heatmap (l.154-216):
//   sigmoid(hm) -> per-class top-K over H*W -> top-K over (class, K) -> gather the regression
//   maps at the winners -> exp(dim), atan2(sin, cos), centre scaling -> POST_CENTER_LIMIT_RANGE
//   and SCORE_THRESH masks -> order-preserving compaction (scores stay sorted descending).
// The reference runs this as ~20 small torch kernels; here it is two launches:
//   topk_class_kernel : one 1024-thread workgroup per class: a logit histogram picks <= 1024 candidates
//                       (block_topk_logits); where that cannot keep the tie rule or they do not fit, a
//                       4-pass radix select of the K-th key (LDS histogram) with ordered tie collection
//                       (block_topk); either way a 1024-wide bitonic sort in LDS
//   decode_kernel     : one workgroup: second top-K, gather, decode, mask, block-scan compaction
// Ties are broken by ascending flat index (torch.topk leaves tie order unspecified).
//
// The same pipeline cut at the peaks (cpd_center_peaks -> cpd_peak_rulebook -> cpd_center_decode_at_peaks), for a head that evaluates
// its regression branches at the K winners only: the selection (topk_class_kernel + the rank merge) needs the hm map alone; the
// winners' pixels then name the 9 hidden sites each that the branches' last 3 x 3 convolution reads, the caller computes those hidden
// rows (one gather_conv launch over the table of cpd_peak_rulebook), and the finish forms the regression values of every peak in
// fp32 and runs decode_box, the masks and the compaction of decode_kernel -- the same functions, so the two paths differ by the
// summation order of the last convolution and nothing else.
#include "common.h"

namespace {

struct MapView {  // map[pixel * pix + channel * ch] of the sample the pointer was offset to
    const float *p;
    int pix, ch;
    __device__ __forceinline__ MapView sample(int b, long long sample_stride) const {
        return MapView{p + (size_t)b * sample_stride, pix, ch};
    }
    __device__ __forceinline__ float at(int pixel, int channel) const {
        return p[(size_t)pixel * pix + (size_t)channel * ch];
    }
};

__device__ __forceinline__ float sigmoidf(float x) { return 1.0f / (1.0f + expf(-x)); }

struct TopkSmem {
    uint32_t hist[256];
    unsigned long long packed[1024];
    uint32_t scan[17];
    uint32_t sel, remaining, cnt_gt;
};

// Block-wide (1024 threads) top-K of keyfn(i), i in [0,n). On return sm.packed[0..K) holds
// (key << 32 | ~index) sorted descending, i.e. key descending then index ascending.
template <class KeyFn>
__device__ void block_topk(int n, int K, KeyFn keyfn, TopkSmem &sm) {
    const int tid = threadIdx.x, nth = blockDim.x;
    uint32_t prefix = 0, pmask = 0;
    uint32_t remaining = (uint32_t)K;
    for (int shift = 24; shift >= 0; shift -= 8) {
        for (int b = tid; b < 256; b += nth) sm.hist[b] = 0;
        __syncthreads();
        for (int i = tid; i < n; i += nth) {
            uint32_t key = keyfn(i);
            if ((key & pmask) == prefix) atomicAdd(&sm.hist[(key >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (tid == 0) {
            uint32_t c = 0;
            int d = 255;
            for (; d > 0; --d) {
                if (c + sm.hist[d] >= remaining) break;
                c += sm.hist[d];
            }
            sm.sel = (uint32_t)d;
            sm.remaining = remaining - c;
        }
        __syncthreads();
        prefix |= sm.sel << shift;
        pmask |= 255u << shift;
        remaining = sm.remaining;
        __syncthreads();
    }
    const uint32_t kth = prefix;          // K-th largest key
    const uint32_t n_gt = (uint32_t)K - remaining;  // keys strictly greater
    if (tid == 0) sm.cnt_gt = 0;
    for (int i = tid; i < 1024; i += nth) sm.packed[i] = 0ull;
    __syncthreads();
    // strictly greater keys: any order (sorted afterwards)
    for (int i = tid; i < n; i += nth) {
        uint32_t key = keyfn(i);
        if (key > kth) {
            uint32_t pos = atomicAdd(&sm.cnt_gt, 1u);
            sm.packed[pos] = ((unsigned long long)key << 32) | (uint32_t)(~(uint32_t)i);
        }
    }
    // ties with the K-th key: lowest indices first -> ordered selection over contiguous chunks
    const int chunk = (n + nth - 1) / nth;
    const int i0 = tid * chunk, i1 = min(n, i0 + chunk);
    uint32_t mine = 0;
    for (int i = i0; i < i1; ++i) mine += keyfn(i) == kth ? 1u : 0u;
    uint32_t tot;
    uint32_t rank = block_excl_scan(mine, sm.scan, &tot);
    for (int i = i0; i < i1 && rank < remaining; ++i)
        if (keyfn(i) == kth) {
            sm.packed[n_gt + rank] = ((unsigned long long)kth << 32) | (uint32_t)(~(uint32_t)i);
            ++rank;
        }
    __syncthreads();
    // bitonic sort, descending, 1024 elements (zeros pad the tail and sink to the end)
    for (int k = 2; k <= 1024; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < 1024; i += nth) {
                int ixj = i ^ j;
                if (ixj > i) {
                    unsigned long long a = sm.packed[i], b = sm.packed[ixj];
                    bool desc = (i & k) == 0;
                    if (desc ? (a < b) : (a > b)) { sm.packed[i] = b; sm.packed[ixj] = a; }
                }
            }
            __syncthreads();
        }
}

// Fast path for the per-class stage: one histogram of the raw logits over 2048 LINEAR bins (low
// LDS-atomic contention, unlike radix digits of sigmoid values that share their exponent byte), a
// suffix scan to the bin holding the K-th element, then an exact bitonic sort of the <= 1024
// candidates above it on their sigmoid keys. Falls back to the exact radix select when the
// candidate set does not fit (degenerate score distributions).
//
// The order promised is (sigmoid key descending, index ascending), and bins are cut on the LOGIT: a pixel left out must not
// carry the K-th key, or its lower index would have won. fp32 sigmoid is flat over many logits (neighbouring positive floats share
// a value, a whole bin width of 40/2048 does from x ~ 12.7 up, everything from ~16.7 is 1.0f), so with b* the bin of the K-th
// logit the candidates are the bins >= b* - 1, and the path is taken only for b* <= TOPK_BIN_MAX, the bin whose lower edge is
// x = 10. A pixel left out then has x < edge(b* - 1) < lo and the K-th logit has x_K >= edge(b*) > hi, with lo / hi a quarter
// bin inside the two edges (the rounding in logit_bin moves an edge by ~1e-5, a quarter bin is 5e-3). A quarter bin changes
// exp(-x) by 0.5 %, far beyond expf's rounding, so expf(-x) > expf(-lo) and expf(-x_K) < expf(-hi) as computed; 1 + e and
// 1 / y round monotonically; hence key(x) <= key(lo) and key(hi) <= key(x_K). And key(lo) < key(hi): they are half a bin,
// 40/4096, apart and hi <= 10, where sigmoid' = s (1 - s) >= 4.5e-5, so the true values differ by >= 4.4e-7 = 7.4 steps of
// 2^-24 (fp32's spacing in [0.5, 1), the coarsest a sigmoid value meets), while a computed value is within 1.5 steps of the true
// one there (half an ulp of 1 + e in [1, 2), carried through 1 / y, plus the division's own half ulp; expf's error on e ~ 5e-5 is
// ~1e-11); for smaller x the difference grows with 1 - s and the spacing only shrinks. So no tie crosses the cut.
// Above bin TOPK_BIN_MAX (heads that saturate: scores over 0.99995) the radix path, which selects on the keys themselves, runs.
struct TopkHist {
    uint32_t hist[2048];
    uint32_t cnt, bstar, ok;
};
__device__ __forceinline__ int logit_bin(float x) {
    float t = (x + 20.0f) * 51.2f;             // [-20, 20) -> [0, 2048)
    t = t < 0.f ? 0.f : (t > 2047.f ? 2047.f : t);
    return (x != x) ? 0 : (int)t;
}
constexpr int TOPK_BIN_MAX = 1536;         // (10 + 20) * 51.2
__device__ bool block_topk_logits(const MapView &hm, int cls, int n, int K, TopkHist &h, TopkSmem &sm) {
    const int tid = threadIdx.x, nth = blockDim.x;
    for (int b = tid; b < 2048; b += nth) h.hist[b] = 0;
    if (tid == 0) { h.cnt = 0; h.ok = 0; }
    __syncthreads();
    for (int i = tid; i < n; i += nth) atomicAdd(&h.hist[logit_bin(hm.at(i, cls))], 1u);
    __syncthreads();
    if (tid < 64) {  // wave 0: suffix sums over 2048 bins, 32 bins per lane, from the top
        const int hi = 2047 - tid * 32;        // lane 0 owns the top 32 bins
        uint32_t s = 0;
        for (int k = 0; k < 32; ++k) s += h.hist[hi - k];
        const uint32_t incl = wave_incl_scan(s), before = incl - s;
        if (before < (uint32_t)K && incl >= (uint32_t)K) {  // the K-th element is in this lane's bins
            uint32_t c = before;
            int b = hi;
            for (; b > hi - 32; --b) {
                c += h.hist[b];
                if (c >= (uint32_t)K) break;
            }
            if (b > 0) c += h.hist[b - 1];     // candidates = everything in bins >= b* - 1 (see above)
            h.bstar = (uint32_t)(b > 0 ? b - 1 : 0);
            h.ok = (c <= 1024u && b <= TOPK_BIN_MAX) ? 1u : 0u;
        }
    }
    __syncthreads();
    if (!h.ok) return false;
    const int bstar = (int)h.bstar;
    for (int i = tid; i < 1024; i += nth) sm.packed[i] = 0ull;
    __syncthreads();
    for (int i = tid; i < n; i += nth) {
        const float x = hm.at(i, cls);
        if (logit_bin(x) >= bstar) {
            const uint32_t pos = atomicAdd(&h.cnt, 1u);
            sm.packed[pos] = ((unsigned long long)float_key(sigmoidf(x)) << 32) | (uint32_t)(~(uint32_t)i);
        }
    }
    __syncthreads();
    for (int k = 2; k <= 1024; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < 1024; i += nth) {
                int ixj = i ^ j;
                if (ixj > i) {
                    unsigned long long a = sm.packed[i], b = sm.packed[ixj];
                    bool desc = (i & k) == 0;
                    if (desc ? (a < b) : (a > b)) { sm.packed[i] = b; sm.packed[ixj] = a; }
                }
            }
            __syncthreads();
        }
    return true;
}

struct SigKey {
    MapView hm;
    int cls;
    __device__ __forceinline__ uint32_t operator()(int i) const { return float_key(sigmoidf(hm.at(i, cls))); }
};
struct ArrKey {
    const float *v;
    __device__ __forceinline__ uint32_t operator()(int i) const { return float_key(v[i]); }
};

__global__ void __launch_bounds__(1024) topk_class_kernel(MapView hm_all, long long sample_stride, int num_class, int hw,
                                                          int K, float *__restrict__ s1, int32_t *__restrict__ i1) {
    __shared__ TopkSmem sm;
    __shared__ TopkHist hist;
    const int cls = blockIdx.x, b = blockIdx.y;
    const MapView hm = hm_all.sample(b, sample_stride);
    if (!block_topk_logits(hm, cls, hw, K, hist, sm)) block_topk(hw, K, SigKey{hm, cls}, sm);
    const size_t o = ((size_t)b * num_class + cls) * K;
    for (int k = threadIdx.x; k < K; k += blockDim.x) {
        unsigned long long p = sm.packed[k];
        s1[o + k] = float_unkey((uint32_t)(p >> 32));
        i1[o + k] = (int32_t)(~(uint32_t)p);
    }
}

struct DecodeGeom {
    int w;
    float stride, vx, vy, lox, loy;
    float lim[6];
    float score_thresh;
};

struct DecodeParams {
    MapView center, center_z, dim, rot;
    long long sample_stride;
    int num_class, h, w, K;
    DecodeGeom g;
};

// the K best of the num_class x K per-class candidates, in (score descending, candidate index ascending) order. The per-class lists
// arrive SORTED (topk_class_kernel), so a candidate's place in the merged order is a sum of ranks: its own position, the entries of
// the classes before it that are >= its key, those of the classes after it that are > its key -- two binary searches per candidate
// instead of a radix select + bitonic sort over all of them (round 5: 54 -> 13 us at 3 x 500; the same order, bit for bit).
// On return sm.packed[0..K) = (key << 32 | ~candidate index) of the winners in their final order.
__device__ __forceinline__ void merge_class_lists(const float *__restrict__ s1, int num_class, int K, TopkSmem &sm) {
    const int n = num_class * K;
    for (int i2 = threadIdx.x; i2 < n; i2 += blockDim.x) {
        const int c = i2 / K, j = i2 - c * K;
        const uint32_t key = float_key(s1[i2]);
        int rank = j;
        for (int c2 = 0; c2 < num_class; ++c2) {
            if (c2 == c) continue;
            const float *l = s1 + (size_t)c2 * K;
            int lo = 0, hi = K;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                const uint32_t km = float_key(l[mid]);
                if (c2 < c ? km >= key : km > key) lo = mid + 1; else hi = mid;
            }
            rank += lo;
        }
        if (rank < K) sm.packed[rank] = ((unsigned long long)key << 32) | (uint32_t)(~(uint32_t)i2);
    }
    __syncthreads();
}

// one winner's box from its pixel and its eight regression values r = (center x, center y, center_z, dim 0..2, rot cos, rot sin;
// center_head.py:266-267) -> does it pass the POST_CENTER_LIMIT_RANGE and SCORE_THRESH masks
__device__ __forceinline__ bool decode_box(const DecodeGeom &g, int ind, float sc, const float r[8], float bx[7]) {
    const float xs = (float)(ind % g.w), ys = (float)(ind / g.w);
    bx[0] = (xs + r[0]) * g.stride * g.vx + g.lox;
    bx[1] = (ys + r[1]) * g.stride * g.vy + g.loy;
    bx[2] = r[2];
    bx[3] = expf(r[3]);
    bx[4] = expf(r[4]);
    bx[5] = expf(r[5]);
    bx[6] = atan2f(r[7], r[6]);
    bool ok = bx[0] >= g.lim[0] && bx[1] >= g.lim[1] && bx[2] >= g.lim[2] && bx[0] <= g.lim[3] &&
              bx[1] <= g.lim[4] && bx[2] <= g.lim[5];
    return ok && (sc > g.score_thresh);
}

// order-preserving compaction of a frame's kept winners (thread k = winner k) + the frame's count
__device__ __forceinline__ void compact_boxes(uint32_t keep, const float bx[7], float sc, int cls, TopkSmem &sm, float *__restrict__ boxes,
                                              float *__restrict__ scores, int32_t *__restrict__ labels, int32_t *__restrict__ n_out) {
    uint32_t tot;
    uint32_t pos = block_excl_scan(keep, sm.scan, &tot);
    if (keep) {
#pragma unroll
        for (int c = 0; c < 7; ++c) boxes[(size_t)pos * 7 + c] = bx[c];
        scores[pos] = sc;
        labels[pos] = cls;
    }
    if (threadIdx.x == 0) *n_out = (int32_t)tot;
}

__global__ void __launch_bounds__(1024) decode_kernel(DecodeParams q, const float *__restrict__ s1,
                                                      const int32_t *__restrict__ i1, float *__restrict__ boxes,
                                                      float *__restrict__ scores, int32_t *__restrict__ labels,
                                                      int32_t *__restrict__ n_out) {
    __shared__ TopkSmem sm;
    const int K = q.K;
    const int bsmp = blockIdx.x;
    s1 += (size_t)bsmp * q.num_class * K;
    i1 += (size_t)bsmp * q.num_class * K;
    boxes += (size_t)bsmp * K * 7;
    scores += (size_t)bsmp * K;
    labels += (size_t)bsmp * K;
    n_out += bsmp;
    q.center = q.center.sample(bsmp, q.sample_stride);
    q.center_z = q.center_z.sample(bsmp, q.sample_stride);
    q.dim = q.dim.sample(bsmp, q.sample_stride);
    q.rot = q.rot.sample(bsmp, q.sample_stride);
    merge_class_lists(s1, q.num_class, K, sm);
    const int k = threadIdx.x;
    float bx[7];
    float sc = 0.f;
    int cls = 0;
    uint32_t keep = 0;
    if (k < K) {
        unsigned long long p = sm.packed[k];
        sc = float_unkey((uint32_t)(p >> 32));
        const int i2 = (int)(~(uint32_t)p);
        cls = i2 / K;
        const int ind = i1[i2];
        const float r[8] = {q.center.at(ind, 0), q.center.at(ind, 1), q.center_z.at(ind, 0), q.dim.at(ind, 0),
                            q.dim.at(ind, 1),    q.dim.at(ind, 2),    q.rot.at(ind, 0),      q.rot.at(ind, 1)};
        keep = decode_box(q.g, ind, sc, r, bx) ? 1u : 0u;
    }
    __syncthreads();
    compact_boxes(keep, bx, sc, cls, sm, boxes, scores, labels, n_out);
}

// ---- the pipeline cut at the peaks ----
// the selection alone: one workgroup per frame merges the per-class lists and writes the K winners in their final order
__global__ void __launch_bounds__(1024) peaks_kernel(int num_class, int K, const float *__restrict__ s1, const int32_t *__restrict__ i1,
                                                     float *__restrict__ peak_score, int32_t *__restrict__ peak_cand,
                                                     int32_t *__restrict__ peak_ind) {
    __shared__ TopkSmem sm;
    const int bsmp = blockIdx.x;
    s1 += (size_t)bsmp * num_class * K;
    i1 += (size_t)bsmp * num_class * K;
    merge_class_lists(s1, num_class, K, sm);
    const int k = threadIdx.x;
    if (k < K) {
        const unsigned long long p = sm.packed[k];
        const int i2 = (int)(~(uint32_t)p);
        peak_score[(size_t)bsmp * K + k] = float_unkey((uint32_t)(p >> 32));
        peak_cand[(size_t)bsmp * K + k] = i2;
        peak_ind[(size_t)bsmp * K + k] = i1[i2];
    }
}

// row (peak * 9 + t) of the table = the hidden site at the peak's pixel + tap t's offset; column u = the shared map's row at that
// site + tap u's offset, -1 outside the image; a hidden site outside the image (or a pixel index that is no pixel) has no input at all
__global__ void __launch_bounds__(256) peak_rulebook_kernel(const int32_t *__restrict__ peak_ind, int n_peaks, int K, int h, int w,
                                                            int32_t *__restrict__ nbr) {
    const long long n_out = (long long)n_peaks * 9;
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_out) return;
    const int p = (int)(j / 9), t = (int)(j - (long long)p * 9);
    const int b = p / K;
    const int ind = peak_ind[p];
    const int sy = ind / w + t / 3 - 1, sx = ind % w + t % 3 - 1;
    const bool site = ind >= 0 && ind < h * w && (unsigned)sy < (unsigned)h && (unsigned)sx < (unsigned)w;
    int u = 0;
    for (int ky = 0; ky < 3; ++ky)
        for (int kx = 0; kx < 3; ++kx, ++u) {
            const int iy = sy - 1 + ky, ix = sx - 1 + kx;
            int32_t r = -1;
            if (site && (unsigned)iy < (unsigned)h && (unsigned)ix < (unsigned)w) r = (int32_t)(((long long)b * h + iy) * w + ix);
            nbr[(size_t)u * n_out + j] = r;
        }
}

// the branches' last 3 x 3 convolution at the peaks: reg[o] = bias[o] + sum over the taps whose hidden site is INSIDE the image (the
// convolution pads the hidden map with zeros: a site outside contributes nothing, whatever its row holds) of
// hidden[peak * 9 + t] . W[t][:, o]. A wave owns PP peaks and lane l the hidden channels 4l .. 4l + 3 of every 256-channel slab; the
// workgroup stages one (tap, slab) of the weight image in LDS at a time and every wave applies it to all its peaks (a wave per peak
// reading its weights from global memory moved the 73 KB image once per peak: 1.7 GB per 48 frames, 780 us). Fixed summation order:
// a lane-local fmaf chain over taps and channels, then a butterfly over the lanes.
template <int NR, int PP>
__global__ void __launch_bounds__(256) peak_regress_kernel(const int32_t *__restrict__ peak_ind, int n_peaks, int h, int w,
                                                           const float *__restrict__ hidden, int hid_ld, int c_hid,
                                                           const float *__restrict__ w_last, const float *__restrict__ bias, int n_reg,
                                                           float *__restrict__ reg) {
    __shared__ float wl[256 * NR];                 // [channel of the slab][NR]: columns past n_reg and channels past c_hid are zero
    const int lane = threadIdx.x & 63;
    const int p0 = (blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * PP;
    int py[PP], px[PP];
#pragma unroll
    for (int i = 0; i < PP; ++i) {
        const int ind = p0 + i < n_peaks ? peak_ind[p0 + i] : -1;
        const bool pixel = ind >= 0 && ind < h * w;
        py[i] = pixel ? ind / w : -4;              // (-4: every tap of the peak is outside)
        px[i] = pixel ? ind % w : -4;
    }
    float acc[PP][NR];
#pragma unroll
    for (int i = 0; i < PP; ++i)
#pragma unroll
        for (int o = 0; o < NR; ++o) acc[i][o] = 0.f;
    for (int t = 0; t < 9; ++t) {
        const int dy = t / 3 - 1, dx = t % 3 - 1;
        for (int cb = 0; cb < c_hid; cb += 256) {
            __syncthreads();                       // the previous stage's readers are done
            for (int i = threadIdx.x; i < 256 * NR; i += blockDim.x) {
                const int c = cb + i / NR, o = i % NR;
                wl[i] = (c < c_hid && o < n_reg) ? w_last[((size_t)t * c_hid + c) * n_reg + o] : 0.f;
            }
            __syncthreads();
            const int c0 = cb + lane * 4;
            if (c0 < c_hid) {
                float wr[4][NR];
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int o = 0; o < NR; ++o) wr[j][o] = wl[(lane * 4 + j) * NR + o];
#pragma unroll
                for (int i = 0; i < PP; ++i) {
                    if (!((unsigned)(py[i] + dy) < (unsigned)h && (unsigned)(px[i] + dx) < (unsigned)w)) continue;      // (wave-uniform)
                    const float4 hv = *reinterpret_cast<const float4 *>(hidden + ((size_t)(p0 + i) * 9 + t) * hid_ld + c0);
                    const float hx[4] = {hv.x, hv.y, hv.z, hv.w};
#pragma unroll
                    for (int j = 0; j < 4; ++j)
#pragma unroll
                        for (int o = 0; o < NR; ++o) acc[i][o] = fmaf(hx[j], wr[j][o], acc[i][o]);
                }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < PP; ++i)
#pragma unroll
        for (int o = 0; o < NR; ++o) {
            float v = acc[i][o];
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
            if (lane == 0 && p0 + i < n_peaks && o < n_reg) reg[(size_t)(p0 + i) * n_reg + o] = v + bias[o];
        }
}

struct PeakDecodeParams {
    int K, n_reg;
    int off[4];         // first channel of center, center_z, dim, rot among the n_reg regression values
    DecodeGeom g;
};

__global__ void __launch_bounds__(1024) decode_peaks_kernel(PeakDecodeParams q, const float *__restrict__ peak_score,
                                                            const int32_t *__restrict__ peak_cand, const int32_t *__restrict__ peak_ind,
                                                            const float *__restrict__ reg, float *__restrict__ boxes,
                                                            float *__restrict__ scores, int32_t *__restrict__ labels,
                                                            int32_t *__restrict__ n_out) {
    __shared__ TopkSmem sm;
    const int K = q.K;
    const int bsmp = blockIdx.x;
    const size_t o = (size_t)bsmp * K;
    const int k = threadIdx.x;
    float bx[7];
    float sc = 0.f;
    int cls = 0;
    uint32_t keep = 0;
    if (k < K) {
        sc = peak_score[o + k];
        cls = peak_cand[o + k] / K;
        const float *v = reg + (o + k) * q.n_reg;
        const float r[8] = {v[q.off[0]], v[q.off[0] + 1], v[q.off[1]], v[q.off[2]], v[q.off[2] + 1], v[q.off[2] + 2], v[q.off[3]], v[q.off[3] + 1]};
        keep = decode_box(q.g, peak_ind[o + k], sc, r, bx) ? 1u : 0u;
    }
    compact_boxes(keep, bx, sc, cls, sm, boxes + o * 7, scores + o, labels + o, n_out + bsmp);
}

static void fill_geom(DecodeGeom &g, int w, float feature_map_stride, const float voxel_xy[2], const float range_lo_xy[2],
                      const float limit_range[6], float score_thresh) {
    g.w = w;
    g.stride = feature_map_stride; g.vx = voxel_xy[0]; g.vy = voxel_xy[1];
    g.lox = range_lo_xy[0]; g.loy = range_lo_xy[1];
    for (int i = 0; i < 6; ++i) g.lim[i] = limit_range[i];
    g.score_thresh = score_thresh;
}

// what cpd_center_decode refuses, the entry points cut from it refuse with the same codes
static int check_topk_shape(int batch, int num_class, int h, int w, int k) {
    if (batch <= 0 || num_class <= 0 || h <= 0 || w <= 0 || k <= 0) return CPD_ERR_ARG;
    const long long hw = (long long)h * w;
    if (k > 1024 || k > hw || (long long)num_class * k > (1 << 24) || hw >= (1ll << 31)) return CPD_ERR_UNSUPPORTED;
    return CPD_OK;
}

// the per-class top-K candidates of cpd_center_decode and cpd_center_peaks: [batch][num_class][k] scores, then their pixels
struct TopkLayout { size_t score, index, total; };
TopkLayout topk_layout(int batch, int num_class, int k) {
    const size_t bytes = (size_t)batch * num_class * k * 4;
    Carve c;
    TopkLayout l;
    l.score = c.take(bytes);
    l.index = c.take(bytes);
    l.total = c.o;
    return l;
}

}  // namespace

extern "C" size_t cpd_center_decode_workspace_bytes(int batch, int num_class, int hw, int k) {
    if (batch <= 0 || num_class <= 0 || hw <= 0 || k <= 0) return 0;
    return topk_layout(batch, num_class, k).total;
}

extern "C" int cpd_center_decode(const float *hm, const float *center, const float *center_z, const float *dim,
                                 const float *rot, int batch, long long sample_stride, int pix_stride, int ch_stride,
                                 int num_class, int h, int w, int k,
                                 float feature_map_stride, const float voxel_xy[2], const float range_lo_xy[2],
                                 const float limit_range[6], float score_thresh, float *boxes, float *scores,
                                 int32_t *labels, int32_t *n_out, void *workspace, size_t workspace_bytes,
                                 cpd_stream_t stream) {
    if (!hm || !center || !center_z || !dim || !rot || !boxes || !scores || !labels || !n_out || !workspace ||
        !voxel_xy || !range_lo_xy || !limit_range)
        return CPD_ERR_ARG;
    if (const int rc = check_topk_shape(batch, num_class, h, w, k)) return rc;
    const long long hw = (long long)h * w;
    const TopkLayout l = topk_layout(batch, num_class, k);
    if (workspace_bytes < l.total) return CPD_ERR_WORKSPACE;
    hipStream_t s = cpd_s(stream);
    float *s1 = ws_at<float>(workspace, l.score);
    int32_t *i1 = ws_at<int32_t>(workspace, l.index);
    topk_class_kernel<<<dim3(num_class, batch), 1024, 0, s>>>(MapView{hm, pix_stride, ch_stride}, sample_stride, num_class,
                                                              (int)hw, k, s1, i1);
    DecodeParams q;
    q.center = MapView{center, pix_stride, ch_stride};
    q.center_z = MapView{center_z, pix_stride, ch_stride};
    q.dim = MapView{dim, pix_stride, ch_stride};
    q.rot = MapView{rot, pix_stride, ch_stride};
    q.sample_stride = sample_stride;
    q.num_class = num_class; q.h = h; q.w = w; q.K = k;
    fill_geom(q.g, w, feature_map_stride, voxel_xy, range_lo_xy, limit_range, score_thresh);
    decode_kernel<<<batch, 1024, 0, s>>>(q, s1, i1, boxes, scores, labels, n_out);
    return cpd_check_launch();
}

extern "C" size_t cpd_center_peaks_workspace_bytes(int batch, int num_class, int hw, int k) {
    return cpd_center_decode_workspace_bytes(batch, num_class, hw, k);
}

extern "C" int cpd_center_peaks(const float *hm, int batch, long long sample_stride, int pix_stride, int ch_stride, int num_class, int h,
                                int w, int k, float *peak_score, int32_t *peak_cand, int32_t *peak_ind, void *workspace,
                                size_t workspace_bytes, cpd_stream_t stream) {
    if (!hm || !peak_score || !peak_cand || !peak_ind || !workspace) return CPD_ERR_ARG;
    if (const int rc = check_topk_shape(batch, num_class, h, w, k)) return rc;
    const int hw = h * w;
    const TopkLayout l = topk_layout(batch, num_class, k);
    if (workspace_bytes < l.total) return CPD_ERR_WORKSPACE;
    hipStream_t s = cpd_s(stream);
    float *s1 = ws_at<float>(workspace, l.score);
    int32_t *i1 = ws_at<int32_t>(workspace, l.index);
    topk_class_kernel<<<dim3(num_class, batch), 1024, 0, s>>>(MapView{hm, pix_stride, ch_stride}, sample_stride, num_class, hw, k, s1, i1);
    peaks_kernel<<<batch, 1024, 0, s>>>(num_class, k, s1, i1, peak_score, peak_cand, peak_ind);
    return cpd_check_launch();
}

extern "C" int cpd_peak_rulebook(const int32_t *peak_ind, int batch, int k, int h, int w, int32_t *nbr, cpd_stream_t stream) {
    if (!peak_ind || !nbr || batch <= 0 || k <= 0 || h <= 0 || w <= 0) return CPD_ERR_ARG;
    const long long hw = (long long)h * w;
    if (k > 1024 || k > hw || batch * hw >= (1ll << 31) || (long long)batch * k * 9 >= (1ll << 31)) return CPD_ERR_UNSUPPORTED;
    const long long n_out = (long long)batch * k * 9;
    peak_rulebook_kernel<<<cpd_div_up(n_out, 256), 256, 0, cpd_s(stream)>>>(peak_ind, batch * k, k, h, w, nbr);
    return cpd_check_launch();
}

extern "C" size_t cpd_center_decode_at_peaks_workspace_bytes(int batch, int k, int n_reg) {
    if (batch <= 0 || k <= 0 || n_reg <= 0) return 0;
    return cpd_align((size_t)batch * k * n_reg * 4);
}

extern "C" int cpd_center_decode_at_peaks(const float *peak_score, const int32_t *peak_cand, const int32_t *peak_ind, const float *hidden,
                                          int hidden_ld, int c_hid, const float *w_last, const float *bias, int n_reg,
                                          const int32_t reg_offsets[4], int batch, int num_class, int h, int w, int k,
                                          float feature_map_stride, const float voxel_xy[2], const float range_lo_xy[2],
                                          const float limit_range[6], float score_thresh, float *boxes, float *scores, int32_t *labels,
                                          int32_t *n_out, void *workspace, size_t workspace_bytes, cpd_stream_t stream) {
    if (!peak_score || !peak_cand || !peak_ind || !hidden || !w_last || !bias || !reg_offsets || !boxes || !scores || !labels || !n_out ||
        !workspace || !voxel_xy || !range_lo_xy || !limit_range || c_hid <= 0 || n_reg <= 0 || hidden_ld < c_hid)
        return CPD_ERR_ARG;
    if (const int rc = check_topk_shape(batch, num_class, h, w, k)) return rc;
    static const int width[4] = {2, 1, 3, 2};        // center, center_z, dim, rot
    for (int i = 0; i < 4; ++i)
        if (reg_offsets[i] < 0 || reg_offsets[i] + width[i] > n_reg) return CPD_ERR_ARG;
    // (16-byte row pieces; at most 16 regression values: the shipped heads have 8)
    if (n_reg > 16 || c_hid % 4 || hidden_ld % 4 || (((uintptr_t)hidden) & 15)) return CPD_ERR_UNSUPPORTED;
    if (workspace_bytes < cpd_center_decode_at_peaks_workspace_bytes(batch, k, n_reg)) return CPD_ERR_WORKSPACE;
    hipStream_t s = cpd_s(stream);
    float *reg = (float *)workspace;
    const int n_peaks = batch * k;
    // peaks per wave: 8 once that still gives every CU two workgroups, else 2 (small batches: more, shorter workgroups)
    const bool wide = n_peaks >= 16384;
    const int blocks = cpd_div_up(n_peaks, 4 * (wide ? 8 : 2));
#define CPD_PEAK_REGRESS(NR, PP) \
    peak_regress_kernel<NR, PP><<<blocks, 256, 0, s>>>(peak_ind, n_peaks, h, w, hidden, hidden_ld, c_hid, w_last, bias, n_reg, reg)
    if (n_reg <= 8) { if (wide) CPD_PEAK_REGRESS(8, 8); else CPD_PEAK_REGRESS(8, 2); }
    else { if (wide) CPD_PEAK_REGRESS(16, 8); else CPD_PEAK_REGRESS(16, 2); }
#undef CPD_PEAK_REGRESS
    PeakDecodeParams q;
    q.K = k; q.n_reg = n_reg;
    for (int i = 0; i < 4; ++i) q.off[i] = reg_offsets[i];
    fill_geom(q.g, w, feature_map_stride, voxel_xy, range_lo_xy, limit_range, score_thresh);
    decode_peaks_kernel<<<batch, 1024, 0, s>>>(q, peak_score, peak_cand, peak_ind, reg, boxes, scores, labels, n_out);
    return cpd_check_launch();
}
