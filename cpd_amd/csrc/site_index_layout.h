// site_index_layout.h -- memory layout of a site index (cpd_index_build / cpd_conv_outset) and the
// device lookup shared by the kernels that consume one: flags (256 B) | occupancy bitmap | per-word
// popcount prefix | scan spine | rank -> row permutation.
#pragma once
#include "common.h"

namespace {

struct IndexView {
    uint64_t *bitmap;
    uint32_t *base;
    uint32_t *bsum;
    int32_t *perm;    // rank -> row id
    int32_t *flags;   // [0]: 0 canonical, 1 perm in use, 2 external rank -> row map at [2..3] (index_order below)
    long long cells, words;
    size_t bytes;
};

static IndexView index_carve(void *mem, int batch, const int32_t shape[3], int n_cap) {
    IndexView v;
    Carve c;
    v.cells = (long long)batch * shape[0] * shape[1] * shape[2];
    v.words = (v.cells + 63) / 64;
    v.flags = ws_at<int32_t>(mem, c.take(256));
    v.bitmap = ws_at<uint64_t>(mem, c.take((size_t)v.words * 8));
    v.base = ws_at<uint32_t>(mem, c.take((size_t)v.words * 4));
    v.bsum = ws_at<uint32_t>(mem, c.take((size_t)scan_num_blocks(v.words) * 4));
    v.perm = ws_at<int32_t>(mem, c.take((size_t)(n_cap > 0 ? n_cap : 1) * 4));
    v.bytes = c.o;
    return v;
}

struct Grid {
    int32_t b, d, h, w;
    __host__ __device__ long long key(int bi, int z, int y, int x) const {
        return (((long long)bi * d + z) * h + y) * w + x;
    }
};

// Which rank -> row map an index uses is recorded in its own flags block and read on the device: flags[0] = 0 canonical
// (row id = rank), 1 the map stored in the index (cpd_index_build over an arbitrary-order list), 2 a caller-owned map whose
// device address sits in flags[2..3] (cpd_index_set_order: rows of a level re-ordered after the index was built).
__device__ __forceinline__ const int32_t *index_order(const int32_t *__restrict__ flags, const int32_t *__restrict__ own_perm) {
    const int f = flags[0];
    if (f == 0) return nullptr;
    if (f == 1) return own_perm;
    return *reinterpret_cast<const int32_t *const *>(flags + 2);
}

__device__ __forceinline__ int32_t site_lookup(const uint64_t *__restrict__ bitmap, const uint32_t *__restrict__ base,
                                               const int32_t *__restrict__ perm, long long key) {
    uint64_t w = bitmap[key >> 6];
    uint64_t bit = 1ull << (key & 63);
    if (!(w & bit)) return -1;
    int32_t r = (int32_t)(base[key >> 6] + __popcll(w & (bit - 1ull)));
    return perm ? perm[r] : r;
}

// ---- what a consumer may read (the index contract) -----------------------------------------------------------------------
// bitmap[w]  every word, always: the builders zero the whole bitmap first.
// bsum[b]    the number of sites before scan block b (SCAN_TILE words), every block, always.
// base[w]    the number of sites before word w -- defined for the words of a scan block that holds at least one site. An index
//            the batched voxelizer leaves behind (cpd_voxelize_batch_index / _canonical / _frames) has NO prefix entries for
//            blocks without a site: its scan visits touched blocks only (device_scan_touched); cpd_index_build and
//            cpd_conv_outset write all of them.
// So: a LOOKUP (site_lookup, the rulebook kernels) may use base[w] after it has found a bit in bitmap[w]; a RANK query at an
// arbitrary cell -- "how many sites lie before this key", whether or not the cell is occupied -- goes through index_rank_before,
// which answers from bsum[] where the word's block is empty. `n_total` is the index's site count (what the rank is past the
// last cell, and what closes the last block: the full scan leaves no total behind bsum[]).
__device__ __forceinline__ uint32_t index_rank_before(const uint64_t *__restrict__ bitmap, const uint32_t *__restrict__ base,
                                                      const uint32_t *__restrict__ bsum, long long words, long long key,
                                                      long long cells, uint32_t n_total) {
    if (key >= cells) return n_total;
    const long long wi = key >> 6;
    const uint64_t w = bitmap[wi];
    if (w == 0) {
        const long long b = wi / SCAN_TILE, nb = (words + SCAN_TILE - 1) / SCAN_TILE;
        const uint32_t start = bsum[b], next = b + 1 < nb ? bsum[b + 1] : n_total;
        if (next == start) return start;             // a block without sites: the rank anywhere inside it is the count at its start
    }
    return base[wi] + (uint32_t)__popcll(w & ((1ull << (key & 63)) - 1ull));
}

}  // namespace
