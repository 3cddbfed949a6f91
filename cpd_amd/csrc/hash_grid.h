// hash_grid.h -- the hashed uniform grid of the fixed-radius neighbour searches: outline.hip's DBSCAN (side eps, tag = frame)
// and ppscore.hip's traversal counts (side r, tag = traversal). Points are binned by floor((double)coord / side) per axis into
// an open-addressing table of (tag, cell) keys; per slot a count, then by one device_scan its range of `members`, which the
// fill kernel writes in cell order. A query walks the 27 cells around its own and decides every member by its float64 squared
// distance. Integer atomics only (slot claims, counts, cursors): the order of a cell's members varies from call to call, and
// nothing that is stored or compared may depend on it. Both users are built with -ffp-contract=off.
#pragma once
#include <math.h>

#include "common.h"

namespace {

constexpr unsigned long long GRID_EMPTY = ~0ull;

struct HashGrid {
    unsigned long long *keys;   // [slots]
    unsigned long long hmask;   // slots - 1
    int32_t *ccount;            // [slots]
    int2 *range;                // [slots] (first member, cursor); the cursor is the end of the cell once the fill has run
    int32_t *cell;              // [n_points] slot, -1 for a row that is not in the grid
    float4 *members;            // [n_points] (x, y, z, w) in cell order
    double side, r2;            // cell side, squared search radius (radius <= side)
};

// ---- host: size and layout ----
static inline unsigned long long grid_slots(long long n_points) {   // power of two >= max(1024, 2 n): a free slot always exists
    unsigned long long h = 1024;
    while (h < 2ull * (unsigned long long)n_points) h <<= 1;
    return h;
}
struct GridLayout {
    size_t keys, ccount, range, cell, members, scan;
    unsigned long long slots;
    HashGrid view(void *ws, double side, double r2) const {
        return HashGrid{ws_at<unsigned long long>(ws, keys), slots - 1, ws_at<int32_t>(ws, ccount), ws_at<int2>(ws, range),
                        ws_at<int32_t>(ws, cell), ws_at<float4>(ws, members), side, r2};
    }
};
static inline GridLayout grid_carve(Carve &c, long long n_points) {
    GridLayout L;
    L.slots = grid_slots(n_points);
    L.keys = c.take(L.slots * 8);
    L.ccount = c.take(L.slots * 4);
    L.range = c.take(L.slots * 8);
    L.cell = c.take((size_t)n_points * 4);
    L.members = c.take((size_t)n_points * 16);
    L.scan = c.take((size_t)scan_num_blocks((long long)L.slots) * 4);   // block sums of a scan over the slots (or anything shorter)
    return L;
}

// ---- device: keys, claim, probe, the 27-cell walk ----
__device__ __forceinline__ long long grid_cell(const HashGrid &g, float v) { return (long long)floor((double)v / g.side); }

// (tag, cx, cy, cz) with the cell coordinates taken modulo 2^18. Cells that alias modulo 2^18 share a slot, and so do their
// members: that costs distance tests, never a wrong answer, because every candidate is decided by its distance and not by
// its slot, and the 27 keys of one query stay distinct (they differ by at most 2 per axis), so no member is met twice. The
// tag fills bits 54..63 and is at most 1022 (1023 frames, 16 traversals), so no key equals GRID_EMPTY.
__device__ __forceinline__ unsigned long long grid_key(int tag, long long cx, long long cy, long long cz) {
    const unsigned long long m = (1ull << 18) - 1;
    return ((unsigned long long)tag << 54) | (((unsigned long long)cx & m) << 36) | (((unsigned long long)cy & m) << 18) |
           ((unsigned long long)cz & m);
}
__device__ __forceinline__ int grid_claim(const HashGrid &g, unsigned long long key) {   // the key's slot, taken if it is new
    unsigned long long s = mix64(key) & g.hmask;
    for (;;) {   // the table holds >= 2 slots per point: a free slot always exists
        const unsigned long long prev = atomicCAS(g.keys + s, GRID_EMPTY, key);
        if (prev == GRID_EMPTY || prev == key) return (int)s;
        s = (s + 1) & g.hmask;
    }
}
__device__ __forceinline__ int grid_find(const HashGrid &g, unsigned long long key) {    // the key's slot, or -1
    unsigned long long s = mix64(key) & g.hmask;
    for (;;) {
        const unsigned long long k = g.keys[s];
        if (k == key) return (int)s;
        if (k == GRID_EMPTY) return -1;
        s = (s + 1) & g.hmask;
    }
}

// every member of `tag` within the radius of (x, y, z), inclusive, in float64: fn(member) returns false to stop
template <class Fn>
__device__ __forceinline__ void grid_for_near(const HashGrid &g, int tag, float fx, float fy, float fz, Fn fn) {
    const double x = fx, y = fy, z = fz;
    const long long cx = grid_cell(g, fx), cy = grid_cell(g, fy), cz = grid_cell(g, fz);
    for (int dx = -1; dx <= 1; ++dx)
        for (int dy = -1; dy <= 1; ++dy)
            for (int dz = -1; dz <= 1; ++dz) {
                const int s = grid_find(g, grid_key(tag, cx + dx, cy + dy, cz + dz));
                if (s < 0) continue;
                const int2 rg = g.range[s];
                for (int m = rg.x; m < rg.y; ++m) {
                    const float4 p = g.members[m];
                    const double ex = x - (double)p.x, ey = y - (double)p.y, ez = z - (double)p.z;
                    if ((ex * ex + ey * ey) + ez * ez <= g.r2 && !fn(p)) return;
                }
            }
}

// ---- build: Src()(i, tag, x, y, z, w) gives row i's tag, position and payload, or false for a row that is not in the grid ----
template <class Src>
__global__ void __launch_bounds__(256) grid_insert_kernel(HashGrid g, int n_points, Src src) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_points) return;
    int tag;
    float x, y, z, w;
    if (!src(i, tag, x, y, z, w)) {
        g.cell[i] = -1;
        return;
    }
    const int s = grid_claim(g, grid_key(tag, grid_cell(g, x), grid_cell(g, y), grid_cell(g, z)));
    g.cell[i] = s;
    atomicAdd(g.ccount + s, 1);
}

template <class Src>
__global__ void __launch_bounds__(256) grid_fill_kernel(HashGrid g, int n_points, Src src) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_points) return;
    const int s = g.cell[i];
    if (s < 0) return;
    int tag;
    float x, y, z, w;
    src(i, tag, x, y, z, w);
    g.members[atomicAdd(&g.range[s].y, 1)] = make_float4(x, y, z, w);
}

// clear, insert, prefix over the slots, fill; scan_ws: GridLayout::scan
template <class Src>
static inline int grid_build(const HashGrid &g, int n_points, Src src, uint32_t *scan_ws, hipStream_t st) {
    const unsigned long long slots = g.hmask + 1;
    CPD_HIP_TRY(hipMemsetAsync(g.keys, 0xff, slots * 8, st));
    CPD_HIP_TRY(hipMemsetAsync(g.ccount, 0, slots * 4, st));
    if (n_points <= 0) return CPD_OK;
    const unsigned blocks = (unsigned)cpd_div_up(n_points, 256);
    grid_insert_kernel<<<blocks, 256, 0, st>>>(g, n_points, src);
    int2 *range = g.range;
    const int32_t *ccount = g.ccount;
    const int rc = device_scan(
        (long long)slots, [=] __device__(long long i) { return (uint32_t)ccount[i]; },
        [=] __device__(long long i, uint32_t, uint32_t pre) { range[i] = make_int2((int)pre, (int)pre); }, scan_ws, nullptr, -1,
        st);
    if (rc != CPD_OK) return rc;
    grid_fill_kernel<<<blocks, 256, 0, st>>>(g, n_points, src);
    return cpd_check_launch();
}

}  // namespace
