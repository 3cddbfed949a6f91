/*
 * cpd_hip.h -- C-ABI of libcpd_hip.so: the MI355X (gfx950) implementation of CPD's detection
 * hot path  voxelize -> sparse 3D conv backbone -> BEV dense head -> rotated NMS.
 *
 * This is the drop-in boundary: plain pointers and sizes, no torch types. Every DATA pointer is
 * a DEVICE pointer unless its comment says HOST; small geometry arrays (voxel size, ranges,
 * shapes, kernel/stride/pad triples) are HOST arrays read at call time. All functions enqueue on
 * `stream` (a hipStream_t passed as void*) and return without synchronising unless stated. They
 * never allocate device memory and never call exit(): workspaces are caller-owned (size queries
 * below) so a whole frame can be captured into a hipGraph. Return value: CPD_OK (0) or a
 * negative CPD_ERR_* code (the reference's exit(-1) CHECK_INPUT macros, iou3d_nms.cpp:14-26,
 * become error codes; the Python shim turns them into exceptions).
 *
 * Each entry point cites the reference interface it replaces (path:line under /root/reference;
 * [SPCONV] = behaviour of the un-vendored dependency spconv-cu111==2.1.22 as used at that call
 * site). INTEGRATION.md shows the reference-side binding for each.
 */
#ifndef CPD_HIP_H
#define CPD_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void *cpd_stream_t; /* hipStream_t; NULL = the default stream, as the reference uses */

#define CPD_OK 0
#define CPD_ERR_ARG (-1)         /* bad argument (null pointer, non-positive size, bad shape) */
#define CPD_ERR_WORKSPACE (-2)   /* caller workspace smaller than the *_bytes() query         */
#define CPD_ERR_LAUNCH (-3)      /* HIP runtime reported an error; see cpd_last_hip_error()   */
#define CPD_ERR_UNSUPPORTED (-4) /* size outside the supported envelope (e.g. >2^31 cells)    */

const char *cpd_version(void);
/* Diagnostics: with the log enabled every conv / weight-gradient call notes the kernel instantiation it launched
 * ("rowwave_conv_f16s_kernel<64,2>", "wgrad_f16_kernel<128,128>", ...). dump writes "name count" lines and returns the bytes
 * needed; enable(…) also clears the log. Host only; tests use it to assert which kernels a full-size step runs.            */
void cpd_launch_log_enable(int on);
void cpd_launch_log_note(const char *kernel);
size_t cpd_launch_log_dump(char *buf, size_t cap);
int cpd_last_hip_error(void); /* hipError_t of the last CPD_ERR_LAUNCH on this thread */

/* ===== B1. Voxelizer (+ fused MeanVFE) =====================================================
 * Replaces VoxelGeneratorWrapper.generate -> [SPCONV] Point2VoxelCPU3d.point_to_voxel
 * (cpd/datasets/processor/data_processor.py:14-59, driver l.128-183) and MeanVFE.forward
 * (cpd/models/backbones_3d/vfe/mean_vfe.py:41-43).
 * Semantics: serial first-appearance voxel order, first `max_points` points of a voxel in
 * point order, fp32 floor((p-lo)/vs), upper bound exclusive, voxel cap `max_voxels`.
 */
/* grid = round((hi-lo)/vs) in fp32, returned (z,y,x). HOST in, HOST out. */
int cpd_voxel_grid_size(const float vsize_xyz[3], const float range_xyz[6], int32_t grid_zyx[3]);
/* = cpd_voxelize_batch_workspace_bytes(n_points, 1, ...); 0 for bad arguments or a grid of >= 2^31 cells. */
size_t cpd_voxelize_workspace_bytes(int n_points, int max_points, int max_voxels,
                                    const float vsize_xyz[3], const float range_xyz[6]);
/* One frame: cpd_voxelize_batch (below) with n_frames = 1, the same kernels. What differs is the boundary: coord_cols and
 * batch_idx shape the coordinates, and n_voxels is ONE int (nothing is written behind it).
 * points [n_points, c] f32 (x,y,z,...). Outputs sized for cap = min(max_voxels, n_points) rows:
 *   voxels        [cap, max_points, c] f32, zero padded            (may be NULL)
 *   coords        [cap, coord_cols] i32; coord_cols 3 -> (z,y,x), 4 -> (batch_idx,z,y,x)
 *                 (the pad of collate_batch, cpd/datasets/dataset.py:264)
 *   num_points    [cap] i32
 *   mean_features [cap, c] f32 = sum_p voxels / max(num,1)         (may be NULL)
 *   n_voxels      device i32 scalar                                                         */
int cpd_voxelize(const float *points, int n_points, int c, const float vsize_xyz[3],
                 const float range_xyz[6], int max_points, int max_voxels, int batch_idx,
                 int coord_cols, float *voxels, int32_t *coords, int32_t *num_points,
                 float *mean_features, int32_t *n_voxels, void *workspace, size_t workspace_bytes,
                 cpd_stream_t stream);

/* All frames of a batch in one set of launches. `points` [frame_offsets[n_frames], c] holds the
 * frames back to back; `frame_offsets` is a HOST array [n_frames + 1] (frame f = rows
 * [off[f], off[f+1])), n_frames <= 64. Per frame the result is exactly cpd_voxelize's (same
 * first-appearance order, max_voxels cap, max_points per voxel); rows of frame f follow those of
 * frame f-1, coords are always (b,z,y,x) with b = f. n_voxels: device int32 [n_frames + 1] =
 * voxels per frame, then their sum. Outputs need min(n_frames*max_voxels, n_total) rows. */
size_t cpd_voxelize_batch_workspace_bytes(int n_total, int n_frames, int max_points_per_voxel,
                                          int max_voxels, const float vsize_xyz[3],
                                          const float range_xyz[6]);
int cpd_voxelize_batch(const float *points, const int32_t *frame_offsets, int n_frames, int c,
                       const float vsize_xyz[3], const float range_xyz[6], int max_points_per_voxel,
                       int max_voxels, float *voxels, int32_t *coords, int32_t *num_points,
                       float *mean_features, int32_t *n_voxels, void *workspace, size_t workspace_bytes,
                       cpd_stream_t stream);
/* cpd_voxelize_batch that builds its occupancy bitmap, popcount prefix and rank -> row map INSIDE the caller's site index
 * (cpd_index_bytes(n_frames, {grid_z + z_extra, grid_y, grid_x}, n_total) bytes) instead of its own workspace: the index is
 * then the level-0 site index of the voxel list (what cpd_index_build would produce from `coords`) at no extra cost.
 * z_extra = 1 gives the backbone's sparse_shape = grid_size[::-1] + [1,0,0] (spconv_backbone.py:412). Voxels beyond a
 * frame's max_voxels cap are not sites (their lookups return -1). */
int cpd_voxelize_batch_index(const float *points, const int32_t *frame_offsets, int n_frames, int c,
                             const float vsize_xyz[3], const float range_xyz[6], int max_points_per_voxel,
                             int max_voxels, float *voxels, int32_t *coords, int32_t *num_points,
                             float *mean_features, int32_t *n_voxels, void *workspace, size_t workspace_bytes,
                             void *index, size_t index_bytes, int z_extra, cpd_stream_t stream);
/* cpd_voxelize_batch_index with the voxel rows in CANONICAL order -- ascending (frame, z, y, x) = the rank of the voxel's cell in
 * the occupancy bitmap -- instead of first appearance. Same voxels, same points per voxel (the max_points smallest point indices),
 * same means; only the row order differs, the site index left behind is canonical (row = rank, no map) and the first-appearance
 * scan over the points is not run. The order at the B1 boundary (Point2VoxelCPU3d) is first appearance: this form is for hosts
 * that consume the rows themselves (CenterPointEngine). The max_voxels cap is defined on first-appearance order and is NOT
 * applied here: n_voxels [n_frames + 1] reports the true counts, a caller that sees a frame above its cap falls back to
 * cpd_voxelize_batch_index. Outputs need min(n_frames * max_voxels, n_total) rows as there (a frame above the cap may exceed
 * that: check the workspace-sized capacity n_total instead when caps can bind). */
int cpd_voxelize_batch_canonical(const float *points, const int32_t *frame_offsets, int n_frames, int c,
                                 const float vsize_xyz[3], const float range_xyz[6], int max_points_per_voxel,
                                 int max_voxels, float *voxels, int32_t *coords, int32_t *num_points,
                                 float *mean_features, int32_t *n_voxels, void *workspace, size_t workspace_bytes,
                                 void *index, size_t index_bytes, int z_extra, cpd_stream_t stream);
/* cpd_voxelize_batch / _index / _canonical for frames that sit in SEPARATE device allocations (clouds arrive one by one from the
 * dataloader, data_processor.py:43-59 is called per frame): frame_points = HOST array of n_frames device pointers, frame f holding
 * frame_offsets[f + 1] - frame_offsets[f] rows of c floats. No concatenated copy of the batch's points is needed (153 MB at 48 frames).
 * index = NULL: cpd_voxelize_batch; index != NULL: cpd_voxelize_batch_index (canonical = 0) or cpd_voxelize_batch_canonical (1). */
int cpd_voxelize_batch_frames(const float *const *frame_points, const int32_t *frame_offsets, int n_frames, int c,
                              const float vsize_xyz[3], const float range_xyz[6], int max_points, int max_voxels,
                              float *voxels, int32_t *coords, int32_t *num_points, float *mean_features,
                              int32_t *n_voxels, void *workspace, size_t workspace_bytes, void *index,
                              size_t index_bytes, int z_extra, int canonical, cpd_stream_t stream);

/* ===== B2. Sparse convolution ==============================================================
 * Replaces [SPCONV] SparseConvTensor / SubMConv3d / SparseConv3d / .dense() as called from
 * cpd/models/backbones_3d/spconv_backbone.py:17-21,108-115,414-455,524-529 and
 * cpd/models/backbones_2d/map_to_bev/height_compression.py:136-138.
 *
 * Site index: a dense occupancy bitmap over (batch, z, y, x) plus a popcount prefix, giving
 * coordinate -> row lookup and, for free, the canonical ascending (b,z,y,x) order of a site set.
 * Rulebook: output-stationary neighbour table nbr[kv][n_out] (i32, -1 = no input), tap index
 * t = (tz*kH + ty)*kW + tx as in the spconv-2.x weight layout (Cout,kD,kH,kW,Cin). The same
 * table is the `indice_dict` entry a SparseConvTensor caches per indice_key.
 */
size_t cpd_index_bytes(int batch, const int32_t shape_zyx[3], int n_capacity);
/* Build the index of `indices` [n,4] i32 (b,z,y,x) (any order; row ids = positions). */
int cpd_index_build(const int32_t *indices, int n, int batch, const int32_t shape_zyx[3],
                    void *index, size_t index_bytes, cpd_stream_t stream);
/* Row order of a level. cpd_order_rows_by_taps: for the canonical-order site list `indices` [n][4] of a level and its site
 * index, a permutation that sorts the rows of every chunk of `chunk_rows` consecutive rows (1024, 4096, 8192 or 16384) by their
 * neighbour pattern under the sub-manifold kernel `ksize` (<= 32 taps): new_to_old [n], old_to_new [n], and (optional)
 * indices_out [n][4] = the site list in the new order. Rows ordered this way make cpd_gather_conv's 16-row tap skipping nearly
 * exact (executed / useful MFMAs 1.3-1.55 -> 1.06-1.12 on Waymo-shape levels) at unchanged cache locality. workspace:
 * cpd_order_rows_by_taps_workspace_bytes(n) = max(n, 1) * 4 bytes (one word per row, not rounded up). cpd_index_set_order installs a caller-owned rank -> row map (old_to_new; NULL = canonical again) in a site index:
 * every lookup through that index (cpd_rulebook_subm / _conv, cpd_voxel_query_index) then returns rows in the new order, so a
 * level is re-ordered by passing its site list in the new order and installing the map -- no kernel sees a difference. The map
 * must outlive the index's use. */
size_t cpd_order_rows_by_taps_workspace_bytes(int n);
int cpd_order_rows_by_taps(const int32_t *indices, int n, int batch, const int32_t shape_zyx[3],
                           const int32_t ksize[3], const void *index, int chunk_rows, int32_t *new_to_old,
                           int32_t *old_to_new, int32_t *indices_out, void *workspace, size_t workspace_bytes,
                           cpd_stream_t stream);
int cpd_index_set_order(void *index, const int32_t *rank_to_row, cpd_stream_t stream);
/* Brick order of a level (round 4; any row order is a valid SparseConvTensor, spconv_backbone.py:502-558 never reads one): rows
 * sorted by (b, z, y / brick_y, x / brick_x, y, x) -- brick_y x brick_x bricks of one z-plane, computed WITHOUT a sort from rank
 * queries on the level's canonical site index -- and then, inside every tile of `tile_rows` (128 or 256) consecutive rows of that order, by their 27-bit
 * sub-manifold neighbour pattern (what cpd_order_rows_by_taps does per chunk). A tile of 128 output rows then touches ~2.9 distinct
 * input rows per row instead of 4.5 (canonical) or 8.8 (4096-row pattern chunks): what cpd_gather_conv_planned stages in LDS.
 * `indices` [n][4]: the CANONICAL list of the level, `index`: its canonical index. Outputs as cpd_order_rows_by_taps.
 * workspace: cpd_order_rows_bricks_workspace_bytes(n) bytes. */
size_t cpd_order_rows_bricks_workspace_bytes(int n);
int cpd_order_rows_bricks(const int32_t *indices, int n, int batch, const int32_t shape_zyx[3], const void *index,
                          int brick_y, int brick_x, int tile_rows, int32_t *new_to_old, int32_t *old_to_new, int32_t *indices_out,
                          void *workspace, size_t workspace_bytes, cpd_stream_t stream);
/* SubMConv3d rulebook: output set == input set, same order; tap t reads coord + t - k/2.
 * tapmask (optional, u32 [ceil(n/16)], kernel volume <= 32): bit t of word s is set iff some row
 * of the 16-row group s has a neighbour at tap t -- lets cpd_gather_conv skip empty
 * (row group, tap) pairs without touching nbr. */
int cpd_rulebook_subm(const int32_t *indices, int n, int batch, const int32_t shape_zyx[3],
                      const int32_t ksize[3], const void *index, int32_t *nbr, uint32_t *tapmask,
                      cpd_stream_t stream);
/* Row plan of a 3 x 3 x 3 sub-manifold rulebook nbr[27][n_out] (round 4): per tile of 128 consecutive output rows and per dz group of
 * nine taps (tap = (dz * 3 + dy) * 3 + dx; the three groups read three different z-planes and share no input row)
 * (tile_rows = 128 or 256: the rows of one workgroup of cpd_gather_conv_planned)
 *   ulist [tiles][3][9 * tile_rows] i32   the distinct input rows the group touches (any order), `count` of them;
 *   slots [tiles][27][tile_rows] u16   per (tap, row of the tile): position of nbr[tap][row] in its group's list, 0xffff = no neighbour;
 *   count [tiles][4]       i32   the three list lengths and their sum.
 * cpd_rulebook_plan_bytes(n_out, which): bytes of slots (0), ulist (1), count (2). Any row order is planned correctly. */
size_t cpd_rulebook_plan_bytes(int n_out, int tile_rows, int which);
int cpd_rulebook_plan(const int32_t *nbr, int kv, int n_out, int tile_rows, uint16_t *slots, int32_t *ulist, int32_t *count,
                      cpd_stream_t stream);
/* cpd_rulebook_subm / cpd_rulebook_conv for a CHUNK-ORDERED output level (cpd_order_rows_by_taps, chunk_rows = 4096): out_canonical
 * [n_out][4] = the level's canonical site list, out_old_to_new [n_out] = its order (NULL = canonical). Gives, bit for bit, the table and
 * tap masks the plain builders give over the re-ordered list, but walks every chunk in canonical order (neighbouring lanes read the
 * same bitmap words) and re-orders it in LDS: a tap-ordered level cost the plain builder 2.2x a canonical one. 3 x 3 x 3 kernels. */
int cpd_rulebook_chunk_ordered(const int32_t *out_canonical, const int32_t *out_old_to_new, int n_out, int batch,
                               const int32_t in_shape[3], const int32_t ksize[3], const int32_t stride[3],
                               const int32_t pad[3], const void *in_index, int chunk_rows, int32_t *nbr, uint32_t *tapmask,
                               cpd_stream_t stream);
/* out_shape = (in + 2*pad - k)/stride + 1. HOST only. */
int cpd_conv_out_shape(const int32_t in_shape[3], const int32_t ksize[3], const int32_t stride[3],
                       const int32_t pad[3], int32_t out_shape[3]);
/* SparseConv3d output set: marks every output coordinate reached by an active input, builds the
 * OUTPUT site index in `out_index` (sized by cpd_index_bytes(batch, out_shape, capacity)) and
 * writes the number of active outputs to the device scalar n_out.                           */
int cpd_conv_outset(const int32_t *in_indices, int n_in, int batch, const int32_t in_shape[3],
                    const int32_t ksize[3], const int32_t stride[3], const int32_t pad[3],
                    void *out_index, size_t out_index_bytes, int32_t *n_out, cpd_stream_t stream);
/* Write the index's sites as [n,4] i32 rows in canonical ascending (b,z,y,x) order. */
int cpd_index_emit(const void *index, int batch, const int32_t shape_zyx[3], int32_t *indices,
                   int n_capacity, cpd_stream_t stream);
/* SparseConv3d rulebook: nbr[t][o] = input row at o*stride - pad + t. */
int cpd_rulebook_conv(const int32_t *out_indices, int n_out, int batch, const int32_t in_shape[3],
                      const int32_t ksize[3], const int32_t stride[3], const int32_t pad[3],
                      const void *in_index, int32_t *nbr, uint32_t *tapmask, cpd_stream_t stream);

/* Weights for cpd_gather_conv: pack a dense [kv][c_in][c_out] f32 tensor (device) into the
 * MFMA-fragment order the kernel streams (zero padded to multiples of 16). One buffer holds every image the conv may run on: the
 * fp32 image; for c_in % 32 == 0 the split-bf16 and split-fp16 images (the latter pre-scaled per output column by a power of two,
 * followed by the descale factors); for c_in == 16 the K = 16 split-fp16 image Ph16[t][g][n][hi 4 | lo 4] + its descale factors
 * (round 3: 16-channel pair rows, CPD_GC_IN_PAIRS). cpd_packed_weight_floats sizes the buffer; every packer (this one, the adjoint
 * one, the batched one) writes every image the buffer has, bit for bit alike.                                                   */
size_t cpd_packed_weight_floats(int kv, int c_in, int c_out);
int cpd_pack_weight(const float *w_kio, int kv, int c_in, int c_out, float *packed,
                    cpd_stream_t stream);
/* The one GEMM-shaped kernel of the path (fp32 MFMA, exact fp32 fma chain):
 *   out[j, :] = act( (sum_t W[t]^T . in[nbr[t][j], :]) * scale + shift + residual[j, :] )
 * Used for SubMConv3d / SparseConv3d (rulebook from above, bias/eval-BatchNorm1d folded into
 * scale/shift, SparseBasicBlock residual + ReLU fused: spconv_backbone.py:100-136) and, with a
 * dense pixel rulebook, for every Conv2d/ConvTranspose2d(+BN+ReLU) of BaseBEVBackbone
 * (cpd/models/backbones_2d/base_bev_backbone.py:31-59) and CenterHead
 * (cpd/models/dense_heads/center_head.py:21-27,73-80) on channels-last maps.
 *   in   [n_in rows, in_ld floats per row], first c_in floats of a row are the features
 *   nbr  [kv][n_out] or NULL (kv must be 1: identity, i.e. a 1x1 conv / linear layer)
 *   tapmask: the rulebook's tap masks (see cpd_rulebook_subm) or NULL (every tap computed)
 *   scale, shift [c_out] or NULL (1 / 0); residual [n_out, res_ld] or NULL; relu 0/1
 *   out  [n_out, out_ld]; only columns [0, c_out) of each row are written
 *   out_row_map: NULL, or i32 destination rows. With out_col_group == 0 it is [n_out]: row j
 *                is written to row out_row_map[j]. With out_col_group = G > 0 the c_out columns
 *                are G-wide groups: column c of row j goes to row out_row_map[(c/G)*n_out + j],
 *                column c % G -- one launch computes the k*k taps of ConvTranspose2d(k, s=k)
 *                (base_bev_backbone.py:52-56) and interleaves them into the upsampled map.
 *   flags: 0 or CPD_GC_DENSE (a performance hint only; results are identical).               */
int cpd_gather_conv(const float *in, int in_ld, int n_in, int c_in, const float *packed_w,
                    const int32_t *nbr, const uint32_t *tapmask, int kv, int n_out, int c_out, const float *scale,
                    const float *shift, const float *residual, int res_ld, int relu, float *out,
                    int out_ld, const int32_t *out_row_map, int out_col_group, int flags,
                    cpd_stream_t stream);
#define CPD_GC_DENSE 1
/* allow the split-bf16 matrix path: fp32 operands split exactly into 3 bf16 terms, 6 partial
 * products accumulated in fp32 (error <= 2^-22 relative per product, i.e. fp32-level); used for
 * dense layers with c_in % 32 == 0 and c_out % 64 == 0 */
#define CPD_GC_BF16X3 2 /* (CPD_GC_DENSE: the rulebook has (almost) no -1 entries -- prefer the LDS-tiled
                          workgroup kernel over the tap-skipping wave kernel) */
/* allow the split-fp16 matrix path instead: fp32 operands written as h + l, two fp16 terms (2 x 11 bits + sign: x to
 * 2^-24 relative, or 2^-25 absolute below 0.5), 3 partial products (hh, hl, lh) accumulated in fp32 -- fp32-level error at
 * half the matrix work of CPD_GC_BF16X3. fp16's range: an input of magnitude >= 65504 gives inf / NaN (0 behind a ReLU
 * epilogue) UNLESS the call comes with its input's absmax block (cpd_gather_conv_ranged / cpd_conv3x3_rows_ranged below: the
 * input is then pre-scaled by a power of two, exact at any magnitude); weights of any magnitude (pre-scaled per output column
 * by a power of two at pack time, undone exactly in the epilogue). Takes precedence over CPD_GC_BF16X3 when both are set. */
#define CPD_GC_F16X2 4
/* fp16-pair rows (engine-internal storage between f16x2 sparse layers; the boundary tensors stay fp32): a row keeps its 4 * C
 * bytes, but every 32-channel block holds the fp16 HIGH terms of its channels (64 B, natural order) followed by the fp16 LOW terms
 * (64 B) -- exactly the split x = h + l the f16x2 kernels make of a gathered fp32 row, made ONCE by the epilogue that produced
 * the row instead of by each of the <= 27 gathers of it. The partial products are those of fp32 rows (the accumulation order inside
 * a 32-channel block differs: fp32 rounding); a residual read back from pairs is h + l (x to 2^-24 relative). Same range as CPD_GC_F16X2 without an absmax block: |x| < 65504
 * (the engine's range guard re-runs such a step on fp32 rows with pre-scaling).
 *   CPD_GC_IN_PAIRS   `in` rows are pairs: needs CPD_GC_F16X2, c_in % 32 == 0, c_out % 32 == 0, kv <= 28, < 4 GB of input, no
 *                     in_absmax, not CPD_GC_DENSE (the row-wave kernel is the one that reads them) -- else CPD_ERR_UNSUPPORTED
 *                     -- or c_in == 16 (c_out 16 or 32; the wave kernel's K = 16 MFMA form): 16-channel pair rows hold, per group of
 *                     four channels, the four high terms (8 B) then the four low terms (8 B)
 *   CPD_GC_OUT_PAIRS  `out` rows are written as pairs (the sparse kernels' epilogues; c_out % 32 == 0 or c_out == 16, no out_col_group)
 *   CPD_GC_RES_PAIRS  `residual` rows are pairs (c_out % 32 == 0 or c_out == 16)
 * Round 5 -- DENSE pair maps (the Conv2d / ConvTranspose2d layers of BaseBEVBackbone and CenterHead, base_bev_backbone.py:31-59,
 * center_head.py:11-45,73-94, between two split-fp16 layers): CPD_GC_DENSE | CPD_GC_F16X2 | CPD_GC_IN_PAIRS | CPD_GC_OUT_PAIRS on
 * cpd_gather_conv* runs the 128 x 128 pair tile kernel (strided conv through its pixel table, 1 x 1 GEMM, ConvTranspose(k = s) through
 * out_row_map / out_col_group with groups of a multiple of 32 columns): c_in % 32 == 0, c_out % 128 == 0, pairs in AND out, no residual,
 * no in_absmax, < 4 GB of input; on cpd_conv3x3_rows* (below) the window kernel's 128 x 128 and 256 x 64 tiles (pairs in and out) and
 * its 256 x 16 tile (pairs in, fp32 rows out: c_out <= 16) -- the tiles cpd_conv3x3_rows_tile reports for the problem. Any other
 * shape: CPD_ERR_UNSUPPORTED (nothing else reads dense pair rows; keep that map fp32). */
#define CPD_GC_IN_PAIRS 16
#define CPD_GC_OUT_PAIRS 32
#define CPD_GC_RES_PAIRS 64

/* 3x3 / stride 1 / pad 1 convolution (+ folded BN / bias, residual, ReLU: same epilogue as
 * cpd_gather_conv) over channels-last pixel rows in[frames*h*w][c_in] WITHOUT a rulebook -- the
 * nn.Conv2d(3, padding=1) layers of BaseBEVBackbone (base_bev_backbone.py:38-62) and of
 * CenterHead / SeparateHead (center_head.py:24-52,78-90). The input row of output row R at tap
 * (dy, dx) is R + dy*w + dx when that pixel exists, so the three dx taps share one gathered and
 * split 130-row window per (32-channel block, dy). packed_w = cpd_pack_weight image of the
 * [9][c_in][c_out] weights (tap = ky*3 + kx). Split-bf16 arithmetic only: returns
 * CPD_ERR_UNSUPPORTED unless flags has CPD_GC_BF16X3, c_in % 32 == 0, c_out % 64 == 0, `in` rows are
 * 16-byte aligned and the problem fills the chip (cpd_conv3x3_rows_supported tells, pointers aside);
 * the caller then uses cpd_rulebook_conv2d + cpd_gather_conv, which computes the same thing.     */
int cpd_conv3x3_rows_supported(int frames, int h, int w, int c_in, int c_out, int flags);
/* Introspection: the (rows x columns) workgroup tile cpd_conv3x3_rows runs for this problem. HOST only. */
int cpd_conv3x3_rows_tile(int frames, int h, int w, int c_in, int c_out, int flags, int *bm, int *bn);
int cpd_conv3x3_rows(const float *in, int in_ld, int frames, int h, int w, int c_in,
                     const float *packed_w, int c_out, const float *scale, const float *shift,
                     const float *residual, int res_ld, int relu, float *out, int out_ld, int flags,
                     cpd_stream_t stream);
/* cpd_gather_conv for a 3 x 3 x 3 SubMConv3d layer (spconv_backbone.py:108-115: the SparseBasicBlock convs) whose rulebook comes with
 * a row plan (cpd_rulebook_plan): the STAGED row-wave kernel. Per tile of 128 output rows and dz group it copies the group's distinct
 * input rows (128-byte channel blocks, whole cache lines) into an LDS window once and forms the MFMA fragments of all nine taps from
 * LDS -- a (row, tap) pair costs a ds_read instead of a gather through the vector L1 (which is what bounded the row-wave kernels:
 * profiles/r03_rowwave_pmc.json). Same arithmetic as cpd_gather_conv with CPD_GC_F16X2 | CPD_GC_IN_PAIRS (identical partial products,
 * accumulated in the same tap order). Takes: kv = 27, c_in % 32 == 0, c_out = 32 / 64 / 128, fp16-pair input rows, >= 512 tiles
 * (cpd_gather_conv_planned_supported tells; otherwise CPD_ERR_UNSUPPORTED and the caller uses cpd_gather_conv_ws: same result).
 * flags: CPD_GC_F16X2 | CPD_GC_IN_PAIRS [| CPD_GC_OUT_PAIRS | CPD_GC_RES_PAIRS]. */
int cpd_gather_conv_planned_supported(int n_in, int n_out, int c_in, int c_out, int in_ld, int kv, int flags);
int cpd_gather_conv_planned(const float *in, int in_ld, int n_in, int c_in, const float *packed_w, const uint32_t *tapmask,
                            const uint16_t *plan_slots, const int32_t *plan_ulist, const int32_t *plan_count, int tile_rows, int kv,
                            int n_out, int c_out, const float *scale, const float *shift, const float *residual, int res_ld,
                            int relu, float *out, int out_ld, int flags, uint32_t *out_absmax, cpd_stream_t stream);
/* Introspection for benchmarks/profilers: which kernel instantiation cpd_gather_conv runs for
 * this problem: wg=1 -> tile_conv_kernel<a,b> (a x b workgroup tile), wg=0 ->
 * gather_conv_kernel<a,b,vec> ((16a) x (16b) wave tile; vec = 16-byte A pieces). HOST only.  */
int cpd_gather_conv_tile(int n_out, int c_in, int c_out, int in_ld, int flags, int *wg, int *a,
                         int *b, int *vec);
/* ... and the launch-log label (cpd_launch_log_*) of that instantiation, from the launcher's own table -- for a problem described
 * without pointers: operands taken as 16-byte aligned, the row-wave kernels' plain (not LDS-epilogue) forms. kv: the tap count
 * (0: unknown; more taps than a row-wave launch keeps are planned as a dense layer, as the launcher does); scaled: an in_absmax
 * block comes with the input (the f16s forms). A static string; NULL when no kernel takes the problem. HOST only. */
const char *cpd_gather_conv_label(int n_out, int c_in, int c_out, int in_ld, int kv, int flags, int scaled);

/* SparseConvTensor.dense() + view(N, C*D, H, W) (height_compression.py:136-138).
 *   nchw: out (B, C*D, H, W), channel = c*D + z   -- the reference layout
 *   nhwc: out (B, H, W, D*C), channel = z*C + c   -- channels-last, feeds cpd_gather_conv
 *   nhwc_cd: out (B, H, W, C*D), channel = c*D + z -- channels-last memory with the reference's channel order: the (N, C*D, H, W)
 *            tensor of height_compression.py:136-138 in torch's channels_last format (what the module path hands to Conv2d)
 * All zero-fill `out` themselves.                                                            */
int cpd_densify_nchw(const float *feat, const int32_t *indices, int n, int c, int batch,
                     const int32_t shape_zyx[3], float *out, cpd_stream_t stream);
int cpd_densify_nhwc(const float *feat, const int32_t *indices, int n, int c, int batch,
                     const int32_t shape_zyx[3], float *out, cpd_stream_t stream);
/* cpd_densify_nhwc into a PERSISTENT map that is all zero on entry (no clear inside), and the call that restores that state afterwards by
 * zeroing the same rows -- queue it after the map's last reader. SparseConvTensor.dense() semantics as above (height_compression.py:136-138);
 * moves 2 x sites x c floats instead of the whole map. */
int cpd_densify_nhwc_rows(const float *feat, const int32_t *indices, int n, int c, int batch,
                          const int32_t shape_zyx[3], float *out, cpd_stream_t stream);
int cpd_densify_nhwc_clear(const int32_t *indices, int n, int c, int batch, const int32_t shape_zyx[3], float *out,
                           cpd_stream_t stream);
int cpd_densify_nhwc_cd(const float *feat, const int32_t *indices, int n, int c, int batch,
                        const int32_t shape_zyx[3], float *out, cpd_stream_t stream);
/* Dense-pixel rulebooks for the BEV convs: nbr[kh*kw][ho*wo*batch] for a (kh x kw, stride, pad)
 * Conv2d over a (batch, h, w) channels-last map. */
int cpd_rulebook_conv2d(int batch, int h, int w, int kh, int kw, int stride, int pad,
                        int32_t *nbr, cpd_stream_t stream);

/* ===== CenterHead decode ===================================================================
 * Replaces CenterHead.generate_predicted_boxes (center_head.py:252-303) ->
 * centernet_utils.decode_bbox_from_heatmap / _topk (centernet_utils.py:136-216) for one sample:
 * sigmoid(hm), exp(dim), per-class top-K then top-K over classes, gather, atan2(sin,cos),
 * centre scaling, POST_CENTER_LIMIT_RANGE and SCORE_THRESH masks, order-preserving compaction.
 * Head maps are addressed as map[pixel*pix_stride + channel*ch_stride] so both the reference's
 * NCHW planes and this library's channels-last rows can be decoded in place.
 * `batch` samples are decoded by one call: sample b's maps start sample_stride floats after
 * sample b-1's. Outputs (capacity K per sample): boxes [batch,K,7] (x,y,z,dx,dy,dz,heading),
 * scores [batch,K], labels [batch,K] i32 (0-based class id), n_out [batch] device counts.     */
size_t cpd_center_decode_workspace_bytes(int batch, int num_class, int hw, int k);
int cpd_center_decode(const float *hm, const float *center, const float *center_z,
                      const float *dim, const float *rot, int batch, long long sample_stride,
                      int pix_stride, int ch_stride, int num_class, int h, int w, int k,
                      float feature_map_stride,
                      const float voxel_xy[2], const float range_lo_xy[2],
                      const float limit_range[6], float score_thresh, float *boxes, float *scores,
                      int32_t *labels, int32_t *n_out, void *workspace, size_t workspace_bytes,
                      cpd_stream_t stream);
/* The same decode cut at the peaks, for a head that evaluates its regression branches only where the decode reads them (the K
 * merged top-K pixels of each frame). Same kernels and arithmetic as cpd_center_decode for the selection, the box decode, the masks
 * and the compaction; same error codes (k > 1024, k > h*w: CPD_ERR_UNSUPPORTED). Nothing here synchronises with the host.
 *
 * cpd_center_peaks: per-class top-K + the merge over classes on the hm map alone. Per frame, the K winners in their final order:
 * peak_score [batch,K], peak_cand [batch,K] (candidate index; class = peak_cand / K), peak_ind [batch,K] (pixel y*w + x). */
size_t cpd_center_peaks_workspace_bytes(int batch, int num_class, int hw, int k);
int cpd_center_peaks(const float *hm, int batch, long long sample_stride, int pix_stride, int ch_stride,
                     int num_class, int h, int w, int k, float *peak_score, int32_t *peak_cand,
                     int32_t *peak_ind, void *workspace, size_t workspace_bytes, cpd_stream_t stream);
/* cpd_peak_rulebook: the neighbour table nbr[9][batch*K*9] of the regression branches' FIRST 3 x 3 / pad 1 convolution, evaluated
 * at the 9 hidden sites the LAST 3 x 3 convolution reads around each peak. Output row (b*K + k)*9 + t is the hidden site at peak
 * (b, k)'s pixel + tap t's offset (t = ky*3 + kx, offset (ky - 1, kx - 1): the tap order of cpd_rulebook_conv2d); nbr[u][row] is
 * the row b*h*w + pixel of the input map at that site + tap u's offset, -1 where that pixel is outside the image, and -1 for every
 * u where the hidden site itself is outside the image. A neighbour never belongs to another frame. */
int cpd_peak_rulebook(const int32_t *peak_ind, int batch, int k, int h, int w, int32_t *nbr,
                      cpd_stream_t stream);
/* cpd_center_decode_at_peaks: hidden [batch*K*9, c_hid] fp32 rows (pitch hidden_ld floats; row order of cpd_peak_rulebook), the last
 * convolutions' weights as ONE fp32 image w_last [9][c_hid][n_reg] (block-diagonal over the branches, zeros included) with bias
 * [n_reg]; reg_offsets = first channel of center (2 values), center_z (1), dim (3), rot (2) among the n_reg. Forms every peak's
 * regression values in fp32 -- a tap whose hidden site lies outside the image contributes NOTHING (the last convolution pads the
 * hidden map with zeros; what the hidden row of such a site holds is ignored) -- then decodes, masks and compacts as
 * cpd_center_decode does. Outputs as cpd_center_decode's. n_reg <= 16, c_hid and hidden_ld multiples of 4, hidden 16-byte aligned. */
size_t cpd_center_decode_at_peaks_workspace_bytes(int batch, int k, int n_reg);
int cpd_center_decode_at_peaks(const float *peak_score, const int32_t *peak_cand, const int32_t *peak_ind,
                               const float *hidden, int hidden_ld, int c_hid, const float *w_last,
                               const float *bias, int n_reg, const int32_t reg_offsets[4], int batch,
                               int num_class, int h, int w, int k, float feature_map_stride,
                               const float voxel_xy[2], const float range_lo_xy[2],
                               const float limit_range[6], float score_thresh, float *boxes, float *scores,
                               int32_t *labels, int32_t *n_out, void *workspace, size_t workspace_bytes,
                               cpd_stream_t stream);

/* ===== B3. iou3d_nms =======================================================================
 * Replaces the iou3d_nms_cuda extension (cpd/ops/iou3d_nms/src/iou3d_nms_api.cpp:11-17).
 * Boxes are [n,7] f32 (x,y,z,dx,dy,dz,heading), contiguous.                                  */
/* boxes_overlap_bev_gpu (iou3d_nms.cpp:49-68): out[n,m] rotated BEV intersection area. */
int cpd_boxes_overlap_bev(const float *a, int n, const float *b, int m, float *out,
                          cpd_stream_t stream);
/* boxes_iou_bev_gpu (iou3d_nms.cpp:70-88): out[n,m] rotated BEV IoU. */
int cpd_boxes_iou_bev(const float *a, int n, const float *b, int m, float *out,
                      cpd_stream_t stream);
/* boxes_iou3d_gpu (iou3d_nms_utils.py:67-100) fused: BEV overlap x height overlap / union. */
int cpd_boxes_iou3d(const float *a, int n, const float *b, int m, float *out,
                    cpd_stream_t stream);
/* nms_gpu / nms_normal_gpu (iou3d_nms.cpp:90-137,139-186): boxes sorted by descending score.
 * The 64x64 bitmask (iou3d_nms_kernel.cu:267-311) AND the greedy scan run on the device; keep
 * [n] i64 and num_keep (i32 scalar) are DEVICE buffers -- the reference's blocking D2H copy of
 * the whole mask is gone; the shim copies keep[:num] back to satisfy the CPU-`keep` contract. */
size_t cpd_nms_workspace_bytes(int n);
int cpd_nms_rotated(const float *boxes, int n, float thresh, int64_t *keep, int32_t *num_keep,
                    void *workspace, size_t workspace_bytes, cpd_stream_t stream);
int cpd_nms_normal(const float *boxes, int n, float thresh, int64_t *keep, int32_t *num_keep,
                   void *workspace, size_t workspace_bytes, cpd_stream_t stream);
/* Batched form for the per-sample NMS loop of generate_predicted_boxes (center_head.py:281-296):
 * boxes [batch, capacity, 7] sorted by descending score per sample, valid counts [batch] ON THE
 * DEVICE (e.g. cpd_center_decode's n_out -- no host read-back in between); keep [batch, capacity],
 * num_keep [batch]; workspace = batch * cpd_nms_workspace_bytes(capacity).                      */
int cpd_nms_batch(const float *boxes, const int32_t *counts, int batch, int capacity, float thresh,
                  int normal, int64_t *keep, int32_t *num_keep, void *workspace,
                  size_t workspace_bytes, cpd_stream_t stream);
/* cpd_nms_batch for callers that keep only the FIRST max_keep survivors of a sample -- class_agnostic_nms keeps
 * selected[:NMS_POST_MAXSIZE] (model_nms_utils.py:115-134), RoIHeadTemplate.proposal_layer 4096 candidates -> the first few hundred
 * (roi_head_template.py:53-114): greedy suppression decides box i from boxes before i only, so the first max_keep survivors are known
 * as soon as the scan has found them. The mask is built for the first `row_limit` boxes of each sample only ((row_limit)^2 / 2 IoUs
 * instead of capacity^2 / 2) and the scan stops after the 64-box block that holds the max_keep-th survivor: keep[b][0 .. min(num_keep[b],
 * max_keep)) are EXACTLY cpd_nms_batch's first entries. incomplete[b] = 1 when sample b has more than row_limit boxes and fewer than
 * max_keep of its first row_limit survived -- the answer then needs boxes the mask does not cover, and the caller runs cpd_nms_batch
 * (the flag is a device word: read it with the counts). workspace = batch * cpd_nms_workspace_bytes(min(row_limit, capacity)). */
int cpd_nms_batch_first(const float *boxes, const int32_t *counts, int batch, int capacity, float thresh,
                        int normal, int max_keep, int row_limit, int64_t *keep, int32_t *num_keep,
                        int32_t *incomplete, void *workspace, size_t workspace_bytes, cpd_stream_t stream);
/* ... and the full call for exactly the samples that asked for it, without a host read-back in between: cpd_nms_batch over the
 * samples b with where[b] != 0 (a device array, e.g. cpd_nms_batch_first's `incomplete`); the others keep their keep / num_keep.
 * The launch costs its empty workgroups when no sample asks (measured: DESIGN 5h).                                              */
int cpd_nms_batch_where(const float *boxes, const int32_t *counts, const int32_t *where, int batch,
                        int capacity, float thresh, int normal, int64_t *keep, int32_t *num_keep,
                        void *workspace, size_t workspace_bytes, cpd_stream_t stream);
/* The score half of Detector3DTemplate.post_processing (cpd/models/detectors/detector3d_template.py:222-343, MULTI_CLASSES_NMS False) and of
 * class_agnostic_nms (cpd/models/model_utils/model_nms_utils.py:113-124) for a whole batch in one launch: per frame, score = max over the
 * n_cls columns of sigmoid(cls) (of cls itself when normalized != 0), rows with score >= score_thresh ranked by score descending (ties: lower
 * index first -- a stable sort), the others after them with score -1; out_boxes / out_scores / out_labels (int32) = the r rows in that order,
 * n_ok[b] = min(#rows above the threshold, pre_max): what cpd_nms_batch + cpd_select_boxes take next. cls [batch, r, n_cls], boxes
 * [batch, r, 7], labels_i64 [batch, r]. r <= 8192, else CPD_ERR_UNSUPPORTED. */
int cpd_rank_scores(const float *cls, int n_cls, const float *boxes, const void *labels_i64, int batch, int r, float score_thresh,
                    int pre_max, int normalized, float *out_boxes, float *out_scores, int32_t *out_labels, int32_t *n_ok,
                    cpd_stream_t stream);
/* class_agnostic_nms tail (model_nms_utils.py:126-127,134) + the `+1` of center_head.py:301, batched:
 * out[b][k] = in[b][keep[b][k]] for k < out_n[b] = min(num_keep[b], post_max).
 * out_boxes [batch,post_max,7], out_scores [batch,post_max], out_labels [batch,post_max] i64.  */
int cpd_select_boxes(const float *boxes, const float *scores, const int32_t *labels,
                     const int64_t *keep, const int32_t *num_keep, int batch, int capacity,
                     int post_max, int label_offset, float *out_boxes, float *out_scores,
                     int64_t *out_labels, int32_t *out_n, cpd_stream_t stream);
/* generate_recall_record (cpd/models/detectors/detector3d_template.py:344-386; called per frame from post_processing, l.326-330, and
 * cpd/models/detectors/centerpoint.py:36-50; summed by tools/eval_utils/eval_utils.py:14-21,94-101) for ALL frames of a batch in one
 * launch, with no host wait. Frame b's final boxes are rows pred_start[b] .. pred_start[b] + pred_count[b] of `pred` (row pitch pred_ld
 * floats, columns 0:7 read); its RoIs likewise in `rois` (NULL: a one-stage model, the roi counters are left alone). The start / count
 * arrays are DEVICE int32 [batch]: a padded block (start = b * capacity, counts from the NMS) and a concatenation of per-frame tensors
 * are addressed alike; every row they name must exist. gt [batch][gt_cap][gt_ld] f32, gt_ld >= 7, columns 0:7 the box: rows 0 .. k of a
 * frame count, k the last row whose float32 sum over all gt_ld columns is not zero and never less than 0 (l.358-362: an all-zero block
 * counts one gt; a zero row between real rows counts); gt_cap == 0 counts nothing. thresh: HOST array of n_thresh (1..8) values >= 0.
 * counters: device int64 [1 + 2 * n_thresh] = gt, roi_<t0> .., rcnn_<t0> ..; ADDED to, never cleared here: a counted gt adds 1 to
 * rcnn_<t> when the largest boxes_iou3d_gpu value (the expression of cpd_boxes_iou3d) of its column over the frame's final boxes is > t
 * (strict; no boxes: nothing), and to roi_<t> likewise over the RoIs (zero-padded RoI rows take part: IoU 0). Optional outputs (NULL to
 * skip): best_rcnn / best_roi [batch][gt_cap] f32 = that largest IoU per counted gt (-1 where the frame has no such boxes), -1 for rows
 * not counted; n_gt [batch] i32 = rows counted per frame. CPD_ERR_ARG: batch outside 1..65535, gt_ld / pred_ld / roi_ld < 7, n_thresh
 * outside 1..8, a negative or NaN threshold, a null required pointer. */
int cpd_recall_record(const float *pred, int pred_ld, const int32_t *pred_start, const int32_t *pred_count,
                      const float *rois, int roi_ld, const int32_t *roi_start, const int32_t *roi_count,
                      const float *gt, int batch, int gt_cap, int gt_ld, const float *thresh, int n_thresh,
                      int64_t *counters, float *best_rcnn, float *best_roi, int32_t *n_gt, cpd_stream_t stream);
/* Weighted box fusion of test-time-augmentation views: DetectionsMerger.compute_WBF (cpd/datasets/kitti/kitti_object_eval_python/
 * merge_detections.py:110-181; the same text as compute_WBF of merge_detections_tracking.py:121-191) and model_nms_utils.compute_WBF
 * (cpd/models/model_utils/model_nms_utils.py:14-113), for ALL segments of a batch in one launch with no host wait. A segment is the
 * boxes of one frame and one class after the score floor, by descending score: rows seg_start[s] .. seg_start[s] + seg_count[s] of
 * boxes [n][7] / scores [n] (DEVICE int32 [n_seg]; segments must not overlap, every row they name must exist; at most
 * CPD_WBF_MAX_SEGMENT rows each). seg_thresh [n_seg][2] f32 = iou_thresh, iou_thresh2 (the second read by the model variant only);
 * seg_mode [n_seg] i32 = 0 (WBF-mean) or a sum of CPD_WBF_MAX (type 'max'), CPD_WBF_MODEL (the model_nms_utils rules),
 * CPD_WBF_NO_RETAIN (retain_low=False; model variant only). One workgroup per segment takes the boxes in order: the lanes take the
 * rotated BEV IoU (the expression of cpd_boxes_iou_bev_cpu) of the box with every cluster so far, a block reduction yields the
 * largest IoU and the lowest cluster index that attains it (np.argmax), one thread applies the rule. Headings are folded first
 * (limit_period(0.5, 2 pi) / model_nms_utils.limit); the inputs are not written.
 * Outputs: out_boxes [n][7] / out_scores [n]: segment s's results in rows seg_start[s] .. + out_count[s], clusters in creation order
 * (model variant: the boxes emitted on their own first, in input order); rows beyond are left alone. out_count [n_seg] i32; -1 for a
 * segment that is out of range or longer than CPD_WBF_MAX_SEGMENT (nothing else is written for it). cluster_of [n] i32: for every box of
 * a segment the cluster it joined (creation index), -1 dropped, -2 emitted on its own.
 * Workspace: cpd_wbf_workspace_bytes(n); the state of the first CPD_WBF_LDS_CLUSTERS clusters of a segment lives in LDS, the rest there. */
#define CPD_WBF_MAX 1
#define CPD_WBF_MODEL 2
#define CPD_WBF_NO_RETAIN 4
#define CPD_WBF_MAX_SEGMENT 8192
#define CPD_WBF_LDS_CLUSTERS 512
#define CPD_WBF_BLOCK 256
size_t cpd_wbf_workspace_bytes(int n);
int cpd_wbf_cluster(const float *boxes, const float *scores, int n, const int32_t *seg_start, const int32_t *seg_count,
                    const float *seg_thresh, const int32_t *seg_mode, int n_seg, float *out_boxes, float *out_scores,
                    int32_t *out_count, int32_t *cluster_of, void *workspace, size_t workspace_bytes, cpd_stream_t stream);
/* The same clustering on the calling thread, HOST pointers throughout (the rules of csrc/wbf_rules.h compiled for the host; like
 * cpd_boxes_iou_bev_cpu it needs no device): same arguments without workspace and stream, same outputs. */
int cpd_wbf_cluster_cpu(const float *boxes, const float *scores, int n, const int32_t *seg_start, const int32_t *seg_count,
                        const float *seg_thresh, const int32_t *seg_mode, int n_seg, float *out_boxes, float *out_scores,
                        int32_t *out_count, int32_t *cluster_of);
/* KITTI transfer evaluation of a Waymo-trained detector (Kitti2WaymoDataset, cpd/datasets/kitti/kitti2waymo_dataset.py): the input
 * stage of __getitem__ (l.414-425) and the output stage of generate_prediction_dicts (l.272-355), each for a whole batch.
 * Per-frame constants travel as `frames` [batch][CPD_K2W_FRAME_WORDS] 32-bit words on the DEVICE: M = np.dot(V2C.T, R0.T) [4][3] f32
 * (words 0-11, row major; formed on the host the way Calibration.lidar_to_rect forms it), P2 [3][4] f32 (words 12-23), then the
 * image height and width as int32 (words 24, 25). All float32 arithmetic is unfused, products and sums from left to right.
 *
 * cpd_kitti_fov_points: Calibration.lidar_to_rect + rect_to_img + get_fov_flag (calibration_kitti.py:110-141,
 * kitti2waymo_dataset.py:102-118) and `points + [0, 0, 1.55, 0]`, `points[:, 3:] = 0`. points [n][ld >= 3] f32, frame f = rows
 * frame_start[f] .. frame_start[f + 1] (DEVICE int32 [batch + 1]); max_len >= the longest frame sizes the grid.
 *   rect = [x y z 1] M;  hom = [rect 1] P2^T;  u = hom0 / rect_z, v = hom1 / rect_z (the rectified z, not hom2);  depth = hom2 - P2[2][3]
 *   keep iff 0 <= u < w, 0 <= v < h, depth >= 0 (NaN and inf compare false)
 * The kept points of frame f go, in their input order, to rows frame_start[f] .. + out_count[f] of out [n][n_feat_out >= 3] as
 * [x, y, (float)((double)z + z_shift), 0, ...]; rows beyond are left alone. out_index (optional, int32 [n]) receives each kept
 * point's index within its frame at the same rows. out_count [batch] i32 stays on the device; -1 for a frame whose bounds are out of
 * range or longer than max_len (nothing else is written for it). Two launches (per-tile counts, then scatter; a tile is
 * CPD_K2W_TILE points), no atomics: the result is bitwise repeatable. Workspace: cpd_kitti_fov_workspace_bytes(batch, max_len). */
#define CPD_K2W_FRAME_WORDS 26
#define CPD_K2W_BLOCK 256
#define CPD_K2W_TILE 1024
size_t cpd_kitti_fov_workspace_bytes(int batch, int max_len);
int cpd_kitti_fov_points(const float *points, int n, int ld, const int32_t *frame_start, int batch, int max_len, const void *frames,
                         double z_shift, int n_feat_out, float *out, int32_t *out_index, int32_t *out_count, void *workspace,
                         size_t workspace_bytes, cpd_stream_t stream);
/* cpd_kitti_export: the final detections of a batch to KITTI annotations. boxes [n][7] f32, scores [n] f32, labels [n] i32 (1-based),
 * frame f = rows seg_start[f] .. seg_start[f + 1] (DEVICE int32 [batch + 1]); one workgroup per frame. The inputs are not written.
 * CPD_K2W_PREDICT restates generate_single_sample_dict op by op in its dtypes (numpy >= 2 scalar rules): z -= 1.55; where the frame
 * holds a label != 0, boxes of label != 0 get z += 0.1, l -= 0.2, w -= 0.2, h -= 0.1 and the frame keeps l < 5 (stable); label 1
 * moves its centre to whichever of +-new_d / 2 along the heading is nearer the origin (float64; new_d = 0.1 + min(|c|, 60) / 60 * 0.3
 * in float32; a tie takes the negative candidate), rounded to float32 when stored; then the camera part. CPD_K2W_CAMERA runs the
 * camera part alone on every box (merge_detections.py:247-255): boxes3d_lidar_to_kitti_camera with its in-place z -= h / 2
 * (box_utils.py:152-166), boxes3d_to_corners3d_kitti_camera, rect_to_img of the 8 corners, min / max, clip to [0, w - 1] /
 * [0, h - 1] (box_utils.py:169-235), alpha = -atan2(-y, x) + ry.
 * Outputs, frame f's kept boxes in rows seg_start[f] .. + out_count[f], rows beyond left alone: out_boxes [n][7] (boxes_lidar, z at
 * the bottom centre), out_scores [n], out_labels [n], out_camera [n][7] = location, dimensions (l, h, w), rotation_y, out_alpha [n],
 * out_bbox [n][4]; out_count [batch] i32, -1 for a frame whose bounds are out of range. scores / labels may be NULL in camera mode. */
#define CPD_K2W_PREDICT 0
#define CPD_K2W_CAMERA 1
int cpd_kitti_export(const float *boxes, const float *scores, const int32_t *labels, int n, const int32_t *seg_start, int batch,
                     const void *frames, int mode, float *out_boxes, float *out_scores, int32_t *out_labels, float *out_camera,
                     float *out_alpha, float *out_bbox, int32_t *out_count, cpd_stream_t stream);
/* boxes_iou_bev_cpu (iou3d_cpu.cpp:232-252): HOST pointers, runs on the calling thread. This is
 * the one CPU entry point the reference extension itself exports (used by the dataloader's
 * gt-sampling, database_sampler.py:445-446); it is product code, not the test oracle.        */
int cpd_boxes_iou_bev_cpu(const float *a, int n, const float *b, int m, float *out);


/* ===== Training step (BASELINE config 3) ====================================================
 * Forward in training mode is cpd_gather_conv (no folded BN) + cpd_bn_stats + cpd_affine_rows; the
 * input gradient of every conv is cpd_gather_conv again on transposed (tap-flipped for SubM /
 * stride-1) weights with the same or the transposed rulebook; the rest is below. These replace
 * what torch autograd + cuDNN + spconv's backward ops do under tools/train_utils/train_utils.py:41
 * (loss.backward()) for the modules of the path.                                               */
size_t cpd_col_reduce_workspace_bytes(int n, int c);
/* column sums of x[n, c] (bias gradients). */
int cpd_col_sum(const float *x, int ldx, int n, int c, float *sum, void *ws, size_t ws_bytes,
                cpd_stream_t stream);
/* training-mode BatchNorm statistics: sum[c], sumsq[c] over the n rows (two-stage, deterministic). */
int cpd_bn_stats(const float *x, int ldx, int n, int c, float *sum, float *sumsq, void *ws,
                 size_t ws_bytes, cpd_stream_t stream);
/* Per-channel bookkeeping after cpd_bn_stats: mean, invstd = 1/sqrt(var_biased + eps), the affine
 * scale = gamma*invstd / shift = beta - mean*scale, and (optional) running-stat update
 * running = (1-momentum)*running + momentum*batch (unbiased variance), as torch.nn.BatchNorm does. */
int cpd_bn_finalize(const float *sum, const float *sumsq, int n, int c, float eps, float momentum,
                    const float *gamma, const float *beta, float *mean, float *invstd, float *scale,
                    float *shift, float *running_mean, float *running_var, cpd_stream_t stream);
/* cpd_bn_stats + cpd_bn_finalize in one call (two launches): the training-mode BatchNorm forward
 * bookkeeping of one layer. */
int cpd_bn_stats_finalize(const float *x, int ldx, int n, int c, float eps, float momentum,
                          const float *gamma, const float *beta, float *mean, float *invstd,
                          float *scale, float *shift, float *running_mean, float *running_var,
                          void *workspace, size_t workspace_bytes, cpd_stream_t stream);
/* out = act(x * scale + shift + residual): BatchNorm apply (scale = gamma*invstd,
 * shift = beta - mean*scale), SparseBasicBlock tail (spconv_backbone.py:131-134). In place allowed. */
int cpd_affine_rows(const float *x, int ldx, int n, int c, const float *scale, const float *shift,
                    const float *residual, int ldr, int relu, float *out, int ldo,
                    cpd_stream_t stream);
/* BatchNorm(+ReLU) backward. dy_m = dy * (y > 0) (y = NULL: no ReLU);
 * reduce: dbeta = sum dy_m, dgamma = sum dy_m * xhat; apply: dx = gamma*invstd*(dy_m - dbeta/n -
 * xhat*dgamma/n), optional dres = dy_m (gradient into a residual added before the ReLU).       */
int cpd_bn_bwd_reduce(const float *dy, int lddy, const float *y, int ldy, const float *x, int ldx,
                      const float *mean, const float *invstd, int n, int c, float *dbeta,
                      float *dgamma, void *ws, size_t ws_bytes, cpd_stream_t stream);
int cpd_bn_bwd_apply(const float *dy, int lddy, const float *y, int ldy, const float *x, int ldx,
                     int n, int c, const float *mean, const float *invstd, const float *gamma,
                     const float *dbeta, const float *dgamma, float *dx, int lddx, float *dres,
                     int lddres, uint32_t *dx_absmax, cpd_stream_t stream);
/* SyncBatchNorm (tools/train.py:32,117 `--sync_bn` -> torch.nn.SyncBatchNorm.convert_sync_batchnorm; off by default in the reference):
 * the host all-reduces (sum, sumsq, row count) between cpd_bn_stats and the finalize, and (sum dy, sum dy * xhat) between
 * cpd_bn_bwd_reduce and the apply, over the data-parallel ranks (RCCL). These two entry points take the row count the sums now stand
 * for as a DEVICE float (`n_total`: the all-reduced count -- ranks hold different numbers of sparse rows, and no rank knows the total
 * on the host); otherwise they are cpd_bn_finalize / cpd_bn_bwd_apply. dgamma / dbeta of the PARAMETERS stay the local sums
 * (torch.nn.SyncBatchNorm's backward: the gradient all-reduce averages them like every other gradient). */
int cpd_bn_finalize_sync(const float *sum, const float *sumsq, const float *n_total, int c, float eps, float momentum,
                         const float *gamma, const float *beta, float *mean, float *invstd, float *scale, float *shift,
                         float *running_mean, float *running_var, cpd_stream_t stream);
int cpd_bn_bwd_apply_sync(const float *dy, int lddy, const float *y, int ldy, const float *x, int ldx, int n, int c,
                          const float *mean, const float *invstd, const float *gamma, const float *sum_dy,
                          const float *sum_dy_xhat, const float *n_total, float *dx, int lddx, float *dres, int lddres,
                          uint32_t *dx_absmax, cpd_stream_t stream);
/* dx_absmax (optional): an "absmax block" -- CPD_ABSMAX_SLOTS device words CPD_ABSMAX_STRIDE uint32 apart (one per
 * 128-byte line: atomics on one line serialise), zeroed by the caller beforehand -- whose words the kernel raises (atomic
 * max) so that their maximum is the bits of max |dx|: what cpd_gather_conv_scaled / cpd_conv_wgrad_scaled need to run a
 * gradient through the split-fp16 path. A caller that knows the maximum writes it to word 0 of a zeroed block. */
#define CPD_ABSMAX_SLOTS 16
#define CPD_ABSMAX_STRIDE 32
#define CPD_ABSMAX_WORDS (CPD_ABSMAX_SLOTS * CPD_ABSMAX_STRIDE)
int cpd_relu_bwd(const float *dy, int lddy, const float *y, int ldy, int n, int c, float *dx,
                 int lddx, cpd_stream_t stream);
/* Weight gradient of cpd_gather_conv: dw[t][ci][co] (+)= sum_j in[nbr[t][j]][ci] * dy[j][co]
 * (dense [kv][c_in][c_out] layout, the layout cpd_pack_weight consumes). Deterministic (row-chunk
 * partials in `ws`, summed in a fixed order). flags: bit 0 = accumulate into dw_kio, CPD_GC_BF16X3 =
 * split-bf16 arithmetic (fp32-equivalent, as in cpd_gather_conv) when c_in and c_out are multiples
 * of 32, with rows that lack the tap compacted away before staging; otherwise fp32 MFMA.        */
size_t cpd_conv_wgrad_workspace_bytes(int n_out, int c_in, int c_out, int kv);
int cpd_conv_wgrad(const float *in, int in_ld, int c_in, const float *dy, int dy_ld, int c_out,
                   const int32_t *nbr, int kv, int n_out, float *dw_kio, int flags, void *ws,
                   size_t ws_bytes, cpd_stream_t stream);
/* The same with flags CPD_GC_F16X2 allowed: split-fp16 arithmetic (three products instead of six). Gradients do not live in
 * fp16's range, so each operand may come with an absmax block (see cpd_bn_bwd_apply) holding the bits of its max |value|
 * (in_absmax for `in`, dy_absmax for `dy`; NULL = use as is): the kernel multiplies the operand by the power of two that puts that maximum at
 * [2^14, 2^15) before splitting and divides the partial sums by it again -- exact, and an element 2^-18 of the maximum or
 * larger keeps its full 2^-24 relative precision (smaller ones 2^-43 of the maximum absolute). */
int cpd_conv_wgrad_scaled(const float *in, int in_ld, int c_in, const float *dy, int dy_ld, int c_out,
                          const int32_t *nbr, int kv, int n_out, float *dw_kio, int flags,
                          const uint32_t *in_absmax, const uint32_t *dy_absmax, void *ws, size_t ws_bytes,
                          cpd_stream_t stream);
/* Input-gradient convolutions through the split-fp16 kernels: cpd_gather_conv / cpd_conv3x3_rows with `in` pre-scaled the
 * same way (in_absmax as above; ignored by the fp32 and split-bf16 kernels, which need no range help). */
int cpd_gather_conv_scaled(const float *in, int in_ld, int n_in, int c_in, const float *packed_w,
                           const int32_t *nbr, const uint32_t *tapmask, int kv, int n_out, int c_out, const float *scale,
                           const float *shift, const float *residual, int res_ld, int relu, float *out,
                           int out_ld, const int32_t *out_row_map, int out_col_group, int flags,
                           const uint32_t *in_absmax, cpd_stream_t stream);
int cpd_conv3x3_rows_scaled(const float *in, int in_ld, int frames, int h, int w, int c_in,
                            const float *packed_w, int c_out, const float *scale, const float *shift,
                            const float *residual, int res_ld, int relu, float *out, int out_ld, int flags,
                            const uint32_t *in_absmax, cpd_stream_t stream);
/* The range guard of the f16x2 INFERENCE path (fp16's narrow exponent is the one way split-fp16 arithmetic differs from the
 * reference's fp32 convolutions, spconv_backbone.py:108-136 / base_bev_backbone.py:31-59): every launch may leave the bits of
 * max |out| behind in an absmax block (out_absmax; zero the block before the first launch that writes it -- several launches
 * may raise the same block, e.g. the two halves of a concat buffer), and takes its input's block as in_absmax exactly like the
 * _scaled calls above: the split-fp16 kernels then pre-scale the input by a power of two and undo it in the epilogue (exact),
 * so an activation of any fp32 magnitude gives the fp32 answer instead of inf / NaN. in_absmax = NULL: input used as is;
 * out_absmax = NULL: nothing recorded. cpd_absmax_rows raises a block to the range of a tensor that came from elsewhere. */
int cpd_gather_conv_ranged(const float *in, int in_ld, int n_in, int c_in, const float *packed_w,
                           const int32_t *nbr, const uint32_t *tapmask, int kv, int n_out, int c_out, const float *scale,
                           const float *shift, const float *residual, int res_ld, int relu, float *out,
                           int out_ld, const int32_t *out_row_map, int out_col_group, int flags,
                           const uint32_t *in_absmax, uint32_t *out_absmax, cpd_stream_t stream);
/* The same with a workspace: small sparse launches (one frame, the train step: fewer row-wave workgroups than ~2 per CU) deal the
 * taps of a row tile to several workgroups that write partial sums into the workspace; a second launch adds them in a fixed order
 * and runs the epilogue (results equal the unsplit launch up to fp32 summation order). cpd_gather_conv_split_bytes: the workspace
 * this problem wants (0: it runs unsplit, and cpd_gather_conv_ws with any workspace is cpd_gather_conv_ranged). HOST only. */
size_t cpd_gather_conv_split_bytes(int n_out, int c_in, int c_out, int in_ld, int kv, int flags);
int cpd_gather_conv_ws(const float *in, int in_ld, int n_in, int c_in, const float *packed_w,
                       const int32_t *nbr, const uint32_t *tapmask, int kv, int n_out, int c_out, const float *scale,
                       const float *shift, const float *residual, int res_ld, int relu, float *out,
                       int out_ld, const int32_t *out_row_map, int out_col_group, int flags,
                       const uint32_t *in_absmax, uint32_t *out_absmax, void *workspace, size_t workspace_bytes,
                       cpd_stream_t stream);
int cpd_conv3x3_rows_ranged(const float *in, int in_ld, int frames, int h, int w, int c_in,
                            const float *packed_w, int c_out, const float *scale, const float *shift,
                            const float *residual, int res_ld, int relu, float *out, int out_ld, int flags,
                            const uint32_t *in_absmax, uint32_t *out_absmax, cpd_stream_t stream);
int cpd_absmax_rows(const float *x, int ld, long long n, int c, uint32_t *absmax_block, cpd_stream_t stream);
/* All packed images of a model in three launches (a train step rewrites every one of them after the optimiser step; one
 * cpd_pack_weight / cpd_pack_weight_adjoint call is four launches). A job names one packed buffer (sized by
 * cpd_packed_weight_floats for the conv the image is FOR) and the [kv][c_in][c_out] tensor it is built from: adjoint = 0
 * is cpd_pack_weight, adjoint = 1 cpd_pack_weight_adjoint(flip_taps). cpd_pack_batch_prepare (HOST call, synchronous copy)
 * writes the device table once -- the pointers must stay valid -- and returns the three grid sizes; cpd_pack_batch_run
 * rebuilds every image: images bit 0 = split-bf16, bit 1 = split-fp16 (the fp32 image always). Results are identical to
 * the per-tensor calls. */
typedef struct {
    const float *w;
    float *packed;
    int32_t kv, c_in, c_out, adjoint, flip_taps;
} cpd_pack_job;
size_t cpd_pack_batch_table_bytes(int n_jobs);
int cpd_pack_batch_prepare(const cpd_pack_job *jobs, int n_jobs, void *table, size_t table_bytes,
                           int32_t grid_blocks[3]);
int cpd_pack_batch_run(const void *table, int n_jobs, const int32_t grid_blocks[3], int images,
                       cpd_stream_t stream);
/* Packed weights of the adjoint conv used for input gradients: Wd[t'][co][ci] = W[t][ci][co],
 * t = kv-1-t' if flip_taps (SubM / stride-1: the forward rulebook is its own transpose up to the
 * tap flip) else t = t' (use with a transposed rulebook). Size: cpd_packed_weight_floats(kv, c_out, c_in). */
int cpd_pack_weight_adjoint(const float *w_kio, int kv, int c_in, int c_out, int flip_taps,
                            float *packed, cpd_stream_t stream);
/* Transposed rulebooks for the input gradient of strided convs: nbr_t[t][i] = output row that
 * input row i feeds through tap t (or -1). Sparse: out_index is the index cpd_conv_outset built. */
int cpd_rulebook_conv_transpose(const int32_t *in_indices, int n_in, int batch,
                                const int32_t in_shape[3], const int32_t ksize[3],
                                const int32_t stride[3], const int32_t pad[3], const void *out_index,
                                int32_t *nbr_t, cpd_stream_t stream);
int cpd_rulebook_conv2d_transpose(int batch, int h, int w, int kh, int kw, int stride, int pad,
                                  int32_t *nbr_t, cpd_stream_t stream);
/* CenterHead.get_loss (center_head.py:225-250) fused with its gradient, on channels-last head rows
 * [batch*hw][ld] (columns 0..7 = center(2), center_z, dim(3), rot(2); columns hm_col.. = heatmap logits):
 * hm loss = FocalLossCenterNet on clamp(sigmoid, 1e-4, 1-1e-4) (loss_utils.py:265-300) x cls_weight,
 * loc loss = sum_d code_weights[d] * RegLossCenterNet_d (masked L1 at the object pixels / max(#objects, 1),
 * loss_utils.py:315-386) x loc_weight. heat [batch][num_classes][hw], target [batch][k][8], inds / masks
 * [batch][k] int64 as assign_targets builds them. Writes d(total)/d(rows) to d_rows [batch*hw][ld] (all
 * columns) and losses[3] = {total, hm, loc} on the device; deterministic (fixed-order sums, no atomics). */
size_t cpd_center_loss_workspace_bytes(int batch, int hw, int ld);
int cpd_center_loss(const float *rows, int ld, int batch, int hw, int num_classes, int hm_col,
                    const float *heat, const float *target, const int64_t *inds,
                    const int64_t *masks, int k, const float code_weights[8], float loc_weight,
                    float cls_weight, float *d_rows, float *losses, void *ws, size_t ws_bytes,
                    cpd_stream_t stream);
/* CenterHead.assign_targets / assign_target_of_single_head (center_head.py:103-219) with centernet_utils.gaussian_radius /
 * draw_gaussian_to_heatmap (centernet_utils.py:9-69) for every sample of a batch, on the device, nothing read back (the reference
 * walks the boxes on the CPU, l.204). gt_boxes [batch][m][8] = x, y, z, dx, dy, dz, heading, class (1..num_classes; < 1 = padding):
 * the boxes with class >= 1 are taken in their order (l.180-196), the first k of them (NUM_MAX_OBJS, l.113) give
 * heat [batch][num_classes][h][w] (gaussians of radius max(min_radius, int(gaussian_radius(dx, dy / pixel, gaussian_overlap))),
 * max-merged), target [batch][k][8] = (x - int x, y - int y, z, log dx, log dy, log dz, cos, sin), inds [batch][k] = y * w + x of the
 * centre pixel, masks [batch][k] = 1 -- boxes with dx <= 0 or dy <= 0 and unused slots give zeros. fp32 in the reference's operation
 * order; the gaussian in double, rounded to float (numpy). Outputs must be 16-byte aligned; m <= 12000. Deterministic. Three launches. */
size_t cpd_center_targets_workspace_bytes(int batch, int k);
int cpd_center_targets(const float *gt_boxes, int batch, int m, int num_classes, int h, int w, int k,
                       const float pc_range_xy[2], const float voxel_xy[2], int feature_map_stride,
                       double gaussian_overlap, int min_radius, float *heat, float *target, int64_t *inds,
                       int64_t *masks, void *ws, size_t ws_bytes, cpd_stream_t stream);
/* AnchorHeadTemplate.get_loss (anchor_head_template.py:179-334) fused with its gradient: sigmoid focal
 * classification loss (alpha 0.25, gamma 2), smooth-L1 (beta 1/9, code_weights) on the residual-coded boxes
 * with the sin-difference heading encoding, cross entropy on the direction bins (dir_preds NULL: no direction
 * classifier); per-sample normalisation by max(#positive anchors, 1), sums divided by batch, times the three
 * loss weights. cls_preds [batch][n_anchors][num_class], box_preds / reg_targets [batch][n_anchors][7],
 * dir_preds [batch][n_anchors][num_dir_bins], labels [batch][n_anchors] (-1 ignore, 0 background, k class k:
 * what cpd_anchor_assign emits), anchors [n_anchors][7]. Outputs: d_cls / d_box / d_dir (same shapes as the
 * predictions) and losses[4] = {total, cls, loc, dir} on the device. Deterministic.                       */
size_t cpd_anchor_loss_workspace_bytes(int batch, int n_anchors);
int cpd_anchor_loss(const float *cls_preds, const float *box_preds, const float *dir_preds,
                    const int32_t *labels, const float *reg_targets, const float *anchors, int batch,
                    int n_anchors, int num_class, int num_dir_bins, float dir_offset,
                    const float code_weights[7], float cls_weight, float loc_weight, float dir_weight,
                    float *d_cls, float *d_box, float *d_dir, float *losses, void *ws,
                    size_t ws_bytes, cpd_stream_t stream);
/* RoIHeadTemplate.get_loss (roi_head_template.py:148-267) of the anchor-head VoxelRCNN fused with its gradient, for n RoI rows
 * (n = batch x ROI_PER_IMAGE): rcnn_cls [n], rcnn_reg / rois [n][7], gt_of_rois (canonical frame) [n][ld_gt] and gt_of_rois_src
 * [n][ld_src] (columns 0..6 used), reg_valid_mask [n] (> 0 = foreground) and rcnn_cls_labels [n] (fractional targets, < 0 ignore),
 * all fp32. Terms: cls = binary cross entropy on sigmoid(rcnn_cls) (torch's -100 log clamp) over the rows with label >= 0 /
 * max(#valid, 1) x cls_weight; reg = smooth-L1 (beta 1/9, code_weights) against the ResidualCoder targets of the canonical gt (RoI
 * with xyz and heading zeroed as the anchor, sizes clamp_min 1e-5), NaN targets ignored, sum over the foreground / max(fg, 1) x
 * reg_weight; corner (corner_regularization and fg > 0) = get_corner_loss_lidar of the decoded boxes (RoI heading kept, rotated and
 * moved to the RoI) against gt_of_rois_src, mean over the foreground x corner_weight; bb = bbloss.bb_loss of the boxes decoded
 * against the RoI with xyz and heading zeroed vs the canonical gt, sum over the foreground / (fg + 1), unweighted, 0 when fg = 0.
 * Writes d(total)/d(rcnn_cls) to d_cls [n], d(total)/d(rcnn_reg) to d_reg [n][7] and losses[6] = {total, cls, reg, corner, bb, fg}
 * on the device. One launch, no workspace, nothing read back; deterministic (fixed-order sums, no atomics). n = 0 writes zero
 * losses (the row pointers may then be NULL).                                                                                   */
int cpd_rcnn_loss(const float *rcnn_cls, const float *rcnn_reg, const float *rois, const float *gt_of_rois, int ld_gt,
                  const float *gt_of_rois_src, int ld_src, const float *reg_valid_mask, const float *rcnn_cls_labels, int n,
                  const float code_weights[7], float cls_weight, float reg_weight, float corner_weight,
                  int corner_regularization, float *d_cls, float *d_reg, float *losses, cpd_stream_t stream);
/* VoxelRCNNProtoHead.get_loss (voxel_rcnn_head.py:388-579: two get_box_cls_layer_loss, two get_box_reg_layer_loss, proto_loss) fused
 * with its gradient, for n RoI rows. Branch 0 is the detection branch, branch 1 the prototype branch: cls0 / cls1 [n], reg0 / reg1
 * [n][7], feat0 / feat1 [n][feat_dim] (the shared features, feat_dim >= 1). The target rows serve both branches and are
 * cpd_rcnn_loss's, plus css_score [n], the prototype confidence. With valid = label >= 0, V = #valid, fgp = mask > 0, Fp = #fgp,
 * fgc = mask x css > 0, Fc = #fgc, Sv = sum valid x css:
 *   cls_j    = cls_weight x sum valid x css x BCE(sigmoid(cls_j), label) / max(V, 1)        (the css weights the numerator only)
 *   reg_j    = reg_weight x sum over fgc of smooth-L1 (beta 1/9, code_weights) / max(Fc, 1)  (cpd_rcnn_loss's targets, NaN rule)
 *   corner_j = corner_weight x mean over fgc of get_corner_loss_lidar                        (corner_regularization and Fc > 0)
 *   b0       = sum over fgp of css x bb_loss(p0, canonical gt, sizes clamp_min 1e-5) / (Fp + 1), 0 when Fp = 0; p_j = reg_j decoded
 *              against the RoI with xyz and heading zeroed
 *   b1       = ramp_weight^2 x sum over fgp of css x bb_loss(p0, p1) / (Fp + 1), p1 a constant (the reference ramps it twice)
 *   feat     = ramp_weight x sum valid x css x (-cos(feat0, feat1)) / max(Sv, 1), feat1 a constant; cos is torch.cosine_similarity:
 *              sum (x / max(|x|, 1e-8)) (y / max(|y|, 1e-8)), whose backward passes through the norm below the bound too (the clamp is
 *              outside the graph) and gives the norm no gradient at a zero vector
 *   total    = cls0 + reg0 + corner0 + proto_weight x (0.5 cls1 + 0.5 (reg1 + corner1) + b0 + b1 + feat)
 * Writes d(total)/d(cls0, reg0, feat0, cls1, reg1) (feat1 and p1 get none; d_feat0 is zero on rows of zero weight) and
 * losses[12] = {total, cls0, reg0, corner0, cls1, reg1, corner1, b0, b1, feat, Fc, Fp} on the device: the branch terms before the
 * 0.5 and proto_weight factors, b1 and feat after their ramp factors. One launch, one workgroup, no workspace, nothing read back;
 * deterministic (fixed-order sums, no atomics). n = 0 writes zero losses (the row pointers may then be NULL).                      */
int cpd_rcnn_proto_loss(const float *cls0, const float *reg0, const float *feat0, const float *cls1, const float *reg1,
                        const float *feat1, int feat_dim, const float *rois, const float *gt_of_rois, int ld_gt,
                        const float *gt_of_rois_src, int ld_src, const float *reg_valid_mask, const float *rcnn_cls_labels,
                        const float *css_score, int n, const float code_weights[7], float cls_weight, float reg_weight,
                        float corner_weight, float proto_weight, float ramp_weight, int corner_regularization, float *d_cls0,
                        float *d_reg0, float *d_feat0, float *d_cls1, float *d_reg1, float *losses, cpd_stream_t stream);
/* The RoI head's proposal-target layer on the device: ProposalTargetLayer (cpd/models/roi_heads/target_assigner/
 * proposal_target_layer.py:32-427: forward, sample_rois_for_rcnn, subsample_rois, get_max_iou_with_same_class) and the canonical
 * transformation of RoIHeadTemplate.assign_targets (cpd/models/roi_heads/roi_head_template.py:116-146) in TWO launches for a whole
 * batch, whatever the batch size and class count. The random numbers stay with the caller: cpd_roi_targets_classify, one read-back of
 * `counts`, the caller's draws (they depend on the counts only), one upload of `picks`, cpd_roi_targets_gather.
 * rois [batch][n][7] f32 (zero padding rows take part, as in the reference), roi_labels [batch][n] i64, roi_scores [batch][n] f32,
 * gt_boxes [batch][m][gt_ld] f32 (gt_ld >= 7; columns 0:7 the box, the LAST column the class), n >= 1, m >= 1, batch <= 65535.
 *
 * cpd_roi_targets_classify. A frame's ground truth is rows 0 .. k, k the last row whose fp32 sum over all gt_ld columns is not zero
 * and never below 0 (l.221-225; cpd_recall_record's rule: zero rows before row k stay, an all-zero block keeps row 0). Every RoI gets
 * its largest cpd_boxes_iou3d value (the same expression, the same bits) over the kept rows -- by_class != 0
 * (SAMPLE_ROI_BY_EACH_CLASS): over the kept rows whose class, truncated to an integer, equals the RoI's label, overlap 0 and row 0 when
 * there is none -- and the LOWEST row that attains it (torch.max(dim=1) on the device). Three pools follow, with thresholds compared
 * as fp32: fg = overlap >= fg_thresh, hard = bg_thresh_lo <= overlap < reg_thresh, easy = overlap < bg_thresh_lo; a RoI may be in
 * fg and hard at once. n_thresh == 0: scalar thresholds fg_thresh[0] (= min(REG_FG_THRESH, CLS_FG_THRESH)) and reg_thresh[0];
 * n_thresh = 1 .. CPD_ROI_TARGETS_MAX_CLASSES: per-class lists (roi_iou_x / roi_ioud_x, l.300-325), entry c serving the RoIs whose
 * assigned row has class c + 1, the others in neither fg nor hard. Both are HOST arrays.
 * Outputs: counts [batch][4] i32 = the lengths of fg, hard, easy and the kept row count; and in the workspace, five pieces of
 * cpd_roi_targets_workspace_bytes(batch, n) / 5 bytes each, every one a [batch][n] array: max_overlaps f32, assignment i32, then the
 * fg, hard and easy pools as ascending RoI indices (nonzero() order; the entries past a pool's length are not written).
 * One workgroup per frame, stable compaction by ballot and prefix: two calls agree bit for bit.
 *
 * cpd_roi_targets_gather reads that workspace and `counts` (device) and picks [batch][per_image][2] i32 = (pool 0 / 1 / 2, position in
 * the pool) per sampled slot (a pick outside its pool reads RoI 0). It writes, per slot: out_rois [..][7], out_roi_labels i64,
 * out_roi_scores, out_gt_iou, out_gt_src [..][gt_ld] (the assigned row, all columns), out_gt_canonical [..][gt_ld] (NULL to skip:
 * the row with its centre moved by the RoI's, turned by -(heading mod 2 pi), the opposite-facing half turn folded and the heading
 * clamped to +-pi/2, operation for operation in fp32), extras_out[k] [batch][per_image] = extras_in[k] [batch][m] through the
 * assignment for each non-NULL k (css_score, outline_cls_mask, outline_reg_mask; extras_in may itself be NULL), out_reg_valid i64 and
 * out_cls_labels (i64 for CPD_ROI_SCORE_CLS, f32 otherwise) for score_type = CLS_SCORE_TYPE (l.57-196). Host arrays of n_cls entries
 * (1 for the scalar types): reg_fg_thresh, cls_fg_thresh, cls_bg_thresh, cls_inv_span = float(1 / (CLS_FG_THRESH - CLS_BG_THRESH)) with
 * the difference and the reciprocal formed in double; for the _X types entry c serves assigned class c + 1, and hard_thresh / hard_every / hard_offset (NULL:
 * ENABLE_HARD_SAMPLING off) switch the batch rows hard_offset[c], + hard_every[c], ... on (hard_every[c] = int(1 /
 * HARD_SAMPLING_RATIO[c]), hard_offset[c] the caller's draw; the reference indexes dimension 0 of the mask). direction (the _IOUD
 * types) = DIRECTION_MIN, DIRECTION_MAX, float(1 / (MAX - MIN)). The soft labels are torch's fp32 kernels one rounding at a time (torch
 * divides a device tensor by a host scalar as a product with the scalar's reciprocal, formed in double and cast to float). */
#define CPD_ROI_TARGETS_MAX_CLASSES 8
#define CPD_ROI_SCORE_CLS 0
#define CPD_ROI_SCORE_ROI_IOU 1
#define CPD_ROI_SCORE_ROI_IOUD 2
#define CPD_ROI_SCORE_ROI_IOU_X 3
#define CPD_ROI_SCORE_ROI_IOUD_X 4
size_t cpd_roi_targets_workspace_bytes(int batch, int n);
int cpd_roi_targets_classify(const float *rois, const int64_t *roi_labels, int batch, int n, const float *gt_boxes, int m,
                             int gt_ld, int by_class, const float *fg_thresh, const float *reg_thresh, int n_thresh,
                             float bg_thresh_lo, int32_t *counts, void *ws, size_t ws_bytes, cpd_stream_t stream);
int cpd_roi_targets_gather(const float *rois, const int64_t *roi_labels, const float *roi_scores, int batch, int n,
                           const float *gt_boxes, int m, int gt_ld, const float *const extras_in[3], const int32_t *picks,
                           int per_image, const int32_t *counts, const void *ws, size_t ws_bytes, int score_type, int n_cls,
                           const float *reg_fg_thresh, const float *cls_fg_thresh, const float *cls_bg_thresh,
                           const float *cls_inv_span, const float *hard_thresh, const int32_t *hard_every,
                           const int32_t *hard_offset, const float direction[3], float *out_rois, int64_t *out_roi_labels,
                           float *out_roi_scores, float *out_gt_iou, float *out_gt_src, float *out_gt_canonical,
                           int64_t *out_reg_valid, void *out_cls_labels, float *const extras_out[3], cpd_stream_t stream);
/* Adam with decoupled weight decay on a flat buffer (tools/train_utils/optimization/fastai_optim.py:
 * 132-150 true_wd semantics): grad is multiplied first by grad_scale (1/world after all-reduce) and,
 * when grad_scale_dev is not NULL, by the float it points to in device memory (the clip factor of
 * clip_grad_norm_, computed on the device so that the step needs no host read-back). `step` counts
 * from 1.                                                                                        */
int cpd_adam_step(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, size_t n,
                  float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                  float grad_scale, const float *grad_scale_dev, cpd_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * RoI-head feature pooling: the pointnet2_stack CUDA extension's voxel query and
 * grouping (cpd/ops/pointnet2/pointnet2_stack/src/pointnet2_api.cpp: voxel_query_wrapper,
 * group_points_wrapper) and generate_voxel2pinds (cpd/utils/spconv_utils.py:4-21).
 * ------------------------------------------------------------------------------------------ */
/* Dense (B,Z,Y,X) int32 volume: row of the voxel in `indices` [n,4] (b,z,y,x), -1 = empty. */
int cpd_voxel2pinds(const int32_t *indices, int n, int batch, const int32_t shape_zyx[3],
                    int32_t *out_volume, cpd_stream_t stream);
/* voxel_query_wrapper (voxel_query_gpu.cu:10-87): for each of m query points (new_xyz [m,3],
 * new_coords [m,4] = (b,z,y,x) voxel coordinates) scan the (2zr+1)(2yr+1)(2xr+1) neighbourhood in
 * dz, dy, dx order and keep the first `nsample` voxels whose centre (xyz [N,3]) lies within
 * `radius`; the first hit pre-fills all slots; no hit: idx[0] = -1 and the other slots are left
 * as the caller initialised them (the reference zero-fills). idx [m, nsample] i32. */
int cpd_voxel_query(int m, int r1, int r2, int r3, int nsample, float radius, int z_range, int y_range,
                    int x_range, const float *new_xyz, const float *xyz, const int32_t *new_coords,
                    const int32_t *point_indices, int32_t *idx, cpd_stream_t stream);
/* Same query through a site index (cpd_index_build / cpd_conv_outset) of the sparse tensor instead
 * of the dense volume. Whether the index's ranks are row ids (canonical lists of cpd_conv_outset)
 * or go through its rank -> row permutation (cpd_index_build over any row order) is recorded in
 * the index and read on the device; `use_perm` is ignored (kept for ABI stability). */
int cpd_voxel_query_index(int m, int batch, int r1, int r2, int r3, int nsample, float radius,
                          int z_range, int y_range, int x_range, const float *new_xyz, const float *xyz,
                          const int32_t *new_coords, const void *index, int use_perm, int n_sites,
                          int32_t *idx, cpd_stream_t stream);
/* RoI grid points and their cell coordinates in one launch: VoxelRCNNHead.get_global_grid_points_of_roi + the `cur_coords` arithmetic of
 * roi_grid_pool (cpd/models/roi_heads/voxel_rcnn_head.py:186-273, 365-386; rotate_points_along_z, cpd/utils/common_utils.py:35-57).
 * rois [n_rois, roi_ld >= 7] (x, y, z, dx, dy, dz, heading), frame of RoI i = i / rois_per_frame. grid_xyz [n_rois * G^3, 3] = the global
 * grid points (fp32, the reference's operation order); for each of n_levels (<= 4) strides, level_coords[l] [n_rois * G^3, 4] int32 =
 * (b, x, y, z) with x = ((px - range_lo.x) // voxel_size.x) // stride (torch floor division on floats, then int), or (b, z, y, x) when
 * bzyx != 0 (the order the neighbour queries take). level_coords pointers must be 16-byte aligned. */
int cpd_roi_grid_points(const float *rois, int roi_ld, int n_rois, int rois_per_frame, int grid_size, const float voxel_size[3],
                        const float range_lo[3], int n_levels, const int32_t *strides, int32_t *const *level_coords, int bzyx,
                        float *grid_xyz, cpd_stream_t stream);
/* The same query for a VOXEL level, where the reference passes xyz = get_voxel_centers(indices) (common_utils.py:66-82;
 * voxel_rcnn_head.py:236-241): a site's coordinates are (cell + 0.5) * cell_xyz + origin_xyz per axis in fp32, so the kernel evaluates
 * the distance test from the cell coordinates (same operations, same order: identical decisions) and reads nothing per candidate
 * until it is a hit. cell_xyz = fp32(voxel_size) * stride, origin_xyz = point_cloud_range[0:3] (host arrays, x y z).
 * 2 * x_range + 1 <= 32, else CPD_ERR_UNSUPPORTED (use cpd_voxel_query_index). */
int cpd_voxel_query_index_grid(int m, int batch, int r1, int r2, int r3, int nsample, float radius,
                               int z_range, int y_range, int x_range, const float *new_xyz,
                               const int32_t *new_coords, const void *index, int n_sites,
                               const float cell_xyz[3], const float origin_xyz[3], int32_t *idx, cpd_stream_t stream);
/* group_points_wrapper (group_points_gpu.cu:69-99): out[pt][c][s] = features[start(batch of pt) +
 * idx[pt][s]][c]; *_batch_cnt are device int32[b]. out [m, c, nsample]. */
int cpd_group_points(int b, int m, int c, int nsample, const float *features,
                     const int32_t *features_batch_cnt, const int32_t *idx, const int32_t *idx_batch_cnt,
                     float *out, cpd_stream_t stream);
/* group_points_grad_wrapper (group_points_gpu.cu:9-66): grad_features [n, c] (zeroed here) += grad_out [m, c, nsample]
 * scattered through idx; the backward of cpd_group_points. Float atomics: the summation order is not fixed, as in the
 * reference. */
int cpd_group_points_grad(int b, int m, int c, int nsample, int n, const float *grad_out,
                          const int32_t *features_batch_cnt, const int32_t *idx, const int32_t *idx_batch_cnt,
                          float *grad_features, cpd_stream_t stream);
/* Fused grouping + position encoding + ReLU + max-pool of NeighborVoxelSAModuleMSG.forward
 * (voxel_pool_modules.py:96-117): out[m][ch] = max_s relu(features_in[idx[m][s]][ch] +
 * (xyz[idx[m][s]] - new_xyz[m]) . w_pos[:, ch] + b_pos[ch]), relu(b_pos[ch]) for an empty ball
 * (idx[m][0] < 0). idx holds global rows; w_pos [3, c] / b_pos [c] = Conv2d(3, c) with its
 * eval BatchNorm folded. A NaN feature or offset in a ball gives NaN (torch's ReLU and max), here and through the
 * output MLP of cpd_voxel_pool_max_mlp below: the range block of the _ranged form then holds a NaN's bits. */
int cpd_voxel_pool_max(int m, int c, int nsample, const float *features_in, int features_ld,
                       const float *xyz, const float *new_xyz, const int32_t *idx, const float *w_pos,
                       const float *b_pos, float *out, int out_ld, cpd_stream_t stream);
/* ... followed in the same kernel by the module's output MLP (mlps_out, voxel_pool_modules.py:118-121: 1 x 1 conv, eval BatchNorm,
 * ReLU): out[m][co] = act(sum_ch pooled[m][ch] * w_out[ch][co] + t_out[co]), w_out [c, c_out] with the BatchNorm scale folded in,
 * t_out [c_out] its shift; the pooled [m, c] tensor is never stored. out may be a column block of a wider row (out_ld): the
 * scales of a level are written side by side, as the reference's torch.cat lays them out. c = 16, 32 or 64 and c_out <= 2 c,
 * else CPD_ERR_UNSUPPORTED. */
int cpd_voxel_pool_max_mlp(int m, int c, int nsample, const float *features_in, int features_ld,
                           const float *xyz, const float *new_xyz, const int32_t *idx, const float *w_pos,
                           const float *b_pos, const float *w_out, const float *t_out, int c_out, int relu,
                           float *out, int out_ld, cpd_stream_t stream);
/* ... and raising `out_absmax` (an absmax block, see cpd_gather_conv_ranged; may be NULL) to the bits of max |out| of the rows this call
 * writes: the RoI head's 27648-wide pooled rows (voxel_rcnn_head.py:186-273 -> shared_fc_layers, l.694-705) reach the split-fp16 FC
 * GEMMs with their range block already filled -- no separate pass over 880 MB of pooled features. */
int cpd_voxel_pool_max_mlp_ranged(int m, int c, int nsample, const float *features_in, int features_ld,
                                  const float *xyz, const float *new_xyz, const int32_t *idx, const float *w_pos,
                                  const float *b_pos, const float *w_out, const float *t_out, int c_out, int relu,
                                  float *out, int out_ld, uint32_t *out_absmax, cpd_stream_t stream);
/* The same pooling for TRAINING, fused and differentiable (voxel_pool_modules.py:96-117 with mlps_pos = Conv2d(3, c, bias=False) +
 * BatchNorm2d on batch statistics): no (m, c, nsample) tensor is stored. With p[m][s] = xyz[idx[m][s]] - new_xyz[m] (0 for an empty
 * ball, idx[m][0] < 0) and n = m * nsample slots -- empty balls and pre-filled duplicates count, as in the reference -- the position
 * branch's batch statistics follow from the moments of p. Row conventions as cpd_voxel_pool_max (features_ld, out_ld, global idx);
 * every gather is guarded: a row outside [0, n_rows) counts as an empty slot. c = 16, 32 or 64 and nsample <= 255, else
 * CPD_ERR_UNSUPPORTED; m * nsample <= 1 is CPD_ERR_ARG (no batch statistics).
 * Workspace of the moments and the gradient entry (device memory, 256-byte aligned): */
size_t cpd_voxel_pool_train_workspace_bytes(int m, int c, int nsample);
/* moments [9] (device float64) = sum p (x y z), sum p p^T (xx xy xz yy yz zz) over all slots (voxel_pool_modules.py:96-117: the input
 * of mlps_pos), accumulated in float64 in a fixed order: bitwise repeatable. */
int cpd_voxel_pool_moments(int m, int nsample, int n_rows, const float *xyz, const float *new_xyz, const int32_t *idx,
                           double *moments, void *workspace, size_t workspace_bytes, cpd_stream_t stream);
/* Forward (voxel_pool_modules.py:96-117). Per channel ch with w = w_pos[ch] (w_pos [c, 3] = the Conv2d weight):
 *   mean = w . S1 / n, var = w (S2 / n - S1 S1^T / n^2) w^T (biased), invstd = 1 / sqrt(var + eps)       -> mean [c], invstd [c]
 *   running_mean / running_var [c] (may both be NULL) updated in place with `momentum` and the unbiased variance, torch's rule
 *   out[m][ch] = max_s relu(keep[m] * features_in[idx[m][s]][ch] + gamma[ch] * ((w . p[m][s]) - mean) * invstd + beta[ch])
 *   arg[m][ch] (uint8, [m, c]) = the first s attaining the maximum, or 255 where out == 0 (no gradient: torch's ReLU rule). */
int cpd_voxel_pool_max_train(int m, int c, int nsample, int n_rows, const float *features_in, int features_ld, const float *xyz,
                             const float *new_xyz, const int32_t *idx, const float *w_pos, const float *gamma, const float *beta,
                             const double *moments, float eps, float momentum, float *running_mean, float *running_var,
                             float *out, int out_ld, uint8_t *arg, float *mean, float *invstd, cpd_stream_t stream);
/* Backward (voxel_pool_modules.py:96-117). With G = grad_out where arg != 255, else 0, and p*, zhat* the values at arg:
 *   grad_features [n_rows, c] (zeroed here) [idx[m][arg]][ch] += keep * G          (float atomics, as cpd_group_points_grad)
 *   grad_beta = sum G, grad_gamma = sum G zhat*,
 *   grad_w [c, 3] = gamma invstd [ sum G p* - (sum G / n) S1 - (sum G zhat* / n) invstd (S2 w - mean S1) ]
 * the three sums in float64 in a fixed order (bitwise repeatable). No gradient reaches xyz / new_xyz. */
int cpd_voxel_pool_max_train_grad(int m, int c, int nsample, int n_rows, const float *grad_out, int grad_out_ld, const uint8_t *arg,
                                  const int32_t *idx, const float *xyz, const float *new_xyz, const float *w_pos, const float *gamma,
                                  const float *mean, const float *invstd, const double *moments, float eps, float *grad_features,
                                  float *grad_w, float *grad_gamma, float *grad_beta, void *workspace, size_t workspace_bytes,
                                  cpd_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Dataloader pre-filter on the device.
 * ------------------------------------------------------------------------------------------ */
/* mask_points_by_range + boolean indexing (cpd/utils/common_utils.py:60-63,
 * data_processor.py:84-85): keeps, in order, the rows of points [n, c] with range[0] <= x <= range[3]
 * and range[1] <= y <= range[4]. out [n, c]; n_out device int32. */
size_t cpd_mask_points_workspace_bytes(int n);
int cpd_mask_points_by_range(const float *points, int n, int c, const float range_xyz[6], float *out,
                             int32_t *n_out, void *workspace, size_t workspace_bytes, cpd_stream_t stream);
/* Multi-sweep merge (waymo_unsupervised_dataset.py:333-360 get_frame with 192-202 points_rigid_transform): the sweeps'
 * points [sweep_offsets[n_sweeps], c] (sweeps back to back; sweep_offsets, poses and cur_pose_inv are HOST arrays) are taken
 * sweep -> world by poses[s] (row-major 4x4 float64) and world -> current frame by cur_pose_inv = inverse(current pose),
 * each product formed in float64 from the float32 coordinates and rounded to float32 as the reference's np.mat arithmetic
 * does; column 3 (intensity) and the last column are set to 0 (l.347-351); other columns are copied. n_sweeps <= 16. */
int cpd_merge_sweeps(const float *points, const int32_t *sweep_offsets, int n_sweeps, int c, const double *poses,
                     const double *cur_pose_inv, float *out, cpd_stream_t stream);
/* points_in_boxes_gpu (roiaware_pool3d_kernel.cu:313-336; check_pt_in_box3d l.23-35 uses MARGIN
 * 1e-5, the CPU twin roiaware_pool3d.cpp:128-140 1e-2): boxes [batch, boxes_num, 7], pts
 * [batch, pts_num, pts_ld >= 3] -> box_idx_of_points [batch, pts_num] = first containing box or -1. */
int cpd_points_in_boxes(int batch, int boxes_num, int pts_num, const float *boxes, const float *pts,
                        int pts_ld, float margin, int32_t *box_idx_of_points, cpd_stream_t stream);

/* Prototype box crop, the point work of sample_prototype_cpu (waymo_unsupervised_dataset.py:205-331).
 * cpd_points_in_boxes_mask = roiaware_pool3d_utils.points_in_boxes_cpu (roiaware_pool3d.cpp:128-168, MARGIN 1e-2, double
 * comparisons): out [k][n] = 1 where point n lies in box k. */
int cpd_points_in_boxes_mask(const float *boxes, int k, const float *pts, int n, int pts_ld, int32_t *out,
                             cpd_stream_t stream);
/* The two retained clouds of l.255-259 / l.317-318 in one pass, without the k x n matrix: out_no_object = the rows of
 * points [n][c] that lie in NO box, out_good_object = the rows that lie in no box with discard[k] != 0; both stable
 * (order preserved), counts on the device. Same in-box test as cpd_points_in_boxes_mask. */
size_t cpd_crop_boxes_workspace_bytes(int n);
int cpd_crop_boxes(const float *points, int n, int c, const float *boxes, const int32_t *discard, int k,
                   float *out_no_object, int32_t *n_no_object, float *out_good_object, int32_t *n_good_object,
                   void *workspace, size_t workspace_bytes, cpd_stream_t stream);
/* Prototype placement (l.277-305): rows (x, y, z, 1) of points [n][ld] times A^T, then times B^T (row-major 4x4 doubles:
 * A = inverse of the prototype box's pose, B = the target box's pose), float64 products without contraction; out [n][c_out]
 * gets the first three components rounded to fp32 and zeros in the other columns. */
int cpd_transform_points(const float *points, int n, int ld, const double a[16], const double b[16], int c_out,
                         float *out, cpd_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Anchor head: anchor_head_template.py / axis_aligned_target_assigner.py / box_utils.py.
 * ------------------------------------------------------------------------------------------ */
/* box_utils.boxes3d_nearest_bev_iou (box_utils.py:275-287): a [n,7], b [m,7] -> out [n,m]. */
int cpd_nearest_bev_iou(const float *a, int n, const float *b, int m, float *out, cpd_stream_t stream);
/* AxisAlignedTargetAssigner.assign_targets_single (axis_aligned_target_assigner.py:153-243) with
 * match_height = False and POS_FRACTION < 0: per-anchor max/argmax IoU and per-GT max are computed
 * without an n x m matrix in HBM. labels [n] (-1 ignore, 0 background, class id), bbox_targets [n,7]
 * (ResidualCoder.encode_torch), reg_weights [n], gt_ious [n]; m <= 2048. */
size_t cpd_anchor_assign_workspace_bytes(int n, int m);
int cpd_anchor_assign(const float *anchors, int n, const float *gt_boxes, int m, const int32_t *gt_classes,
                      float matched_threshold, float unmatched_threshold, int norm_by_num_examples,
                      int32_t *labels, float *bbox_targets, float *reg_weights, float *gt_ious,
                      void *workspace, size_t workspace_bytes, cpd_stream_t stream);
/* AxisAlignedTargetAssigner.assign_targets (l.46-151) for a whole batch: every (frame, anchor set) pair in at most three launches
 * and two memsets, with cpd_anchor_assign's arithmetic per pair and the reference's output layout. anchors [sum(set_n)][7], the
 * sets one after another (device); the five set_* arrays are HOST arrays of n_sets <= 8 entries: anchors per set, anchors per
 * outer position (outer = set_n / set_inner, the reference's feature_map_size product, must be the same for all sets), the
 * 1-based position of the set's class in class_names (each class at most once), the two thresholds. gt_boxes
 * [batch][m][gt_ld] (device), columns 0-6 the box, column gt_ld - 1 the class id as a float; gt_ld >= 8, m <= 2048. Per frame,
 * on the device: rows 0 .. last with a non-zero column among 0 .. gt_ld - 2 are kept (at least row 0); a kept row with class id c
 * (truncated to int) belongs to the set of class c, and for c <= 0 of class c + num_classes -- Python's index wrap in the
 * reference's class_names[c - 1]: an all-zero row goes to the LAST class; rows keep their order inside a set. Anchor i of set s
 * goes to column (i / set_inner[s]) * sum(set_inner) + set_inner[0] + ... + set_inner[s - 1] + i % set_inner[s] of its frame.
 * Outputs: labels, reg_weights, gt_ious [batch][sum(set_n)], bbox_targets [batch][sum(set_n)][7], and the state between the
 * passes, zeroed here: gt_max_iou [batch][m] = per row the largest IoU an anchor of its set attains (0: none, or a dropped row),
 * n_examples [batch][n_sets] = labels >= 0 per pair (the divisor under norm_by_num_examples). No workspace. */
int cpd_anchor_assign_batch(const float *anchors, int n_sets, const int32_t set_n[], const int32_t set_inner[],
                            const int32_t set_class[], const float set_matched[], const float set_unmatched[],
                            int num_classes, const float *gt_boxes, int batch, int m, int gt_ld,
                            int norm_by_num_examples, int32_t *labels, float *bbox_targets, float *reg_weights,
                            float *gt_ious, float *gt_max_iou, int32_t *n_examples, cpd_stream_t stream);
/* AnchorHeadTemplate.generate_predicted_boxes (anchor_head_template.py:336-383): ResidualCoder
 * decode of box_preds [batch,n,7] against anchors [n,7] plus the direction-classifier correction
 * (dir_cls_preds [batch,n,num_dir_bins] or NULL). out [batch,n,7]. */
int cpd_anchor_decode(const float *box_preds, const float *anchors, const float *dir_cls_preds, int batch,
                      int n, int num_dir_bins, float dir_offset, float dir_limit_offset, float *out,
                      cpd_stream_t stream);

/* ATSSTargetAssigner.assign_targets_single (atss_target_assigner.py:76-141) for ONE frame and ONE anchor set, without the
 * n x m IoU / distance / "ious_inf" matrices the reference builds: per GT the `topk` nearest anchors (ties: lower index; the
 * reference's torch.topk leaves them unspecified), their IoUs (boxes_iou_bev, or boxes_iou3d_gpu when match_height), the
 * mean + std threshold and the centre-in-box test; per anchor the candidate GT of highest IoU; then every GT's argmax anchor
 * (lowest index on ties, anchor 0 when nothing overlaps) is forced to it, in GT order. gt_boxes [m][gt_ld], columns 0-6 the
 * box, column gt_ld-1 the class (float, as in gt_boxes_with_classes), trailing all-zero rows already trimmed (l.40-45).
 * Outputs (zeroed here): labels [n] float class ids (0 = background), reg_targets [n][7] (ResidualCoder.encode_torch),
 * reg_weights [n]. topk <= 64, topk * m <= 4096. */
size_t cpd_atss_workspace_bytes(int m, int topk);
int cpd_atss_assign(const float *anchors, int n_anchors, const float *gt_boxes, int gt_ld, int m, int topk,
                    int match_height, float *labels, float *reg_targets, float *reg_weights, void *workspace,
                    size_t workspace_bytes, cpd_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * KITTI-protocol evaluation (csrc/kitti_eval.hip): the numba / numba.cuda hot loops of
 * cpd/datasets/kitti/kitti_object_eval_python/eval.py and rotate_iou.py, for all frames of a set at once.
 * Frames are CSR segments: dt_off / gt_off / dc_off [n_frames + 1] int32 row offsets (device), pair_off
 * [n_frames + 1] int64 offsets of each frame's dt x gt block in the packed overlaps (pair_off[f + 1] - pair_off[f]
 * = n_dt(f) * n_gt(f); block row-major, dt rows, gt columns: the reference's overlaps[f]).
 * ------------------------------------------------------------------------------------------ */
/* calculate_iou_partly(dt_annos, gt_annos, metric) (eval.py:340-415, called at l.485) without the cross-frame blocks:
 *   metric 0: image_box_overlap (eval.py:91-117), dt / gt [n][4] float64 bbox, `criterion` as there;
 *   metric 1: rotate_iou_gpu_eval (rotate_iou.py:17-330), dt / gt [n][5] float32 (x, z, l, w, ry), `criterion` -1 / 0 / 1 / 2
 *             (0 divides by the gt = query box's area: the launcher calls devRotateIoUEval(query, box), l.289-291);
 *   metric 2: d3_box_overlap (eval.py:121-155), dt / gt [n][7] float64 camera boxes (x, y, z, l, h, w, ry): float32 BEV
 *             intersection times the float64 height overlap over the union (`criterion` picks the divisor as in
 *             d3_box_overlap_kernel), rounded to float32.
 * out [n_pairs] float64. At most 8 intersection points per pair (the reference's buffer). */
int cpd_kitti_overlaps(int metric, int criterion, const void *dt_boxes, const void *gt_boxes, const int32_t *dt_off,
                       const int32_t *gt_off, const int64_t *pair_off, int n_frames, int64_t n_pairs, double *out,
                       cpd_stream_t stream);
/* Workspace of cpd_kitti_match_scores / cpd_kitti_match_pr (HOST): n_sweeps x 41 x n_frames per-frame results + flags. */
size_t cpd_kitti_match_workspace_bytes(int n_sweeps, int n_frames, int total_dt);
/* compute_statistics_jit(compute_fp=False) (eval.py:158-259) as eval_class's first loop calls it (l.502-517), for every
 * sweep s (one (class, difficulty, min_overlap): ignored-flag row sweep_cd[s] of ig_gt [n_cd][total_gt] / ig_dt
 * [n_cd][total_dt], int8 -1 / 0 / 1 from clean_data; threshold sweep_min_overlap[s]) and frame. Outputs [n_sweeps][total_gt]:
 * matched[s][g] = 1 where the reference appends a score to `thresholds` for gt g, scores[s][g] that score (strict > on the
 * score, lowest detection index on ties). dt_score [total_dt] float64. */
int cpd_kitti_match_scores(const double *overlaps, const int64_t *pair_off, const int32_t *dt_off, const int32_t *gt_off,
                           int n_frames, const int8_t *ig_gt, const int8_t *ig_dt, const double *dt_score,
                           const int32_t *sweep_cd, const double *sweep_min_overlap, int n_sweeps, int total_gt, int total_dt,
                           double *scores, int8_t *matched, void *workspace, size_t workspace_bytes, cpd_stream_t stream);
/* fused_compute_statistics (eval.py:275-337) -> compute_statistics_jit(compute_fp=True) for every sweep, frame and
 * threshold t < n_thresholds[s] of thresholds [n_sweeps][41] (get_thresholds' output), summed over frames in frame order:
 * pr_counts [n_sweeps][41][3] int64 tp / fp / fn, pr_sim [n_sweeps][41] float64 similarity (frames whose similarity is -1
 * skipped); rows t >= n_thresholds[s] are zero. metric 0 applies the don't-care suppression (dc_bbox [total_dc][4] float64);
 * compute_aos adds (1 + cos(gt alpha - dt alpha)) / 2 per true positive. dt_bbox [total_dt][4], dt / gt alpha float64. */
int cpd_kitti_match_pr(const double *overlaps, const int64_t *pair_off, const int32_t *dt_off, const int32_t *gt_off,
                       const int32_t *dc_off, int n_frames, const int8_t *ig_gt, const int8_t *ig_dt, const double *dt_score,
                       const double *dt_alpha, const double *gt_alpha, const double *dt_bbox, const double *dc_bbox, int metric,
                       int compute_aos, const int32_t *sweep_cd, const double *sweep_min_overlap, const double *thresholds,
                       const int32_t *n_thresholds, int n_sweeps, int total_gt, int total_dt, int64_t *pr_counts,
                       double *pr_sim, void *workspace, size_t workspace_bytes, cpd_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Waymo-protocol detection metrics (csrc/waymo_eval.hip): the per-frame work behind
 * cpd/datasets/waymo_unsupervised/waymo_eval.py (waymo_evaluation, l.178-216; its metric config, build_config l.86-108:
 * object types 1..4 with IoU thresholds 0.7 / 0.5 / 0.5 / 0.5, levels 1 and 2, 101 score cut-offs, Hungarian matcher, 3-D boxes).
 * The metric op itself is outside the reference tree; the protocol computed here is the one cpd_amd/waymo_eval.py states.
 * A "problem" is one (frame, type): problem q = 4 * frame + (type - 1), n_problems = 4 * n_frames. Problems are CSR segments:
 * pd_off / gt_off [n_problems + 1] int32 row offsets (device), pair_off [n_problems + 1] int64 offsets of each problem's
 * prediction x ground-truth block in the packed IoUs (row-major, prediction rows, ground-truth columns). */
#define CPD_WAYMO_TYPES 4
#define CPD_WAYMO_CUTOFFS 101   /* c_k = (float)(k * 0.01) for k < 100, c_100 = 1 */
#define CPD_WAYMO_MAX_PD 4096   /* predictions per problem  */
#define CPD_WAYMO_MAX_GT 1024   /* ground truths per problem */
/* Rotated 3-D IoU of every pair of every problem (the boxes the estimator feeds its op, generate_waymo_type_results l.26-84):
 * rows (cx, cy, cz, dx, dy, dz, heading) float32, dx along the heading; float64 arithmetic; BEV rectangle intersection times
 * the z overlap over the union; 0 for an empty intersection, a non-positive union or a non-finite value. out [n_pairs] float64. */
int cpd_waymo_iou(const float *pd_boxes, const float *gt_boxes, const int32_t *pd_off, const int32_t *gt_off,
                  const int64_t *pair_off, int n_problems, int64_t n_pairs, double *out, cpd_stream_t stream);
/* The same for the BEV protocol (cpd/datasets/waymo_unsupervised/waymo_eval2d.py:63,69,87-102: box_type TYPE_2D, the boxes are
 * columns [0, 1, 3, 4, 6], thresholds 0.5 / 0.3 / 0.3 / 0.3): rows (cx, cy, dx, dy, heading) float32, stride 5, dx along the
 * heading; float64 arithmetic; area of the two rotated rectangles' intersection over dx_a dy_a + dx_b dy_b - that area, with no
 * z term: boxes one above the other overlap. 0 for an empty intersection, fewer than 3 clipped vertices, a non-positive union,
 * a size that is not positive, a non-finite value, and any value of magnitude 2^29 or more (which holds neither a position nor
 * a direction in float32).
 * Same packing and arguments as cpd_waymo_iou; cpd_waymo_match takes the block as it is, with column 4 as the headings. */
int cpd_waymo_iou_bev(const float *pd_boxes, const float *gt_boxes, const int32_t *pd_off, const int32_t *gt_off,
                      const int64_t *pair_off, int n_problems, int64_t n_pairs, double *out, cpd_stream_t stream);
/* Workspace of cpd_waymo_match (HOST): the score order of total_pd predictions and 101 per-problem results. */
size_t cpd_waymo_match_workspace_bytes(int n_problems, int total_pd);
/* The counts the metric op accumulates for waymo_evaluation (l.206-215): per problem and cut-off k the maximum-weight matching
 * (sum of IoU over pairs with IoU >= iou_thresholds[type - 1], HOST [4]) of the predictions with score >= c_k and all ground
 * truths; summed over frames in frame order into counts [4][2 levels][101][3] int64 (tp, fp, fn) and ha [4][2][101] float64
 * (sum over true positives of 1 - |wrap(heading difference)| / pi). A ground truth counts at level 1 when gt_difficulty == 1 and
 * at level 2 when it is 1 or 2; fp = unmatched predictions. pd_score / pd_heading [total_pd] float32, gt_difficulty [total_gt]
 * uint8, gt_heading [total_gt] float32. max_pd / max_gt: the largest row / column count of a problem (they size the LDS;
 * beyond CPD_WAYMO_MAX_PD / CPD_WAYMO_MAX_GT: CPD_ERR_UNSUPPORTED; a problem larger than them poisons the result: counts -1,
 * ha NaN). accumulate != 0 continues from the values in counts / ha (the next chunk of frames of the same set). */
int cpd_waymo_match(const double *iou, const int64_t *pair_off, const int32_t *pd_off, const int32_t *gt_off, int n_problems,
                    int total_pd, int total_gt, const float *pd_score, const uint8_t *gt_difficulty, const float *pd_heading,
                    const float *gt_heading, const double *iou_thresholds, int max_pd, int max_gt, int accumulate,
                    int64_t *counts, double *ha, void *workspace, size_t workspace_bytes, cpd_stream_t stream);

/* Diagnostic (csrc/diag.hip; replaces nothing in the reference): the matrix pipe's sustained rate on THIS part under its socket power
 * cap -- `blocks` workgroups of four waves, each wave `iters` x 16 v_mfma_f32_16x16x32_f16 on register operands (a 64 x 64 x 32 tile
 * step), nothing else in the loop. a_operands / b_operands: 512 x 16 bytes of fp16 values each (what the operand DATA is matters: the
 * clock the cap allows depends on it); sink: blocks * 256 floats. cpd_mfma_burn_flops: the flops of one such launch (HOST only).
 * bench.py times it beside the dominant kernel: roofline.power_capped_peak. */
double cpd_mfma_burn_flops(int blocks, int iters);
int cpd_mfma_burn(const void *a_operands, const void *b_operands, float *sink, int blocks, int iters, cpd_stream_t stream);

/* ---- DBSCAN pseudo-label generator (csrc/outline.hip): cpd/unsupervised_core/outline_utils.py OutlineFitter.remove_ground /
 * clustering / box_fit (l.542-576, 789-846, 609-701, 761-787) and ground_removal.py Processor / Segmentation (l.60-242) for a
 * batch of frames. frame_off is a DEVICE int32 array [n_frames + 1] of row offsets (n_points = frame_off[n_frames]). No host
 * synchronisation and no allocation inside a call. */
size_t cpd_outline_ground_workspace_bytes(int n_frames, int n_points);
/* remove_ground: points [n_points][row_stride] float16 (is_half = 1) or float32, x y z in the first three columns. consts =
 * (pi, 2 pi / 150, 0.3, 149.7 / 150, ground_max_threshold) rounded to the input dtype; thr [n_bands] = ground_min_threshold, dist [7] =
 * ground_min_distance padded (entries 0 .. max(1, n_bands - 1) are read; they must not decrease from entry 1 on), 1 <= n_bands
 * <= 6. Frame f's non-ground points go to out_xyz [n_points][3] / out_src (row within the frame) at rows frame_off[f] ..
 * frame_off[f] + out_count[f], in the canonical order (distance bands; in a band the high points in input order, then the low
 * points by segment, input order within a segment). *err |= 1 when a segment index falls outside the table (not expected). */
int cpd_outline_ground(const void *points, int is_half, int row_stride, const int32_t *frame_off, int n_frames, int n_points,
                       const float consts[5], double sensor_height, const double *thr, const double *dist, int n_bands,
                       float *out_xyz, int32_t *out_src, int32_t *out_count, int32_t *err, void *workspace,
                       size_t workspace_bytes, cpd_stream_t stream);
size_t cpd_outline_dbscan_workspace_bytes(int n_frames, int n_points);
/* sklearn.cluster.DBSCAN(eps, min_samples).fit(xyz).labels_ per frame (clustering, l.789-807): frame f = rows frame_off[f] ..
 * frame_off[f] + frame_count[f] (DEVICE [n_frames]) of xyz [n_points][3] float32, neighbours by float64
 * (dx*dx + dy*dy) + dz*dz <= eps*eps. labels [n_points] (-1 noise and padding rows), n_clusters [n_frames]. n_frames <= 1023. */
int cpd_outline_dbscan(const float *xyz, const int32_t *frame_off, const int32_t *frame_count, int n_frames, int n_points,
                       double eps, int min_samples, int32_t *labels, int32_t *n_clusters, void *workspace,
                       size_t workspace_bytes, cpd_stream_t stream);
size_t cpd_outline_boxes_workspace_bytes(int n_frames, int n_points);
/* box_fit over the clusters of cpd_outline_dbscan's labels (rows as there): with apply_cluster_filter the clustering filter
 * (size > cluster_min_points, max z < discard_max_height) first. params = (cluster_min_points, discard_max_height,
 * min_box_volume, min_box_height, max_box_volume, max_box_len, ground_min_threshold[0], ground_min_distance[1]). Every hull
 * edge is a candidate angle (the reference omits the closing edge). out [n_frames + 8 * box_cap] float64: box
 * counts per frame, then the boxes frame by frame in cluster order, each [x y z dx dy dz heading, cluster number]; boxes past
 * box_cap are counted but not written. */
int cpd_outline_boxes(const float *xyz, const int32_t *frame_off, const int32_t *frame_count, int n_frames, int n_points,
                      const int32_t *labels, const int32_t *n_clusters, int apply_cluster_filter, const double params[8],
                      int box_cap, double *out, void *workspace, size_t workspace_bytes, cpd_stream_t stream);

/* ---- PP-score precompute (csrc/ppscore.hip): cpd/unsupervised_core/precompute_ppscore.py for ONE current frame against its
 * n_trav <= 16 traversals. Caller-owned workspace; no allocation, no read-back, no host synchronisation inside a call. */
size_t cpd_ppscore_workspace_bytes(int n_query, int n_ref_total, int n_trav);
/* compute_ppscore (l.23-34: one cKDTree per traversal, count_neighbors l.8-14, compute_ephe_score l.16-21) with the two
 * points_rigid_transform products of save_pp_score (l.36-45, 85-94) folded in. query [n_query][query_stride] and ref
 * [n_ref_total][ref_stride] are DEVICE rows of float32 (dtype 0) or float16 (dtype 1), x y z in the first three columns;
 * traversal t is rows trav_offsets[t] .. trav_offsets[t + 1] of ref (HOST int32 [n_trav + 1], trav_offsets[0] = 0). poses (HOST
 * [n_trav][16] row-major sweep -> world) and cur_pose_inv (HOST [16], inverse of the current pose) are given together or both
 * NULL (ref is already in the current frame): each product is the float64 accumulation of the reference's np.mat product
 * (m0*x, then fused multiply-adds of m1*y and m2*z, then + m3) rounded to float32. The query
 * rows are used as they are (the reference does not transform them). counts [n_query][n_trav] (DEVICE, may be NULL): points
 * of traversal t with float64 (dx*dx + dy*dy) + dz*dz <= radius*radius, inclusive. h [n_query] (DEVICE, may be NULL): the
 * normalised entropy H = sum_t -P log(P + 1e-8) / log(n_trav), P = c / (sum c + 1e-8), as float16 bits; NaN (0x7e00) where
 * n_trav < 2 (the reference divides by log(1) = 0). An empty traversal gives a zero column; n_query = 0 is legal.
 * CPD_ERR_UNSUPPORTED: n_trav > 16; CPD_ERR_ARG: radius <= 0 or NaN, bad offsets / strides / dtypes. */
int cpd_ppscore(const void *query, int n_query, int query_stride, int query_dtype, const void *ref, const int32_t *trav_offsets,
                int n_trav, int ref_stride, int ref_dtype, const double *poses, const double *cur_pose_inv, double radius,
                int32_t *counts, uint16_t *h, void *workspace, size_t workspace_bytes, cpd_stream_t stream);

/* ---- C_PROTO refiner, first stage (csrc/cproto.hip): cpd/unsupervised_core/c_proto_refine.py:65-195
 * compute_css_score_and_raw_proto for n_segments <= 1022 SEGMENTS, a segment = one (frame, box) pair of a chunk of frames. Ground
 * removal and DBSCAN between cpd_cproto_filter and cpd_cproto_score are cpd_outline_ground / cpd_outline_dbscan with
 * n_frames = n_segments + 1 and frame_off = filt_off. All arrays are DEVICE memory unless marked HOST. Caller-owned workspace; no
 * allocation, no read-back, no host synchronisation inside a call. */
size_t cpd_cproto_crop_workspace_bytes(int n_segments);
/* Radius crop (l.120-123), counting pass. points / is_half / row_stride / frame_off / n_frames as in cpd_outline_ground; boxes
 * [n_segments][7] float64; seg_frame [n_segments] the frame of each segment. A row of the segment's frame is kept when
 * sqrt(dx*dx + dy*dy) < max(box[3], box[4]) in float64 (strict). seg_off [n_segments + 1]: row offsets of the segments' slices;
 * seg_off[n_segments] is the total the caller reads to size the buffers of the calls below. */
int cpd_cproto_crop_count(const void *points, int is_half, int row_stride, const int32_t *frame_off, int n_frames,
                          const double *boxes, const int32_t *seg_frame, int n_segments, int32_t *seg_off, void *workspace,
                          size_t workspace_bytes, cpd_stream_t stream);
/* Radius crop, filling pass: the kept rows in input order, x y z in the input dtype, to out_rows [n_rows][3] and their row
 * within the frame to out_src [n_rows]; n_rows = seg_off[n_segments] (rows past n_rows are never written). */
int cpd_cproto_crop_fill(const void *points, int is_half, int row_stride, const int32_t *frame_off, int n_frames,
                         const double *boxes, const int32_t *seg_frame, int n_segments, const int32_t *seg_off, int n_rows,
                         void *out_rows, int32_t *out_src, cpd_stream_t stream);
size_t cpd_cproto_filter_workspace_bytes(int n_segments, int n_rows);
/* smooth_points (outline_utils.py:391-396) and the height window (l.125-147) over the crop (rows / seg_off / crop_src = the
 * crop's out_rows / seg_off / out_src). dens_mask [n_rows]: 1 where more than 3 rows of the same segment, the row itself
 * included, lie within float64 (dx*dx + dy*dy) + dz*dz <= radius*radius. z_min [S]: the least z of the dense rows, or
 * box[2] - box[5] / 2 where there are none; new_box [S][7] = [x, y, h/2 + z_min, l, w, h, yaw] with h = max(box[2] + box[5]/2 -
 * z_min, 1.3), where the clamp applies and dense rows exist h/2 + z_min is the sum in the input dtype (numpy 2 adds
 * the Python float 0.65 to the z_min scalar in its dtype); had_points [S]: 1 where dense rows exist. filt_rows [n_rows][3] (input dtype) / filt_src [n_rows] (row within
 * the frame): the dense rows with z > T(z_min + 0.2) (the sum rounded to the input dtype) and float64 z < box[2] + box[5]/2,
 * order kept, segment s at filt_off[s] .. filt_off[s + 1]. filt_off has n_segments + 2 entries: the rows from
 * filt_off[n_segments] to n_rows = filt_off[n_segments + 1] are zeroed and form one more segment, which holds no non-ground
 * row, so that the calls that follow keep n_points = n_rows without a read-back. */
int cpd_cproto_filter(const void *rows, int is_half, const int32_t *seg_off, const int32_t *crop_src, const double *boxes,
                      int n_segments, int n_rows, double radius, uint8_t *dens_mask, double *z_min, double *new_box,
                      int32_t *had_points, void *filt_rows, int32_t *filt_src, int32_t *filt_off, void *workspace,
                      size_t workspace_bytes, cpd_stream_t stream);
size_t cpd_cproto_score_workspace_bytes(int n_segments, int n_rows);
/* The cluster the reference scores (clustering l.789-807, l.151-159) and compute_confidence's cell counts (l.398-436).
 * ng_xyz / ng_src / ng_count = cpd_outline_ground's out_xyz / out_src / out_count, labels / n_clusters = cpd_outline_dbscan's.
 * A segment scores when had_points, ng_count > min_rows (the reference's 10) and a cluster with more than cluster_min_points rows and max z <
 * discard_max_height exists; best_label [S] is the first such cluster of strictly greatest size (-1: none), best_count [S] its
 * size. m [S][8] float32: rows 0 and 1 of the inverse box transform; for the chosen rows X = ((x*m00 + y*m01) + z*m02) + m03
 * and Y likewise in float64, unfused. occ [S][n_parts]: for parts[p] (HOST, n_parts <= 4, each <= 16) the number of cells
 * (i, j) with more than one row, -l/2 + i*(l/parts) <= X < -l/2 + (i+1)*(l/parts) and the same for Y with w (l, w of new_box).
 * out_xyz [n_rows][3] / out_src [n_rows] (row within the frame): the chosen clusters' rows, segment s at out_off[s] ..
 * out_off[s + 1] (out_off [n_segments + 1]). */
int cpd_cproto_score(const float *ng_xyz, const int32_t *ng_src, const int32_t *filt_off, const int32_t *ng_count,
                     const int32_t *labels, const int32_t *n_clusters, const int32_t *had_points, const int32_t *filt_src,
                     const float *m, const double *new_box, int n_segments, int n_rows, const int32_t *parts, int n_parts,
                     int min_rows, int cluster_min_points, double discard_max_height, int32_t *occ, int32_t *best_label,
                     int32_t *best_count, int32_t *out_off, float *out_xyz, int32_t *out_src, void *workspace,
                     size_t workspace_bytes, cpd_stream_t stream);

/* ---- C_PROTO refiner, second stage (csrc/cproto_refine.hip): cpd/unsupervised_core/c_proto_refine.py:332-475 refine_box_size on
 * the segments of the first stage (n_segments <= 1022). The launch order is crop, filter, cpd_refine_fit_size, ground, dbscan,
 * score, cpd_refine_orient_drift. All arrays are DEVICE memory unless marked HOST. Caller-owned workspace; no allocation, no
 * read-back, no host synchronisation inside a call. */
/* The prototype size fit (l.410-436). new_box [S][7] is cpd_cproto_filter's output, updated in place; seg_cls [S]: 0 Vehicle,
 * 1 Pedestrian, 2 Cyclist (any other value: fit_index -1, the row untouched); basic_whl [S][3]: the whl of
 * basic_proto_set[cls][proto_id] where the box's own id is a basic prototype, a NaN row otherwise. hq_whl [3][cap][3]: each
 * class's high-quality prototype whl in the file's insertion order, hq_count (HOST [3]) of them, cap <= 64; predefined
 * (HOST [3][3]): PredifinedSize per class. fit_index [S]: -2 the own basic prototype (l.415-417); k >= 0 the first minimum of
 * |hq_whl[cls][k][2] - h|, h = new_box[5] (np.argmin, l.428); -1 the predefined size, where the class has no high-quality
 * prototype (l.423-426). Only Vehicle rows get new_box[3], new_box[4] overwritten with the fitted size (l.433-436).
 * CPD_ERR_UNSUPPORTED: cap outside 1..64; CPD_ERR_ARG: a count outside 0..cap, n_segments > 1022. */
int cpd_refine_fit_size(double *new_box, const int32_t *seg_cls, const double *basic_whl, int n_segments, const double *hq_whl,
                        const int32_t *hq_count, int cap, const double *predefined, int32_t *fit_index, cpd_stream_t stream);
size_t cpd_refine_orient_drift_workspace_bytes(int n_segments);
/* correct_orientation (outline_utils.py:127-326) and density_guided_drift (outline_utils.py:41-92) on the chosen clusters:
 * out_xyz / out_off / best_label are cpd_cproto_score's, new_box [S][7] the fitted boxes, m [S][8] float32 rows 0 and 1 of the
 * inverse box transform. Box-frame coordinates X = ((x*m00 + y*m01) + z*m02) + m03 and Y likewise in float64, unfused; the
 * forward transform's cos yaw, sin yaw, x, y are rounded to float32 (the reference's float32 trans_mat). box_drift [S][7] =
 * density_guided_drift(cluster, box); box_orient [S][7] = correct_orientation(cluster, box): the 2 x 7 bins (mid + i*delta, mid +
 * (i+1)*delta] and (min + i*delta, min + (i+1)*delta] along x when ((max_x-min_x)/l)*2 > (max_y-min_y)/w (strict), else along y,
 * per bin the row of greatest (more than half of all rows positive) or least other coordinate, ties to the lowest row, yaw +=
 * arctan of the slope between the means of the picked rows; box_orient_drift [S][7] = density_guided_drift(cluster,
 * box_orient), with the inverse of the re-oriented transform formed on the device (closed form over the float32 entries, rounded
 * to float32). All three equal new_box where best_label < 0. The workspace holds the re-oriented inverse rows. */
int cpd_refine_orient_drift(const float *out_xyz, const int32_t *out_off, const int32_t *best_label, const double *new_box,
                            const float *m, int n_segments, int n_rows, double *box_drift, double *box_orient_drift,
                            double *box_orient, void *workspace, size_t workspace_bytes, cpd_stream_t stream);

/* ---- MFCF pseudo-label generator, per-frame half (csrc/mfcf.hip): cpd/unsupervised_core/mfcf.py:46-80 for a chunk of current
 * frames. The launch order is cpd_mfcf_gather, cpd_mfcf_voxel_sample, cpd_outline_ground (float32), cpd_outline_dbscan,
 * cpd_outline_boxes, cpd_mfcf_fit_dgd. All arrays are DEVICE memory unless marked HOST. Caller-owned workspace; no allocation, no
 * read-back, no host synchronisation inside a call. */
size_t cpd_mfcf_gather_workspace_bytes(int max_rows);
/* The aggregation (mfcf.py:53-72). n_sweeps uploaded sweeps: sweep_pts (HOST [n_sweeps] device pointers to rows of
 * sweep_stride[s] >= 3 elements, float32 (sweep_dtype[s] = 0) or float16 (1), x y z first), sweep_h (HOST [n_sweeps] device
 * pointers to float16 PP scores, sweep_rows[s] each), sweep_pose (HOST [n_sweeps][16] row-major sweep -> world). Current frame
 * f: its window is sweeps win_sweep[f][0 .. win_count[f]) (HOST [n_frames][16], loop order, win_count <= 16), its own sweep
 * cur_sweep[f], cur_pose_inv (HOST [n_frames][16]) the inverse of its pose. out [out_off[n_frames]][3] float32: frame f's slice
 * starts at row out_off[f] (HOST [n_frames + 1], out_off[0] = 0, each slice at least the window's rows plus the current sweep's)
 * and holds out_count[f] (DEVICE) rows: of every window sweep in order the rows with H > thresh, taken sweep -> world -> current
 * frame by the two products of cpd_ppscore (float64 accumulation in the reference's order, each rounded to float32, l.63, 69),
 * then the current sweep's own rows converted to float32 (l.72). thresh is the threshold as numpy rounds it against a float16
 * array (l.71); both sides are compared exactly and a NaN score is dropped. max_rows for the workspace: the largest
 * window-plus-current row count. CPD_ERR_UNSUPPORTED: a window of more than 16 sweeps. */
int cpd_mfcf_gather(const void *const *sweep_pts, const void *const *sweep_h, const int32_t *sweep_rows,
                    const int32_t *sweep_stride, const int32_t *sweep_dtype, const double *sweep_pose, int n_sweeps,
                    const int32_t *win_sweep, const int32_t *win_count, const int32_t *cur_sweep, const double *cur_pose_inv,
                    const int32_t *out_off, int n_frames, float thresh, float *out, int32_t *out_count, void *workspace,
                    size_t workspace_bytes, cpd_stream_t stream);
size_t cpd_mfcf_voxel_sample_workspace_bytes(int n_frames, int n_points);
/* voxel_sampling (outline_utils.py:368-389) per frame: frame f = rows frame_off[f] .. frame_off[f] + frame_count[f] of points
 * [n_points][3] float32 (frame_off [n_frames + 1], frame_count [n_frames]; frame_off[f + 1] - frame_off[f] >= frame_count[f]).
 * The cell of a row is (x - min) // res per axis in float32 with numpy's floor_divide (the quotient of the fmod-reduced
 * numerator, floored, with its half-ulp correction), min the least coordinate of the frame; cells come out in the order of
 * their first row, each with the coordinates of its LAST row (a dict keyed by cell, values overwritten). out [n_points][3]
 * and out_src [n_points] (that row's index within its frame; may be NULL):
 * frame f's rows at out_off[f] .. out_off[f + 1], back to back; out_off has n_frames + 2 entries: the rows from
 * out_off[n_frames] to n_points = out_off[n_frames + 1] are zero and form one more frame, which holds no non-ground row, so that
 * the calls that follow take n_frames + 1 frames and n_points rows without a read-back. *err |= 1 where a coordinate is NaN or a
 * cell index does not fit 21 bits (CPD_ERR_UNSUPPORTED, reported by the caller after its one copy back), |= 2 where a slice
 * runs past n_points (its rows are left out). */
int cpd_mfcf_voxel_sample(const float *points, const int32_t *frame_off, const int32_t *frame_count, int n_frames, int n_points,
                          float res, float *out, int32_t *out_src, int32_t *out_off, int32_t *err, void *workspace,
                          size_t workspace_bytes, cpd_stream_t stream);
/* box_fit_DGD's tail (outline_utils.py:881-883) on boxes = cpd_outline_boxes' out (box_cap as there; xyz, frame_off,
 * frame_count, labels as there): for box k of frame f and cluster c the rows of the frame with label c and z > min z + 0.2
 * (box_fit's filter, l.853-856) go through density_guided_drift (l.41-92), then correct_orientation (l.127-326), then
 * correct_heading (l.444-485: ten slabs -l/2 + i*(l/10) <= X < -l/2 + (i+1)*(l/10), per non-empty slab the greatest box-frame
 * z, the mean over the slabs whose lower bound is < 0 against the mean over those whose upper bound is > 0, 0 for none, yaw +=
 * pi where the first is smaller), each step on the closed-form float32 inverse of the box the step before left (arithmetic as
 * cpd_refine_orient_drift). steps: 1 drift | 2 orientation | 4 heading select the steps that run (7: box_fit_DGD; the one-call
 * forms run one), | 8 takes every row of the cluster, without the height filter. out [box_cap][7]. bits [box_cap]: 1 drift took
 * the max side on x, 2 on y, 4 orientation binned along x, 8 it took the maxima, 16 it turned the box, 32 the heading was
 * flipped. n_out [1]: min(boxes, box_cap). One workgroup per box, any number of boxes. */
int cpd_mfcf_fit_dgd(const float *xyz, const int32_t *frame_off, const int32_t *frame_count, int n_frames, int n_points,
                     const int32_t *labels, const double *boxes, int box_cap, int steps, double *out, int32_t *bits,
                     int32_t *n_out, cpd_stream_t stream);

/* ---- OYSTER pseudo-label generator (csrc/oyster.hip): the per-track size consensus of cpd/unsupervised_core/oyster.py:89-115
 * and corner_align (outline_utils.py:94-123) for every qualifying track of a sequence in one launch. boxes [n_rows][7] float64
 * (x y z l w h yaw) in track-major order, each track's rows in frame order; track t is rows track_off[t] .. track_off[t + 1]
 * (track_off [n_tracks + 1], DEVICE like every array here, non-decreasing, within 0..n_rows: the caller checks it on the host
 * before the upload; a track whose offsets break that is skipped untouched). track_top [n_tracks]: max(3, int(n * (1 - 0.95)))
 * as Python evaluates it for the track's n rows (1 - 0.95 is 0.050000000000000044), computed on the host; clamped to 1..n.
 * Per track: dis = sqrt((x*x + y*y) + z*z), rows ordered ascending by dis (ties to the lower row, NaN last), mean_l / mean_w
 * the sums of l / w over the track_top nearest rows added one after another in that order (np.mean(axis=0)), divided by
 * their number. Per row: l_off = mean_l - l, w_off = mean_w - w; the candidates (l_off/2, w_off/2), (-, -), (+, -), (-, +) go
 * through the box's pose with cos yaw, sin yaw, x, y, z rounded to float32 (the reference's float32 trans_mat) and the products
 * and sums in float64, unfused; the candidate of the GREATEST norm of (x', y', z', 1) is taken (the reference's arg_min is an
 * argmax), the first on ties. out [n_rows][7] (not overlapping boxes): x y of that candidate, z = float32(z), l + l_off,
 * w + w_off, h and yaw as they came. Rows outside every track are not written. One workgroup per track, any track length, any
 * number of tracks; no workspace, no allocation, no read-back. n_tracks == 0 or n_rows == 0: CPD_OK without a launch.
 * CPD_ERR_ARG: a negative count, a null pointer. */
int cpd_oyster_align_tracks(const double *boxes, const int32_t *track_off, const int32_t *track_top, int n_tracks, int n_rows,
                            double *out, cpd_stream_t stream);

/* ---- training-time augmentor (csrc/augment.hip): the point work of DataAugmentor.forward with gt_sampling
 * (database_sampler.py:359-416 add_sampled_boxes_to_scene, augmentor_utils.py:8-105, common_utils.py:60-63) in one flag pass
 * and one scan / emit.
 *   scene [n][c] f32 (c >= 3); obj_base [obj_rows][c_obj] f32 (c_obj >= c): the database rows; HOST obj_start [k_obj] (first row
 *   of a pasted object in obj_base), obj_count [k_obj], obj_centre [k_obj][3] float64 -- segments in any order, overlapping or
 *   not; boxes [k][7] f32 DEVICE: the enlarged sampled boxes (k = 0: nothing is removed); HOST op_kind [n_ops] / op_param
 *   [n_ops][2], applied in order: CPD_AUG_FLIP_X y = -y; CPD_AUG_FLIP_Y x = -x; CPD_AUG_ROT with param = (cos, sin) as float32
 *   values: x' = fma(y, -sin, fl(x cos)), y' = fma(y, cos, fl(x sin)); CPD_AUG_SCALE with param[0] = f: v = fl(v * (float)f), a float32 product,
 *   for x, y, z. range_xyz HOST [6] or NULL: keep a row iff r0 <= x <= r3 && r1 <= y <= r4 after the ops (NaN: dropped).
 * out [n + m][c], m = sum(obj_count): first the object rows in segment order, columns 0-2 = (float)((double)v + centre),
 * columns 3..c-1 copied, columns >= c dropped; then the scene rows inside no box (check_pt_in_box3d_cpu, MARGIN 1e-2) in their
 * order; every row through the ops and the range test; compacted stably; *n_out (device) = rows written.
 * CPD_ERR_UNSUPPORTED: k > 512, k_obj > 512, n_ops > CPD_AUG_MAX_OPS, n + m >= 2^31. CPD_ERR_ARG: null pointers, negative
 * sizes, c_obj < c, a segment outside [0, obj_rows), an unknown op. n, m, k, n_ops may each be 0. */
#define CPD_AUG_FLIP_X 0
#define CPD_AUG_FLIP_Y 1
#define CPD_AUG_ROT 2
#define CPD_AUG_SCALE 3
#define CPD_AUG_MAX_OPS 8
size_t cpd_augment_scene_workspace_bytes(int n, int m, int k_obj);
int cpd_augment_scene(const float *scene, int n, int c, const float *obj_base, long long obj_rows, int c_obj,
                      const int64_t *obj_start, const int32_t *obj_count, const double *obj_centre, int k_obj,
                      const float *boxes, int k, const int32_t *op_kind, const double *op_param, int n_ops,
                      const float *range_xyz, float *out, int32_t *n_out, void *workspace, size_t workspace_bytes,
                      cpd_stream_t stream);

/* The point work of create_track_groundtruth_database (waymo_unsupervised_dataset.py:711-725). points [n][c] f32, box_idx [n]
 * int32 (cpd_points_in_boxes: -1 = background; ids >= k are treated as background), HOST centre [k][3] float64. out [n][c]:
 * the rows with box_idx >= 0 grouped by ascending box, point order kept inside a box, columns 0-2 = (float)((double)v - centre);
 * offsets [k + 1] device int32: box b is rows offsets[b] .. offsets[b + 1]. CPD_ERR_UNSUPPORTED: k > 1024. Any n an int holds;
 * the workspace holds two (box, block) tables of ceil(n / 2048) * k words each (8 MB at n = 2^21, k = 1024): ask the query. */
size_t cpd_group_points_by_box_workspace_bytes(int n, int k);
int cpd_group_points_by_box(const float *points, int n, int c, const int32_t *box_idx, int k, const double *centre, float *out,
                            int32_t *offsets, void *workspace, size_t workspace_bytes, cpd_stream_t stream);

/* ---- test-time augmentation around an engine step (csrc/tta.hip): TestAugmentor.forward of every view on a packed batch, and
 * TestAugmentor.backward + DetectionsMerger's per-class floor and sort (merge_detections.py:195-207) on the views' result blocks.
 * Both are queued on the stream and read nothing back.
 *
 * cpd_tta_views: points [n_total][c] f32 (c >= 3) = the frames of a batch one after the other, HOST frame_offsets [batch + 1] int64
 * (first row of a frame; [0] = 0, ascending, [batch] = n_total). Per view v < n_views a HOST op list op_kind [n_views][CPD_AUG_MAX_OPS],
 * op_param [n_views][CPD_AUG_MAX_OPS][2], n_ops [n_views], kinds and parameters as cpd_augment_scene takes them and applied by the same
 * device function. out [n_views * n_total][c]: view v of frame f is rows v * n_total + frame_offsets[f] .. v * n_total +
 * frame_offsets[f + 1] (view-major: v0f0, v0f1, .., v1f0, ..), the points in their order, columns >= 3 copied; no range filter, no
 * compaction. CPD_ERR_ARG: n_views outside 1 .. CPD_TTA_MAX_VIEWS, n_ops[v] outside 0 .. CPD_AUG_MAX_OPS, an unknown op,
 * n_views * n_total >= 2^31, offsets that are not as described, c < 3, a null pointer.
 *
 * cpd_tta_collect: the engine's results for the view-major batch as padded DEVICE blocks: boxes [n_views * batch][cap][7] f32, scores
 * [n_views * batch][cap] f32, labels [n_views * batch][cap] i64 (1-based), counts [n_views * batch] i32 (rows past a count are not
 * read). HOST: per view the REVERSED op queue as TestAugmentor.test_back_queue applies it to boxes: back_kind [n_views][CPD_AUG_MAX_OPS],
 * back_param [n_views][CPD_AUG_MAX_OPS][3], n_back [n_views]: CPD_AUG_SCALE param[0] = WORLD_SCALE: columns 0-5 /= (float)scale, float32
 * quotients; CPD_AUG_ROT param = (cos, sin, angle) of angle = -WORLD_ROT, cos / sin as the float32 values torch derives: x' = fl(fl(x cos)
 * + fl(y (-sin))), y' = fl(fl(x sin) + fl(y cos)), heading += (float)angle; CPD_AUG_FLIP_X: columns 1 and 6 = -(v + 0); CPD_AUG_FLIP_Y:
 * column 0 = -(v + 0), column 6 = -(v + (float)pi). Per class c < n_class HOST cls_floor [n_class] f32 (WBF_PRE_SCORES), cls_iou [n_class]
 * f32 (WBF_IOUS) and cls_mode [n_class] i32: 0 or CPD_WBF_MAX for a fused class, CPD_TTA_MODE_NMS for a class that goes through NMS.
 * Segment s = f * n_class + c (frame-major, classes in list order, empty ones included) is one workgroup: the candidate slots
 * p = v * cap + row of frame f in ascending p; kept: row < counts[v * batch + f], label == c + 1, score >= cls_floor[c] (float32; NaN
 * dropped); the kept slots by descending score, equal scores by ascending p (np.argsort(-scores, kind="stable")).
 * Outputs, DEVICE, the segment's rows from the FIXED row s * n_views * cap: out_boxes [S * n_views * cap][7] after the backward
 * transform, out_scores, out_src (the slot p); seg_start [S] = s * n_views * cap, seg_count [S], seg_thresh [S][2] = (cls_iou[c], 0),
 * seg_mode [S] = cls_mode[c]: the arrays cpd_wbf_cluster reads; seg_count_wbf [S] = the count for a fused class and 0 for an NMS class,
 * seg_count_nms [S] the reverse (cpd_nms_batch's counts with capacity n_views * cap). A segment of more than CPD_WBF_MAX_SEGMENT kept
 * slots gets seg_count = seg_count_wbf = -1 (cpd_wbf_cluster's refusal), seg_count_nms = 0 and no rows.
 * CPD_ERR_ARG: n_views outside 1 .. CPD_TTA_MAX_VIEWS, n_class > CPD_TTA_MAX_CLASSES, n_back[v] outside 0 .. CPD_AUG_MAX_OPS, an unknown
 * op, a zero scale, S * n_views * cap >= 2^31, a null pointer.
 *
 * cpd_tta_collect_cpu: the same on the calling thread, HOST pointers throughout (the rules of csrc/tta_rules.h compiled for the host). */
#define CPD_TTA_MAX_VIEWS 16
#define CPD_TTA_MAX_CLASSES 16
#define CPD_TTA_MODE_NMS (-1)
int cpd_tta_views(const float *points, long long n_total, int c, const int64_t *frame_offsets, int batch, const int32_t *op_kind,
                  const double *op_param, const int32_t *n_ops, int n_views, float *out, cpd_stream_t stream);
int cpd_tta_collect(const float *boxes, const float *scores, const int64_t *labels, const int32_t *counts, int n_views, int batch, int cap,
                    const int32_t *back_kind, const double *back_param, const int32_t *n_back, const float *cls_floor,
                    const float *cls_iou, const int32_t *cls_mode, int n_class, float *out_boxes, float *out_scores, int32_t *out_src,
                    int32_t *seg_start, int32_t *seg_count, int32_t *seg_count_wbf, int32_t *seg_count_nms, float *seg_thresh,
                    int32_t *seg_mode, cpd_stream_t stream);
int cpd_tta_collect_cpu(const float *boxes, const float *scores, const int64_t *labels, const int32_t *counts, int n_views, int batch,
                        int cap, const int32_t *back_kind, const double *back_param, const int32_t *n_back, const float *cls_floor,
                        const float *cls_iou, const int32_t *cls_mode, int n_class, float *out_boxes, float *out_scores,
                        int32_t *out_src, int32_t *seg_start, int32_t *seg_count, int32_t *seg_count_wbf, int32_t *seg_count_nms,
                        float *seg_thresh, int32_t *seg_mode);

#ifdef __cplusplus
}
#endif
#endif /* CPD_HIP_H */
