"""What every *_workspace_bytes query of include/cpd_hip.h returns, pinned byte for byte (CPU only: a size query launches nothing).

A launcher carves its workspace with the layout function that answers the query, so a change of a layout shows up here before it
shows up as a kernel writing past a host's allocation. The expected values are the answers of the library as it was before the
layouts were given one definition each (recorded from a build of that commit, not from the code under test). Per query: the
smallest legal shape, a shape at which a piece's raw size is a whole number of 256-byte units, the same shape with one more element,
a refused shape (0 or 256, as the query has always answered; a few queries clamp a bad count to 1 instead), and for the queries
with a scan spine a count on either side of one 4096-item scan tile. The two row-order queries are newer than that recording:
their values are the expressions their hosts used to compute themselves. cpd_voxelize has since become the one-frame call of the
batched voxelizer: its five positive rows are what cpd_voxelize_batch_workspace_bytes(n, 1, ...) answered for the same arguments in
the library BEFORE that change (the per-frame tail of the batch layout is always there now)."""
import pytest

from cpd_amd import _lib

VS, RG = (1.0, 1.0, 1.0), (0.0, 0.0, 0.0, 8.0, 8.0, 4.0)       # voxel size and range of an 8 x 8 x 4 grid (voxelizer queries)

SIZES = {
    "cpd_voxelize_workspace_bytes": [
        ((0, 1, 1, VS, RG), 3584), ((64, 1, 64, VS, RG), 3584), ((65, 1, 65, VS, RG), 5120), ((4096, 5, 100, VS, RG), 70144),
        ((4097, 5, 100, VS, RG), 71168), ((-1, 1, 1, VS, RG), 0), ((1, 0, 1, VS, RG), 0),
    ],
    "cpd_voxelize_batch_workspace_bytes": [
        ((0, 1, 1, 1, VS, RG), 3584), ((64, 1, 1, 64, VS, RG), 3584), ((65, 1, 1, 65, VS, RG), 5120),
        ((4096, 2, 5, 100, VS, RG), 72704), ((4097, 2, 5, 100, VS, RG), 73728), ((64, 64, 1, 1, VS, RG), 6144),
        ((1, 65, 1, 1, VS, RG), 0), ((1, 0, 1, 1, VS, RG), 0),
    ],
    "cpd_center_decode_workspace_bytes": [
        ((1, 1, 1, 1), 512), ((1, 1, 64, 64), 512), ((1, 1, 65, 65), 1024), ((2, 3, 35344, 500), 24064), ((0, 1, 1, 1), 0),
    ],
    "cpd_center_peaks_workspace_bytes": [
        ((1, 1, 1, 1), 512), ((1, 1, 64, 64), 512), ((1, 1, 65, 65), 1024), ((2, 3, 35344, 500), 24064), ((1, 1, 1, 0), 0),
    ],
    "cpd_center_decode_at_peaks_workspace_bytes": [
        ((1, 1, 1), 256), ((1, 64, 1), 256), ((1, 65, 1), 512), ((2, 500, 8), 32000), ((1, 1, 0), 0),
    ],
    "cpd_nms_workspace_bytes": [
        ((1,), 256), ((32,), 256), ((33,), 512), ((64,), 512), ((65,), 1280), ((4096,), 2097152), ((4097,), 2130688), ((0,), 256),
    ],
    "cpd_wbf_workspace_bytes": [
        ((0,), 512), ((1,), 512), ((64,), 6656), ((65,), 7168), ((4096,), 425984), ((4097,), 426496), ((-1,), 512),
    ],
    "cpd_kitti_fov_workspace_bytes": [
        ((0, 0), 0), ((1, 1), 256), ((64, 1024), 256), ((65, 1024), 512), ((64, 1025), 512), ((2, 4096), 256), ((2, 4097), 256),
        ((-1, 0), 0),
    ],
    "cpd_col_reduce_workspace_bytes": [
        ((1, 1), 4096), ((1, 32), 131072), ((1, 33), 135168), ((4096, 64), 262144), ((4097, 64), 262144), ((0, 1), 0),
    ],
    "cpd_mask_points_workspace_bytes": [
        ((0,), 256), ((1,), 256), ((4096,), 256), ((4097,), 256), ((241664,), 256), ((241665,), 512), ((-1,), 256),
    ],
    "cpd_anchor_assign_workspace_bytes": [
        ((0, 0), 512), ((1, 1), 512), ((32, 60), 512), ((33, 60), 768), ((32, 61), 768), ((4096, 2048), 41216), ((4097, 2048), 41472),
        ((-1, -1), 512),
    ],
    "cpd_crop_boxes_workspace_bytes": [
        ((0,), 512), ((1,), 512), ((256,), 512), ((257,), 768), ((4096,), 4352), ((4097,), 4608), ((241664,), 241920),
        ((241665,), 242432), ((-1,), 512),
    ],
    "cpd_atss_workspace_bytes": [
        ((1, 1), 1024), ((32, 2), 1024), ((33, 2), 2048), ((32, 3), 1792), ((100, 9), 12544), ((0, 1), 256), ((1, 0), 256),
    ],
    "cpd_voxel_pool_train_workspace_bytes": [
        ((1, 16, 1), 768), ((64, 32, 16), 1280), ((65, 32, 16), 2560), ((4096, 64, 16), 327680), ((4097, 64, 16), 330240),
        ((0, 16, 1), 256), ((1, 17, 1), 256),
    ],
    "cpd_conv_wgrad_workspace_bytes": [
        ((1, 1, 1, 1), 256), ((1000, 8, 8, 1), 1024), ((1000, 5, 13, 1), 1280), ((4096, 16, 16, 27), 442368),
        ((4097, 16, 16, 27), 470016), ((0, 1, 1, 1), 0),
    ],
    "cpd_center_targets_workspace_bytes": [
        ((1, 1), 256), ((1, 16), 256), ((1, 17), 512), ((4, 500), 32000), ((0, 1), 0),
    ],
    "cpd_center_loss_workspace_bytes": [
        ((1, 1, 1), 256), ((1, 512, 10), 512), ((1, 513, 10), 768), ((2, 35344, 11), 72960), ((0, 1, 1), 0),
    ],
    "cpd_anchor_loss_workspace_bytes": [
        ((1, 1), 512), ((1, 8192), 1024), ((1, 8193), 1280), ((64, 128), 1024), ((65, 128), 1536), ((0, 1), 0),
    ],
    "cpd_roi_targets_workspace_bytes": [
        ((1, 1), 1280), ((1, 64), 1280), ((1, 65), 2560), ((4, 512), 40960), ((0, 1), 0),
    ],
    "cpd_kitti_match_workspace_bytes": [
        ((1, 1, 0), 1024), ((1, 1, 256), 1280), ((1, 1, 257), 1536), ((32, 1, 8), 26624), ((33, 1, 8), 27904), ((32, 2, 8), 52736),
        ((3, 100, 4096), 258560), ((3, 100, 4097), 258816), ((0, 1, 0), 0), ((1, 1, -1), 0),
    ],
    "cpd_waymo_match_workspace_bytes": [
        ((4, 0), 15104), ((4, 64), 15360), ((4, 65), 15616), ((64, 256), 233984), ((68, 256), 248832), ((8, 4096), 46080),
        ((8, 4097), 46336), ((3, 0), 0),
    ],
    "cpd_outline_ground_workspace_bytes": [
        ((1, 0), 826880), ((1, 64), 827392), ((1, 65), 827904), ((64, 4096), 52877312), ((65, 4097), 53704448), ((0, 0), 0),
    ],
    "cpd_outline_dbscan_workspace_bytes": [
        ((1, 0), 20992), ((1, 64), 22784), ((1, 65), 23552), ((64, 4096), 279040), ((65, 4097), 443648), ((0, 0), 0),
    ],
    "cpd_outline_boxes_workspace_bytes": [
        ((1, 0), 768), ((1, 64), 7680), ((1, 65), 9984), ((64, 4096), 443136), ((65, 4097), 445696), ((0, 0), 0),
    ],
    "cpd_ppscore_workspace_bytes": [
        ((0, 0, 0), 20736), ((64, 64, 1), 22272), ((65, 64, 1), 22528), ((64, 65, 1), 22784), ((4096, 4096, 2), 278784),
        ((4097, 4097, 2), 443392), ((0, 0, 17), 0),
    ],
    "cpd_cproto_crop_workspace_bytes": [
        ((0,), 256), ((64,), 256), ((65,), 512), ((-1,), 0),
    ],
    "cpd_cproto_filter_workspace_bytes": [
        ((0, 0), 512), ((64, 0), 512), ((65, 0), 1024), ((64, 4097), 512), ((-1, 0), 0),
    ],
    "cpd_cproto_score_workspace_bytes": [
        ((0, 0), 768), ((64, 64), 768), ((65, 64), 1024), ((64, 65), 1280), ((64, 4096), 33024), ((64, 4097), 33536), ((0, -1), 0),
    ],
    "cpd_refine_orient_drift_workspace_bytes": [
        ((0,), 256), ((8,), 256), ((9,), 512), ((-1,), 0),
    ],
    "cpd_mfcf_gather_workspace_bytes": [
        ((0,), 256), ((1,), 256), ((4096,), 256), ((4097,), 256), ((258048,), 256), ((258049,), 512), ((-1,), 0),
    ],
    "cpd_mfcf_voxel_sample_workspace_bytes": [
        ((1, 0), 512), ((1, 64), 2816), ((1, 65), 3840), ((64, 4096), 148480), ((65, 4097), 149760), ((0, 0), 0),
    ],
    "cpd_augment_scene_workspace_bytes": [
        ((0, 0, 0), 19200), ((256, 0, 0), 19200), ((257, 0, 0), 19456), ((4096, 0, 1), 23040), ((4096, 1, 1), 23296),
        ((241664, 0, 0), 260608), ((241664, 1, 0), 261120), ((-1, 0, 0), 0),
    ],
    "cpd_group_points_by_box_workspace_bytes": [
        ((0, 0), 1024), ((64, 64), 2304), ((65, 64), 2304), ((64, 65), 3072), ((4096, 4), 1024), ((4097, 4), 1024), ((1, 1025), 0),
    ],
}


def _a256(x):
    return (x + 255) // 256 * 256


# cpd_order_rows_bricks: what ops.order_rows_bricks allocated before the query existed; cpd_order_rows_by_taps: one word per row,
# NOT rounded up to 256 (include/cpd_hip.h) -- its hosts have always been free to pass exactly that
SIZES["cpd_order_rows_bricks_workspace_bytes"] = [((n,), 2 * _a256(4 * max(n, 1)) + _a256(16 * max(n, 1))) for n in (0, 1, 64, 65)]
SIZES["cpd_order_rows_by_taps_workspace_bytes"] = [((n,), max(n, 1) * 4) for n in (0, 1, 64, 65)]


def test_every_workspace_query_is_pinned():
    assert sorted(SIZES) == sorted(n for n in _lib.SIGNATURES if n.endswith("_workspace_bytes"))


def test_one_frame_voxelizer_query_is_the_batch_query_of_one_frame():
    one, batch = _lib.lib().cpd_voxelize_workspace_bytes, _lib.lib().cpd_voxelize_batch_workspace_bytes
    for (n, p, v, vs, rg), want in SIZES["cpd_voxelize_workspace_bytes"]:
        if want:
            assert one(n, p, v, _lib.farr(vs), _lib.farr(rg)) == batch(n, 1, p, v, _lib.farr(vs), _lib.farr(rg)) == want


@pytest.mark.parametrize("name", sorted(SIZES))
def test_workspace_query_sizes(name):
    query = getattr(_lib.lib(), name)
    for args, want in SIZES[name]:
        got = query(*[_lib.farr(a) if isinstance(a, tuple) else a for a in args])
        assert got == want, "%s%r = %d, was %d" % (name, args, got, want)
