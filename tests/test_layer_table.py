"""cpd_amd.layer_table on the host: the table's names against init_state_dict's keys, every layout helper against its inverse on
tensors whose dimensions all differ (a transposed pair cannot hide), fuse_branches, final_shape. No kernel is launched."""
import numpy as np
import pytest
import torch

from cpd_amd import layer_table as lt
from cpd_amd.engine import ModelConfig, init_state_dict


def train_cfg():
    """the train tests' reduced config (tests/test_gpu_train.py::small_cfg)"""
    return ModelConfig(point_cloud_range=[-20.0, -20.0, -2.0, 20.0, 20.0, 4.0], post_center_limit_range=[-20, -20, -2, 20, 20, 4],
                       bev_num_filters=[64, 128], bev_num_upsample_filters=[128, 128], bev_layer_nums=[2, 2], max_obj_per_sample=100)


def numbered(*shape):
    return torch.arange(int(np.prod(shape)), dtype=torch.float32).reshape(*shape)


def same(a, b):
    assert tuple(a.shape) == tuple(b.shape)
    np.testing.assert_array_equal(a.contiguous().numpy(), b.contiguous().numpy())


@pytest.mark.parametrize("cfg", [ModelConfig(), train_cfg()], ids=["default", "train_small"])
def test_table_names_are_the_state_dict_keys(cfg):
    layers = lt.centerpoint_layers(cfg)
    names = lt.state_dict_names(layers)
    assert len(names) == len(set(names))
    keys = {k for k in init_state_dict(cfg) if not k.endswith("num_batches_tracked")}
    assert set(names) - keys == set()
    assert keys - set(names) == set()
    assert len({L.slot for L in layers}) == len(layers)
    sd = init_state_dict(cfg)
    for L in layers:
        assert tuple(sd[L.conv + ".weight"].shape) == L.weight_shape(), L.conv


def test_sparse_layout_round_trip():
    w = numbered(7, 3, 1, 2, 5)                                  # (Cout, kD, kH, kW, Cin)
    k = lt.sparse_kio(w)
    assert tuple(k.shape) == (6, 5, 7)
    assert k[4, 3, 2] == w[2, 2, 0, 0, 3]                        # tap 4 = (kd 2, kh 0, kw 0)
    same(lt.sparse_from_kio(k, (3, 1, 2)), w)
    same(lt.sparse_kio(lt.sparse_from_kio(k, (3, 1, 2))), k)


def test_conv2d_layout_round_trip():
    w = numbered(6, 5, 3, 3)                                     # (Cout, Cin, k, k)
    k = lt.conv2d_kio(w)
    assert tuple(k.shape) == (9, 5, 6)
    assert k[7, 4, 1] == w[1, 4, 2, 1]                           # tap 7 = (ky 2, kx 1)
    same(lt.conv2d_from_kio(k, 3), w)
    same(lt.conv2d_kio(lt.conv2d_from_kio(k, 3)), k)


def test_deconv_layout_round_trip():
    w = numbered(5, 4, 2, 2)                                     # (Cin, Cout, u, u)
    k = lt.deconv_kio(w, 2)
    assert tuple(k.shape) == (1, 5, 16)
    assert k[0, 3, (1 * 2 + 0) * 4 + 2] == w[3, 2, 1, 0]         # column = (tap a, b) * Cout + co
    same(lt.deconv_from_kio(k, 2, 4), w)
    same(lt.deconv_kio(lt.deconv_from_kio(k, 2, 4), 2), k)


def test_first_bev_conv_channel_permutation():
    C, D, cout = 3, 2, 4
    w = numbered(cout, C * D, 3, 3)
    z = lt.bev_first_conv_zc(w, C, D)
    assert tuple(z.shape) == tuple(w.shape)
    for c in range(C):
        for d in range(D):
            same(z[:, d * C + c], w[:, c * D + d])               # ours z*C + c  <-  the reference's c*D + z
    same(lt.bev_first_conv_from_zc(z, C, D), w)
    same(lt.bev_first_conv_zc(lt.bev_first_conv_from_zc(w, C, D), C, D), w)


def test_record_layouts_invert():
    """LayerSpec.kio / from_kio pick the helpers by kind (and the channel permutation for the first BEV conv only)."""
    cfg = train_cfg()
    depth = lt.final_shape(cfg)[0]
    seen = set()
    for L in lt.centerpoint_layers(cfg):
        key = (L.kind, L.ksize, L.first_bev)
        if key in seen:
            continue
        seen.add(key)
        w = numbered(*L.weight_shape())
        k = L.kio(w, cfg.out_features, depth)
        u2 = L.up * L.up
        assert tuple(k.shape) == (int(np.prod(L.ksize)) // u2, L.c_in, L.c_out * u2), L.conv
        same(L.from_kio(k, cfg.out_features, depth), w)
    assert {k[0] for k in seen} == {"sparse", "conv2d", "deconv"} and any(k[2] for k in seen)


@pytest.mark.parametrize("kv", [9, 1])
def test_fuse_branches(kv):
    g = torch.Generator().manual_seed(0)
    cin, widths = 4, [1, 2, 3]
    first = [torch.randn(kv, cin, cin, generator=g) for _ in widths]
    scale = [torch.randn(cin, generator=g) for _ in widths]
    shift = [torch.randn(cin, generator=g) for _ in widths]
    last = [torch.randn(kv, cin, co, generator=g) for co in widths]
    bias = [torch.randn(co, generator=g) for co in widths]
    w1, s1, t1, w2, b2, slices = lt.fuse_branches(first, scale, shift, last, bias)
    assert tuple(w1.shape) == (kv, cin, 3 * cin) and tuple(w2.shape) == (kv, 3 * cin, 6) and tuple(b2.shape) == (6,)
    assert slices == [(0, 1), (1, 2), (3, 3)]
    off = torch.ones_like(w2, dtype=torch.bool)
    for i, (col, co) in enumerate(slices):
        rows = slice(i * cin, (i + 1) * cin)
        same(w1[:, :, rows], first[i])
        same(s1[rows], scale[i])
        same(t1[rows], shift[i])
        same(w2[:, rows, col:col + co], last[i])
        same(b2[col:col + co], bias[i])
        off[:, rows, col:col + co] = False
    assert int(off.sum()) == kv * (3 * cin * 6 - cin * 6) and not w2[off].any()


def test_final_shape():
    assert lt.final_shape(ModelConfig()) == [2, 188, 188]
