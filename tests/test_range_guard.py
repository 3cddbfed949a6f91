"""cpd_amd/range_guard.py without a GPU: the hysteresis of RangeGuard step by step, as the engines (a verdict in every pass) and the
module path (no verdict in a guarded step) drive it, and BlockPool's hand-out, exhaustion, thresholds and reset on the CPU."""
import struct
import warnings

import pytest
import torch

from cpd_amd.range_guard import GUARDED_BITS, OPTIMISTIC_BITS, BlockPool, RangeGuard

STICKY = 16


def state(g):
    return g.reruns, g.guarded_steps, g.left


def step(g, *bits):
    """one engine step: a pass per bit; every pass but the last must ask for the re-run, the last must not"""
    g.begin_step()
    for i, bit in enumerate(bits):
        again = g.verdict(bit)
        assert again == (i + 1 < len(bits)), (i, bits)
        if again:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                g.trip()
    g.end_step()
    assert not g.scaled and not g.high


def tripped(second_bit):
    g = RangeGuard(STICKY)
    step(g, 1, second_bit)
    return g


def bits(x):
    return struct.unpack("<i", struct.pack("<f", x))[0]


def test_thresholds_are_the_bits_of_two_powers():
    assert OPTIMISTIC_BITS == bits(32768.0) == 0x47000000 and GUARDED_BITS == bits(16384.0) == 0x46800000


def test_a_step_inside_the_range_changes_nothing():
    g = RangeGuard(STICKY)
    assert state(g) == (0, 0, 0) and not g.scaled
    g.begin_step()
    assert not g.scaled and g.verdict(0) is False
    g.end_step()
    assert state(g) == (0, 0, 0)


@pytest.mark.parametrize("second_bit", [1, 0])
def test_a_trip_reruns_the_step_guarded_and_a_guarded_pass_is_never_rerun(second_bit):
    g = RangeGuard(STICKY)
    g.begin_step()
    assert g.verdict(1) is True
    with pytest.warns(UserWarning, match="range-guarded"):
        g.trip()
    assert g.left == STICKY + 1 and g.scaled
    assert g.verdict(second_bit) is False            # guarded: exact whatever the range
    g.end_step()
    assert state(g) == (1, 1, STICKY) and not g.scaled


def test_a_hot_guarded_step_extends_the_stay_and_a_cool_one_counts_down():
    for bit, left in ((1, STICKY), (0, STICKY - 1)):
        g = tripped(0)
        g.begin_step()
        assert g.scaled                              # guarded from the start: no trip
        assert g.verdict(bit) is False
        g.end_step()
        assert state(g) == (1, 2, left)


def test_sixteen_cool_guarded_steps_return_to_the_optimistic_kernels():
    g = tripped(1)
    for k in range(STICKY):
        assert g.left == STICKY - k
        step(g, 0)
    assert state(g) == (1, 1 + STICKY, 0)
    g.begin_step()
    assert not g.scaled
    g.end_step()
    g = tripped(1)                                   # a hot step in between starts the count again
    for _ in range(5):
        step(g, 0)
    step(g, 1)
    assert g.left == STICKY


def test_module_flavour_counts_down_without_verdicts():
    """CenterPoint._run_modules: a guarded step reads no verdict, so nothing extends the stay"""
    g = RangeGuard(STICKY, "model")
    g.begin_step()
    assert g.verdict(1)
    with pytest.warns(UserWarning, match="re-run.*the model stays guarded for the next 16 steps"):
        g.trip()
    assert g.left == STICKY + 1
    g.end_step()
    for left in range(STICKY, 0, -1):
        assert g.left == left
        g.begin_step()
        assert g.scaled
        g.end_step()
    assert state(g) == (1, 1 + STICKY, 0)
    g.begin_step()
    assert not g.scaled


def test_only_the_first_trip_warns():
    g = RangeGuard(2)
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        for _ in range(2):
            g.begin_step()
            assert g.verdict(1)
            g.trip()
            g.end_step()
            while g.left:
                step(g, 0)
    assert g.reruns == 2
    assert [str(w.message) for w in seen] == ["cpd_amd: an activation reached 2^15 -- step re-run with the range-guarded f16x2 kernels; "
                                              "the engine stays guarded for the next 2 steps"]


def test_block_pool_hands_out_zeroed_blocks_in_order_and_reset_rewinds():
    pool = BlockPool("pool of %d")
    pool.reset(3, "cpu")
    got = [pool.new_block() for _ in range(3)]
    assert [b.data_ptr() for b in got] == [pool.blocks[i].data_ptr() for i in range(3)]
    assert all(b.dtype == torch.int32 and int(b.abs().max()) == 0 for b in got)
    with pytest.raises(RuntimeError, match="pool of 3"):
        pool.new_block()
    got[1][0] = OPTIMISTIC_BITS
    held = pool.blocks
    pool.reset(3, "cpu")
    assert pool.blocks is held and int(held.abs().max()) == 0            # the same pool, zeroed again
    assert pool.new_block().data_ptr() == got[0].data_ptr()
    pool.reset(5, "cpu")                                                   # another size: a new pool
    assert pool.blocks.shape[0] == 5 and pool.next == 0


@pytest.mark.parametrize("threshold", [OPTIMISTIC_BITS, GUARDED_BITS])
def test_block_pool_flag_at_and_below_the_threshold(threshold):
    pool = BlockPool("%d")
    pool.reset(4, "cpu")
    blocks = [pool.new_block() for _ in range(4)]
    flag = pool.flag(threshold)
    assert flag.dtype == torch.int32 and tuple(flag.shape) == (1,) and int(flag) == 0
    blocks[2][3] = threshold - 1                                           # the largest float below the threshold
    assert int(pool.flag(threshold)) == 0
    blocks[2][3] = threshold
    assert int(pool.flag(threshold)) == 1
    for special in (float("inf"), float("nan")):
        pool.reset(4, "cpu")
        assert int(pool.flag(threshold)) == 0
        pool.new_block()[0] = bits(special)
        assert int(pool.flag(threshold)) == 1, special


def test_each_owner_s_exhaustion_error_says_where_the_pool_is_sized():
    from cpd_amd.engine import CenterPointEngine, ModelConfig
    from cpd_amd.spconv.pytorch import conv as spc

    class NoLayers(CenterPointEngine):               # (packing the weights needs the device; the guard's wiring does not)
        def _build_layers(self):
            pass
    with spc.range_pass("cpu", n_blocks=2):
        spc.record_block(), spc.record_block()
        with pytest.raises(RuntimeError, match=r"range_pass: more fused conv launches than the 2 absmax blocks"):
            spc.record_block()
    cfg = ModelConfig(conv_math="f16x2", bev_layer_nums=[1, 1])
    eng = NoLayers(cfg, {}, device="cpu")
    eng._range_reset()
    n = eng._pool.blocks.shape[0]
    assert n == 21 + 2 + 2 + 1 + 3 + 16
    for _ in range(n):
        eng._range_new()
    with pytest.raises(RuntimeError, match=r"than the %d absmax blocks the engine sized from its config \(engine\._range_reset\)" % n):
        eng._range_new()
    # the counters of the engine are the guard's
    assert (eng.range_reruns, eng.range_guarded_steps, eng._guard_left) == (0, 0, 0)
    eng.range_reruns = 3
    assert eng.guard.reruns == 3
    off = ModelConfig(conv_math="f32", bev_layer_nums=[1, 1])
    eng = NoLayers(off, {}, device="cpu")
    eng._range_reset()
    assert eng._pool is None and eng._range_new() is None and eng._range_exceeded_flag() is None


def test_the_module_detectors_own_a_guard_and_keep_their_counter_names():
    from cpd_amd import models
    for net in (models.CenterPoint(), models.VoxelRCNN()):
        assert (net.guard.sticky, net.guard.owner) == (net.FAST_EVAL_STICKY_STEPS, "model") == (16, "model")
        assert (net.range_reruns, net._guard_left) == (0, 0)
        net.guard.reruns = 2
        assert net.range_reruns == 2
        net.range_reruns = 0
        assert net.guard.reruns == 0 and "guard" not in net.state_dict() and "range_reruns" not in net.__dict__
