#!/usr/bin/env python3
"""AxisAlignedTargetAssigner.assign_targets at Waymo size, the host loop (fused off: one cpd_anchor_assign per frame and class)
against the batched call (fused on: one cpd_anchor_assign_batch), in one process.

Three sets of 188 x 188 x 2 anchors, 20 boxes per class per frame, batch 2 (the dbscan yaml's BATCH_SIZE_PER_GPU) and batch 8
(DESIGN 5c's figure). Both paths are warmed up; a window is `--calls` calls under a host clock and ends in a device synchronise;
the two paths alternate; per path the median of `--windows` windows and their spread (min .. max) are printed in ms per call,
after a bit-for-bit comparison of the two results. Device operations per call (kernels, memsets, copies) come from the
profiler in a run of their own, after the timing."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cpd_amd import anchor_head as ah  # noqa: E402

CLASSES = ["Vehicle", "Pedestrian", "Cyclist"]
SIZES = np.array([[4.7, 2.1, 1.7], [0.91, 0.86, 1.73], [1.78, 0.84, 1.78]])


def make_gt(batch, per_class, seed=0):
    """[batch][3 * per_class + 4][8]: per frame per_class boxes of every class in a shuffled order, then padding."""
    rng = np.random.default_rng(seed)
    m = 3 * per_class
    gt = np.zeros((batch, m + 4, 8), np.float32)
    for b in range(batch):
        c = rng.permutation(np.repeat(np.arange(1, 4), per_class))
        gt[b, :m] = np.concatenate([rng.uniform(-70, 70, (m, 2)), rng.uniform(-1, 1, (m, 1)), SIZES[c - 1] * rng.uniform(0.85, 1.15, (m, 3)),
                                    rng.uniform(-3.1, 3.1, (m, 1)), c[:, None]], 1)
    return torch.from_numpy(gt).cuda()


def window(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls * 1e3


def device_ops(fn):
    """Device operations of one call, counted by the profiler: (kernels, memsets and copies)."""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    dev = [e for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA")]
    mem = sum(1 for e in dev if "memset" in e.name.lower() or "memcpy" in e.name.lower())
    return len(dev) - mem, mem


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[2, 8])
    ap.add_argument("--per-class", type=int, default=20)
    ap.add_argument("--grid", type=int, default=188)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--no-ops", action="store_true", help="skip the profiler run")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    assert args.windows >= 5
    cfgs = [dict(class_name=n, anchor_sizes=[s], anchor_rotations=[0, 1.57], anchor_bottom_heights=[0], matched_threshold=mt,
                 unmatched_threshold=ut)
            for n, s, mt, ut in (("Vehicle", SIZES[0].tolist(), 0.55, 0.5), ("Pedestrian", SIZES[1].tolist(), 0.55, 0.4),
                                 ("Cyclist", SIZES[2].tolist(), 0.55, 0.4))]
    anchors, _ = ah.AnchorGenerator([-75.2, -75.2, -2, 75.2, 75.2, 4], cfgs).generate_anchors([[args.grid, args.grid]] * 3)
    n_anchor = sum(a.numel() // 7 for a in anchors)
    loop_asg = ah.AxisAlignedTargetAssigner(cfgs, CLASSES)
    fused_asg = ah.AxisAlignedTargetAssigner(cfgs, CLASSES)
    fused_asg.fused = True
    for batch in args.batches:
        gt = make_gt(batch, args.per_class)
        paths = {"loop": lambda: loop_asg.assign_targets(anchors, gt), "fused": lambda: fused_asg.assign_targets(anchors, gt)}
        want, got = paths["loop"](), paths["fused"]()
        same = all(torch.equal(want[k], got[k]) for k in want)
        assert same, "the two paths differ"
        for fn in paths.values():                                   # warm-up: both paths, the shapes of the timed windows
            window(fn, 5)
        times = {k: [] for k in paths}
        for _ in range(args.windows):                               # alternate the paths
            for k, fn in paths.items():
                times[k].append(window(fn, args.calls))
        med = {k: statistics.median(v) for k, v in times.items()}
        print("batch %d, %d anchors x %d boxes per frame (%d positives): results equal bit for bit" %
              (batch, n_anchor, 3 * args.per_class, int((want["box_cls_labels"] > 0).sum())))
        for k in paths:
            print("  %-5s %8.3f ms per call (median of %d windows of %d calls; %.3f .. %.3f)" %
                  (k, med[k], args.windows, args.calls, min(times[k]), max(times[k])))
        print("  loop / fused = %.1f" % (med["loop"] / med["fused"]), flush=True)
    for batch in [] if args.no_ops else args.batches:               # the profiler slows the host: after all timing
        gt = make_gt(batch, args.per_class)
        for k, asg in (("loop", loop_asg), ("fused", fused_asg)):
            kernels, mem = device_ops(lambda: asg.assign_targets(anchors, gt))
            print("batch %d %-5s %d kernel launches + %d memsets / copies per call" % (batch, k, kernels, mem), flush=True)


if __name__ == "__main__":
    main()
