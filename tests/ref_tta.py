"""Shared cases and host references of the test-time-augmentation tests (test_tta_host.py on cpd_tta_collect_cpu, test_gpu_tta.py
on the device entry points): built once per process, never modified."""
import functools

import numpy as np

import ref_augment as RA

CLASSES = tuple(RA.CLASSES)
ROT = 0.39269908169872414


def view_cfg(rot=0, axis="None", scale=1):
    return [dict(NAME="world_rotation", WORLD_ROT=rot), dict(NAME="world_flip", ALONG_AXIS=axis), dict(NAME="world_scaling", WORLD_SCALE=scale)]


SHIPPED = [RA.test_view_config(rot, axis) for rot, axis in RA.TEST_VIEWS]            # the six views of the dataset configs
EIGHT = SHIPPED + [view_cfg(axis="y"), view_cfg(scale=0.95)]
ROTATED = [rot != 0 for rot, _ in RA.TEST_VIEWS] + [False, False]
INVERTIBLE = [view_cfg(), view_cfg(axis="x"), view_cfg(axis="y"), view_cfg(scale=0.95), view_cfg(axis="x", scale=0.95)]

MERGE = dict(WBF_IOUS=[0.5, 0.4, 0.3], WBF_PRE_SCORES=[0.25, 0.1, 0.3], MERGE_TYPE=["WBF-mean", "NMS", "WBF-max"], NMS_IOU=0.1)
MAX_SEGMENT = 8192


def augmentors(views):
    from cpd_amd.augmentor import TestAugmentor
    return [TestAugmentor(v, CLASSES) for v in views]


def random_boxes(rng, shape):
    b = rng.normal(size=shape + (7,)) * np.array([30, 30, 1, 0, 0, 0, 2.5])
    b[..., 3:6] = rng.uniform(0.4, 5.0, size=shape + (3,))
    return b.astype(np.float32)


def host_backward(augs, boxes, counts, batch):
    """TestAugmentor.backward per (view, frame) block of the padded [V * B, K, 7] table -> same shape, rows past a count untouched"""
    out = boxes.copy()
    for v, aug in enumerate(augs):
        for f in range(batch):
            i, c = v * batch + f, int(counts[v * batch + f])
            out[i, :c] = aug.backward(dict(boxes_lidar=boxes[i, :c].copy()))["boxes_lidar"]
    return out


def frame_lists(names_of, scores, boxes, counts, n_views, batch):
    """per frame (names, scores, boxes, slot): the views' first `count` rows concatenated in view order, as wbf.merge_frames
    concatenates them; slot = view * K + row of every entry"""
    k = scores.shape[1]
    out = []
    for f in range(batch):
        idx = [(v * batch + f, int(counts[v * batch + f])) for v in range(n_views)]
        out.append((np.concatenate([names_of[i, :c] for i, c in idx]), np.concatenate([scores[i, :c] for i, c in idx]),
                    np.concatenate([boxes[i, :c] for i, c in idx]).reshape(-1, 7),
                    np.concatenate([v * k + np.arange(c) for v, (_, c) in enumerate(idx)]).astype(np.int64)))
    return out


def label_names(labels):
    """1-based labels -> names; labels outside the class list get names no class matches"""
    table = np.array(["below"] + list(CLASSES) + ["above%d" % i for i in range(4)])
    return table[np.clip(labels, 0, len(table) - 1)]


@functools.lru_cache(maxsize=None)
def segment_case():
    """The segment case of the issue: V = 8 views, K = 1100, B = 4 frames, classes and floors of MERGE.
    frame 0: counts 1, 63, 64, 65, 0 (an empty view), 200, 300, 37; scores on a grid of 1 / 64 (ties within and across views); per class a
             score exactly at the floor and one a float32 step below; labels 0 .. 5 (0, 4 and 5 are outside the class list)
    frame 1: no box at all
    frame 2: exactly MAX_SEGMENT boxes of class 0 at or above the floor (8 x 1024), the other rows below it
    frame 3: one more than that"""
    rng = np.random.default_rng(20261)
    n_views, cap, batch = 8, 1100, 4
    counts = np.zeros((n_views, batch), np.int32)
    counts[:, 0] = [1, 63, 64, 65, 0, 200, 300, 37]
    counts[:, 2] = cap
    counts[:, 3] = cap
    scores = (rng.integers(0, 65, (n_views, batch, cap)) / 64.0).astype(np.float32)
    labels = rng.integers(0, 6, (n_views, batch, cap)).astype(np.int64)
    floors = np.asarray(MERGE["WBF_PRE_SCORES"], np.float32)
    special = {}
    for c, fl in enumerate(floors):                      # view 5 / 6 of frame 0: rows 10 + 2 c (at the floor), 11 + 2 c (one step below)
        for v in (5, 6):
            labels[v, 0, 10 + 2 * c:12 + 2 * c] = c + 1
            scores[v, 0, 10 + 2 * c] = fl
            scores[v, 0, 11 + 2 * c] = np.nextafter(fl, np.float32(0))
            special[(c, v)] = (v * cap + 10 + 2 * c, v * cap + 11 + 2 * c)
    for f, extra in ((2, 0), (3, 1)):
        labels[:, f] = 1
        scores[:, f] = np.where(np.arange(cap)[None, :] < 1024, scores[:, f] * np.float32(0.5) + np.float32(0.25), scores[:, f] * np.float32(0.2))
        scores[0, f, 1024:1024 + extra] = 0.5
        labels[:, f, 1050:] = rng.integers(2, 4, (n_views, cap - 1050))
        scores[:, f, 1050:] = (rng.integers(0, 65, (n_views, cap - 1050)) / 64.0).astype(np.float32)
    boxes = random_boxes(rng, (n_views, batch, cap))
    flat = lambda a: np.ascontiguousarray(a.reshape((n_views * batch,) + a.shape[2:]))
    case = dict(n_views=n_views, cap=cap, batch=batch, boxes=flat(boxes), scores=flat(scores), labels=flat(labels), counts=flat(counts),
                special=special)
    for a in case.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return case


@functools.lru_cache(maxsize=None)
def backward_case():
    """The backward case: the eight views, one frame, 257 boxes per view, one class with no floor: every slot is kept"""
    rng = np.random.default_rng(20262)
    n_views, cap = 8, 257
    boxes = random_boxes(rng, (n_views, cap))
    scores = rng.permutation(n_views * cap).reshape(n_views, cap).astype(np.float32) / np.float32(4096)
    case = dict(n_views=n_views, cap=cap, batch=1, boxes=boxes, scores=scores, labels=np.ones((n_views, cap), np.int64),
                counts=np.full((n_views,), cap, np.int32))
    for a in case.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return case


def xy_bound(before):
    """4 float32 units in the last place of max(|x|, |y|) of the box BEFORE the rotation: each side rounds two products to half a unit
    of at most that and their sum (at most sqrt 2 of it, so in the next binade at worst) to half a unit of the result; torch's host
    matmul may fuse one product away. 0.5 + 0.5 + 1 on our side, 0.5 + 1 on torch's."""
    return 4 * np.spacing(np.maximum(np.abs(before[..., 0]), np.abs(before[..., 1])).astype(np.float32))


def check_backward(got, want, before, rotated, what):
    """the rule of the issue for one view's back-transformed boxes"""
    if not rotated:
        assert got.tobytes() == want.tobytes(), what
        return
    assert got[..., 2:].tobytes() == want[..., 2:].tobytes(), what
    err = np.abs(got[..., :2].astype(np.float64) - want[..., :2].astype(np.float64)).max(-1)
    assert (err <= xy_bound(before)).all(), (what, float((err / xy_bound(before)).max()))
