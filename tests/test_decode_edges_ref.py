"""The decode fixtures of tests/ref_decode_edges.py on the CPU: the oracle against the plain numpy restatement, the conditions that
let the reference alone decide each case, and the proof that `saturated` tells the contract's rule from bin-then-sort."""
import numpy as np
import pytest

import ref_decode_edges as R

CASES = R.cases()


def oracle_decode(oracle, logits, k, limit_range=R.WIDE, score_thresh=-1.0):
    nc, h, w = logits.shape
    return oracle.center_decode(logits, *R.maps(h, w), k, R.STRIDE, R.VOXEL, R.RANGE_LO, limit_range, score_thresh)


def test_the_issue_cases_are_all_there():
    want = (["const-k%d" % k for k in (1, 7, 500, 1024)] + ["const_per_class-k500"] + ["tie_group-k%d" % k for k in (100, 38, 2037)] +
            ["tie_group_whole-k1024", "one_bin-k100", "one_bin-k1024", "saturated-k100"] + ["quantised-k%d" % k for k in (1, 100, 500)] +
            ["whole_map_4x5-k20", "whole_map_32x32-k1024", "identical_classes-k64"])
    assert sorted(CASES) == sorted(want)
    shapes = {"const": (3, 40, 30), "const_per_class": (3, 40, 30), "tie_group": (1, 64, 64), "tie_group_whole": (1, 64, 64),
              "one_bin": (1, 32, 64), "saturated": (1, 64, 64), "quantised": (3, 64, 64), "whole_map_4x5": (3, 4, 5),
              "whole_map_32x32": (1, 32, 32), "identical_classes": (5, 8, 8)}
    for name, (logits, k, notes) in CASES.items():
        assert logits.shape == shapes[name.rsplit("-k", 1)[0]] and logits.dtype == np.float32
        assert notes["supported"] == (k <= 1024)
        assert notes["fallback"] == (name.split("-")[0] in ("const", "const_per_class", "tie_group", "tie_group_whole", "one_bin"))


@pytest.mark.parametrize("name", sorted(CASES))
def test_fixture_conditions_hold(name):
    logits, k, notes = CASES[name]
    R.check_conditions(logits, k, notes)


def test_fixture_content_is_what_the_names_say():
    tg = CASES["tie_group-k100"][0].ravel()
    level, count = np.unique(tg, return_counts=True)
    tied = level[count.argmax()]
    assert count.max() == 2000 and (tg > tied).sum() == 37 and np.unique(tg[tg > tied]).size == 37
    tw = CASES["tie_group_whole-k1024"][0].ravel()
    level, count = np.unique(tw, return_counts=True)
    tied = level[count.argmax()]
    assert count.max() == 987 and (tw > tied).sum() == 37                      # 37 + 987 = K: the whole group and nothing else
    ob = CASES["one_bin-k100"][0].ravel()
    assert np.unique(ob).size == 2048 and np.unique(R.logit_bin(ob)).size == 1
    key = R.sigmoid32(ob).view(np.uint32)                                      # the radix select works on these bits
    assert all(np.unique((key >> s) & 255).size > 1 for s in (16, 8, 0)) and np.unique(key >> 24).size == 1
    sat = CASES["saturated-k100"][0].ravel()
    assert np.isposinf(sat).sum() == 3 and np.isneginf(sat).sum() == 3 and ((sat >= 18) & np.isfinite(sat)).sum() == 147
    q = CASES["quantised-k100"][0]
    assert (q * 8 == np.round(q * 8)).all() and np.abs(q).max() <= 8
    assert np.intersect1d(q[0], q[1]).size > 50                                # levels shared across classes
    ident = CASES["identical_classes-k64"][0]
    assert (ident == ident[0]).all()
    for name in ("whole_map_4x5-k20", "whole_map_32x32-k1024", "identical_classes-k64"):
        logits, k, _ = CASES[name]
        assert k == logits.shape[1] * logits.shape[2]


@pytest.mark.parametrize("name", sorted(CASES))
def test_oracle_equals_the_numpy_restatement(oracle, name):
    logits, k, _ = CASES[name]
    boxes, scores, labels = oracle_decode(oracle, logits, k)
    rb, rs, rl, rp = R.decode_ref(logits, k)
    assert boxes.shape[0] == k == rp.size
    np.testing.assert_array_equal(boxes[:, 2].astype(np.int64), rp)            # the pixel, exactly
    np.testing.assert_array_equal(labels, rl)
    np.testing.assert_array_equal(scores.view(np.uint32), rs.view(np.uint32))  # bit for bit: both are host fp32
    np.testing.assert_array_equal(boxes, rb)
    assert (np.diff(scores) <= 0).all()


def test_known_answers():
    """What the rule gives where it can be said without a computation."""
    _, s, l, p = R.decode_ref(*CASES["const-k500"][:2])
    assert (s == np.float32(0.5)).all() and (l == 0).all() and (p == np.arange(500)).all()
    _, s, l, p = R.decode_ref(*CASES["const_per_class-k500"][:2])
    assert (l == 2).all() and (p == np.arange(500)).all()
    logits, k, _ = CASES["identical_classes-k64"]
    _, s, l, p = R.decode_ref(logits, k)
    best = R.topk_order(R.sigmoid32(logits[0]).ravel(), 64)[0]
    assert l[0] == 0 and p[0] == best and set(l.tolist()) == set(range(5))     # every score ties across the five classes: class 0 first
    logits, k, _ = CASES["saturated-k100"]
    _, s, l, p = R.decode_ref(logits, k)
    assert (p == np.nonzero(logits.ravel() >= 18)[0][:100]).all() and (s == np.float32(1.0)).all()


def test_masks_in_the_restatement_match_the_oracle(oracle):
    logits, k, _ = CASES["quantised-k100"]
    boxes, _, _, pixel = R.decode_ref(logits, k)
    x0, y0, z0 = boxes[50, :3]
    for lim, thr in (((x0, -1e9, -1e9, 1e9, 1e9, 1e9), -1.0), ((-1e9, -1e9, -1e9, 1e9, y0, z0), 0.2), (R.WIDE, 2.0)):
        b, s, l = oracle_decode(oracle, logits, k, lim, thr)
        rb, rs, rl, _ = R.decode_ref(logits, k, lim, thr)
        np.testing.assert_array_equal(b, rb)
        np.testing.assert_array_equal(s, rs)
        np.testing.assert_array_equal(l, rl)


def test_saturated_separates_the_contract_from_bin_then_sort(oracle):
    """Selecting by logit bin first and ordering by (score, index) afterwards is NOT the contract: on `saturated` every winner
    scores 1.0f, the contract takes the 100 lowest indices among all 150 of them, and the bins keep only the ~100 largest logits."""
    logits, k, _ = CASES["saturated-k100"]
    boxes, _, _ = oracle_decode(oracle, logits, k)
    want = boxes[:, 2].astype(np.int64)
    got = R.bin_then_sort_topk(logits[0], k)
    assert got is not None                                    # few enough candidates: this is the rule a histogram fast path applies
    assert np.setdiff1d(want, got).size >= 10
    # and where scores are distinct the two rules agree (the fixture, not the restatement, makes the difference)
    logits, k, _ = CASES["quantised-k100"]
    for c in range(3):
        np.testing.assert_array_equal(R.bin_then_sort_topk(logits[c], k), R.topk_order(R.sigmoid32(logits[c]).ravel(), k))
    for name in ("const-k7", "tie_group-k100", "one_bin-k100"):                # more than 1024 candidates: the fast path gives up
        assert R.bin_then_sort_topk(CASES[name][0][0], CASES[name][1]) is None
