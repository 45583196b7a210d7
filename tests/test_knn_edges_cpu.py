"""CPU tests of tests/knn_edges.py: the error bound E behind the certain-neighbour rule holds for an emulation
of k_knn_pack's operands (RNE bf16 factors, hi/lo norm columns, fp32 sums, the 31-ulp key) on every input the
GPU edge tests use, each input's reference reaches its cap, and check() rejects what it is there to reject."""
import numpy as np
import pytest

import knn_edges as K

NAMES = sorted(K.CAPS) + list(K.ENVELOPE)


@pytest.mark.parametrize("name", NAMES + ["normal_d1", "ties99000", "group100"])
def test_emulated_scores_stay_within_the_bound(name):
    if name == "ties99000":
        emb, groups = K.with_ties(99_000)
        rows = np.concatenate(groups)
    elif name == "group100":
        emb, rows = K.big_group()
    else:
        emb, rows = K.case(name)
    excess = K.emulation_excess(emb, rows)
    print(name, "max (|emulated - s| + key) / E =", round(excess, 4))
    assert excess <= 1.0


def test_bound_is_not_slack_by_a_factor_of_two():
    """Normal data of dim 1 comes within 3 % of the bound: the bf16 rounding error is 2^-8 of a factor, and a
    bound built on 2^-9 (half of E's first term) is exceeded."""
    assert K.emulation_excess(*K.case("normal_d1")) > 0.9


@pytest.mark.parametrize("name", sorted(K.CAPS))
def test_reference_reaches_its_cap(name):
    r = K.ref(name)
    print(name, "certain items %.4f fully certain queries %.4f" % (r.item_share, r.query_share))
    a, b = K.CAPS[name]
    assert r.item_share >= a and r.query_share >= b
    assert r.item_share <= a + 0.06 and r.query_share <= b + 0.06  # a stale cap: recompute it


def test_certain_mask_equals_its_definition():
    emb = K._normal(3000, 64, 5)
    rows = np.arange(0, 3000, 100)
    r = K.reference(emb, rows, 20)
    s, err = K.scores64(emb, rows)
    _, d21 = K.oracle.topk_exact(emb, rows, 21)
    for q in range(len(rows)):
        for j, v in enumerate(r.idx[q]):
            others = int(((s[q] + err[q]) >= (s[q, v] - err[q, v])).sum()) - 1
            resolved = d21[q, 20] - d21[q, j] > r.rr * (d21[q, 20] + d21[q, j])
            assert r.certain[q, j] == (others < K.KN_C and resolved)
    assert 0.0 < r.item_share < 1.0


def test_small_index_is_all_certain_and_padded():
    emb = K._normal(5, 100, 6)
    r = K.reference(emb, np.arange(5), 8)
    assert np.all(r.idx[:, 5:] == -1) and np.all(np.isinf(r.d2[:, 5:]))
    assert np.all(r.certain[:, :5]) and not r.certain[:, 5:].any()
    assert r.item_share == 1.0 and r.query_share == 1.0
    K.check(r, r.idx, r.d2, min_exact=1.0, min_items=1.0, min_queries=1.0)


def test_check_rejects_a_lost_certain_neighbour_and_accepts_a_lost_uncertain_one():
    emb, rows = K.case("nq")
    r = K.ref("nq")
    gi, gd = r.idx.copy(), r.d2.copy()
    K.check(r, gi, gd, min_exact=1.0)
    i21 = K.reference(emb, rows, 21)
    # the 20th neighbour swapped for the 21st where the 20th is not certain: only the share of equal sets moves
    q = int(np.flatnonzero(~r.certain[:, 19])[0])
    gi[q, 19], gd[q, 19] = i21.idx[q, 20], i21.d2[q, 20]
    assert K.check(r, gi, gd, min_exact=0.0) == pytest.approx(1 - 1 / len(rows))
    with pytest.raises(AssertionError):
        K.check(r, gi, gd, min_exact=1.0)
    # ... where it is certain: rejected whatever the share
    gi, gd = r.idx.copy(), r.d2.copy()
    q = int(np.flatnonzero(r.certain[:, 19])[0])
    gi[q, 19], gd[q, 19] = i21.idx[q, 20], i21.d2[q, 20]
    with pytest.raises(AssertionError):
        K.check(r, gi, gd, min_exact=0.0)
    # two neighbours of a fully certain query in swapped order
    gi, gd = r.idx.copy(), r.d2.copy()
    q = int(np.flatnonzero(r.certain.all(1))[0])
    assert gd[q, 4] - gd[q, 3] > 0.01  # far above the fp32 rerank's 1e-3
    gi[q, [3, 4]] = gi[q, [4, 3]]
    with pytest.raises(AssertionError):
        K.check(r, gi, gd, min_exact=0.0)
    # ... unless the fp32 rerank cannot tell the two apart
    r2 = K.Ref(r.rows, r.k, r.idx, r.d2.copy(), r.certain, r.rr, r.item_share, r.query_share)
    r2.d2[q, 4] = r2.d2[q, 3] * (1 + r.rr)
    K.check(r2, gi, r2.d2, min_exact=0.0)
    # a cap the reference does not reach fails before the result is looked at
    with pytest.raises(AssertionError):
        K.check(r, None, None, min_items=0.99)


def test_tie_groups_sit_in_distinct_blocks_and_positions_of_sampled_tiles():
    groups = K.tie_groups()
    assert len(np.unique(np.concatenate(groups))) == 72
    for r in groups:
        assert np.all((r // K.KN_IT) % K.PRE_STRIDE == 0) and r.max() < 98_304
        assert len(np.unique(r // 32)) == 24 and len(np.unique(r % 32)) == 24 and np.all(np.diff(r) > 0)
    _, rows = K.big_group()
    assert len(np.unique(rows)) == 100 and np.all((rows // K.KN_IT) % K.PRE_STRIDE == 0) and rows.max() < 99_000 - 184
