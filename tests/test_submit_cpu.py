"""The submission csv without a GPU: the line key against sorted() of the strings, the restatement
(tests/submit_oracle.py) against the project's host path (rank.submission_frame, submission.parse_submission), the
acceptor's offsets, and the argument checks that precede the first library call."""
import io

import numpy as np
import pandas as pd
import pytest

import submit_fixtures as F
import submit_oracle as O

H = O.HEADER


def test_line_key_orders_as_the_strings():
    from otto_recommender_amd import submission as SB
    rng = np.random.default_rng(5)
    ses = list(F.SESSIONS)
    for d in range(1, 11):  # every digit count: the ends of its range and random members
        lo, hi = (0 if d == 1 else 10 ** (d - 1)), min(10 ** d - 1, 2147483647)
        ses += [lo, hi] + [int(x) for x in rng.integers(lo, hi + 1, 250)]
    ses = sorted(set(ses))
    keys = np.concatenate([SB.line_key(np.array(ses), t) for t in O.TYPES])
    names = [f"{s}_{t}" for t in O.TYPES for s in ses]
    assert len(set(keys.tolist())) == len(names) and keys.max() < 2 ** 37 and keys.min() >= 0
    assert [names[i] for i in np.argsort(keys, kind="stable")] == sorted(names)
    assert SB.line_key(123, "carts") < SB.line_key(12, "carts") < SB.line_key(12, "clicks") < SB.line_key(12, "orders")
    with pytest.raises(ValueError):
        SB.line_key(np.array([-1]), "carts")


def test_restated_writer_equals_the_host_path():
    from otto_recommender_amd import rank as R
    frames = F.random_ranked(np.random.default_rng(8), 300, 20)
    aids = np.array((F.AIDS * 2)[:len(F.SESSIONS)], np.int32)
    frames["clicks"] = pd.concat([frames["clicks"], pd.DataFrame(
        {"session": np.array(F.SESSIONS, np.int32), "aid_next": aids, "pred_rank": np.ones(len(aids), np.int16)})],
        ignore_index=True)
    del frames["orders"]
    want = R.submission_frame(frames).to_csv(index=False).encode()
    assert O.write_csv(F.as_tuples(frames), 64) == want
    # pandas writes the file unquoted
    one = {"carts": pd.DataFrame({"session": [12, 12, 12], "aid_next": [2, 1, 3], "pred_rank": [2, 1, 3]})}
    assert R.submission_frame(one).to_csv(index=False).encode() == b"session_type,labels\n12_carts,1 2 3\n"
    assert O.write_csv(F.as_tuples(one), 20) == b"session_type,labels\n12_carts,1 2 3\n"
    # the filter, and equal ranks in input order
    two = {"carts": ([5, 5, 5, 5, 7], [40, 30, 20, 10, 1], [2, 1, 2, 3, 4])}
    assert O.write_csv(two, 2) == b"session_type,labels\n5_carts,30 40 20\n"
    assert O.write_csv({}, 20) == O.write_csv({"clicks": ([], [], [])}, 20) == H
    # the edge case of the device tests, where the host path takes it (no rank above the filter)
    edge = {t: tuple(c[v[2] <= 64] for c in v) for t, v in F.edge_case().items()}
    frames = {t: pd.DataFrame(dict(zip(("session", "aid_next", "pred_rank"), v))) for t, v in edge.items()}
    assert O.write_csv(F.edge_case(), 64) == R.submission_frame(frames).to_csv(index=False).encode()


def _host_rows(data: bytes):
    from otto_recommender_amd import submission as SB
    return SB.parse_submission(pd.read_csv(io.BytesIO(data), dtype=str))


def test_restated_parser_equals_the_host_path():
    frames = F.random_ranked(np.random.default_rng(9), 200, 20)
    text = O.write_csv(F.as_tuples(frames), 20)
    for data in (text, text[:-1], O.write_csv(F.edge_case(), 64),
                 b"session_type,labels\n12_carts,1 2 3\n0_orders,0\n2147483647_clicks,2147483647 7"):
        got, want = O.parse_csv(data), _host_rows(data)
        assert got == O.parse_csv(data, fast=False)
        assert list(got) == list(want)
        for t in want:
            np.testing.assert_array_equal(np.array(got[t][0], np.int32), want[t]["session"])
            np.testing.assert_array_equal(np.array(got[t][1], np.int32), want[t]["aid_next"])
    assert O.parse_csv(H) == {} and O.parse_csv(H[:-1]) == {}
    # empty labels: the target is present with no rows
    for fast in (True, False):
        got = O.parse_csv(b"session_type,labels\n5_carts,\n6_clicks,1\n7_carts,", fast)
        assert got == {"clicks": ([6], [1]), "carts": ([], [])}


@pytest.mark.parametrize("what, data, offset, reason", F.VIOLATIONS, ids=[v[0] for v in F.VIOLATIONS])
def test_acceptor_rejects_at_the_expected_offset(what, data, offset, reason):
    assert O.parse_csv(data) == O.parse_csv(data, fast=False) == (offset, reason)
    # behind good lines the offset moves with them
    if data.startswith(H) and data != H:
        good = b"1_clicks,5 6\n" * 3
        assert O.parse_csv(H + good + data[len(H):]) == (offset + len(good), reason)


def test_acceptor_reports_the_first_of_two_bad_bytes():
    data = H + b"12_carts,1\t2\n" + b"13_views,1\n"
    assert O.parse_csv(data) == (len(H) + 10, O.BYTE)
    data = H + b"13_views,1\n" + b"12_carts,1\t2\n"
    assert O.parse_csv(data) == (len(H) + 3, O.TARGET)


@pytest.mark.parametrize("k", [0, 65, -1])
def test_keep_top_k_outside_the_rank_stage_bound(k):
    """checked before the library is loaded or a device is asked for"""
    from otto_recommender_amd import submission as SB
    ranked = {"carts": pd.DataFrame({"session": [1], "aid_next": [2], "pred_rank": [1]})}
    with pytest.raises(ValueError, match="keep_top_k"):
        SB.submission_bytes(ranked, keep_top_k=k)
    with pytest.raises(ValueError, match="keep_top_k"):
        SB.write_submission(ranked, "unused.csv", keep_top_k=k)
