"""The submission csv on the device (csrc/submit.hip) against tests/submit_oracle.py and the project's host path:
the writer's bytes and the reader's rows exactly, the reader's errors at the restated acceptor's offsets."""
import io

import numpy as np
import pandas as pd
import pytest

import submit_fixtures as F
import submit_oracle as O

pytestmark = pytest.mark.gpu
H = O.HEADER


def _dev(gpu, ranked):
    import torch
    dev = torch.device("cuda", gpu.device)
    names = ("session", "aid_next", "pred_rank")
    return {t: {c: torch.from_numpy(np.ascontiguousarray(v[i])).to(dev) for i, c in enumerate(names)}
            for t, v in ranked.items()}


def _bytes(gpu, ranked, k):
    from otto_recommender_amd import submission as SB
    return SB.submission_bytes(_dev(gpu, ranked), k, gpu).cpu().numpy().tobytes()


def _host_rows(data: bytes):
    from otto_recommender_amd import submission as SB
    return SB.parse_submission(pd.read_csv(io.BytesIO(data), dtype=str))


def _check_rows(got, want):
    """got: read_submission's dict; want: the oracle's {target: (sessions, aids)}"""
    import torch
    assert list(got) == list(want)
    for t in want:
        assert got[t]["session"].dtype == got[t]["aid_next"].dtype == torch.int32 and got[t]["session"].is_cuda
        np.testing.assert_array_equal(got[t]["session"].cpu().numpy(), np.array(want[t][0], np.int32), err_msg=t)
        np.testing.assert_array_equal(got[t]["aid_next"].cpu().numpy(), np.array(want[t][1], np.int32), err_msg=t)


@pytest.fixture(scope="module")
def big():
    """~50 k sessions x 3 targets with 1-20 aids each: the frames, the restated bytes and rows (computed once)"""
    frames = F.random_ranked(np.random.default_rng(21), 50_000, 20, lo=0, hi=3_000_000)
    text = O.write_csv(F.as_tuples(frames), 20)
    return frames, text, O.parse_csv(text)


@pytest.mark.parametrize("variant", ["two targets", "carts empty", "orders absent, carts empty"])
@pytest.mark.parametrize("k", [64, 20, 1])
def test_edge_case_bytes(gpu, variant, k):
    ranked = F.edge_case()
    if variant != "two targets":
        ranked["carts"] = (np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int16))
    if variant == "orders absent, carts empty":
        del ranked["orders"]
    want = O.write_csv(ranked, k)
    assert want.count(b"\n") > 12
    assert _bytes(gpu, ranked, k) == want


def test_bytes_at_a_size_that_crosses_every_tile(gpu, big):
    from otto_recommender_amd import rank as R
    from otto_recommender_amd import submission as SB
    frames, text, _ = big
    assert sum(len(f) for f in frames.values()) > 1_000_000
    got = SB.submission_bytes(frames, 20, gpu)  # DataFrames, as rank_job returns them
    assert got.cpu().numpy().tobytes() == text
    again = SB.submission_bytes(frames, 20, gpu)
    assert bool((got == again).all())
    assert text == R.submission_frame(frames).to_csv(index=False).encode()
    # a smaller filter drops rows of every line
    assert _bytes(gpu, F.as_tuples(frames), 7) == O.write_csv(F.as_tuples(frames), 7)


def test_byte_range_edges(gpu):
    from otto_recommender_amd import submission as SB
    one = {"carts": (np.array([12, 12, 12], np.int32), np.array([2, 1, 3], np.int32), np.array([2, 1, 3], np.int16))}
    assert _bytes(gpu, one, 20) == b"session_type,labels\n12_carts,1 2 3\n"  # 35 bytes: no multiple of 16
    assert _bytes(gpu, one, 1) == b"session_type,labels\n12_carts,1\n"
    assert _bytes(gpu, {}, 20) == H
    empty = (np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int16))
    assert _bytes(gpu, {"clicks": empty, "orders": empty}, 20) == H
    filtered = {"carts": (one["carts"][0], one["carts"][1], np.array([21, 22, 23], np.int16))}
    assert _bytes(gpu, filtered, 20) == H
    buf, lines = SB._submission_bytes(_dev(gpu, one), 20, gpu)
    assert lines == 1 and buf.numel() == 35


@pytest.mark.parametrize("first_rows", [16, 24])
def test_block_boundaries_at_every_alignment(gpu, first_rows):
    """A write block owns 1024 rows. The first line, "0_carts", has first_rows aids whose digits grow by 0..31 bytes,
    so the later blocks' byte ranges start at every alignment; the lines behind it have 20 ten-digit aids each, so
    row 1024 is a line's first row (first_rows = 24: its head stands at the boundary) or a row inside a line
    (first_rows = 16: ten-digit aids on both sides of the boundary)."""
    n_lines = 110
    ses = np.repeat(np.arange(1000, 1000 + n_lines, dtype=np.int32), 20)
    aid = (2147483647 - np.arange(len(ses))).astype(np.int32)
    rank = np.tile(np.arange(1, 21, dtype=np.int16), n_lines)
    assert (first_rows + len(ses)) > 2048 and (1024 - first_rows) % 20 == (0 if first_rows == 24 else 8)
    for extra in range(32):
        a0 = np.array([10 ** min(2, max(0, extra - 2 * j)) for j in range(first_rows)], np.int32)
        ranked = {"carts": (np.r_[np.zeros(first_rows, np.int32), ses], np.r_[a0, aid],
                            np.r_[np.arange(1, first_rows + 1, dtype=np.int16), rank])}
        want = O.write_csv(ranked, 64)
        assert len(want.split(b"\n")[1]) == len("0_carts,") + 2 * first_rows - 1 + extra
        assert _bytes(gpu, ranked, 64) == want, extra


def test_rows_that_cannot_be_written(gpu):
    from otto_recommender_amd import submission as SB
    ranked = {"clicks": (np.array([1, -2, 3, 4], np.int32), np.array([5, 6, -7, -8], np.int32),
                         np.array([1, 1, 1, 30], np.int16)),
              "orders": (np.array([1, 2], np.int32), np.array([5, 6], np.int32), np.array([0, -3], np.int16))}
    with pytest.raises(ValueError, match="5 rows cannot be written: 1 with session < 0, 2 with aid_next < 0, 2 with "
                                         "pred_rank < 1"):
        SB.submission_bytes(_dev(gpu, ranked), 20, gpu)
    ranked["orders"] = (np.array([1], np.int32), np.array([5], np.int32), np.array([1], np.int16))
    ranked["clicks"] = tuple(c[:1] for c in ranked["clicks"])
    assert _bytes(gpu, ranked, 20) == H + b"1_clicks,5\n1_orders,5\n"  # the context goes on working


def test_reader_rows(gpu, big):
    from otto_recommender_amd import submission as SB
    frames, text, rows = big
    _check_rows(SB.read_submission(text, ctx=gpu), rows)
    host = _host_rows(text)
    got = SB.read_submission(text, piece_bytes=1 << 20, ctx=gpu)  # a dozen pieces
    assert list(got) == list(host)
    for t in host:
        np.testing.assert_array_equal(got[t]["session"].cpu().numpy(), host[t]["session"])
        np.testing.assert_array_equal(got[t]["aid_next"].cpu().numpy(), host[t]["aid_next"])
    edge = O.write_csv(F.edge_case(), 64)
    for data in (edge, edge[:-1], H, H[:-1], H + b"7_orders,1"):
        want = O.parse_csv(data)
        assert isinstance(want, dict)
        _check_rows(SB.read_submission(data, ctx=gpu), want)
        host = _host_rows(data)
        assert list(host) == list(want) and all(host[t]["aid_next"].tolist() == want[t][1] for t in want)
        for piece in (1, 40, 100):  # 1: every line is a piece of its own
            _check_rows(SB.read_submission(data, piece_bytes=piece, ctx=gpu), want)


def test_reader_empty_labels(gpu):
    from otto_recommender_amd import submission as SB
    for data in (H + b"5_carts,\n6_clicks,1\n7_carts,", H + b"5_carts,\n", H + b"5_orders,\n6_orders,3 4\n7_orders,\n8_clicks,\n"):
        want = O.parse_csv(data)
        assert isinstance(want, dict) and any(len(v[0]) == 0 for v in want.values())
        for piece in (None, 1):
            _check_rows(SB.read_submission(data, piece_bytes=piece, ctx=gpu), want)


@pytest.mark.parametrize("what, data, offset, reason", F.VIOLATIONS, ids=[v[0] for v in F.VIOLATIONS])
def test_reader_errors(gpu, what, data, offset, reason):
    from otto_recommender_amd import submission as SB
    good = b"1_clicks,5 6\n" * 3
    cases = [(data, offset, 2 if offset >= len(H) else 1)]
    if data.startswith(H) and data != H:
        cases.append((H + good + data[len(H):], offset + len(good), 5))
    for text, off, line in cases:
        assert O.parse_csv(text) == (off, reason)
        for piece in (None, 1):
            with pytest.raises(ValueError) as e:
                SB.read_submission(text, piece_bytes=piece, ctx=gpu)
            assert (e.value.offset, e.value.reason) == (off, reason), piece
            if what != "blank line":
                assert e.value.line == line
            assert f"byte {off}" in str(e.value)


def test_reader_first_error_wins_and_buffer_ends(gpu):
    import torch
    from otto_recommender_amd import etl
    from otto_recommender_amd import submission as SB
    tile = etl.tile_bytes()
    good = b"1234567_clicks,1855602 99999 10\n"
    body = good * (4 * tile // len(good))
    at = [len(H) + i * len(good) for i in (2, 3 * tile // len(good))]  # line starts in the first and the third tile
    assert at[1] // tile >= 2 + at[0] // tile
    for bad0, bad1, reason in ((b"1234567_clicks,1855602\t99999 10\n", b"1234567_clocks,1855602 99999 10\n", O.BYTE),
                               (b"1234567_clocks,1855602 99999 10\n", b"1234567_clicks,1855602\t99999 10\n", O.TARGET)):
        text = bytearray(H + body)
        text[at[0]:at[0] + len(good)] = bad0
        text[at[1]:at[1] + len(good)] = bad1
        want = O.parse_csv(bytes(text))
        assert want[1] == reason and at[0] < want[0] < at[0] + len(good)
        with pytest.raises(ValueError) as e:
            SB.read_submission(bytes(text), ctx=gpu)
        assert (e.value.offset, e.value.reason) == want
    # a bad byte in the last, short 16-byte chunk; the text fills its tensor to the last byte
    text = H + body + b"7_orders,1\n" + b"12_carts,1 2x"
    assert len(text) % 16 == 12  # the last chunk holds 12 bytes, the bad one last
    dev = torch.device("cuda", gpu.device)
    for data in (text, text[:-1]):
        t = torch.empty(len(data), dtype=torch.uint8, device=dev)
        t.copy_(torch.frombuffer(bytearray(data), dtype=torch.uint8))
        want = O.parse_csv(data)
        if isinstance(want, dict):
            _check_rows(SB.read_submission(t, ctx=gpu), want)
        else:
            assert want == (len(text) - 1, O.BYTE)
            with pytest.raises(ValueError) as e:
                SB.read_submission(t, ctx=gpu)
            assert (e.value.offset, e.value.reason) == want


def _planted(rng, n_sessions=600):
    """ranked rows (ranks 1..n per session and target, up to 30) and labels that some of them hit"""
    frames = F.random_ranked(rng, n_sessions, 30, lo=40_000, hi=60_000)
    lab = []
    for t, name in enumerate(O.TYPES):
        f = frames[name]
        hit = f.iloc[rng.choice(len(f), size=len(f) // 6, replace=False)]
        lab += [(int(s), int(a), t) for s, a in zip(hit["session"], hit["aid_next"])]
        lab += [(int(s), 1_900_000, t) for s in rng.choice(f["session"], size=50)]  # never submitted
    lab += [(7, 1, 0), (8, 2, 2)]  # sessions only in the labels
    labels = pd.DataFrame(lab, columns=["session", "aid", "type"]).drop_duplicates(ignore_index=True)
    return frames, labels


def test_round_trip_and_scores(gpu, tmp_path):
    from otto_recommender_amd import submission as SB
    frames, labels = _planted(np.random.default_rng(17))
    path = str(tmp_path / "out" / "submission.csv")
    n_lines = SB.write_submission(_dev(gpu, F.as_tuples(frames)), path, 20, gpu)
    data = open(path, "rb").read()
    assert data == O.write_csv(F.as_tuples(frames), 20) and n_lines == data.count(b"\n") - 1
    got = SB.read_submission(path, ctx=gpu)
    # the kept rows in file order: lines by session_type, a line's rows by rank
    for t in O.TYPES:
        f = frames[t][frames[t]["pred_rank"] <= 20]
        names = np.array([f"{s}_" for s in f["session"]])  # '_' sorts above the digits: "123_" < "12_"
        order = np.lexsort((f["pred_rank"].to_numpy(), names))
        np.testing.assert_array_equal(got[t]["session"].cpu().numpy(), f["session"].to_numpy()[order])
        np.testing.assert_array_equal(got[t]["aid_next"].cpu().numpy(), f["aid_next"].to_numpy()[order])
    topk = {t: f[f["pred_rank"] <= 20].reset_index(drop=True) for t, f in frames.items()}
    want = SB.eval_ranked(topk, labels, gpu)
    assert 0 < want["clicks"] < 1 and 0 < want["carts"] < 1 and 0 < want["orders"] < 1
    assert SB.eval_submission(path, labels, device=True, ctx=gpu) == want
    assert SB.eval_submission(data, labels, device=True, ctx=gpu) == want
    assert SB.eval_submission(path, labels, ctx=gpu) == want
    with pytest.raises(TypeError):
        SB.eval_submission(pd.DataFrame(), labels, device=True)


def test_submit_from_ranked_files(gpu, tmp_path):
    from otto_recommender_amd import rank as R
    from otto_recommender_amd import submission as SB
    frames = F.random_ranked(np.random.default_rng(4), 400, 25)
    for t, f in frames.items():
        f = f.sort_values(["session", "pred_rank"], kind="stable").reset_index(drop=True)
        f["pred_score"] = -f["pred_rank"].astype(np.float64)
        half = len(f) // 2
        R.write_ranked(f.iloc[:half], str(tmp_path / "ranked" / t / "0001.parquet"))
        R.write_ranked(f.iloc[half:], str(tmp_path / "ranked" / t / "0002.parquet"))
    want = O.write_csv(F.as_tuples(frames), 20)
    path = SB.submit(str(tmp_path / "ranked"), str(tmp_path / "sub"), ctx=gpu)
    assert path == str(tmp_path / "sub" / "submission.csv") and open(path, "rb").read() == want
    path = SB.submit(str(tmp_path / "ranked"), str(tmp_path / "sub"), keep_top_k=5, tag="v2", ctx=gpu)
    assert path.endswith("submission-v2.csv") and open(path, "rb").read() == O.write_csv(F.as_tuples(frames), 5)
    assert SB.submit(str(tmp_path / "ranked"), str(tmp_path / "sub"), name="final", ctx=gpu).endswith("final.csv")
