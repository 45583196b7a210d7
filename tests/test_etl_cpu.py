"""The jsonl ETL's restatement and acceptor (tests/etl_oracle.py) against the hand-written known answers, and the host
rules that need no GPU: the ts quotient, the chunk names, the piece cutter."""
import io
import json
import os

import numpy as np
import pytest

import etl_fixtures as F
import etl_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _kat(name):
    with open(os.path.join(GOLDEN, name), "rb") as fh:
        return fh.read()


EXPECTED = json.loads(_kat("etl_kat_expected.json"))


@pytest.mark.parametrize("kind, file, cols", [("sessions", "etl_kat.jsonl", ("session", "aid", "ts", "type")),
                                              ("labels", "etl_kat_labels.jsonl", ("session", "type", "aid"))])
def test_restatement_reproduces_the_known_answers(kind, file, cols):
    text, want = _kat(file), EXPECTED[kind]
    got = (O.sessions_rows if kind == "sessions" else O.labels_rows)(text)
    for c in cols:
        np.testing.assert_array_equal(got[c].astype(np.int64), np.array(want[c], np.int64), err_msg=c)
    assert got["type"].dtype == np.int8 and got["aid"].dtype == got["session"].dtype == np.int32
    np.testing.assert_array_equal(got["rows_per_line"], want["rows_per_line"])
    cs = EXPECTED["chunksize"]
    assert O.chunk_names(len(got["rows_per_line"]), cs) == want["names"]
    assert O.chunk_rows(got["rows_per_line"], cs) == want["chunk_rows"]


@pytest.mark.parametrize("kind, file", [("sessions", "etl_kat.jsonl"), ("labels", "etl_kat_labels.jsonl")])
def test_acceptor_agrees_with_json_on_every_known_line(kind, file):
    lines = O.lines_of(_kat(file))
    assert len(lines) == 12 and [i for i, _ in lines] != list(range(1, 13))  # one blank line is skipped
    for _, ln in lines:
        obj = json.loads(ln)
        assert set(obj) == {"session", "events" if kind == "sessions" else "labels"}
        assert O.accepts_line(ln, kind), ln
        assert not O.accepts_line(ln, "labels" if kind == "sessions" else "sessions"), ln


@pytest.mark.parametrize("bad", [
    b'{"session":1,"events":[{"aid":1,"ts":2,"type":"clicks"}],}', b'{"session":01,"events":[]}',
    b'{"session":1,"events":[{"aid":-1,"ts":2,"type":"clicks"}]}', b'{"session":1,"events":[{"aid":1,"ts":2}]}',
    b'{"session":1,"events":[{"aid":1,"ts":2.0,"type":"clicks"}]}', b'{"session":1,"events":[]} x',
    b'{"session":1,"events":[{"aid":1,"ts":2,"type":"clicks","aid":1}]}', b'{"session":1,"events":[],"x":1}',
    b'{"session":2147483648,"events":[]}', b'{"session":1,"events":[{"aid":1,"ts":2147483648000,"type":"clicks"}]}',
    b'{"session":1,"events":[{"aid":1,"ts":1234567890123456789,"type":"clicks"}]}',
])
def test_acceptor_refuses(bad):
    assert not O.accepts_line(bad, "sessions")


def test_labels_acceptor_refuses_a_repeated_type():
    assert O.accepts_line(b'{"session":1,"labels":{"clicks":1,"carts":[2]}}', "labels")
    assert not O.accepts_line(b'{"session":1,"labels":{"clicks":1,"clicks":2}}', "labels")
    assert not O.accepts_line(b'{"session":1,"labels":{"views":1}}', "labels")


def test_ts_integer_quotient_equals_the_float64_form():
    rng = np.random.default_rng(7)
    ms = np.concatenate([rng.integers(0, 2**31 * 1000, size=1_000_000, dtype=np.int64),
                         np.array([0, 999, 1000, 1661724000999, 2147483647999], np.int64)])
    np.testing.assert_array_equal(ms // 1000, (ms / 1000).astype(np.int32).astype(np.int64))


def test_chunk_names_of_250_lines():
    from otto_recommender_amd import etl
    for names in (O.chunk_names, etl.chunk_names):
        assert names(250, 100) == ["000_100", "100_200", "200_300"]
        assert names(0, 100) == []
        assert names(100000, 100000) == ["000000_100000"]
    np.testing.assert_array_equal(etl.chunk_rows(np.arange(7), 3), [3, 12, 6])


def test_pieces_are_whole_lines_and_grow_for_a_long_line():
    from otto_recommender_amd import etl
    text = b"aa\nbbbb\n" + b"c" * 50 + b"\ndd\nlast"
    for pb in (1, 4, 8, 16, 1000):
        pieces = list(etl._pieces(io.BytesIO(text), pb))
        assert b"".join(pieces) == text
        assert all(p.endswith(b"\n") for p in pieces[:-1])
        assert all(len(p) <= pb or b"\n" not in p[:-1] for p in pieces)  # longer only as one single line
    assert list(etl._pieces(io.BytesIO(b""), 16)) == []


def test_unknown_type_data_raises(tmp_path):
    from otto_recommender_amd import etl
    with pytest.raises(ValueError):
        etl.transform_jsonl_to_parquet(str(tmp_path / "x.jsonl"), str(tmp_path), type_data="other")


def test_number_of_lines(tmp_path):
    from otto_recommender_amd import etl
    for text, n in ((b"", 0), (b"a\n", 1), (b"a\nb", 2), (b"a\n\nb\n", 3)):
        p = tmp_path / "f.jsonl"
        p.write_bytes(text)
        assert etl.get_number_of_lines(str(p)) == n


def test_fixture_writers_agree():
    from otto_recommender_amd import synth
    ev = synth.generate(300, first_session=1000, seed=3)
    text = F.sessions_text(ev)
    assert b"".join(F.sessions_text_fast(ev, block=1000)) == text
    assert O.accepts(text) and O.accepts(F.sessions_text(ev, "spaced", shuffle=True, crlf=True, final_newline=False))
    rows = O.sessions_rows(text)
    np.testing.assert_array_equal(rows["aid"], ev.aid)
    np.testing.assert_array_equal(rows["ts"], ev.ts)
    np.testing.assert_array_equal(rows["type"], ev.type)
    np.testing.assert_array_equal(rows["session"], ev.session)
    ms = F.ts_ms(ev.ts)
    assert ms[0] % 1000 == 0 and ms[-1] % 1000 == 999
