"""The jsonl ETL on the GPU (csrc/etl.hip, otto_recommender_amd/etl.py) against tests/etl_oracle.py. Everything is
exact: integer columns, rows per line, file names, error codes and line numbers."""
import json
import os
import re
import time

import numpy as np
import pytest

import etl_fixtures as F
import etl_oracle as O

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SESSION_COLS = ("session", "aid", "ts", "type")
LABEL_COLS = ("session", "type", "aid")
EINVAL, ELIMIT = -1, -5


def _kat(name):
    with open(os.path.join(GOLDEN, name), "rb") as fh:
        return fh.read()


def parse(gpu, text, kind="sessions", piece_bytes=None):
    """columns and rows per line as host arrays, through the package's piece reader"""
    from otto_recommender_amd import etl
    cols, rpl = etl.parse_bytes(text, kind, piece_bytes, ctx=gpu)
    names = SESSION_COLS if kind == "sessions" else LABEL_COLS
    out = {k: c.cpu().numpy() for k, c in zip(names, cols)}
    out["rows_per_line"] = rpl
    return out


def parse_resident(gpu, text, kind=0):
    """one piece, uploaded with a plain copy: the bare entry points (many tiny launches in the sweeps)"""
    import torch
    from otto_recommender_amd import etl
    dev = torch.frombuffer(bytearray(text), dtype=torch.uint8).cuda()
    cols, rpl, _ = etl._parse_piece(gpu, kind, dev, len(text), 0)
    return [c.cpu().numpy() for c in cols] + [rpl]


def assert_same(got, want, cols=SESSION_COLS):
    for k in cols + ("rows_per_line",):
        assert got[k].dtype == want[k].dtype, k
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)


@pytest.fixture(scope="module")
def base():
    from otto_recommender_amd import synth
    ev = synth.generate(3000)
    text = F.sessions_text(ev)
    return ev, text, O.sessions_rows(text)


def test_round_trip(gpu, base):
    from otto_recommender_amd import etl
    ev, text, want = base
    tile = etl.tile_bytes()
    assert len(text) // tile > 2048 and ev.n_events > 40_000  # hundreds of tiles, more than one scan block
    got = parse(gpu, text)
    assert_same(got, want)
    for k in SESSION_COLS:  # and the events the text was written from
        np.testing.assert_array_equal(got[k], getattr(ev, k), err_msg=k)
    np.testing.assert_array_equal(got["rows_per_line"], np.diff(ev.session_offsets))
    again = parse(gpu, text)
    for k in SESSION_COLS + ("rows_per_line",):
        assert got[k].tobytes() == again[k].tobytes(), k


@pytest.mark.parametrize("opts", [dict(style="spaced"), dict(shuffle=True), dict(crlf=True), dict(final_newline=False),
                                  dict(blank_tail=3), dict(style="spaced", shuffle=True, crlf=True, final_newline=False)],
                         ids=lambda o: "-".join(o))
def test_styles_give_the_same_rows(gpu, base, opts):
    ev = base[0].slice_sessions(0, 400)
    text = F.sessions_text(ev, **opts)
    got = parse(gpu, text)
    assert_same(got, O.sessions_rows(text))
    for k in SESSION_COLS:
        np.testing.assert_array_equal(got[k], getattr(ev, k), err_msg=k)


def test_token_alignment(gpu, base):
    """k spaces behind the first '{' move every later token over every 16-byte lane boundary and every tile boundary.
    All k in [0, 2 * tile + 17) are run: tiny launches."""
    from otto_recommender_amd import etl
    ev = base[0].slice_sessions(0, 40)
    text = F.sessions_text(ev, shuffle=True)
    want = parse_resident(gpu, text)
    for k, w in zip(SESSION_COLS, want):
        np.testing.assert_array_equal(w, getattr(ev, k), err_msg=k)
    t0 = time.perf_counter()
    n_k = 2 * etl.tile_bytes() + 17
    for k in range(n_k):
        got = parse_resident(gpu, text[:1] + b" " * k + text[1:])
        for g, w in zip(got, want):
            assert np.array_equal(g, w), k
    print(f"token alignment: {n_k} texts in {time.perf_counter() - t0:.2f} s")


def test_pieces(gpu, base):
    ev = base[0]
    lens = np.diff(ev.session_offsets)
    i = int(np.argmax(lens))
    assert lens[i] == 500
    part = ev.slice_sessions(max(i - 150, 0), min(i + 150, ev.n_sessions))
    text = F.sessions_text(part)
    longest = max(len(ln) for ln in text.split(b"\n")) + 1
    assert longest > 4096  # longer than the small pieces: they have to grow
    one = parse(gpu, text)
    assert_same(one, O.sessions_rows(text))
    for pb in (4096, 65536, longest):
        assert_same(parse(gpu, text, piece_bytes=pb), one)


def test_known_answers_and_extremes(gpu):
    exp = json.loads(_kat("etl_kat_expected.json"))
    for kind, file, cols in (("sessions", "etl_kat.jsonl", SESSION_COLS), ("labels", "etl_kat_labels.jsonl", LABEL_COLS)):
        text = _kat(file)
        for pb in (None, 64):
            got = parse(gpu, text, kind, pb)
            for k in cols + ("rows_per_line",):
                np.testing.assert_array_equal(got[k].astype(np.int64), np.array(exp[kind][k], np.int64), err_msg=k)
            assert_same(got, (O.sessions_rows if kind == "sessions" else O.labels_rows)(text), cols)
    one = b'{"session":7,"events":[{"aid":3,"ts":5999,"type":"orders"}]}'
    for text in (one, one + b"\n"):
        got = parse(gpu, text)
        assert [got[k].tolist() for k in SESSION_COLS] == [[7], [3], [5], [2]] and got["rows_per_line"].tolist() == [1]
    for text in (b"", b"\n", b" \r\n\n"):
        for kind in ("sessions", "labels"):
            got = parse(gpu, text, kind)
            assert all(len(v) == 0 for v in got.values())
            assert got["session"].dtype == np.int32 and got["type"].dtype == np.int8


V = b'{"session":1,"events":[{"aid":1,"ts":2000,"type":"clicks"},{"aid":2,"ts":3000,"type":"carts"}]}'
LV = b'{"session":1,"labels":{"clicks":1,"carts":[2,3]}}'


def _ev(body):
    return b'{"session":1,"events":[' + body + b']}'


REJECTIONS = [  # (id, kind, bad line, code)
    ("event-unknown-key", "sessions", _ev(b'{"aid":1,"ts":2,"type":"clicks","x":1}'), EINVAL),
    ("line-unknown-key", "sessions", b'{"session":1,"events":[],"foo":1}', EINVAL),
    ("event-missing-key", "sessions", _ev(b'{"aid":1,"type":"clicks"}'), EINVAL),
    ("line-missing-events", "sessions", b'{"session":1}', EINVAL),
    ("event-duplicate-key", "sessions", _ev(b'{"aid":1,"ts":2,"aid":1,"type":"clicks"}'), EINVAL),
    ("line-duplicate-key", "sessions", b'{"session":1,"session":1,"events":[]}', EINVAL),
    ("sign", "sessions", _ev(b'{"aid":-1,"ts":2,"type":"clicks"}'), EINVAL),
    ("fraction", "sessions", _ev(b'{"aid":1,"ts":2.5,"type":"clicks"}'), EINVAL),
    ("exponent", "sessions", _ev(b'{"aid":1,"ts":2e3,"type":"clicks"}'), EINVAL),
    ("leading-zero", "sessions", _ev(b'{"aid":01,"ts":2,"type":"clicks"}'), EINVAL),
    ("escape", "sessions", _ev(b'{"aid":1,"ts":2,"type":"cl\\u0069cks"}'), EINVAL),
    ("high-byte", "sessions", _ev(b'{"aid":1,"ts":2,"type":"clicks\xc3\xa9"}'), EINVAL),
    ("control-byte", "sessions", _ev(b'{"aid":1,\x01"ts":2,"type":"clicks"}'), EINVAL),
    ("type-name", "sessions", _ev(b'{"aid":1,"ts":2,"type":"views"}'), EINVAL),
    ("trailing-text", "sessions", V + b" x", EINVAL),
    ("two-objects", "sessions", V + V, EINVAL),
    ("list-closed-twice", "sessions", _ev(b'{"aid":1,"ts":2,"type":"clicks"}],{"aid":1,"ts":2,"type":"clicks"}'), EINVAL),
    ("trailing-comma", "sessions", _ev(b'{"aid":1,"ts":2,"type":"clicks"},'), EINVAL),
    ("event-not-closed", "sessions", _ev(b'{"aid":1,"ts":2,"type":"clicks"'), EINVAL),
    ("session-limit", "sessions", b'{"session":2147483648,"events":[]}', ELIMIT),
    ("aid-limit", "sessions", _ev(b'{"aid":2147483648,"ts":2,"type":"clicks"}'), ELIMIT),
    ("ts-limit", "sessions", _ev(b'{"aid":1,"ts":2147483648000,"type":"clicks"}'), ELIMIT),
    ("digits-limit", "sessions", _ev(b'{"aid":1,"ts":1234567890123456789,"type":"clicks"}'), ELIMIT),
    ("labels-duplicate-type", "labels", b'{"session":1,"labels":{"clicks":1,"clicks":2}}', EINVAL),
    ("labels-unknown-type", "labels", b'{"session":1,"labels":{"views":1}}', EINVAL),
    ("labels-nested-list", "labels", b'{"session":1,"labels":{"carts":[[1]]}}', EINVAL),
    ("labels-missing", "labels", b'{"session":1}', EINVAL),
    ("labels-aid-limit", "labels", b'{"session":1,"labels":{"carts":[1,2147483648]}}', ELIMIT),
]


def _rejected(gpu, text, kind, code, line, piece_bytes=None):
    from otto_recommender_amd import _lib
    assert O.first_bad_line(text, kind) == line  # the acceptor names the same line
    with pytest.raises(_lib.OttoHipError) as e:
        parse(gpu, text, kind, piece_bytes)
    assert e.value.rc == code, str(e.value)
    m = re.search(r"line (\d+)", str(e.value))
    assert m and int(m.group(1)) == line, str(e.value)
    ok = V if kind == "sessions" else LV  # the context still parses
    assert parse(gpu, ok + b"\n", kind)["session"].tolist() == ([1, 1] if kind == "sessions" else [1, 1, 1])


@pytest.mark.parametrize("kind, bad, code", [r[1:] for r in REJECTIONS], ids=[r[0] for r in REJECTIONS])
def test_rejections(gpu, kind, bad, code):
    ok = V if kind == "sessions" else LV
    _rejected(gpu, ok + b"\n" + bad + b"\n" + ok + b"\n", kind, code, 2)


def test_rejection_of_a_line_cut_short_at_the_end_of_the_buffer(gpu):
    for cut in (1, 12, 30, len(V) - 2, len(V) - 1):
        _rejected(gpu, V + b"\n\n" + V[:cut], "sessions", EINVAL, 3)  # the blank line counts in the line number


def test_rejection_in_a_second_piece_names_the_line_of_the_file(gpu):
    bad = _ev(b'{"aid":1,"ts":2,"type":"views"}')
    text = (V + b"\n") * 100 + bad + b"\n" + V + b"\n"
    for pb in (1024, 4096, None):
        _rejected(gpu, text, "sessions", EINVAL, 101, pb)


def test_mutations_agree_with_the_acceptor(gpu):
    """300 seeded single-byte substitutions of a 3-line text: the device accepts exactly when the acceptor does, and
    then gives the restatement's rows. Every case counts."""
    from otto_recommender_amd import _lib
    text = (b'{"session":12,"events":[{"aid":59625,"ts":1661724000278,"type":"clicks"},{"ts":1661724058352,"aid":1,"type":"carts"}]}\n'
            b'{"session": 13, "events": [{"aid": 0, "ts": 999, "type": "orders"}]}\r\n'
            b'{"events":[],"session":7}\n')
    assert O.accepts(text)
    rng = np.random.default_rng(11)
    pool = np.frombuffer(b'{}[]",: \t\r\n' + b"0123456789" * 3 + b"acdeiklorstyp-.+\\", np.uint8)
    disagree, n_accept = [], 0
    for _ in range(300):
        pos = int(rng.integers(0, len(text)))
        while True:
            b = int(pool[rng.integers(0, len(pool))]) if rng.random() < 0.7 else int(rng.integers(0, 256))
            if b != text[pos]:
                break
        mut = text[:pos] + bytes([b]) + text[pos + 1:]
        want = O.accepts(mut)
        try:
            got = parse_resident(gpu, mut)
            accepted = True
        except _lib.OttoHipError as e:
            assert e.rc in (EINVAL, ELIMIT)
            accepted = False
        if accepted != want:
            disagree.append((pos, b, want))
        elif accepted:
            n_accept += 1
            ref = O.sessions_rows(mut)
            for g, k in zip(got, SESSION_COLS + ("rows_per_line",)):
                np.testing.assert_array_equal(g, ref[k], err_msg=f"{k} at {pos} <- {b}")
    assert disagree == []
    assert n_accept >= 5  # digit for digit and white space for white space: the accepting side is exercised


def test_files(gpu, tmp_path):
    import pyarrow as pa
    import pyarrow.parquet as pq
    from otto_recommender_amd import covis, etl, synth
    ev = synth.generate(2500, first_session=50_000, seed=4)
    src = tmp_path / "train_sessions.jsonl"
    text = F.sessions_text(ev)
    src.write_bytes(text)
    paths = etl.transform_jsonl_to_parquet(str(src), str(tmp_path / "out"), chunksize=1000, piece_bytes=1 << 20, ctx=gpu)
    assert [os.path.relpath(p, tmp_path) for p in paths] == [f"out/train_sessions/{n}.parquet"
                                                            for n in ("0000_1000", "1000_2000", "2000_3000")]
    want = O.sessions_rows(text)
    bounds = np.concatenate([[0], np.cumsum(O.chunk_rows(want["rows_per_line"], 1000))])
    for f, p in enumerate(paths):
        t = pq.read_table(p)
        assert t.schema.names == list(SESSION_COLS)
        assert [t.schema.field(k).type for k in SESSION_COLS] == [pa.int32(), pa.int32(), pa.int32(), pa.int8()]
        for k in SESSION_COLS:
            np.testing.assert_array_equal(t.column(k).to_numpy(), want[k][bounds[f]:bounds[f + 1]], err_msg=k)
    a = etl.events_from_jsonl(str(src), chunksize=1000, piece_bytes=1 << 20, ctx=gpu)
    b = covis.DeviceEvents.from_parquet(paths, ctx=gpu)
    assert (a.n_sessions, a.n_events) == (b.n_sessions, b.n_events) == (ev.n_sessions, ev.n_events)
    np.testing.assert_array_equal(a.file_bounds, b.file_bounds)
    for k in ("offsets", "aid", "ts", "type"):
        np.testing.assert_array_equal(getattr(a, k).cpu().numpy(), getattr(b, k).cpu().numpy(), err_msg=k)
    ta, tb = covis.count_co_events_fused(a), covis.count_co_events_fused(b)
    assert ta.names == tb.names
    for n in ta.names:
        for x, y in zip(ta.to_numpy(n), tb.to_numpy(n)):
            np.testing.assert_array_equal(x, y, err_msg=n)
    with pytest.raises(ValueError):
        etl.transform_jsonl_to_parquet(str(src), str(tmp_path / "out"), type_data="other")
    empty = tmp_path / "empty.jsonl"
    empty.write_bytes(b"")
    assert etl.transform_jsonl_to_parquet(str(empty), str(tmp_path / "out"), ctx=gpu) == []
    assert os.listdir(tmp_path / "out" / "empty") == []


def test_labels(gpu, tmp_path):
    import pyarrow as pa
    import pyarrow.parquet as pq
    from otto_recommender_amd import etl, synth
    _, _, labels = synth.split_test_labels(synth.generate(8000))
    text = F.labels_text(labels)
    want = O.labels_rows(text)
    assert len(want["rows_per_line"]) > 1500 and len(text) > 64 * etl.tile_bytes()
    assert_same(parse(gpu, text, "labels"), want, LABEL_COLS)
    assert_same(parse(gpu, text, "labels", piece_bytes=8192), want, LABEL_COLS)
    spaced = F.labels_text(labels.iloc[:600], style="spaced")
    assert_same(parse(gpu, spaced, "labels"), O.labels_rows(spaced), LABEL_COLS)
    src = tmp_path / "test_labels.jsonl"
    src.write_bytes(text)
    df = etl.labels_from_jsonl(str(src), ctx=gpu)
    assert list(df.columns) == list(LABEL_COLS) and [str(d) for d in df.dtypes] == ["int32", "int8", "int32"]
    for k in LABEL_COLS:
        np.testing.assert_array_equal(df[k].to_numpy(), want[k], err_msg=k)
    paths = etl.transform_jsonl_to_parquet(str(src), str(tmp_path), "labels", chunksize=1000, ctx=gpu)
    assert [os.path.basename(p) for p in paths] == [n + ".parquet" for n in O.chunk_names(len(want["rows_per_line"]), 1000)]
    got = pa.concat_tables([pq.read_table(p) for p in paths])
    assert got.schema.names == list(LABEL_COLS)
    assert [got.schema.field(k).type for k in LABEL_COLS] == [pa.int32(), pa.int8(), pa.int32()]
    for k in LABEL_COLS:
        np.testing.assert_array_equal(got.column(k).to_numpy(), want[k], err_msg=k)
