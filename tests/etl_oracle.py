"""Restatement of the jsonl ETL (etl/jsonl_to_parquet.py:23-56) for the parity tests: json.loads per line plus the
column rules, and the strict acceptor the device parser is held to. Written from the rules in DESIGN.md (ETL); it
shares no code with the package's parser.

Column rules: session, aid -> int32; type -> clicks 0, carts 1, orders 2 (int8); ts -> ms // 1000 (int32), which for
ts >= 0 equals the reference's (ts / 1000).astype(int32) in float64. Rows in line order, then event order (labels: key
order as written, then list order; a scalar is one row). Lines of white space only are skipped and not counted.

The acceptor is one full-match regular expression per line kind, built from the grammar token by token, followed by
the value limits (session, aid and ts // 1000 at most 2^31 - 1), which a regular expression cannot state."""
import itertools
import json
import re

import numpy as np

TYPE2ID = {"clicks": 0, "carts": 1, "orders": 2}
INT32_MAX = 2**31 - 1

_WS = rb"[ \t\r]*"
_INT = rb"(?:0|[1-9][0-9]{0,17})"
_TYPE = rb'"(?:clicks|carts|orders)"'


def _seq(*tokens):
    """tokens with optional white space between any two"""
    return _WS.join(tokens)


def _any_order(members):
    return rb"(?:" + rb"|".join(_seq(*[x for m in p for x in (m, rb",")][:-1]) for p in itertools.permutations(members)) + rb")"


_EVENT = _seq(rb"\{", _any_order([_seq(rb'"aid"', rb":", _INT), _seq(rb'"ts"', rb":", _INT), _seq(rb'"type"', rb":", _TYPE)]),
              rb"\}")
_EVENTS = _seq(rb'"events"', rb":", rb"\[") + rb"(?:" + _WS + _EVENT + rb"(?:" + _WS + rb"," + _WS + _EVENT + rb")*)?" + _WS + rb"\]"
_SESSION = _seq(rb'"session"', rb":", _INT)
_INTS = rb"\[(?:" + _WS + _INT + rb"(?:" + _WS + rb"," + _WS + _INT + rb")*)?" + _WS + rb"\]"
_LABEL = _seq(_TYPE, rb":", rb"(?:" + _INT + rb"|" + _INTS + rb")")
_LABELS = _seq(rb'"labels"', rb":", rb"\{") + rb"(?:" + _WS + _LABEL + rb"(?:" + _WS + rb"," + _WS + _LABEL + rb")*)?" + _WS + rb"\}"
_NO_DUP = rb"".join(rb'(?!.*"' + t + rb'".*"' + t + rb'")' for t in (b"clicks", b"carts", b"orders"))

SESSIONS_LINE = re.compile(_WS + _seq(rb"\{", _any_order([_SESSION, _EVENTS]), rb"\}") + _WS, re.S)
LABELS_LINE = re.compile(_NO_DUP + _WS + _seq(rb"\{", _any_order([_SESSION, _LABELS]), rb"\}") + _WS, re.S)
_BLANK = re.compile(_WS)


def lines_of(text: bytes) -> list:
    """(1-based line number, line) of every line that is not white space only"""
    parts = text.split(b"\n")
    if parts and parts[-1] == b"":
        parts.pop()
    return [(i + 1, ln) for i, ln in enumerate(parts) if not _BLANK.fullmatch(ln)]


def _in_limits(obj, kind) -> bool:
    if obj["session"] > INT32_MAX:
        return False
    if kind == "sessions":
        return all(e["aid"] <= INT32_MAX and e["ts"] // 1000 <= INT32_MAX for e in obj["events"])
    return all(a <= INT32_MAX for v in obj["labels"].values() for a in (v if isinstance(v, list) else [v]))


def accepts_line(line: bytes, kind: str = "sessions") -> bool:
    rx = SESSIONS_LINE if kind == "sessions" else LABELS_LINE
    return bool(rx.fullmatch(line)) and _in_limits(json.loads(line), kind)


def accepts(text: bytes, kind: str = "sessions") -> bool:
    return all(accepts_line(ln, kind) for _, ln in lines_of(text))


def first_bad_line(text: bytes, kind: str = "sessions"):
    """1-based number of the first line the acceptor refuses, or None"""
    return next((i for i, ln in lines_of(text) if not accepts_line(ln, kind)), None)


def sessions_rows(text: bytes) -> dict:
    """session, aid, ts, type columns and the rows of every counted line"""
    s, a, t, y, rpl = [], [], [], [], []
    for _, ln in lines_of(text):
        obj = json.loads(ln)
        rpl.append(len(obj["events"]))
        for e in obj["events"]:
            s.append(obj["session"]); a.append(e["aid"]); t.append(e["ts"] // 1000); y.append(TYPE2ID[e["type"]])
    return {"session": np.array(s, np.int64).astype(np.int32), "aid": np.array(a, np.int64).astype(np.int32),
            "ts": np.array(t, np.int64).astype(np.int32), "type": np.array(y, np.int64).astype(np.int8),
            "rows_per_line": np.array(rpl, np.int64)}


def labels_rows(text: bytes) -> dict:
    s, y, a, rpl = [], [], [], []
    for _, ln in lines_of(text):
        obj = json.loads(ln)
        n0 = len(a)
        for k, v in obj["labels"].items():
            for x in (v if isinstance(v, list) else [v]):
                s.append(obj["session"]); y.append(TYPE2ID[k]); a.append(x)
        rpl.append(len(a) - n0)
    return {"session": np.array(s, np.int64).astype(np.int32), "type": np.array(y, np.int64).astype(np.int8),
            "aid": np.array(a, np.int64).astype(np.int32), "rows_per_line": np.array(rpl, np.int64)}


def chunk_names(n_lines: int, chunksize: int) -> list:
    """'{start}_{end}' per chunk, zero-padded to len(str(n_lines)); end = start + chunksize for the last chunk too"""
    nd = len(str(n_lines))
    return [f"{str(i).zfill(nd)}_{str(i + chunksize).zfill(nd)}" for i in range(0, n_lines, chunksize)]


def chunk_rows(rows_per_line, chunksize: int) -> list:
    r = np.asarray(rows_per_line, np.int64)
    return [int(r[i:i + chunksize].sum()) for i in range(0, len(r), chunksize)]


def pandas_sessions(path_or_buf, chunksize: int = 100000) -> dict:
    """The reference's algorithm: pandas.read_json(lines=True, chunksize) and a Python loop over the events, then the
    dtype conversions with ts in float64 (the host figure of tools/etl_timing.py)."""
    import pandas as pd
    cols = {"session": [], "aid": [], "ts": [], "type": []}
    for chunk in pd.read_json(path_or_buf, lines=True, chunksize=chunksize):
        for session, events in zip(chunk["session"].tolist(), chunk["events"].tolist()):
            for e in events:
                cols["session"].append(session); cols["aid"].append(e["aid"]); cols["ts"].append(e["ts"])
                cols["type"].append(e["type"])
    df = pd.DataFrame(cols)
    return {"session": df["session"].to_numpy().astype(np.int32), "aid": df["aid"].to_numpy().astype(np.int32),
            "ts": (df["ts"] / 1000).to_numpy().astype(np.int32),
            "type": df["type"].map(TYPE2ID).to_numpy().astype(np.int8)}
