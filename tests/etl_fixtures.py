"""jsonl text for the ETL tests and tools/etl_timing.py, written from synth Events.

Styles: 'compact' is the data set's own (no spaces), 'spaced' is json.dumps' default separators. Options: member
order shuffled per event, CRLF line ends, no final newline, trailing blank lines. ts in milliseconds is
ts * 1000 + r with r drawn by seed from [0, 999]; 0 and 999 are forced to occur (first and last event)."""
import json

import numpy as np

ID2TYPE = ["clicks", "carts", "orders"]


def ts_ms(ts: np.ndarray, seed: int = 1) -> np.ndarray:
    r = np.random.default_rng(seed).integers(0, 1000, size=len(ts), dtype=np.int64)
    if len(r):
        r[0], r[-1] = 0, 999
    return ts.astype(np.int64) * 1000 + r


def sessions_text(ev, style: str = "compact", shuffle: bool = False, crlf: bool = False, final_newline: bool = True,
                  blank_tail: int = 0, seed: int = 1) -> bytes:
    """One line per session of ev (a synth.Events), in session order"""
    sep = (",", ":") if style == "compact" else (", ", ": ")
    ms = ts_ms(ev.ts, seed)
    rng = np.random.default_rng(seed + 1)
    off = ev.session_offsets - ev.session_offsets[0]
    aid, ty = ev.aid.tolist(), ev.type.tolist()
    ms = ms.tolist()
    lines = []
    for s in range(ev.n_sessions):
        a, b = int(off[s]), int(off[s + 1])
        events = []
        for i in range(a, b):
            items = [("aid", aid[i]), ("ts", ms[i]), ("type", ID2TYPE[ty[i]])]
            if shuffle:
                items = [items[j] for j in rng.permutation(3)]
            events.append(dict(items))
        lines.append(json.dumps({"session": int(ev.session[a]) if b > a else int(ev.first_session + s), "events": events},
                                separators=sep))
    nl = "\r\n" if crlf else "\n"
    text = nl.join(lines) + (nl if final_newline and lines else "")
    return (text + nl * blank_tail).encode()


def sessions_text_fast(ev, seed: int = 1, block: int = 2_000_000):
    """Compact text of ev, yielded in blocks of whole lines; the event objects are built with numpy string
    operations, so 20 M events take seconds, not minutes. Same bytes as sessions_text(ev, 'compact', seed=seed)."""
    ms = ts_ms(ev.ts, seed)
    off = ev.session_offsets - ev.session_offsets[0]
    types = np.array([b"clicks", b"carts", b"orders"])
    s0 = 0
    while s0 < ev.n_sessions:
        s1 = min(int(np.searchsorted(off, off[s0] + block, side="left")), ev.n_sessions)
        s1 = max(s1, s0 + 1)
        a, b = int(off[s0]), int(off[s1])
        add = np.char.add
        obj = add(add(add(add(add(b'{"aid":', ev.aid[a:b].astype("S")), b',"ts":'), ms[a:b].astype("S")),
                      add(b',"type":"', types[ev.type[a:b]])), b'"}').tolist()
        out = []
        for s in range(s0, s1):
            i, j = int(off[s]) - a, int(off[s + 1]) - a
            sid = int(ev.session[a + i]) if j > i else int(ev.first_session + s)
            out.append(b'{"session":%d,"events":[' % sid + b",".join(obj[i:j]) + b"]}\n")
        yield b"".join(out)
        s0 = s1


def labels_text(labels, style: str = "compact") -> bytes:
    """labels: DataFrame[session, aid, type] (synth.split_test_labels) -> one line per session: clicks a scalar,
    carts and orders lists, keys without labels absent"""
    sep = (",", ":") if style == "compact" else (", ", ": ")
    lines = []
    for sid, g in labels.groupby("session", sort=True):
        d = {}
        for t in (0, 1, 2):
            aids = [int(x) for x in g["aid"][g["type"] == t].tolist()]
            if not aids:
                continue
            d[ID2TYPE[t]] = aids[0] if t == 0 else aids
        lines.append(json.dumps({"session": int(sid), "labels": d}, separators=sep))
    return ("\n".join(lines) + ("\n" if lines else "")).encode()
