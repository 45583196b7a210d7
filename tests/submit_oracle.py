"""The submission csv restated in plain Python (imports nothing from the package).

write_csv: model/submit.py:36-60 as rank.submission_frame restates it: keep 1 <= pred_rank <= keep_top_k, order each
(session, target) by pred_rank with equal ranks in input order, one line '{session}_{target},{aid aid ...}' per
group, lines sorted as strings, behind the header.
parse_csv: the strict grammar as a sequential acceptor: rows per target in file order, or (offset, reason) of the
first byte that the grammar does not allow. The reasons are the library's texts.

  file   := "session_type,labels\\n" line*
  line   := number "_" ("clicks" | "carts" | "orders") "," [number (" " number)*] "\\n"     (the last "\\n" may be missing)
  number := "0" | [1-9][0-9]*        (at most 10 digits, value <= 2147483647)
"""
import re

import numpy as np

TYPES = ["clicks", "carts", "orders"]
HEADER = b"session_type,labels\n"

BYTE = "unexpected byte"
HEAD = "the first line is not session_type,labels"
ZERO = "leading zero"
TARGET = "target is not clicks, carts or orders"
CUT = "text ends inside the line"
DIGITS = "number of more than 10 digits"
RANGE = "number does not fit int32"


def write_csv(ranked: dict, keep_top_k: int) -> bytes:
    """ranked: {target: (session, aid_next, pred_rank)} of equal-length integer sequences"""
    lines = []
    for target in TYPES:
        if target not in ranked:
            continue
        ses, aid, rank = (np.asarray(c).astype(np.int64) for c in ranked[target])
        groups = {}
        for i in range(len(ses)):
            if 1 <= rank[i] <= keep_top_k:
                groups.setdefault(int(ses[i]), []).append((int(rank[i]), i, int(aid[i])))
        for s, rows in groups.items():
            rows.sort(key=lambda r: (r[0], r[1]))  # rank, then input order
            lines.append(f"{s}_{target}," + " ".join(str(r[2]) for r in rows))
    lines.sort()
    return HEADER + "".join(l + "\n" for l in lines).encode()


class _Bad(Exception):
    pass


_NUM = rb"(?:0|[1-9][0-9]{0,9})"
_LINE = re.compile(rb"(" + _NUM + rb")_(clicks|carts|orders),((?:" + _NUM + rb"(?: " + _NUM + rb")*)?)")


def parse_csv(data: bytes, fast: bool = True):
    """-> {target: (session list, aid list)} for the targets that a line names, in TYPES order, or (offset, reason).
    fast: the lines that a regular expression of the grammar accepts are taken whole; the byte walk below, which
    defines the result, starts at the first line it does not accept (a large valid file is then read in seconds)."""
    n = len(data)
    rows = {}
    start = 0
    if fast and data.startswith(HEADER):
        start = len(HEADER)
        while start < n:
            end = data.find(b"\n", start)
            m = _LINE.fullmatch(data, start, n if end < 0 else end)
            vals = [int(x) for x in m.group(3).split()] if m else []
            if not m or int(m.group(1)) > 2147483647 or any(v > 2147483647 for v in vals):
                break
            r = rows.setdefault(m.group(2).decode(), ([], []))
            r[0].extend([int(m.group(1))] * len(vals))
            r[1].extend(vals)
            start = n if end < 0 else end + 1

    def bad(p, why):
        raise _Bad((min(p, n), CUT if p >= n else why))

    def lit(p, s, why):
        for ch in s:
            if p >= n or data[p] != ch:
                bad(p, why)
            p += 1
        return p

    def digit(p):
        return p < n and 48 <= data[p] <= 57

    def number(p):
        at = p
        if not digit(p):
            bad(p, BYTE)
        if data[p] == 48:
            if digit(p + 1):
                bad(p + 1, ZERO)
            return p + 1, 0
        x = 0
        while digit(p):
            if p - at == 10:
                bad(p, DIGITS)
            x = x * 10 + data[p] - 48
            p += 1
        if x > 2147483647:
            raise _Bad((at, RANGE))
        return p, x

    try:
        p = start
        if p == 0:
            p = lit(0, HEADER[:-1], HEAD)
            if p < n:
                if data[p] != 10:
                    bad(p, HEAD)
                p += 1
        while p < n:
            p, ses = number(p)
            if p >= n or data[p] != 95:
                bad(p, BYTE)
            p += 1
            if p < n and data[p] == 99:  # 'c'
                name = "clicks" if p + 1 < n and data[p + 1] == 108 else "carts"
            else:
                name = "orders"
            p = lit(p, name.encode(), TARGET)
            if p >= n or data[p] != 44:
                bad(p, BYTE)
            p += 1
            r = rows.setdefault(name, ([], []))
            if p < n and data[p] != 10:
                while True:
                    p, aid = number(p)
                    r[0].append(ses)
                    r[1].append(aid)
                    if p >= n or data[p] == 10:
                        break
                    if data[p] != 32:
                        bad(p, BYTE)
                    p += 1
                    if not digit(p):
                        bad(p, BYTE)
            p += 1  # the line's '\n', or past the end
    except _Bad as e:
        return e.args[0]
    return {t: rows[t] for t in TYPES if t in rows}
