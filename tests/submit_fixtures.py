"""Inputs shared by the submission csv tests: ranked rows, the edge case, the grammar violations."""
import numpy as np
import pandas as pd

import submit_oracle as O

SESSIONS = [0, 9, 10, 12, 123, 1234, 99, 100, 999999999, 1000000000, 2147483647]
AIDS = [0, 9, 10, 99999, 1855602, 2147483647]


def random_ranked(rng, n_sessions, max_rank, lo=0, hi=3000):
    """{target: DataFrame[session, aid_next, pred_rank]}: ranks 1..n of each session, rows shuffled"""
    out = {}
    for target in O.TYPES:
        ses = rng.choice(np.arange(lo, hi), size=n_sessions, replace=False)
        cnt = rng.integers(1, max_rank + 1, n_sessions)
        s = np.repeat(ses, cnt).astype(np.int32)
        r = np.concatenate([np.arange(1, c + 1) for c in cnt]).astype(np.int16)
        a = rng.integers(0, 1855603, len(s)).astype(np.int32)
        p = rng.permutation(len(s))
        out[target] = pd.DataFrame({"session": s[p], "aid_next": a[p], "pred_rank": r[p]})
    return out


def as_tuples(frames):
    return {t: (np.asarray(f["session"]), np.asarray(f["aid_next"]), np.asarray(f["pred_rank"])) for t, f in frames.items()}


def edge_case():
    """{target: (session, aid_next, pred_rank)}: every digit count of the sessions and aids, lines of 1, 2, 20 and 64
    aids, ranks above every keep_top_k, a (session, target, rank) given twice, a session under one target only, a
    session whose rows stand at the two ends of the input; carts is empty and orders is absent in one variant"""
    rng = np.random.default_rng(3)
    rows = {"clicks": [], "orders": []}
    for i, s in enumerate(SESSIONS):
        n = [1, 2, 20, 64][i % 4]
        for t in ("clicks", "orders"):
            if t == "orders" and s == 123:
                continue  # 123 under clicks only
            aids = [AIDS[(i + j) % len(AIDS)] for j in range(n)]
            rows[t] += [(s, a, j + 1) for j, a in enumerate(aids)]
            rows[t] += [(s, 777, 65), (s, 778, 100), (s, 779, 32767)]  # above every keep_top_k
    rows["orders"] += [(4321, 5, 1)]  # under orders only
    rows["clicks"] += [(77, 30, 2), (77, 10, 1), (77, 20, 2), (77, 40, 2), (77, 50, 3)]  # rank 2 three times
    out = {}
    for t, r in rows.items():
        r = [r[i] for i in rng.permutation(len(r))]
        split = [(55555, 100 + j, j + 1) for j in range(10)]
        r = split[5:] + r + split[:5]  # one session at both ends of the input
        out[t] = tuple(np.array([x[c] for x in r], dt) for c, dt in enumerate((np.int32, np.int32, np.int16)))
    return out


H = O.HEADER
VIOLATIONS = [
    ("quote", H + b'12_carts,"1 2"\n', len(H) + 9, O.BYTE),
    ("quoted head", H + b'"12_carts",1\n', len(H), O.BYTE),
    ("carriage return", H + b"12_carts,1 2\r\n", len(H) + 12, O.BYTE),
    ("tab", H + b"12_carts,1\t2\n", len(H) + 10, O.BYTE),
    ("doubled space", H + b"12_carts,1  2\n", len(H) + 11, O.BYTE),
    ("trailing space", H + b"12_carts,1 2 \n", len(H) + 13, O.BYTE),
    ("trailing space at the end", H + b"12_carts,1 2 ", len(H) + 13, O.CUT),
    ("leading space", H + b"12_carts, 1\n", len(H) + 9, O.BYTE),
    ("sign", H + b"12_carts,-1\n", len(H) + 9, O.BYTE),
    ("plus", H + b"+12_carts,1\n", len(H), O.BYTE),
    ("leading zero", H + b"12_carts,1 02\n", len(H) + 12, O.ZERO),
    ("leading zero in the session", H + b"012_carts,1\n", len(H) + 1, O.ZERO),
    ("unknown target", H + b"12_views,1\n", len(H) + 3, O.TARGET),
    ("cut target", H + b"12_cart,1\n", len(H) + 7, O.TARGET),
    ("upper case", H + b"12_Carts,1\n", len(H) + 3, O.TARGET),
    ("missing comma", H + b"12_carts 1\n", len(H) + 8, O.BYTE),
    ("missing comma at the end", H + b"12_carts", len(H) + 8, O.CUT),
    ("missing underscore", H + b"12carts,1\n", len(H) + 2, O.BYTE),
    ("blank line", H + b"12_carts,1\n\n13_carts,1\n", len(H) + 11, O.BYTE),
    ("wrong header", b"session_type,label\n12_carts,1\n", 18, O.HEAD),
    ("missing header", b"12_carts,1\n", 0, O.HEAD),
    ("header with a tail", b"session_type,labels,x\n", 19, O.HEAD),
    ("empty file", b"", 0, O.CUT),
    ("aid above int32", H + b"12_carts,1 2147483648\n", len(H) + 11, O.RANGE),
    ("session above int32", H + b"4000000000_carts,1\n", len(H), O.RANGE),
    ("eleven digits", H + b"12_carts,12345678901\n", len(H) + 19, O.DIGITS),
    ("letters in a number", H + b"12_carts,1a\n", len(H) + 10, O.BYTE),
    ("float", H + b"12_carts,1.0\n", len(H) + 10, O.BYTE),
]
