"""CPU oracle (TEST INFRASTRUCTURE ONLY) for negative downsampling (model/downsample_retrieved.py:34-62) and the
submission metric (model/eval_submission.py:22-68), restated on numpy / pandas.

polars is not available here, so the reference's shuffle(seed=42) stream cannot be drawn: parity with it is
unpinned. The draw below is the one the product is held to, exactly.

Draw         mix(z): z += 0x9E3779B97F4A7C15; z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27;
                     z *= 0x94D049BB133111EB; z ^= z >> 31                                  (uint64, wrapping)
             h(row) = mix(mix(seed) ^ (uint64(uint32(session)) << 32 | uint64(uint32(aid_next))))
             random(row) = negatives of the same session and target with (h, aid_next) smaller
Downsample   per target over a frame sorted by session, target values 0 or 1: n_pos = sum of the target over the
             session; sessions with n_pos == 0 are dropped; max_n_neg = min(n_pos * ratio, cap) in float64; positives
             are kept; a negative is kept iff random < max_n_neg. Output order within a session: positives in frame
             order, then the kept negatives in frame order. Columns: all but the other two target columns.
Submission   per (session, type): labels unique per (session, type, aid); hit = submitted entries that are labels
             (an aid submitted n times counts n); true = min(20, sum over labels of max(times submitted, 1));
             sessions with labels and nothing submitted add to true, submitted rows without labels add nothing.
             recall@20 = sum hit / sum true (0.0 when sum true is 0: the reference yields NaN); total = 0.1 clicks +
             0.3 carts + 0.6 orders.
"""
from __future__ import annotations

import json
import os

import numpy as np
import pandas as pd

TARGETS = ["clicks", "carts", "orders"]
WEIGHTS = {"clicks": 0.1, "carts": 0.3, "orders": 0.6}
KAT_JSON = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kat_downsample.json")


def mix(z) -> np.ndarray:
    z = np.asarray(z, np.uint64).copy()
    with np.errstate(over="ignore"):
        z += np.uint64(0x9E3779B97F4A7C15)
        z ^= z >> np.uint64(30)
        z *= np.uint64(0xBF58476D1CE4E5B9)
        z ^= z >> np.uint64(27)
        z *= np.uint64(0x94D049BB133111EB)
        z ^= z >> np.uint64(31)
    return z


def draw(seed: int, session, aid_next) -> np.ndarray:
    """h of every row (uint64)"""
    s = np.asarray(session).astype(np.int64).astype(np.uint64) & np.uint64(0xFFFFFFFF)
    a = np.asarray(aid_next).astype(np.int64).astype(np.uint64) & np.uint64(0xFFFFFFFF)
    return mix(mix(np.uint64(int(seed) & 0xFFFFFFFFFFFFFFFF)) ^ ((s << np.uint64(32)) | a))


def session_offsets(session) -> np.ndarray:
    """row offsets of the runs of equal session ids"""
    session = np.asarray(session)
    if not len(session):
        return np.zeros(1, np.int64)
    return np.r_[np.flatnonzero(np.r_[True, session[1:] != session[:-1]]), len(session)].astype(np.int64)


def plan(off, session, aid_next, target, ratio: float = 40.0, cap: float = 100.0, seed: int = 42):
    """(out_off [S + 1], rows): the kept source rows of one target in output order; off [S + 1] relative to off[0]"""
    off = np.asarray(off, np.int64) - int(np.asarray(off)[0])
    target = np.asarray(target)
    aid_next = np.asarray(aid_next)
    h = draw(seed, session, aid_next)
    rows, counts = [], []
    for a, b in zip(off[:-1], off[1:]):
        t = target[a:b]
        n_pos = int(t.astype(np.int64).sum())
        if n_pos == 0:
            counts.append(0)
            continue
        max_n_neg = min(np.float64(n_pos) * np.float64(ratio), np.float64(cap))
        pos = np.flatnonzero(t != 0)
        neg = np.flatnonzero(t == 0)
        order = np.lexsort((aid_next[a:b][neg], h[a:b][neg]))
        random = np.empty(len(neg), np.int64)
        random[order] = np.arange(len(neg))
        kept = neg[random.astype(np.float64) < max_n_neg]
        rows += [a + pos, a + kept]
        counts.append(len(pos) + len(kept))
    out_off = np.r_[0, np.cumsum(counts)].astype(np.int64)
    return out_off, (np.concatenate(rows) if rows else np.zeros(0)).astype(np.int64)


def downsample(frame: pd.DataFrame, target: str, ratio: float = 40.0, cap: float = 100.0, seed: int = 42) -> pd.DataFrame:
    """the downsampled frame of one target from a frame sorted by session"""
    off = session_offsets(frame["session"].to_numpy())
    _, rows = plan(off, frame["session"].to_numpy(), frame["aid_next"].to_numpy(), frame[f"target_{target}"].to_numpy(),
                   ratio, cap, seed)
    cols = [c for c in frame.columns if c not in [f"target_{t}" for t in TARGETS if t != target]]
    return frame[cols].iloc[rows].reset_index(drop=True)


def recall_sums(submitted: dict, labels: pd.DataFrame) -> list:
    """[hit, true] per type, flat: submitted {type name: (session array, aid array)}, labels [session, aid, type]"""
    out = []
    lab = labels.drop_duplicates(["session", "type", "aid"])
    for t, name in enumerate(TARGETS):
        times = {}
        if name in submitted:
            for s, a in zip(np.asarray(submitted[name][0]).tolist(), np.asarray(submitted[name][1]).tolist()):
                times[(s, a)] = times.get((s, a), 0) + 1
        hit_sum = true_sum = 0
        lt = lab[lab["type"] == t]
        for s, g in lt.groupby("session"):
            n = [times.get((s, a), 0) for a in g["aid"].tolist()]
            hit_sum += sum(n)
            true_sum += min(20, sum(max(x, 1) for x in n))
        out += [hit_sum, true_sum]
    return out


def recall_from_sums(sums) -> dict:
    res = {name: (sums[2 * t] / sums[2 * t + 1] if sums[2 * t + 1] else 0.0) for t, name in enumerate(TARGETS)}
    res["total"] = sum(WEIGHTS[n] * res[n] for n in TARGETS)
    return res


# ---------------------------------------------------------------- the known answer
KAT_TRIPLES = [(42, 0, 0), (42, 1, 2), (43, 1, 2), (42, -1, 5), (42, 5, -1), (42, 2147483647, 2147483647),
               (42, -2147483648, 2147483647), (0, 12899779, 1855602), (2 ** 64 - 1, 7, 7)]


def kat_frame() -> pd.DataFrame:
    """three sessions: 2 positives of 12 (cap 3 keeps 3 of 10 negatives), no positive (dropped), all kept"""
    n = [12, 5, 4]
    ses = np.repeat(np.array([11, 12, 2147483647], np.int32), n)
    aid = np.array([5, 9, 1, 7, 3, 8, 2, 6, 4, 10, 12, 11, 1, 2, 3, 4, 5, 9, 8, 7, -6], np.int32)
    tc = np.zeros(len(ses), np.int8)
    tc[[3, 9]] = 1
    tc[[18]] = 1
    return pd.DataFrame({"session": ses, "aid_next": aid, "feat": (np.arange(len(ses)) * 3).astype(np.int16),
                         "target_clicks": tc, "target_carts": np.zeros(len(ses), np.int8),
                         "target_orders": np.zeros(len(ses), np.int8)})


def make_kat() -> dict:
    f = kat_frame()
    kept = downsample(f, "clicks", ratio=40.0, cap=3.0, seed=42)
    return {"hash": [{"seed": str(s), "session": a, "aid_next": b, "h": str(int(draw(s, [a], [b])[0]))}
                     for s, a, b in KAT_TRIPLES],
            "frame": {"ratio": 40.0, "cap": 3.0, "seed": 42, "target": "clicks",
                      "kept": {c: kept[c].tolist() for c in kept.columns}}}


if __name__ == "__main__":
    with open(KAT_JSON, "w") as fh:
        json.dump(make_kat(), fh, indent=1)
        fh.write("\n")
