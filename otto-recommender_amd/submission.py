"""The competition metric on ranked output (model/eval_submission.py): recall@20 per type, weighted 0.1 / 0.3 / 0.6.

Mirrors model/eval_submission.py:22-68. Per (session, type), with labels unique per (session, type, aid) as
candidates.labels_csr makes them: every submitted entry that is a label counts one hit (an aid submitted n times
counts n, as the outer join of :44-49 does), true = min(20, sum over labels of max(times submitted, 1)) (the
joined row count of :48, clipped); a session with labels and nothing submitted adds to true, submitted rows without
labels add nothing. recall@20 = sum hit / sum true per type. The sums are computed in libottohip.so
(csrc/downsample.hip, ottohip_submission_recall) from two CSRs over the sorted union of session ids; ranked rows go
in as they come out of the rank stage, device tensors or DataFrames, never through strings.
"""
from __future__ import annotations

import ctypes
import json
import os

import numpy as np

from . import _lib
from . import config

WEIGHTS = {"clicks": 0.1, "carts": 0.3, "orders": 0.6}


def _pair(r):
    """(session, aid_next) of one target's ranked rows: a {column: tensor} dict or a DataFrame"""
    import torch
    get = lambda c: r[c] if isinstance(r[c], torch.Tensor) else torch.from_numpy(np.ascontiguousarray(r[c].to_numpy()
                                                                                   if hasattr(r[c], "to_numpy") else r[c]))
    return get("session"), get("aid_next")


def session_csrs(ranked: dict, df_labels, ctx=None):
    """The scorer's inputs: (S, lab_off, lab_aid, sub_off, sub_aid) on the device, both CSRs in the labels_csr layout
    ([3 * (S + 1)] offsets) over the sorted union of the session ids of df_labels and of the ranked rows (built on
    the host; the submitted rows are grouped on the device)."""
    import torch
    from .candidates import labels_csr
    ctx = ctx or _lib.context()
    dev = torch.device("cuda", ctx.device)
    subs, ids = {}, [df_labels["session"].to_numpy().astype(np.int64)]
    for t, name in enumerate(config.TYPES):
        if name not in ranked:
            continue
        s, a = _pair(ranked[name])
        s, a = s.to(dev, torch.int64), a.to(dev, torch.int32)
        subs[t] = (s, a)
        ids.append(torch.unique(s).cpu().numpy())
    universe = np.unique(np.concatenate(ids))
    S = len(universe)
    if S == 0:
        return 0, None, None, None, None
    lab_off, lab_aid = labels_csr(df_labels, universe)
    uni_d = torch.from_numpy(universe).to(dev)
    offs, aids, base = [], [], 0
    for t in range(3):
        if t in subs and subs[t][0].numel():
            idx = torch.searchsorted(uni_d, subs[t][0])
            order = torch.argsort(idx, stable=True)
            cnt = torch.bincount(idx, minlength=S)
            aids.append(subs[t][1][order])
        else:
            cnt = torch.zeros(S, dtype=torch.int64, device=dev)
        o = torch.zeros(S + 1, dtype=torch.int64, device=dev)
        torch.cumsum(cnt, 0, out=o[1:])
        offs.append(o + base)
        base += int(cnt.sum().item())
    sub_off = torch.cat(offs).contiguous()
    sub_aid = torch.cat(aids).contiguous() if aids else torch.zeros(1, dtype=torch.int32, device=dev)
    lo = torch.from_numpy(lab_off).to(dev)
    la = torch.from_numpy(lab_aid).to(dev) if len(lab_aid) else torch.zeros(1, dtype=torch.int32, device=dev)
    return S, lo, la, sub_off, sub_aid


def recall_sums(ranked: dict, df_labels, ctx=None, stream=None) -> list:
    """[hit, true] per type of config.TYPES, flat (six ints; additive over disjoint session sets). ranked:
    {target: {session, aid_next, ...}} as Ranker.rank (device tensors) or rank_job (DataFrames) return it; a target
    that is absent submits nothing. df_labels [session, aid, type]."""
    ctx = ctx or _lib.context()
    S, lo, la, sub_off, sub_aid = session_csrs(ranked, df_labels, ctx)
    sums = (ctypes.c_int64 * 6)()
    if S:
        _lib.check(_lib.load().ottohip_submission_recall(ctx.h, S, _lib.ptr(lo), _lib.ptr(la), _lib.ptr(sub_off),
                                                         _lib.ptr(sub_aid), sums, _lib.stream_handle(stream)))
    return list(sums)


def recall_from_sums(sums) -> dict:
    """model/eval_submission.py:50-58: {"clicks", "carts", "orders", "total"}. A type whose sum of true is 0 scores
    0.0, as candidates.recall_from_sums does (the reference divides and yields NaN there)."""
    res = {n: (sums[2 * t] / sums[2 * t + 1] if sums[2 * t + 1] else 0.0) for t, n in enumerate(config.TYPES)}
    res["total"] = sum(WEIGHTS[n] * res[n] for n in config.TYPES)
    return res


def eval_ranked(ranked: dict, df_labels, ctx=None, stream=None) -> dict:
    """recall@20 per type and the weighted total of ranked rows (see recall_sums)."""
    return recall_from_sums(recall_sums(ranked, df_labels, ctx, stream))


def parse_submission(df) -> dict:
    """model/eval_submission.py:34-42, host only: DataFrame[session_type, labels] as rank.submission_frame writes it
    -> {target: {session int32, aid_next int32}} with one row per submitted aid, in file order."""
    st = df["session_type"].astype(str).str.split("_", n=1, expand=True)
    out = {}
    if not len(df):
        return out
    ses = st[0].to_numpy().astype(np.int64)
    typ = st[1].to_numpy()
    lists = [[int(x) for x in str(v).split(" ") if x != ""] for v in df["labels"].tolist()]
    n = np.array([len(x) for x in lists], np.int64)
    aid = np.array([a for x in lists for a in x], np.int64)
    row_ses, row_typ = np.repeat(ses, n), np.repeat(typ, n)
    for name in config.TYPES:
        m = row_typ == name
        if m.any() or (typ == name).any():
            out[name] = {"session": row_ses[m].astype(np.int32), "aid_next": aid[m].astype(np.int32)}
    return out


def eval_submission(file_submit_or_frame, df_labels, dir_out: str | None = None, name: str | None = None,
                    ctx=None) -> dict:
    """The __main__ of model/eval_submission.py: a submission csv (or its DataFrame[session_type, labels]) scored
    against df_labels [session, aid, type]. With dir_out also writes {dir_out}/{name}.json (the four figures, keys
    sorted) and {dir_out}/{name}.csv ([type, recall@20], rows clicks, carts, orders, total) (:67-70); name defaults
    to the file's basename, or 'submission'."""
    import pandas as pd
    if isinstance(file_submit_or_frame, (str, os.PathLike)):
        df = pd.read_csv(file_submit_or_frame, dtype=str)
        name = name or os.path.basename(str(file_submit_or_frame))
    else:
        df = file_submit_or_frame
    res = eval_ranked(parse_submission(df), df_labels, ctx)
    if dir_out is not None:
        stem = (name or "submission")
        stem = stem[:-4] if stem.endswith(".csv") else stem
        os.makedirs(dir_out, exist_ok=True)
        with open(os.path.join(dir_out, stem + ".json"), "w") as fh:
            json.dump(res, fh, indent=2, sort_keys=True)
        order = config.TYPES + ["total"]
        pd.DataFrame({"type": order, "recall@20": [res[k] for k in order]}).to_csv(os.path.join(dir_out, stem + ".csv"),
                                                                                     index=False)
    return res
