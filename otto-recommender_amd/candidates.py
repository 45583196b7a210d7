"""Config-5 candidate generation and recall on MI355X.

Mirrors the candidate part of model/retrieve.py (retrieve_and_gen_feats :422-657 without the
ranker features: get_session_aid_pairs_unique :138-232, get_all_aid_pairs :244-290, the trim
rule :490-516, the source flags :549-559, the cl50 popularity candidates :571-585 and the final
(session, ts_order_aid) order :647) and the recall of model/eval_retrieved.py:45-118.
Everything runs in libottohip.so (csrc/candidates.hip); pandas/pyarrow only at the boundary.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

from . import _lib
from . import config

SRC_NAMES = ["src_self", "src_click_to_click", "src_click_to_cart_or_buy", "src_cart_to_cart", "src_cart_to_buy",
             "src_buy_to_buy", "src_w2vec_all", "src_w2vec_1_2", "src_pop_cl50"]
SRC_BIT = {n: 1 << i for i, n in enumerate(SRC_NAMES)}


class CandLists(ctypes.Structure):
    _fields_ = [("off", ctypes.c_void_p * 7), ("nxt", ctypes.c_void_p * 7), ("rank", ctypes.c_void_p * 7),
                ("n_items", ctypes.c_int32), ("pop_off", ctypes.c_void_p), ("pop_aid", ctypes.c_void_p),
                ("n_clusters", ctypes.c_int32), ("max_list_total", ctypes.c_int32)]


def _dev(ctx):
    import torch
    return torch.device("cuda", ctx.device)


def build_lists(key, nxt, rank, n_keys: int, ctx=None, stream=None):
    """Rows (key, nxt[, rank]) -> CSR by key (stable): torch (off u32 as int32 [n_keys+1], nxt, rank)."""
    import torch
    ctx = ctx or _lib.context()
    dev = _dev(ctx)
    k = torch.as_tensor(key).to(dev, torch.int32).contiguous()
    x = torch.as_tensor(nxt).to(dev, torch.int32).contiguous()
    r = None if rank is None else torch.as_tensor(rank).to(dev, torch.int16).contiguous()
    n = int(k.numel())
    off = torch.empty(n_keys + 1, dtype=torch.int32, device=dev)
    on = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    orr = torch.empty(max(n, 1), dtype=torch.int16, device=dev) if r is not None else None
    _lib.check(_lib.load().ottohip_lists_build(ctx.h, _lib.ptr(k) if n else None, _lib.ptr(x) if n else None,
                                               _lib.ptr(r) if (r is not None and n) else None, n, int(n_keys),
                                               _lib.ptr(off), _lib.ptr(on) if n else None,
                                               _lib.ptr(orr) if (orr is not None and n) else None,
                                               _lib.stream_handle(stream)))
    # empty lists keep a 1-element buffer: a zero-element tensor reports data_ptr() == 0
    return off, (on[:n] if n else on), ((orr[:n] if n else orr) if orr is not None else None)


class CandidateSources:
    """Device CSR lists per aid for the 7 pair sources + the cl50 popularity lists.
    r1: {rule name: (aid, aid_next, rank)} (R1 outputs); knn_all / knn_12: (aid, aid_next, rank);
    pop: (cluster index, aid) rows of the clusters' top aids (min cl50 rank <= 20)."""

    def __init__(self, r1: dict, knn_all, knn_12, pop=None, n_clusters: int = 0, n_items: int = config.N_ITEMS_OTTO,
                 ctx=None):
        import torch
        self.ctx = ctx or _lib.context()
        self.n_items = int(n_items)
        self.keep = []
        srcs = [r1.get(n) for n in config.CO_EVENTS_TO_COUNT] + [knn_all, knn_12]
        self.abi = CandLists()
        total = 0
        for q, src in enumerate(srcs):
            if src is None:
                self.abi.off[q] = self.abi.nxt[q] = self.abi.rank[q] = None
                continue
            a, b, r = src
            off, nx, rk = build_lists(a, b, r, self.n_items, self.ctx)
            self.keep += [off, nx, rk]
            self.abi.off[q], self.abi.nxt[q], self.abi.rank[q] = _lib.ptr(off), _lib.ptr(nx), _lib.ptr(rk)
            if int(off[-1].item()) > 0:
                total += int((off[1:] - off[:-1]).max().item())
        self.abi.n_items = self.n_items
        self.abi.max_list_total = total
        self.n_clusters = int(n_clusters)
        if pop is not None and self.n_clusters > 0:
            c, a = pop
            off, nx, _ = build_lists(c, a, None, self.n_clusters, self.ctx)
            self.keep += [off, nx]
            self.abi.pop_off, self.abi.pop_aid, self.abi.n_clusters = _lib.ptr(off), _lib.ptr(nx), self.n_clusters
        else:
            self.abi.pop_off = self.abi.pop_aid = None
            self.abi.n_clusters = 0


CL50_RANKS = ["rank_clicks_cl50", "rank_carts_cl50", "rank_orders_cl50", "rank_clicks_7d_cl50",
              "rank_carts_7d_cl50", "rank_orders_7d_cl50"]
CL1_RANKS = ["rank_clicks_cl1", "rank_carts_cl1", "rank_orders_cl1"]
_FEAT_NP = {0: np.int8, 1: np.int16, 2: np.int32, 3: np.float32}


def feature_columns(with_targets: bool = True) -> list:
    """ottohip_feature_columns (no GPU call): [(name, numpy dtype)] of the feature frame in file order."""
    lib = _lib.load()
    n = lib.ottohip_feature_columns(-1, None, None)
    out = []
    for i in range(n):
        nm, dt = ctypes.c_char_p(), ctypes.c_int()
        lib.ottohip_feature_columns(i, ctypes.byref(nm), ctypes.byref(dt))
        out.append((nm.value.decode(), np.dtype(_FEAT_NP[dt.value])))
    return out if with_targets else [c for c in out if not c[0].startswith("target_")]


class FeatValues(ctypes.Structure):
    _fields_ = [("count", ctypes.c_void_p * 5), ("count_pop", ctypes.c_void_p * 5), ("perc_pop", ctypes.c_void_p * 5),
                ("count_rel", ctypes.c_void_p * 5), ("dist", ctypes.c_void_p * 2), ("pop_ranks6", ctypes.c_void_p),
                ("cl1_ranks3", ctypes.c_void_p)]


def list_order(key, n_keys: int, ctx=None):
    """The row permutation build_lists applies (stable by key): row i of the CSR is input row perm[i]."""
    import torch
    n = len(key)
    _, perm, _ = build_lists(key, torch.arange(n, dtype=torch.int32), None, n_keys, ctx)
    return perm[:n].long()


class FeatureValues:
    """Value columns aligned entry for entry with the lists of a CandidateSources (ottohip_feat_values), rows given
    in the same order as the rows the sources were built from.
    r1: {rule: (aid, count, count_pop, perc_pop, count_rel)}; knn_all / knn_12: (aid, dist);
    pop: (cluster index, ranks6 [n, 6]) for the rows of the sources' pop lists; cl1: (aid, ranks3 [n, 3]) or None."""

    def __init__(self, sources: CandidateSources, r1: dict, knn_all, knn_12, pop=None, cl1=None):
        import torch
        self.ctx = sources.ctx
        dev = _dev(self.ctx)
        self.keep = []
        self.abi = FeatValues()

        def put(vals, perm, dt):
            v = (vals if isinstance(vals, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(vals))).to(dev, dt)
            v = v[perm].contiguous() if v.numel() else torch.zeros(1, dtype=dt, device=dev)
            self.keep.append(v)
            return _lib.ptr(v)

        for q, n in enumerate(config.CO_EVENTS_TO_COUNT):
            src = r1.get(n)
            if src is None:
                continue
            a, c, cp, pp, cr = src
            perm = list_order(a, sources.n_items, self.ctx)
            self.abi.count[q] = put(c, perm, torch.int32)
            self.abi.count_pop[q] = put(cp, perm, torch.int16)
            self.abi.perc_pop[q] = put(pp, perm, torch.int16)
            self.abi.count_rel[q] = put(cr, perm, torch.int8)
        for w, src in enumerate((knn_all, knn_12)):
            if src is None:
                continue
            a, d = src
            self.abi.dist[w] = put(d, list_order(a, sources.n_items, self.ctx), torch.int32)
        if pop is not None and sources.n_clusters > 0:
            c, r6 = pop
            self.abi.pop_ranks6 = put(np.asarray(r6).reshape(-1, 6), list_order(c, sources.n_clusters, self.ctx),
                                      torch.int16)
        if cl1 is not None:
            a, r3 = cl1
            dense = np.full((sources.n_items, 3), -1, np.int16)
            dense[np.asarray(a, np.int64)] = np.asarray(r3, np.int16).reshape(-1, 3)
            t = torch.from_numpy(dense).to(dev)
            self.keep.append(t)
            self.abi.cl1_ranks3 = _lib.ptr(t)


class Candidates:
    """Device CSR of candidates per session: off [S+1], aid_next, ts_order_aid, flags."""

    def __init__(self, h, ctx):
        self.h, self.ctx = h, ctx
        ns, nc = ctypes.c_int64(), ctypes.c_int64()
        _lib.check(_lib.load().ottohip_candidates_info(h, ctypes.byref(ns), ctypes.byref(nc)))
        self.n_sessions, self.n_cand = int(ns.value), int(nc.value)

    def free(self):
        if self.h:
            _lib.load().ottohip_candidates_free(self.h)
            self.h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

    def to_torch(self, stream=None) -> dict:
        import torch
        dev = _dev(self.ctx)
        off = torch.empty(self.n_sessions + 1, dtype=torch.int64, device=dev)
        nc = max(self.n_cand, 1)
        nxt = torch.empty(nc, dtype=torch.int32, device=dev)
        ordr = torch.empty(nc, dtype=torch.int16, device=dev)
        flags = torch.empty(nc, dtype=torch.int16, device=dev)
        _lib.check(_lib.load().ottohip_candidates_copy(self.h, _lib.ptr(off), _lib.ptr(nxt), _lib.ptr(ordr),
                                                       _lib.ptr(flags), _lib.stream_handle(stream)))
        k = self.n_cand
        return {"off": off, "aid_next": nxt[:k], "ts_order_aid": ordr[:k], "flags": flags[:k]}

    def view(self) -> dict:
        """The device arrays' addresses (ottohip_candidates_view, no copy; valid while this object lives):
        {"off", "aid_next", "ts_order_aid", "flags"} -> int."""
        p = [ctypes.c_void_p() for _ in range(4)]
        _lib.check(_lib.load().ottohip_candidates_view(self.h, *(ctypes.byref(x) for x in p)))
        return {k: int(x.value or 0) for k, x in zip(("off", "aid_next", "ts_order_aid", "flags"), p)}

    def features(self, events, sources: CandidateSources, values: FeatureValues, session_cl=None, labels=None,
                 lo: int = 0, hi: int | None = None, stream=None) -> dict:
        """ottohip_candidates_features for the sessions [lo, hi): {column name: torch tensor} in the order of
        feature_columns(), one value per candidate of the range in the handle's order. events = (offsets, aid, ts,
        type), sources and session_cl are those the handle was generated from (device tensors are used in place);
        labels = (lab_off, lab_aid) in the labels_csr layout, None omits the target columns. "session" holds the
        session's index in the handle; cos_sim_ses_aid / eucl_dist_ses_aid hold their null fills (0, -1): they are
        popularity.session_item_similarity's outputs over the same range."""
        import torch
        dev = _dev(self.ctx)
        hi = self.n_sessions if hi is None else int(hi)
        lo = int(lo)
        if not (0 <= lo <= hi <= self.n_sessions):
            raise ValueError(f"session range [{lo}, {hi}) outside [0, {self.n_sessions}]")
        t = lambda x, d: (x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))).to(dev, d).contiguous()
        off, a, s_, y = (t(events[0], torch.int64), t(events[1], torch.int32), t(events[2], torch.int32),
                         t(events[3], torch.int8))
        if off.numel() and int(off[0].item()) != 0:
            off = off - off[0]
        cl = None if session_cl is None else t(session_cl, torch.int32)
        lab = None if labels is None else (t(labels[0], torch.int64), t(labels[1], torch.int32))
        coff = getattr(self, "_off_host", None)
        if coff is None:
            coff = self._off_host = self.to_torch()["off"].cpu().numpy()
        n = int(coff[hi] - coff[lo])
        table = feature_columns(labels is not None)
        out, ptrs = {}, (ctypes.c_void_p * len(table))()
        for i, (nm, dt) in enumerate(table):
            tt = getattr(torch, dt.name)
            if nm == "cos_sim_ses_aid":
                out[nm] = torch.zeros(n, dtype=tt, device=dev)
            elif nm == "eucl_dist_ses_aid":
                out[nm] = torch.full((n,), -1.0, dtype=tt, device=dev)
            else:
                out[nm] = torch.empty(n, dtype=tt, device=dev)
            ptrs[i] = _lib.ptr(out[nm]) if n else None
        _lib.check(_lib.load().ottohip_candidates_features(
            self.ctx.h, self.h, _lib.ptr(off), _lib.ptr(a) if a.numel() else None, _lib.ptr(s_) if a.numel() else None,
            _lib.ptr(y) if a.numel() else None, ctypes.addressof(sources.abi), ctypes.addressof(values.abi),
            _lib.ptr(cl) if cl is not None else None, _lib.ptr(lab[0]) if lab is not None else None,
            _lib.ptr(lab[1]) if (lab is not None and lab[1].numel()) else None, lo, hi, ptrs, len(table),
            _lib.stream_handle(stream)))
        return out

    def to_pandas(self, session_ids=None):
        """DataFrame[session, aid_next:int32, ts_order_aid:int16, src_*:int8] in output order."""
        import pandas as pd
        t = {k: v.cpu().numpy() for k, v in self.to_torch().items()}
        sess = np.arange(self.n_sessions) if session_ids is None else np.asarray(session_ids)
        out = {"session": np.repeat(sess, np.diff(t["off"])), "aid_next": t["aid_next"],
               "ts_order_aid": t["ts_order_aid"]}
        f = t["flags"].view(np.uint16)
        for i, n in enumerate(SRC_NAMES):
            out[n] = ((f >> i) & 1).astype(np.int8)
        return pd.DataFrame(out)

    def recall(self, labels_off, labels_aid, src: str | None = None, max_k: int = 20, stream=None) -> dict:
        """R9 on the device: labels as CSR [3 * (S+1)] offsets (int64) + aids (int32)."""
        return recall_from_sums(self.recall_sums(labels_off, labels_aid, src, max_k, stream))

    def recall_sums(self, labels_off, labels_aid, src: str | None = None, max_k: int = 20, stream=None) -> list:
        """The 15 integer sums behind recall (per type: hit@20, @100, @200, @all, true; clipped at
        max_k per session): additive over session shards."""
        import torch
        dev = _dev(self.ctx)
        lo = torch.as_tensor(labels_off).to(dev, torch.int64).contiguous()
        la = torch.as_tensor(labels_aid).to(dev, torch.int32).contiguous()
        sums = (ctypes.c_int64 * 15)()
        mask = 0 if src in (None, "src_any") else SRC_BIT[src]
        _lib.check(_lib.load().ottohip_candidates_recall(self.ctx.h, self.h, _lib.ptr(lo),
                                                         _lib.ptr(la) if la.numel() else None, mask, int(max_k), sums,
                                                         _lib.stream_handle(stream)))
        return list(sums)


def recall_from_sums(s) -> dict:
    """model/eval_retrieved.py:81-110: per type sums -> recall@k, total weighted 0.1/0.3/0.6."""
    res = {}
    for t, nm in enumerate(["clicks", "carts", "orders"]):
        h20, h100, h200, hall, tru = s[t * 5:(t + 1) * 5]
        res[nm] = {k: (v / tru if tru else 0.0) for k, v in
                   (("top20", h20), ("top100", h100), ("top200", h200), ("topall", hall))}
    res["total"] = {k: 0.1 * res["clicks"][k] + 0.3 * res["carts"][k] + 0.6 * res["orders"][k] for k in res["clicks"]}
    return res


def generate(offsets, aid, ts, type_, sources: CandidateSources, session_cl=None, stream=None) -> Candidates:
    """Candidates for every session of a session-sorted event table (device or host columns)."""
    import torch
    ctx = sources.ctx
    dev = _dev(ctx)
    t = lambda x, d: torch.as_tensor(np.asarray(x) if not isinstance(x, torch.Tensor) else x).to(dev, d).contiguous()
    off = t(offsets, torch.int64)
    off = off - off[0]
    a, s_, y = t(aid, torch.int32), t(ts, torch.int32), t(type_, torch.int8)
    S = int(off.numel()) - 1
    cl = None if session_cl is None else t(session_cl, torch.int32)
    h = ctypes.c_void_p()
    _lib.check(_lib.load().ottohip_candidates_generate(ctx.h, _lib.ptr(off), S, _lib.ptr(a), _lib.ptr(s_), _lib.ptr(y),
                                                       ctypes.addressof(sources.abi), _lib.ptr(cl) if cl is not None else None,
                                                       ctypes.byref(h), _lib.stream_handle(stream)))
    return Candidates(h, ctx)


def labels_csr_device(session, aid, type_, session_ids, ctx=None, stream=None):
    """ottohip_labels_csr: label rows (session, aid, type; device tensors or host arrays) -> the
    device CSR (off int64 [3*(S+1)], aid int32) that Candidates.recall reads, sessions in the order
    of session_ids; unique per (session, type), aids ascending."""
    import torch
    ctx = ctx or _lib.context()
    dev = _dev(ctx)
    t = lambda x, d: (x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))).to(dev, d).contiguous()
    se, ai, ty, sid = t(session, torch.int32), t(aid, torch.int32), t(type_, torch.int8), t(session_ids, torch.int32)
    n, S = int(se.numel()), int(sid.numel())
    off = torch.empty(3 * (S + 1), dtype=torch.int64, device=dev)
    out = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    m = ctypes.c_int64()
    _lib.check(_lib.load().ottohip_labels_csr(ctx.h, _lib.ptr(sid) if S else None, S, _lib.ptr(se) if n else None,
                                              _lib.ptr(ai) if n else None, _lib.ptr(ty) if n else None, n,
                                              _lib.ptr(off), _lib.ptr(out) if n else None, ctypes.byref(m),
                                              _lib.stream_handle(stream)))
    return off, out[:int(m.value)]


def labels_csr(labels, session_ids):
    """labels DataFrame[session, aid, type] -> (off [3*(S+1)] int64, aid int32), unique per (session, type),
    sessions in the order of session_ids."""
    sid = np.asarray(session_ids, np.int64)
    S = len(sid)
    order = np.argsort(sid, kind="stable")
    ss = sid[order]
    ls = labels["session"].to_numpy().astype(np.int64)
    la = labels["aid"].to_numpy().astype(np.int64)
    lt = labels["type"].to_numpy().astype(np.int64)
    j = np.searchsorted(ss, ls)
    ok = (j < S) & (ss[np.minimum(j, S - 1)] == ls) & (lt >= 0) & (lt <= 2)
    si = order[np.minimum(j, S - 1)][ok]
    la, lt = la[ok], lt[ok]
    key = (lt << 60) | (si << 32) | la  # type, session index, aid (aid < 2^31 checked by the device ABI)
    key = np.unique(key)
    t_, s_, a_ = key >> 60, (key >> 32) & ((1 << 28) - 1), key & 0xFFFFFFFF
    offs = []
    for t in range(3):
        cnt = np.bincount(s_[t_ == t], minlength=S)
        o = np.zeros(S + 1, np.int64)
        np.cumsum(cnt, out=o[1:])
        offs.append(o + int((t_ < t).sum()))
    return np.concatenate(offs), a_.astype(np.int32)


def retrieve_candidates(df_sessions_aids_full, aid_pairs_co_events: dict, df_knns_w2vec_all, df_knns_w2vec_1_2,
                        df_session_cl=None, df_pop_cl50=None, n_items: int | None = None, file_out: str | None = None):
    """Candidate-only variant of retrieve_and_gen_feats (model/retrieve.py:422-657), pandas in/out.
    df_sessions_aids_full [session, aid, ts, type]; aid_pairs_co_events {name: R1 frame}; kNN frames
    [aid, aid_next, dist_w2vec*, rank_w2vec*]; df_session_cl [session, cl50]; df_pop_cl50 [aid, cl50, rank_*_cl50].
    Returns DataFrame[session, aid_next, ts_order_aid, src_*] sorted by (session, ts_order_aid, aid_next);
    file_out: also written in the retrieved schema (write_retrieved, :651-655)."""
    from .synth import events_from_columns
    d = df_sessions_aids_full
    ev = events_from_columns(d["session"].to_numpy(), d["aid"].to_numpy(), d["ts"].to_numpy(), d["type"].to_numpy())
    sess_ids = ev.session[ev.session_offsets[:-1]] if ev.n_sessions else np.zeros(0, np.int32)
    mx = [int(ev.aid.max()) + 1 if len(ev.aid) else 1]
    r1 = {}
    for n, df in aid_pairs_co_events.items():
        r1[n] = (df["aid"].to_numpy(), df["aid_next"].to_numpy(), df[f"{n}_rank"].to_numpy())
        mx.append(int(df["aid"].max()) + 1 if len(df) else 1)

    def knn(df):
        rc = [c for c in df.columns if c.startswith("rank_w2vec")][0]
        mx.append(int(df["aid"].max()) + 1 if len(df) else 1)
        return df["aid"].to_numpy(), df["aid_next"].to_numpy(), df[rc].to_numpy()

    ka, k12 = knn(df_knns_w2vec_all), knn(df_knns_w2vec_1_2)
    n_items = max(mx + [n_items or 0, config.N_ITEMS_OTTO])
    pop, ncl, scl = None, 0, None
    if df_session_cl is not None and df_pop_cl50 is not None:
        rank_cols = [c for c in df_pop_cl50.columns if c.startswith("rank_") and c.endswith("_cl50")]
        p = df_pop_cl50[df_pop_cl50[rank_cols].min(axis=1) <= 20] if rank_cols else df_pop_cl50
        clusters = np.unique(np.concatenate([p["cl50"].to_numpy(), df_session_cl["cl50"].dropna().to_numpy()]))
        cmap = {int(c): i for i, c in enumerate(clusters)}
        pop = (p["cl50"].map(cmap).to_numpy(), p["aid"].to_numpy())
        ncl = len(clusters)
        scl = session_cluster_index(df_session_cl, clusters, sess_ids)
    src = CandidateSources(r1, ka, k12, pop, ncl, n_items)
    c = generate(ev.session_offsets, ev.aid, ev.ts, ev.type, src, scl)
    out = c.to_pandas(sess_ids)
    c.free()
    if file_out is not None:
        write_retrieved(out, file_out)
    return out


class FeatureJob:
    """The device state behind retrieve_and_gen_feats for one sessions file: the candidates of every session
    (generate) and the sources, value columns, labels and embeddings their features are made of. range(lo, hi)
    returns the finished columns of the sessions [lo, hi) (positions in session-id order), so a caller, or each
    rank of several, takes the file in pieces that fit its memory. Frames as retrieve_and_gen_feats takes them."""

    def __init__(self, df_sessions_aids_full, aid_pairs_co_events: dict, df_knns_w2vec_all, df_knns_w2vec_1_2,
                 df_session_cl, df_pop_cl1, df_pop_cl50, df_aid_embeddings, df_session_embeddings, df_labels,
                 n_items: int | None = None):
        import torch
        from . import popularity as gp
        from .synth import events_from_columns
        d = df_sessions_aids_full
        ses = d["session"].to_numpy()
        if len(ses) and np.any(np.diff(ses.astype(np.int64)) < 0):
            d = d.iloc[np.argsort(ses, kind="stable")]
        ev = events_from_columns(d["session"].to_numpy(), d["aid"].to_numpy(), d["ts"].to_numpy(), d["type"].to_numpy())
        sess_ids = ev.session[ev.session_offsets[:-1]] if ev.n_sessions else np.zeros(0, np.int32)
        mx = [int(ev.aid.max()) + 1 if len(ev.aid) else 1, int(df_pop_cl1["aid"].max()) + 1 if len(df_pop_cl1) else 1]
        r1, r1v = {}, {}
        for n, df in aid_pairs_co_events.items():
            a = df["aid"].to_numpy()
            r1[n] = (a, df["aid_next"].to_numpy(), df[f"{n}_rank"].to_numpy())
            r1v[n] = (a, df[f"{n}_count"].to_numpy(), df[f"{n}_count_pop"].to_numpy(), df[f"{n}_perc_pop"].to_numpy(),
                      df[f"{n}_count_rel"].to_numpy())
            mx.append(int(df["aid"].max()) + 1 if len(df) else 1)

        def knn(df):
            rc = [c for c in df.columns if c.startswith("rank_w2vec")][0]
            dc = [c for c in df.columns if c.startswith("dist_w2vec")][0]
            mx.append(int(df["aid"].max()) + 1 if len(df) else 1)
            return (df["aid"].to_numpy(), df["aid_next"].to_numpy(), df[rc].to_numpy()), (df["aid"].to_numpy(), df[dc].to_numpy())

        (ka, kav), (k12, k12v) = knn(df_knns_w2vec_all), knn(df_knns_w2vec_1_2)
        n_items = max(mx + [n_items or 0, config.N_ITEMS_OTTO])
        p = df_pop_cl50[df_pop_cl50[CL50_RANKS].min(axis=1) <= 20]  # :581-582
        clusters = np.unique(np.concatenate([p["cl50"].to_numpy(), df_session_cl["cl50"].dropna().to_numpy()]))
        pc = np.searchsorted(clusters, p["cl50"].to_numpy())
        scl = session_cluster_index(df_session_cl, clusters, sess_ids)
        src = CandidateSources(r1, ka, k12, (pc, p["aid"].to_numpy()), len(clusters), n_items)
        val = FeatureValues(src, r1v, kav, k12v, (pc, p[CL50_RANKS].to_numpy()),
                            (df_pop_cl1["aid"].to_numpy(), df_pop_cl1[CL1_RANKS].to_numpy()))
        dev = _dev(src.ctx)
        events = tuple(torch.as_tensor(x).to(dev) for x in (ev.session_offsets, ev.aid, ev.ts, ev.type))
        scl_d = torch.from_numpy(scl).to(dev)
        c = generate(*events, src, scl_d)
        labels = None
        if df_labels is not None:
            lo_, la_ = labels_csr(df_labels, sess_ids)
            labels = (torch.from_numpy(lo_).to(dev), torch.from_numpy(la_).to(dev))
        # R7 inputs: session embedding rows in session order, item embeddings by aid
        dim_a = [x for x in df_aid_embeddings.columns if x.startswith("dim_")]
        dim_s = [x for x in df_session_embeddings.columns if x.startswith("dim_")]
        sim = None
        if len(dim_a) and len(dim_a) == len(dim_s) and len(df_aid_embeddings):
            se = np.zeros((ev.n_sessions, len(dim_s)), np.float32)
            has = np.zeros(ev.n_sessions, np.uint8)
            order = np.argsort(sess_ids, kind="stable")
            ks = df_session_embeddings["session"].to_numpy().astype(np.int64)
            j = np.searchsorted(sess_ids[order], ks)
            ok = (j < ev.n_sessions) & (sess_ids[order][np.minimum(j, max(ev.n_sessions - 1, 0))] == ks)
            se[order[j[ok]]] = df_session_embeddings[dim_s].to_numpy().astype(np.float32)[ok]
            has[order[j[ok]]] = 1
            words = df_aid_embeddings["aid"].to_numpy()
            emb = torch.from_numpy(np.ascontiguousarray(df_aid_embeddings[dim_a].to_numpy().astype(np.float32))).to(dev)
            sim = (torch.from_numpy(se).to(dev), torch.from_numpy(has).to(dev), emb,
                   gp.row_of_aid_map(words, n_items, dev), words)
        self.cands, self.events, self.sources, self.values, self.session_cl = c, events, src, val, scl_d
        self.labels, self.sim, self.n_items, self.n_sessions = labels, sim, n_items, ev.n_sessions
        self.table = feature_columns(labels is not None)
        t = c.to_torch()
        self.cand_off, self.cand_next = t["off"], t["aid_next"]
        self.cand_off_host = t["off"].cpu().numpy()
        self.session_ids = torch.from_numpy(np.ascontiguousarray(sess_ids).astype(np.int32)).to(dev)

    def range(self, lo: int, hi: int) -> dict:
        """{column: torch tensor} of the sessions [lo, hi): Candidates.features with the session ids filled in and
        cos / eucl from ottohip_session_item_similarity over the same range."""
        from . import popularity as gp
        f = self.cands.features(self.events, self.sources, self.values, self.session_cl, self.labels, lo, hi)
        if f["session"].numel():
            f["session"] = self.session_ids[f["session"].long()]
            if self.sim is not None:
                se, has, emb, rmap, words = self.sim
                co = self.cand_off_host
                off_r = self.cand_off[lo:hi + 1] - self.cand_off[lo]
                f["cos_sim_ses_aid"], f["eucl_dist_ses_aid"] = gp.session_item_similarity(
                    off_r, self.cand_next[int(co[lo]):int(co[hi])], se[lo:hi], words, emb, sess_has=has[lo:hi],
                    n_items=self.n_items, ctx=self.sources.ctx, rmap=rmap)
        return f

    def free(self):
        self.cands.free()


def retrieve_and_gen_feats(df_sessions_aids_full, aid_pairs_co_events: dict, df_knns_w2vec_all, df_knns_w2vec_1_2,
                           df_session_cl, df_pop_cl1, df_pop_cl50, df_aid_embeddings, df_session_embeddings, df_labels,
                           file_out: str | None, n_items: int | None = None, memory_budget: int = 2 << 30):
    """retrieve_and_gen_feats of model/retrieve.py:422-657, pandas in / out: candidates with every ranker feature
    column, written to file_out (parquet, the reference's column names and dtypes, rows sorted by (session,
    ts_order_aid, aid_next)) and returned. aid_pairs_co_events {rule: R1 frame with all seven columns}; kNN frames
    [aid, aid_next, dist_w2vec_*, rank_w2vec_*]; df_session_cl [session, cl50]; df_pop_cl1 [aid, rank_*_cl1];
    df_pop_cl50 [aid, cl50, six rank_*_cl50]; df_aid_embeddings [aid, dim_*]; df_session_embeddings [session,
    dim_*]; df_labels [session, aid, type] or None (no target columns). Sessions are processed in ranges whose
    feature columns fit memory_budget bytes on the device."""
    import pandas as pd
    job = FeatureJob(df_sessions_aids_full, aid_pairs_co_events, df_knns_w2vec_all, df_knns_w2vec_1_2, df_session_cl,
                     df_pop_cl1, df_pop_cl50, df_aid_embeddings, df_session_embeddings, df_labels, n_items)
    table, coff, S = job.table, job.cand_off_host, job.n_sessions
    max_rows = max(1, int(memory_budget) // sum(dt.itemsize for _, dt in table))
    writer, frames = None, []
    if file_out is not None:
        import pyarrow as pa
        import pyarrow.parquet as pq
        os.makedirs(os.path.dirname(os.path.abspath(file_out)), exist_ok=True)
        schema = pa.schema([(nm, pa.from_numpy_dtype(dt)) for nm, dt in table])
        writer = pq.ParquetWriter(file_out, schema)
    lo = 0
    while True:
        hi = int(np.searchsorted(coff, coff[lo] + max_rows, side="right")) - 1
        hi = min(max(hi, lo + 1), S)  # at least one session per range
        f = job.range(lo, hi)
        host = {nm: f[nm].cpu().numpy() for nm, _ in table}
        frames.append(pd.DataFrame(host))
        if writer is not None:
            writer.write_table(pa.table({nm: pa.array(host[nm]) for nm, _ in table}, schema=schema))
        lo = hi
        if lo >= S:
            break
    if writer is not None:
        writer.close()
    job.free()
    return pd.concat(frames, ignore_index=True) if len(frames) > 1 else frames[0]


def session_cluster_index(df_session_cl, clusters, sess_ids) -> np.ndarray:
    """Dense cluster index (position in the sorted `clusters`) of every session in sess_ids, -1 for a
    session without a row or with a null cl50: one sorted search. A session listed more than once
    takes its LAST row (the dict lookup this replaced kept the last value of a duplicated key)."""
    sc = df_session_cl.dropna(subset=["cl50"])
    ks = sc["session"].to_numpy().astype(np.int64)
    kc = np.searchsorted(clusters, sc["cl50"].to_numpy())
    o = np.argsort(ks, kind="stable")
    ks, kc = ks[o], kc[o]
    q = np.asarray(sess_ids, np.int64)
    j = np.searchsorted(ks, q, side="right") - 1  # the last of equal sessions (stable order)
    hit = j >= 0
    hit[hit] = ks[j[hit]] == q[hit]
    return np.where(hit, kc[np.maximum(j, 0)] if len(ks) else -1, -1).astype(np.int32)


def write_retrieved(df, file_out):
    """The retrieved-candidates file of retrieve_and_gen_feats (model/retrieve.py:647-655):
    rows sorted by (session, ts_order_aid) -- ties by aid_next here -- written to parquet with the
    candidate columns [session:int32, aid_next:int32, ts_order_aid:int16, src_*:int8], the columns
    model/eval_retrieved.py:45-53 reads (session, aid_next, src_*; rank = position in the session)."""
    import pyarrow as pa
    import pyarrow.parquet as pq
    d = df.sort_values(["session", "ts_order_aid", "aid_next"], kind="stable")
    cols = {"session": pa.array(d["session"].to_numpy().astype(np.int32)),
            "aid_next": pa.array(d["aid_next"].to_numpy().astype(np.int32)),
            "ts_order_aid": pa.array(d["ts_order_aid"].to_numpy().astype(np.int16))}
    for n in SRC_NAMES:
        if n in d.columns:
            cols[n] = pa.array(d[n].to_numpy().astype(np.int8))
    os.makedirs(os.path.dirname(os.path.abspath(file_out)), exist_ok=True)
    pq.write_table(pa.table(cols), file_out)
