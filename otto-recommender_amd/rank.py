"""The rank stage on MI355X: LightGBM booster scoring and the per-session top-k (model/rank.py, model/submit.py).

Mirrors model/rank.py:37-59 (load_lgbm, Booster.predict over the retrieved candidates, ordinal rank by
pred_score descending per session, keep pred_rank <= keep_top_k, sort by (session, pred_rank)) and the join of
model/submit.py:32-56. The model is LightGBM's text booster file, parsed here (lightgbm is not needed); scoring
and ranking run in libottohip.so (csrc/rank.hip) on the typed feature columns as they sit on the device: no
float64 matrix is built, the frame is read once for all targets, and only the kept rows leave the device.

Semantics: numeric splits only, raw-score objectives only, every tree used, score = 0.0 + the
leaves in tree order in float64; ties in pred_score go to the earlier row of the frame's (ts_order_aid, aid_next)
order.
"""
from __future__ import annotations

import ctypes
import glob
import os
from dataclasses import dataclass, field

import numpy as np

from . import _lib
from . import config

RAW_SCORE_OBJECTIVES = ("lambdarank", "rank_xendcg", "regression")
RANKED_DTYPES = (("session", np.int32), ("aid_next", np.int32), ("pred_score", np.float64), ("pred_rank", np.int16))


@dataclass
class Forest:
    """One booster as its model file holds it. Node arrays are the trees' concatenated: tree t has
    tree_off[t + 1] - tree_off[t] internal nodes and one more leaf (leaf_value[tree_off[t] + t ...]);
    split_feature indexes feature_names."""
    feature_names: list
    objective: str
    version: str
    max_feature_idx: int
    tree_off: np.ndarray
    split_feature: np.ndarray
    threshold: np.ndarray
    decision_type: np.ndarray
    left_child: np.ndarray
    right_child: np.ndarray
    leaf_value: np.ndarray
    shrinkage: np.ndarray = field(default_factory=lambda: np.zeros(0))

    @property
    def n_trees(self) -> int:
        return len(self.tree_off) - 1

    @property
    def num_leaves(self) -> np.ndarray:
        return np.diff(self.tree_off) + 1


def _column_names(columns) -> list:
    if columns is None:
        from .candidates import feature_columns
        columns = feature_columns(with_targets=False)
    return [c if isinstance(c, str) else c[0] for c in columns]


def parse_booster(path_or_text, columns=None) -> Forest:
    """LightGBM's text model (Booster.save_model, *.booster.lgbm) -> Forest, host only. A model this stage cannot
    score exactly raises ValueError: several classes or trees per iteration, categorical or linear trees,
    average_output, an objective whose predict is not the raw score, a threshold or leaf value that is not finite,
    a child outside its tree, a feature that is not a column (columns: names or (name, dtype) pairs; default the
    feature frame without targets). Everything after 'end of trees' is ignored."""
    text = path_or_text
    if "\n" not in str(path_or_text):
        with open(path_or_text) as fh:
            text = fh.read()
    lines = [ln.strip() for ln in str(text).splitlines()]
    head, trees, cur, ended = {}, [], None, False
    for ln in lines:
        if ln == "end of trees":
            ended = True
            break
        if not ln:
            continue
        if ln.startswith("Tree="):
            cur = {}
            trees.append(cur)
            continue
        k, sep, v = ln.partition("=")
        tgt = head if cur is None else cur
        tgt[k] = v if sep else True
    if "tree" not in head or not ended:
        raise ValueError("not a LightGBM text model: no 'tree' header or no 'end of trees'")
    version = head.get("version", "")
    if version not in ("v2", "v3", "v4"):
        raise ValueError(f"model version {version!r} is not v2, v3 or v4")
    if int(head.get("num_class", 1)) != 1 or int(head.get("num_tree_per_iteration", 1)) != 1:
        raise ValueError("num_class and num_tree_per_iteration must be 1")
    if "average_output" in head:
        raise ValueError("average_output models (random forest mode) are not supported")
    objective = str(head.get("objective", "")).split(" ")[0]
    if objective not in RAW_SCORE_OBJECTIVES:
        raise ValueError(f"objective {objective!r}: predict is the raw score only for {RAW_SCORE_OBJECTIVES}")
    names = str(head.get("feature_names", "")).split()
    max_idx = int(head.get("max_feature_idx", len(names) - 1))
    if len(names) != max_idx + 1:
        raise ValueError(f"feature_names has {len(names)} names, max_feature_idx is {max_idx}")
    known = set(_column_names(columns))
    for n in names:
        if n not in known:
            raise ValueError(f"model feature {n!r} is not a column of the feature frame")

    def arr(t, key, dtype, n, i):
        v = np.array(str(t.get(key, "")).split(), dtype=np.float64 if dtype is np.float64 else np.int64)
        if len(v) != n:
            raise ValueError(f"Tree={i}: {key} has {len(v)} values, expected {n}")
        return v

    off, sf, th, dt, lc, rc, lv, shr = [0], [], [], [], [], [], [], []
    for i, t in enumerate(trees):
        nl = int(t.get("num_leaves", 0))
        if nl < 1:
            raise ValueError(f"Tree={i}: num_leaves {nl}")
        if int(t.get("num_cat", 0)) > 0:
            raise ValueError(f"Tree={i}: categorical splits (num_cat > 0) are not supported")
        if int(t.get("is_linear", 0)) != 0:
            raise ValueError(f"Tree={i}: linear trees are not supported")
        ni = nl - 1
        leaf = arr(t, "leaf_value", np.float64, nl, i)
        if not np.all(np.isfinite(leaf)):
            raise ValueError(f"Tree={i}: a leaf value is not finite")
        lv.append(leaf)
        shr.append(float(t.get("shrinkage", 1.0)))
        off.append(off[-1] + ni)
        if ni == 0:
            continue
        f, x, d = arr(t, "split_feature", np.int64, ni, i), arr(t, "threshold", np.float64, ni, i), \
            arr(t, "decision_type", np.int64, ni, i)
        l, r = arr(t, "left_child", np.int64, ni, i), arr(t, "right_child", np.int64, ni, i)
        if not np.all(np.isfinite(x)):
            raise ValueError(f"Tree={i}: a threshold is not finite")
        if np.any(d & 1):
            raise ValueError(f"Tree={i}: categorical split (decision_type bit 0)")
        if np.any((d < 0) | (d > 15) | (((d >> 2) & 3) == 3)):
            raise ValueError(f"Tree={i}: decision_type outside the numeric split encodings")
        if np.any((f < 0) | (f > max_idx)):
            raise ValueError(f"Tree={i}: split_feature outside [0, {max_idx}]")
        for c in (l, r):
            if np.any((c >= ni) | (c < -nl)):
                raise ValueError(f"Tree={i}: a child index is outside the tree")
        sf.append(f); th.append(x); dt.append(d); lc.append(l); rc.append(r)
    cat = lambda parts, dtype: (np.concatenate(parts) if parts else np.zeros(0)).astype(dtype)
    return Forest(names, objective, version, max_idx, np.asarray(off, np.int32), cat(sf, np.int32), cat(th, np.float64),
                  cat(dt, np.int32), cat(lc, np.int32), cat(rc, np.int32), cat(lv, np.float64), np.asarray(shr))


_DT_CODE = {np.dtype(np.int8): 0, np.dtype(np.int16): 1, np.dtype(np.int32): 2, np.dtype(np.float32): 3}


def lower_threshold(threshold: float, decision_type: int, dtype) -> tuple:
    """ottohip_rank_lower (no GPU call): the split as the device compares it on a column of numpy dtype `dtype`:
    (key, flags, band_lo, band_hi); see include/ottohip.h."""
    key, fl, lo, hi = ctypes.c_int32(), ctypes.c_int(), ctypes.c_int32(), ctypes.c_int32()
    _lib.check(_lib.load().ottohip_rank_lower(float(threshold), int(decision_type), _DT_CODE[np.dtype(dtype)],
                                              ctypes.byref(key), ctypes.byref(fl), ctypes.byref(lo), ctypes.byref(hi)))
    return key.value, fl.value, lo.value, hi.value


class Ranker:
    """The boosters of the targets on the device (ottohip_ranker_create). models: {target: Forest or model file};
    columns: [(name, numpy dtype)] the feature tensors are given in (default the feature frame without targets)."""

    def __init__(self, models: dict, ctx=None, columns=None):
        if columns is None:
            from .candidates import feature_columns
            columns = feature_columns(with_targets=False)
        self.ctx = ctx or _lib.context()
        self.columns = [(n, np.dtype(d)) for n, d in columns]
        self.targets = list(models)
        index = {n: i for i, (n, _) in enumerate(self.columns)}
        self.forests = [m if isinstance(m, Forest) else parse_booster(m, self.columns) for m in models.values()]
        abi = (_lib.Forest * len(self.forests))()
        self._keep = []
        for a, f in zip(abi, self.forests):
            missing = [n for n in f.feature_names if n not in index]
            if missing:
                raise ValueError(f"model features {missing} are not columns of the feature frame")
            cmap = np.array([index[n] for n in f.feature_names], np.int32)
            arrays = [np.ascontiguousarray(f.tree_off, np.int32),
                      np.ascontiguousarray(cmap[f.split_feature] if len(f.split_feature) else f.split_feature, np.int32),
                      np.ascontiguousarray(f.threshold, np.float64), np.ascontiguousarray(f.decision_type, np.int32),
                      np.ascontiguousarray(f.left_child, np.int32), np.ascontiguousarray(f.right_child, np.int32),
                      np.ascontiguousarray(f.leaf_value, np.float64)]
            self._keep.append(arrays)
            a.n_trees = f.n_trees
            (a.tree_off, a.split_feature, a.threshold, a.decision_type, a.left_child, a.right_child,
             a.leaf_value) = [x.ctypes.data if x.size else None for x in arrays]
        codes = (ctypes.c_int * len(self.columns))(*[_DT_CODE[d] for _, d in self.columns])
        self.h = ctypes.c_void_p()
        _lib.check(_lib.load().ottohip_ranker_create(self.ctx.h, abi, len(self.forests), codes, len(self.columns),
                                                     ctypes.byref(self.h)))

    def info(self) -> dict:
        nf, nu, nr, lds = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int64()
        _lib.check(_lib.load().ottohip_ranker_info(self.h, ctypes.byref(nf), ctypes.byref(nu), ctypes.byref(nr),
                                                   ctypes.byref(lds)))
        return {"n_forests": nf.value, "n_used_columns": nu.value, "n_lds_resident": nr.value, "lds_bytes": lds.value}

    def free(self):
        if getattr(self, "h", None):
            _lib.load().ottohip_ranker_free(self.h)
            self.h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

    def _scores(self, features: dict, stream=None):
        import torch
        dev = torch.device("cuda", self.ctx.device)
        ptrs = (ctypes.c_void_p * len(self.columns))()
        n, keep = None, []
        for i, (nm, dt) in enumerate(self.columns):
            t = features.get(nm)
            if t is None:
                continue  # a column no forest reads may be absent; one that is read is the library's argument error
            if str(t.dtype) != f"torch.{dt.name}":
                raise TypeError(f"column {nm}: {t.dtype}, the ranker was created for {dt.name}")
            if t.device != dev or t.dim() != 1:
                raise ValueError(f"column {nm}: a 1-d tensor on {dev} is needed")
            t = t.contiguous()
            keep.append(t)
            if n is None:
                n = int(t.numel())
            elif int(t.numel()) != n:
                raise ValueError(f"column {nm} has {int(t.numel())} rows, others {n}")
            ptrs[i] = _lib.ptr(t) if n else None
        if n is None:
            raise ValueError("no feature column given")
        scores = torch.empty((len(self.forests), n), dtype=torch.float64, device=dev)
        if n:
            _lib.check(_lib.load().ottohip_ranker_predict(self.ctx.h, self.h, ptrs, len(self.columns), n,
                                                          _lib.ptr(scores), _lib.stream_handle(stream)))
        else:  # the argument check still applies to an empty frame
            _lib.check(_lib.load().ottohip_ranker_predict(self.ctx.h, self.h, ptrs, len(self.columns), 0, None,
                                                          _lib.stream_handle(stream)))
        return scores

    def predict(self, features: dict, stream=None) -> dict:
        """Booster.predict (model/rank.py:50) of every target in one pass over the frame: {column: device tensor}
        -> {target: float64 tensor}."""
        s = self._scores(features, stream)
        return {t: s[i] for i, t in enumerate(self.targets)}

    def topk(self, scores, cand_off, aid_next, keep_top_k: int = config.KEEP_TOP_K, stream=None) -> list:
        """ottohip_ranker_topk on a [n_forests, n_rows] score tensor: per forest {session (index), aid_next,
        pred_score, pred_rank} of the kept rows in (session, pred_rank) order."""
        import torch
        dev = scores.device
        off = cand_off.to(dev, torch.int64).contiguous()
        S = int(off.numel()) - 1
        nf, n = int(scores.shape[0]), int(scores.shape[1])
        k = int(keep_top_k)
        cap = max(min(n, S * max(k, 0)), 0)
        out_off = torch.empty(S + 1, dtype=torch.int64, device=dev)
        o_s = torch.empty(max(nf * cap, 1), dtype=torch.int32, device=dev)
        o_a = torch.empty(max(nf * cap, 1), dtype=torch.int32, device=dev)
        o_p = torch.empty(max(nf * cap, 1), dtype=torch.float64, device=dev)
        o_r = torch.empty(max(nf * cap, 1), dtype=torch.int16, device=dev)
        an = aid_next.to(dev, torch.int32).contiguous()
        _lib.check(_lib.load().ottohip_ranker_topk(self.ctx.h, _lib.ptr(scores) if n else None, nf, n, _lib.ptr(off), S,
                                                   _lib.ptr(an) if n else None, k, cap, _lib.ptr(out_off), _lib.ptr(o_s),
                                                   _lib.ptr(o_a), _lib.ptr(o_p), _lib.ptr(o_r),
                                                   _lib.stream_handle(stream)))
        m = int(out_off[-1].item())
        return [{"session": o_s[f * cap:f * cap + m], "aid_next": o_a[f * cap:f * cap + m],
                 "pred_score": o_p[f * cap:f * cap + m], "pred_rank": o_r[f * cap:f * cap + m]} for f in range(nf)]

    def rank(self, features: dict, cand_off, keep_top_k: int = config.KEEP_TOP_K, session_ids=None, stream=None) -> dict:
        """model/rank.py:50-57 on the device: score the frame, keep each session's keep_top_k (<= 64) best rows.
        features holds the ranker's columns and aid_next; cand_off [S + 1] are the sessions' row offsets (relative
        to cand_off[0]). 'session' of the result is session_ids[s] when given, else the frame's session column
        when present, else the session's index. -> {target: {session, aid_next, pred_score, pred_rank}}."""
        import torch
        scores = self._scores(features, stream)
        off = torch.as_tensor(cand_off).to(scores.device, torch.int64)
        res = self.topk(scores, off, features["aid_next"], keep_top_k, stream)
        out = {}
        for t, r in zip(self.targets, res):
            s = r["session"].long()
            if session_ids is not None:
                r["session"] = torch.as_tensor(session_ids).to(scores.device, torch.int32)[s]
            elif "session" in features:
                r["session"] = features["session"][(off[:-1] - off[0])[s]].to(torch.int32)
            out[t] = r
        return out


def _frame(parts: list):
    import pandas as pd
    cols = {}
    for nm, dt in RANKED_DTYPES:
        v = [p[nm].cpu().numpy() for p in parts]
        cols[nm] = (np.concatenate(v) if v else np.zeros(0)).astype(dt, copy=False)
    return pd.DataFrame(cols)


def write_ranked(df, file_out: str):
    """A ranked file of model/rank.py:59: [session:int32, aid_next:int32, pred_score:float64, pred_rank:int16]."""
    import pyarrow as pa
    import pyarrow.parquet as pq
    os.makedirs(os.path.dirname(os.path.abspath(file_out)), exist_ok=True)
    pq.write_table(pa.table({nm: pa.array(df[nm].to_numpy().astype(dt, copy=False)) for nm, dt in RANKED_DTYPES}),
                   file_out)


def rank_job(job, ranker: Ranker, keep_top_k: int = config.KEEP_TOP_K, memory_budget: int = 2 << 30) -> dict:
    """Scores and ranks a candidates.FeatureJob a session range at a time (the range sizing of
    retrieve_and_gen_feats): the feature columns of a range live only on the device, the kept rows are
    concatenated. -> {target: DataFrame[session, aid_next, pred_score, pred_rank]}."""
    table, coff, S = job.table, job.cand_off_host, job.n_sessions
    max_rows = max(1, int(memory_budget) // sum(dt.itemsize for _, dt in table))
    parts = {t: [] for t in ranker.targets}
    lo = 0
    while lo < S:
        hi = int(np.searchsorted(coff, coff[lo] + max_rows, side="right")) - 1
        hi = min(max(hi, lo + 1), S)
        f = job.range(lo, hi)
        if int(coff[hi] - coff[lo]) > 0:
            r = ranker.rank(f, job.cand_off[lo:hi + 1], keep_top_k, session_ids=job.session_ids[lo:hi])
            for t in ranker.targets:
                parts[t].append(r[t])
        lo = hi
    return {t: _frame(parts[t]) for t in ranker.targets}


def retrieve_and_rank(df_sessions_aids_full, aid_pairs_co_events: dict, df_knns_w2vec_all, df_knns_w2vec_1_2,
                      df_session_cl, df_pop_cl1, df_pop_cl50, df_aid_embeddings, df_session_embeddings, df_labels,
                      models, dir_out: str | None = None, keep_top_k: int = config.KEEP_TOP_K, name: str = "ranked",
                      n_items: int | None = None, memory_budget: int = 2 << 30) -> dict:
    """retrieve_and_gen_feats followed by model/rank.py without the retrieved file in between: the arguments of
    candidates.retrieve_and_gen_feats (df_labels is accepted and not used: no target column is needed), models
    {target: Forest or model file} or a Ranker. Returns {target: DataFrame}; with dir_out also writes
    dir_out/{target}/{name}.parquet."""
    from .candidates import FeatureJob
    job = FeatureJob(df_sessions_aids_full, aid_pairs_co_events, df_knns_w2vec_all, df_knns_w2vec_1_2, df_session_cl,
                     df_pop_cl1, df_pop_cl50, df_aid_embeddings, df_session_embeddings, None, n_items)
    ranker = models if isinstance(models, Ranker) else Ranker(models, job.sources.ctx)
    try:
        out = rank_job(job, ranker, keep_top_k, memory_budget)
    finally:
        job.free()
        if ranker is not models:
            ranker.free()
    if dir_out is not None:
        for t, df in out.items():
            write_ranked(df, os.path.join(dir_out, t, f"{name}.parquet"))
    return out


def rank_files(dir_retrieved: str, dir_models: str, dir_out: str, targets=("clicks", "carts", "orders"),
               keep_top_k: int = config.KEEP_TOP_K, ctx=None) -> list:
    """The __main__ of model/rank.py: every *.parquet of dir_retrieved (files of retrieve_and_gen_feats) scored
    with {dir_models}/{target}.booster.lgbm and written to {dir_out}/{target}/{basename}. Each file's columns
    are uploaded once and all targets scored in one call. Returns the written paths."""
    import pyarrow.parquet as pq
    import torch
    ranker = Ranker({t: os.path.join(dir_models, f"{t}.booster.lgbm") for t in targets}, ctx)
    dev = torch.device("cuda", ranker.ctx.device)
    need = {"session", "aid_next"}
    for f in ranker.forests:
        need.update(f.feature_names)
    written = []
    try:
        for path in sorted(glob.glob(os.path.join(dir_retrieved, "*.parquet"))):
            have = set(pq.read_schema(path).names)
            order = dict.fromkeys(["session", "aid_next"] + [n for n, _ in ranker.columns])
            tab = pq.read_table(path, columns=[n for n in order if n in need and n in have])
            dts = dict(ranker.columns, session=np.dtype(np.int32), aid_next=np.dtype(np.int32))
            host = {n: np.array(tab[n].to_numpy(), dtype=dts[n]) for n in tab.column_names}  # writable copies
            ses = host["session"]
            # the file is sorted by session: a session is a run of equal ids
            starts = np.flatnonzero(np.r_[True, ses[1:] != ses[:-1]]) if len(ses) else np.zeros(0, np.int64)
            off = np.r_[starts, len(ses)].astype(np.int64)
            feats = {n: torch.from_numpy(v).to(dev) for n, v in host.items()}
            r = ranker.rank(feats, torch.from_numpy(off).to(dev), keep_top_k)
            for t in ranker.targets:
                out = os.path.join(dir_out, t, os.path.basename(path))
                write_ranked(_frame([r[t]]), out)
                written.append(out)
    finally:
        ranker.free()
    return written


def submission_frame(ranked: dict):
    """model/submit.py:32-56, host only: {target: ranked frame} -> DataFrame[session_type, labels]: one row per
    (session, target) named '{session}_{target}', labels the aid_next joined by spaces in pred_rank order, rows
    sorted by session_type (as strings)."""
    import pandas as pd
    frames = []
    for target in config.TYPES:
        if target not in ranked:
            continue
        d = ranked[target].sort_values(["session", "pred_rank"], kind="stable")
        g = d.groupby("session", sort=True)["aid_next"].agg(lambda a: " ".join(str(int(x)) for x in a))
        frames.append(pd.DataFrame({"session_type": [f"{int(s)}_{target}" for s in g.index],
                                    "labels": g.to_numpy().astype(object)}))
    if not frames:
        return pd.DataFrame({"session_type": np.zeros(0, object), "labels": np.zeros(0, object)})
    return pd.concat(frames, ignore_index=True).sort_values("session_type", kind="stable").reset_index(drop=True)
