"""Negative downsampling of the retrieved candidates on MI355X (model/downsample_retrieved.py) and the loader a
trainer reads the result with (model/train_lgbm_rankers.py:38-60).

Mirrors model/downsample_retrieved.py:34-62 per target over a frame sorted by session: sessions without a positive
are dropped, every positive is kept, and of a session's negatives those with random < max_n_neg =
min(n_pos * keep_ratio_neg_to_pos, max_neg_per_session) (float64), random a permutation of [0, n_neg). The target
columns hold 0 or 1, as the feature stage writes them. The select and the column gather run in libottohip.so
(csrc/downsample.hip) on the frame as it sits on the device in session ranges; only the kept rows are copied to
the host.

The draw (downsample; parity with polars' shuffle(seed=42) is unpinned) is counter-based, so it does
not depend on row order, range boundaries or rank count: h(row) = mix(mix(seed) ^ (uint32(session) << 32 |
uint32(aid_next))) with splitmix64's mix, random(row) = the negatives of the same session and target with a smaller
(h, aid_next). Output order within a session: positives in frame order, then the kept negatives in frame order.
"""
from __future__ import annotations

import ctypes
import glob
import os

import numpy as np

from . import _lib
from . import config

_DT_CODE = {"int8": 0, "int16": 1, "int32": 2, "float32": 3}
MAX_GATHER_COLS = 128
NON_FEATS = ["session", "aid_next", "target_clicks", "target_carts", "target_orders", "rank_total_cl1"]  # :39


def draw_hash(seed: int, session: int, aid_next: int) -> int:
    """ottohip_downsample_hash (no GPU call): h of one row."""
    to32 = lambda v: ((int(v) + 2 ** 31) % 2 ** 32) - 2 ** 31
    return int(_lib.load().ottohip_downsample_hash(int(seed) & (2 ** 64 - 1), to32(session), to32(aid_next)))


def lds_rows() -> int:
    """The select's path switch (ottohip_downsample_lds_rows): sessions above it are ranked over global memory."""
    return int(_lib.load().ottohip_downsample_lds_rows())


def plan(cand_off, session, aid_next, target_columns: dict,
         keep_ratio_neg_to_pos: float = config.DOWNSAMPLE_RATIO_NEG_TO_POS,
         max_neg_per_session: float = config.DOWNSAMPLE_MAX_NEG_PER_SESSION, seed: int = 42, ctx=None,
         stream=None) -> dict:
    """ottohip_downsample_plan: {target: (out_off int64 [S + 1], rows int64)} for target_columns {target name of
    config.TYPES: int8 device tensor of 0 / 1}. cand_off [S + 1] are the sessions' row offsets, relative to
    cand_off[0]; rows are the source rows of the output rows in output order."""
    import torch
    ctx = ctx or _lib.context()
    dev = torch.device("cuda", ctx.device)
    lib = _lib.load()
    off = torch.as_tensor(cand_off).to(dev, torch.int64).contiguous()
    S = int(off.numel()) - 1
    if S < 0:
        raise ValueError("cand_off needs at least one entry")
    ses = torch.as_tensor(session).to(dev, torch.int32).contiguous()
    aid = torch.as_tensor(aid_next).to(dev, torch.int32).contiguous()
    n = int(ses.numel())
    if int(aid.numel()) != n:
        raise ValueError(f"aid_next has {int(aid.numel())} rows, session {n}")
    tg = (ctypes.c_void_p * 3)()
    keep = {}
    for name, col in target_columns.items():
        t = torch.as_tensor(col)
        if t.dtype != torch.int8:
            raise TypeError(f"target_{name}: {t.dtype}, the feature frame holds int8")
        t = t.to(dev).contiguous()
        if int(t.numel()) != n:
            raise ValueError(f"target_{name} has {int(t.numel())} rows, session {n}")
        # an empty column keeps a one-element buffer: the library reads a NULL pointer as "target not asked for"
        keep[name] = t if n else torch.zeros(1, dtype=torch.int8, device=dev)
        tg[config.TYPE2ID[name]] = _lib.ptr(keep[name])
    offs = {name: torch.empty(S + 1, dtype=torch.int64, device=dev) for name in keep}
    po = (ctypes.c_void_p * 3)()
    for name, o in offs.items():
        po[config.TYPE2ID[name]] = _lib.ptr(o)
    n_out = (ctypes.c_int64 * 3)()
    args = (ctx.h, _lib.ptr(off), S, n, _lib.ptr(ses) if n else None, _lib.ptr(aid) if n else None, tg,
            float(keep_ratio_neg_to_pos), float(max_neg_per_session), int(seed) & (2 ** 64 - 1), po)
    _lib.check(lib.ottohip_downsample_plan(*args, None, 0, n_out, _lib.stream_handle(stream)))
    cap = max([int(n_out[config.TYPE2ID[name]]) for name in keep] + [0])
    rows = {name: torch.empty(max(cap, 1), dtype=torch.int64, device=dev) for name in keep}
    pr = (ctypes.c_void_p * 3)()
    for name, r in rows.items():
        pr[config.TYPE2ID[name]] = _lib.ptr(r)
    _lib.check(lib.ottohip_downsample_plan(*args, pr, cap, n_out, _lib.stream_handle(stream)))
    return {name: (offs[name], rows[name][:int(n_out[config.TYPE2ID[name]])]) for name in keep}


def gather_rows(columns: dict, rows, ctx=None, stream=None) -> dict:
    """ottohip_gather_rows: {column: device tensor}[rows] for int8 / int16 / int32 / float32 columns of one length,
    one launch per 128 columns. rows: int64 device tensor of row indices."""
    import torch
    ctx = ctx or _lib.context()
    dev = torch.device("cuda", ctx.device)
    lib = _lib.load()
    idx = torch.as_tensor(rows).to(dev, torch.int64).contiguous()
    m = int(idx.numel())
    names = list(columns)
    src, n = {}, None
    for nm in names:
        t = columns[nm]
        code = _DT_CODE.get(str(t.dtype).replace("torch.", ""))
        if code is None:
            raise TypeError(f"column {nm}: {t.dtype} is not int8, int16, int32 or float32")
        if t.device != dev or t.dim() != 1:
            raise ValueError(f"column {nm}: a 1-d tensor on {dev} is needed")
        if n is None:
            n = int(t.numel())
        elif int(t.numel()) != n:
            raise ValueError(f"column {nm} has {int(t.numel())} rows, others {n}")
        src[nm] = (t.contiguous(), code)
    out = {nm: torch.empty(m, dtype=src[nm][0].dtype, device=dev) for nm in names}
    for c0 in range(0, len(names), MAX_GATHER_COLS):
        part = names[c0:c0 + MAX_GATHER_COLS]
        k = len(part)
        ps, pd_, codes = (ctypes.c_void_p * k)(), (ctypes.c_void_p * k)(), (ctypes.c_int * k)()
        for i, nm in enumerate(part):
            ps[i] = _lib.ptr(src[nm][0]) if n else None
            pd_[i] = _lib.ptr(out[nm]) if m else None
            codes[i] = src[nm][1]
        _lib.check(lib.ottohip_gather_rows(ctx.h, ps, pd_, codes, k, _lib.ptr(idx) if m else None, m, n or 0,
                                           _lib.stream_handle(stream)))
    return out


def _target_columns(features: dict, targets) -> dict:
    for t in targets:
        if t not in config.TYPES:
            raise ValueError(f"target {t!r} is not one of {config.TYPES}")
        if f"target_{t}" not in features:
            raise ValueError(f"the frame has no target_{t} column (a FeatureJob built without labels?)")
    return {t: features[f"target_{t}"] for t in targets}


def downsample(features: dict, cand_off, targets=config.TYPES,
               keep_ratio_neg_to_pos: float = config.DOWNSAMPLE_RATIO_NEG_TO_POS,
               max_neg_per_session: float = config.DOWNSAMPLE_MAX_NEG_PER_SESSION, seed: int = 42, ctx=None,
               stream=None) -> dict:
    """model/downsample_retrieved.py:39-58 on the device. features: {column: device tensor}, a frame as
    FeatureJob.range returns it (sorted by session, 'session' holding session ids, target columns 0 or 1);
    cand_off [S + 1]: the sessions' row offsets, relative to cand_off[0]. -> {target: {column: device tensor}}:
    every column of the frame except the other two target columns, rows in the output order of the module's
    docstring."""
    ctx = ctx or _lib.context()
    targets = list(targets)
    plans = plan(cand_off, features["session"], features["aid_next"], _target_columns(features, targets),
                 keep_ratio_neg_to_pos, max_neg_per_session, seed, ctx, stream)
    out = {}
    for t in targets:
        drop = {f"target_{o}" for o in config.TYPES if o != t}
        out[t] = gather_rows({n: c for n, c in features.items() if n not in drop}, plans[t][1], ctx, stream)
    return out


def _host_frame(parts: list, columns: list):
    import pandas as pd
    cols = {}
    for nm, dt in columns:
        v = [p[nm].cpu().numpy() for p in parts]
        cols[nm] = np.concatenate(v).astype(dt, copy=False) if v else np.zeros(0, dt)
    return pd.DataFrame(cols)


def downsample_job(job, targets=config.TYPES, keep_ratio_neg_to_pos: float = config.DOWNSAMPLE_RATIO_NEG_TO_POS,
                   max_neg_per_session: float = config.DOWNSAMPLE_MAX_NEG_PER_SESSION, seed: int = 42,
                   memory_budget: int = 2 << 30) -> dict:
    """Downsamples a candidates.FeatureJob built with labels a session range at a time (the range sizing of
    rank_job): the feature columns of a range live only on the device, the kept rows are copied to the host and
    concatenated. The draw does not depend on the ranges. -> {target: DataFrame} in the retrieved schema minus the
    other two target columns."""
    if job.labels is None:
        raise ValueError("downsample_job needs a FeatureJob built with labels (no target columns otherwise)")
    targets = list(targets)
    table, coff, S = job.table, job.cand_off_host, job.n_sessions
    max_rows = max(1, int(memory_budget) // sum(dt.itemsize for _, dt in table))
    parts = {t: [] for t in targets}
    lo = 0
    while lo < S:
        hi = int(np.searchsorted(coff, coff[lo] + max_rows, side="right")) - 1
        hi = min(max(hi, lo + 1), S)
        f = job.range(lo, hi)
        if int(coff[hi] - coff[lo]) > 0:
            d = downsample(f, job.cand_off[lo:hi + 1], targets, keep_ratio_neg_to_pos, max_neg_per_session, seed,
                           job.sources.ctx)
            for t in targets:
                parts[t].append(d[t])
        lo = hi
    cols = lambda t: [(n, dt) for n, dt in table if n not in {f"target_{o}" for o in config.TYPES if o != t}]
    return {t: _host_frame(parts[t], cols(t)) for t in targets}


def write_downsampled(df, file_out: str):
    """One target's downsampled file (model/downsample_retrieved.py:61-62): the frame's columns and dtypes as is."""
    import pyarrow as pa
    import pyarrow.parquet as pq
    os.makedirs(os.path.dirname(os.path.abspath(file_out)), exist_ok=True)
    pq.write_table(pa.table({n: pa.array(df[n].to_numpy()) for n in df.columns}), file_out)


def retrieve_and_downsample(df_sessions_aids_full, aid_pairs_co_events: dict, df_knns_w2vec_all, df_knns_w2vec_1_2,
                            df_session_cl, df_pop_cl1, df_pop_cl50, df_aid_embeddings, df_session_embeddings,
                            df_labels, dir_out: str | None = None, name: str = "downsampled",
                            targets=config.TYPES, keep_ratio_neg_to_pos: float = config.DOWNSAMPLE_RATIO_NEG_TO_POS,
                            max_neg_per_session: float = config.DOWNSAMPLE_MAX_NEG_PER_SESSION, seed: int = 42,
                            n_items: int | None = None, memory_budget: int = 2 << 30) -> dict:
    """retrieve_and_gen_feats followed by model/downsample_retrieved.py without the retrieved file in between: the
    arguments of candidates.retrieve_and_gen_feats (df_labels is required: it makes the target columns). Returns
    {target: DataFrame}; with dir_out also writes dir_out/{target}/{name}.parquet."""
    from .candidates import FeatureJob
    if df_labels is None:
        raise ValueError("retrieve_and_downsample needs df_labels")
    job = FeatureJob(df_sessions_aids_full, aid_pairs_co_events, df_knns_w2vec_all, df_knns_w2vec_1_2, df_session_cl,
                     df_pop_cl1, df_pop_cl50, df_aid_embeddings, df_session_embeddings, df_labels, n_items)
    try:
        out = downsample_job(job, targets, keep_ratio_neg_to_pos, max_neg_per_session, seed, memory_budget)
    finally:
        job.free()
    if dir_out is not None:
        for t, df in out.items():
            write_downsampled(df, os.path.join(dir_out, t, f"{name}.parquet"))
    return out


def frame_stats(df, target: str, n_rows_in: int) -> dict:
    """The figures model/downsample_retrieved.py:64-70 logs for one written file."""
    n_ses = int(df["session"].nunique()) if len(df) else 0
    return {"target": target, "rows": int(len(df)), "rows_in": int(n_rows_in),
            "avg_nr_candidates_per_session": (len(df) / n_ses) if n_ses else 0.0,
            "avg_nr_pos_per_session": (float(df[f"target_{target}"].sum()) / n_ses) if n_ses else 0.0}


def downsample_files(dir_retrieved: str, dir_out: str, targets=config.TYPES,
                     keep_ratio_neg_to_pos: float = config.DOWNSAMPLE_RATIO_NEG_TO_POS,
                     max_neg_per_session: float = config.DOWNSAMPLE_MAX_NEG_PER_SESSION, seed: int = 42,
                     ctx=None) -> list:
    """The __main__ of model/downsample_retrieved.py: every *.parquet of dir_retrieved (files of
    retrieve_and_gen_feats, sorted by session) downsampled per target and written to {dir_out}/{target}/{basename}.
    A file's columns are uploaded once and the three targets selected in one pass. Returns per file and target
    {file, path, target, rows, rows_in, avg_nr_candidates_per_session, avg_nr_pos_per_session}."""
    import pyarrow.parquet as pq
    import torch
    ctx = ctx or _lib.context()
    dev = torch.device("cuda", ctx.device)
    targets = list(targets)
    stats = []
    for path in sorted(glob.glob(os.path.join(dir_retrieved, "*.parquet"))):
        tab = pq.read_table(path)
        host = {n: np.array(tab[n].to_numpy()) for n in tab.column_names}  # writable copies
        ses = host["session"]
        starts = np.flatnonzero(np.r_[True, ses[1:] != ses[:-1]]) if len(ses) else np.zeros(0, np.int64)
        off = np.r_[starts, len(ses)].astype(np.int64)
        feats = {n: torch.from_numpy(v).to(dev) for n, v in host.items()}
        d = downsample(feats, torch.from_numpy(off).to(dev), targets, keep_ratio_neg_to_pos, max_neg_per_session,
                       seed, ctx)
        for t in targets:
            df = _host_frame([d[t]], [(n, host[n].dtype) for n in d[t]])
            out = os.path.join(dir_out, t, os.path.basename(path))
            write_downsampled(df, out)
            stats.append({"file": os.path.basename(path), "path": out, **frame_stats(df, t, len(ses))})
    return stats


def load_data_for_lgbm(source, target: str, feats: list | None = None):
    """load_data_for_lgbm_standard of model/train_lgbm_rankers.py:38-60, host only: source a parquet file, a
    directory pattern or a list of files (read in the given order) -> (X, y, group_counts, feats). target is the
    label column ('target_clicks', or 'clicks' for short); feats defaults to every column that is not one of
    session, aid_next, the three targets and rank_total_cl1 (:39); group_counts are the run lengths of session in
    file order, the group sizes a LightGBM ranker takes."""
    import pandas as pd
    paths = [source] if isinstance(source, str) else list(source)
    files = []
    for p in paths:
        files += sorted(glob.glob(p)) if any(ch in p for ch in "*?[") else [p]
    if not files:
        raise ValueError(f"no file in {source!r}")
    df = pd.concat([pd.read_parquet(f) for f in files], ignore_index=True) if len(files) > 1 else pd.read_parquet(files[0])
    if feats is None:
        feats = [c for c in df.columns if c not in NON_FEATS]
    col = target if target in df.columns else f"target_{target}"
    X = df[list(feats)].values
    y = df[col].to_numpy()
    ses = df["session"].to_numpy()
    starts = np.flatnonzero(np.r_[True, ses[1:] != ses[:-1]]) if len(ses) else np.zeros(0, np.int64)
    group_counts = np.diff(np.r_[starts, len(ses)]).astype(np.int64)
    return X, y, group_counts, list(feats)
