"""CPU oracle (TEST INFRASTRUCTURE ONLY) for the ranker feature columns of retrieve_and_gen_feats
(model/retrieve.py:138-232 with all 20 columns, :293-403, :522-602, :604-657), restated on pandas.

polars is not available here and the reference pins no version; its API use (with_column,
pl.min([...]), rank(reverse=)) dates it before 0.17. The semantics below are DECISIONS, parity unpinned:

  Nulls     arithmetic and comparisons propagate null; aggregates skip nulls; an aggregate over a group
            with no non-null value is null -- INCLUDING sum (polars before 0.20). One switch:
            SUM_OF_ALL_NULL_IS_NULL.
  Self      (aid == aid_next) * col is 0 on a non-self row with a non-null col and null where col is null:
            the slf_* minima are 0 whenever another aid also proposes the candidate and that aid's col is
            non-null; the slf_max_ts* are maxima over {0 (non-self rows), the self row's value}.
  Means     mean is f64(sum of the non-null values) / f64(their count); '/' between integers is f64
            division; casts to integer truncate toward zero; round(0) rounds half away from zero; the
            operation order of the source is kept (a / b * 100). A weighted mean whose weight sum is 0
            (no R1 table produces a zero count) is null.
  Products  products and sums of integer columns are taken in 64 bits; polars' Int32 wrap
            (count_pop * count above 2^31) is NOT reproduced (as oracle/retrieve.py for the source flags).
  Overflow  a finished value outside its column's dtype raises OverflowError (polars' strict cast raises).
  Fills     src_* nulls -> 0, ts_order_aid nulls -> 999, every other null -> -1 (:592-602); cos 0, eucl -1.
  Ties      ordinal ranks break ties by aid ascending; the final (session, ts_order_aid) sort by aid_next
            (oracle/retrieve.py's deterministic choices).
  Order     columns follow the reference's construction; rows (session, ts_order_aid, aid_next).
"""
from __future__ import annotations

import numpy as np
import pandas as pd

import retrieve as R

SUM_OF_ALL_NULL_IS_NULL = True
RULES = R.RULES
W2V = ["all", "1_2"]
TYPES = ["clicks", "carts", "orders"]
CL50_RANKS = ["rank_clicks_cl50", "rank_carts_cl50", "rank_orders_cl50", "rank_clicks_7d_cl50",
              "rank_carts_7d_cl50", "rank_orders_7d_cl50"]
CL1_RANKS = ["rank_clicks_cl1", "rank_carts_cl1", "rank_orders_cl1"]
_LIM = {"int8": (-128, 127), "int16": (-32768, 32767), "int32": (-2 ** 31, 2 ** 31 - 1)}


def _i(s):
    return pd.Series(s).astype("Int64")


def _f(s):
    """nullable integer Series -> float64 numpy, NaN for null"""
    return pd.Series(s).astype("Int64").to_numpy(dtype="float64", na_value=np.nan)


def _trunc(x, index):
    """f64 -> integer, truncating toward zero; NaN -> null"""
    x = np.asarray(x, np.float64)
    out = pd.Series(pd.array([None] * len(x), dtype="Int64"), index=index)
    ok = ~np.isnan(x)
    out[ok] = np.trunc(x[ok]).astype(np.int64)
    return out


def _round(x):
    """round(0), half away from zero"""
    return np.sign(x) * np.floor(np.abs(x) + 0.5)


def _sum(g, col):
    return g[col].sum(min_count=1 if SUM_OF_ALL_NULL_IS_NULL else 0)


def session_aid_pairs_full(ev):
    """model/retrieve.py:138-232, all 20 columns (+ session), after the keep filter; nullable Int64."""
    sa = R.session_aid_pairs_unique(ev)  # the filtered rows with counts, last ts and the ordinal ranks
    g = ev.groupby("session")
    last = ev.groupby(["session", "aid"])["ts"].max().reset_index()
    ses = pd.DataFrame({"n_distinct": g["aid"].nunique(),  # :175 max of ts_order_aid BEFORE the filter
                        "mx": last.groupby("session")["ts"].max(),  # :190-191 over max_ts_aid, before the filter
                        "mn": last.groupby("session")["ts"].min()}).reset_index()
    sa = sa.merge(ses, on="session", how="left")
    for c in list(sa.columns):
        sa[c] = _i(sa[c])
    sa["ts_order_aid_rel"] = _trunc(_round(_f(sa["ts_order_aid"]) / _f(sa["n_distinct"]) * 100), sa.index)
    den = np.maximum(_f(sa["mx"] - sa["mn"]), 3600.0)
    sa["ts_aid_rel_pos_in_session"] = _trunc(_round(_f(sa["mx"] - sa["max_ts_aid"]) / den * 100), sa.index)
    # :183-185 Kleene or, then fill_null(0)
    a = ((sa["n_aid_carts"] > 0) & (sa["n_aid_orders"] == 0)).to_numpy(dtype=bool, na_value=False)
    both = (sa["max_ts_aid_carts"].notna() & sa["max_ts_aid_orders"].notna()).to_numpy()
    b = both & (_f(sa["max_ts_aid_carts"]) > _f(sa["max_ts_aid_orders"]))
    sa["left_in_cart"] = _i((a | b).astype(np.int64))
    cols = ["session", "aid", "n_aid", "n_aid_clicks", "n_aid_carts", "n_aid_orders", "rank_by_n_aid",
            "rank_by_n_aid_carts", "rank_by_n_aid_orders", "max_ts_aid", "max_ts_aid_clicks", "max_ts_aid_carts",
            "max_ts_aid_orders", "ts_aid_rel_pos_in_session", "ts_order_aid", "ts_order_aid_rel",
            "ts_order_aid_clicks", "ts_order_aid_carts", "ts_order_aid_orders", "left_in_cart"]
    return sa[cols]


def session_stats(ev):
    """compute_session_stats (:115-135)"""
    g = ev.groupby("session")
    st = pd.DataFrame({"n_events_session": g["aid"].size(), "n_aids_session": g["aid"].nunique()})
    for t, nm in enumerate(TYPES):
        st[f"n_{nm}_session"] = (ev["type"] == t).astype(np.int64).groupby(ev["session"]).sum()
    st["min_ts_session"] = g["ts"].min()
    st["max_ts_session"] = g["ts"].max()
    st["duration_session"] = st["max_ts_session"] - st["min_ts_session"]
    st["only_orders_session"] = ((st["n_clicks_session"] == 0) & (st["n_carts_session"] == 0)
                                 & (st["n_orders_session"] > 0)).astype(np.int64)
    st = st.reset_index()
    for c in st.columns:
        st[c] = _i(st[c])
    return st


def kept_pairs(sa, r1, knn_all, knn_12):
    """get_all_aid_pairs (:244-290), the left joins of every table (:480-488) and the trim (:490-516):
    rows (session, aid, aid_next) with the 20 session-aid columns and every source's value columns."""
    aids = sa["aid"].unique()
    lst = [pd.DataFrame({"aid": aids, "aid_next": aids})]
    for n in RULES:
        lst.append(r1[n][["aid", "aid_next"]][r1[n]["aid"].isin(aids)])
    lst += [knn_all[["aid", "aid_next"]], knn_12[["aid", "aid_next"]]]
    pairs = pd.concat(lst).astype(np.int64).drop_duplicates()
    df = sa.merge(_nullable(pairs), on="aid", how="left")
    for n in RULES:
        df = df.merge(_nullable(r1[n]), on=["aid", "aid_next"], how="left")
    df = df.merge(_nullable(knn_all), on=["aid", "aid_next"], how="left")
    df = df.merge(_nullable(knn_12), on=["aid", "aid_next"], how="left")

    def hmin(cols):  # horizontal min, nulls skipped (oracle/retrieve.py R5)
        return np.nanmin(np.stack([_f(df[c]) for c in cols] + [np.full(len(df), np.inf)]), axis=0)
    best_order = hmin(["rank_by_n_aid", "ts_order_aid", "ts_order_aid_clicks", "ts_order_aid_carts",
                       "ts_order_aid_orders"])
    th = np.maximum(20 - (20 - 3) / (20 - 1) * (best_order - 1), 3)
    best_co = hmin([f"{n}_rank" for n in RULES])
    best_w2v = hmin(["rank_w2vec_all", "rank_w2vec_1_2"])
    keep = (df["aid"] == df["aid_next"]).to_numpy(dtype=bool, na_value=False) | (best_co <= th) | (best_w2v <= th)
    return df[keep].reset_index(drop=True)


def _nullable(df):
    return pd.DataFrame({c: _i(df[c].to_numpy()) for c in df.columns})


def keep_sessions_aids_next(df):
    """:293-403. Returns the aggregated frame, columns in the reference's order (nullable Int64)."""
    d = df.copy()
    slf = _i((d["aid"] == d["aid_next"]).astype("Int64"))
    d["_self"] = slf
    tmp = {}
    self_cols = ["n_aid", "n_aid_clicks", "n_aid_carts", "n_aid_orders", "rank_by_n_aid", "rank_by_n_aid_carts",
                 "rank_by_n_aid_orders", "max_ts_aid", "max_ts_aid_clicks", "max_ts_aid_carts", "max_ts_aid_orders",
                 "ts_aid_rel_pos_in_session", "ts_order_aid", "ts_order_aid_rel", "ts_order_aid_clicks",
                 "ts_order_aid_carts", "ts_order_aid_orders", "left_in_cart"]
    for c in self_cols:
        tmp[f"_s_{c}"] = slf * d[c]
    for t in TYPES:
        tmp[f"_pos_{t}"] = _i((d[f"n_aid_{t}"] > 0).astype("Int64"))
    for n in RULES:
        for feat in ["count_pop", "perc_pop", "rank", "count_rel"]:
            tmp[f"_w_{n}_{feat}"] = d[f"{n}_{feat}"] * d[f"{n}_count"]
    for w in W2V:
        tmp[f"_pos_w_{w}"] = (d[f"rank_w2vec_{w}"] > 0).astype("Int64")
    d = pd.concat([d, pd.DataFrame(tmp, index=d.index)], axis=1)
    g = d.groupby(["session", "aid_next"], sort=True)
    idx = g.size().index
    o = {}

    def mean(col):
        return _trunc(_f(g[col].sum(min_count=1)) / _f(g[col].count().where(g[col].count() > 0)), idx)

    # feats_self (:309-334)
    o["aid_next_is_aid"] = _sum(g, "_self")
    for a, c in (("slf_n", "n_aid"), ("slf_n_clicks", "n_aid_clicks"), ("slf_n_carts", "n_aid_carts"),
                 ("slf_n_orders", "n_aid_orders")):
        o[a] = _sum(g, f"_s_{c}")
    for a, c in (("slf_rank_by_n", "rank_by_n_aid"), ("slf_rank_by_n_carts", "rank_by_n_aid_carts"),
                 ("slf_rank_by_n_orders", "rank_by_n_aid_orders")):
        o[a] = g[f"_s_{c}"].min()
    for a, c in (("slf_max_ts", "max_ts_aid"), ("slf_max_ts_clicks", "max_ts_aid_clicks"),
                 ("slf_max_ts_carts", "max_ts_aid_carts"), ("slf_max_ts_orders", "max_ts_aid_orders")):
        o[a] = g[f"_s_{c}"].max()
    for a, c in (("slf_ts_rel_pos_in_session", "ts_aid_rel_pos_in_session"), ("slf_ts_order", "ts_order_aid"),
                 ("slf_ts_order_rel", "ts_order_aid_rel"), ("slf_ts_order_clicks", "ts_order_aid_clicks"),
                 ("slf_ts_order_carts", "ts_order_aid_carts"), ("slf_ts_order_orders", "ts_order_aid_orders")):
        o[a] = g[f"_s_{c}"].min()
    o["slf_left_in_cart"] = _sum(g, "_s_left_in_cart")
    # aggs_events_session (:337-364)
    o["n_uniq_aid"] = g.size()
    for t in TYPES:
        o[f"n_uniq_aid_{t}"] = _sum(g, f"_pos_{t}")
    for c in ("n_aid", "n_aid_clicks", "n_aid_carts", "n_aid_orders"):
        o[c] = _sum(g, c)
    for c in ("max_ts_aid", "max_ts_aid_clicks", "max_ts_aid_carts", "max_ts_aid_orders"):
        o[c] = g[c].max()
    o["mean_max_ts_aid"] = mean("max_ts_aid")
    o["mean_max_ts_aid_orders"] = mean("max_ts_aid_orders")
    for c in ("ts_order_aid", "ts_order_aid_rel", "ts_order_aid_clicks", "ts_order_aid_carts", "ts_order_aid_orders"):
        o[c] = g[c].min()
    o["ts_aid_rel_pos_in_session"] = mean("ts_aid_rel_pos_in_session")
    o["rank_by_n_aid"] = g["rank_by_n_aid"].min()
    # aggs_counts_co_events (:367-376)
    for n in RULES:
        cs = _sum(g, f"{n}_count")
        o[f"{n}_count"] = cs
        den = _f(cs.where(cs != 0))
        for feat in ["count_pop", "perc_pop", "rank", "count_rel"]:
            o[f"{n}_{feat}"] = _trunc(_f(_sum(g, f"_w_{n}_{feat}")) / den, idx)
    # aggs_w2vec (:379-389)
    for w in W2V:
        o[f"n_w2vec_{w}"] = _sum(g, f"_pos_w_{w}")
        o[f"dist_w2vec_{w}"] = mean(f"dist_w2vec_{w}")
        o[f"rank_w2vec_{w}"] = mean(f"rank_w2vec_{w}")
        o[f"best_rank_w2vec_{w}"] = g[f"rank_w2vec_{w}"].min()
    out = pd.DataFrame({k: _i(pd.Series(v, index=idx)) for k, v in o.items()}, index=idx).reset_index()
    out["session"], out["aid_next"] = _i(out["session"]), _i(out["aid_next"])
    return out


def _emb(df, key):
    cols = [c for c in df.columns if c.startswith("dim_")]
    return df[key].to_numpy().astype(np.int64), df[cols].to_numpy().astype(np.float64)


def retrieve_and_gen_feats(df_sessions_aids_full, aid_pairs_co_events, df_knns_w2vec_all, df_knns_w2vec_1_2,
                           df_session_cl, df_pop_cl1, df_pop_cl50, df_aid_embeddings, df_session_embeddings,
                           df_labels):
    """The frame model/retrieve.py:422-657 writes (pandas; integer columns in the reference's dtypes,
    cos / eucl float64 here -- compared at rtol 1e-5)."""
    ev = df_sessions_aids_full
    sa = session_aid_pairs_full(ev)
    df = keep_sessions_aids_next(kept_pairs(sa, aid_pairs_co_events, df_knns_w2vec_all, df_knns_w2vec_1_2))
    df = df.merge(session_stats(ev), on="session", how="left")  # :522-523
    # :526-551
    mx, mn = df["max_ts_session"], df["min_ts_session"]
    new = {}
    for a, c in (("since_ts_aid", "max_ts_aid"), ("since_ts_aid_clicks", "max_ts_aid_clicks"),
                 ("since_ts_aid_carts", "max_ts_aid_carts"), ("since_ts_aid_orders", "max_ts_aid_orders"),
                 ("slf_since_ts", "slf_max_ts"), ("slf_since_ts_clicks", "slf_max_ts_clicks"),
                 ("slf_since_ts_carts", "slf_max_ts_carts"), ("slf_since_ts_orders", "slf_max_ts_orders")):
        new[a] = mx - df[c]
    new["since_session_start_ts_aid"] = df["max_ts_aid"] - mn
    new["since_session_start_ts_aid_orders"] = df["max_ts_aid_orders"] - mn
    for a, c in (("rel_pos_max_ts_aid_in_session", "max_ts_aid"),
                 ("rel_pos_mean_max_ts_aid_in_session", "mean_max_ts_aid"),
                 ("rel_pos_mean_max_ts_aid_orders_in_session", "mean_max_ts_aid_orders")):
        new[a] = _trunc(_f(df[c] - mn) / _f(mx - mn + 1) * 100, df.index)
    for k, v in new.items():
        df[k] = v
    df = df.drop(columns=["min_ts_session", "max_ts_session", "max_ts_aid", "max_ts_aid_clicks", "max_ts_aid_carts",
                          "max_ts_aid_orders", "mean_max_ts_aid", "mean_max_ts_aid_orders", "slf_max_ts",
                          "slf_max_ts_clicks", "slf_max_ts_carts", "slf_max_ts_orders"])
    # :558-569 (64-bit products; null > 0 is null)
    pos = lambda s: _i((s > 0).astype("Int64"))
    df["src_any"] = _i(np.ones(len(df), np.int64))
    df["src_self"] = pos(df["aid_next_is_aid"])
    for n in RULES:
        df[f"src_{n}"] = pos(df[f"n_aid_{TYPES[R.RULE_TYPE[n]]}"] * df[f"{n}_count"])
    for w in W2V:
        df[f"src_w2vec_{w}"] = pos(df[f"n_w2vec_{w}"])
    df = df.drop(columns=["aid_next_is_aid"])
    # :571-585
    cl = _nullable(df_session_cl[["session", "cl50"]].dropna())
    df = df.merge(cl, on="session", how="left")
    pop = _nullable(df_pop_cl50[["cl50", "aid"] + CL50_RANKS]).rename(columns={"aid": "aid_next"})
    sc = df[["session", "cl50"]].drop_duplicates().dropna()
    sc = sc.merge(pop, on="cl50", how="inner")
    sc["src_pop_cl50"] = _i(np.ones(len(sc), np.int64))
    sc = sc[sc[CL50_RANKS].min(axis=1) <= 20]
    df = df.merge(sc, on=["session", "cl50", "aid_next"], how="outer").drop(columns=["cl50"])
    # :588-590
    c1 = _nullable(df_pop_cl1[["aid"] + CL1_RANKS]).rename(columns={"aid": "aid_next"})
    df = df.merge(c1, on="aid_next", how="left")
    # :592-602
    df["src_any"] = _i(np.ones(len(df), np.int64))
    for c in df.columns:
        if "src_" in c:
            df[c] = df[c].fillna(0)
    df["ts_order_aid"] = df["ts_order_aid"].fillna(999)
    df = df.fillna(-1)
    # :604-625
    sk, sv = _emb(df_session_embeddings, "session")
    ak, av = _emb(df_aid_embeddings, "aid")
    s_row = pd.Series(np.arange(len(sk)), index=sk).reindex(df["session"].to_numpy().astype(np.int64)).to_numpy()
    a_row = pd.Series(np.arange(len(ak)), index=ak).reindex(df["aid_next"].to_numpy().astype(np.int64)).to_numpy()
    ok = ~np.isnan(s_row) & ~np.isnan(a_row)
    cos = np.zeros(len(df))
    eu = np.full(len(df), -1.0)
    if ok.any():
        x, y = sv[s_row[ok].astype(np.int64)], av[a_row[ok].astype(np.int64)]
        cos[ok] = (x * y).sum(1) / (np.sqrt((x * x).sum(1)) * np.sqrt((y * y).sum(1)))
        eu[ok] = np.sqrt(((x - y) ** 2).sum(1))
    df["cos_sim_ses_aid"], df["eucl_dist_ses_aid"] = cos, eu
    # :630-644
    if df_labels is not None:
        for t, nm in enumerate(TYPES):
            lab = df_labels[df_labels["type"] == t][["session", "aid"]].drop_duplicates()
            lab = _nullable(lab).rename(columns={"aid": "aid_next"})
            lab[f"target_{nm}"] = _i(np.ones(len(lab), np.int64))
            df = df.merge(lab, on=["session", "aid_next"], how="left")
            df[f"target_{nm}"] = df[f"target_{nm}"].fillna(0)
    # dtypes (strict casts) and the final order (:651)
    dt = column_dtypes(df_labels is not None)
    assert list(df.columns) == list(dt), (list(df.columns), list(dt))
    out = {}
    for c, t in dt.items():
        if t == "float32":
            out[c] = df[c].to_numpy().astype(np.float64)
            continue
        v = df[c].to_numpy(dtype=np.int64)
        lo, hi = _LIM[t]
        if len(v) and (v.min() < lo or v.max() > hi):
            raise OverflowError(f"{c}: a value does not fit {t}")
        out[c] = v.astype(t)
    out = pd.DataFrame(out)
    return out.sort_values(["session", "ts_order_aid", "aid_next"], kind="stable").reset_index(drop=True)


def column_dtypes(with_targets: bool = True) -> dict:
    """name -> dtype of the written file, in the reference's column order, from the casts of the source
    (session, aid, ts: int32 and type: int8 as etl/jsonl_to_parquet.py writes them; a difference of two
    Int32 columns is Int32; the embeddings and so cos / eucl are float32)."""
    d = {"session": "int32", "aid_next": "int32"}
    for c in ("slf_n", "slf_n_clicks", "slf_n_carts", "slf_n_orders", "slf_rank_by_n", "slf_rank_by_n_carts",
              "slf_rank_by_n_orders", "slf_ts_rel_pos_in_session", "slf_ts_order", "slf_ts_order_rel",
              "slf_ts_order_clicks", "slf_ts_order_carts", "slf_ts_order_orders"):
        d[c] = "int16"
    d["slf_left_in_cart"] = "int8"
    for c in ("n_uniq_aid", "n_uniq_aid_clicks", "n_uniq_aid_carts", "n_uniq_aid_orders", "n_aid", "n_aid_clicks",
              "n_aid_carts", "n_aid_orders", "ts_order_aid", "ts_order_aid_rel", "ts_order_aid_clicks",
              "ts_order_aid_carts", "ts_order_aid_orders", "ts_aid_rel_pos_in_session", "rank_by_n_aid"):
        d[c] = "int16"
    for n in RULES:
        d[f"{n}_count"] = "int32"
        for feat in ["count_pop", "perc_pop", "rank", "count_rel"]:
            d[f"{n}_{feat}"] = "int16"
    for w in W2V:
        d[f"n_w2vec_{w}"] = "int16"
        d[f"dist_w2vec_{w}"] = "int32"
        d[f"rank_w2vec_{w}"] = "int16"
        d[f"best_rank_w2vec_{w}"] = "int16"
    for c in ("n_events_session", "n_aids_session", "n_clicks_session", "n_carts_session", "n_orders_session"):
        d[c] = "int16"
    d["duration_session"] = "int32"
    d["only_orders_session"] = "int8"
    for c in ("since_ts_aid", "since_ts_aid_clicks", "since_ts_aid_carts", "since_ts_aid_orders", "slf_since_ts",
              "slf_since_ts_clicks", "slf_since_ts_carts", "slf_since_ts_orders", "since_session_start_ts_aid",
              "since_session_start_ts_aid_orders"):
        d[c] = "int32"
    for c in ("rel_pos_max_ts_aid_in_session", "rel_pos_mean_max_ts_aid_in_session",
              "rel_pos_mean_max_ts_aid_orders_in_session"):
        d[c] = "int8"
    for c in ["src_any"] + R.SRC_NAMES[:8]:
        d[c] = "int8"
    for c in CL50_RANKS:
        d[c] = "int16"
    d["src_pop_cl50"] = "int8"
    for c in CL1_RANKS:
        d[c] = "int16"
    d["cos_sim_ses_aid"] = "float32"
    d["eucl_dist_ses_aid"] = "float32"
    if with_targets:
        for t in TYPES:
            d[f"target_{t}"] = "int8"
    return d
