"""CPU oracle (TEST INFRASTRUCTURE ONLY) for the rank stage (model/rank.py, model/submit.py), restated on numpy.

LightGBM and polars are not available here, so this restates the documented model format and decision rule;
parity with LightGBM itself is unpinned. The semantics below are the ones the product is held to, bit for bit.

Model file   LightGBM's text booster (Booster.save_model). A header block of key=value lines (tree, version,
             num_class, num_tree_per_iteration, max_feature_idx, objective, feature_names, feature_infos), then
             'Tree=i' blocks until 'end of trees'; the rest is ignored. A tree block holds num_leaves, num_cat,
             split_feature, threshold, decision_type, left_child, right_child, leaf_value (a one-leaf tree: only
             num_leaves=1, num_cat=0, leaf_value); other keys are ignored.
Decision     at an internal node, on the feature value v as a double:
               default_left = decision_type & 2;  missing = (decision_type >> 2) & 3  (0 none, 1 zero, 2 NaN)
               v NaN and missing != 2            -> v = 0.0
               missing == 1 and |v| <= 1e-35f    -> the default side   (the float32 constant, taken as a double)
               missing == 2 and v NaN            -> the default side
               otherwise                         -> left iff v <= threshold
             a child c >= 0 is internal node c, c < 0 is leaf ~c.
Raw score    0.0 + leaf(tree 0) + leaf(tree 1) + ... in float64, in tree order; all trees, no transform
             (objectives lambdarank, rank_xendcg, regression).
Rank         per session, pred_rank is 1-based by pred_score descending; scores compare as doubles (-0.0 == 0.0);
             ties go to the earlier row of the frame (a DECISION: polars' ordinal reverse rank is unpinned). Kept:
             pred_rank <= keep_top_k, sorted by (session, pred_rank); columns session:int32, aid_next:int32,
             pred_score:float64, pred_rank:int16 (model/rank.py:52-59).
Features     the typed columns convert exactly to double.
Submission   model/submit.py:32-56: '{session}_{target}', aid_next joined by spaces in pred_rank order, rows
             sorted by session_type as strings.
"""
from __future__ import annotations

import numpy as np
import pandas as pd

K_ZERO = float(np.float32(1e-35))
TARGETS = ["clicks", "carts", "orders"]


def parse(text: str) -> dict:
    """{'feature_names': [...], 'trees': [{num_leaves, split_feature, threshold, decision_type, left_child,
    right_child, leaf_value}]} -- a minimal reader of its own (no validation)."""
    head, trees, cur = {}, [], None
    for ln in text.splitlines():
        ln = ln.strip()
        if ln == "end of trees":
            break
        if ln.startswith("Tree="):
            cur = {}
            trees.append(cur)
        elif "=" in ln:
            k, v = ln.split("=", 1)
            (head if cur is None else cur)[k] = v
    out = []
    for t in trees:
        nl = int(t["num_leaves"])
        d = {"num_leaves": nl, "leaf_value": np.array(t["leaf_value"].split(), np.float64)}
        if nl > 1:
            d["split_feature"] = np.array(t["split_feature"].split(), np.int64)
            d["threshold"] = np.array(t["threshold"].split(), np.float64)
            for k in ("decision_type", "left_child", "right_child"):
                d[k] = np.array(t[k].split(), np.int64)
        out.append(d)
    return {"feature_names": head["feature_names"].split(), "trees": out}


def goes_left(v, threshold: float, decision_type: int):
    """the decision rule on float64 values v (vectorised)"""
    v = np.array(v, np.float64)
    default_left = bool(decision_type & 2)
    missing = (decision_type >> 2) & 3
    if missing != 2:
        v[np.isnan(v)] = 0.0
    if missing == 1:
        dflt = np.abs(v) <= K_ZERO
    elif missing == 2:
        dflt = np.isnan(v)
    else:
        dflt = np.zeros(len(v), bool)
    with np.errstate(invalid="ignore"):
        return np.where(dflt, default_left, v <= threshold)


def predict(model: dict, cols: dict) -> np.ndarray:
    """raw scores (float64) of the rows of cols {feature name: array}"""
    names = model["feature_names"]
    n = len(next(iter(cols.values())))
    X = {}
    score = np.zeros(n, np.float64)
    for t in model["trees"]:
        if t["num_leaves"] == 1:
            score = score + t["leaf_value"][0]
            continue
        node = np.zeros(n, np.int64)
        while True:
            act = np.flatnonzero(node >= 0)
            if not len(act):
                break
            for i in np.unique(node[act]):
                rows = act[node[act] == i]
                f = names[t["split_feature"][i]]
                if f not in X:
                    X[f] = np.asarray(cols[f]).astype(np.float64)
                left = goes_left(X[f][rows], t["threshold"][i], int(t["decision_type"][i]))
                node[rows] = np.where(left, t["left_child"][i], t["right_child"][i])
        score = score + t["leaf_value"][~node]
    return score


def rank(session, aid_next, score, keep_top_k: int) -> pd.DataFrame:
    """model/rank.py:52-57 with the tie rule above; sessions ascending"""
    session = np.asarray(session)
    score = np.asarray(score, np.float64) + 0.0  # -0.0 -> 0.0
    pos = np.arange(len(score))
    order = np.lexsort((pos, -score, session))
    s = session[order]
    start = np.r_[True, s[1:] != s[:-1]] if len(s) else np.zeros(0, bool)
    first = np.maximum.accumulate(np.where(start, np.arange(len(s)), 0)) if len(s) else np.zeros(0, np.int64)
    r = np.arange(len(s)) - first + 1
    keep = r <= keep_top_k
    o = order[keep]
    return pd.DataFrame({"session": session[o].astype(np.int32), "aid_next": np.asarray(aid_next)[o].astype(np.int32),
                         "pred_score": np.asarray(score)[o], "pred_rank": r[keep].astype(np.int16)})


def submission(ranked: dict) -> pd.DataFrame:
    rows = []
    for target in TARGETS:
        if target not in ranked:
            continue
        d = ranked[target]
        ses, aid, rk = d["session"].to_numpy(), d["aid_next"].to_numpy(), d["pred_rank"].to_numpy()
        for s in np.unique(ses):
            m = ses == s
            rows.append((f"{int(s)}_{target}", " ".join(str(int(a)) for a in aid[m][np.argsort(rk[m], kind="stable")])))
    rows.sort(key=lambda x: x[0])
    return pd.DataFrame(rows, columns=["session_type", "labels"])
