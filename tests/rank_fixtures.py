"""Inputs shared by tests/test_rank_cpu.py and tests/test_rank_gpu.py (test infrastructure): a writer of random
boosters in LightGBM's text format, column generators with the edge values of each dtype planted, threshold
samplers that draw from the data's own values and their neighbours, and the known answer of
tests/golden/kat_rank.json."""
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
KAT_JSON = os.path.join(HERE, "golden", "kat_rank.json")
KAT_MODEL = os.path.join(HERE, "golden", "kat_rank.booster.lgbm")
DTYPES = [np.dtype(np.int8), np.dtype(np.int16), np.dtype(np.int32), np.dtype(np.float32)]
F32_EDGES = np.array([np.nan, 0.0, -0.0, 1e-36, -1e-36, 1e-35, -1e-35, np.inf, -np.inf, 1e-45, -1e-45, 1e-40, -1e-40,
                      np.finfo(np.float32).max, np.finfo(np.float32).min, np.finfo(np.float32).tiny,
                      -np.finfo(np.float32).tiny, 1.0, -1.0, 0.5], np.float32)
# the float32 neighbours of +-1e-35f, the edge of the zero band
F32_EDGES = np.concatenate([F32_EDGES, np.nextafter(np.float32(1e-35), np.float32([np.inf, -np.inf])),
                            np.nextafter(np.float32(-1e-35), np.float32([np.inf, -np.inf]))]).astype(np.float32)


def _num(x) -> str:
    return format(float(x), ".17g")


def random_tree(rng, num_leaves: int, n_features: int, threshold_of, leaf_values=None) -> dict:
    """a tree grown as LightGBM numbers it: splitting leaf L at step i makes internal node i, whose left child is
    leaf L and right child the new leaf i + 1. threshold_of(feature) -> float; leaf_values: choices or None."""
    t = {"num_leaves": num_leaves}
    leaf = (rng.normal(size=num_leaves) if leaf_values is None else rng.choice(leaf_values, size=num_leaves))
    t["leaf_value"] = np.asarray(leaf, np.float64)
    if num_leaves == 1:
        return t
    ni = num_leaves - 1
    left, right = np.zeros(ni, np.int64), np.zeros(ni, np.int64)
    parent = {0: -1}
    for i in range(ni):
        L = int(rng.integers(0, i + 1))
        p = parent[L]
        if p >= 0:
            if left[p] == ~L:
                left[p] = i
            else:
                right[p] = i
        left[i], right[i] = ~L, ~(i + 1)
        parent[L] = parent[i + 1] = i
    feat = rng.integers(0, n_features, ni)
    t.update(split_feature=feat, threshold=np.array([threshold_of(int(f)) for f in feat], np.float64),
             decision_type=(rng.integers(0, 2, ni) * 2) | (rng.integers(0, 3, ni) << 2), left_child=left,
             right_child=right)
    return t


def booster_text(trees: list, feature_names: list, version: str = "v3", objective: str = "lambdarank",
                 head_extra: tuple = (), tree_extra: dict | None = None) -> str:
    """LightGBM's text model of the trees; tree_extra {tree index: [extra lines]}"""
    out = ["tree", f"version={version}", "num_class=1", "num_tree_per_iteration=1", "label_index=0",
           f"max_feature_idx={len(feature_names) - 1}", f"objective={objective}",
           "feature_names=" + " ".join(feature_names), "feature_infos=" + " ".join(["[0:1]"] * len(feature_names)),
           *head_extra, "tree_sizes=" + " ".join(["0"] * len(trees)), ""]
    for i, t in enumerate(trees):
        out += [f"Tree={i}", f"num_leaves={t['num_leaves']}", "num_cat=0"]
        if t["num_leaves"] > 1:
            ni = t["num_leaves"] - 1
            out += ["split_feature=" + " ".join(str(int(x)) for x in t["split_feature"]),
                    "split_gain=" + " ".join(["1"] * ni),
                    "threshold=" + " ".join(_num(x) for x in t["threshold"]),
                    "decision_type=" + " ".join(str(int(x)) for x in t["decision_type"]),
                    "left_child=" + " ".join(str(int(x)) for x in t["left_child"]),
                    "right_child=" + " ".join(str(int(x)) for x in t["right_child"])]
        out += ["leaf_value=" + " ".join(_num(x) for x in t["leaf_value"])]
        if t["num_leaves"] > 1:
            out += ["leaf_weight=" + " ".join(["1"] * t["num_leaves"]), "leaf_count=" + " ".join(["1"] * t["num_leaves"]),
                    "internal_value=" + " ".join(["0"] * ni), "internal_weight=" + " ".join(["0"] * ni),
                    "internal_count=" + " ".join(["2"] * ni)]
            if version == "v4":
                out += ["is_linear=0"]
            out += ["shrinkage=0.25"]
        out += (tree_extra or {}).get(i, [])
        out += ["", ""]
    out += ["end of trees", "", "feature_importances:", "parameters:", "[objective: lambdarank]", "end of parameters", ""]
    return "\n".join(out)


def edge_values(dtype) -> np.ndarray:
    dtype = np.dtype(dtype)
    if dtype.kind == "f":
        return F32_EDGES.copy()
    i = np.iinfo(dtype)
    return np.array([i.min, i.min + 1, -1, 0, 1, i.max - 1, i.max], dtype)


def random_column(rng, dtype, n: int) -> np.ndarray:
    """n values of dtype: few distinct values (so thresholds hit them), the dtype's edge values planted"""
    dtype = np.dtype(dtype)
    if dtype.kind == "f":
        pool = np.concatenate([rng.normal(size=24).astype(np.float32), F32_EDGES])
    else:
        i = np.iinfo(dtype)
        pool = np.concatenate([rng.integers(max(i.min, -1000), min(i.max, 1000), 24).astype(dtype), edge_values(dtype)])
    col = rng.choice(pool, size=n).astype(dtype)
    e = edge_values(dtype)
    if n >= len(e):
        col[rng.choice(n, size=len(e), replace=False)] = e
    return col


def thresholds_near(values, rng, n: int) -> np.ndarray:
    """n finite float64 thresholds from the column's values: the value, its float64 and float32 neighbours,
    and value +- 0.5"""
    v = np.asarray(values).astype(np.float64)
    v = v[np.isfinite(v)]
    if not len(v):
        return np.zeros(n)
    x = rng.choice(v, size=n)
    kind = rng.integers(0, 7, n)
    with np.errstate(over="ignore"):
        f32up = np.nextafter(x.astype(np.float32), np.float32(np.inf)).astype(np.float64)
        f32dn = np.nextafter(x.astype(np.float32), np.float32(-np.inf)).astype(np.float64)
    out = np.select([kind == 0, kind == 1, kind == 2, kind == 3, kind == 4, kind == 5],
                    [x, np.nextafter(x, np.inf), np.nextafter(x, -np.inf), f32up, f32dn, x + 0.5], x - 0.5)
    return np.where(np.isfinite(out), out, x)


def random_forest_text(rng, n_trees: int, max_leaves: int, columns: dict, names=None, leaf_values=None,
                       exact_leaves: bool = False) -> str:
    """a random booster over the columns {name: array}; thresholds from the data (thresholds_near)"""
    names = list(columns) if names is None else list(names)
    pools = {i: thresholds_near(columns[n], rng, 64) for i, n in enumerate(names)}
    pick = lambda f: float(rng.choice(pools[f]))
    trees = [random_tree(rng, max_leaves if exact_leaves else int(rng.integers(1, max_leaves + 1)), len(names), pick,
                         leaf_values) for _ in range(n_trees)]
    return booster_text(trees, names)


def kat():
    """(columns {name: typed array}, session, aid_next, expected dict) of tests/golden/kat_rank.json"""
    k = json.load(open(KAT_JSON))
    cols = {}
    for name, spec in k["columns"].items():
        v = [np.nan if x is None else x for x in spec["values"]]
        cols[name] = np.array(v, np.dtype(spec["dtype"]))
    return cols, np.array(k["session"], np.int32), np.array(k["aid_next"], np.int32), k
