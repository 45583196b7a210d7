"""The train stage on MI355X: LambdaRank GBDT rankers saved as LightGBM text models (model/train_lgbm_rankers.py).

A deterministic, histogram-based, leaf-wise GBDT with the LambdaRank objective in LightGBM's shape, defined by
DESIGN.md (train) and not by LightGBM's code: lightgbm is not needed and parity with it is not pinned. The hot
stages run in libottohip.so (csrc/train.hip): bin lookup, the pairwise gradients per session, the quantiser, the
integer gradient histograms of a leaf's rows, the split scan, the stable row partition, the tree walk that updates
the scores, and NDCG, and the boosting loop over them behind an opaque trainer handle (the feature draw and the leaf
choice from one small read per split on the host side of the library). This module finds the bin boundaries once per
fit and writes the model text that rank.parse_booster / rank.Ranker read.

Every exp and log2 the objective needs is a float64 table built here with numpy and handed to the kernels as data;
all other float64 arithmetic is + - * / in a fixed order and every histogram is an integer sum, so two fits of the
same input give the same bytes.
"""
from __future__ import annotations

import ctypes
import glob
import math
import os

import numpy as np

from . import _lib
from . import config
from .rank import _DT_CODE, Forest, parse_booster

MASK64 = (1 << 64) - 1
N_DISC = 10000          # discounts, and the rows of a session at most (LightGBM's query limit)
N_SIG = 1 << 20         # entries of the sigmoid table
N_LOG2 = 4096           # intervals of the log2 table over the mantissa [0.5, 1)
MAX_LABEL = 30
HIST_BINS = 256
ACCEPTED_AND_UNUSED = ("subsample", "metric", "importance_type", "verbose", "n_jobs", "random_state")


# ---------------------------------------------------------------- host pieces
def mix(z: int) -> int:
    """splitmix64's finaliser with its increment (the draw of csrc/downsample.hip), uint64 wrapping"""
    z = (z + 0x9E3779B97F4A7C15) & MASK64
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & MASK64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & MASK64
    z ^= z >> 31
    return z


def feature_draw(valid, colsample_bytree: float, seed: int, tree: int) -> list:
    """The features of tree `tree`: of the valid feature indices the k = max(1, floor(n_valid * colsample + 0.5))
    with the smallest mix(mix(seed) ^ (tree << 32 | feature)), returned ascending. No valid feature: []."""
    valid = [int(f) for f in valid]
    if not valid:
        return []
    k = min(len(valid), max(1, int(math.floor(len(valid) * float(colsample_bytree) + 0.5))))
    sm = mix(int(seed) & MASK64)
    keyed = sorted((mix(sm ^ (((int(tree) << 32) | f) & MASK64)), f) for f in valid)
    return sorted(f for _, f in keyed[:k])


def _distinct(col):
    """(distinct values ascending as float64 with -0.0 folded into 0.0, their counts); NaN raises ValueError"""
    try:
        import torch
    except ImportError:  # host-only use
        torch = None
    if torch is not None and isinstance(col, torch.Tensor):
        if col.is_floating_point() and bool(torch.isnan(col).any()):
            raise ValueError("NaN in a training column")
        u, c = torch.unique(col, return_counts=True)
        u, c = u.cpu().numpy(), c.cpu().numpy()
    else:
        col = np.asarray(col)
        if col.dtype.kind == "f" and np.isnan(col).any():
            raise ValueError("NaN in a training column")
        u, c = np.unique(col, return_counts=True)
    v = u.astype(np.float64) + 0.0
    c = c.astype(np.int64)
    if len(v) > 1:
        first = np.flatnonzero(np.r_[True, v[1:] != v[:-1]])
        c = np.add.reduceat(c, first)
        v = v[first]
    return v, c


def find_bins(col, max_bin: int = 255) -> dict:
    """The bins of one column (numpy array or tensor): {bounds: float64 [n_bins - 1], n_bins, min, max}. One bin per
    distinct value when there are at most max_bin of them; else value i goes to floor(first_rank_i * max_bin / n)
    (first_rank_i = rows with a smaller value), the ids compacted. bounds[b] is the float64 midpoint of the largest
    value of bin b and the smallest of bin b + 1, the lower value where the midpoint is not strictly below the upper
    one, and -DBL_MAX where that is -inf (a threshold has to be finite): value <= bounds[b] <=> bin <= b."""
    if not 2 <= int(max_bin) <= HIST_BINS:
        raise ValueError(f"max_bin {max_bin} outside [2, {HIST_BINS}]")
    v, c = _distinct(col)
    if len(v) == 0:
        return {"bounds": np.zeros(0), "n_bins": 0, "min": 0.0, "max": 0.0}
    if len(v) <= max_bin:
        ids = np.arange(len(v), dtype=np.int64)
    else:
        first_rank = np.cumsum(c) - c
        raw = (first_rank * int(max_bin)) // int(c.sum())
        ids = np.cumsum(np.r_[0, (raw[1:] != raw[:-1]).astype(np.int64)])
    ends = np.flatnonzero(ids[1:] != ids[:-1])
    lo, hi = v[ends], v[ends + 1]
    with np.errstate(invalid="ignore", over="ignore"):
        mid = (lo + hi) / 2.0
        b = np.where(mid < hi, mid, lo)
    b = np.where(b == -np.inf, -np.finfo(np.float64).max, b)
    return {"bounds": b.astype(np.float64), "n_bins": int(ids[-1]) + 1, "min": float(v[0]), "max": float(v[-1])}


def bin_values(values, bounds) -> np.ndarray:
    """host restatement of the bin lookup: the number of bounds below each value"""
    return np.searchsorted(np.asarray(bounds, np.float64), np.asarray(values).astype(np.float64), side="left")


def label_gain(n: int = MAX_LABEL + 1) -> np.ndarray:
    return np.array([float((1 << l) - 1) for l in range(n)], np.float64)


def build_tables(sigmoid: float = 1.0) -> dict:
    """The float64 tables the kernels read: disc[r] = 1 / log2(2 + r); sig: LightGBM's sigmoid table (2^20 entries
    over [-50 / sigmoid / 2, 50 / sigmoid / 2], entry i = 1 / (1 + exp(sigmoid * d_i)), d_i = i / factor + min);
    log2t[i] = log2(0.5 + i / 8192)."""
    sigmoid = float(sigmoid)
    if not sigmoid > 0:
        raise ValueError("sigmoid must be > 0")
    mn = -50.0 / sigmoid / 2.0
    mx = -mn
    factor = N_SIG / (mx - mn)
    d = np.arange(N_SIG, dtype=np.float64) / factor + mn
    with np.errstate(over="ignore"):
        sig = 1.0 / (1.0 + np.exp(d * sigmoid))
    return {"gain": label_gain(), "disc": 1.0 / np.log2(2.0 + np.arange(N_DISC, dtype=np.float64)), "sig": sig,
            "log2t": np.log2(0.5 + np.arange(N_LOG2 + 1, dtype=np.float64) / 8192.0), "sig_min": mn, "sig_max": mx,
            "sig_factor": factor, "sigma": sigmoid}


def log2_table_form(x: float, log2t) -> float:
    """LOG2(x) for x >= 1 as the kernel computes it: frexp, then linear interpolation of log2t on the mantissa"""
    m, e = math.frexp(float(x))
    t = (m - 0.5) * 8192.0
    i = math.floor(t)
    f = t - i
    return (float(e) + float(log2t[i])) + f * (float(log2t[i + 1]) - float(log2t[i]))


def inv_max_dcg(labels, off, k: int, gain, disc) -> np.ndarray:
    """per session 1 / (sum over the first k positions of the labels sorted descending of gain * disc, added in
    position order), 0 where that sum is 0"""
    labels = np.asarray(labels).astype(np.int64)
    off = np.asarray(off, np.int64) - int(off[0]) if len(off) else np.zeros(1, np.int64)
    S = len(off) - 1
    n = np.diff(off)
    ses = np.repeat(np.arange(S), n)
    cnt = np.bincount(ses * (MAX_LABEL + 1) + labels, minlength=S * (MAX_LABEL + 1)).reshape(S, MAX_LABEL + 1)
    cum = np.cumsum(cnt[:, ::-1], axis=1)  # cum[s, j]: rows with label >= MAX_LABEL - j
    acc = np.zeros(S, np.float64)
    for p in range(int(k)):
        lab = MAX_LABEL - (cum <= p).sum(axis=1)
        live = p < n
        acc = np.where(live, acc + gain[np.where(live, lab, 0)] * disc[p], acc)
    with np.errstate(divide="ignore"):
        return np.where(acc > 0, 1.0 / acc, 0.0)


def resolve_params(params: dict | None = None) -> dict:
    """config.PARAMS_LGBM and config.PARAMS_LGBM_DEFAULTS overridden by params, under LightGBM's sklearn names; what
    this trainer does not do raises ValueError."""
    p = dict(config.PARAMS_LGBM_DEFAULTS)
    p.update(config.PARAMS_LGBM)
    alias = {"feature_fraction": "colsample_bytree", "min_data_in_leaf": "min_child_samples", "reg_lambda": "lambda_l2",
             "reg_alpha": "lambda_l1", "bagging_freq": "subsample_freq", "bagging_fraction": "subsample",
             "num_iterations": "n_estimators", "min_child_weight": "min_sum_hessian_in_leaf",
             "categorical_feature": "categorical_feature", "boosting": "boosting_type"}
    for k, v in (params or {}).items():
        p[alias.get(k, k)] = v
    known = set(config.PARAMS_LGBM_DEFAULTS) | set(config.PARAMS_LGBM) | {"categorical_feature", "eval_every"} | \
        set(ACCEPTED_AND_UNUSED)
    unknown = sorted(set(p) - known)
    if unknown:
        raise ValueError(f"unknown parameters {unknown}")
    if p.get("boosting_type", "gbdt") != "gbdt":
        raise ValueError("only boosting_type='gbdt' is trained")
    if p.get("objective", "lambdarank") != "lambdarank":
        raise ValueError("only objective='lambdarank' is trained")
    if p.get("subsample_freq", 0):
        raise ValueError("bagging (a non-zero subsample_freq) is not trained")
    if p.get("lambda_l1", 0):
        raise ValueError("lambda_l1 is not supported")
    cat = p.get("categorical_feature")
    if cat is not None and not (isinstance(cat, str) and cat in ("", "auto")) and len(cat):
        raise ValueError("categorical features are not supported")
    if not 2 <= int(p["max_bin"]) <= HIST_BINS:
        raise ValueError(f"max_bin outside [2, {HIST_BINS}]")
    if int(p["num_leaves"]) < 2 or int(p["n_estimators"]) < 0 or int(p["lambdarank_truncation_level"]) < 1:
        raise ValueError("num_leaves >= 2, n_estimators >= 0 and lambdarank_truncation_level >= 1 are needed")
    if not (0 < float(p["colsample_bytree"]) <= 1):
        raise ValueError("colsample_bytree outside (0, 1]")
    gain = p.get("label_gain")
    p["label_gain"] = label_gain() if gain is None else np.asarray(gain, np.float64)
    if len(p["label_gain"]) != MAX_LABEL + 1:
        raise ValueError(f"label_gain needs {MAX_LABEL + 1} entries")
    p.setdefault("eval_every", config.PARAMS_LGBM_FIT["verbose"])
    return p


# ---------------------------------------------------------------- stage wrappers
def lds_rows() -> int:
    """the gradient kernel's path switch (ottohip_train_lds_rows)"""
    return int(_lib.load().ottohip_train_lds_rows())


def _dev(ctx):
    import torch
    return torch.device("cuda", ctx.device)


class Tables:
    """The float64 tables on the device and the objective's parameters (ottohip_train_tables)."""

    def __init__(self, sigmoid: float = 1.0, truncation_level: int = 30, norm: bool = True, gain=None, ctx=None):
        import torch
        self.ctx = ctx or _lib.context()
        self.host = build_tables(sigmoid)
        if gain is not None:
            self.host["gain"] = np.asarray(gain, np.float64)
        self.truncation_level, self.norm = int(truncation_level), bool(norm)
        self.dev = {k: torch.from_numpy(v).to(_dev(self.ctx)) for k, v in self.host.items() if isinstance(v, np.ndarray)}

    def struct(self, inv_max) -> _lib.TrainTables:
        h = self.host
        return _lib.TrainTables(_lib.ptr(self.dev["gain"]), _lib.ptr(self.dev["disc"]), _lib.ptr(self.dev["sig"]),
                                _lib.ptr(self.dev["log2t"]), _lib.ptr(inv_max), N_SIG, h["sig_min"], h["sig_max"],
                                h["sig_factor"], h["sigma"], self.truncation_level, 1 if self.norm else 0)

    def inv_max_dcg(self, labels, off, k=None):
        """inv_max_dcg of a frame (host arrays) at k (default the truncation level) as a device tensor"""
        import torch
        v = inv_max_dcg(labels, off, self.truncation_level if k is None else k, self.host["gain"], self.host["disc"])
        return torch.from_numpy(v).to(_dev(self.ctx))


def _need(t, dtype: str, what: str, ndim: int = 1, like=None):
    """the stage wrappers hand raw pointers to the library: the tensor must be what the kernel reads"""
    import torch
    if not isinstance(t, torch.Tensor) or str(t.dtype) != f"torch.{dtype}" or t.dim() != ndim or not t.is_cuda or \
            not t.is_contiguous() or (like is not None and t.device != like.device):
        raise TypeError(f"{what}: a contiguous {ndim}-d {dtype} tensor on the device is needed, got "
                        f"{getattr(t, 'dtype', type(t))} {tuple(getattr(t, 'shape', ()))}")
    return t


def lambdarank_gradients(scores, labels, off, tables: Tables, inv_max=None, stream=None):
    """ottohip_train_gradients: float64 scores, int8 labels, int64 off [S + 1] (device) -> (g, h) float64 tensors"""
    import torch
    _need(scores, "float64", "scores"), _need(labels, "int8", "labels", like=scores), _need(off, "int64", "off", like=scores)
    if int(labels.numel()) != int(scores.numel()) or int(off.numel()) < 1:
        raise ValueError("scores and labels of one length and at least one offset are needed")
    n, S = int(scores.numel()), int(off.numel()) - 1
    if inv_max is None:
        inv_max = tables.inv_max_dcg(labels.cpu().numpy(), off.cpu().numpy())
    g = torch.empty(n, dtype=torch.float64, device=scores.device)
    h = torch.empty(n, dtype=torch.float64, device=scores.device)
    t = tables.struct(inv_max)
    _lib.check(_lib.load().ottohip_train_gradients(tables.ctx.h, _lib.ptr(scores), _lib.ptr(labels), _lib.ptr(off), S, n,
                                                   ctypes.byref(t), _lib.ptr(g), _lib.ptr(h), _lib.stream_handle(stream)))
    return g, h


def quantise(g, h, ctx=None, stream=None):
    """ottohip_train_quantise -> (gh int32 [n, 2], e_g, e_h, all_zero)"""
    import torch
    ctx = ctx or _lib.context()
    _need(g, "float64", "g"), _need(h, "float64", "h", like=g)
    if int(h.numel()) != int(g.numel()):
        raise ValueError("g and h of one length are needed")
    n = int(g.numel())
    gh = torch.empty((n, 2), dtype=torch.int32, device=g.device)
    eg, eh, z = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    _lib.check(_lib.load().ottohip_train_quantise(ctx.h, _lib.ptr(g), _lib.ptr(h), n, _lib.ptr(gh), ctypes.byref(eg),
                                                  ctypes.byref(eh), ctypes.byref(z), _lib.stream_handle(stream)))
    return gh, eg.value, eh.value, bool(z.value)


def histograms(bins, gh, rows, feats, max_blocks: int = 0, ctx=None, stream=None):
    """ottohip_train_histogram: bins uint8 [n, stride], gh int32 [n, 2], rows int32 [m], feats int32 [k] (device)
    -> int64 [k, 256, 3] = (sum q_g, sum q_h, count) per bin"""
    import torch
    ctx = ctx or _lib.context()
    _need(bins, "uint8", "bins", 2), _need(gh, "int32", "gh", 2, bins), _need(rows, "int32", "rows", like=bins)
    _need(feats, "int32", "feats", like=bins)
    if tuple(gh.shape) != (int(bins.shape[0]), 2):
        raise ValueError("gh holds one (q_g, q_h) pair per row of bins")
    k = int(feats.numel())
    hist = torch.empty((k, HIST_BINS, 3), dtype=torch.int64, device=bins.device)
    _lib.check(_lib.load().ottohip_train_histogram(ctx.h, _lib.ptr(bins), int(bins.shape[1]), int(bins.shape[0]),
                                                   _lib.ptr(gh), _lib.ptr(rows), int(rows.numel()), _lib.ptr(feats), k,
                                                   _lib.ptr(hist), int(max_blocks), _lib.stream_handle(stream)))
    return hist


def split_scan(hist, n_bins, e_g: int, e_h: int, min_child_samples: int, min_sum_hessian: float, lambda_l2: float,
               ctx=None, stream=None) -> list:
    """ottohip_train_split_scan on hist [m, k, 256, 3] -> per histogram and feature (gain, bin or -1, Qg left,
    Qh left, count left, Qg, Qh, count) as a host array [m, k] of records"""
    import torch
    ctx = ctx or _lib.context()
    _need(hist, "int64", "hist", 4), _need(n_bins, "int32", "n_bins", like=hist)
    if tuple(hist.shape[2:]) != (HIST_BINS, 3) or int(n_bins.numel()) != int(hist.shape[1]):
        raise ValueError(f"hist [m, k, {HIST_BINS}, 3] and n_bins [k] are needed")
    m, k = int(hist.shape[0]), int(hist.shape[1])
    rec = torch.empty((m * k, 8), dtype=torch.int64, device=hist.device)
    _lib.check(_lib.load().ottohip_train_split_scan(ctx.h, _lib.ptr(hist), m, k, _lib.ptr(n_bins), int(e_g), int(e_h),
                                                    int(min_child_samples), float(min_sum_hessian), float(lambda_l2),
                                                    _lib.ptr(rec), _lib.stream_handle(stream)))
    r = rec.cpu().numpy()
    gains = r[:, 0].copy().view(np.float64)
    return [[(float(gains[i * k + j]),) + tuple(int(x) for x in r[i * k + j, 1:]) for j in range(k)] for i in range(m)]


def partition(bins, feature: int, bin_: int, rows, ctx=None, stream=None):
    """ottohip_train_partition -> (rows_out, n_left): the rows with bin <= bin_ first, both sides in their order"""
    import torch
    ctx = ctx or _lib.context()
    _need(bins, "uint8", "bins", 2), _need(rows, "int32", "rows", like=bins)
    if not 0 <= int(feature) < int(bins.shape[1]):
        raise ValueError("feature outside the matrix")
    out = torch.empty_like(rows)
    nl = ctypes.c_int64()
    _lib.check(_lib.load().ottohip_train_partition(ctx.h, _lib.ptr(bins), int(bins.shape[1]), int(bins.shape[0]),
                                                   int(feature), int(bin_), _lib.ptr(rows), int(rows.numel()),
                                                   _lib.ptr(out), ctypes.byref(nl), _lib.stream_handle(stream)))
    return out, int(nl.value)


def apply_tree(bins, tree: dict, scores, ctx=None, stream=None):
    """ottohip_train_apply: scores += the tree's leaf values, in place"""
    import torch
    ctx = ctx or _lib.context()
    _need(bins, "uint8", "bins", 2), _need(scores, "float64", "scores", like=bins)
    if int(scores.numel()) != int(bins.shape[0]):
        raise ValueError("one score per row of bins is needed")
    dev = bins.device
    i32 = lambda k: torch.tensor(np.asarray(tree.get(k, []), np.int32), dtype=torch.int32, device=dev)
    sf, sb, lc, rc = i32("split_feature"), i32("split_bin"), i32("left_child"), i32("right_child")
    lv = torch.tensor(np.asarray(tree["leaf_value"], np.float64), dtype=torch.float64, device=dev)
    _lib.check(_lib.load().ottohip_train_apply(ctx.h, _lib.ptr(bins), int(bins.shape[1]), int(bins.shape[0]),
                                               _lib.ptr(sf), _lib.ptr(sb), _lib.ptr(lc), _lib.ptr(rc), _lib.ptr(lv),
                                               int(tree["num_leaves"]), _lib.ptr(scores), _lib.stream_handle(stream)))
    return scores


def ndcg_per_session(scores, labels, off, tables: Tables, inv_max_k, k: int = 20, stream=None):
    """ottohip_train_ndcg -> float64 [S] (device)"""
    import torch
    _need(scores, "float64", "scores"), _need(labels, "int8", "labels", like=scores), _need(off, "int64", "off", like=scores)
    _need(inv_max_k, "float64", "inv_max_k", like=scores)
    if int(labels.numel()) != int(scores.numel()) or int(inv_max_k.numel()) != int(off.numel()) - 1:
        raise ValueError("one label per score and one inv_max_dcg per session are needed")
    S = int(off.numel()) - 1
    out = torch.empty(S, dtype=torch.float64, device=scores.device)
    _lib.check(_lib.load().ottohip_train_ndcg(tables.ctx.h, _lib.ptr(scores), _lib.ptr(labels), _lib.ptr(off), S,
                                              int(scores.numel()), _lib.ptr(tables.dev["gain"]),
                                              _lib.ptr(tables.dev["disc"]), _lib.ptr(inv_max_k), int(k), _lib.ptr(out),
                                              _lib.stream_handle(stream)))
    return out


def mean_ndcg(per_session) -> float:
    """the exactly rounded mean (math.fsum): it does not depend on the order of the sessions' terms"""
    v = per_session.cpu().numpy().tolist()
    if not v:
        raise ValueError("NDCG of a frame without sessions")
    return math.fsum(v) / len(v)


# ---------------------------------------------------------------- binning of a frame
def _typed_columns(X, feats) -> dict:
    """{name: 1-d array or tensor}: X is that already, or a 2-d host matrix whose columns are typed int32 where all
    values are whole and fit, else float32 (a value neither holds raises ValueError)"""
    if isinstance(X, dict):
        return {n: X[n] for n in feats}
    M = np.asarray(X)
    if M.ndim != 2 or M.shape[1] != len(feats):
        raise ValueError("X: {name: column} or a matrix of len(feats) columns is needed")
    out = {}
    for j, n in enumerate(feats):
        c = M[:, j]
        if c.dtype in _DT_CODE:
            out[n] = np.ascontiguousarray(c)
            continue
        c64 = c.astype(np.float64)
        if np.isnan(c64).any():
            raise ValueError("NaN in a training column")
        i32 = np.iinfo(np.int32)
        fin = np.isfinite(c64)
        if fin.all() and (c64 == np.rint(c64)).all() and (c64 >= i32.min).all() and (c64 <= i32.max).all():
            out[n] = c64.astype(np.int32)
        else:
            f = c64.astype(np.float32)
            if not np.array_equal(f.astype(np.float64), c64):
                raise ValueError(f"column {n}: values that neither int32 nor float32 holds")
            out[n] = f
    return out


class Binner:
    """The bins of a training frame's features, found once per fit; bins further frames with the same boundaries."""

    def __init__(self, columns: dict, feats: list, max_bin: int = 255, ctx=None):
        import torch
        self.ctx = ctx or _lib.context()
        self.feats = list(feats)
        self.stride = max(4, (len(self.feats) + 3) // 4 * 4)  # a row's bin record is whole dwords
        self.info = [find_bins(self._tensor(columns[n]), max_bin) for n in self.feats]
        self.n_bins = [b["n_bins"] for b in self.info]
        self.valid = [f for f, nb in enumerate(self.n_bins) if nb > 1]
        self.bounds = [torch.from_numpy(b["bounds"]).to(_dev(self.ctx)) for b in self.info]

    def _tensor(self, c):
        import torch
        t = c if isinstance(c, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(c))
        if np.dtype(str(t.dtype).replace("torch.", "")) not in _DT_CODE:
            raise TypeError(f"a training column is {t.dtype}: int8, int16, int32 or float32 is needed")
        return t.to(_dev(self.ctx)).contiguous()

    def bin_frame(self, columns: dict, stream=None):
        """uint8 [n, stride] (device), row-major; columns past the features are 0"""
        import torch
        cols = [self._tensor(columns[n]) for n in self.feats]
        n = int(cols[0].numel()) if cols else 0
        bins = torch.zeros((n, self.stride), dtype=torch.uint8, device=_dev(self.ctx))
        for f, t in enumerate(cols):
            if int(t.numel()) != n:
                raise ValueError("columns of different lengths")
            if t.is_floating_point() and bool(torch.isnan(t).any()):
                raise ValueError("NaN in a training column")
            code = _DT_CODE[np.dtype(str(t.dtype).replace("torch.", ""))]
            _lib.check(_lib.load().ottohip_train_bin_column(self.ctx.h, _lib.ptr(t), code, n, _lib.ptr(self.bounds[f]),
                                                            int(self.bounds[f].numel()), _lib.ptr(bins), self.stride,
                                                            f, _lib.stream_handle(stream)))
        torch.cuda.current_stream().synchronize()  # the typed columns may be freed by the caller
        return bins


# ---------------------------------------------------------------- trainer
def _best(records: list, drawn: list):
    """the best split of a leaf from its features' records: larger gain, then the smaller feature index"""
    best = None
    for j, r in enumerate(records):
        if r[1] >= 0 and r[0] > 0.0 and (best is None or r[0] > best[0]):
            best = (r[0], drawn[j], r[1], r[2], r[3], r[4])
    return best


class Trainer:
    """The library's trainer handle (ottohip_trainer_create / _boost / _tree / _scores / _free) on a binned frame
    (device): bins uint8 [n, stride], labels int8 [n], off int64 [S + 1]; n_bins per feature of the matrix; params of
    resolve_params. The boosting loop, the feature draw and the leaf choice run inside the library; this class keeps
    the trees it reads back and scores a validation frame (bins, labels, off) along."""

    def __init__(self, bins, labels, off, n_bins: list, params: dict, ctx=None, valid=None, tables: Tables | None = None):
        import torch
        self.ctx = ctx or _lib.context()
        self.p = params
        self.bins, self.labels, self.off = bins, labels.contiguous(), off.to(torch.int64).contiguous()
        _need(self.bins, "uint8", "bins", 2), _need(self.labels, "int8", "labels", like=bins)
        if int(self.labels.numel()) != int(bins.shape[0]) or len(n_bins) > int(bins.shape[1]):
            raise ValueError("one label per row of bins and at most stride features are needed")
        self.n = int(bins.shape[0])
        if self.n >= 1 << 31:
            raise ValueError("a frame of 2^31 rows or more: row lists are int32")
        self.n_bins = [int(x) for x in n_bins]
        self.valid_feats = [f for f, nb in enumerate(self.n_bins) if nb > 1]
        self.tables = tables or Tables(params["sigmoid"], params["lambdarank_truncation_level"],
                                       params["lambdarank_norm"], params["label_gain"], self.ctx)
        lab_h, off_h = self.labels.cpu().numpy(), self.off.cpu().numpy()
        if len(lab_h) and (lab_h.min() < 0 or lab_h.max() > MAX_LABEL):
            raise ValueError(f"a label outside [0, {MAX_LABEL}]")
        self.eval_k = int(config.PARAMS_LGBM_FIT["eval_at"][0])
        self.inv_max = self.tables.inv_max_dcg(lab_h, off_h)
        self.inv_max_k = self.tables.inv_max_dcg(lab_h, off_h, self.eval_k)
        self.valid = None
        if valid is not None:
            vb, vl, vo = valid
            vo = vo.to(torch.int64).contiguous()
            self.valid = {"bins": vb, "labels": vl.contiguous(), "off": vo,
                          "inv_max_k": self.tables.inv_max_dcg(vl.cpu().numpy(), vo.cpu().numpy(), self.eval_k),
                          "scores": torch.zeros(int(vb.shape[0]), dtype=torch.float64, device=bins.device)}
        self.trees = []
        p = params
        self._tables = self.tables.struct(self.inv_max)  # kept alive with the tensors it points to
        self._params = _lib.TrainParams(int(p["num_leaves"]), int(p["max_depth"]), int(p["min_child_samples"]),
                                        float(p["min_sum_hessian_in_leaf"]), float(p["lambda_l2"]),
                                        float(p["learning_rate"]), float(p["colsample_bytree"]),
                                        int(p["seed"]) & MASK64)
        nb = (ctypes.c_int32 * max(len(self.n_bins), 1))(*self.n_bins)
        self.h = ctypes.c_void_p()
        _lib.check(_lib.load().ottohip_trainer_create(
            self.ctx.h, _lib.ptr(self.bins), int(bins.shape[1]), self.n, nb, len(self.n_bins), _lib.ptr(self.labels),
            _lib.ptr(self.off), int(self.off.numel()) - 1, ctypes.byref(self._tables), ctypes.byref(self._params),
            ctypes.byref(self.h)))

    def ndcg(self) -> dict:
        out = {"train": mean_ndcg(ndcg_per_session(self.scores, self.labels, self.off, self.tables, self.inv_max_k,
                                                   self.eval_k))}
        if self.valid is not None:
            v = self.valid
            out["valid"] = mean_ndcg(ndcg_per_session(v["scores"], v["labels"], v["off"], self.tables, v["inv_max_k"],
                                                      self.eval_k))
        return out

    def boost_one(self) -> bool:
        """One iteration (ottohip_trainer_boost); False (and no tree) when the gradients are all zero or the tree
        finds no split."""
        nl = ctypes.c_int()
        _lib.check(_lib.load().ottohip_trainer_boost(self.h, ctypes.byref(nl), _lib.stream_handle(None)))
        if nl.value == 0:
            return False
        tree = self.last_tree()
        self.trees.append(tree)
        if self.valid is not None:
            apply_tree(self.valid["bins"], tree, self.valid["scores"], self.ctx)
        return True

    def last_tree(self) -> dict:
        """ottohip_trainer_tree: the last tree as the model text writes it"""
        cap = int(self.p["num_leaves"])
        i32 = lambda n: np.zeros(n, np.int32)
        f64 = lambda n: np.zeros(n, np.float64)
        i64 = lambda n: np.zeros(n, np.int64)
        a = [i32(cap - 1), i32(cap - 1), f64(cap - 1), i32(cap - 1), i32(cap - 1), f64(cap - 1), f64(cap - 1),
             i64(cap - 1), f64(cap), f64(cap), i64(cap)]
        nl = ctypes.c_int()
        _lib.check(_lib.load().ottohip_trainer_tree(self.h, cap, *[x.ctypes.data for x in a], ctypes.byref(nl)))
        nl = nl.value
        keys = ("split_feature", "split_bin", "split_gain", "left_child", "right_child", "internal_value",
                "internal_weight", "internal_count", "leaf_value", "leaf_weight", "leaf_count")
        t = {k: x[:nl if k.startswith("leaf") else nl - 1].tolist() for k, x in zip(keys, a)}
        t["num_leaves"] = nl
        t["shrinkage"] = float(self.p["learning_rate"])
        return t

    @property
    def scores(self):
        """the training scores (ottohip_trainer_scores): a copy, float64 [n] on the device"""
        import torch
        out = torch.empty(self.n, dtype=torch.float64, device=self.bins.device)
        _lib.check(_lib.load().ottohip_trainer_scores(self.h, _lib.ptr(out), _lib.stream_handle(None)))
        return out

    def free(self):
        if getattr(self, "h", None):
            _lib.load().ottohip_trainer_free(self.h)
            self.h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


# ---------------------------------------------------------------- model text
def _num(x) -> str:
    return format(float(x), ".17g")


def tree_text(i: int, t: dict, thresholds: list) -> str:
    """one tree's block, 'Tree=i' up to and including its two closing blank lines"""
    j = lambda k, fmt=_num: " ".join(fmt(x) for x in t[k])
    integer = lambda x: str(int(x))
    out = [f"Tree={i}", f"num_leaves={t['num_leaves']}", "num_cat=0",
           "split_feature=" + j("split_feature", integer), "split_gain=" + j("split_gain"),
           "threshold=" + " ".join(_num(x) for x in thresholds),
           "decision_type=" + " ".join(["2"] * len(thresholds)),
           "left_child=" + j("left_child", integer), "right_child=" + j("right_child", integer),
           "leaf_value=" + j("leaf_value"), "leaf_weight=" + j("leaf_weight"), "leaf_count=" + j("leaf_count", integer),
           "internal_value=" + j("internal_value"), "internal_weight=" + j("internal_weight"),
           "internal_count=" + j("internal_count", integer), "is_linear=0", "shrinkage=" + _num(t["shrinkage"]), "", ""]
    return "\n".join(out) + "\n"


def gain_importance(trees: list, n_features: int) -> np.ndarray:
    imp = np.zeros(n_features, np.float64)
    for t in trees:
        for f, gn in zip(t["split_feature"], t["split_gain"]):
            imp[f] = imp[f] + gn
    return imp


def model_text(trees: list, feats: list, bin_info: list, params: dict) -> str:
    """LightGBM's text model (version v3): header, the trees with tree_sizes their blocks' byte lengths, the gain
    feature importances and the parameters"""
    infos = [f"[{_num(b['min'])}:{_num(b['max'])}]" if b["n_bins"] > 1 else "none" for b in bin_info]
    blocks = [tree_text(i, t, [bin_info[f]["bounds"][b] for f, b in zip(t["split_feature"], t["split_bin"])])
              for i, t in enumerate(trees)]
    head = ["tree", "version=v3", "num_class=1", "num_tree_per_iteration=1", "label_index=0",
            f"max_feature_idx={len(feats) - 1}", "objective=lambdarank", "feature_names=" + " ".join(feats),
            "feature_infos=" + " ".join(infos), "tree_sizes=" + " ".join(str(len(b.encode())) for b in blocks), "", ""]
    imp = gain_importance(trees, len(feats))
    order = sorted((f for f in range(len(feats)) if imp[f] > 0), key=lambda f: (-imp[f], f))
    tail = ["end of trees", "", "feature_importances:"] + [f"{feats[f]}={_num(imp[f])}" for f in order] + \
           ["", "parameters:"]
    for k in sorted(params):
        v = params[k]
        if isinstance(v, np.ndarray):
            v = ",".join(_num(x) for x in v)
        elif isinstance(v, bool):
            v = int(v)
        tail.append(f"[{k}: {v}]")
    tail += ["end of parameters", "", "pandas_categorical:null", ""]
    return "\n".join(head) + "".join(blocks) + "\n".join(tail)


# ---------------------------------------------------------------- the reference's functions
def _offsets(group) -> np.ndarray:
    return np.r_[0, np.cumsum(np.asarray(group, np.int64))].astype(np.int64)


def fit_lgbm(X_train, y_train, group_train, feats, X_valid=None, y_valid=None, group_valid=None, ctx=None, **params):
    """fit_lgbm of model/train_lgbm_rankers.py:110-129. X: {name: column} (device tensors or arrays of int8, int16,
    int32, float32) or a host matrix with feats naming its columns; y: labels in [0, 30]; group: the sessions' row
    counts in frame order. -> (model, history): model a rank.Forest (the parsed text) with .text, .trees,
    .bin_info, .params and .history; history {'iteration': [...], 'train': [...], 'valid': [...]} the NDCG@20 every
    eval_every iterations and after the last tree."""
    import torch
    p = resolve_params(params)
    ctx = ctx or _lib.context()
    dev = _dev(ctx)
    feats = list(feats)
    cols = _typed_columns(X_train, feats)
    binner = Binner(cols, feats, p["max_bin"], ctx)
    to_dev = lambda y: torch.as_tensor(np.asarray(y.cpu() if isinstance(y, torch.Tensor) else y)).to(torch.int8).to(dev)
    y_host = np.asarray(y_train.cpu() if isinstance(y_train, torch.Tensor) else y_train)
    if len(y_host) and (y_host.min() < 0 or y_host.max() > MAX_LABEL):
        raise ValueError(f"a label outside [0, {MAX_LABEL}]")
    off = _offsets(group_train)
    bins = binner.bin_frame(cols)
    if int(off[-1]) != int(bins.shape[0]) or len(y_host) != int(bins.shape[0]):
        raise ValueError("group counts, labels and columns disagree on the number of rows")
    if np.diff(off).max(initial=0) > N_DISC:
        raise _lib.OttoHipError(_lib.OTTOHIP_ELIMIT, f"a session has more than {N_DISC} rows")
    valid = None
    if X_valid is not None and y_valid is not None and group_valid is not None:
        voff = _offsets(group_valid)
        valid = (binner.bin_frame(_typed_columns(X_valid, feats)), to_dev(y_valid), torch.from_numpy(voff).to(dev))
    tr = Trainer(bins, to_dev(y_train), torch.from_numpy(off).to(dev), binner.n_bins, p, ctx, valid)
    hist = {"iteration": [], "train": []}
    if valid is not None:
        hist["valid"] = []

    def record(it):
        m = tr.ndcg()
        hist["iteration"].append(it)
        for k, v in m.items():
            hist[k].append(v)

    for it in range(1, int(p["n_estimators"]) + 1):
        if not tr.boost_one():
            break
        if it % int(p["eval_every"]) == 0:
            record(it)
    if not hist["iteration"] or hist["iteration"][-1] != len(tr.trees):
        record(len(tr.trees))
    text = model_text(tr.trees, feats, binner.info, p)
    model = parse_booster(text, columns=feats)
    model.text, model.trees, model.bin_info, model.params, model.history = text, tr.trees, binner.info, p, hist
    model.scores = tr.scores
    return model, hist


def save_lgbm(model, file_name: str) -> str:
    """save_lgbm (:147-159): writes {file_name}.booster.lgbm, the file rank.Ranker and rank.rank_files read"""
    path = f"{file_name}.booster.lgbm"
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "wb") as fh:
        fh.write(model.text.encode())
    return path


def feature_importance_lgbm(model, feature_names=None, importance_type: str = "gain"):
    """:132-144: the importances normalised to sum 1 and rounded to 4 places, sorted descending"""
    import pandas as pd
    names = list(feature_names) if feature_names is not None else list(model.feature_names)
    if importance_type == "gain":
        imp = gain_importance(model.trees, len(names))
    elif importance_type == "split":
        imp = np.bincount(np.concatenate([np.asarray(t["split_feature"], np.int64) for t in model.trees] or
                                         [np.zeros(0, np.int64)]), minlength=len(names)).astype(np.float64)
    else:
        raise ValueError("importance_type: 'gain' or 'split'")
    tot = imp.sum()
    imp = list(np.round(imp / tot, 4)) if tot > 0 else [0.0] * len(names)
    df = pd.DataFrame({"feature": names, "importance": imp})
    return df.sort_values(by=["importance"], ascending=False, kind="stable")


def split_files_to_train_valid(files, valid_frac, max_files_in_train=None, max_files_in_valid=None):
    """:184-204"""
    files = list(files)
    if valid_frac > 0:
        if not valid_frac < 1:
            raise ValueError("valid_frac must be < 1")
        if len(files) < 2:
            raise ValueError("need at least 2 files for train/test split")
        n_train = min(int((1 - valid_frac) * len(files)), len(files) - 1)
        files_train, files_valid = files[:n_train], files[n_train:]
    else:
        files_train, files_valid = files, None
    if max_files_in_train is not None:
        files_train = files_train[:int(max_files_in_train)]
    if max_files_in_valid is not None and files_valid is not None:
        files_valid = files_valid[:int(max_files_in_valid)]
    return files_train, files_valid


def train_files(dir_downsampled: str, dir_out: str, targets=("clicks", "carts", "orders"), valid_frac: float = 0,
                max_files_in_train=None, max_files_in_valid=None, ctx=None, **params) -> dict:
    """The __main__ of model/train_lgbm_rankers.py: per target the files {dir_downsampled}/{target}/*.parquet split
    into train and valid, read as a trainer reads them (downsample.load_data_for_lgbm), fitted and saved as
    {dir_out}/{target}.booster.lgbm. -> {target: {path, model, history}}"""
    from .downsample import load_data_for_lgbm
    out = {}
    for target in targets:
        files = sorted(glob.glob(os.path.join(dir_downsampled, target, "*.parquet")))
        if not files:
            raise ValueError(f"no file in {os.path.join(dir_downsampled, target)}")
        ftr, fva = split_files_to_train_valid(files, valid_frac, max_files_in_train, max_files_in_valid)
        X, y, group, feats = load_data_for_lgbm(ftr, f"target_{target}")
        Xv = yv = gv = None
        if fva is not None:
            Xv, yv, gv, _ = load_data_for_lgbm(fva, f"target_{target}", feats)
        model, hist = fit_lgbm(X, y, group, feats, Xv, yv, gv, ctx=ctx, **params)
        out[target] = {"path": save_lgbm(model, os.path.join(dir_out, target)), "model": model, "history": hist}
    return out
