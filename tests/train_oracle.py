"""numpy / plain-Python restatement of the train stage (train; test infrastructure). Written from the
stated semantics, not from the kernels: LightGBM's double loop over pairs for the gradients, per-leaf row lists and
histograms from scratch for the trees (no parent-minus-child), plain loops wherever the order of float64 additions
matters. The device must match it bit for bit."""
import math

import numpy as np

M64 = (1 << 64) - 1
N_SIG = 1 << 20
DEFAULTS = dict(n_estimators=150, learning_rate=0.25, max_depth=4, num_leaves=15, colsample_bytree=0.25,
                min_child_samples=20, seed=42, max_bin=255, min_sum_hessian_in_leaf=1e-3, lambda_l2=0.0, sigmoid=1.0,
                lambdarank_truncation_level=30, lambdarank_norm=True, eval_every=25, eval_at=20)


def mix(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9 & M64
    z = (z ^ (z >> 27)) * 0x94D049BB133111EB & M64
    return z ^ (z >> 31)


def feature_draw(valid, colsample, seed, tree):
    if len(valid) == 0:
        return []
    k = max(1, int(math.floor(len(valid) * colsample + 0.5)))
    ranked = sorted(valid, key=lambda f: (mix(mix(seed) ^ ((tree << 32) | f)), f))
    return sorted(ranked[:k])


# ---------------------------------------------------------------- bins
def find_bins(col, max_bin=255):
    """-> (bounds, n_bins, min, max)"""
    x = np.sort(np.asarray(col).astype(np.float64) + 0.0, kind="stable")
    if np.isnan(x).any():
        raise ValueError("NaN")
    n = len(x)
    vals, ranks = [], []  # distinct values and the number of rows below each
    for i in range(n):
        if i == 0 or x[i] != x[i - 1]:
            vals.append(float(x[i]))
            ranks.append(i)
    if len(vals) <= max_bin:
        ids = list(range(len(vals)))
    else:
        raw = [(r * max_bin) // n for r in ranks]
        ids, cur = [], -1
        for i, r in enumerate(raw):
            if i == 0 or r != raw[i - 1]:
                cur += 1
            ids.append(cur)
    bounds = []
    for i in range(len(vals) - 1):
        if ids[i + 1] != ids[i]:
            lo, hi = vals[i], vals[i + 1]
            with np.errstate(all="ignore"):
                mid = float((np.float64(lo) + np.float64(hi)) / np.float64(2.0))
            b = mid if mid < hi else lo
            if b == -math.inf:
                b = -1.7976931348623157e308
            bounds.append(b)
    return np.array(bounds, np.float64), (ids[-1] + 1 if ids else 0), vals[0], vals[-1]


def bin_column(col, bounds):
    v = np.asarray(col).astype(np.float64)
    return np.array([int(np.sum(bounds < x)) for x in v], np.int64) if len(bounds) < 8 else \
        np.searchsorted(bounds, v, side="left").astype(np.int64)


# ---------------------------------------------------------------- tables
def tables(sigma=1.0):
    mn = -50.0 / sigma / 2.0
    mx = -mn
    factor = N_SIG / (mx - mn)
    with np.errstate(over="ignore"):
        sig = 1.0 / (1.0 + np.exp((np.arange(N_SIG, dtype=np.float64) / factor + mn) * sigma))
    return dict(gain=[float(2 ** l - 1) for l in range(31)],
                disc=(1.0 / np.log2(2.0 + np.arange(10000, dtype=np.float64))).tolist(), sig=sig.tolist(), sig_min=mn,
                sig_max=mx, factor=factor, log2t=np.log2(0.5 + np.arange(4097, dtype=np.float64) / 8192.0).tolist(),
                sigma=float(sigma))


def sig_lookup(d, T):
    if d <= T["sig_min"]:
        return T["sig"][0]
    if d >= T["sig_max"]:
        return T["sig"][-1]
    return T["sig"][min(int((d - T["sig_min"]) * T["factor"]), N_SIG - 1)]


def log2_form(x, T):
    m, e = math.frexp(x)
    t = (m - 0.5) * 8192.0
    i = int(math.floor(t))
    f = t - i
    L = T["log2t"]
    return (e + L[i]) + f * (L[i + 1] - L[i])


def inv_max_dcg(labels, k, T):
    top = sorted((int(l) for l in labels), reverse=True)[:k]
    s = 0.0
    for p, l in enumerate(top):
        s += T["gain"][l] * T["disc"][p]
    return 1.0 / s if s > 0 else 0.0


def sorted_positions(scores):
    """row indices by score descending, stable in frame order, -0.0 == 0.0"""
    s = [float(v) for v in scores]
    return sorted(range(len(s)), key=lambda i: -s[i])


# ---------------------------------------------------------------- gradients
def session_gradients(scores, labels, inv, T, trunc=30, norm=True):
    n = len(scores)
    order = sorted_positions(scores)
    ss = [float(scores[i]) for i in order]
    sl = [int(labels[i]) for i in order]
    g, h, a = [0.0] * n, [0.0] * n, [0.0] * n
    sigma = T["sigma"]
    normalise = norm and n > 0 and ss[0] != ss[-1]
    for i in range(min(n, trunc)):
        for j in range(i + 1, n):
            if sl[i] == sl[j]:
                continue
            hi, lo = (i, j) if sl[i] > sl[j] else (j, i)
            d = ss[hi] - ss[lo]
            w = ((T["gain"][sl[hi]] - T["gain"][sl[lo]]) * abs(T["disc"][hi] - T["disc"][lo])) * inv
            if normalise:
                w = w / (0.01 + abs(d))
            p = sig_lookup(d, T)
            lam = p * (sigma * w)
            hes = (p * (1.0 - p)) * ((sigma * sigma) * w)
            g[hi] -= lam
            g[lo] += lam
            h[hi] += hes
            h[lo] += hes
            a[hi] += lam
            a[lo] += lam
    total = 0.0
    for r in range(n):
        total += a[r]
    if norm and total > 0:
        f = log2_form(1.0 + total, T) / total
        g = [x * f for x in g]
        h = [x * f for x in h]
    og, oh = np.zeros(n), np.zeros(n)
    for r, i in enumerate(order):
        og[i], oh[i] = g[r], h[r]
    return og, oh


def gradients(scores, labels, off, T, trunc=30, norm=True, inv=None):
    g, h = np.zeros(len(scores)), np.zeros(len(scores))
    for s in range(len(off) - 1):
        a, b = int(off[s]), int(off[s + 1])
        if b - a > 10000:
            raise OverflowError("session above 10000 rows")
        iv = inv[s] if inv is not None else inv_max_dcg(labels[a:b], trunc, T)
        g[a:b], h[a:b] = session_gradients(scores[a:b], labels[a:b], iv, T, trunc, norm)
    return g, h


def quantise(g, h):
    """-> (q_g, q_h int64, e_g, e_h, all_zero)"""
    mg = float(np.max(np.abs(g))) if len(g) else 0.0
    mh = float(np.max(np.abs(h))) if len(h) else 0.0
    eg, eh = math.frexp(mg)[1], math.frexp(mh)[1]
    return np.rint(np.ldexp(g, 15 - eg)).astype(np.int64), np.rint(np.ldexp(h, 15 - eh)).astype(np.int64), eg, eh, \
        mg == 0.0


# ---------------------------------------------------------------- trees
def histogram(bins, qg, qh, rows, feats):
    """bins [n, F] ints -> int64 [k, 256, 3]"""
    H = np.zeros((len(feats), 256, 3), np.int64)
    rows = np.asarray(rows, np.int64)
    for j, f in enumerate(feats):
        b = bins[rows, f]
        np.add.at(H[j, :, 0], b, qg[rows])
        np.add.at(H[j, :, 1], b, qh[rows])
        np.add.at(H[j, :, 2], b, 1)
    return H


def best_split_of_feature(H, n_bins, sg, sh, min_child, min_hess, l2):
    """-> (gain, bin, Qg left, Qh left, count left) or None; larger gain, then the smaller bin"""
    QG, QH, C = int(H[:, 0].sum()), int(H[:, 1].sum()), int(H[:, 2].sum())
    G, Hs = QG * sg, QH * sh
    best = None
    ql = hl = cl = 0
    for b in range(n_bins - 1):
        ql += int(H[b, 0]); hl += int(H[b, 1]); cl += int(H[b, 2])
        if cl < min_child or C - cl < min_child:
            continue
        GL, HL, GR, HR = ql * sg, hl * sh, (QG - ql) * sg, (QH - hl) * sh
        if HL < min_hess or HR < min_hess:
            continue
        with np.errstate(all="ignore"):
            gain = float((np.float64(GL * GL) / np.float64(HL + l2) + np.float64(GR * GR) / np.float64(HR + l2)) -
                         np.float64(G * G) / np.float64(Hs + l2))
        if gain > 0 and (best is None or gain > best[0]):
            best = (gain, b, ql, hl, cl)
    return best


def best_split(bins, qg, qh, rows, drawn, n_bins, sg, sh, P):
    """the leaf's best split over the drawn features: larger gain, then the smaller feature index"""
    H = histogram(bins, qg, qh, rows, drawn)
    best = None
    for j, f in enumerate(drawn):
        s = best_split_of_feature(H[j], n_bins[f], sg, sh, P["min_child_samples"], P["min_sum_hessian_in_leaf"],
                                  P["lambda_l2"])
        if s is not None and (best is None or s[0] > best[0]):
            best = (s[0], f) + s[1:]
    return best


def partition(bins, rows, f, b):
    left = [r for r in rows if bins[r, f] <= b]
    right = [r for r in rows if bins[r, f] > b]
    return left, right


def grow_tree(bins, qg, qh, eg, eh, drawn, n_bins, P):
    n = bins.shape[0]
    sg, sh = math.ldexp(1.0, eg - 15), math.ldexp(1.0, eh - 15)
    l2, lr = P["lambda_l2"], P["learning_rate"]

    def out(QG, QH):
        Hs = QH * sh + l2
        return 0.0 if Hs == 0.0 else (-(QG * sg) / Hs) * lr

    def leaf(rows, depth, parent):
        rows = list(rows)
        idx = np.asarray(rows, np.int64)
        return dict(rows=rows, depth=depth, parent=parent, QG=int(qg[idx].sum()), QH=int(qh[idx].sum()),
                    best=best_split(bins, qg, qh, rows, drawn, n_bins, sg, sh, P))

    leaves = [leaf(range(n), 0, -1)]
    T = dict(split_feature=[], split_bin=[], split_gain=[], left_child=[], right_child=[], internal_value=[],
             internal_weight=[], internal_count=[])
    for i in range(P["num_leaves"] - 1):
        cand = [(-lf["best"][0], L) for L, lf in enumerate(leaves)
                if lf["best"] is not None and (P["max_depth"] <= 0 or lf["depth"] < P["max_depth"])]
        if not cand:
            break
        L = min(cand)[1]
        lf = leaves[L]
        gain, f, b = lf["best"][:3]
        lrows, rrows = partition(bins, lf["rows"], f, b)
        if lf["parent"] >= 0:
            p = lf["parent"]
            if T["left_child"][p] == ~L:
                T["left_child"][p] = i
            else:
                T["right_child"][p] = i
        T["split_feature"].append(f); T["split_bin"].append(b); T["split_gain"].append(gain)
        T["left_child"].append(~L); T["right_child"].append(~(i + 1))
        T["internal_value"].append(out(lf["QG"], lf["QH"])); T["internal_weight"].append(lf["QH"] * sh)
        T["internal_count"].append(len(lf["rows"]))
        leaves[L] = leaf(lrows, lf["depth"] + 1, i)
        leaves.append(leaf(rrows, lf["depth"] + 1, i))
    if not T["split_feature"]:
        return None
    T["num_leaves"] = len(leaves)
    T["leaf_value"] = [out(lf["QG"], lf["QH"]) for lf in leaves]
    T["leaf_weight"] = [lf["QH"] * sh for lf in leaves]
    T["leaf_count"] = [len(lf["rows"]) for lf in leaves]
    T["leaf_rows"] = [lf["rows"] for lf in leaves]
    return T


def tree_leaf(T, brow):
    node = 0
    while True:
        nx = T["left_child"][node] if brow[T["split_feature"][node]] <= T["split_bin"][node] else T["right_child"][node]
        if nx < 0:
            return ~nx
        node = nx


def apply_tree(T, bins, scores):
    for r in range(bins.shape[0]):
        scores[r] = scores[r] + T["leaf_value"][tree_leaf(T, bins[r])]


def ndcg(scores, labels, off, k, T):
    vals = []
    for s in range(len(off) - 1):
        a, b = int(off[s]), int(off[s + 1])
        inv = inv_max_dcg(labels[a:b], k, T)
        if inv <= 0:
            vals.append(1.0)
            continue
        order = sorted_positions(scores[a:b])
        dcg = 0.0
        for p in range(min(k, b - a)):
            dcg += T["gain"][int(labels[a + order[p]])] * T["disc"][p]
        vals.append(dcg * inv)
    if not vals:
        raise ValueError("NDCG of a frame without sessions")
    return math.fsum(vals) / len(vals)


# ---------------------------------------------------------------- model text
def _n(x):
    return "%.17g" % float(x)


def model_text(trees, feats, binfo, params_block):
    """binfo: per feature (bounds, n_bins, min, max); params_block: the lines between 'parameters:' and its end"""
    blocks = []
    for i, t in enumerate(trees):
        thr = [binfo[f][0][b] for f, b in zip(t["split_feature"], t["split_bin"])]
        ln = ["Tree=%d" % i, "num_leaves=%d" % t["num_leaves"], "num_cat=0",
              "split_feature=" + " ".join(str(x) for x in t["split_feature"]),
              "split_gain=" + " ".join(_n(x) for x in t["split_gain"]),
              "threshold=" + " ".join(_n(x) for x in thr),
              "decision_type=" + " ".join("2" for _ in thr),
              "left_child=" + " ".join(str(x) for x in t["left_child"]),
              "right_child=" + " ".join(str(x) for x in t["right_child"]),
              "leaf_value=" + " ".join(_n(x) for x in t["leaf_value"]),
              "leaf_weight=" + " ".join(_n(x) for x in t["leaf_weight"]),
              "leaf_count=" + " ".join(str(x) for x in t["leaf_count"]),
              "internal_value=" + " ".join(_n(x) for x in t["internal_value"]),
              "internal_weight=" + " ".join(_n(x) for x in t["internal_weight"]),
              "internal_count=" + " ".join(str(x) for x in t["internal_count"]),
              "is_linear=0", "shrinkage=" + _n(t["shrinkage"])]
        blocks.append("".join(x + "\n" for x in ln) + "\n\n")
    infos = " ".join("[%s:%s]" % (_n(b[2]), _n(b[3])) if b[1] > 1 else "none" for b in binfo)
    text = "tree\nversion=v3\nnum_class=1\nnum_tree_per_iteration=1\nlabel_index=0\n"
    text += "max_feature_idx=%d\nobjective=lambdarank\n" % (len(feats) - 1)
    text += "feature_names=" + " ".join(feats) + "\nfeature_infos=" + infos + "\n"
    text += "tree_sizes=" + " ".join(str(len(b.encode())) for b in blocks) + "\n\n"
    text += "".join(blocks)
    imp = [0.0] * len(feats)
    for t in trees:
        for f, gn in zip(t["split_feature"], t["split_gain"]):
            imp[f] = imp[f] + gn
    text += "end of trees\n\nfeature_importances:\n"
    for f in sorted(range(len(feats)), key=lambda f: (-imp[f], f)):
        if imp[f] > 0:
            text += "%s=%s\n" % (feats[f], _n(imp[f]))
    text += "\nparameters:\n" + "".join(x + "\n" for x in params_block) + "end of parameters\n\npandas_categorical:null\n"
    return text


def fit(cols, feats, labels, off, params=None, valid=None, params_block=()):
    """cols {name: typed array}; valid (cols, labels, off) or None -> dict(text, history, scores, trees, bins, binfo)"""
    P = dict(DEFAULTS)
    P.update(params or {})
    T = tables(P["sigmoid"])
    binfo = [find_bins(cols[n], P["max_bin"]) for n in feats]
    n_bins = [b[1] for b in binfo]
    bins = np.stack([bin_column(cols[n], binfo[f][0]) for f, n in enumerate(feats)], axis=1)
    validf = [f for f, nb in enumerate(n_bins) if nb > 1]
    labels = np.asarray(labels)
    scores = np.zeros(len(labels))
    frames = {"train": (bins, labels, off, scores)}
    if valid is not None:
        vbins = np.stack([bin_column(valid[0][n], binfo[f][0]) for f, n in enumerate(feats)], axis=1)
        frames["valid"] = (vbins, np.asarray(valid[1]), valid[2], np.zeros(len(valid[1])))
    hist = {"iteration": [], "train": []}
    if valid is not None:
        hist["valid"] = []

    def record(it):
        hist["iteration"].append(it)
        for k, (b_, l_, o_, s_) in frames.items():
            hist[k].append(ndcg(s_, l_, o_, P["eval_at"], T))

    inv = [inv_max_dcg(labels[int(off[s]):int(off[s + 1])], P["lambdarank_truncation_level"], T)
           for s in range(len(off) - 1)]
    trees = []
    for it in range(1, P["n_estimators"] + 1):
        g, h = gradients(scores, labels, off, T, P["lambdarank_truncation_level"], P["lambdarank_norm"], inv)
        qg, qh, eg, eh, zero = quantise(g, h)
        if zero:
            break
        drawn = feature_draw(validf, P["colsample_bytree"], P["seed"], len(trees))
        t = grow_tree(bins, qg, qh, eg, eh, drawn, n_bins, P) if drawn else None
        if t is None:
            break
        t["shrinkage"] = P["learning_rate"]
        trees.append(t)
        for b_, l_, o_, s_ in frames.values():
            apply_tree(t, b_, s_)
        if it % P["eval_every"] == 0:
            record(it)
    if not hist["iteration"] or hist["iteration"][-1] != len(trees):
        record(len(trees))
    return dict(text=model_text(trees, feats, binfo, list(params_block)), history=hist, scores=scores, trees=trees,
                bins=bins, binfo=binfo, n_bins=n_bins)
