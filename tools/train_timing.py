#!/usr/bin/env python
"""Train stage timing on the MI355X -> profiles/train_timing.json (the first record: no earlier path exists, so there
is no time target).

A synthetic frame of the downsampled shape: about 3 M rows (what the clicks frame keeps of 20 M retrieved rows,
profiles/downsample_timing.json) over the real feature dtype table, lognormal session lengths, one positive per
session placed by a noisy function of two columns, the reference's parameters (config.PARAMS_LGBM). Steps, each run
as its own process so that each can sit under its own time limit; every step merges its figures into --out:

  --step stages   binning once; then gradients, quantiser, root histogram (the tree's drawn features), split scan,
                  root partition, tree apply, NDCG@20: median of --reps after a warm-up
  --step trees    boost_one for --trees iterations: per-tree seconds (the first apart), extrapolated to n_estimators
  --step cpu      placements on this host's CPU, neither a comparison with LightGBM: the numpy restatement
                  (tests/train_oracle.py) on a subset, and scikit-learn's HistGradientBoostingRegressor on the 0 / 1
                  label at the same bins, leaves and depth when scikit-learn is installed

  python tools/train_timing.py --step stages [--rows 3000000] [--reps 3] [--out profiles/train_timing.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def frame(rows, seed=1):
    """host columns {name: typed array}, labels int8, session sizes"""
    from otto_recommender_amd import candidates as C
    rng = np.random.default_rng(seed)
    table = [(n, dt) for n, dt in C.feature_columns(with_targets=False) if n not in ("session", "aid_next")]
    lens = np.clip(rng.lognormal(mean=np.log(40) - 0.32, sigma=0.8, size=int(rows / 20)), 2, 400).astype(np.int64)
    lens = lens[np.cumsum(lens) <= rows]
    off = np.r_[0, np.cumsum(lens)]
    n = int(off[-1])
    cols = {}
    for nm, dt in table:
        if dt.kind == "f":
            cols[nm] = rng.standard_normal(n, dtype=np.float32)
        else:
            hi = {1: 100, 2: 2000, 4: 1_000_000}[dt.itemsize]
            cols[nm] = rng.integers(-1, hi, n).astype(dt)
    fl = [nm for nm, dt in table if dt.kind == "f"][:2]
    key = cols[fl[0]] + 0.5 * cols[fl[1]] + rng.standard_normal(n, dtype=np.float32)
    top = np.maximum.reduceat(key, off[:-1])
    y = (key == np.repeat(top, lens)).astype(np.int8)
    return cols, y, lens, [nm for nm, _ in table]


def merge(out, part):
    res = {}
    if os.path.exists(out):
        with open(out) as fh:
            res = json.load(fh)
    res.update(part)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(part))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=("stages", "trees", "cpu"), required=True)
    ap.add_argument("--rows", type=int, default=3_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--trees", type=int, default=8)
    ap.add_argument("--cpu-rows", type=int, default=30_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_timing.json"))
    a = ap.parse_args()
    if a.step != "cpu":
        import torch  # before the package loads libottohip.so: one HIP runtime in the process, torch's
    from otto_recommender_amd import config
    from otto_recommender_amd import train as T
    cols, y, lens, names = frame(a.rows)
    n = len(y)
    P = T.resolve_params({})
    if a.step == "cpu":
        import train_oracle as O
        m = int(np.searchsorted(np.cumsum(lens), a.cpu_rows))
        sub = int(np.sum(lens[:m]))
        sc = {k: v[:sub] for k, v in cols.items()}
        t0 = time.perf_counter()
        r = O.fit(sc, names, y[:sub], np.r_[0, np.cumsum(lens[:m])], dict(n_estimators=2))
        part = {"cpu_numpy_restatement": {"note": "tests/train_oracle.py on the host CPU: a placement, not LightGBM",
                                          "rows": sub, "trees": len(r["trees"]),
                                          "seconds_per_tree_with_binning": (time.perf_counter() - t0) / 2}}
        try:
            from sklearn.ensemble import HistGradientBoostingRegressor
            X = np.stack([cols[k][:1_000_000].astype(np.float32) for k in names], axis=1)
            t0 = time.perf_counter()
            HistGradientBoostingRegressor(max_iter=10, max_leaf_nodes=P["num_leaves"], max_depth=P["max_depth"],
                                          max_bins=255, learning_rate=P["learning_rate"], early_stopping=False,
                                          min_samples_leaf=P["min_child_samples"]).fit(X, y[:len(X)].astype(np.float32))
            part["cpu_sklearn_hist_gbdt"] = {
                "note": "least squares on the 0 / 1 label, every feature in every tree, all host cores: a placement",
                "rows": int(len(X)), "trees": 10, "seconds_per_tree_with_binning": (time.perf_counter() - t0) / 10}
        except ImportError:
            part["cpu_sklearn_hist_gbdt"] = {"note": "scikit-learn is not installed"}
        merge(a.out, part)
        return
    import torch
    from otto_recommender_amd import _lib
    ctx = _lib.context(0)
    dev = torch.device("cuda", 0)

    def timed(fn, reps=a.reps):
        ms = []
        for _ in range(reps + 1):  # the first run warms up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ms[1:])), out

    dcols = {k: torch.from_numpy(v).to(dev) for k, v in cols.items()}
    t0 = time.perf_counter()
    binner = T.Binner(dcols, names, P["max_bin"], ctx)
    t1 = time.perf_counter()
    bins = binner.bin_frame(dcols)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    off = torch.from_numpy(np.r_[0, np.cumsum(lens)].astype(np.int64)).to(dev)
    tr = T.Trainer(bins, torch.from_numpy(y).to(dev), off, binner.n_bins, P, ctx)
    head = {"rows": n, "sessions": int(len(lens)), "mean_session_len": float(lens.mean()), "features": len(names),
            "valid_features": len(binner.valid), "bin_stride_bytes": binner.stride,
            "params": {k: P[k] for k in ("n_estimators", "learning_rate", "max_depth", "num_leaves", "colsample_bytree",
                                         "min_child_samples", "max_bin")},
            "reps": a.reps, "timer": "host wall clock around a synchronised call, median after one warm-up"}
    if a.step == "stages":
        drawn = T.feature_draw(binner.valid, P["colsample_bytree"], P["seed"], 0)
        feats = torch.tensor(drawn, dtype=torch.int32, device=dev)
        nb = torch.tensor([binner.n_bins[f] for f in drawn], dtype=torch.int32, device=dev)
        rows = torch.arange(n, dtype=torch.int32, device=dev)
        perm = torch.randperm(n, device=dev)[:n // 2].sort().values.to(torch.int32)
        ms_g, (g, h) = timed(lambda: T.lambdarank_gradients(tr.scores, tr.labels, tr.off, tr.tables, tr.inv_max))
        ms_q, (gh, eg, eh, _) = timed(lambda: T.quantise(g, h, ctx))
        ms_h, H = timed(lambda: T.histograms(bins, gh, rows, feats, 0, ctx))
        ms_h2, _ = timed(lambda: T.histograms(bins, gh, perm, feats, 0, ctx))
        ms_s, rec = timed(lambda: T.split_scan(H[None], nb, eg, eh, P["min_child_samples"],
                                               P["min_sum_hessian_in_leaf"], P["lambda_l2"], ctx))
        best = T._best(rec[0], drawn)
        ms_p, _ = timed(lambda: T.partition(bins, best[1], best[2], rows, ctx))
        tree = {"num_leaves": 2, "split_feature": [best[1]], "split_bin": [best[2]], "left_child": [-1],
                "right_child": [-2], "leaf_value": [0.0, 0.0]}
        ms_a, _ = timed(lambda: T.apply_tree(bins, tree, tr.scores, ctx))
        ms_n, _ = timed(lambda: tr.ndcg())
        k = len(drawn)
        part = dict(head)
        part["binning"] = {"find_bins_s": t1 - t0, "bin_frame_s": t2 - t1}
        part["stages_ms"] = {"gradients": ms_g, "quantise": ms_q, "histogram_root": ms_h,
                             "histogram_half_scattered": ms_h2, "split_scan": ms_s, "partition_root": ms_p,
                             "tree_apply": ms_a, "ndcg_at_20": ms_n}
        part["histogram_root"] = {
            "drawn_features": k, "row_feature_items_per_s": n * k / ms_h * 1e3, "lds_atomics_per_s": 3 * n * k / ms_h * 1e3,
            "bytes_read_lower_bound": n * (8 + 4 + binner.stride),
            "GB_per_s_at_lower_bound": n * (8 + 4 + binner.stride) / ms_h / 1e6}
        merge(a.out, part)
        return
    times = []
    for _ in range(a.trees):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ok = tr.boost_one()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
        if not ok:
            break
    rest = times[1:] or times
    part = dict(head)
    part["trees"] = {"boosted": len(tr.trees), "leaves": [t["num_leaves"] for t in tr.trees],
                     "first_tree_s": times[0], "per_tree_s_median": float(np.median(rest)),
                     "per_tree_s": times, "fit_s_extrapolated_to_n_estimators": float(np.median(rest)) * P["n_estimators"],
                     "train_ndcg_at_20": tr.ndcg()["train"]}
    merge(a.out, part)


if __name__ == "__main__":
    main()
