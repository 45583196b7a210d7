#!/usr/bin/env python
"""Rank stage timing on the MI355X -> profiles/rank_timing.json (the first record: no earlier path exists).

A synthetic frame over the real 105-column dtype table (ottohip_feature_columns without targets), rankers of the
reference's shape (config.PARAMS_LGBM: 150 trees, num_leaves 15, max_depth 4) whose thresholds are the columns' own
quantiles, session lengths drawn with a mean of about 126 candidates. Reported: rows/s of the scoring kernel for
1 and for 3 targets, the top-k stage apart, the fraction of the frame-read-once HBM bound, and beside them the
numpy restatement of tests/rank_oracle.py timed on this host over a subsample -- the only CPU baseline available,
since LightGBM is not installed.

  python tools/rank_timing.py [--rows 20000000] [--reps 3] [--out profiles/rank_timing.json]
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

HBM_BYTES_PER_S = 8.0e12  # MI355X HBM3E peak, the denominator of the read-once bound


def depth4_tree(rng, n_features, quantiles, num_leaves=15, max_depth=4):
    """a tree of num_leaves leaves and depth <= max_depth in LightGBM's numbering (split leaf L at step i ->
    internal node i, left child leaf L, right child leaf i + 1)"""
    ni = num_leaves - 1
    left, right = np.zeros(ni, np.int64), np.zeros(ni, np.int64)
    parent, depth = {0: -1}, {0: 0}
    for i in range(ni):
        ok = [L for L in range(i + 1) if depth[L] < max_depth]
        L = int(rng.choice(ok))
        p = parent[L]
        if p >= 0:
            if left[p] == ~L:
                left[p] = i
            else:
                right[p] = i
        left[i], right[i] = ~L, ~(i + 1)
        parent[L] = parent[i + 1] = i
        depth[L] = depth[i + 1] = depth[L] + 1
    feat = rng.integers(0, n_features, ni)
    return {"num_leaves": num_leaves, "leaf_value": rng.normal(size=num_leaves) * 0.25, "split_feature": feat,
            "threshold": np.array([float(rng.choice(quantiles[int(f)])) for f in feat]),
            "decision_type": np.full(ni, 2 | (2 << 2)),  # LightGBM's usual: NaN missing, default left
            "left_child": left, "right_child": right}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=20_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cpu-rows", type=int, default=200_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rank_timing.json"))
    a = ap.parse_args()
    import torch
    import rank_fixtures as RF
    import rank_oracle as O
    from otto_recommender_amd import _lib, config
    from otto_recommender_amd import candidates as C
    from otto_recommender_amd import rank as R

    ctx = _lib.context(0)
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(1)
    table = C.feature_columns(with_targets=False)
    names = [n for n, _ in table if n not in ("session", "aid_next")]
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    # session lengths: lognormal with mean ~126, clipped to the handle's limit
    lens = np.clip(rng.lognormal(mean=np.log(126) - 0.5, sigma=1.0, size=int(a.rows / 100)), 1, 4096).astype(np.int64)
    lens = lens[np.cumsum(lens) <= a.rows]
    off = np.r_[0, np.cumsum(lens)].astype(np.int64)
    n = int(off[-1])
    feats, row_bytes = {}, 0
    for nm, dt in table:
        if dt.kind == "f":
            feats[nm] = torch.randn(n, device=dev, generator=g, dtype=torch.float32)
        else:
            hi = {1: 100, 2: 2000, 4: 1_000_000}[dt.itemsize]
            feats[nm] = torch.randint(-1, hi, (n,), device=dev, generator=g, dtype=torch.int32).to(getattr(torch, dt.name))
        row_bytes += dt.itemsize
    sub = torch.randperm(n, device=dev, generator=g)[:a.cpu_rows]
    host = {nm: feats[nm][sub].cpu().numpy() for nm in names}
    qs = np.linspace(0.02, 0.98, 49)
    quant = [np.unique(np.quantile(host[nm].astype(np.float64), qs)) for nm in names]
    P = config.PARAMS_LGBM
    texts = {t: RF.booster_text([depth4_tree(rng, len(names), quant, P["num_leaves"], P["max_depth"])
                                 for _ in range(P["n_estimators"])], names) for t in config.TYPES}
    off_d = torch.from_numpy(off).to(dev)

    def timed(fn):
        ms = []
        for _ in range(a.reps + 1):  # the first run warms up
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        return float(np.median(ms[1:])), out

    res = {"rows": n, "sessions": int(len(lens)), "mean_session_len": float(lens.mean()), "row_bytes": row_bytes,
           "columns": len(table), "model": {k: P[k] for k in ("n_estimators", "num_leaves", "max_depth")},
           "reps": a.reps, "hbm_bytes_per_s_assumed": HBM_BYTES_PER_S}
    bound_ms = n * row_bytes / HBM_BYTES_PER_S * 1e3
    for label, targets in (("targets_1", config.TYPES[:1]), ("targets_3", config.TYPES)):
        rk = R.Ranker({t: R.parse_booster(texts[t]) for t in targets}, ctx)
        ms_s, scores = timed(lambda: rk._scores(feats))
        ms_k, ranked = timed(lambda: rk.topk(scores, off_d, feats["aid_next"], config.KEEP_TOP_K))
        res[label] = {"ranker": rk.info(), "score_ms": ms_s, "score_rows_per_s": n / ms_s * 1e3,
                      "score_fraction_of_read_once_hbm_bound": bound_ms / ms_s,
                      "topk_ms": ms_k, "topk_rows_per_s": n / ms_k * 1e3,
                      "kept_rows_per_target": int(ranked[0]["session"].numel())}
        if label == "targets_3":
            got = scores[:, sub].cpu().numpy()
        rk.free()
    # the numpy restatement on this host, same models, a subsample of the same rows (bit-equal scores expected)
    t0 = time.perf_counter()
    ref = [O.predict(O.parse(texts[t]), host) for t in config.TYPES]
    cpu_s = time.perf_counter() - t0
    res["cpu_numpy_restatement"] = {
        "note": "tests/rank_oracle.py on the host CPU; LightGBM is not installed, so this is the only CPU baseline",
        "rows": int(a.cpu_rows), "targets": 3, "seconds": cpu_s, "rows_per_s_3_targets": a.cpu_rows / cpu_s,
        "scores_bit_equal_to_device": bool(all(np.array_equal((r + 0.0).view(np.uint64), (x + 0.0).view(np.uint64))
                                               for r, x in zip(ref, got)))}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
