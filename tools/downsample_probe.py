#!/usr/bin/env python
"""Downsample and submission-scoring timing on the MI355X -> profiles/downsample_timing.json (the first record of
this stage: no earlier path exists, so no threshold is set).

A synthetic frame of about 20 M rows over the full feature table (ottohip_feature_columns with targets), session
lengths drawn with a mean of about 126 candidates, targets at the reference's positive rates (0.0045 / 0.0015 /
0.0012). Timed with device events, the first run of each shape discarded: the plan (both calls: the sizing count
and the count + select), the column gather of each target's kept rows, and ottohip_submission_recall on 20 submitted
aids per (session, type). Beside them the numpy restatement of tests/downsample_oracle.py on this host over a prefix
of the same frame, whose kept rows are compared with the device's.

  python tools/downsample_probe.py [--rows 20000000] [--reps 5] [--commit HASH] [--out profiles/downsample_timing.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

POS_RATE = {"clicks": 0.004535, "carts": 0.001491, "orders": 0.00122}  # model/train_lgbm_rankers.py:32-35
N_ITEMS = 1_855_603


def commit_hash(given):
    if given:
        return given
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True,
                              check=True).stdout.strip()
    except Exception:
        return "unknown"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=20_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cpu-rows", type=int, default=500_000)
    ap.add_argument("--cpu-score-sessions", type=int, default=5_000)
    ap.add_argument("--commit", default=os.environ.get("OTTOHIP_COMMIT", ""))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "downsample_timing.json"))
    a = ap.parse_args()
    import ctypes
    import pandas as pd
    import torch
    import downsample_oracle as O
    from otto_recommender_amd import _lib, config
    from otto_recommender_amd import candidates as C
    from otto_recommender_amd import downsample as D
    from otto_recommender_amd import submission as SB

    ctx = _lib.context(0)
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(1)
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    table = C.feature_columns(with_targets=True)
    lens = np.clip(rng.lognormal(mean=np.log(126) - 0.5, sigma=1.0, size=int(a.rows / 100)), 1, 2500).astype(np.int64)
    lens = lens[np.cumsum(lens) <= a.rows]
    off = np.r_[0, np.cumsum(lens)].astype(np.int64)
    n, S = int(off[-1]), len(lens)
    off_d = torch.from_numpy(off).to(dev)
    feats, row_bytes = {}, 0
    for nm, dt in table:
        tt = getattr(torch, dt.name)
        if nm == "session":
            feats[nm] = torch.repeat_interleave(torch.arange(S, device=dev, dtype=torch.int32), torch.from_numpy(lens).to(dev))
        elif nm == "aid_next":  # distinct within any window shorter than the catalogue
            feats[nm] = ((torch.arange(n, device=dev, dtype=torch.int64) * 7919) % N_ITEMS).to(torch.int32)
        elif nm.startswith("target_"):
            feats[nm] = (torch.rand(n, device=dev, generator=g) < POS_RATE[nm[len("target_"):]]).to(torch.int8)
        elif dt.kind == "f":
            feats[nm] = torch.randn(n, device=dev, generator=g, dtype=torch.float32)
        else:
            hi = {1: 100, 2: 2000, 4: 1_000_000}[dt.itemsize]
            feats[nm] = torch.randint(-1, hi, (n,), device=dev, generator=g, dtype=torch.int32).to(tt)
        row_bytes += dt.itemsize

    def timed(fn):
        ms = []
        for _ in range(a.reps + 1):  # the first run warms up
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        return float(np.median(ms[1:])), [float(x) for x in ms[1:]], out

    res = {"commit": commit_hash(a.commit), "rows": n, "sessions": S, "mean_session_len": float(lens.mean()),
           "max_session_len": int(lens.max()), "row_bytes": row_bytes, "columns": len(table), "reps": a.reps,
           "lds_rows": D.lds_rows(), "keep_ratio_neg_to_pos": config.DOWNSAMPLE_RATIO_NEG_TO_POS,
           "max_neg_per_session": config.DOWNSAMPLE_MAX_NEG_PER_SESSION, "seed": 42}
    tg = {t: feats[f"target_{t}"] for t in config.TYPES}
    ctx.set_timing(True)
    ms, runs, plans = timed(lambda: D.plan(off_d, feats["session"], feats["aid_next"], tg, ctx=ctx))
    phases = {nm: p_ms for nm, p_ms, _ in ctx.timings()}  # the second call of the last plan: count + select
    ctx.set_timing(False)
    res["plan"] = {"ms_both_calls": ms, "runs_ms": runs, "rows_per_s": n / ms * 1e3,
                   "last_call_phases_ms": phases,
                   "kept_rows": {t: int(plans[t][1].numel()) for t in config.TYPES},
                   "kept_sessions": {t: int((plans[t][0][1:] != plans[t][0][:-1]).sum().item()) for t in config.TYPES},
                   "read_bytes_model": n * (3 + 3 + 8), "note": "count reads 3 B/row twice, select 11 B/row at most"}
    res["gather"] = {}
    for t in config.TYPES:
        drop = {f"target_{o}" for o in config.TYPES if o != t}
        cols = {nm: c for nm, c in feats.items() if nm not in drop}
        cb = sum(dt.itemsize for nm, dt in table if nm not in drop)
        m = int(plans[t][1].numel())
        ms, runs, _ = timed(lambda: D.gather_rows(cols, plans[t][1], ctx))
        model = m * (2 * cb + 8 * -(-len(cols) // 16))
        res["gather"][t] = {"ms": ms, "runs_ms": runs, "rows_out": m, "columns": len(cols), "row_bytes": cb,
                            "traffic_model_bytes": model, "model_bytes_per_s": model / ms * 1e3,
                            "includes": "output allocation and the error-flag read of each call"}
    # the scorer: 20 submitted aids per (session, type), one to three labels, about one in four submitted
    k = 20
    ses_rows = torch.arange(S, device=dev, dtype=torch.int32).repeat_interleave(k)
    ranked = {t: {"session": ses_rows, "aid_next": torch.randint(0, 400, (S * k,), device=dev, generator=g,
                                                                  dtype=torch.int32)} for t in config.TYPES}
    n_lab = rng.integers(1, 4, S * 3)
    labels = pd.DataFrame({"session": np.repeat(np.tile(np.arange(S), 3), n_lab),
                           "aid": rng.integers(0, 400, int(n_lab.sum())),
                           "type": np.repeat(np.repeat(np.arange(3), S), n_lab)})
    t0 = time.perf_counter()
    Sx, lo, la, so, sa = SB.session_csrs(ranked, labels, ctx)
    torch.cuda.synchronize()
    csr_s = time.perf_counter() - t0
    sums = (ctypes.c_int64 * 6)()

    def score():
        _lib.check(_lib.load().ottohip_submission_recall(ctx.h, Sx, _lib.ptr(lo), _lib.ptr(la), _lib.ptr(so),
                                                         _lib.ptr(sa), sums, _lib.stream_handle()))
        return list(sums)

    ms, runs, got_sums = timed(score)
    res["scorer"] = {"ms": ms, "runs_ms": runs, "sessions": Sx, "submitted_rows": int(sa.numel()),
                     "label_rows": int(la.numel()), "sums": got_sums, "recall": SB.recall_from_sums(got_sums),
                     "csr_build_seconds_host_and_device": csr_s}
    # the numpy restatement on this host over a prefix of the same frame
    s_cpu = int(np.searchsorted(off, a.cpu_rows, side="right")) - 1
    n_cpu = int(off[s_cpu])
    host = {nm: feats[nm][:n_cpu].cpu().numpy() for nm in ("session", "aid_next", *[f"target_{t}" for t in config.TYPES])}
    t0 = time.perf_counter()
    ref = {t: O.plan(off[:s_cpu + 1], host["session"], host["aid_next"], host[f"target_{t}"]) for t in config.TYPES}
    cpu_s = time.perf_counter() - t0
    same = all(np.array_equal(plans[t][1][:int(plans[t][0][s_cpu].item())].cpu().numpy(), ref[t][1]) and
               np.array_equal(plans[t][0][:s_cpu + 1].cpu().numpy(), ref[t][0]) for t in config.TYPES)
    s_sc = min(a.cpu_score_sessions, S)
    sub_h = {t: (ranked[t]["session"][:s_sc * k].cpu().numpy(), ranked[t]["aid_next"][:s_sc * k].cpu().numpy())
             for t in config.TYPES}
    lab_h = labels[labels["session"] < s_sc]
    t0 = time.perf_counter()
    ref_sums = O.recall_sums(sub_h, lab_h)
    cpu_sc = time.perf_counter() - t0
    dev_sums = SB.recall_sums({t: {"session": torch.from_numpy(v[0]), "aid_next": torch.from_numpy(v[1])}
                               for t, v in sub_h.items()}, lab_h, ctx)
    res["cpu_numpy_restatement"] = {
        "note": "tests/downsample_oracle.py on the host CPU (polars is not installed: the only CPU baseline)",
        "plan_rows": n_cpu, "plan_sessions": s_cpu, "plan_targets": 3, "plan_seconds": cpu_s,
        "plan_rows_per_s_3_targets": n_cpu / cpu_s, "plan_rows_equal_to_device": bool(same),
        "score_sessions": s_sc, "score_seconds": cpu_sc, "score_sums_equal_to_device": ref_sums == dev_sums}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
