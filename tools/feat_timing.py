"""First measurement of the ranker feature columns (csrc/features.hip): one 100k-session file's
Candidates.features call (whole call, and its fold kernel alone from the context's phase events) on the device,
and the pandas restatement (tests/feats_oracle.py) on a slice of the same file, to place the number.

Inputs are a config-5 shaped synthetic job: --sessions synthetic sessions counted into the five co-count tables
(reference min counts, R1 top-N with every value column), kNN lists of both embedding tables for the first
--knn-queries vocabulary rows (dist = trunc of the squared distance, a stand-in for the reference's Int32 cast),
random session clusters with the device's C3 cl50 ranks, cl1 ranks, labels by the OTTO protocol. The file is the
first --file-sessions sessions of the test split.

  python tools/feat_timing.py --out profiles/feat_fold.json
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sessions", type=int, default=1_500_000)
    ap.add_argument("--file-sessions", type=int, default=100_000)
    ap.add_argument("--knn-queries", type=int, default=600_000)
    ap.add_argument("--oracle-sessions", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import pandas as pd
    import torch
    import otto_recommender_amd.synth as synth
    from otto_recommender_amd import _lib, config, covis as gc, retrieve as gr, popularity as gp, candidates as gcand
    from otto_recommender_amd.w2vec import KnnIndex
    ctx = _lib.context()
    dev = torch.device("cuda", ctx.device)
    ev = synth.generate(args.sessions)
    train, test, labels = synth.split_test_labels(ev)
    fb = synth.file_session_bounds(ev.n_sessions)
    dev_all = gc.DeviceEvents.from_host(ev, fb)
    tab = gc.count_co_events_fused(dev_all)
    r1, r1v = {}, {}
    for n in config.CO_EVENTS_TO_COUNT:
        a, b, c = tab.finalize(n)
        r = gr.topk_per_aid(a, b, c, config.RETRIEVAL_FIRST_N_CO_COUNTS[n], ctx=ctx)
        r1[n] = (r["aid"], r["aid_next"], r["rank"])
        r1v[n] = (r["aid"], r["count"], r["count_pop"], r["perc_pop"], r["count_rel"])
    tab.free()
    words = synth.item_words()
    w = torch.as_tensor(np.asarray(words, np.int32)).to(dev)
    knn, knnv = [], []
    for seed in (1, 3):
        emb = torch.from_numpy(synth.embeddings(len(words), seed=seed)).to(dev)
        idx = KnnIndex(emb, ctx)
        nq = min(args.knn_queries, idx.n_items)
        i, d2 = idx.search(torch.arange(nq, dtype=torch.int32, device=dev), k=config.W2VEC_K)
        idx.free()
        valid = i >= 0
        q = w[:nq].view(nq, 1).expand(nq, config.W2VEC_K)[valid].contiguous()
        rk = torch.arange(1, config.W2VEC_K + 1, device=dev, dtype=torch.int16).view(1, -1).expand(nq, -1)[valid]
        knn.append((q, w[i.clamp(min=0).long()][valid].contiguous(), rk.contiguous()))
        knnv.append((q, d2[valid].clamp(max=2e9).to(torch.int32).contiguous()))
        if seed == 1:
            emb_all = emb
        del emb
    rng = np.random.default_rng(0)
    cl_all = rng.integers(0, 50, ev.n_sessions).astype(np.int32)
    pop50 = gp.count_popularity(dev_all.offsets, dev_all.aid, dev_all.ts, dev_all.type, cl_all, 50, ctx=ctx)
    pop1 = gp.count_popularity(dev_all.offsets, dev_all.aid, dev_all.ts, dev_all.type, np.zeros(ev.n_sessions, np.int32),
                               1, suffix="cl1", ctx=ctx)
    p = pop50[pop50[gcand.CL50_RANKS].min(axis=1) <= 20]
    src = gcand.CandidateSources(r1, knn[0], knn[1], (p["cl50"].to_numpy(), p["aid"].to_numpy()), 50, ctx=ctx)
    val = gcand.FeatureValues(src, r1v, knnv[0], knnv[1], (p["cl50"].to_numpy(), p[gcand.CL50_RANKS].to_numpy()),
                              (pop1["aid"].to_numpy(), pop1[gcand.CL1_RANKS[0:3]].to_numpy()))
    # the file: the first file-sessions test sessions
    S = min(args.file_sessions, test.n_sessions)
    e1 = int(test.session_offsets[S] - test.session_offsets[0])
    off = test.session_offsets[:S + 1] - test.session_offsets[0]
    f_aid, f_ts, f_ty = test.aid[:e1], test.ts[:e1], test.type[:e1]
    sess_ids = test.session[test.session_offsets[:S] - test.session_offsets[0]]
    n_train = train.n_sessions
    scl = torch.from_numpy(cl_all[n_train:n_train + S]).to(dev)
    events = tuple(torch.as_tensor(np.ascontiguousarray(x)).to(dev) for x in (off, f_aid, f_ts, f_ty))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    c = gcand.generate(*events, src, scl)
    torch.cuda.synchronize()
    t_gen = time.perf_counter() - t0
    lab = labels[labels["session"].isin(sess_ids)]
    lo, la = gcand.labels_csr_device(lab["session"].to_numpy(), lab["aid"].to_numpy(), lab["type"].to_numpy(), sess_ids,
                                     ctx=ctx)
    whole, fold, aids = [], [], []
    for rep in range(args.reps + 1):  # the first call is the warm-up (allocations, code object load)
        ctx.set_timing(True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f = c.features(events, src, val, scl, (lo, la), 0, S)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        ph = {n: ms for n, ms, _ in ctx.timings()}
        ctx.set_timing(False)
        if rep:
            whole.append(dt * 1e3)
            fold.append(ph.get("feat_fold", float("nan")))
            aids.append(ph.get("feat_aids", float("nan")))
        if rep < args.reps:
            del f
    n_cand = int(f["session"].numel())
    per = np.diff(c.to_torch()["off"].cpu().numpy())
    # the pandas restatement on a slice of the same file
    import feats_oracle as F
    So = min(args.oracle_sessions, S)
    eo = int(off[So])
    df = pd.DataFrame({"session": np.repeat(sess_ids[:So], np.diff(off[:So + 1])), "aid": f_aid[:eo], "ts": f_ts[:eo],
                       "type": f_ty[:eo]})
    h = lambda t: t.cpu().numpy()
    own = np.unique(f_aid[:eo])
    # the list frames restricted to the slice's aids (every join of the restatement is on a session aid, so the
    # result is the same; the untimed restriction keeps the timed part to the restatement's own work)
    mine = lambda fr: fr[fr["aid"].isin(own)].reset_index(drop=True)
    r1f = {}
    for n in config.CO_EVENTS_TO_COUNT:
        r1f[n] = mine(pd.DataFrame({"aid": h(r1[n][0]), "aid_next": h(r1[n][1]), f"{n}_count": h(r1v[n][1]),
                                    f"{n}_count_pop": h(r1v[n][2]), f"{n}_perc_pop": h(r1v[n][3]),
                                    f"{n}_rank": h(r1[n][2]), f"{n}_count_rel": h(r1v[n][4])}))
    kf = [mine(pd.DataFrame({"aid": h(knn[k][0]), "aid_next": h(knn[k][1]), f"dist_w2vec_{nm}": h(knnv[k][1]),
                             f"rank_w2vec_{nm}": h(knn[k][2])})) for k, nm in enumerate(("all", "1_2"))]
    scf = pd.DataFrame({"session": sess_ids[:So], "cl50": cl_all[n_train:n_train + So]})
    none_a = pd.DataFrame({"aid": np.zeros(0, np.int32), "dim_0_aid": np.zeros(0, np.float32)})
    none_s = pd.DataFrame({"session": np.zeros(0, np.int32), "dim_0_ses": np.zeros(0, np.float32)})
    t0 = time.perf_counter()
    ref = F.retrieve_and_gen_feats(df, r1f, kf[0], kf[1], scf, pop1, pop50, none_a, none_s,
                                   lab[lab["session"].isin(sess_ids[:So])])
    t_oracle = time.perf_counter() - t0
    # the slice's device columns equal the restatement (cos / eucl are not part of the features call)
    k = len(ref)
    sid = sess_ids[h(f["session"][:k]).astype(np.int64)]
    bad = [nm for nm in ref.columns if not nm.endswith("_ses_aid") and not np.array_equal(
        (sid if nm == "session" else h(f[nm][:k])).astype(np.int64), ref[nm].to_numpy().astype(np.int64))]
    head = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    out = {"what": "Candidates.features on one file of a config-5 shaped synthetic job (tools/feat_timing.py)",
           "commit": head or None, "device": torch.cuda.get_device_name(ctx.device),
           "job_sessions": args.sessions, "file_sessions": S, "file_events": e1, "candidates": n_cand,
           "candidates_per_session": {"mean": float(per.mean()), "p50": float(np.percentile(per, 50)),
                                      "p99": float(np.percentile(per, 99)), "max": int(per.max())},
           "list_rows": {n: int(r1[n][0].numel()) for n in r1} | {"w2vec_all": int(knn[0][0].numel()),
                                                                  "w2vec_1_2": int(knn[1][0].numel())},
           "generate_ms": t_gen * 1e3, "features_call_ms": whole, "feat_fold_kernel_ms": fold,
           "feat_aids_kernel_ms": aids, "reps": args.reps,
           "oracle": {"sessions": So, "rows": k, "seconds": t_oracle, "columns_equal_device": not bad,
                      "columns_differing": bad}}
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
    c.free()


if __name__ == "__main__":
    main()
