#!/usr/bin/env python
"""Word2Vec trainer timing on the MI355X -> profiles/w2v_timing.json (the first record: no earlier path exists, so
there is no time target).

The synthetic event stream of BASELINE configs[2] (synth.generate_events, the OTTO catalogue of 1 855 603 items), the
reference's parameters (vector_size 100, window 10, min_count 5, all types) and the recalled gensim defaults
(config.W2VEC_DEFAULTS). Steps, each run as its own process so that each can sit under its own time limit; every step
merges its figures into --out under the key "events_<N>":

  --step epochs   the trainer's epochs 0 .. --epochs - 1 (ottohip_w2v_epoch), a host clock around each synchronised
                  call: seconds per epoch, kept positions per second, the fit extrapolated to the configured epochs
  --step phases   one trained epoch, then the stages of the next on those weights, device events around each call:
                  compaction (median of --reps), and for --batches batches spread over the epoch the batch kernel and
                  the two apply passes; rows touched per batch; atomic bytes per second of the batch kernel

  python tools/w2v_timing.py --step epochs [--events 20000000] [--epochs 2] [--out profiles/w2v_timing.json]

The only outside figure is the reference's own note (model/w2vec_aids.py:210-211): 43 min for the all-types model and
22 min for the carts+orders one, on 16 CPU threads of hardware it does not name. Nothing here is a comparison with it.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def merge(out, key, part):
    res = {}
    if os.path.exists(out):
        with open(out) as fh:
            res = json.load(fh)
    res.setdefault(key, {}).update(part)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps({key: part}))


def context_counts(W, rows_n, orig, sid, coff, b0, b1, window, seed, epoch):
    """contexts per position of [b0, b1), from the definition's reduced-window draw (host numpy)"""
    sm = W.mix(int(seed) & W.MASK64)
    inner = W.mix(sm ^ ((int(epoch) << 32) | 1))
    d = W._mix_np(np.uint64(inner) ^ (orig[b0:b1].astype(np.int64) & 0xFFFFFFFF).astype(np.uint64))
    eff = window - (d % np.uint64(window)).astype(np.int64)
    p = np.arange(b0, b1, dtype=np.int64)
    s = sid[b0:b1].astype(np.int64)
    lo, hi = np.maximum(coff[s], p - eff), np.minimum(coff[s + 1] - 1, p + eff)
    return hi - lo


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=("epochs", "phases"), required=True)
    ap.add_argument("--events", type=int, default=20_000_000)
    ap.add_argument("--epochs", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batches", type=int, default=12)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "w2v_timing.json"))
    a = ap.parse_args()
    import torch  # before the package loads libottohip.so: one HIP runtime in the process, torch's
    from otto_recommender_amd import _lib, config, synth
    from otto_recommender_amd import w2vec as W
    from otto_recommender_amd.covis import DeviceEvents
    ctx = _lib.context(0)
    t0 = time.perf_counter()
    ev = synth.generate_events(a.events, seed=0)
    t_gen = time.perf_counter() - t0
    dev_ev = DeviceEvents.from_host(ev)
    params = {"vector_size": config.W2VEC_VECTOR_SIZE, "window": 10, "min_count": 5}
    t0 = time.perf_counter()
    tr = W.Word2VecTrainer(dev_ev, None, config.N_ITEMS_OTTO, ctx, params)
    torch.cuda.synchronize()
    t_setup = time.perf_counter() - t0
    P, V, dim = tr.params, tr.n_vocab, tr.dim
    B = int(P["batch_positions"])
    key = f"events_{ev.n_events}"
    head = {"events": int(ev.n_events), "sessions": int(ev.n_sessions), "n_vocab": int(V), "dim": dim,
            "window": int(P["window"]), "negative": int(P["negative"]), "sample": P["sample"],
            "batch_positions": B, "fixed_shift": config.W2VEC_FIXED_SHIFT,
            "host_generate_events_s": t_gen, "vocabulary_tables_initial_weights_s": t_setup}
    if a.step == "epochs":
        secs, kept, nbs = [], [], []
        for e in range(a.epochs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            nk, nb = tr.epoch(e)
            torch.cuda.synchronize()
            secs.append(time.perf_counter() - t0); kept.append(nk); nbs.append(nb)
        rest = secs[1:] or secs
        vec = tr.vectors()
        part = dict(head)
        part["epochs"] = {"timer": "host wall clock around a synchronised ottohip_w2v_epoch (compaction, every batch, "
                                   "every apply); the first epoch also builds the event -> session map",
                          "seconds": secs, "kept_positions": kept, "batches": nbs,
                          "kept_positions_per_s": [k / s for k, s in zip(kept, secs)],
                          "fit_s_extrapolated_to_configured_epochs": secs[0] + float(np.median(rest)) * (int(P["epochs"]) - 1),
                          "configured_epochs": int(P["epochs"]),
                          "vectors_finite": bool(torch.isfinite(vec).all().item()),
                          "vectors_abs_max": float(vec.abs().max().item())}
        merge(a.out, key, part)
        tr.free()
        return

    def timed(fn):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record(); out = fn(); e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e), out

    tr.epoch(0)
    syn0, syn1 = tr.vectors(with_syn1neg=True)
    tr.free()
    epoch = 1
    ms_c = []
    for _ in range(a.reps + 1):  # the first run warms up
        ms, comp = timed(lambda: W.w2v_compact(dev_ev, tr.row_of_aid, tr.keep_thr, tr.mask, P["seed"], epoch, ctx=ctx))
        ms_c.append(ms)
    rows, orig, sid, coff = comp
    N = int(rows.numel())
    n_b = (N + B - 1) // B
    h_orig, h_sid, h_coff = orig.cpu().numpy(), sid.cpu().numpy(), coff.cpu().numpy()
    acc0, acc1 = (torch.zeros((V, dim), dtype=torch.int64, device=syn0.device) for _ in range(2))
    f0, f1 = (torch.zeros(V, dtype=torch.uint8, device=syn0.device) for _ in range(2))
    lr = float(np.float32(P["alpha"]))
    picks = sorted({int(x) for x in np.linspace(0, max(n_b - 2, 0), a.batches)})  # full batches, spread over the epoch
    recs = []
    for i, b in enumerate([picks[0]] + picks):  # the first batch once more to warm up
        b0, b1 = b * B, min(N, (b + 1) * B)
        ms_b, _ = timed(lambda: W.w2v_batch(rows, orig, sid, coff, b0, b1, syn0, syn1, tr.cum, tr.sig, tr.abi_params,
                                            epoch, lr, acc0, acc1, f0, f1, ctx=ctx))
        touched = (int(f0.sum().item()), int(f1.sum().item()))
        ms_a0, _ = timed(lambda: W.w2v_apply(syn0, acc0, f0, ctx=ctx))
        ms_a1, _ = timed(lambda: W.w2v_apply(syn1, acc1, f1, ctx=ctx))
        if i == 0:
            continue
        nctx = context_counts(W, N, h_orig, h_sid, h_coff, b0, b1, int(P["window"]), P["seed"], epoch)
        n_pos = int((nctx > 0).sum())
        adds = int(nctx.sum()) + n_pos * (1 + int(P["negative"]))  # row adds: contexts exactly, targets at most
        recs.append({"batch": b, "positions": b1 - b0, "positions_with_context": n_pos, "batch_ms": ms_b,
                     "apply_syn0_ms": ms_a0, "apply_syn1neg_ms": ms_a1, "rows_touched_syn0": touched[0],
                     "rows_touched_syn1neg": touched[1], "row_adds_upper": adds, "atomic_bytes_upper": adds * dim * 8})
    med = lambda k: float(np.median([r[k] for r in recs]))
    bm, am = med("batch_ms"), med("apply_syn0_ms") + med("apply_syn1neg_ms")
    part = dict(head)
    part["phases"] = {
        "timer": "device events around each stage call; compaction: median after one warm-up (it ends in a host read); "
                 "batch / apply: median over the sampled batches, weights after one trained epoch",
        "epoch": epoch, "kept_positions": N, "batches": n_b,
        "compact_ms": float(np.median(ms_c[1:])), "batch_ms_median": bm, "apply_ms_median_both_matrices": am,
        "ms_per_epoch_by_phase": {"compact": float(np.median(ms_c[1:])), "batch": bm * N / B, "apply": am * N / B},
        "positions_per_s_batch_kernel": med("positions") / bm * 1e3,
        "atomic_bytes_per_s_upper": med("atomic_bytes_upper") / bm * 1e3,
        "atomic_bytes_note": "8 bytes x dim per row add; context adds counted exactly from the window draws, target adds "
                             "at 1 + negative per position (targets skipped as equal to the word or saturated are not "
                             "subtracted): an upper figure of what the kernel issued, not a roof. The rate of 64-bit "
                             "integer atomics on gfx950 is not otherwise measured",
        "rows_touched_per_batch_median": {"syn0": med("rows_touched_syn0"), "syn1neg": med("rows_touched_syn1neg")},
        "sampled_batches": recs}
    merge(a.out, key, part)


if __name__ == "__main__":
    main()
