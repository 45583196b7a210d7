#!/usr/bin/env python
"""Submission csv timing on the MI355X -> profiles/submit_timing.json (the first record of this path: no time target).

Input: --sessions sessions (default 1,671,803, the competition's test set) x 3 targets x 20 aids, aids uniform below
1,855,603 from a fixed seed, the rows in (session, pred_rank) order as the rank stage leaves them. Steps, each its own
process so that each can sit under its own time limit; every step merges its figures into --out under "sessions_<N>":

  --step device   the ranked rows resident in HBM: ottohip_submit_plan and ottohip_submit_write timed apart with device
                  events (and the context's events around each pass), then the written text, resident as one piece:
                  ottohip_submission_scan and the whole read (scan, allocation, ottohip_submission_parse) the same way;
                  median of --reps after one warm-up; bytes/s against the text size. --label NAME stores the figures
                  under "device_NAME": the A/B of the write kernel runs this step with OTTOHIP_LIB set to the
                  library of `make submit_plain`
  --step file     host wall clock of write_submission and read_submission, the file included
  --step host     the host path at 1/16 of the sessions: rank.submission_frame + to_csv, read_csv + parse_submission

  python tools/submit_timing.py --step device [--sessions 1671803] [--commit HASH] [--out profiles/submit_timing.json]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

TARGETS = ("clicks", "carts", "orders")
FIRST_SESSION = 12_899_779  # the first test session of the data set: eight-digit ids
N_AIDS = 1_855_603
K = 20


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


def commit_of(given):
    if given:
        return given
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except Exception:
        return "unknown"


def host_columns(n_sessions, seed=0):
    rng = np.random.default_rng(seed)
    ses = np.repeat(np.arange(FIRST_SESSION, FIRST_SESSION + n_sessions, dtype=np.int32), K)
    rank = np.tile(np.arange(1, K + 1, dtype=np.int16), n_sessions)
    return {t: {"session": ses, "aid_next": rng.integers(0, N_AIDS, len(ses)).astype(np.int32), "pred_rank": rank}
            for t in TARGETS}


def timed(fn, reps):
    """median device milliseconds of fn() over reps runs after one warm-up, and the last result"""
    import torch
    ms, res = [], None
    for _ in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        res = fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms[1:])), res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=("device", "file", "host"), required=True)
    ap.add_argument("--sessions", type=int, default=1_671_803)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--label", default=None)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "submit_timing.json"))
    a = ap.parse_args()
    key = f"sessions_{a.sessions}"
    head = {"commit": commit_of(a.commit), "sessions": a.sessions, "targets": 3, "aids_per_line": K,
            "rows": a.sessions * 3 * K, "lines": a.sessions * 3}

    if a.step == "host":
        import io
        import pandas as pd
        from otto_recommender_amd import rank as R
        from otto_recommender_amd import submission as SB
        n = a.sessions // 16
        frames = {t: pd.DataFrame(c) for t, c in host_columns(n).items()}
        t0 = time.perf_counter()
        text = R.submission_frame(frames).to_csv(index=False).encode()
        t_w = time.perf_counter() - t0
        t0 = time.perf_counter()
        rows = SB.parse_submission(pd.read_csv(io.BytesIO(text), dtype=str))
        t_r = time.perf_counter() - t0
        n_rows = sum(len(v["aid_next"]) for v in rows.values())
        assert n_rows == n * 3 * K
        part = dict(head)
        part["host"] = {"timer": "host wall clock, one run, the text kept in memory (no file)",
                        "sessions": n, "rows": n_rows, "text_bytes": len(text),
                        "submission_frame_and_to_csv_s": t_w, "read_csv_and_parse_submission_s": t_r,
                        "write_rows_per_s": n_rows / t_w, "read_rows_per_s": n_rows / t_r,
                        "write_bytes_per_s": len(text) / t_w, "read_bytes_per_s": len(text) / t_r}
        merge(a.out, key, part)
        return

    import torch  # before the package loads libottohip.so: one HIP runtime in the process, torch's
    from otto_recommender_amd import _lib
    from otto_recommender_amd import submission as SB
    ctx = _lib.context(0)
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    ranked = {t: {c: torch.from_numpy(v).to(dev) for c, v in cols.items()} for t, cols in host_columns(a.sessions).items()}
    n_rows = a.sessions * 3 * K

    if a.step == "device":
        ctx.set_timing(True)
        phases = {}

        def plan():
            _, p, n_lines, n_bytes = SB._submit_plan(ranked, K, ctx)
            phases["plan"] = {k: ms for k, ms, _ in ctx.timings()}
            lib.ottohip_submit_free(p)
            return n_lines, n_bytes

        plan_ms, (n_lines, n_bytes) = timed(plan, a.reps)
        _, p, _, _ = SB._submit_plan(ranked, K, ctx)
        out = torch.empty(n_bytes, dtype=torch.uint8, device=dev)

        def write():
            _lib.check(lib.ottohip_submit_write(ctx.h, p, _lib.ptr(out), n_bytes, _lib.stream_handle()))

        write_ms, _ = timed(write, a.reps)
        lib.ottohip_submit_free(p)
        assert n_lines == a.sessions * 3
        scan_ms, _ = timed(lambda: SB._scan_piece(ctx, out, n_bytes, True), a.reps)
        phases["scan"] = {k: ms for k, ms, _ in ctx.timings()}
        read_ms, (cols, seen, lines) = timed(lambda: SB._read_piece(ctx, out, n_bytes, True, 0, 0), a.reps)
        phases["parse"] = {k: ms for k, ms, _ in ctx.timings()}
        ctx.set_timing(False)
        assert lines == n_lines and seen == 7 and sum(c[0].numel() for c in cols) == n_rows
        for t, name in enumerate(("clicks", "carts", "orders")):  # the rows come back as they went in
            assert torch.equal(cols[t][1], ranked[name]["aid_next"]) and torch.equal(cols[t][0], ranked[name]["session"])
        part = dict(head)
        part["device" + (f"_{a.label}" if a.label else "")] = {
            "timer": f"device events around each call, median of {a.reps} runs after one warm-up; phase_ms: the "
                     "context's events around the passes of the last run's call. plan includes its two host reads "
                     "(the counts, the total); read = scan + allocation of the columns + parse (which repeats the "
                     "scan's passes)",
            "library": os.path.basename(os.environ.get("OTTOHIP_LIB") or "") or "in-tree",
            "text_bytes": n_bytes, "plan_ms": plan_ms, "write_ms": write_ms, "scan_ms": scan_ms, "read_ms": read_ms,
            "parse_call_ms": read_ms - scan_ms, "phase_ms": phases,
            "write_bytes_per_s": n_bytes / write_ms * 1e3, "plan_and_write_bytes_per_s": n_bytes / (plan_ms + write_ms) * 1e3,
            "plan_and_write_rows_per_s": n_rows / (plan_ms + write_ms) * 1e3,
            "read_bytes_per_s": n_bytes / read_ms * 1e3, "read_rows_per_s": n_rows / read_ms * 1e3}
        merge(a.out, key, part)
        return

    # --step file
    small = {t: {c: v[:2000] for c, v in cols.items()} for t, cols in ranked.items()}
    with tempfile.TemporaryDirectory() as d:
        SB.read_submission(SB.submission_bytes(small, K, ctx).cpu().numpy().tobytes(), ctx=ctx)  # kernels loaded
        path = os.path.join(d, "submission.csv")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n_lines = SB.write_submission(ranked, path, K, ctx)
        t_w = time.perf_counter() - t0
        size = os.path.getsize(path)
        t0 = time.perf_counter()
        rows = SB.read_submission(path, ctx=ctx)
        torch.cuda.synchronize()
        t_r = time.perf_counter() - t0
    assert n_lines == a.sessions * 3 and sum(v["aid_next"].numel() for v in rows.values()) == n_rows
    part = dict(head)
    part["file"] = {"timer": "host wall clock, one run after a small warm-up; the file is written to the temp dir and "
                             "read back from the page cache",
                    "text_bytes": size, "write_submission_s": t_w, "read_submission_s": t_r,
                    "write_rows_per_s": n_rows / t_w, "read_rows_per_s": n_rows / t_r,
                    "write_bytes_per_s": size / t_w, "read_bytes_per_s": size / t_r}
    merge(a.out, key, part)


if __name__ == "__main__":
    main()
