#!/usr/bin/env python
"""jsonl ETL timing on the MI355X -> profiles/etl_timing.json (the first record of this path: no time target).

Input: the sessions text of synth.generate_events(--events) in the data set's compact style, written once to --text
(default: a file in the temp dir) by whichever step runs first. Steps, each its own process so that each can sit
under its own time limit; every step merges its figures into --out under the key "events_<N>":

  --step device   the text resident in HBM as one piece (the first 2^31 - 1 bytes of whole lines if it is longer):
                  ottohip_jsonl_count, then ottohip_jsonl_sessions with the context's device events around classify,
                  scan, locate and parse; median of --reps after one warm-up; bytes/s, events/s and the fraction of
                  8 TB/s on the byte model stated in the output
  --step file     from the file, a host clock: events_from_jsonl (read, pinned upload, parse, CSR), and
                  transform_jsonl_to_parquet on its own (writing parquet is host work)
  --step host     the only comparison made: on a prefix of at least --host-lines whole lines of the same text,
                  pandas.read_json(lines=True) plus the column loop (the reference's algorithm, restated in
                  tests/etl_oracle.py) and plain json.loads per line; the extrapolation to the whole text by bytes is
                  labelled as one

  python tools/etl_timing.py --step device [--events 20000000] [--out profiles/etl_timing.json]

The only outside figure is the reference's own note (etl/jsonl_to_parquet.py:93): "ETA ~15min" for the whole data set
on hardware it does not name. Nothing here is a comparison with it.
"""
import argparse
import io
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

HBM_BYTES_PER_S = 8e12


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


def ensure_text(path, n_events):
    """writes the text once; returns (bytes, events, lines, seconds spent writing or 0)"""
    from otto_recommender_amd import synth
    import etl_fixtures as F
    meta = path + ".meta.json"
    if os.path.exists(path) and os.path.exists(meta):
        with open(meta) as fh:
            m = json.load(fh)
        if m.get("target_events") == n_events and m.get("bytes") == os.path.getsize(path):
            return m["bytes"], m["events"], m["lines"], 0.0
    t0 = time.perf_counter()
    ev = synth.generate_events(n_events, seed=0)
    with open(path, "wb") as fh:
        for block in F.sessions_text_fast(ev):
            fh.write(block)
    m = {"target_events": n_events, "bytes": os.path.getsize(path), "events": int(ev.n_events), "lines": int(ev.n_sessions)}
    with open(meta, "w") as fh:
        json.dump(m, fh)
    return m["bytes"], m["events"], m["lines"], time.perf_counter() - t0


def prefix_of_lines(path, n_lines):
    """the first n_lines whole lines of the file as bytes"""
    out, got = [], 0
    with open(path, "rb") as fh:
        while got < n_lines:
            buf = fh.read(64 << 20)
            if not buf:
                break
            c = buf.count(b"\n")
            if got + c < n_lines:
                out.append(buf)
                got += c
                continue
            pos = -1
            for _ in range(n_lines - got):
                pos = buf.index(b"\n", pos + 1)
            out.append(buf[:pos + 1])
            got = n_lines
    return b"".join(out), got


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=("device", "file", "host"), required=True)
    ap.add_argument("--events", type=int, default=20_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-lines", type=int, default=200_000)
    ap.add_argument("--text", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "etl_timing.json"))
    a = ap.parse_args()
    path = a.text or os.path.join(tempfile.gettempdir(), f"etl_timing_{a.events}.jsonl")
    n_bytes, n_events, n_lines, t_write = ensure_text(path, a.events)
    key = f"events_{n_events}"
    head = {"text_bytes": n_bytes, "events": n_events, "lines": n_lines, "bytes_per_event": n_bytes / max(n_events, 1)}
    if t_write:
        head["host_generate_and_write_text_s"] = t_write

    if a.step == "host":
        import etl_oracle as O
        data, got = prefix_of_lines(path, a.host_lines)
        t0 = time.perf_counter()
        cols = O.pandas_sessions(io.BytesIO(data))
        t_pd = time.perf_counter() - t0
        t0 = time.perf_counter()
        n = 0
        for ln in data.splitlines():
            n += len(json.loads(ln)["events"])
        t_js = time.perf_counter() - t0
        assert n == len(cols["aid"])
        scale = n_bytes / len(data)
        part = dict(head)
        part["host"] = {
            "timer": "host wall clock, one run, one CPU thread",
            "prefix_lines": got, "prefix_bytes": len(data), "prefix_events": n,
            "pandas_read_json_and_column_loop_s": t_pd, "json_loads_per_line_s": t_js,
            "pandas_bytes_per_s": len(data) / t_pd, "json_loads_bytes_per_s": len(data) / t_js,
            "extrapolated_to_the_whole_text_s": {"pandas_read_json_and_column_loop": t_pd * scale,
                                                 "json_loads_per_line": t_js * scale,
                                                 "note": "an extrapolation by bytes from the prefix, not a measurement"},
            "outside_figure": "the reference notes 'ETA ~15min' for the whole data set (etl/jsonl_to_parquet.py:93) on "
                              "hardware it does not name; quoted, not compared"}
        merge(a.out, key, part)
        return

    import torch  # before the package loads libottohip.so: one HIP runtime in the process, torch's
    from otto_recommender_amd import _lib, etl
    ctx = _lib.context(0)

    if a.step == "device":
        limit = (1 << 31) - 1
        with open(path, "rb") as fh:
            data = fh.read(limit)
        if len(data) == limit:
            data = data[:data.rfind(b"\n") + 1]
        dev = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
        n = len(data)
        ctx.set_timing(True)
        lib = _lib.load()
        recs, totals = [], []
        for _ in range(a.reps + 1):  # the first run warms up (workspace allocation)
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            cols, rpl, L = etl._parse_piece(ctx, 0, dev, n, 0)
            e.record()
            torch.cuda.synchronize()
            totals.append(s.elapsed_time(e))
            recs.append({k: ms for k, ms, _ in ctx.timings()})  # the phases of the last call, the parse
        ctx.set_timing(False)
        rows = int(cols[0].numel())
        med = {k: float(np.median([r[k] for r in recs[1:]])) for k in recs[0]}
        ms_call = sum(med.values())
        model = 3.0 * n + 13.0 * rows + 16.0 * rows + 16.0 * L + 24.0 * (n / etl.tile_bytes())
        part = dict(head)
        part["device"] = {
            "timer": "device events of the context around each pass of one ottohip_jsonl_sessions call; median of "
                     f"{a.reps} runs after one warm-up; count_and_sessions_ms: device events around the sizing call "
                     "(ottohip_jsonl_count: one more classify and scan), the parse call and the host's read of the "
                     "rows per line",
            "piece_bytes": n, "rows": rows, "lines": int(L), "tile_bytes": etl.tile_bytes(),
            "phase_ms": med, "sessions_call_ms": ms_call, "count_and_sessions_ms": float(np.median(totals[1:])),
            "bytes_per_s": n / ms_call * 1e3, "events_per_s": rows / ms_call * 1e3,
            "byte_model": "text read by each of the three passes that read it (classify, locate, parse) + 13 B per row "
                          "written + 8 B of positions per event and per line written and read once + 24 B per tile "
                          "(count written, scanned, base read)",
            "model_bytes": model, "fraction_of_8_TB_per_s": model / (ms_call * 1e-3) / HBM_BYTES_PER_S}
        merge(a.out, key, part)
        return

    # --step file
    small, _ = prefix_of_lines(path, 1000)
    etl.parse_bytes(small, ctx=ctx)  # context, streams, kernels loaded
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ev = etl.events_from_jsonl(path, ctx=ctx)
    torch.cuda.synchronize()
    t_ev = time.perf_counter() - t0
    assert ev.n_events == n_events and ev.n_sessions == n_lines
    del ev
    with tempfile.TemporaryDirectory() as out_dir:
        t0 = time.perf_counter()
        paths = etl.transform_jsonl_to_parquet(path, out_dir, ctx=ctx)
        t_pq = time.perf_counter() - t0
        pq_bytes = sum(os.path.getsize(p) for p in paths)
    part = dict(head)
    part["file"] = {
        "timer": "host wall clock, one run after a 1000-line warm-up; the file was written or read just before, so it "
                 "comes from the page cache",
        "piece_bytes": etl.PIECE_BYTES,
        "events_from_jsonl_s": t_ev, "events_from_jsonl_bytes_per_s": n_bytes / t_ev,
        "transform_jsonl_to_parquet_s": t_pq, "parquet_files": len(paths), "parquet_bytes": pq_bytes}
    merge(a.out, key, part)


if __name__ == "__main__":
    main()
