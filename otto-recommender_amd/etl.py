"""ETL on MI355X behind the reference's function signatures (etl/jsonl_to_parquet.py).

  get_number_of_lines(file_path)                                            :17-20
  transform_jsonl_to_parquet(file_jsonl, out_dir, type_data, chunksize)     :59-84
  run(dir_jsonl, dir_parquet)                                               :95-105 (the __main__ order)
plus the direct routes that skip the parquet round trip:
  events_from_jsonl(file_jsonl) -> DeviceEvents      labels_from_jsonl(file_jsonl) -> DataFrame

The file is read in pieces of whole lines; each piece is uploaded from a pinned buffer on a side stream while the
piece before it is parsed by ottohip_jsonl_sessions / ottohip_jsonl_labels (csrc/etl.hip). The grammar is strict
(ETL): what pandas would coerce or skip is an error here, reported with its line number in the file.
Blank lines are skipped and do not count as lines, as pandas.read_json(lines=True) skips them."""
from __future__ import annotations

import ctypes
import io
import os
from pathlib import Path

import numpy as np

from . import _lib
from . import config

KINDS = {"sessions": 0, "labels": 1}
PIECE_BYTES = 256 << 20


def get_number_of_lines(file_path) -> int:
    """Lines of the file, a last line without its line end included (etl/jsonl_to_parquet.py:17-20)."""
    n, last = 0, b"\n"
    with open(file_path, "rb") as fp:
        while True:
            buf = fp.read(16 << 20)
            if not buf:
                break
            n += buf.count(b"\n")
            last = buf[-1:]
    return n + (last != b"\n")


def tile_bytes() -> int:
    """Bytes of text one wave classifies (the tile of csrc/etl.hip)."""
    return int(_lib.load().ottohip_jsonl_tile_bytes())


def _pieces(fp, piece_bytes: int):
    """Whole-line pieces of at most piece_bytes; a piece grows while it holds no line end."""
    piece_bytes = max(int(piece_bytes), 1)
    carry = b""
    while True:
        buf = fp.read(piece_bytes - len(carry) if len(carry) < piece_bytes else piece_bytes)
        if not buf:
            if carry:
                yield carry
            return
        data = carry + buf  # carry never holds a line end
        cut = (data.rfind(b"\n") if len(data) <= piece_bytes else data.find(b"\n", len(carry))) + 1
        if cut == 0:
            carry = data
            continue
        yield data[:cut]
        carry = data[cut:]


class _Uploader:
    """Two pinned host buffers and two device buffers; copies run on a side stream."""

    def __init__(self, dev):
        import torch
        self.dev = dev
        self.stream = torch.cuda.Stream(device=dev)
        self.pin = [None, None]
        self.buf = [None, None]
        self.done = [None, None]
        self.i = 0

    def put(self, data: bytes):
        import torch
        i, n = self.i, len(data)
        self.i ^= 1
        if self.done[i] is not None:
            self.done[i].synchronize()  # the buffer's last copy has left the pinned memory
        if self.pin[i] is None or self.pin[i].numel() < n:
            cap = max(n, 4096)
            self.pin[i] = torch.empty(cap, dtype=torch.uint8, pin_memory=True)
            self.buf[i] = torch.empty(cap, dtype=torch.uint8, device=self.dev)
        self.pin[i].numpy()[:n] = np.frombuffer(data, np.uint8)
        self.stream.wait_stream(torch.cuda.current_stream(self.dev))  # the parse that last read this buffer
        with torch.cuda.stream(self.stream):
            self.buf[i][:n].copy_(self.pin[i][:n], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(self.stream)
        self.done[i] = ev
        return self.buf[i], n, ev


def _parse_piece(ctx, kind: int, text, n: int, line_base: int):
    """One resident piece -> (columns in the ABI's order, rows of its non-blank lines, lines of the piece)."""
    import torch
    lib = _lib.load()
    s = _lib.stream_handle()
    n_lines, n_rows = ctypes.c_int64(0), ctypes.c_int64(0)
    _lib.check(lib.ottohip_jsonl_count(ctx.h, _lib.ptr(text), n, kind, ctypes.byref(n_lines), ctypes.byref(n_rows), s))
    L, R = int(n_lines.value), int(n_rows.value)
    dev = text.device
    i32 = lambda: torch.empty(R, dtype=torch.int32, device=dev)
    i8 = lambda: torch.empty(R, dtype=torch.int8, device=dev)
    rpl = torch.empty(L, dtype=torch.int64, device=dev)
    if kind == 0:
        cols = (i32(), i32(), i32(), i8())  # session, aid, ts, type
        _lib.check(lib.ottohip_jsonl_sessions(ctx.h, _lib.ptr(text), n, line_base, *[_lib.ptr(c) for c in cols],
                                              _lib.ptr(rpl), R, L, s))
    else:
        cols = (i32(), i8(), i32())  # session, type, aid
        _lib.check(lib.ottohip_jsonl_labels(ctx.h, _lib.ptr(text), n, line_base, *[_lib.ptr(c) for c in cols],
                                            _lib.ptr(rpl), R, L, s))
    rows = rpl.cpu().numpy()
    return cols, rows[rows >= 0], L


def parse_stream(fp, type_data: str = "sessions", piece_bytes: int = PIECE_BYTES, ctx=None):
    """A binary file object of jsonl text -> (device columns, rows per non-blank line as a host int64 array).
    Columns: (session, aid, ts, type) for 'sessions', (session, type, aid) for 'labels'."""
    import torch
    if type_data not in KINDS:
        raise ValueError(f"type_data={type_data} not recognized, must be 'sessions' or 'labels'")
    _lib.require_gpu()
    kind = KINDS[type_data]
    ctx = ctx or _lib.context()
    dev = torch.device("cuda", ctx.device)
    up = _Uploader(dev)
    it = _pieces(fp, piece_bytes)
    parts, rows, line_base = [], [], 0
    try:
        nxt = next(it, None)
        cur = up.put(nxt) if nxt is not None else None
        while cur is not None:
            nxt = next(it, None)
            ahead = up.put(nxt) if nxt is not None else None  # uploads while this piece is parsed
            text, n, ev = cur
            torch.cuda.current_stream(dev).wait_event(ev)
            cols, r, n_lines = _parse_piece(ctx, kind, text, n, line_base)
            parts.append(cols)
            rows.append(r)
            line_base += n_lines
            cur = ahead
    finally:
        up.stream.synchronize()  # no copy is in flight when the buffers go back to the allocator
    n_cols = 4 if kind == 0 else 3
    dts = (torch.int32, torch.int32, torch.int32, torch.int8) if kind == 0 else (torch.int32, torch.int8, torch.int32)
    if not parts:
        return tuple(torch.empty(0, dtype=dt, device=dev) for dt in dts), np.zeros(0, np.int64)
    cols = tuple(parts[0][c] if len(parts) == 1 else torch.cat([p[c] for p in parts]) for c in range(n_cols))
    return cols, np.concatenate(rows)


def parse_bytes(data: bytes, type_data: str = "sessions", piece_bytes: int | None = None, ctx=None):
    """parse_stream over text held in memory (one piece unless piece_bytes is given)."""
    return parse_stream(io.BytesIO(data), type_data, piece_bytes or max(len(data), 1), ctx)


def chunk_rows(rows_per_line: np.ndarray, chunksize: int) -> np.ndarray:
    """Rows of every chunk of `chunksize` lines (the last chunk may be short)."""
    if len(rows_per_line) == 0:
        return np.zeros(0, np.int64)
    return np.add.reduceat(rows_per_line, np.arange(0, len(rows_per_line), chunksize)).astype(np.int64)


def chunk_names(n_lines: int, chunksize: int) -> list:
    """'{start}_{end}' of every chunk, zero-padded to len(str(n_lines)); end = start + chunksize also for the last,
    short chunk (etl/jsonl_to_parquet.py:81-84)."""
    nd = len(str(n_lines))
    n_chunks = -(-n_lines // chunksize)
    return [f"{str(i * chunksize).zfill(nd)}_{str(i * chunksize + chunksize).zfill(nd)}" for i in range(n_chunks)]


def transform_jsonl_to_parquet(file_jsonl, out_dir, type_data="sessions", chunksize=100000, piece_bytes=PIECE_BYTES,
                               ctx=None) -> list:
    """Writes {out_dir}/{stem}/{start}_{end}.parquet, one file per `chunksize` lines, and returns the paths."""
    import pyarrow as pa
    import pyarrow.parquet as pq
    if type_data not in KINDS:
        raise ValueError(f"type_data={type_data} not recognized, must be 'sessions' or 'labels'")
    dir_parquets = f"{out_dir}/{Path(file_jsonl).stem}"
    os.makedirs(dir_parquets, exist_ok=True)
    with open(file_jsonl, "rb") as fp:
        cols, rpl = parse_stream(fp, type_data, piece_bytes, ctx)
    names = ("session", "aid", "ts", "type") if type_data == "sessions" else ("session", "type", "aid")
    host = [c.cpu().numpy() for c in cols]
    starts = np.concatenate([[0], np.cumsum(chunk_rows(rpl, chunksize))]).astype(np.int64)
    paths = []
    for i, name in enumerate(chunk_names(len(rpl), chunksize)):
        a, b = int(starts[i]), int(starts[i + 1])
        path = f"{dir_parquets}/{name}.parquet"
        pq.write_table(pa.table({k: h[a:b] for k, h in zip(names, host)}), path)
        paths.append(path)
    return paths


def events_from_jsonl(file_jsonl, chunksize=100000, piece_bytes=PIECE_BYTES, ctx=None):
    """The sessions file as DeviceEvents, one file entry per `chunksize` lines: what DeviceEvents.from_parquet gives
    on the files transform_jsonl_to_parquet writes, without writing them."""
    from .covis import DeviceEvents
    with open(file_jsonl, "rb") as fp:
        (session, aid, ts, type_), rpl = parse_stream(fp, "sessions", piece_bytes, ctx)
    file_rows = chunk_rows(rpl, chunksize)
    return DeviceEvents.from_columns(session, aid, ts, type_, file_rows=list(file_rows) if len(file_rows) else None,
                                     device=session.device.index, ctx=ctx)


def labels_from_jsonl(file_jsonl, piece_bytes=PIECE_BYTES, ctx=None):
    """The labels file as a DataFrame[session:int32, type:int8, aid:int32], one row per aid in order of appearance."""
    import pandas as pd
    with open(file_jsonl, "rb") as fp:
        (session, type_, aid), _ = parse_stream(fp, "labels", piece_bytes, ctx)
    return pd.DataFrame({"session": session.cpu().numpy(), "type": type_.cpu().numpy(), "aid": aid.cpu().numpy()})


def run(dir_jsonl, dir_parquet):
    """The reference's __main__ (etl/jsonl_to_parquet.py:95-105): the optional files are skipped when absent."""
    transform_jsonl_to_parquet(f"{dir_jsonl}/test_sessions.jsonl", dir_parquet)
    transform_jsonl_to_parquet(f"{dir_jsonl}/train_sessions.jsonl", dir_parquet)
    if os.path.exists(f"{dir_jsonl}/test_labels.jsonl"):
        transform_jsonl_to_parquet(f"{dir_jsonl}/test_labels.jsonl", dir_parquet, "labels")
    if os.path.exists(f"{dir_jsonl}/test_sessions_full.jsonl"):
        transform_jsonl_to_parquet(f"{dir_jsonl}/test_sessions_full.jsonl", dir_parquet)
