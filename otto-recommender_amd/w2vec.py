"""Word2Vec top-K similarity lookup on MI355X behind the reference's signatures.

Mirrors model/w2vec_aids.py:
  load_index_faiss_ivff(embeddings, model_name)                           :98-110
  get_top_k_similar_faiss(words_q, words, map_word_embedding, index, k)   :125-173
  retrieve_w2vec_knns_via_faiss_index(model_name, k, first_n_aids)        :176-206
The index scans every row (bf16 MFMA scores keep 24 candidates per query, an exact fp32 rerank orders
them; see csrc/knn.hip): a true neighbour is certain to be returned when fewer than 24 other rows come
within the bf16 scores' error of it (DESIGN.md §5 kNN states the bound and the envelope in which this is
an exact search: embeddings centred near the origin, not tightly clustered). The reference's faiss
IVFFlat (nlist 100, nprobe 3) probes 3 of 100 lists. The embeddings are an input of these functions (a
vocabulary `words` in index_to_key order + vectors); train_w2vec_model below produces them on the device.

That default search is exact inside the envelope only. `exact=True` (KnnIndex.search and every function
below) is exact for every input: the index is packed centred (`center=True`), the main pass keeps every row
within a derived margin of the running 24th-best score, all of them that can be among the top k are reranked
in fp32, and a query with more than 512 such rows is answered by an fp32 scan of all rows (DESIGN.md §5 kNN,
"Exact mode"). It costs time only where the data is hostile; `KnnIndex.last_exact_stats` says how often.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

from . import _lib
from . import config
from .train import MASK64, mix  # splitmix64's finaliser: the draw of csrc/downsample.hip, train.hip and w2v.hip


class KnnIndex:
    """Device index over item embeddings (fp32 [V, dim] kept resident + packed bf16 operand).
    center=True packs the rows minus their column mean (the operand of the exact search; distances and the
    default search's results on centred data do not depend on it)."""

    def __init__(self, embeddings, ctx=None, stream=None, center: bool = False):
        import torch
        _lib.require_gpu()
        self.ctx = ctx or _lib.context()
        dev = torch.device("cuda", self.ctx.device)
        emb = embeddings if isinstance(embeddings, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(embeddings))
        self.emb = emb.to(dev, torch.float32).contiguous()
        self.n_items, self.dim = (int(x) for x in self.emb.shape)
        self.h = ctypes.c_void_p()
        self.center = bool(center)
        self.last_exact_stats = None
        lib = _lib.load()
        if center:
            _lib.check(lib.ottohip_knn_index_create_ex(self.ctx.h, _lib.ptr(self.emb), self.n_items, self.dim,
                                                       _lib.KNN_CENTER, ctypes.byref(self.h), _lib.stream_handle(stream)))
        else:
            _lib.check(lib.ottohip_knn_index_create(self.ctx.h, _lib.ptr(self.emb), self.n_items, self.dim,
                                                    ctypes.byref(self.h), _lib.stream_handle(stream)))

    def free(self):
        if self.h:
            _lib.load().ottohip_knn_index_free(self.h)
            self.h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

    def search(self, query_rows=None, n_q=None, k: int = 20, stream=None, exact: bool = False):
        """k nearest rows per query row in ascending fp32 squared L2, ties by row index: returns torch
        (idx:int32 [n_q, k], d2:float32 [n_q, k]) on the device; slots past the index size are -1 / inf.
        The rows are the best k of 24 candidates chosen by bf16 scores (module docstring), so "ties by row
        index" holds among at most 24 equal-score candidates: of more identical rows, some k come back.
        exact=True: the exact search (module docstring): the same outputs for every input, ties by row index
        among all equal rows; self.last_exact_stats = {"n_overflow", "max_appends", "sum_appends"} of the call."""
        import torch
        dev = self.emb.device
        if query_rows is None:
            n = self.n_items if n_q is None else int(n_q)
            qr = None
        else:
            qr = torch.as_tensor(query_rows, dtype=torch.int32).to(dev).contiguous()
            n = int(qr.numel())
        idx = torch.empty((n, k), dtype=torch.int32, device=dev)
        d2 = torch.empty((n, k), dtype=torch.float32, device=dev)
        if exact:
            st = _lib.KnnExactStats()
            _lib.check(_lib.load().ottohip_knn_topk_exact(self.ctx.h, self.h, _lib.ptr(qr), n, k, _lib.ptr(idx),
                                                          _lib.ptr(d2), ctypes.byref(st), _lib.stream_handle(stream)))
            self.last_exact_stats = {"n_overflow": int(st.n_overflow), "max_appends": int(st.max_appends),
                                     "sum_appends": int(st.sum_appends)}
            return idx, d2
        _lib.check(_lib.load().ottohip_knn_topk(self.ctx.h, self.h, _lib.ptr(qr), n, k, _lib.ptr(idx), _lib.ptr(d2),
                                                _lib.stream_handle(stream)))
        return idx, d2


def load_index_faiss_ivff(embeddings, model_name: str | None = None, exact: bool = False) -> KnnIndex:
    """w2vec_aids.py:98-110 (the nlist/nprobe of config.W2VEC_MODELS do not apply: every row is scanned).
    exact=True: a centred index, the operand of the exact search."""
    return KnnIndex(embeddings, center=exact)


def word_rows(words, words_q) -> np.ndarray:
    """Row of each query word in the vocabulary `words` (-1 = not in it): the index lookup of
    w2vec_aids.py:156-163 as one sorted search (any vocabulary size, no per-word host loop).
    A word listed more than once maps to its LAST row, as the reference's dict(zip(words, ...))
    keeps the last value of a duplicated key."""
    words = np.asarray(words, np.int64)
    wq = np.asarray(words_q, np.int64)
    if len(words) == 0:
        return np.full(len(wq), -1, np.int64)
    order = np.argsort(words, kind="stable")
    sw = words[order]
    pos = np.searchsorted(sw, wq, side="right") - 1  # the last of equal words (stable order)
    hit = pos >= 0
    hit[hit] = sw[pos[hit]] == wq[hit]
    return np.where(hit, order[np.maximum(pos, 0)], -1).astype(np.int64)


def get_top_k_similar_faiss(words_q, words, map_word_embedding=None, index_faiss_ivff=None, k: int = 20,
                            return_itself: bool = True, exact: bool = False):
    """w2vec_aids.py:125-173. words_q: query aids; words: the vocabulary (row order of the
    index); index_faiss_ivff: a KnnIndex over embeddings in `words` order (map_word_embedding
    is accepted for signature compatibility; rows come from `words`). Words without an
    embedding are dropped as in :156-163. Returns pandas DataFrame
    [aid:int32, aid_next:int32, dist_w2vec:int32, rank_w2vec:int8] (dist_w2vec = trunc of the
    squared L2 distance, :169; rank_w2vec = ordinal position 1..k clipped at 127, :170-171).
    exact=True: the exact search on the given index (best built with load_index_faiss_ivff(exact=True))."""
    import pandas as pd
    import torch
    index = index_faiss_ivff
    if index is None:
        raise ValueError("index_faiss_ivff (a KnnIndex) is required")
    words = np.asarray(words, np.int64)
    wq = np.asarray(words_q, np.int64)
    rows = word_rows(words, wq)
    found = rows >= 0
    rows, wq = rows[found], wq[found]
    if len(rows) == 0:
        return pd.DataFrame({"aid": np.zeros(0, np.int32), "aid_next": np.zeros(0, np.int32),
                             "dist_w2vec": np.zeros(0, np.int32), "rank_w2vec": np.zeros(0, np.int8)})
    res = knn_table(index, torch.from_numpy(words.astype(np.int32)), torch.from_numpy(rows.astype(np.int32)), k,
                    exact=exact)
    return pd.DataFrame({c: t.cpu().numpy() for c, t in res.items()})


def knn_table(index: KnnIndex, words, query_rows, k: int = 20, stream=None, exact: bool = False) -> dict:
    """Device form of the output of :167-171 for query rows: dict of torch columns
    aid, aid_next (int32), dist_w2vec (int32, truncated squared L2), rank_w2vec (int8).
    exact=True: the rows of the exact search (KnnIndex.search)."""
    import torch
    dev = index.emb.device
    words = torch.as_tensor(words).to(dev, torch.int32)
    qr = torch.as_tensor(query_rows).to(dev, torch.int32)
    idx, d2 = index.search(qr, k=k, stream=stream, exact=exact)
    n = qr.numel()
    valid = idx >= 0
    aid = words[qr.long()].view(n, 1).expand(n, k)
    nxt = torch.where(valid, words[idx.clamp(min=0).long()], torch.full_like(idx, -1))
    dist = torch.trunc(d2).to(torch.int32)
    rank = torch.arange(1, k + 1, device=dev, dtype=torch.int32).clamp(max=127).to(torch.int8).view(1, k).expand(n, k)
    m = valid.reshape(-1)
    return {"aid": aid.reshape(-1)[m].contiguous(), "aid_next": nxt.reshape(-1)[m].contiguous(),
            "dist_w2vec": dist.reshape(-1)[m].contiguous(), "rank_w2vec": rank.reshape(-1)[m].contiguous()}


def retrieve_w2vec_knns_via_faiss_index(embeddings, words, k: int | None = None, first_n_aids: int | None = None,
                                        cache_file: str | None = None, exact: bool = False):
    """w2vec_aids.py:176-206 with the trained model replaced by its outputs (vocabulary `words`
    in index_to_key order and `embeddings`): neighbours of the first `first_n_aids` words,
    cached to parquet like :191-204. exact=True: a centred index and the exact search."""
    import pandas as pd
    k = config.W2VEC_K if k is None else k
    first_n_aids = config.W2VEC_SEARCH_SIMILAR_FOR_FIRST_N_AIDS if first_n_aids is None else first_n_aids
    if cache_file and os.path.exists(cache_file):
        return pd.read_parquet(cache_file)
    index = KnnIndex(embeddings, center=exact)
    n_q = min(first_n_aids, index.n_items)
    import torch
    res = knn_table(index, torch.as_tensor(np.asarray(words, np.int32)), torch.arange(n_q, dtype=torch.int32), k,
                    exact=exact)
    df = pd.DataFrame({c: t.cpu().numpy() for c, t in res.items()})
    index.free()
    if cache_file:
        os.makedirs(os.path.dirname(cache_file) or ".", exist_ok=True)
        df.to_parquet(cache_file)
    return df


# ---------------------------------------------------------------------------------------------------------------
# Training (model/w2vec_aids.py:18-70): CBOW with negative sampling as synchronous mini-batches on the device.
# DESIGN.md "Word2Vec trainer" is the definition; csrc/w2v.hip runs it. The functions below that take numpy
# arrays are host plumbing (vocabulary, tables, initial weights) and need no GPU.
W2V_MAX_DIM, W2V_MAX_WINDOW, W2V_MAX_NEGATIVE = 128, 31, 32


def draw(seed: int, epoch: int, slot: int, index: int) -> int:
    """The trainer's counter-based draw: slot 0 keep, 1 reduced window, 2 + j negative j; index: the event's place
    in the CSR, so no draw depends on the compaction or on the batch size."""
    return mix(mix(mix(int(seed) & MASK64) ^ ((int(epoch) << 32) | int(slot))) ^ int(index))


def _mix_np(z):
    """mix over a uint64 array"""
    from .synth import _mix
    with np.errstate(over="ignore"):
        return _mix(np.asarray(z, np.uint64) + np.uint64(0x9E3779B97F4A7C15))


def vocabulary(counts_by_aid, min_count: int = 5):
    """(index_to_key, counts) from the per-aid event counts: the aids with count >= min_count, by count descending,
    ties by aid ascending."""
    c = np.asarray(counts_by_aid, np.int64)
    keys = np.flatnonzero(c >= max(int(min_count), 1))
    cnt = c[keys]
    order = np.lexsort((keys, -cnt))
    return keys[order].astype(np.int64), cnt[order].astype(np.int64)


def keep_thresholds(counts, sample: float = 1e-3) -> np.ndarray:
    """uint32 of the kept probability (sqrt(c / (sample T)) + 1) (sample T) / c capped at 1, T the kept words' total
    count: an event is kept when the high 32 bits of its draw are <= the threshold. sample = 0 keeps everything."""
    counts = np.asarray(counts, np.float64)
    if sample <= 0:
        return np.full(len(counts), 0xFFFFFFFF, np.uint32)
    if sample > 1:
        raise ValueError("sample: a share of the corpus in [0, 1]")
    tc = float(sample) * float(counts.sum())
    p = (np.sqrt(counts / tc) + 1.0) * (tc / counts)
    thr = np.minimum(np.floor(np.minimum(p, 1.0) * 4294967296.0), 4294967295.0)
    return np.where(p >= 1.0, 4294967295.0, thr).astype(np.uint32)


def negative_table(counts, ns_exponent: float = 0.75) -> np.ndarray:
    """31-bit cumulative table of count^ns_exponent (uint32 [V], last entry 2^31): a 31-bit draw x picks the first
    row whose entry is > x."""
    cs = np.cumsum(np.asarray(counts, np.float64) ** float(ns_exponent))
    cum = np.rint(cs / cs[-1] * 2147483648.0)
    cum[-1] = 2147483648.0
    return cum.astype(np.uint32)


def sigmoid_table(n_sig: int = config.W2VEC_SIGMOID_ENTRIES, max_exp: float = config.W2VEC_MAX_EXP) -> np.ndarray:
    """fp32 sigmoid at the n_sig left edges of equal cells of [-max_exp, max_exp)"""
    x = (np.arange(n_sig, dtype=np.float64) / n_sig * 2.0 - 1.0) * max_exp
    return (1.0 / (1.0 + np.exp(-x))).astype(np.float32)


def initial_weights(seed: int, n_vocab: int, dim: int) -> np.ndarray:
    """syn0[r][d] = (u - 0.5) / dim in fp32, u the top 24 bits of a draw on (seed, r, d) times 2^-24"""
    sm = mix(int(seed) & MASK64)
    out = np.empty((n_vocab, dim), np.float32)
    r = np.arange(n_vocab, dtype=np.uint64)
    for d in range(dim):
        u = _mix_np(np.uint64(mix(sm ^ ((0xFFFFFFFF << 32) | d))) ^ r) >> np.uint64(40)
        out[:, d] = (u.astype(np.float32) * np.float32(2.0 ** -24) - np.float32(0.5)) / np.float32(dim)
    return out


def _type_mask(types) -> int:
    if types is None:
        return 0b111
    m = 0
    for t in types:
        t = config.TYPE2ID.get(t, t) if isinstance(t, str) else t
        if not 0 <= int(t) < 3:
            raise ValueError(f"types: {t!r} is not an event type")
        m |= 1 << int(t)
    return m


def _device_events(events):
    from .covis import DeviceEvents
    return events if isinstance(events, DeviceEvents) else DeviceEvents.from_host(events)


def load_sessions_as_sentences(events, types=None):
    """w2vec_aids.py:18-39 over resident events: a pandas DataFrame [session (index in the CSR), n_aid, sentence] with
    one row per session that has an event of `types` (None = all), the sentence its aids in event order."""
    import pandas as pd
    import torch
    ev = _device_events(events)
    mask = _type_mask(types)
    ty = ev.type.to(torch.int64)
    keep = ((torch.tensor(mask, device=ty.device) >> ty) & 1).bool()
    lens = ev.offsets[1:] - ev.offsets[:-1]
    sid = torch.repeat_interleave(torch.arange(ev.n_sessions, device=ty.device), lens)[keep]
    aid = ev.aid[keep].cpu().numpy()
    cnt = torch.bincount(sid, minlength=ev.n_sessions).cpu().numpy()
    has = np.flatnonzero(cnt)
    cuts = np.cumsum(cnt[has])[:-1]
    return pd.DataFrame({"session": has.astype(np.int64), "n_aid": cnt[has].astype(np.uint16),
                         "sentence": np.split(aid, cuts) if len(has) else []})


class KeyedVectors:
    """The two attributes the reference reads of gensim's: index_to_key (aids, most frequent first) and vectors."""

    def __init__(self, index_to_key, vectors):
        self.index_to_key = np.asarray(index_to_key, np.int64)
        self.vectors = np.ascontiguousarray(vectors, np.float32)


class Word2VecModel:
    """A trained model: .wv.index_to_key, .wv.vectors, .params, .save(path) (an .npz of its own, not gensim's pickle)."""

    def __init__(self, index_to_key, vectors, params: dict | None = None):
        self.wv = KeyedVectors(index_to_key, vectors)
        self.params = dict(params or {})

    def save(self, path: str):
        import json
        os.makedirs(os.path.dirname(os.path.abspath(path)) or ".", exist_ok=True)
        with open(path, "wb") as f:  # a file object: numpy appends no suffix to the name
            np.savez(f, index_to_key=self.wv.index_to_key, vectors=self.wv.vectors,
                     params=np.frombuffer(json.dumps(self.params, sort_keys=True).encode(), np.uint8))

    @staticmethod
    def load(path: str) -> "Word2VecModel":
        import json
        with np.load(path) as z:
            return Word2VecModel(z["index_to_key"], z["vectors"], json.loads(bytes(z["params"]).decode()))


def _w2v_params(params: dict) -> dict:
    p = dict(config.W2VEC_DEFAULTS)
    p.update({"vector_size": config.W2VEC_VECTOR_SIZE, "window": 5, "min_count": 5, "workers": 1,
              "batch_positions": config.W2VEC_BATCH_POSITIONS})
    unknown = set(params) - set(p)
    if unknown:
        raise TypeError(f"train_w2vec_model: unknown parameters {sorted(unknown)}")
    p.update(params)
    if p["sg"] != 0:
        raise NotImplementedError("sg=1 (skip-gram) is not supported: the trainer is CBOW")
    if p["hs"] != 0:
        raise NotImplementedError("hs=1 (hierarchical softmax) is not supported: the trainer samples negatives")
    if p["cbow_mean"] != 1:
        raise NotImplementedError("cbow_mean=0 is not supported: the context is averaged")
    if not p["shrink_windows"]:
        raise NotImplementedError("shrink_windows=False is not supported: every position draws its window")
    if not 1 <= int(p["vector_size"]) <= W2V_MAX_DIM:
        raise ValueError(f"vector_size: 1..{W2V_MAX_DIM} (two dims per lane of a wave)")
    if not 1 <= int(p["window"]) <= W2V_MAX_WINDOW:
        raise ValueError(f"window: 1..{W2V_MAX_WINDOW} (a window's rows sit one per lane)")
    if not 1 <= int(p["negative"]) <= W2V_MAX_NEGATIVE:
        raise ValueError(f"negative: 1..{W2V_MAX_NEGATIVE}")
    if int(p["epochs"]) < 1 or int(p["batch_positions"]) < 1:
        raise ValueError("epochs and batch_positions: at least 1")
    return p


def w2v_abi_params(p: dict, type_mask: int = 0b111) -> "_lib.W2vParams":
    return _lib.W2vParams(dim=int(p["vector_size"]), window=int(p["window"]), negative=int(p["negative"]),
                          n_sig=int(p.get("n_sig", config.W2VEC_SIGMOID_ENTRIES)), epochs=int(p["epochs"]),
                          shift=int(p.get("shift", config.W2VEC_FIXED_SHIFT)),
                          batch_positions=int(p["batch_positions"]), seed=int(p["seed"]) & MASK64,
                          alpha=float(p["alpha"]), min_alpha=float(p["min_alpha"]),
                          max_exp=float(p.get("max_exp", config.W2VEC_MAX_EXP)), type_mask=int(type_mask))


class Word2VecTrainer:
    """The device trainer behind train_w2vec_model (ottohip_w2v_*): vocabulary and tables from the events, then
    epoch(e) for e = 0 .. epochs - 1 in order, vectors() and free(). params: the resolved dict of _w2v_params."""

    def __init__(self, events, types=None, n_items: int | None = None, ctx=None, params: dict | None = None):
        import torch
        p = self.params = _w2v_params(params or {})
        self.types = None if types is None else list(types)
        self.mask = _type_mask(types)
        _lib.require_gpu()
        ev = self.events = _device_events(events)
        self.ctx = ctx or _lib.context()
        dev = self.device = ev.aid.device
        self.dim = int(p["vector_size"])
        ty = ev.type.to(torch.int64)
        sel = ((torch.tensor(self.mask, device=dev) >> ty) & 1).bool()
        aid_sel = ev.aid[sel].to(torch.int64)
        if aid_sel.numel() and int(aid_sel.min()) < 0:
            raise ValueError("events: negative aid")
        self.n_items = int(n_items) if n_items is not None else (int(ev.aid.max()) + 1 if ev.n_events else 0)
        counts_by_aid = torch.bincount(aid_sel[aid_sel < self.n_items], minlength=self.n_items).cpu().numpy()
        self.index_to_key, self.counts = vocabulary(counts_by_aid, p["min_count"])
        V = self.n_vocab = len(self.index_to_key)
        self.h = ctypes.c_void_p()
        if V == 0:
            return
        row_of_aid = np.full(self.n_items, -1, np.int32)
        row_of_aid[self.index_to_key] = np.arange(V, dtype=np.int32)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        # device arrays the handle reads for its whole life (uint32 tables travel as their int32 bits)
        self.row_of_aid, self.keep_thr = up(row_of_aid), up(keep_thresholds(self.counts, p["sample"]).view(np.int32))
        self.cum, self.sig = up(negative_table(self.counts, p["ns_exponent"]).view(np.int32)), up(sigmoid_table())
        init = up(initial_weights(p["seed"], V, self.dim))
        self._abi_ev, self.abi_params = ev.abi(), w2v_abi_params(p, self.mask)
        _lib.check(_lib.load().ottohip_w2v_create(self.ctx.h, ctypes.byref(self._abi_ev), _lib.ptr(self.row_of_aid),
                                                  self.n_items, _lib.ptr(self.keep_thr), _lib.ptr(self.cum), V,
                                                  _lib.ptr(self.sig), _lib.ptr(init), ctypes.byref(self.abi_params),
                                                  ctypes.byref(self.h)))

    def epoch(self, e: int, stream=None):
        """(kept positions, batches) of epoch e"""
        nk, nb = ctypes.c_int64(), ctypes.c_int64()
        _lib.check(_lib.load().ottohip_w2v_epoch(self.h, int(e), ctypes.byref(nk), ctypes.byref(nb),
                                                 _lib.stream_handle(stream)))
        return int(nk.value), int(nb.value)

    def vectors(self, with_syn1neg: bool = False, stream=None):
        """syn0 (and syn1neg) as device tensors [n_vocab, dim]"""
        import torch
        out = [torch.empty((self.n_vocab, self.dim), dtype=torch.float32, device=self.device)
               for _ in range(2 if with_syn1neg else 1)]
        if self.n_vocab:
            _lib.check(_lib.load().ottohip_w2v_vectors(self.h, _lib.ptr(out[0]), _lib.ptr(out[1]) if with_syn1neg else None,
                                                       _lib.stream_handle(stream)))
        return tuple(out) if with_syn1neg else out[0]

    def free(self):
        if self.h:
            _lib.load().ottohip_w2v_free(self.h)
            self.h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def train_w2vec_model(events, types=None, n_items: int | None = None, ctx=None, stream=None, stats: dict | None = None,
                      **params) -> Word2VecModel:
    """w2vec_aids.py:56-70 on the device: Word2Vec(sentences, vector_size, window, min_count, ...) over the sessions of
    `events` (covis.DeviceEvents, or host synth.Events) restricted to `types`. Parameters are gensim's names
    (config.W2VEC_DEFAULTS; plus batch_positions); sg=1, hs=1 and cbow_mean=0 raise NotImplementedError, workers is
    accepted and unused. Two calls with the same input return the same bytes. stats (optional dict) receives
    n_kept / n_batches per epoch."""
    t = Word2VecTrainer(events, types, n_items, ctx, params)
    p = t.params
    try:
        for e in range(int(p["epochs"]) if t.n_vocab else 0):
            nk, nb = t.epoch(e, stream)
            if stats is not None:
                stats.setdefault("n_kept", []).append(nk)
                stats.setdefault("n_batches", []).append(nb)
        vectors = t.vectors(stream=stream).cpu().numpy()
    finally:
        t.free()
    return Word2VecModel(t.index_to_key, vectors, {k: p[k] for k in sorted(p)} | {"types": t.types})


def get_model_file(model_name: str) -> str:
    """w2vec_aids.py:42-43 (an .npz here)"""
    return f"{config.DIR_ARTIFACTS}/word2vec/{model_name}.npz"


def load_w2vec_model(path_or_name: str, events=None, types=None, use_cache: bool | None = None, **params) -> Word2VecModel:
    """w2vec_aids.py:46-53: the cached model file when config.W2VEC_USE_CACHE and it exists, else a model trained
    from `events` and saved there. A name of config.W2VEC_MODELS supplies the file (get_model_file), `types` and
    the parameters; anything else is taken as the file's path."""
    cfg = config.W2VEC_MODELS.get(path_or_name)
    path = get_model_file(path_or_name) if cfg is not None else path_or_name
    use_cache = config.W2VEC_USE_CACHE if use_cache is None else use_cache
    if use_cache and os.path.exists(path):
        return Word2VecModel.load(path)
    if events is None:
        raise FileNotFoundError(f"{path}: no cached model, and no events to train one from")
    if cfg is not None:
        types = cfg.get("types") if types is None else types
        params = {**cfg["params"], **params}
    model = train_w2vec_model(events, types=types, **params)
    model.save(path)
    return model


def retrieve_w2vec_knns(model, k: int | None = None, first_n_aids: int | None = None, events=None, types=None,
                        cache_file: str | None = None, exact: bool = False, **params):
    """w2vec_aids.py:176-206 from the model on: `model` is a Word2VecModel, or a name / path for load_w2vec_model
    (trained from `events` when no cached file exists). Neighbours of the first `first_n_aids` words as
    get_top_k_similar_faiss returns them: [aid, aid_next, dist_w2vec, rank_w2vec]."""
    if isinstance(model, str):
        cfg = config.W2VEC_MODELS.get(model, {})
        k = cfg.get("k") if k is None else k
        first_n_aids = cfg.get("first_n_aids") if first_n_aids is None else first_n_aids
        model = load_w2vec_model(model, events=events, types=types, **params)
    return retrieve_w2vec_knns_via_faiss_index(model.wv.vectors, model.wv.index_to_key, k=k, first_n_aids=first_n_aids,
                                               cache_file=cache_file, exact=exact)


# ---- the trainer's stages on their own (parity tests, tools/w2v_timing.py): device tensors in and out
def w2v_compact(events, row_of_aid, keep_thr, type_mask: int, seed: int, epoch: int, ctx=None, stream=None):
    """One epoch's compaction (ottohip_w2v_compact): (rows, orig, sid, offsets) as device tensors cut to the kept
    count; row_of_aid int32 [n_items] and keep_thr (uint32 bits, [n_vocab]) are device tensors."""
    import torch
    ev = _device_events(events)
    ctx = ctx or _lib.context()
    dev = ev.aid.device
    n = max(ev.n_events, 1)
    rows, orig, sid = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(3))
    off = torch.empty(ev.n_sessions + 1, dtype=torch.int64, device=dev)
    nk = ctypes.c_int64()
    abi_ev = ev.abi()
    _lib.check(_lib.load().ottohip_w2v_compact(ctx.h, ctypes.byref(abi_ev), _lib.ptr(row_of_aid), int(row_of_aid.numel()),
                                               _lib.ptr(keep_thr), int(keep_thr.numel()), int(type_mask),
                                               int(seed) & MASK64, int(epoch), _lib.ptr(rows), _lib.ptr(orig),
                                               _lib.ptr(sid), _lib.ptr(off), ctypes.byref(nk), _lib.stream_handle(stream)))
    k = int(nk.value)
    return rows[:k], orig[:k], sid[:k], off


def w2v_batch(rows, orig, sid, offsets, b0: int, b1: int, syn0, syn1neg, cum, sig, abi_params, epoch: int, lr: float,
              acc0, acc1, flag0, flag1, ctx=None, stream=None):
    """The kept positions [b0, b1) from the given weights (ottohip_w2v_batch): adds into acc0 / acc1 (int64
    [n_vocab, dim]) and sets flag0 / flag1 (uint8 [n_vocab]). All arguments are device tensors."""
    ctx = ctx or _lib.context()
    _lib.check(_lib.load().ottohip_w2v_batch(ctx.h, _lib.ptr(rows), _lib.ptr(orig), _lib.ptr(sid), _lib.ptr(offsets),
                                             int(rows.numel()), int(offsets.numel()) - 1, int(b0), int(b1),
                                             _lib.ptr(syn0), _lib.ptr(syn1neg), int(syn0.shape[0]), _lib.ptr(cum),
                                             _lib.ptr(sig), ctypes.byref(abi_params), int(epoch), float(lr),
                                             _lib.ptr(acc0), _lib.ptr(acc1), _lib.ptr(flag0), _lib.ptr(flag1),
                                             _lib.stream_handle(stream)))


def w2v_apply(weights, acc, flag, shift: int = config.W2VEC_FIXED_SHIFT, ctx=None, stream=None):
    """weights += the fixed-point sums of the flagged rows, in place; sums and flags are zeroed (ottohip_w2v_apply)"""
    ctx = ctx or _lib.context()
    _lib.check(_lib.load().ottohip_w2v_apply(ctx.h, _lib.ptr(weights), _lib.ptr(acc), _lib.ptr(flag),
                                             int(weights.shape[0]), int(weights.shape[1]), int(shift),
                                             _lib.stream_handle(stream)))
