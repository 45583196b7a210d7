"""numpy restatement of the Word2Vec trainer defined in DESIGN.md ("Word2Vec trainer").

Every fp32 operation of the device is restated with np.float32 arithmetic in the stated order (no fused multiply-add:
numpy rounds a * b and + c separately), the accumulators in np.int64. Lane l of the device holds dims l and l + 64, so
vectors are padded with zeros to 128 dims here; the dot's reduction is the xor butterfly over 32, 16, 8, 4, 2, 1.
Independent of the package: it imports nothing from it."""
import math

import numpy as np

MASK64 = (1 << 64) - 1
PAD = 128
_LANE = np.arange(64)


def mix(z: int) -> int:
    """splitmix64's finaliser with its increment, uint64 wrapping"""
    z = (z + 0x9E3779B97F4A7C15) & MASK64
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & MASK64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & MASK64
    z ^= z >> 31
    return z


def draw(seed: int, epoch: int, slot: int, index: int) -> int:
    """slot 0: keep, 1: reduced window, 2 + j: negative j; index: the event's place in the CSR"""
    return mix(mix(mix(int(seed) & MASK64) ^ ((int(epoch) << 32) | int(slot))) ^ int(index))


def mix_np(z):
    z = np.asarray(z, np.uint64)
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = z ^ (z >> np.uint64(30))
        z = z * np.uint64(0xBF58476D1CE4E5B9)
        z = z ^ (z >> np.uint64(27))
        z = z * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return z


def draw_np(seed, epoch, slot, index):
    inner = mix(mix(int(seed) & MASK64) ^ ((int(epoch) << 32) | int(slot)))
    return mix_np(np.uint64(inner) ^ np.asarray(index, np.uint64))


def build_vocab(aid, type_, types, min_count):
    """(index_to_key, counts): aids with count >= min_count over the events of `types`, count desc, aid asc"""
    aid = np.asarray(aid, np.int64)
    if types is not None:
        aid = aid[np.isin(np.asarray(type_), list(types))]
    keys, cnt = np.unique(aid, return_counts=True)
    m = cnt >= min_count
    keys, cnt = keys[m], cnt[m]
    order = np.lexsort((keys, -cnt))
    return keys[order].astype(np.int64), cnt[order].astype(np.int64)


def keep_thresholds(counts, sample):
    counts = np.asarray(counts, np.float64)
    if sample <= 0:
        return np.full(len(counts), 0xFFFFFFFF, np.uint32)
    tc = float(sample) * float(counts.sum())
    p = (np.sqrt(counts / tc) + 1.0) * (tc / counts)
    thr = np.minimum(np.floor(np.minimum(p, 1.0) * 4294967296.0), 4294967295.0)
    return np.where(p >= 1.0, 4294967295.0, thr).astype(np.uint32)


def negative_table(counts, ns_exponent=0.75):
    cs = np.cumsum(np.asarray(counts, np.float64) ** float(ns_exponent))
    cum = np.rint(cs / cs[-1] * 2147483648.0)
    cum[-1] = 2147483648.0
    return cum.astype(np.uint32)


def sigmoid_table(n_sig=1000, max_exp=6.0):
    x = (np.arange(n_sig, dtype=np.float64) / n_sig * 2.0 - 1.0) * max_exp
    return (1.0 / (1.0 + np.exp(-x))).astype(np.float32)


def init_weights(seed, n_vocab, dim):
    sm = mix(int(seed) & MASK64)
    out = np.empty((n_vocab, dim), np.float32)
    r = np.arange(n_vocab, dtype=np.uint64)
    for d in range(dim):
        u = mix_np(np.uint64(mix(sm ^ ((0xFFFFFFFF << 32) | d))) ^ r) >> np.uint64(40)
        out[:, d] = (u.astype(np.float32) * np.float32(2.0 ** -24) - np.float32(0.5)) / np.float32(dim)
    return out


def bits_for(n):
    return (int(n) - 1).bit_length() if n > 1 else 0


def clamp_of(batch_positions, window, negative):
    """a power of two C: (the most contributions one row can get in a batch) * C <= 2^62"""
    return 2.0 ** (62 - bits_for(int(batch_positions) * max(1 + negative, 2 * window)))


def compact(off, aid, type_, row_of_aid, keep_thr, n_vocab, type_mask, seed, epoch):
    """rows, orig, sid (per kept event) and the sentence offsets [n_sessions + 1]"""
    off = np.asarray(off, np.int64)
    n, S = len(aid), len(off) - 1
    rows, orig, sid = [], [], []
    coff = np.zeros(S + 1, np.int64)
    for s in range(S):
        coff[s] = len(rows)
        for i in range(int(off[s]), int(off[s + 1])):
            ty = int(type_[i])
            if not (0 <= ty < 32 and (type_mask >> ty) & 1):
                continue
            a = int(aid[i])
            r = int(row_of_aid[a]) if 0 <= a < len(row_of_aid) else -1
            if r < 0 or r >= n_vocab:
                continue
            if (draw(seed, epoch, 0, i) >> 32) <= int(keep_thr[r]):
                rows.append(r); orig.append(i); sid.append(s)
    coff[S] = len(rows)
    assert n == int(off[-1])
    return (np.asarray(rows, np.int32), np.asarray(orig, np.int32), np.asarray(sid, np.int32), coff)


def _pad(w):
    out = np.zeros((w.shape[0], PAD), np.float32)
    out[:, :w.shape[1]] = w
    return out


def fixed(x, shift, clamp):
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.rint(np.asarray(x, np.float32).astype(np.float64) * 2.0 ** shift)
    v[np.isnan(v)] = 0.0
    return np.clip(v, -clamp, clamp).astype(np.int64)


def wave_sum(v):
    for m in (32, 16, 8, 4, 2, 1):
        v = v + v[_LANE ^ m]
    return v[0]


def batch(rows, orig, sid, coff, b0, b1, syn0, syn1, cum, sig, *, window, negative, shift, batch_positions, seed,
          epoch, lr, max_exp=6.0, acc0=None, acc1=None, flag0=None, flag1=None, visited=None, trace=None):
    """the contributions of the kept positions [b0, b1) from the given weights: (acc0, acc1, flag0, flag1)"""
    V, dim = syn0.shape
    S0, S1 = _pad(np.asarray(syn0, np.float32)), _pad(np.asarray(syn1, np.float32))
    acc0 = np.zeros((V, dim), np.int64) if acc0 is None else acc0
    acc1 = np.zeros((V, dim), np.int64) if acc1 is None else acc1
    flag0 = np.zeros(V, np.uint8) if flag0 is None else flag0
    flag1 = np.zeros(V, np.uint8) if flag1 is None else flag1
    clamp = clamp_of(batch_positions, window, negative)
    n_sig = len(sig)
    mx = np.float32(max_exp)
    scale = np.float32(n_sig / (2.0 * max_exp))
    lr = np.float32(lr)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for p in range(b0, b1):
            w, sd, oi = int(rows[p]), int(sid[p]), int(orig[p]) & 0xFFFFFFFF
            eff = window - draw(seed, epoch, 1, oi) % window
            lo, hi = max(int(coff[sd]), p - eff), min(int(coff[sd + 1]) - 1, p + eff)
            ctx = [int(rows[j]) for j in range(lo, hi + 1) if j != p]
            if visited is not None:
                visited.append((p, tuple(ctx)))
            if not ctx:
                continue
            a = np.zeros(PAD, np.float32)
            for c in ctx:
                a = a + S0[c]
            h = a / np.float32(len(ctx))
            e = np.zeros(PAD, np.float32)
            for t in range(negative + 1):
                if t == 0:
                    tr, label = w, np.float32(1.0)
                else:
                    x = draw(seed, epoch, 1 + t, oi) >> 33
                    tr, label = min(int(np.searchsorted(cum, x, side="right")), V - 1), np.float32(0.0)
                    if tr == w:
                        continue
                s = S1[tr]
                f = wave_sum(h[:64] * s[:64] + h[64:] * s[64:])
                if trace is not None:
                    trace.append((p, t, tr, eff, float(f)))
                if not (f > -mx and f < mx):
                    continue
                idx = min(max(int((f + mx) * scale), 0), n_sig - 1)
                g = (label - sig[idx]) * lr
                e = e + g * s
                acc1[tr] += fixed(g * h, shift, clamp)[:dim]
                flag1[tr] = 1
            v = fixed(e, shift, clamp)[:dim]
            for c in ctx:
                acc0[c] += v
                flag0[c] = 1
    return acc0, acc1, flag0, flag1


def apply(w, acc, flag, shift):
    """in place: the flagged rows take their sums; sums and flags are zeroed"""
    on = flag != 0
    with np.errstate(over="ignore"):
        w[on] = w[on] + (acc[on].astype(np.float64) * 2.0 ** -shift).astype(np.float32)
    acc[on] = 0
    flag[:] = 0


def learning_rate(alpha, min_alpha, epoch, b, batch_positions, n_kept, epochs):
    a = alpha - (alpha - min_alpha) * ((float(epoch) + float(b * batch_positions) / float(n_kept)) / float(epochs))
    return np.float32(max(a, min_alpha))


def fit(off, aid, type_, n_items, *, types=None, dim=100, window=10, min_count=5, negative=5, ns_exponent=0.75,
        alpha=0.025, min_alpha=1e-4, sample=1e-3, epochs=5, seed=1, batch_positions=65536, shift=32, n_sig=1000,
        max_exp=6.0, visited=None):
    """(index_to_key, vectors) of the whole definition"""
    keys, counts = build_vocab(aid, type_, types, min_count)
    V = len(keys)
    row_of_aid = np.full(n_items, -1, np.int32)
    row_of_aid[keys] = np.arange(V, dtype=np.int32)
    thr, cum, sig = keep_thresholds(counts, sample), negative_table(counts, ns_exponent), sigmoid_table(n_sig, max_exp)
    mask = 7 if types is None else sum(1 << int(t) for t in types)
    syn0, syn1 = init_weights(seed, V, dim), np.zeros((V, dim), np.float32)
    acc0, acc1 = np.zeros((V, dim), np.int64), np.zeros((V, dim), np.int64)
    flag0, flag1 = np.zeros(V, np.uint8), np.zeros(V, np.uint8)
    for e in range(epochs):
        rows, orig, sid, coff = compact(off, aid, type_, row_of_aid, thr, V, mask, seed, e)
        N = len(rows)
        for b in range(math.ceil(N / batch_positions)):
            lr = learning_rate(alpha, min_alpha, e, b, batch_positions, N, epochs)
            batch(rows, orig, sid, coff, b * batch_positions, min(N, (b + 1) * batch_positions), syn0, syn1, cum, sig,
                  window=window, negative=negative, shift=shift, batch_positions=batch_positions, seed=seed, epoch=e,
                  lr=lr, max_exp=max_exp, acc0=acc0, acc1=acc1, flag0=flag0, flag1=flag1, visited=visited)
            apply(syn0, acc0, flag0, shift)
            apply(syn1, acc1, flag1, shift)
    return keys, syn0
