"""Helper of tests/test_knn_edges_gpu.py and tests/test_knn_edges_cpu.py: what the bf16 MFMA search can
guarantee, derived from its number formats, and the inputs the edge tests share.

For a query q and an item v let s = q.v - |v|^2/2 in float64 (|q - v|^2 = |q|^2 - 2 s, so s ranks like
the negated distance). The main pass ranks by a device score that differs from s by at most

    E(q, v) = 1.01 * 2^-7 * sum_d |q_d v_d|  +  2^-15 * (|v|^2 / 2 + |s|)  (+ 2^-144: the key of a score 0)

- every factor is rounded to bf16 (RNE, 8 significant bits: the spacing is 2^-7 of the value, the
  rounding error <= 2^-8 of it), so a product of two rounded factors is off by <= (1 + 2^-8)^2 - 1
  = 2^-7 + 2^-16 of |q_d v_d|, and the row sum by that share of sum_d |q_d v_d| (<= |q| |v| by
  Cauchy-Schwarz, the form DESIGN.md quotes; the sum is what the tests use, it is the tighter of the two);
- -|v|^2/2 travels as a hi/lo pair of bf16: the residual is <= 2^-8 * 2^-8 = 2^-16 of |v|^2/2;
- the candidate key replaces the 5 low mantissa bits of the fp32 score by the row slot: <= 31 ulp
  < 2^-18 |s|;
- fp32 accumulation of <= 128 terms: <= 2^-17 of (sum_d |q_d v_d| + |v|^2/2), inside the 1 % on the first
  term and the factor 2 the second term leaves over the hi/lo residual.
(With 2^-9 for the bf16 rounding error, half the true figure, the emulation in test_knn_edges_cpu.py
exceeds the bound 1.96-fold on normal data of dim 1, where Cauchy-Schwarz is an equality; it stays within
this one on every input used here.)

The main pass keeps KN_C = 24 candidates per query, so an exact top-k item v is a candidate whatever the
rounding did when fewer than KN_C other items w have s(w) + E(q, w) >= s(v) - E(q, v).

The rerank orders the candidates by |q - v|^2 in fp32: t = fl(q_d - v_d) is off by <= 2^-24 of itself, t^2
by 2^-23, and each of the dim fused multiply-adds rounds once, by <= 2^-24 of the running sum, so the fp32
distance is within R(d2) = 1.01 * (dim + 2) * 2^-24 * d2 of the exact one. Two rows can come back in
swapped order only if their exact distances differ by no more than the sum of their R (on N(0, 1) rows of
dim 100 that is 1e-3 at d2 = 140, a few per 10 000 neighbour pairs).

An exact top-k item is CERTAIN to be returned when it is such a candidate and the exact (k + 1)-th distance
lies more than both R above its own.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np
import torch

import knn as oracle

KN_C = 24      # csrc/knn.hip
KN_IT = 256    # items per tile
PRE_STRIDE = 16


def scores64(emb: np.ndarray, rows) -> tuple:
    """(s, E) as float64 torch [n_q, V] for the query rows."""
    e = torch.from_numpy(np.ascontiguousarray(emb, np.float32)).double()
    r = torch.from_numpy(np.asarray(rows, np.int64))
    vn = (e * e).sum(1)
    s = e[r] @ e.T - 0.5 * vn[None, :]
    err = 1.01 * 2.0 ** -7 * (e[r].abs() @ e.abs().T) + 2.0 ** -15 * (0.5 * vn[None, :] + s.abs()) + 2.0 ** -144
    return s, err


def emulated_scores(emb: np.ndarray, rows) -> torch.Tensor:
    """The packed operands of k_knn_pack (RNE bf16 factors, the hi/lo bf16 columns of -|v|^2/2 against
    1, 1 in the query) multiplied with fp32 sums: float32 [n_q, V]."""
    e = torch.from_numpy(np.ascontiguousarray(emb, np.float32))
    r = torch.from_numpy(np.asarray(rows, np.int64))
    nh = -0.5 * (e * e).sum(1)
    hi = nh.bfloat16().float()
    lo = (nh - hi).bfloat16().float()
    items = torch.cat([e.bfloat16().float(), hi[:, None], lo[:, None]], 1)
    queries = torch.cat([e[r].bfloat16().float(), torch.ones(len(r), 2)], 1)
    return queries @ items.T


def emulation_excess(emb: np.ndarray, rows, chunk: int = 128) -> float:
    """max over (q, v) of (|emulated - s| + 31 ulp of the emulated score) / E: <= 1 when the bound holds."""
    rows = np.asarray(rows, np.int64)
    worst = 0.0
    for a in range(0, len(rows), chunk):
        s, err = scores64(emb, rows[a:a + chunk])
        em = emulated_scores(emb, rows[a:a + chunk])
        key = 31.0 * torch.from_numpy(np.spacing(np.abs(em.numpy()))).double()
        worst = max(worst, float((((em.double() - s).abs() + key) / err).max()))
    return worst


@dataclass
class Ref:
    rows: np.ndarray
    k: int
    idx: np.ndarray        # oracle top-k rows, int64 [n_q, k], -1 past the index size
    d2: np.ndarray         # float64 [n_q, k], inf past the index size
    certain: np.ndarray    # bool [n_q, k]
    rr: float              # R(d2) / d2 of the fp32 rerank
    item_share: float      # certain items / top-k items
    query_share: float     # queries whose top-k items are all certain


def reference(emb: np.ndarray, rows, k: int = 20, chunk: int = 128) -> Ref:
    rows = np.asarray(rows, np.int64)
    V = emb.shape[0]
    kk = min(k, V)
    oi, od = oracle.topk_exact(emb, rows, min(k + 1, V))
    nxt = od[:, k:k + 1] if V > k else np.full((len(rows), 1), np.inf)  # the exact (k + 1)-th distance
    oi, od = oi[:, :kk], od[:, :kk]
    rr = 1.01 * (emb.shape[1] + 2) * 2.0 ** -24
    idx = np.full((len(rows), k), -1, np.int64)
    d2 = np.full((len(rows), k), np.inf)
    idx[:, :kk], d2[:, :kk] = oi, od
    cert = np.zeros((len(rows), k), bool)
    for a in range(0, len(rows), chunk):
        s, err = scores64(emb, rows[a:a + chunk])
        top = torch.from_numpy(oi[a:a + chunk])
        lo = (s - err).gather(1, top)
        if V <= KN_C:  # every item fits the candidate list
            cert[a:a + chunk, :kk] = True
        else:  # fewer than KN_C others reach lo  <=>  the (KN_C + 1)-th largest upper bound is below lo
            u = torch.topk(s + err, KN_C + 1, dim=1).values[:, -1:]
            cert[a:a + chunk, :kk] = (lo > u).numpy()
    cert[:, :kk] &= np.isinf(nxt) | (nxt - od > rr * (np.where(np.isinf(nxt), 0.0, nxt) + od))
    valid = idx >= 0
    return Ref(rows, k, idx, d2, cert, rr, float(cert.sum() / max(valid.sum(), 1)),
               float(np.mean(np.all(cert | ~valid, axis=1))))


def check(ref: Ref, gi: np.ndarray, gd: np.ndarray, min_exact: float = 0.995, min_items: float = 0.0,
          min_queries: float = 0.0) -> float:
    """min_items / min_queries cap what the certain-item rule may skip; they are asserted on the reference
    before the result is looked at. Returns the share of queries whose neighbour sets equal the oracle's."""
    assert ref.item_share >= min_items, (ref.item_share, min_items)
    assert ref.query_share >= min_queries, (ref.query_share, min_queries)
    gi, gd = np.asarray(gi), np.asarray(gd)
    assert gi.shape == ref.idx.shape and gd.shape == ref.d2.shape
    # 1. every certain item is returned
    found = (ref.idx[:, :, None] == gi[:, None, :]).any(-1)
    miss = np.argwhere(ref.certain & ~found)
    assert len(miss) == 0, [(int(ref.rows[q]), int(ref.idx[q, j]), j) for q, j in miss[:8]]
    # 2. a query whose exact top-k are all certain gets exactly the oracle's rows, in the oracle's order but
    #    for rows whose exact distances the fp32 rerank cannot tell apart
    full = np.all(ref.certain | (ref.idx < 0), axis=1)
    np.testing.assert_array_equal(np.sort(gi[full], axis=1), np.sort(ref.idx[full], axis=1))
    pos = (gi[full][:, :, None] == ref.idx[full][:, None, :]).argmax(-1)  # oracle position of each returned row
    moved = gi[full] != ref.idx[full]  # never a slot past the index size: the sorted rows are equal
    dg, dr = np.take_along_axis(ref.d2[full], pos, axis=1)[moved], ref.d2[full][moved]
    assert np.all(np.abs(dg - dr) <= ref.rr * (dg + dr)), np.argwhere(moved)[:8]
    # 3. tests/test_knn.py::_check
    same = float(np.mean([set(a) == set(b) for a, b in zip(gi, ref.idx)]))
    assert same >= min_exact, same
    ok = np.all(gi == ref.idx, axis=1)
    np.testing.assert_allclose(gd[ok], ref.d2[ok], rtol=1e-5, atol=1e-6)
    assert np.all(gd[:, 1:] >= gd[:, :-1])
    return same


# ---- shared inputs: name -> (embeddings, query rows); each reference is computed once per process ----

def _normal(V, dim, seed):
    return np.random.default_rng(seed).normal(size=(V, dim)).astype(np.float32)


def tie_groups(n_groups: int = 3, size: int = KN_C):
    """Rows for groups of duplicates: row j of group g sits in sampled tile 16 j (tiles 0 .. 16 * 23), in a
    32-item block of its own, at in-block position (j + 3 g) % 32: 24 different blocks and positions."""
    out = []
    for g in range(n_groups):
        j = np.arange(size)
        out.append(PRE_STRIDE * j * KN_IT + ((2 * g + j) % 8) * 32 + (j + 3 * g) % 32)
    return out


def with_ties(V: int):
    emb = _normal(V, 100, 21)
    vec = _normal(3, 100, 22)
    groups = tie_groups()
    for g, r in enumerate(groups):
        emb[r] = vec[g]
    return emb, groups


def big_group(V: int = 99_000, size: int = 100):
    """`size` duplicates over sampled tiles 0, 16, .. 384, four blocks of each."""
    emb = _normal(V, 100, 23)
    j = np.arange(size)
    rows = PRE_STRIDE * (j % 25) * KN_IT + (j // 25) * 64 + (7 * j) % 32
    emb[rows] = _normal(1, 100, 24)[0]
    return emb, np.sort(rows)


def shrinking_shells(V: int = 3000, dim: int = 100, scale: float = 1.0):
    """Row i = q0 + r_i u_i with unit directions u_i and r_i falling from 30 to 0.5, the last row q0: seen
    from the last row every item is nearer than all before it, so its list takes an insert per item."""
    rng = np.random.default_rng(31)
    q0 = scale * rng.normal(size=dim)
    u = rng.normal(size=(V, dim))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    r = np.linspace(30.0, 0.5, V)
    emb = q0[None, :] + r[:, None] * u
    emb[-1] = q0
    return emb.astype(np.float32)


def _clusters(V, dim, sigma, seed):
    rng = np.random.default_rng(seed)
    centres = rng.normal(size=(200, dim))
    return (centres[rng.integers(0, 200, V)] + sigma * rng.normal(size=(V, dim))).astype(np.float32)


def half_line(dim: int, seed: int):
    """dim 1 and 2 leave bf16 too few bits for random data (in one dimension the 20 nearest of 2 000 normal
    points differ in the 4th digit), so these rows are exact in bf16: x = i / 2 for all i in -255 .. 255 in
    shuffled order and, at dim 2, y = +-1. Every product, -|v|^2/2 = hi + lo and every partial sum is then
    exact in fp32, distinct distances differ by >= 0.125 in s against a key error of 31 ulp <= 0.015, and
    rows at equal distance come in pairs (x - d, x + d), which never straddle the 24 candidates' end."""
    rng = np.random.default_rng(seed)
    emb = (rng.permutation(511).astype(np.float32)[:, None] - 255) / 2
    if dim == 2:
        emb = np.concatenate([emb, rng.choice(np.float32([-1, 1]), size=(511, 1))], 1)
    return np.ascontiguousarray(emb, np.float32)


def _spread(V, n):
    return np.unique(np.linspace(0, V - 1, n).astype(np.int64))


DIMS = (1, 2, 101, 102, 103, 104, 109)
SIZES = (1, 31, 32, 33, 255, 256, 257, 512)
ENVELOPE = ("offset2", "offset4", "offset8", "clusters0.3", "clusters0.1")


@functools.lru_cache(maxsize=None)
def case(name: str):
    import otto_recommender_amd.synth as synth
    if name == "normal_d100":
        return _normal(20_000, 100, 41), np.arange(0, 20_000, 40)
    if name == "normal_d1":  # emulation only: Cauchy-Schwarz is an equality here, the bound is nearly attained
        return _normal(2001, 1, 44), np.arange(0, 2001, 5)
    if name == "normal_d16":
        return _normal(20_000, 16, 42), np.arange(0, 20_000, 40)
    if name in ("pre98304", "pre98305"):
        V = int(name[3:])
        return synth.embeddings(V, seed=13), _spread(V, 300)
    if name == "shells":
        emb = shrinking_shells(scale=0.25)  # |q0| = 2.5: at |q0| = 10 the inner shells (0.5 apart) leave the envelope
        return emb, np.concatenate([np.arange(0, 3000, 4), [2999]])
    if name.startswith("dim"):
        d = int(name[3:])
        if d <= 2:
            return half_line(d, 50 + d), np.arange(511)
        return _normal(2001, d, 50 + d), np.arange(0, 2001, 5)
    if name.startswith("size"):
        V = int(name[4:])
        return _normal(V, 100, 60), np.arange(V)
    if name == "nq":
        return _normal(2000, 100, 70), np.arange(257)
    if name.startswith("offset"):
        return _normal(20_000, 100, 41) + np.float32(name[6:]), np.arange(0, 20_000, 40)
    if name.startswith("clusters"):
        return _clusters(20_000, 100, float(name[8:]), 43), np.arange(0, 20_000, 40)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def ref(name: str, k: int = 20) -> Ref:
    emb, rows = case(name)
    return reference(emb, rows, k)


# (certain items, fully certain queries) each input's reference must reach before a result is looked at:
# the shares computed on a CPU (tests/test_knn_edges_cpu.py prints them, quoted beside each cap) less 0.03.
# The envelope inputs carry no cap: few of their items are certain.
CAPS = {
    "normal_d100": (0.84, 0.16),  # 0.8718 0.1940
    "normal_d16": (0.89, 0.36),   # 0.9278 0.3980
    "pre98304": (0.91, 0.54),     # 0.9463 0.5700
    "pre98305": (0.92, 0.55),     # 0.9508 0.5833
    "shells": (0.81, 0.13),       # 0.8405 0.1611
    "nq": (0.90, 0.39),           # 0.9331 0.4280
    # dim 1, 2: the bound does not know that these rows are exact in bf16, and the pair at equal distance
    # across rank 20 / 21 keeps a query from being fully certain; there the 99.5 % of equal sets is what bites
    "dim1": (0.20, 0.0),          # 0.2322 0
    "dim2": (0.20, 0.04),         # 0.2323 0.0724
    "dim101": (0.89, 0.35),       # 0.9277 0.3890
    "dim102": (0.90, 0.41),       # 0.9342 0.4464
    "dim103": (0.90, 0.40),       # 0.9337 0.4339
    "dim104": (0.89, 0.35),       # 0.9273 0.3840
    "dim109": (0.89, 0.30),       # 0.9229 0.3367
    "size1": (0.97, 0.97), "size31": (0.97, 0.97), "size32": (0.97, 0.97), "size33": (0.97, 0.97),  # 1 1
    "size255": (0.95, 0.70),      # 0.9802 0.7333
    "size256": (0.95, 0.70),      # 0.9803 0.7344
    "size257": (0.95, 0.69),      # 0.9800 0.7276
    "size512": (0.93, 0.59),      # 0.9644 0.6230
}


def caps(name: str) -> dict:
    a, b = CAPS[name]
    return {"min_items": a, "min_queries": b}
