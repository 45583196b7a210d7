"""The exact kNN mode through the C-ABI (ottohip_knn_index_create_ex, ottohip_knn_topk_exact; csrc/knn.hip): centred
packing, the score margin in the main pass, the fp32 rerank of every buffered row that can be among the top k, and
the fp32 scan of all rows for a query whose buffer overflowed ("Exact mode").

The check is tests/knn_edges.py::check on a reference whose `certain` is the fp32 rerank's rule alone: an exact
top-k row must come back when the exact (k + 1)-th distance lies more than both R = 1.01 (dim + 2) 2^-24 d2 above its
own, or there is no (k + 1)-th. The bf16 scores put no condition on it: that is what the mode is for. Each input's
caps on what the rule may skip are asserted on the reference before the result is looked at; the shares they cap were
computed with oracle/knn.topk_exact on a CPU and are quoted beside each (cap = share less 0.03, certain items 0.99
throughout)."""
import functools

import numpy as np
import pytest

import knn as oracle
import knn_edges as K

pytestmark = pytest.mark.gpu

MIN_ITEMS = 0.99
MIN_EXACT = 0.98  # a set can differ from the oracle's only on a query that is not fully certain
# fully certain queries each reference must reach (computed share in the comment)
MIN_QUERIES = {
    "normal_d100": 0.96, "offset4": 0.96, "offset8": 0.96,  # 0.9940
    "clusters0.1": 0.96, "clusters0.3": 0.96,                # 0.9980
    "shells": 0.95,                                          # 0.9867
    "pre98305": 0.96,                                        # 0.9967
    "size1": 0.97, "size31": 0.97, "size33": 0.97, "size257": 0.97, "dim109": 0.97,  # 1.0
    "nq": 0.97, "normal_d16": 0.97,                          # 1.0 (normal_d16: k = 1, 5 and 20)
    "dim126": 0.96,                                          # 0.9975
}


def rerank_reference(emb, rows, k=20) -> K.Ref:
    """tests/knn_edges.py::reference with the certain-item rule reduced to the fp32 rerank's."""
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
    cert[:, :kk] = np.isinf(nxt) | (nxt - od > rr * (np.where(np.isinf(nxt), 0.0, nxt) + od))
    valid = idx >= 0
    return K.Ref(rows, k, idx, d2, cert, rr, float(cert.sum() / max(valid.sum(), 1)),
                 float(np.mean(np.all(cert | ~valid, axis=1))))


def _case(name):
    if name == "dim126":  # made like dim109
        return K._normal(2001, 126, 50 + 126), np.arange(0, 2001, 5)
    return K.case(name)


@functools.lru_cache(maxsize=None)
def _ref(name, k=20) -> K.Ref:
    return rerank_reference(*_case(name), k)


def _search(ctx, emb, rows=None, n_q=None, k=20, center=True, exact=True):
    """(idx, d2, stats of the exact call or None, phase names) through KnnIndex, i.e. the C-ABI."""
    from otto_recommender_amd.w2vec import KnnIndex
    ix = KnnIndex(emb, ctx, center=center)
    ctx.set_timing(True)
    try:
        i, d = ix.search(rows, n_q=n_q, k=k, exact=exact)
        phases = [n for n, _, _ in ctx.timings()]
    finally:
        ctx.set_timing(False)
    out = i.cpu().numpy(), d.cpu().numpy(), ix.last_exact_stats if exact else None, phases
    ix.free()
    return out


def _run(ctx, name, k=20, center=True, **caps):
    emb, rows = _case(name)
    ref = _ref(name, k)
    gi, gd, st, phases = _search(ctx, emb, rows, k=k, center=center)
    print(f"{name} k={k}: certain items {ref.item_share:.4f}, queries {ref.query_share:.4f}; appends per query "
          f"{st['sum_appends'] / len(rows):.1f}, max {st['max_appends']}, overflowed {st['n_overflow']}")
    caps = {"min_exact": MIN_EXACT, "min_items": MIN_ITEMS, "min_queries": MIN_QUERIES.get(name, 0.0), **caps}
    same = K.check(ref, gi, gd, **caps)
    print(f"{name} k={k}: sets equal {same:.4f}")
    assert "knn_rerank_buf" in phases and "knn_select" not in phases and "knn_rerank" not in phases, phases
    return gi, gd, st, phases, ref


# ---- 1: outside the default search's envelope ----

@pytest.mark.parametrize("name", ["offset8", "offset4", "clusters0.1", "clusters0.3"])
def test_outside_the_envelope_the_exact_search_is_exact(gpu, name):
    """A common offset and tight clusters: the default search returns the oracle's set on 0.13 - 0.998 of these
    queries (test_outside_the_envelope_only_certain_neighbours_are_promised); the exact one on all that the fp32
    rerank can resolve. Centred, offset8 and clusters0.1 stay inside the 512-entry buffers."""
    _, _, st, _, _ = _run(gpu, name)
    if name in ("offset8", "clusters0.1"):
        assert st["n_overflow"] == 0, st


# ---- 2: inside it: the same rows as the default search ----

@pytest.mark.parametrize("name", ["normal_d100", "pre98305"])
def test_inside_the_envelope_equal_to_the_default_search(gpu, name):
    """Bit-equal (idx, d2) to the default search on every query where the two sets are equal (the distances come
    from the same fp32 code), which is at least 98 % of them; pre98305 runs the pre-pass."""
    emb, rows = _case(name)
    gi, gd, _, phases, _ = _run(gpu, name)
    assert ("knn_pre" in phases) == (name == "pre98305"), phases
    di, dd, _, _ = _search(gpu, emb, rows, center=False, exact=False)
    same = np.array([set(a) == set(b) for a, b in zip(gi, di)])
    print(f"{name}: sets equal to the default search's {same.mean():.4f}")
    assert same.mean() >= 0.98
    np.testing.assert_array_equal(gi[same], di[same])
    np.testing.assert_array_equal(gd[same].view(np.uint32), dd[same].view(np.uint32))


# ---- 3, 4: buffer overflow -> the fp32 scan ----

def test_shells_overflow_is_answered_by_the_fp32_scan(gpu):
    """Shrinking shells: seen from the last row every item is nearer than all before it, so that query appends one
    entry per item (3 000 > 512) and is answered by k_knn_scan_f32."""
    gi, gd, st, phases, ref = _run(gpu, "shells")
    assert st["n_overflow"] >= 1 and st["max_appends"] > 512, st
    assert "knn_scan_f32" in phases, phases
    assert ref.rows[-1] == 2999
    np.testing.assert_array_equal(gi[-1], ref.idx[-1])
    np.testing.assert_allclose(gd[-1], ref.d2[-1], rtol=1e-5, atol=1e-6)


def test_uncentred_offset8_overflows_on_every_query_and_stays_exact(gpu):
    """The exact search on an index that was not centred: the margin from the uncentred norms (delta ~ 100) lets
    every row in, all 16 queries overflow, and the scan returns the oracle's rows."""
    emb, rows = K.case("offset8")
    rows = rows[:16]
    ref = rerank_reference(emb, rows)  # certain items 1.0, fully certain queries 1.0 on these 16 rows
    gi, gd, st, phases = _search(gpu, emb, rows, center=False)
    print("uncentred offset8:", st)
    K.check(ref, gi, gd, min_exact=MIN_EXACT, min_items=MIN_ITEMS, min_queries=0.97)
    assert st["n_overflow"] == 16, st
    assert "knn_scan_f32" in phases, phases


# ---- 5, 6: ties by row index among all equal rows ----

def test_a_hundred_identical_rows_come_back_lowest_index_first(gpu):
    """100 identical rows (V = 99 000, pre-pass active): every member's top-20 are the 20 lowest member rows in
    ascending order at distance 0. The default search returns some 20 of them (test_more_ties_than_candidates)."""
    emb, rows = K.big_group()
    gi, gd, st, phases = _search(gpu, emb, rows)
    assert "knn_pre" in phases, phases
    np.testing.assert_array_equal(gi, np.tile(rows[:20], (len(rows), 1)))
    assert np.all(gd == 0)


def test_tie_groups_at_the_prepass_bound_come_back_complete(gpu):
    emb, groups = K.with_ties(99_000)
    rows = np.concatenate(groups)
    want = np.concatenate([np.tile(g[:20], (24, 1)) for g in groups])
    gi, gd, st, phases = _search(gpu, emb, rows)
    assert "knn_pre" in phases, phases
    np.testing.assert_array_equal(gi, want)
    assert np.all(gd == 0)


# ---- 7: shapes ----

@pytest.mark.parametrize("V", [1, 31, 33, 257])
def test_index_sizes(gpu, V):
    """All rows as queries. V < 24: every row is a candidate; slots past V are -1 / inf."""
    gi, gd, _, _, _ = _run(gpu, f"size{V}")
    n = min(V, 20)
    assert np.all(gi[:, :n] >= 0) and np.all(gi[:, :n] < V) and np.all(np.isfinite(gd[:, :n]))
    assert np.all(gi[:, n:] == -1) and np.all(np.isinf(gd[:, n:]))
    assert np.all(gi[:, 0] == np.arange(V)) and np.all(gd[:, 0] == 0)


@pytest.mark.parametrize("dim", [1, 2])
def test_dims_1_and_2_certain_items(gpu, dim):
    """Half-line rows have pairs at equal distance across rank 20 / 21 (fully certain queries 0.04 / 0.52), so only
    the certain-item rule is asserted: certain items 0.952 (dim 1), 0.976 (dim 2)."""
    _run(gpu, f"dim{dim}", min_exact=0.0, min_items=0.93, min_queries=0.0)


@pytest.mark.parametrize("name", ["dim109", "dim126", "nq"])
def test_wide_rows_and_a_workgroup_boundary(gpu, name):
    """dim 109 is the first on eight k-steps, dim 126 the widest row; nq has 257 queries (one past a workgroup)."""
    gi, gd, _, _, ref = _run(gpu, name)
    assert np.all(gi[:, 0] == ref.rows) and np.all(gd[:, 0] == 0)


@pytest.mark.parametrize("k", [1, 5])
def test_small_k(gpu, k):
    gi, _, _, _, _ = _run(gpu, "normal_d16", k=k)
    assert gi.shape == (500, k)


# ---- 8: argument errors ----

def test_argument_errors(gpu):
    import ctypes
    import torch
    from otto_recommender_amd import _lib as L
    from otto_recommender_amd.w2vec import KnnIndex
    emb, _ = K.case("nq")
    ix = KnnIndex(emb, gpu, center=True)
    with pytest.raises(L.OttoHipError) as e:
        ix.search(np.arange(4), k=21, exact=True)
    assert e.value.rc == -1  # OTTOHIP_EINVAL
    with pytest.raises(L.OttoHipError) as e:
        ix.search(np.array([0, ix.n_items]), k=5, exact=True)
    assert e.value.rc == -2  # OTTOHIP_ERANGE
    st = L.KnnExactStats()
    assert L.load().ottohip_knn_topk_exact(gpu.h, ix.h, None, 0, 20, None, None, ctypes.byref(st),
                                           L.stream_handle(None)) == 0
    assert L.load().ottohip_knn_topk_exact(gpu.h, ix.h, None, 0, 20, None, None, None, L.stream_handle(None)) == 0
    h = ctypes.c_void_p()
    assert L.load().ottohip_knn_index_create_ex(gpu.h, L.ptr(ix.emb), ix.n_items, ix.dim, 2, ctypes.byref(h),
                                                L.stream_handle(None)) != 0  # an unknown flag
    torch.cuda.synchronize()
    ix.free()


# ---- 9: the reference's signatures ----

def test_knn_table_and_get_top_k_similar_faiss_exact(gpu):
    import torch
    import otto_recommender_amd.synth as synth
    from otto_recommender_amd import w2vec
    emb = synth.embeddings(2000, seed=2)
    words = np.random.default_rng(0).permutation(10_000)[:2000].astype(np.int32)
    ref = rerank_reference(emb, np.arange(300))  # certain items 0.9997, fully certain queries 0.9933
    assert ref.item_share >= MIN_ITEMS and ref.query_share >= 0.96
    full = ref.certain.all(1)
    # ... of which the queries whose neighbours the fp32 rerank also orders as the oracle does (every gap above both R)
    ordered = full & np.all(np.diff(ref.d2, axis=1) > ref.rr * (ref.d2[:, 1:] + ref.d2[:, :-1]), axis=1)
    assert ordered.sum() >= 250
    ix = w2vec.load_index_faiss_ivff(emb, exact=True)
    assert ix.center
    wq = list(words[:300]) + [10_000_000]  # a word without an embedding is dropped
    df = w2vec.get_top_k_similar_faiss(wq, words, None, ix, k=20, exact=True)
    tab = w2vec.knn_table(ix, torch.from_numpy(words), torch.arange(300, dtype=torch.int32), 20, exact=True)
    assert ix.last_exact_stats is not None and ix.last_exact_stats["sum_appends"] >= 300 * 20
    for cols in (df, {c: t.cpu().numpy() for c, t in tab.items()}):
        nxt = np.asarray(cols["aid_next"]).reshape(300, 20)
        np.testing.assert_array_equal(nxt[ordered], words[ref.idx][ordered])
        np.testing.assert_array_equal(np.sort(nxt[full], axis=1), np.sort(words[ref.idx][full], axis=1))
        assert np.mean([set(a) == set(b) for a, b in zip(nxt, words[ref.idx])]) >= MIN_EXACT
        dist = np.asarray(cols["dist_w2vec"]).reshape(300, 20)
        assert np.all(np.abs(dist[full] - np.trunc(ref.d2[full])) <= 1)
        np.testing.assert_array_equal(np.asarray(cols["rank_w2vec"]).reshape(300, 20), np.tile(np.arange(1, 21), (300, 1)))
        np.testing.assert_array_equal(np.asarray(cols["aid"]).reshape(300, 20)[:, 0], words[:300])
    ix.free()
