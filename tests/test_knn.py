"""W2V kNN (model/w2vec_aids.py:125-173): MFMA path vs the exact brute-force oracle.

Tolerance (floating point): neighbour sets equal to the exact fp32/fp64 search on >= 99.5 %
of queries (SURVEY.md §8c asks >= 0.99 overlap; the reference's own IVF reached 0.973/0.980),
squared distances within 1e-5 relative (+1e-6 absolute), dist_w2vec = trunc(d2) within 1,
rank_w2vec = position 1..k, the query itself first with distance 0.
These are friendly inputs; tests/test_knn_edges_gpu.py holds the derived certain-neighbour rule, the pre-pass,
the index-list rerun, the k-step variants and the shape edges."""
import numpy as np
import pytest

import knn as oracle
import otto_recommender_amd.synth as synth

pytestmark = pytest.mark.gpu


def _check(emb, rows, k, gi, gd, min_exact=0.995):
    ri, rd = oracle.topk_exact(emb, rows, k)
    same = np.mean([set(a) == set(b) for a, b in zip(gi, ri)])
    assert same >= min_exact, same
    ok = np.all(gi == ri, axis=1)
    np.testing.assert_allclose(gd[ok], rd[ok], rtol=1e-5, atol=1e-6)
    assert np.all(np.diff(gd, axis=1) >= 0)


def test_knn_small_exact(gpu):
    from otto_recommender_amd.w2vec import KnnIndex
    emb = synth.embeddings(30_000, seed=3)
    ix = KnnIndex(emb)
    rows = np.arange(2000)
    i, d = ix.search(rows, k=20)
    gi, gd = i.cpu().numpy(), d.cpu().numpy()
    assert np.all(gi[:, 0] == rows) and np.all(gd[:, 0] == 0)
    _check(emb, rows, 20, gi, gd)


def test_knn_candidate_buffers_equal_index_lists(gpu, monkeypatch):
    """The main pass with per-query candidate buffers (scores-only register lists, the first KN_C inserts
    by score and insertion order selected before the rerank) returns exactly the indices and distances
    of the index-list pass (OTTOHIP_KNN_BUF=0), on clustered embeddings with many near-equal scores."""
    from otto_recommender_amd.w2vec import KnnIndex
    emb = synth.embeddings(120_000, seed=9)
    emb[1000:1100] = emb[5]  # exact duplicates: equal scores inserted in order
    rows = np.concatenate([np.arange(0, 3000), np.arange(1000, 1100)])
    out = []
    for buf in ("0", "1"):
        monkeypatch.setenv("OTTOHIP_KNN_BUF", buf)
        ix = KnnIndex(emb)
        i, d = ix.search(rows, k=20)
        out.append((i.cpu().numpy(), d.cpu().numpy()))
        ix.free()
    np.testing.assert_array_equal(out[0][0], out[1][0])
    np.testing.assert_array_equal(out[0][1], out[1][1])


def test_knn_arbitrary_rows_tiny_index_and_ties(gpu):
    from otto_recommender_amd.w2vec import KnnIndex
    rng = np.random.default_rng(1)
    emb = rng.normal(size=(40, 100)).astype(np.float32)
    emb[7] = emb[3]  # exact duplicate: tie broken by row index
    ix = KnnIndex(emb)
    rows = np.array([3, 7, 39, 0, 11])
    i, d = ix.search(rows, k=20)
    gi, gd = i.cpu().numpy(), d.cpu().numpy()
    assert list(gi[0][:2]) == [3, 7] and list(gi[1][:2]) == [3, 7]
    _check(emb, rows, 20, gi, gd, min_exact=1.0)
    # fewer items than k
    ix2 = KnnIndex(emb[:5])
    i2, d2 = ix2.search(np.array([0, 4]), k=8)
    assert list(i2.cpu().numpy()[0][5:]) == [-1, -1, -1] and np.all(np.isinf(d2.cpu().numpy()[:, 5:]))


@pytest.mark.parametrize("dim", [16, 110, 111, 126])
def test_knn_dims_around_the_k_step_split(gpu, dim):
    """dim + 2 <= 112 runs 7 k-steps of 16 (the zero padding is neither streamed nor multiplied),
    larger dims 8: both sides of the split and the smallest/largest dims."""
    from otto_recommender_amd.w2vec import KnnIndex
    rng = np.random.default_rng(dim)
    emb = rng.normal(size=(9_000, dim)).astype(np.float32)
    ix = KnnIndex(emb)
    rows = np.arange(0, 9_000, 7)
    i, d = ix.search(rows, k=20)
    gi, gd = i.cpu().numpy(), d.cpu().numpy()
    assert np.all(gi[:, 0] == rows) and np.all(gd[:, 0] == 0)
    _check(emb, rows, 20, gi, gd)


def test_get_top_k_similar_faiss_frame(gpu):
    from otto_recommender_amd import w2vec
    emb = synth.embeddings(5000, seed=2)
    words = np.random.default_rng(0).permutation(10_000)[:5000].astype(np.int32)
    ix = w2vec.load_index_faiss_ivff(emb)
    wq = list(words[:50]) + [10_000_000]  # a word without an embedding is dropped (:156-163)
    df = w2vec.get_top_k_similar_faiss(wq, words, None, ix, k=20)
    assert list(df.columns) == ["aid", "aid_next", "dist_w2vec", "rank_w2vec"]
    assert len(df) == 50 * 20
    assert str(df["dist_w2vec"].dtype) == "int32" and str(df["rank_w2vec"].dtype) == "int8"
    ri, rd = oracle.topk_exact(emb, np.arange(50), 20)
    assert np.array_equal(df["aid_next"].to_numpy().reshape(50, 20), words[ri])
    assert np.all(np.abs(df["dist_w2vec"].to_numpy().reshape(50, 20) - np.trunc(rd)) <= 1)
    assert np.array_equal(df["rank_w2vec"].to_numpy().reshape(50, 20), np.tile(np.arange(1, 21), (50, 1)))
    assert np.array_equal(df["aid"].to_numpy().reshape(50, 20)[:, 0], words[:50])


def test_retrieve_knns_parquet_cache(gpu, tmp_path):
    """retrieve_w2vec_knns_via_faiss_index (w2vec_aids.py:176-206): neighbours of the first
    first_n_aids words, written to the cache parquet (:191, :204) with the frame's dtypes and read
    back instead of searching on the next call (:193-195)."""
    import pandas as pd
    import pyarrow.parquet as pq
    from otto_recommender_amd import w2vec
    emb = synth.embeddings(6000, seed=5)
    words = synth.item_words(seed=0, n_items=6000)
    cache = str(tmp_path / "w2v" / "model.top-20-nns-300-aids.parquet")
    df = w2vec.retrieve_w2vec_knns_via_faiss_index(emb, words, k=20, first_n_aids=300, cache_file=cache)
    schema = pq.read_schema(cache)
    assert [(f.name, str(f.type)) for f in schema][:4] == [("aid", "int32"), ("aid_next", "int32"),
                                                            ("dist_w2vec", "int32"), ("rank_w2vec", "int8")]
    ri, rd = oracle.topk_exact(emb, np.arange(300), 20)
    assert np.array_equal(df["aid"].to_numpy().reshape(300, 20)[:, 0], words[:300])
    got = df["aid_next"].to_numpy().reshape(300, 20)
    assert np.mean([set(a) == set(b) for a, b in zip(got, words[ri])]) >= 0.995
    again = w2vec.retrieve_w2vec_knns_via_faiss_index(None, None, k=20, first_n_aids=300, cache_file=cache)
    pd.testing.assert_frame_equal(again.reset_index(drop=True), df.reset_index(drop=True))


def test_knn_rejects_out_of_range_rows(gpu):
    from otto_recommender_amd import _lib as L
    from otto_recommender_amd.w2vec import KnnIndex
    ix = KnnIndex(synth.embeddings(100, seed=4))
    with pytest.raises(L.OttoHipError):
        ix.search(np.array([0, 100]), k=5)
    with pytest.raises(L.OttoHipError):
        ix.search(None, n_q=101, k=5)


@pytest.mark.slow
def test_knn_full_size_config3(gpu):
    """BASELINE configs[2] at full size: 1,855,603 items x 100, the first 600,000 rows as queries
    (config.py:125), k = 20; 2,500 queries sampled over the whole query range (both ends included)
    checked against the exact oracle."""
    from otto_recommender_amd.w2vec import KnnIndex
    emb = synth.embeddings(1_855_603)
    ix = KnnIndex(emb)
    i, d = ix.search(None, n_q=600_000, k=20)
    rng = np.random.default_rng(11)
    rows = np.unique(np.concatenate([[0, 1, 599_998, 599_999], rng.choice(600_000, 2_496, replace=False)]))
    gi, gd = i[rows].cpu().numpy(), d[rows].cpu().numpy()
    assert np.all(gi[:, 0] == rows) and np.all(gd[:, 0] == 0)
    _check(emb, rows, 20, gi, gd)
    ix.free()
