"""Word2Vec trainer, host side (no GPU): vocabulary, keep thresholds, negative table, draws, model files, and the
invariants of the numpy restatement (tests/w2v_oracle.py) the GPU tests compare against."""
import math

import numpy as np
import pytest

import w2v_oracle as O


@pytest.fixture(scope="module")
def W():
    from otto_recommender_amd import w2vec
    return w2vec


def test_vocabulary_order_and_count_ties(W):
    counts = np.zeros(12, np.int64)
    counts[[9, 2, 7, 4, 11, 5]] = [7, 7, 9, 5, 4, 7]
    keys, cnt = W.vocabulary(counts, min_count=5)
    assert keys.tolist() == [7, 2, 5, 9, 4]      # 9 first, then the three 7s by aid, then 5; count 4 is dropped
    assert cnt.tolist() == [9, 7, 7, 7, 5]
    aid = np.repeat(np.arange(12), counts)
    ok, oc = O.build_vocab(aid, np.zeros(len(aid), np.int8), None, 5)
    assert ok.tolist() == keys.tolist() and oc.tolist() == cnt.tolist()
    # the type filter of the restatement
    ty = np.zeros(len(aid), np.int8); ty[aid == 7] = 1
    ok, oc = O.build_vocab(aid, ty, [1], 5)
    assert ok.tolist() == [7] and oc.tolist() == [9]


def test_keep_thresholds_hand_cases(W):
    # T = 10100, sample = 0.01 -> sample T = 101: c = 10000: p = (sqrt(10000 / 101) + 1) 101 / 10000; c = 100: p > 1
    counts = np.array([10000, 100], np.int64)
    p0 = (math.sqrt(10000 / 101.0) + 1.0) * (101.0 / 10000)
    for f in (W.keep_thresholds, O.keep_thresholds):
        thr = f(counts, 0.01)
        assert thr.dtype == np.uint32
        assert int(thr[0]) == math.floor(p0 * 2 ** 32) and 0 < int(thr[0]) < 2 ** 32 - 1
        assert int(thr[1]) == 0xFFFFFFFF
        assert (f(counts, 0) == 0xFFFFFFFF).all()   # sample = 0 keeps everything
    # c = 4 sample T with p = (2 + 1) / 4 exactly
    thr = W.keep_thresholds(np.array([400, 0 + 600], np.int64), 0.1)   # sample T = 100: c = 400 -> 0.75
    assert int(thr[0]) == 3 << 30


def test_negative_table_hand_cases(W):
    for f in (W.negative_table, O.negative_table):
        cum = f(np.array([16, 1, 1], np.int64), 0.75)          # 8, 1, 1 of 10
        assert cum.dtype == np.uint32
        assert cum.tolist() == [round(0.8 * 2 ** 31), round(0.9 * 2 ** 31), 2 ** 31]
        assert f(np.array([5], np.int64), 0.75).tolist() == [2 ** 31]
        assert f(np.array([3, 3, 3, 3], np.int64), 0.0).tolist() == [2 ** 29, 2 ** 30, 3 * 2 ** 29, 2 ** 31]
    # a 31-bit draw picks the first row whose entry is above it
    cum = W.negative_table(np.array([16, 1, 1], np.int64))
    assert np.searchsorted(cum, [0, cum[0] - 1, cum[0], cum[1], 2 ** 31 - 1], side="right").tolist() == [0, 0, 1, 2, 2]


def test_draw_is_train_mix(W):
    from otto_recommender_amd import train
    for z in (0, 1, 12345678901234567, (1 << 64) - 1):
        assert O.mix(z) == train.mix(z) == W.mix(z)
        assert int(O.mix_np(np.array([z], np.uint64))[0]) == train.mix(z)
    for seed, e, slot, i in ((1, 0, 0, 0), (42, 3, 7, 2 ** 31 - 1), (2 ** 63 + 5, 19, 1, 12345)):
        want = train.mix(train.mix(train.mix(seed) ^ ((e << 32) | slot)) ^ i)
        assert O.draw(seed, e, slot, i) == want == W.draw(seed, e, slot, i)
        assert int(O.draw_np(seed, e, slot, np.array([i]))[0]) == want


def test_tables_and_initial_weights_agree(W):
    assert np.array_equal(W.sigmoid_table(), O.sigmoid_table())
    assert W.sigmoid_table()[500] == np.float32(0.5) and len(W.sigmoid_table()) == 1000
    a, b = W.initial_weights(7, 33, 10), O.init_weights(7, 33, 10)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert a.dtype == np.float32 and np.abs(a).max() <= 0.05 and len(np.unique(a)) > 300
    assert not np.array_equal(a, W.initial_weights(8, 33, 10))


def _corpus(seed=0, n_sessions=40, n_items=30):
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, 14, n_sessions)
    lens[3] = 1
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    aid = rng.integers(0, n_items, int(off[-1])).astype(np.int32)
    ty = rng.integers(0, 3, int(off[-1])).astype(np.int8)
    return off, aid, ty


def _setup(off, aid, ty, n_items=30, sample=0.0, seed=5, epoch=0, dim=8):
    keys, counts = O.build_vocab(aid, ty, None, 1)
    V = len(keys)
    rmap = np.full(n_items, -1, np.int32); rmap[keys] = np.arange(V)
    comp = O.compact(off, aid, ty, rmap, O.keep_thresholds(counts, sample), V, 7, seed, epoch)
    rng = np.random.default_rng(1)
    syn0 = (rng.random((V, dim), np.float32) - 0.5).astype(np.float32)
    syn1 = (rng.random((V, dim), np.float32) - 0.5).astype(np.float32)
    return comp, syn0, syn1, O.negative_table(counts), counts


def test_restatement_single_word_sentence_gives_no_update():
    off = np.array([0, 1], np.int64)
    (rows, orig, sid, coff), syn0, syn1, cum, _ = _setup(off, np.array([3], np.int32), np.zeros(1, np.int8))
    a0, a1, f0, f1 = O.batch(rows, orig, sid, coff, 0, 1, syn0, syn1, cum, O.sigmoid_table(), window=5, negative=5,
                             shift=32, batch_positions=8, seed=5, epoch=0, lr=0.025)
    assert not a0.any() and not a1.any() and not f0.any() and not f1.any()


def test_restatement_sample_zero_keeps_all_and_sampling_drops_some():
    off, aid, ty = _corpus()
    (rows, orig, sid, coff), *_ = _setup(off, aid, ty, sample=0.0)
    assert len(rows) == len(aid) and orig.tolist() == list(range(len(aid))) and np.array_equal(coff, off)
    (rows2, orig2, _, coff2), *_ = _setup(off, aid, ty, sample=1e-3)
    assert 0 < len(rows2) < len(aid) and coff2[-1] == len(rows2)
    assert set(orig2.tolist()) <= set(orig.tolist())


def test_restatement_batch_size_does_not_change_the_positions():
    off, aid, ty = _corpus(seed=2)
    (rows, orig, sid, coff), syn0, syn1, cum, _ = _setup(off, aid, ty)
    N = len(rows)
    kw = dict(window=4, negative=3, shift=32, seed=5, epoch=1, lr=0.025)
    seen = {}
    for B in (1, 7, N):
        v = []
        for b in range(math.ceil(N / B)):
            O.batch(rows, orig, sid, coff, b * B, min(N, (b + 1) * B), syn0, syn1, cum, O.sigmoid_table(),
                    batch_positions=B, visited=v, **kw)
        seen[B] = v
    assert seen[1] == seen[7] == seen[N] and len(seen[1]) == N
    # windows span the sentence only, never further than the window, and exclude the position itself
    for p, ctx in seen[1]:
        s = int(sid[p])
        assert len(ctx) <= min(2 * 4, int(coff[s + 1] - coff[s]) - 1)
    # with the same clamp the sums of one batch of N equal the sums over batches of 1 (integers: any order)
    one = O.batch(rows, orig, sid, coff, 0, N, syn0, syn1, cum, O.sigmoid_table(), batch_positions=N, **kw)
    acc = None
    for p in range(N):
        acc = O.batch(rows, orig, sid, coff, p, p + 1, syn0, syn1, cum, O.sigmoid_table(), batch_positions=N,
                      acc0=None if acc is None else acc[0], acc1=None if acc is None else acc[1],
                      flag0=None if acc is None else acc[2], flag1=None if acc is None else acc[3], **kw)
    assert all(np.array_equal(x, y) for x, y in zip(one, acc)) and one[0].any() and one[1].any()


def test_restatement_clamp_bound_cannot_wrap():
    for B, w, n in ((1, 1, 1), (512, 10, 5), (65536, 10, 5), (2 ** 30, 31, 32)):
        K = B * max(1 + n, 2 * w)
        C = O.clamp_of(B, w, n)
        assert C == 2.0 ** round(math.log2(C)) and K * int(C) <= 2 ** 62 < 2 ** 63 - 1
    x = np.array([np.inf, -np.inf, np.nan, 1e30, 0.5, -0.75], np.float32)
    C = O.clamp_of(512, 10, 5)
    assert O.fixed(x, 32, C).tolist() == [int(C), -int(C), 0, int(C), 2 ** 31, -3 * 2 ** 30]


def test_save_load_round_trip(W, tmp_path):
    rng = np.random.default_rng(0)
    m = W.Word2VecModel([5, 3, 9], rng.random((3, 4), np.float32), {"window": 10, "seed": 1})
    path = str(tmp_path / "sub" / "m.npz")
    m.save(path)
    back = W.Word2VecModel.load(path)
    assert back.wv.index_to_key.tolist() == [5, 3, 9]
    assert np.array_equal(back.wv.vectors.view(np.uint32), m.wv.vectors.view(np.uint32))
    assert back.params == {"window": 10, "seed": 1}
    # the cache rule of load_w2vec_model: an existing file is loaded, nothing is trained
    again = W.load_w2vec_model(path)
    assert again.wv.index_to_key.tolist() == [5, 3, 9]
    with pytest.raises(FileNotFoundError):
        W.load_w2vec_model(str(tmp_path / "none.npz"))


@pytest.mark.parametrize("bad", [{"sg": 1}, {"hs": 1}, {"cbow_mean": 0}])
def test_unsupported_family_raises(W, bad):
    with pytest.raises(NotImplementedError):
        W.train_w2vec_model(None, **bad)


def test_parameter_limits_and_config(W):
    from otto_recommender_amd import config
    with pytest.raises(ValueError):
        W.train_w2vec_model(None, vector_size=129)
    with pytest.raises(ValueError):
        W.train_w2vec_model(None, window=32)
    with pytest.raises(TypeError):
        W.train_w2vec_model(None, no_such_parameter=1)
    assert len(config.W2VEC_MODELS) == 3
    for name, m in config.W2VEC_MODELS.items():
        assert m["params"] == {"vector_size": 100, "window": 10, "min_count": 5} and m["k"] == 20
        assert m["types"] in ([0, 1, 2], [1, 2]) and m["first_n_aids"] == 600_000
        assert W.get_model_file(name).endswith(name + ".npz")
