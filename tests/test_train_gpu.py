"""Train stage on the GPU against tests/train_oracle.py, bit for bit: float64 compared as uint64, integers exactly,
model files byte for byte. References are computed once per module."""
import os

import numpy as np
import pytest

import rank_fixtures as RF
import train_oracle as O

pytestmark = pytest.mark.gpu


def _u64(x):
    return np.ascontiguousarray(np.asarray(x, np.float64)).view(np.uint64)


def _same_f64(a, b, what=""):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, what
    bad = np.flatnonzero(_u64(a) != _u64(b))
    assert len(bad) == 0, (what, len(bad), bad[:5], a[bad[:5]], b[bad[:5]])


@pytest.fixture(scope="module")
def T(gpu):
    from otto_recommender_amd import train
    return train


@pytest.fixture(scope="module")
def OT():
    return O.tables(1.0)


def _dev(gpu, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", gpu.device))


def _frame(rng, sizes, special=()):
    """scores with ties and int8 labels (mostly 0) of sessions of the given sizes; special: {session: kind}"""
    special = dict(special)
    sc, lb = [], []
    for s, n in enumerate(sizes):
        x = np.round(rng.normal(size=n) * 2, 1)
        y = ((rng.random(n) < 0.12).astype(np.int8) + 2 * (rng.random(n) < 0.03).astype(np.int8)).astype(np.int8)
        kind = special.get(s)
        if kind == "labels_equal":
            y[:] = 1
        elif kind == "scores_equal":
            x[:] = 0.5
            y = rng.integers(0, 3, n).astype(np.int8)
        elif kind == "zeros":
            x = rng.choice(np.array([0.0, -0.0, 1.0, -1.0]), size=n)
            y = rng.integers(0, 3, n).astype(np.int8)
        elif kind == "far":
            x = np.round(rng.normal(size=n) * 40, 1)  # |d| beyond the sigmoid table's +-25
            y = rng.integers(0, 4, n).astype(np.int8)
        elif kind == "labels30":
            y = rng.integers(0, 31, n).astype(np.int8)
            y[:2] = (30, 0)
        sc.append(x)
        lb.append(y)
    off = np.r_[0, np.cumsum(sizes)].astype(np.int64)
    return np.concatenate(sc).astype(np.float64), np.concatenate(lb).astype(np.int8), off


def _grad(gpu, T, scores, labels, off, trunc=30, norm=True):
    tb = T.Tables(1.0, trunc, norm, ctx=gpu)
    g, h = T.lambdarank_gradients(_dev(gpu, scores), _dev(gpu, labels), _dev(gpu, off), tb)
    return g, h


@pytest.fixture(scope="module")
def grads(gpu, T, OT):
    """every listed session size, both sides of the path switch, 10,000 rows, and the special cases, norm on and
    truncation 30: the device's (g, h) and the reference's"""
    rng = np.random.default_rng(5)
    L = T.lds_rows()
    sizes = [1, 2, 3, 29, 30, 31, 63, 64, 65, 255, 256, 257, L - 1, L, L + 1, 10000, 31, 64, 30, 65, 65, 0, 40]
    special = {16: "labels_equal", 17: "scores_equal", 18: "zeros", 19: "far", 20: "labels30"}
    scores, labels, off = _frame(rng, sizes, special)
    g, h = _grad(gpu, T, scores, labels, off)
    rg, rh = O.gradients(scores, labels, off, OT)
    return dict(sizes=sizes, scores=scores, labels=labels, off=off, g=g, h=h, rg=rg, rh=rh)


def test_gradients_equal_the_reference_at_every_size_and_case(grads):
    g, h = grads["g"].cpu().numpy(), grads["h"].cpu().numpy()
    off = grads["off"]
    for s, n in enumerate(grads["sizes"]):
        a, b = off[s], off[s + 1]
        _same_f64(g[a:b], grads["rg"][a:b], ("g", s, n))
        _same_f64(h[a:b], grads["rh"][a:b], ("h", s, n))
    a, b = off[16], off[17]
    assert not g[a:b].any() and not h[a:b].any()  # all labels equal
    assert np.abs(grads["rg"]).max() > 0


@pytest.mark.parametrize("trunc,norm", [(1, True), (30, False), (1, False)])
def test_gradients_truncation_and_norm(gpu, T, OT, trunc, norm):
    rng = np.random.default_rng(6)
    sizes = [1, 2, 3, 29, 30, 31, 65, 257, 33]
    scores, labels, off = _frame(rng, sizes, {8: "scores_equal"})
    g, h = _grad(gpu, T, scores, labels, off, trunc, norm)
    rg, rh = O.gradients(scores, labels, off, OT, trunc, norm)
    _same_f64(g.cpu().numpy(), rg, "g")
    _same_f64(h.cpu().numpy(), rh, "h")


def test_session_of_10001_rows_is_the_engine_limit(gpu, T):
    from otto_recommender_amd import _lib
    scores = np.zeros(10001)
    labels = np.zeros(10001, np.int8)
    labels[0] = 1
    with pytest.raises(_lib.OttoHipError) as e:
        _grad(gpu, T, scores, labels, np.array([0, 10001], np.int64))
    assert e.value.rc == _lib.OTTOHIP_ELIMIT


def test_quantiser_exponents_and_integers(gpu, T, grads):
    gh, eg, eh, zero = T.quantise(grads["g"], grads["h"], gpu)
    qg, qh, reg, reh, rzero = O.quantise(grads["rg"], grads["rh"])
    assert (eg, eh, zero) == (reg, reh, rzero) and not zero
    got = gh.cpu().numpy().astype(np.int64)
    assert np.array_equal(got[:, 0], qg) and np.array_equal(got[:, 1], qh)
    assert np.abs(got).max() <= 1 << 15 and np.abs(got[:, 0]).max() >= 1 << 14
    # halves round to even: g = 2.5 and 3.5 units of the scale under a maximum of 2^14 units
    g = np.array([16384.0, 2.5, 3.5, -2.5, -0.5])
    gh, eg, eh, zero = T.quantise(_dev(gpu, g), _dev(gpu, np.abs(g)), gpu)
    assert eg == 15 and gh.cpu().numpy()[:, 0].tolist() == [16384, 2, 4, -2, 0]


def test_quantiser_reports_all_zero(gpu, T):
    z = _dev(gpu, np.zeros(100))
    gh, eg, eh, zero = T.quantise(z, z, gpu)
    assert zero and not gh.cpu().numpy().any()


@pytest.fixture(scope="module")
def hist_world(gpu):
    """a binned matrix of 105 features (stride 108): feature 0 has 2 bins, feature 1 has 255, the others random"""
    rng = np.random.default_rng(9)
    n, F, stride = 3 * (1 << 15) + 77, 105, 108
    bins = np.zeros((n, stride), np.uint8)
    bins[:, :F] = rng.integers(0, 256, (n, F), dtype=np.uint8)
    bins[:, 0] = rng.integers(0, 2, n)
    bins[:, 1] = rng.integers(0, 255, n)
    bins[:, 2] = (rng.integers(0, 16, n) ** 2) % 256  # hot bins
    gh = rng.integers(-(1 << 15), (1 << 15) + 1, (n, 2)).astype(np.int32)
    return dict(n=n, F=F, bins=bins, gh=gh, d_bins=_dev(gpu, bins), d_gh=_dev(gpu, gh), rng=rng)


def _hist_check(gpu, T, w, rows, feats, max_blocks=0):
    got = T.histograms(w["d_bins"], w["d_gh"], _dev(gpu, rows.astype(np.int32)), _dev(gpu, np.asarray(feats, np.int32)),
                       max_blocks, gpu).cpu().numpy()
    ref = O.histogram(w["bins"].astype(np.int64), w["gh"][:, 0].astype(np.int64), w["gh"][:, 1].astype(np.int64), rows,
                      list(feats))
    assert np.array_equal(got, ref)


@pytest.mark.parametrize("m", [0, 1, 63, 64, 65, (1 << 15) - 1, 1 << 15, (1 << 15) + 1, 3 << 15])
def test_histogram_row_list_sizes(gpu, T, hist_world, m):
    w = hist_world
    rows = np.sort(w["rng"].choice(w["n"], size=m, replace=False)) if m else np.zeros(0, np.int64)  # scattered
    _hist_check(gpu, T, w, rows, [0, 1, 2, 50, 104])
    if m >= 1 << 15:
        _hist_check(gpu, T, w, rows, [0, 1, 2, 50, 104], max_blocks=1)  # one workgroup: the 2^15-row flush


@pytest.mark.parametrize("k", [1, 3, 4, 5, 26, 105])
def test_histogram_drawn_feature_counts(gpu, T, hist_world, k):
    w = hist_world
    feats = np.sort(w["rng"].choice(w["F"], size=k, replace=False)) if k < 105 else np.arange(105)
    rows = w["rng"].permutation(w["n"])[:5000]  # scattered, unordered
    _hist_check(gpu, T, w, rows, feats)


@pytest.mark.parametrize("max_blocks", [0, 1])
def test_histogram_overflow_case_one_bin_at_full_scale(gpu, T, max_blocks):
    n = 3 << 15
    bins = np.full((n, 4), 7, np.uint8)
    gh = np.full((n, 2), 1 << 15, np.int32)
    got = T.histograms(_dev(gpu, bins), _dev(gpu, gh), _dev(gpu, np.arange(n, dtype=np.int32)),
                       _dev(gpu, np.array([0, 3], np.int32)), max_blocks, gpu).cpu().numpy()
    want = np.zeros((2, 256, 3), np.int64)
    want[:, 7] = (n << 15, n << 15, n)
    assert np.array_equal(got, want)
    gh[:, 0] = -(1 << 15)
    got = T.histograms(_dev(gpu, bins), _dev(gpu, gh), _dev(gpu, np.arange(n, dtype=np.int32)),
                       _dev(gpu, np.array([1], np.int32)), max_blocks, gpu).cpu().numpy()
    assert got[0, 7].tolist() == [-(n << 15), n << 15, n] and np.count_nonzero(got) == 3


def test_split_scan_equals_the_reference(gpu, T, hist_world):
    w = hist_world
    feats = [0, 1, 2, 50]
    n_bins = [2, 255, 226, 256]
    rows = w["rng"].permutation(w["n"])[:3000]
    qg, qh = w["gh"][:, 0].astype(np.int64), np.abs(w["gh"][:, 1]).astype(np.int64)
    H = O.histogram(w["bins"].astype(np.int64), qg, qh, rows, feats)
    rec = T.split_scan(_dev(gpu, H[None]), _dev(gpu, np.array(n_bins, np.int32)), -3, 2, 20, 1e-3, 0.0, gpu)[0]
    import math
    for j in range(len(feats)):
        ref = O.best_split_of_feature(H[j], n_bins[j], math.ldexp(1.0, -18), math.ldexp(1.0, -13), 20, 1e-3, 0.0)
        if ref is None:
            assert rec[j][1] == -1
            continue
        assert _u64(rec[j][0]) == _u64(ref[0]) and rec[j][1:5] == ref[1:]
        assert rec[j][5:] == (int(H[j, :, 0].sum()), int(H[j, :, 1].sum()), len(rows))


@pytest.mark.parametrize("m", [0, 1, 255, 256, 257, 5000])
def test_partition_is_stable_and_equals_the_reference(gpu, T, hist_world, m):
    w = hist_world
    rows = w["rng"].permutation(w["n"])[:m].astype(np.int32)
    out, n_left = T.partition(w["d_bins"], 50, 100, _dev(gpu, rows), gpu)
    left, right = O.partition(w["bins"], rows.tolist(), 50, 100)
    assert n_left == len(left) and out.cpu().numpy().tolist() == left + right


# ---------------------------------------------------------------- end to end
PARAMS = dict(n_estimators=8, eval_every=3)


def _e2e_frame(seed, n_sessions=300):
    rng = np.random.default_rng(seed)
    sizes = rng.integers(0, 61, n_sessions)
    off = np.r_[0, np.cumsum(sizes)].astype(np.int64)
    n = int(off[-1])
    cols = {}
    for i in range(12):
        c = RF.random_column(rng, RF.DTYPES[i % 4], n)
        if c.dtype.kind == "f":
            c[np.isnan(c)] = np.float32(0.25)
        cols[f"c{i}"] = c
    y = ((rng.random(n) < 0.06).astype(np.int8) + 3 * (rng.random(n) < 0.01).astype(np.int8)).astype(np.int8)
    y = np.where((cols["c1"] > 100) & (rng.random(n) < 0.5), y + 1, y).astype(np.int8)  # something to learn
    return cols, y, off, sizes


def _params_block(p):
    out = []
    for k in sorted(p):
        v = p[k]
        if isinstance(v, np.ndarray):
            v = ",".join("%.17g" % x for x in v)
        elif isinstance(v, bool):
            v = int(v)
        out.append(f"[{k}: {v}]")
    return out


@pytest.fixture(scope="module")
def e2e(gpu, T):
    cols, y, off, sizes = _e2e_frame(21)
    vcols, vy, voff, vsizes = _e2e_frame(22, 80)
    dcols = {n: _dev(gpu, v) for n, v in cols.items()}
    model, hist = T.fit_lgbm(dcols, y, sizes, list(cols), {n: _dev(gpu, v) for n, v in vcols.items()}, vy, vsizes,
                             ctx=gpu, **PARAMS)
    ref = O.fit(cols, list(cols), y, off, PARAMS, valid=(vcols, vy, voff), params_block=_params_block(model.params))
    return dict(cols=cols, dcols=dcols, y=y, off=off, sizes=sizes, model=model, hist=hist, ref=ref)


def test_model_text_and_history_equal_the_reference(e2e):
    assert len(e2e["model"].trees) == 8
    assert e2e["model"].text.encode() == e2e["ref"]["text"].encode()
    assert e2e["hist"]["iteration"] == [3, 6, 8]
    for k in ("iteration", "train", "valid"):
        assert e2e["hist"][k] == e2e["ref"]["history"][k], k
    _same_f64(e2e["model"].scores.cpu().numpy(), e2e["ref"]["scores"], "scores")


@pytest.mark.parametrize("variant", [dict(num_leaves=2), dict(max_depth=-1, num_leaves=31),
                                     dict(colsample_bytree=1.0), dict(min_child_samples=100000)],
                         ids=["two_leaves", "no_depth_limit_31_leaves", "all_features", "no_split_possible"])
def test_variants_equal_the_reference(gpu, T, e2e, variant):
    from otto_recommender_amd import rank
    p = dict(PARAMS, n_estimators=4, **variant)
    model, hist = T.fit_lgbm(e2e["dcols"], e2e["y"], e2e["sizes"], list(e2e["cols"]), ctx=gpu, **p)
    ref = O.fit(e2e["cols"], list(e2e["cols"]), e2e["y"], e2e["off"], p, params_block=_params_block(model.params))
    assert model.text.encode() == ref["text"].encode()
    assert hist == ref["history"]
    f = rank.parse_booster(model.text, columns=list(e2e["cols"]))
    if "min_child_samples" in variant:
        assert f.n_trees == 0 and hist["iteration"] == [0]
    else:
        assert f.n_trees == 4
        if "num_leaves" in variant:
            assert f.num_leaves.max() == variant["num_leaves"]


def test_two_fits_give_identical_bytes(gpu, T, e2e):
    model, _ = T.fit_lgbm(e2e["dcols"], e2e["y"], e2e["sizes"], list(e2e["cols"]), ctx=gpu, **dict(PARAMS, n_estimators=4))
    again, _ = T.fit_lgbm(e2e["dcols"], e2e["y"], e2e["sizes"], list(e2e["cols"]), ctx=gpu, **dict(PARAMS, n_estimators=4))
    assert model.text.encode() == again.text.encode()


def test_ranker_predicts_the_trainers_scores(gpu, T, e2e, tmp_path):
    from otto_recommender_amd import rank
    path = T.save_lgbm(e2e["model"], str(tmp_path / "clicks"))
    assert path.endswith("clicks.booster.lgbm")
    r = rank.Ranker({"clicks": path}, gpu, columns=[(n, v.dtype) for n, v in e2e["cols"].items()])
    try:
        pred = r.predict(e2e["dcols"])["clicks"].cpu().numpy()
    finally:
        r.free()
    _same_f64(pred, e2e["model"].scores.cpu().numpy(), "Ranker.predict")
    assert np.unique(pred).size > 8


def test_it_learns_a_threshold_label(gpu, T):
    rng = np.random.default_rng(3)
    sizes = rng.integers(5, 40, 150)
    n = int(sizes.sum())
    c0 = rng.integers(0, 200, n).astype(np.int32)  # one bin per value: the label's threshold is a bin boundary
    cols = {"c0": c0, "c1": (c0 // 10).astype(np.int16)}
    y = (c0 > 150).astype(np.int8)  # rows are in random order inside their sessions
    model, hist = T.fit_lgbm({k: _dev(gpu, v) for k, v in cols.items()}, y, sizes, ["c0", "c1"], ctx=gpu,
                             n_estimators=5, eval_every=1, colsample_bytree=1.0)
    zero, _ = T.fit_lgbm({k: _dev(gpu, v) for k, v in cols.items()}, y, sizes, ["c0", "c1"], ctx=gpu, n_estimators=0)
    assert zero.history["iteration"] == [0] and zero.history["train"][0] < 1.0
    assert hist["train"][-1] == 1.0


def test_train_files_feeds_rank_files(gpu, T, tmp_path):
    import pandas as pd
    import feats_fixtures as X
    from otto_recommender_amd import candidates as C
    from otto_recommender_amd import downsample as D
    from otto_recommender_amd import rank
    args = X.random_fixture(n_sessions=120)
    tmp = str(tmp_path)
    C.retrieve_and_gen_feats(*args, file_out=os.path.join(tmp, "retrieved", "part0.parquet"))
    D.downsample_files(os.path.join(tmp, "retrieved"), os.path.join(tmp, "downsampled"))
    res = T.train_files(os.path.join(tmp, "downsampled"), os.path.join(tmp, "lgbm"), ctx=gpu, n_estimators=3,
                        min_child_samples=2)
    for t in ("clicks", "carts", "orders"):
        assert os.path.basename(res[t]["path"]) == f"{t}.booster.lgbm" and len(res[t]["model"].trees) == 3, t
    written = rank.rank_files(os.path.join(tmp, "retrieved"), os.path.join(tmp, "lgbm"), os.path.join(tmp, "ranked"))
    assert len(written) == 3
    for path in written:
        df = pd.read_parquet(path)
        assert len(df) and df["pred_rank"].min() == 1 and df["pred_score"].nunique() > 1


def test_nan_score_is_reported_and_writes_nothing(gpu, T):
    from otto_recommender_amd import _lib
    rng = np.random.default_rng(4)
    scores, labels, off = _frame(rng, [40, 300, 7])
    scores[45] = np.nan
    with pytest.raises(_lib.OttoHipError) as e:
        _grad(gpu, T, scores, labels, off)
    assert e.value.rc == -2 and "NaN" in str(e.value)


def test_gradients_without_sessions_are_zero(gpu, T):
    import torch
    tb = T.Tables(ctx=gpu)
    g, h = T.lambdarank_gradients(_dev(gpu, np.ones(50)), _dev(gpu, np.ones(50, np.int8)),
                                  _dev(gpu, np.zeros(1, np.int64)), tb, inv_max=torch.zeros(1, dtype=torch.float64,
                                                                                            device=f"cuda:{gpu.device}"))
    assert not g.cpu().numpy().any() and not h.cpu().numpy().any()


def test_stage_wrappers_refuse_tensors_the_kernels_would_misread(gpu, T, hist_world):
    w = hist_world
    rows64 = _dev(gpu, np.arange(10, dtype=np.int64))
    feats = _dev(gpu, np.array([0, 1], np.int32))
    with pytest.raises(TypeError):
        T.histograms(w["d_bins"], w["d_gh"], rows64, feats, 0, gpu)
    with pytest.raises(TypeError):
        T.histograms(w["d_bins"][:, :8], w["d_gh"], rows64.int(), feats, 0, gpu)  # a view that is not contiguous
    with pytest.raises(TypeError):
        T.partition(w["d_bins"], 0, 1, rows64, gpu)
    with pytest.raises(TypeError):
        T.apply_tree(w["d_bins"], {"num_leaves": 1, "leaf_value": [0.0]}, _dev(gpu, np.zeros(w["n"], np.float32)), gpu)


def test_trainer_handle_reads_back_what_it_boosted(gpu, T, e2e):
    """the handle alone: its trees are the fit's trees, tree before a boost is an error, scores are a copy"""
    from otto_recommender_amd import _lib
    import torch
    cols = e2e["cols"]
    binner = T.Binner(e2e["dcols"], list(cols), 255, gpu)
    bins = binner.bin_frame(e2e["dcols"])
    p = T.resolve_params(PARAMS)
    tr = T.Trainer(bins, _dev(gpu, e2e["y"]), _dev(gpu, e2e["off"]), binner.n_bins, p, gpu)
    with pytest.raises(_lib.OttoHipError):
        tr.last_tree()
    assert not tr.scores.cpu().numpy().any()
    for i in range(3):
        assert tr.boost_one()
        assert tr.trees[i] == {k: v for k, v in e2e["ref"]["trees"][i].items() if k != "leaf_rows"}
    s = tr.scores
    s.zero_()
    assert tr.scores.cpu().numpy().any()
    tr.free()
