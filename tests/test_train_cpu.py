"""Host pieces of the train stage and its numpy reference (tests/train_oracle.py): no GPU needed."""
import json
import math
import os

import numpy as np
import pytest

import rank_fixtures as RF
import train_oracle as O
from otto_recommender_amd import rank
from otto_recommender_amd import train as T

KAT = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kat_train.json")))
# the known answers are decimal and the tables take exp / log2 from the host's libm: a few ulp
KAT_REL = 1e-12


@pytest.fixture(scope="module")
def OT():
    return O.tables(1.0)


@pytest.mark.parametrize("k", [0, 1])
def test_known_answer_gradients(OT, k):
    s = KAT["sessions"][k]
    scores, labels = np.array(s["scores"]), np.array(s["labels"], np.int8)
    assert O.sorted_positions(scores) == s["sorted_rows"]
    assert O.inv_max_dcg(labels, 30, OT) == pytest.approx(s["inv_max_dcg"], rel=KAT_REL)
    g, h = O.gradients(scores, labels, np.array([0, len(scores)]), OT)
    assert g.tolist() == pytest.approx(s["g"], rel=KAT_REL) and h.tolist() == pytest.approx(s["h"], rel=KAT_REL)
    tables = T.build_tables(1.0)
    assert T.inv_max_dcg(labels, [0, len(labels)], 30, tables["gain"], tables["disc"])[0] == \
        pytest.approx(s["inv_max_dcg"], rel=KAT_REL)


@pytest.mark.parametrize("key,min_child", [("min_child_20", 20), ("min_child_1", 1)])
def test_known_answer_first_split(key, min_child):
    s, want = KAT["split"], KAT["split"][key]
    x = np.array(s["x"], np.int16)
    bounds, n_bins, lo, hi = O.find_bins(x)
    assert n_bins == 10 and (lo, hi) == (0.0, 9.0)
    bins = O.bin_column(x, bounds)[:, None]
    H = O.histogram(bins, np.array(s["q_g"]), np.array(s["q_h"]), np.arange(40), [0])[0]
    got = O.best_split_of_feature(H, n_bins, math.ldexp(1.0, s["e_g"] - 15), math.ldexp(1.0, s["e_h"] - 15), min_child,
                                  1e-3, 0.0)
    assert got[0] == want["gain"] and got[1] == want["bin"] and got[4] == want["count_left"]
    assert bounds[got[1]] == want["threshold"] == T.find_bins(x)["bounds"][got[1]]


@pytest.mark.parametrize("seed", range(4))
def test_split_equals_an_exhaustive_search_on_raw_values(seed):
    rng = np.random.default_rng(seed)
    n = 500
    x = RF.random_column(rng, RF.DTYPES[seed % 4], n)
    if x.dtype.kind == "f":
        x[np.isnan(x)] = np.float32(2.5)
    qg, qh = rng.integers(-(1 << 15), (1 << 15) + 1, n), rng.integers(0, (1 << 15) + 1, n)
    eg, eh, mc, mh, l2 = -2, 3, 20, 1e-3, 0.0
    sg, sh = math.ldexp(1.0, eg - 15), math.ldexp(1.0, eh - 15)
    best = None
    G, Hs = int(qg.sum()) * sg, int(qh.sum()) * sh
    for v in np.unique(x.astype(np.float64))[:-1]:
        left = x.astype(np.float64) <= v
        if left.sum() < mc or (~left).sum() < mc:
            continue
        GL, HL = int(qg[left].sum()) * sg, int(qh[left].sum()) * sh
        GR, HR = int(qg[~left].sum()) * sg, int(qh[~left].sum()) * sh
        if HL < mh or HR < mh:
            continue
        gain = (GL * GL / (HL + l2) + GR * GR / (HR + l2)) - G * G / (Hs + l2)
        if gain > 0 and (best is None or gain > best[0]):
            best = (gain, float(v), int(left.sum()))
    bounds, n_bins, _, _ = O.find_bins(x)
    H = O.histogram(O.bin_column(x, bounds)[:, None], qg, qh, np.arange(n), [0])[0]
    got = O.best_split_of_feature(H, n_bins, sg, sh, mc, mh, l2)
    assert best is not None and got[0] == best[0] and got[4] == best[2]
    # the written threshold separates the same rows as the raw value
    assert np.array_equal(x.astype(np.float64) <= bounds[got[1]], x.astype(np.float64) <= best[1])


def _bin_cases():
    rng = np.random.default_rng(11)
    cases = {}
    for D in (1, 2, 255, 256, 257):
        cases[f"D{D}"] = rng.choice(np.arange(D, dtype=np.int32) * 3 - 100, size=4000).astype(np.int32)
        cases[f"D{D}"][:D] = np.arange(D, dtype=np.int32) * 3 - 100
    heavy = rng.integers(0, 1000, 5000).astype(np.int16)
    heavy[rng.random(5000) < 0.7] = 17  # one value holds most rows
    cases["heavy_ties"] = heavy
    big = (1 << 24) + rng.integers(0, 400, 3000).astype(np.int32)  # float32 cannot tell these apart
    cases["int32_beyond_2^24"] = np.concatenate([big, -big]).astype(np.int32)
    base = np.float32(1.0)
    near = [base]
    for _ in range(300):
        near.append(np.nextafter(near[-1], np.float32(2)))
    cases["float32_neighbours"] = rng.choice(np.array(near, np.float32), size=3000)
    cases["float32_edges"] = np.concatenate([RF.F32_EDGES[~np.isnan(RF.F32_EDGES)], rng.normal(size=500).astype(np.float32)])
    return cases


@pytest.mark.parametrize("name,col", list(_bin_cases().items()))
def test_find_bins(name, col):
    b = T.find_bins(col, 255)
    ob = O.find_bins(col, 255)
    assert np.array_equal(b["bounds"], ob[0]) and (b["n_bins"], b["min"], b["max"]) == ob[1:]
    D = len(np.unique(col.astype(np.float64) + 0.0))
    assert b["n_bins"] == min(D, 255) if D <= 255 else 2 <= b["n_bins"] <= 255
    assert len(b["bounds"]) == b["n_bins"] - 1 and np.all(np.isfinite(b["bounds"])) and np.all(np.diff(b["bounds"]) > 0)
    v = col.astype(np.float64)
    bins = T.bin_values(col, b["bounds"])
    assert np.array_equal(bins, O.bin_column(col, ob[0]))
    order = np.argsort(v, kind="stable")
    assert np.all(np.diff(bins[order]) >= 0) and bins.min() == 0 and bins.max() == b["n_bins"] - 1  # monotone
    for x in np.unique(v):
        assert len(np.unique(bins[v == x])) == 1  # equal values in equal bins
    for k, thr in enumerate(b["bounds"]):
        assert np.array_equal(v <= thr, bins <= k), (name, k)


def test_feature_draw_count_and_determinism():
    valid = [0, 2, 3, 5, 8, 9, 10, 11, 12, 13, 14, 20]
    for frac, k in ((0.25, 3), (0.01, 1), (1.0, 12), (0.5, 6), (0.29, 3), (0.3, 4)):
        d = T.feature_draw(valid, frac, 42, 0)
        assert len(d) == k and d == sorted(d) and set(d) <= set(valid)
    draws = [tuple(T.feature_draw(valid, 0.25, 42, t)) for t in range(40)]
    assert draws == [tuple(T.feature_draw(valid, 0.25, 42, t)) for t in range(40)]
    assert draws == [tuple(O.feature_draw(valid, 0.25, 42, t)) for t in range(40)]
    assert len(set(draws)) > 10 and draws != [tuple(T.feature_draw(valid, 0.25, 43, t)) for t in range(40)]
    assert set(f for d in draws for f in d) == set(valid)
    assert T.feature_draw([], 0.25, 42, 0) == []
    from otto_recommender_amd import _lib
    assert T.mix(T.mix(42) ^ ((7 << 32) | 9)) == _lib.load().ottohip_downsample_hash(42, 7, 9)


def test_log2_table_form_is_within_1e_7():
    L = T.build_tables(1.0)["log2t"]
    rng = np.random.default_rng(2)
    xs = np.concatenate([np.exp2(rng.uniform(0, 40, 20000)), [1.0, 2.0, 1.0 + 2 ** -40, 2.0 ** 40, 3.0, 1.5]])
    err = max(abs(T.log2_table_form(x, L) - math.log2(x)) for x in xs)
    assert err < 1e-7
    OT = O.tables(1.0)
    assert all(T.log2_table_form(x, L) == O.log2_form(float(x), OT) for x in xs[:500])


def test_tables_are_the_same_data_in_product_and_reference():
    a, b = T.build_tables(1.0), O.tables(1.0)
    for k in ("gain", "disc", "sig", "log2t"):
        assert a[k].tolist() == b[k], k
    assert (a["sig_min"], a["sig_max"], a["sig_factor"]) == (b["sig_min"], b["sig_max"], b["factor"])
    assert a["sig"][1 << 19] == 0.5 and a["disc"][0] == 1.0 and a["gain"][30] == 2.0 ** 30 - 1


@pytest.fixture(scope="module")
def fitted():
    """a reference fit on a small frame and the product's text of its trees"""
    rng = np.random.default_rng(8)
    sizes = rng.integers(0, 40, 80)
    off = np.r_[0, np.cumsum(sizes)].astype(np.int64)
    n = int(off[-1])
    cols = {f"c{i}": RF.random_column(rng, RF.DTYPES[i % 4], n) for i in range(6)}
    for c in cols.values():
        if c.dtype.kind == "f":
            c[np.isnan(c)] = np.float32(0.5)
    cols["const"] = np.full(n, 3, np.int8)
    y = (rng.random(n) < 0.1).astype(np.int8)
    params = T.resolve_params(dict(n_estimators=5, min_child_samples=5, eval_every=2))
    block = [ln for ln in T.model_text([], ["a"], [T.find_bins(np.arange(3))], params).splitlines() if ln.startswith("[")]
    ref = O.fit(cols, list(cols), y, off, dict(n_estimators=5, min_child_samples=5, eval_every=2), params_block=block)
    info = [T.find_bins(cols[n_]) for n_ in cols]
    return dict(cols=cols, ref=ref, text=T.model_text(ref["trees"], list(cols), info, params))


def test_written_text_parses_and_tree_sizes_are_true(fitted):
    text = fitted["text"]
    assert text == fitted["ref"]["text"] and len(fitted["ref"]["trees"]) == 5
    f = rank.parse_booster(text, columns=list(fitted["cols"]))
    assert f.n_trees == 5 and f.objective == "lambdarank" and f.version == "v3"
    assert np.all(f.decision_type == 2) and np.all(f.shrinkage == 0.25)
    raw = text.encode()
    head = dict(ln.split("=", 1) for ln in text.split("\n\n")[0].splitlines() if "=" in ln)
    assert head["feature_infos"].split()[-1] == "none" and head["feature_infos"].split()[0].startswith("[")
    sizes = [int(x) for x in head["tree_sizes"].split()]
    pos = raw.index(b"Tree=0")
    assert raw[:pos].endswith(b"\n\n")
    for i, sz in enumerate(sizes):  # LightGBM's loader seeks from tree to tree by these
        block = raw[pos:pos + sz]
        assert block.startswith(f"Tree={i}\n".encode()) and block.endswith(b"\n\n\n") and block.count(b"Tree=") == 1
        pos += sz
    assert raw[pos:].startswith(b"end of trees\n")
    assert "feature_importances:" in text and "[lambdarank_truncation_level: 30]" in text


def test_unsupported_settings_raise():
    for bad in (dict(subsample_freq=1), dict(bagging_freq=5), dict(lambda_l1=0.1), dict(reg_alpha=1.0),
                dict(boosting_type="dart"), dict(categorical_feature=[0]), dict(max_bin=1000), dict(no_such_thing=1)):
        with pytest.raises(ValueError):
            T.resolve_params(bad)
    p = T.resolve_params(dict(subsample=0.5))  # accepted, no effect
    assert p["n_estimators"] == 150 and p["colsample_bytree"] == 0.25 and p["seed"] == 42 and p["max_bin"] == 255
    with pytest.raises(ValueError):
        T.find_bins(np.array([1.0, np.nan, 2.0], np.float32))
    with pytest.raises(ValueError):
        T._typed_columns(np.array([[1.0, np.nan]]), ["a", "b"])


def test_split_files_to_train_valid():
    files = [f"f{i}" for i in range(8)]
    assert T.split_files_to_train_valid(files, 0) == (files, None)
    assert T.split_files_to_train_valid(files, 0.25) == (files[:6], files[6:])
    assert T.split_files_to_train_valid(files, 0.25, 2, 1) == (files[:2], files[6:7])
    assert T.split_files_to_train_valid(files[:2], 0.9) == ([], files[:2])  # int(0.1 * 2) = 0, as the reference
    with pytest.raises(ValueError):
        T.split_files_to_train_valid(files[:1], 0.5)


def test_matrix_columns_are_typed_without_loss():
    M = np.array([[1.0, 0.5, 2.0 ** 30], [-3.0, np.float64(np.float32(0.1)), 7.0]])
    c = T._typed_columns(M, ["a", "b", "c"])
    assert [c[k].dtype.name for k in "abc"] == ["int32", "float32", "int32"]
    assert all(np.array_equal(c[k].astype(np.float64), M[:, j]) for j, k in enumerate("abc"))
    with pytest.raises(ValueError):
        T._typed_columns(np.array([[0.1]]), ["a"])  # float64 0.1 is not a float32
