"""Submission scoring on the GPU against tests/downsample_oracle.py: the six integer sums exactly."""
import numpy as np
import pandas as pd
import pytest

import downsample_oracle as O
import rank_fixtures as RF

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def case():
    """~2,000 sessions with the cases of the metric planted; {type: (session, aid)} and the label rows"""
    rng = np.random.default_rng(31)
    lab, sub = [], {t: ([], []) for t in O.TARGETS}

    def put(name, s, aids):
        sub[name][0].extend([s] * len(aids))
        sub[name][1].extend(int(a) for a in aids)

    for s in range(50_000, 52_000):
        for t, name in enumerate(O.TARGETS):
            kind = rng.integers(0, 10)
            n_lab = 0 if kind == 0 else int(rng.integers(1, 4)) if kind < 8 else int(rng.integers(15, 40))
            aids = rng.choice(200, size=n_lab, replace=False)
            lab += [(s, int(a), t) for a in aids]
            if kind == 1:
                continue  # labels only
            n_sub = int(rng.integers(0, 21))
            picks = rng.integers(0, 200, n_sub)
            if n_lab and n_sub:
                picks[:rng.integers(0, min(n_lab, n_sub) + 1)] = aids[:1]  # hits, some of them repeated
            put(name, s, picks)
    lab += [(7, 1, 0), (7, 2, 1), (2147483647, 3, 2)]            # sessions only in the labels
    put("clicks", 9, [1, 2, 3]); put("orders", -5, [4])         # sessions only in the submission
    lab += [(60_000, a, 1) for a in range(100)]                  # 100 labels: true clips at 20, hits count them all
    put("carts", 60_000, list(range(70, 134)))                   # a 64-long list with 30 of the labels
    lab += [(60_001, 5, 2), (60_001, 6, 2)]
    put("orders", 60_001, [5] * 30 + [6])                        # one label submitted 30 times
    lab += [(60_002, 1, 0)]
    put("clicks", 60_002, [])                                    # an empty list
    labels = pd.DataFrame(lab, columns=["session", "aid", "type"])
    labels = pd.concat([labels, labels.iloc[::50]], ignore_index=True)  # duplicate rows are deduplicated
    return sub, labels, O.recall_sums(sub, labels)


def _frames(sub):
    return {t: pd.DataFrame({"session": np.asarray(v[0], np.int32), "aid_next": np.asarray(v[1], np.int32)})
            for t, v in sub.items()}


def test_sums_equal_the_oracle(gpu, case):
    import torch
    from otto_recommender_amd import submission as SB
    sub, labels, ref = case
    assert ref[2] >= 30 and all(x > 0 for x in ref)
    frames = _frames(sub)
    assert SB.recall_sums(frames, labels, gpu) == ref
    dev = torch.device("cuda", gpu.device)
    tensors = {t: {c: torch.from_numpy(f[c].to_numpy()).to(dev) for c in f.columns} for t, f in frames.items()}
    assert SB.recall_sums(tensors, labels, gpu) == ref
    # the metric is a sum over sessions: row order inside the submission does not matter
    rng = np.random.default_rng(1)
    shuffled = {t: f.iloc[rng.permutation(len(f))].reset_index(drop=True) for t, f in frames.items()}
    assert SB.recall_sums(shuffled, labels, gpu) == ref
    assert SB.eval_ranked(frames, labels, gpu) == O.recall_from_sums(ref)


def test_planted_cases_alone(gpu):
    from otto_recommender_amd import submission as SB
    L = lambda rows: pd.DataFrame(rows, columns=["session", "aid", "type"])
    F = lambda s, a: pd.DataFrame({"session": np.asarray(s, np.int32), "aid_next": np.asarray(a, np.int32)})
    # labels only; submission only; both absent types
    assert SB.recall_sums({}, L([(1, 5, 0), (1, 6, 0), (2, 5, 2)]), gpu) == [0, 2, 0, 0, 0, 1]
    assert SB.recall_sums({"clicks": F([1, 1], [5, 6])}, L([]).astype(np.int64), gpu) == [0] * 6
    # a 64-long list against 100 labels: 30 hits, true = 100 clipped to 20
    got = SB.recall_sums({"carts": F([3] * 64, range(70, 134))}, L([(3, a, 1) for a in range(100)]), gpu)
    assert got == [0, 0, 30, 20, 0, 0]
    # a label submitted three times beside one never submitted: hit 3, true 3 + 1
    got = SB.recall_sums({"orders": F([4] * 4, [9, 9, 9, 3])}, L([(4, 9, 2), (4, 8, 2)]), gpu)
    assert got == [0, 0, 0, 0, 3, 4]
    assert SB.eval_ranked({}, L([]).astype(np.int64), gpu) == {"clicks": 0.0, "carts": 0.0, "orders": 0.0, "total": 0.0}


def test_argument_errors_before_any_launch(gpu):
    import ctypes
    from otto_recommender_amd import _lib
    lib = _lib.load()
    sums = (ctypes.c_int64 * 6)()
    assert lib.ottohip_submission_recall(gpu.h, -1, None, None, None, None, sums, None) == -1
    assert lib.ottohip_submission_recall(gpu.h, 5, None, None, None, None, sums, None) == -1
    assert lib.ottohip_submission_recall(gpu.h, 0, None, None, None, None, None, None) == -1
    assert lib.ottohip_submission_recall(gpu.h, 0, None, None, None, None, sums, None) == 0 and list(sums) == [0] * 6


def test_ranked_rows_from_the_ranker_frames_and_submission_file_agree(gpu, tmp_path):
    """eval_ranked on the device tensors of Ranker.rank == the same rows as DataFrames == through submission_frame
    and eval_submission == the oracle"""
    import json
    import torch
    from otto_recommender_amd import rank as R
    from otto_recommender_amd import submission as SB
    rng = np.random.default_rng(12)
    table = [(f"c{i}", RF.DTYPES[i % 4]) for i in range(8)]
    counts = rng.integers(0, 90, 150)
    off = np.r_[0, np.cumsum(counts)].astype(np.int64)
    n = int(off[-1])
    cols = {nm: RF.random_column(rng, dt, n) for nm, dt in table}
    session = np.repeat(np.arange(3000, 3000 + len(counts), dtype=np.int32), counts)
    aid = np.concatenate([rng.choice(5000, size=c, replace=False) for c in counts]).astype(np.int32)
    dev = torch.device("cuda", gpu.device)
    feats = {nm: torch.from_numpy(v).to(dev) for nm, v in cols.items()}
    feats["aid_next"], feats["session"] = torch.from_numpy(aid).to(dev), torch.from_numpy(session).to(dev)
    ranker = R.Ranker({t: R.parse_booster(RF.random_forest_text(rng, 20, 15, cols), table) for t in O.TARGETS}, gpu,
                      columns=table)
    ranked = ranker.rank(feats, torch.from_numpy(off).to(dev), keep_top_k=20)
    ranker.free()
    # labels: candidates of the session (some ranked, some not), aids that are no candidate, and an unranked session
    rows = [(int(session[i]), int(aid[i]), int(rng.integers(0, 3))) for i in rng.choice(n, size=600, replace=False)]
    rows += [(int(s), 9999, int(rng.integers(0, 3))) for s in rng.choice(session, size=40)] + [(99, 1, 0)]
    labels = pd.DataFrame(rows, columns=["session", "aid", "type"])
    frames = {t: pd.DataFrame({c: v.cpu().numpy() for c, v in r.items()}) for t, r in ranked.items()}
    ref = O.recall_sums({t: (f["session"].to_numpy(), f["aid_next"].to_numpy()) for t, f in frames.items()}, labels)
    assert all(0 < ref[2 * t] < ref[2 * t + 1] for t in range(3))
    assert SB.recall_sums(ranked, labels, gpu) == ref
    assert SB.recall_sums(frames, labels, gpu) == ref
    want = O.recall_from_sums(ref)
    assert SB.eval_ranked(ranked, labels, gpu) == want
    sub = R.submission_frame(frames)
    assert SB.eval_submission(sub, labels) == want
    sub.to_csv(tmp_path / "submission-v1.csv", index=False)
    got = SB.eval_submission(str(tmp_path / "submission-v1.csv"), labels, dir_out=str(tmp_path / "eval"))
    assert got == want
    assert json.load(open(tmp_path / "eval" / "submission-v1.json")) == want
    csv = pd.read_csv(tmp_path / "eval" / "submission-v1.csv")
    assert csv["type"].tolist() == ["clicks", "carts", "orders", "total"]
    assert csv["recall@20"].tolist() == pytest.approx([want[k] for k in csv["type"]], rel=1e-12)
