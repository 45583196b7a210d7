"""Inputs shared by tests/test_feats_cpu.py and tests/test_feats_gpu.py (test infrastructure): the known answer of
tests/golden/kat_feats.json as frames, and a random fixture built as tests/test_candidates_gpu.py::_fixture does,
with full R1 frames, non-zero kNN distances, six-rank cl50 and cl1 frames, labels and embeddings."""
import json
import os

import numpy as np
import pandas as pd

import covis as oracle
import retrieve as oracle_retrieve
import feats_oracle as F

RULES = oracle_retrieve.RULES
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kat_feats.json")


def r1_frame(n, d):
    """columns of the R1 output (model/retrieve.py:53-61) for rule n from a dict of arrays"""
    return pd.DataFrame({"aid": np.asarray(d["aid"], np.int32), "aid_next": np.asarray(d["aid_next"], np.int32),
                         f"{n}_count": np.asarray(d["count"], np.int32),
                         f"{n}_count_pop": np.asarray(d["count_pop"], np.int16),
                         f"{n}_perc_pop": np.asarray(d["perc_pop"], np.int16),
                         f"{n}_rank": np.asarray(d["rank"], np.int16),
                         f"{n}_count_rel": np.asarray(d["count_rel"], np.int8)})


def knn_frame(name, d):
    return pd.DataFrame({"aid": np.asarray(d["aid"], np.int32), "aid_next": np.asarray(d["aid_next"], np.int32),
                         f"dist_w2vec_{name}": np.asarray(d["dist"], np.int32),
                         f"rank_w2vec_{name}": np.asarray(d["rank"], np.int8)})


def empty_r1(n):
    z = np.zeros(0)
    return r1_frame(n, {k: z for k in ("aid", "aid_next", "count", "count_pop", "perc_pop", "rank", "count_rel")})


def kat():
    """(args of retrieve_and_gen_feats without file_out, expected {column: list})"""
    k = json.load(open(GOLDEN))
    ev = pd.DataFrame(k["events"]).astype({"session": np.int32, "aid": np.int32, "ts": np.int32, "type": np.int8})
    r1 = {n: (r1_frame(n, k["r1"][n]) if n in k["r1"] else empty_r1(n)) for n in RULES}
    args = (ev, r1, knn_frame("all", k["knn_all"]), knn_frame("1_2", k["knn_1_2"]), pd.DataFrame(k["session_cl"]),
            pd.DataFrame(k["pop_cl1"]), pd.DataFrame(k["pop_cl50"]), pd.DataFrame(k["aid_embeddings"]),
            pd.DataFrame(k["session_embeddings"]), pd.DataFrame(k["labels"]))
    return args, k["expected"]


def labels_for(df, seed=3):
    rng = np.random.default_rng(seed)
    rows = []
    for s, g in df.groupby("session"):
        a = g["aid"].to_numpy()
        rows.append((s, int(rng.choice(a)), 0))
        for t, k in ((1, rng.integers(0, 3)), (2, rng.integers(0, 2))):
            for x in rng.choice(a, size=k):
                rows.append((s, int(x), t))
        if rng.random() < 0.3:
            rows.append((s, int(rng.integers(0, 1855603)), 1))
    return pd.DataFrame(rows, columns=["session", "aid", "type"]).drop_duplicates()


def full_inputs(df, r1, rng, dim=8, n_pop=(5, 40)):
    """kNN frames, clusters, popularity frames, embeddings and labels around events df and R1 frames r1"""
    uni = np.unique(df["aid"].to_numpy())
    knn = []
    for name in ("all", "1_2"):
        q = uni[rng.random(len(uni)) < 0.8]
        nb = rng.choice(uni, size=(len(q), 19))
        k = pd.DataFrame({"aid": np.repeat(q, 20).astype(np.int32),
                          "aid_next": np.concatenate([q[:, None], nb], 1).ravel().astype(np.int32),
                          f"dist_w2vec_{name}": rng.integers(1, 2_000_000, len(q) * 20).astype(np.int32),
                          f"rank_w2vec_{name}": np.tile(np.arange(1, 21, dtype=np.int8), len(q))})
        knn.append(k.drop_duplicates(["aid", "aid_next"]).reset_index(drop=True))
    sess = np.unique(df["session"].to_numpy())
    cl = pd.DataFrame({"session": sess, "cl50": rng.integers(-1, 6, len(sess))})
    cl = cl[rng.random(len(cl)) < 0.9].reset_index(drop=True)
    pop = []
    for c in range(-1, 6):
        aids = rng.choice(uni, size=rng.integers(*n_pop), replace=False)
        pop.append(pd.DataFrame({"aid": aids.astype(np.int32), "cl50": c,
                                 **{r: rng.integers(1, 60, len(aids)).astype(np.int16) for r in F.CL50_RANKS}}))
    pop = pd.concat(pop).reset_index(drop=True)
    a1 = uni[rng.random(len(uni)) < 0.5]
    cl1 = pd.DataFrame({"aid": a1.astype(np.int32),
                        **{r: rng.integers(1, 1000, len(a1)).astype(np.int16) for r in F.CL1_RANKS}})
    ea = uni[rng.random(len(uni)) < 0.8]
    aemb = pd.DataFrame({"aid": ea.astype(np.int32),
                         **{f"dim_{i}_aid": rng.normal(size=len(ea)).astype(np.float32) for i in range(dim)}})
    es = sess[rng.random(len(sess)) < 0.8]
    semb = pd.DataFrame({"session": es.astype(np.int32),
                         **{f"dim_{i}_ses": rng.normal(size=len(es)).astype(np.float32) for i in range(dim)}})
    return knn[0], knn[1], cl, cl1, pop, aemb, semb, labels_for(df)


def random_fixture(n_sessions=600, seed=7, first=4242):
    """args of retrieve_and_gen_feats (without file_out) over synth.generate sessions"""
    import otto_recommender_amd.synth as synth
    ev = synth.generate(n_sessions, first_session=first, seed=seed)
    df = ev.to_pandas()
    per = oracle.count_co_events_file(ev.session_offsets, ev.aid, ev.ts, ev.type)
    r1 = {}
    for n in RULES:
        a, b, c = per[n]
        o = np.lexsort((b, a, -c.astype(np.int64)))
        first_n = 10 if n.startswith("click_to") else 20
        t = oracle_retrieve.get_df_count_for_co_event_type(a[o], b[o], c[o].astype(np.int32), first_n)
        r1[n] = r1_frame(n, t)
    rng = np.random.default_rng(seed)
    return (df, r1) + full_inputs(df, r1, rng)


def candidate_args(args):
    """the arguments of oracle/retrieve.py::candidates for the same inputs"""
    df, r1, ka, k12, cl, cl1, pop = args[:7]
    pf = pop[pop[F.CL50_RANKS].min(axis=1) <= 20]
    return (df, r1, ka.rename(columns={"rank_w2vec_all": "rank"}), k12.rename(columns={"rank_w2vec_1_2": "rank"}),
            cl, pf[["cl50", "aid"]])


def compare(got, ref, cols=None):
    """every column exactly as int64; cos / eucl at the project's rtol 1e-5 (cos with the atol 1e-6 of
    tests/test_popularity_gpu.py's R7 check: a cosine near 0 has no relative precision in fp32)"""
    assert len(got) == len(ref), (len(got), len(ref))
    for c in (cols or list(ref.columns)):
        g, r = got[c].to_numpy(), ref[c].to_numpy()
        if c in ("cos_sim_ses_aid", "eucl_dist_ses_aid"):
            np.testing.assert_allclose(g.astype(np.float64), r.astype(np.float64), rtol=1e-5,
                                       atol=1e-6 if c.startswith("cos") else 0.0, err_msg=c)
        else:
            np.testing.assert_array_equal(g.astype(np.int64), r.astype(np.int64), err_msg=c)
