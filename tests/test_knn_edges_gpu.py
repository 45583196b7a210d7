"""W2V kNN (csrc/knn.hip) on the paths tests/test_knn.py leaves out: the threshold pre-pass against the
oracle (its first index size, ties at its bound), the index-list rerun after a candidate buffer overflow, the
k-step variants on both sides of the 8-column step, and the shape edges of V, n_q and k.

The check is tests/knn_edges.py::check: every neighbour the bf16 scores cannot lose (the certain-item rule
derived there) is returned, a query whose neighbours are all certain gets the oracle's rows exactly, and the
assertions of tests/test_knn.py::_check hold. Each input's cap on what the rule may skip is asserted on the
reference first (tests/knn_edges.py::CAPS; tests/test_knn_edges_cpu.py recomputes them without a GPU)."""
import numpy as np
import pytest

import knn as oracle
import knn_edges as K

pytestmark = pytest.mark.gpu


def _search(ctx, emb, rows=None, n_q=None, k=20, index=None):
    """(idx, d2, phase names of the call) as numpy / list."""
    from otto_recommender_amd.w2vec import KnnIndex
    ix = index or KnnIndex(emb, ctx)
    ctx.set_timing(True)
    try:
        i, d = ix.search(rows, n_q=n_q, k=k)
        phases = [n for n, _, _ in ctx.timings()]
    finally:
        ctx.set_timing(False)
    out = i.cpu().numpy(), d.cpu().numpy(), phases
    if index is None:
        ix.free()
    return out


def _run(ctx, name, min_exact=0.995, capped=True):
    emb, rows = K.case(name)
    ref = K.ref(name)
    gi, gd, phases = _search(ctx, emb, rows)
    same = K.check(ref, gi, gd, min_exact=min_exact, **(K.caps(name) if capped else {}))
    print(f"{name}: sets equal {same:.4f}, certain items {ref.item_share:.4f}, queries {ref.query_share:.4f}")
    return gi, gd, phases, ref


# ---- A: the rule on the data its envelope was measured on ----

@pytest.mark.parametrize("name", ["normal_d100", "normal_d16"])
def test_normal_data(gpu, name):
    _run(gpu, name)


# ---- B: the pre-pass ----

@pytest.mark.parametrize("V", [98_304, 98_305])
def test_prepass_first_index_size(gpu, V):
    """98 304 rows are 384 tiles: (384 - 1) / 16 = 23 sampled tiles, no pre-pass. 98 305 rows are 385: the
    pre-pass runs over exactly 24 tiles and the last tile holds one item. 300 query rows spread over the
    index, the first and the last row included."""
    gi, gd, phases, ref = _run(gpu, f"pre{V}")
    assert ("knn_pre" in phases) == (V == 98_305), phases
    assert ref.rows[0] == 0 and ref.rows[-1] == V - 1
    assert np.all(gi[:, 0] == ref.rows) and np.all(gd[:, 0] == 0)


@pytest.mark.parametrize("buf", ["0", "1"])
@pytest.mark.parametrize("V", [98_304, 99_000])
def test_ties_at_the_prepass_bound(gpu, monkeypatch, V, buf):
    """Three groups of 24 identical rows, each row in a 32-item block of its own in the sampled tiles 0, 16,
    .. 368 and at 24 different in-block positions. A member's query scores S = |q|^2/2 on all 24, so at
    V = 99 000 the pre-pass bound is S itself, and the main pass must still insert all 24: their keys lie up to
    31 ulp below S. The top-20 of each member are the 20 lowest rows of its group at distance 0. V = 98 304
    (no pre-pass) is the control.
    With the bound one ulp below S, V = 99 000 lost the members whose row slot was below S's 5 low mantissa
    bits: the three groups kept 7, 22 and 10 of their 24 members (the same for every query of a group and for
    both OTTOHIP_KNN_BUF settings), and the first and third returned 13 and 10 slots of -1 / inf."""
    monkeypatch.setenv("OTTOHIP_KNN_BUF", buf)
    emb, groups = K.with_ties(V)
    rows = np.concatenate(groups)
    want = np.concatenate([np.tile(g[:20], (24, 1)) for g in groups])
    ri, rd = oracle.topk_exact(emb, rows, 20)
    assert np.array_equal(ri, want) and np.all(rd == 0)
    gi, gd, phases = _search(gpu, emb, rows)
    assert ("knn_pre" in phases) == (V == 99_000), phases
    lost = [(int(r), sorted(set(w) - set(g))) for r, g, w in zip(rows, gi, want) if set(w) - set(g)]
    assert not lost, lost[:6]
    np.testing.assert_array_equal(gi, want)
    assert np.all(gd == 0)


def test_more_ties_than_candidates(gpu):
    """100 identical rows over the sampled tiles: more equal scores than the KN_C = 24 candidates. Which 20
    come back is not specified (KnnIndex.search); all are members at distance 0."""
    emb, rows = K.big_group()
    gi, gd, phases = _search(gpu, emb, rows)
    assert "knn_pre" in phases
    assert np.all(gd == 0) and np.all(np.isin(gi, rows))
    assert all(len(set(g)) == 20 for g in gi)


# ---- C: candidate buffer overflow -> index lists ----

def test_list_fallback(gpu, monkeypatch):
    """Shrinking shells: every query's list takes an insert for nearly every later row, the last row's one
    for each of the 3 000, far above KN_BCAP = 512, so the call reruns with index lists."""
    monkeypatch.delenv("OTTOHIP_KNN_BUF", raising=False)
    emb, rows = K.case("shells")
    gi, gd, phases, _ = _run(gpu, "shells")
    assert "knn_main_lists" in phases, phases
    monkeypatch.setenv("OTTOHIP_KNN_BUF", "0")
    li, ld, lphases = _search(gpu, emb, rows)
    assert "knn_main_lists" not in lphases and "knn_select" not in lphases
    np.testing.assert_array_equal(gi, li)
    np.testing.assert_array_equal(gd.view(np.uint32), ld.view(np.uint32))
    # no stale overflow flag: an ordinary search on the same context stays on the buffers
    monkeypatch.delenv("OTTOHIP_KNN_BUF")
    emb2, _ = K.case("nq")
    ni, nd, nphases = _search(gpu, emb2, None, n_q=257)
    assert "knn_select" in nphases and "knn_main_lists" not in nphases, nphases
    K.check(K.ref("nq"), ni, nd, **K.caps("nq"))


# ---- D: k-step variants and shape edges ----

@pytest.mark.parametrize("dim", K.DIMS)
def test_dims_around_the_8_column_step(gpu, monkeypatch, dim):
    """dim + 2 <= 104 takes the 8-column last k-step (HALF): dim 102 puts the two norm columns in its last two
    columns, dim 103 is the first dim on seven 16-column steps; OTTOHIP_KNN_HALF=0 runs those on every dim.
    dim 1 and 2 (norm columns in the first chunk) use rows that are exact in bf16."""
    monkeypatch.delenv("OTTOHIP_KNN_HALF", raising=False)
    gi, gd, _, ref = _run(gpu, f"dim{dim}")
    monkeypatch.setenv("OTTOHIP_KNN_HALF", "0")
    hi, hd, _, _ = _run(gpu, f"dim{dim}")
    # the exact rows of dim 1 and 2 score exactly on either path; elsewhere the fully certain queries must agree
    full = np.ones(len(ref.rows), bool) if dim <= 2 else ref.certain.all(1)
    assert full.sum() >= 100
    np.testing.assert_array_equal(gi[full], hi[full])
    np.testing.assert_array_equal(gd[full], hd[full])
    assert np.all(gi[:, 0] == ref.rows) and np.all(gd[:, 0] == 0)


def test_dim_127_is_rejected(gpu):
    from otto_recommender_amd import _lib as L
    from otto_recommender_amd.w2vec import KnnIndex
    KnnIndex(K._normal(40, 126, 1), gpu).free()
    with pytest.raises(L.OttoHipError):
        KnnIndex(K._normal(40, 127, 1), gpu)


@pytest.mark.parametrize("V", K.SIZES)
def test_index_sizes_around_block_and_tile(gpu, V):
    """All rows as queries; 256 and 512 fill their last tile. Slots past V are -1 / inf."""
    gi, gd, _, _ = _run(gpu, f"size{V}", min_exact=1.0)
    n = min(V, 20)
    assert np.all(gi[:, :n] >= 0) and np.all(gi[:, :n] < V) and np.all(np.isfinite(gd[:, :n]))
    assert np.all(gi[:, n:] == -1) and np.all(np.isinf(gd[:, n:]))


@pytest.mark.parametrize("n_q", [1, 63, 64, 65, 255, 256, 257])
def test_query_counts_around_wave_and_workgroup(gpu, n_q):
    """Rows 0 .. n_q - 1 given as a count and as explicit rows in descending order: the same result row for
    row, and the oracle's."""
    from otto_recommender_amd.w2vec import KnnIndex
    emb, _ = K.case("nq")
    ix = KnnIndex(emb, gpu)
    ci, cd, _ = _search(gpu, emb, None, n_q=n_q, index=ix)
    ri, rd, _ = _search(gpu, emb, np.arange(n_q)[::-1].copy(), index=ix)
    ix.free()
    assert ci.shape == (n_q, 20)
    np.testing.assert_array_equal(ci, ri[::-1])
    np.testing.assert_array_equal(cd.view(np.uint32), rd[::-1].view(np.uint32))
    ref = K.ref("nq")
    if n_q == 257:
        K.check(ref, ci, cd, **K.caps("nq"))
    else:  # a prefix of the reference's queries: the rule without the shares
        sub = K.Ref(ref.rows[:n_q], 20, ref.idx[:n_q], ref.d2[:n_q], ref.certain[:n_q], ref.rr, 0.0, 0.0)
        K.check(sub, ci, cd, min_exact=0.0)


def test_k_prefixes_and_argument_errors(gpu):
    from otto_recommender_amd import _lib as L
    from otto_recommender_amd.w2vec import KnnIndex
    emb, rows = K.case("nq")
    ix = KnnIndex(emb, gpu)
    i20, d20, _ = _search(gpu, emb, rows, index=ix)
    for k in (1, 19):
        ik, dk, _ = _search(gpu, emb, rows, k=k, index=ix)
        assert ik.shape == (257, k)
        np.testing.assert_array_equal(ik, i20[:, :k])
        np.testing.assert_array_equal(dk.view(np.uint32), d20[:, :k].view(np.uint32))
    for k in (0, 21):
        with pytest.raises(L.OttoHipError):
            ix.search(rows, k=k)
    for i, d in (ix.search(None, n_q=0, k=20), ix.search(np.zeros(0, np.int32), k=20)):
        assert tuple(i.shape) == (0, 20) and tuple(d.shape) == (0, 20)
    ix.free()


@pytest.mark.parametrize("n_q", [65, 257])
def test_output_guard_rows(gpu, n_q):
    """The outputs sit between two guard rows: nothing is written before row 0 or past row n_q - 1 (65 and 257
    leave the last wave / workgroup with one query)."""
    import torch
    from otto_recommender_amd import _lib as L
    from otto_recommender_amd.w2vec import KnnIndex
    emb, _ = K.case("nq")
    ix = KnnIndex(emb, gpu)
    dev = ix.emb.device
    for k in (20, 1):
        bi = torch.full((n_q + 2, k), -77, dtype=torch.int32, device=dev)
        bd = torch.full((n_q + 2, k), -5.0, dtype=torch.float32, device=dev)
        L.check(L.load().ottohip_knn_topk(gpu.h, ix.h, None, n_q, k, L.ptr(bi[1:]), L.ptr(bd[1:]),
                                          L.stream_handle(None)))
        torch.cuda.synchronize()
        gi, gd = bi.cpu().numpy(), bd.cpu().numpy()
        assert np.all(gi[[0, -1]] == -77) and np.all(gd[[0, -1]] == -5.0)
        ref = K.ref("nq")
        assert np.all(gi[1:-1, 0] == np.arange(n_q)) and np.all(gd[1:-1] >= 0)
        np.testing.assert_array_equal(gi[1:-1][ref.certain[:n_q].all(1)][:, :k], ref.idx[:n_q][ref.certain[:n_q].all(1)][:, :k])
    ix.free()


# ---- E: outside the envelope ----

@pytest.mark.parametrize("name", K.ENVELOPE)
def test_outside_the_envelope_only_certain_neighbours_are_promised(gpu, name):
    """A common offset (2, 4, 8 on every component) or tight clusters (sigma 0.3, 0.1 of the centres' scale)
    grow |q||v| against the distance gaps: the bf16 top-24 no longer holds the exact top-20 (DESIGN.md quotes
    the shares), and what remains promised is the certain-item rule alone, without a cap."""
    _run(gpu, name, min_exact=0.0, capped=False)
