"""The fold of the register-sort reduce leaves (csrc/covis_kernels.h: fold_pass, k_agg_sort) at the class edges.

One hub aid per variant receives exactly L words in its clicks row from two-event sessions, for the L at which a
row changes its task class (64 * M words, M = 1 ... 16). The rows, the counts and all four per-rule statistics
are compared with the per-file tables of the CPU oracle: count = sum of the per-file counts, count_ge2 = sum of
the per-file counts >= 2, file_rows = rows per file summed, file_rows_ge2 = rows per file with count >= 2 summed.
Every comparison is bit-exact (integer work)."""
import functools

import numpy as np
import pytest

import covis as oracle
import otto_recommender_amd.synth as synth

pytestmark = pytest.mark.gpu
NAMES = list(oracle.REFERENCE_RULES)
N_ITEMS = 8192
EDGES = [1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024]
CLICK, CART = 0, 1
# hub aids (below every partner, so a symmetric rule stores all of a hub's pairs in the hub's row)
ONE, DISTINCT, RUNS, BOTH, DIAG = range(5)


def _partners(hub, n):
    return 16 + hub * 1024 + np.arange(n)


def _hub_sessions(L):
    """{hub: [(partner aid, partner type)]}: L two-event sessions (hub click at ts 0, partner at ts 10) per hub,
    except DIAG, whose sessions (hub, hub) give two words each (both orders of the equal aids)."""
    out = {ONE: [(16 + ONE * 1024, CLICK)] * L,  # a single k-run of count L
           DISTINCT: [(int(p), CLICK) for p in _partners(DISTINCT, L)]}  # L k-runs of count 1
    runs, p = [], 0
    while len(runs) < L:  # k-runs of 3, 5, 7, 11 words: they straddle the 1 ... 16 registers of a lane
        runs += [(16 + RUNS * 1024 + p, CLICK)] * (3, 5, 7, 11)[p % 4]
        p += 1
    out[RUNS] = runs[:L]
    n0 = min(L, (L // 2) | 1)  # odd: the q = 0 / q = 1 boundary is inside a lane for every M >= 2
    out[BOTH] = ([(int(x), CLICK) for x in _partners(BOTH, 1)[0] + np.arange(n0) // 3] +  # click_to_click, runs of 3
                 [(int(x), CART) for x in _partners(BOTH, 1)[0] + np.arange(L - n0) // 2])  # click_to_cart_or_buy, of 2
    nd = min(3, L // 2)  # diagonal sessions: 2 * nd words of the row (DIAG, DIAG), the rest off the diagonal
    out[DIAG] = [(DIAG, CLICK)] * nd + [(int(x), CLICK) for x in _partners(DIAG, 1)[0] + np.arange(L - 2 * nd) // 2]
    return out


def _events(hubs, seed):
    sessions = [(h, p, t) for h, ps in hubs.items() for p, t in ps]
    order = np.random.default_rng(seed).permutation(len(sessions))  # deals every hub's sessions over the files
    rows = []
    for s, i in enumerate(order):
        h, p, t = sessions[i]
        rows += [(s, h, 0, CLICK), (s, p, 10, t)]
    a = np.array(rows)
    return synth.events_from_columns(a[:, 0], a[:, 1], a[:, 2], a[:, 3])


def _bounds(ev, nf):
    return np.linspace(0, ev.n_sessions, nf + 1).astype(np.int64)


def _merge(parts):
    """Per-file tables [(aid, aid_next, count)] -> merged (aid, aid_next, count, count_ge2, file_rows, file_rows_ge2)."""
    a = np.concatenate([p[0] for p in parts]).astype(np.int64)
    b = np.concatenate([p[1] for p in parts]).astype(np.int64)
    c = np.concatenate([p[2] for p in parts]).astype(np.int64)
    key, inv = np.unique((a << 32) | b, return_inverse=True)
    cnt = np.bincount(inv, weights=c, minlength=len(key)).astype(np.int64)
    ge2 = np.bincount(inv, weights=np.where(c >= 2, c, 0), minlength=len(key)).astype(np.int64)
    return (key >> 32).astype(np.int32), (key & 0xFFFFFFFF).astype(np.int32), cnt, ge2, len(a), int((c >= 2).sum())


@functools.lru_cache(maxsize=None)
def _case(L, nf):
    """Events of the five hubs at L words each and their oracle tables over nf files (computed once, read-only)."""
    ev = _events(_hub_sessions(L), seed=L)
    fb = _bounds(ev, nf)
    per_file = oracle.count_co_events_files(ev.session_offsets, ev.aid, ev.ts, ev.type, fb)
    ref = {n: _merge([p[n] for p in per_file]) for n in NAMES}
    a, _, c = ref["click_to_click"][:3]
    for h in (ONE, DISTINCT, RUNS, DIAG):  # the construction: every hub's clicks row holds exactly L words
        assert int(c[a == h].sum()) == L, (h, L)
    assert int(c[a == BOTH].sum()) + int(ref["click_to_cart_or_buy"][2][ref["click_to_cart_or_buy"][0] == BOTH].sum()) == L
    return ev, fb, per_file, ref


def _assert_tables(tab, ref, names=NAMES):
    for n in names:
        a, b, c, c2 = tab.to_numpy(n)
        ra, rb, rc, rc2, fr, fr2 = ref[n]
        np.testing.assert_array_equal(a, ra, err_msg=n)  # a stale row in an unmarked slot would show up here
        np.testing.assert_array_equal(b, rb, err_msg=n)
        np.testing.assert_array_equal(c.astype(np.int64), rc, err_msg=n)
        np.testing.assert_array_equal(c2.astype(np.int64), rc2, err_msg=n)
        st = tab.stats(n)
        assert (st["n_rows"], st["n_pairs"], st["file_rows"], st["file_rows_ge2"]) == (len(ra), int(rc.sum()), fr, fr2), n


@pytest.mark.parametrize("nf", [1, 2, 3])
@pytest.mark.parametrize("L", EDGES)
def test_class_edges(gpu, L, nf):
    from otto_recommender_amd import covis as gc
    ev, fb, _, ref = _case(L, nf)
    tab = gc.count_co_events_fused(gc.DeviceEvents.from_host(ev, fb), n_items=N_ITEMS)
    _assert_tables(tab, ref)
    tab.free()


@pytest.mark.parametrize("L", EDGES)
def test_class_edges_dedup_off(gpu, L):
    """dedup=False (no event has an exact twin, so the oracle's tables are the same): the diagonal row of the
    symmetric click_to_click (DIAG, DIAG) counts once next to off-diagonal rows that count twice."""
    from otto_recommender_amd import covis as gc
    ev, fb, _, ref = _case(L, 2)
    if L >= 2:
        a, b = ref["click_to_click"][:2]
        assert ((a == DIAG) & (b == DIAG)).any()
    tab = gc.count_co_events_fused(gc.DeviceEvents.from_host(ev, fb), n_items=N_ITEMS, dedup=False)
    _assert_tables(tab, ref)
    tab.free()


@pytest.mark.parametrize("L", EDGES)
def test_class_edges_per_file_rows(gpu, L):
    """per_file_rule: the leaves that also histogram the rule's per-file rows."""
    from otto_recommender_amd import covis as gc
    ev, fb, per_file, ref = _case(L, 3)
    n = "click_to_click"
    tab = gc.count_co_events_fused(gc.DeviceEvents.from_host(ev, fb), n_items=N_ITEMS, per_file_rule=n)
    _assert_tables(tab, ref)
    np.testing.assert_array_equal(tab.file_rows_per_file, [len(p[n][0]) for p in per_file])
    np.testing.assert_array_equal(tab.file_rows_ge2_per_file, [int((p[n][2] >= 2).sum()) for p in per_file])
    tab.free()


@pytest.mark.parametrize("L", [70, 129, 520])
def test_hole_tails(gpu, L):
    """Rows of L words that fold to L - t rows, t = 1, 2, 3, 4, 5, 63 unused slots after the last row: every slot
    of the unused tail is marked as a hole, at whatever alignment the row's slots start."""
    from otto_recommender_amd import covis as gc
    hubs = {}
    for h, t in enumerate((1, 2, 3, 4, 5, 63)):
        p = _partners(h, L - t)
        hubs[h] = [(int(x), CLICK) for x in p] + [(int(p[0]), CLICK)] * t
    ev = _events(hubs, seed=L)
    fb = _bounds(ev, 1)
    per_file = oracle.count_co_events_files(ev.session_offsets, ev.aid, ev.ts, ev.type, fb)
    ref = {n: _merge([p[n] for p in per_file]) for n in NAMES}
    a, _, c = ref["click_to_click"][:3]
    for h, t in enumerate((1, 2, 3, 4, 5, 63)):
        assert int(c[a == h].sum()) == L and int((a == h).sum()) == L - t
    tab = gc.count_co_events_fused(gc.DeviceEvents.from_host(ev, fb), n_items=N_ITEMS)
    _assert_tables(tab, ref)
    tab.free()
