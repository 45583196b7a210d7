"""The split scatter of the reduce (csrc/covis_kernels.h: k_split_scatter_lds, k_split_scatter) at the chunk edges.

One hub aid per partner pattern receives exactly L words in its clicks row from two-event sessions, for the L at
which a split task changes its number of 16384-word chunks or digits: the smallest split task (1025 words, 3 digits,
one partial chunk), one full chunk and a second chunk of one word, two full chunks and a third of one word, three
chunks and a short tail, and 215,041 words (512 digits, 14 chunks, the last one partial); and 4096 and 4097 words, the
longest one-chunk task that k_split_scatter counts and scatters in one sub-tile and the shortest chunk that the
chunk-staged kernel takes. Partner patterns: all
partners distinct (every digit populated), one partner (one digit's cursor takes the whole chunk, and the bucket goes
on to the hash leaf), runs of 3, 5, 7 and 11 equal partners, and both click rules in one row. Every case runs with
the chunk-staged kernel on and off (OTTOHIP_SPLIT_LDS), over 1 and 3 files, and is compared bit-exactly with the
per-file tables of the CPU oracle: rows, count, count_ge2 and the four per-rule statistics."""
import functools

import numpy as np
import pytest

import covis as oracle
import otto_recommender_amd.synth as synth

pytestmark = pytest.mark.gpu
NAMES = list(oracle.REFERENCE_RULES)
LENGTHS = [1025, 4096, 4097, 16383, 16384, 16385, 32768, 32769, 3 * 16384 + 5, 215041]
CLICK, CART = 0, 1
ONE, DISTINCT, RUNS, BOTH = range(4)  # hub aids (below every partner: a symmetric rule stores a hub's pairs in its row)
STRIDE = 1 << 18  # partner aids of hub h: 16 + h * STRIDE + (0 .. L - 1)
N_ITEMS = 16 + 4 * STRIDE


def _hub_sessions(L):
    """(hub, partner aid, partner type) of L two-event sessions per hub, as three arrays."""
    base = lambda h: 16 + h * STRIDE
    run_len = np.array([3, 5, 7, 11])[np.arange(L) % 4]  # more runs than needed
    runs = np.repeat(np.arange(L), run_len)[:L]
    n0 = (L // 2) | 1
    cols = [(ONE, np.full(L, base(ONE)), np.full(L, CLICK)),
            (DISTINCT, base(DISTINCT) + np.arange(L), np.full(L, CLICK)),
            (RUNS, base(RUNS) + runs, np.full(L, CLICK)),
            (BOTH, base(BOTH) + np.concatenate([np.arange(n0) // 3, np.arange(L - n0) // 2]),  # click_to_click runs of 3,
             np.concatenate([np.full(n0, CLICK), np.full(L - n0, CART)]))]                      # click_to_cart_or_buy of 2
    return (np.concatenate([np.full(L, h) for h, _, _ in cols]), np.concatenate([p for _, p, _ in cols]),
            np.concatenate([t for _, _, t in cols]))


def _events(L):
    h, p, t = _hub_sessions(L)
    order = np.random.default_rng(L).permutation(len(h))  # deals every hub's sessions over the files
    h, p, t = h[order], p[order], t[order]
    n = len(h)
    sess = np.repeat(np.arange(n), 2)
    aid = np.stack([h, p], 1).ravel()
    ts = np.tile([0, 10], n)
    ty = np.stack([np.full(n, CLICK), t], 1).ravel()
    return synth.events_from_columns(sess, aid, ts, ty)


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
    """Events of the four hubs at L words each and their oracle tables over nf files (computed once, read-only)."""
    ev = _events(L)
    fb = np.linspace(0, ev.n_sessions, nf + 1).astype(np.int64)
    per_file = oracle.count_co_events_files(ev.session_offsets, ev.aid, ev.ts, ev.type, fb)
    ref = {n: _merge([p[n] for p in per_file]) for n in NAMES}
    a, _, c = ref["click_to_click"][:3]
    for h in (ONE, DISTINCT, RUNS):  # the construction: every hub's clicks row holds exactly L words
        assert int(c[a == h].sum()) == L, (h, L)
    a2, _, c2 = ref["click_to_cart_or_buy"][:3]
    assert int(c[a == BOTH].sum()) + int(c2[a2 == BOTH].sum()) == L
    return ev, fb, ref


@pytest.mark.parametrize("nf", [1, 3])
@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("lds", ["1", "0"])
def test_chunk_edges(gpu, monkeypatch, lds, L, nf):
    from otto_recommender_amd import covis as gc
    monkeypatch.setenv("OTTOHIP_SPLIT_LDS", lds)
    ev, fb, ref = _case(L, nf)
    tab = gc.count_co_events_fused(gc.DeviceEvents.from_host(ev, fb), n_items=N_ITEMS)
    for n in NAMES:
        a, b, c, c2 = tab.to_numpy(n)
        ra, rb, rc, rc2, fr, fr2 = ref[n]
        np.testing.assert_array_equal(a, ra, err_msg=n)
        np.testing.assert_array_equal(b, rb, err_msg=n)
        np.testing.assert_array_equal(c.astype(np.int64), rc, err_msg=n)
        np.testing.assert_array_equal(c2.astype(np.int64), rc2, err_msg=n)
        st = tab.stats(n)
        assert (st["n_rows"], st["n_pairs"], st["file_rows"], st["file_rows_ge2"]) == (len(ra), int(rc.sum()), fr, fr2), n
    tab.free()


@pytest.mark.parametrize("lds_min,lds_t,pipe", [("1", "1024", "0"), ("16384", "512", "0"), ("4097", "1024", "1")])
def test_both_kernels_share_a_split(gpu, monkeypatch, lds_min, lds_t, pipe):
    """OTTOHIP_SPLIT_LDS_MIN moves the chunk length at which the staged kernel takes over: at 1 it scatters every
    chunk (the one-word tail chunks too), at 16384 only the full chunks, and k_split_scatter the tails.
    OTTOHIP_SPLIT_LDS_T selects its 512-thread form. With OTTOHIP_SPLIT_PIPE the split runs as two launches per
    kernel over chunk ranges (chunk0 > 0 in the second)."""
    from otto_recommender_amd import covis as gc
    monkeypatch.setenv("OTTOHIP_SPLIT_LDS", "1")
    monkeypatch.setenv("OTTOHIP_SPLIT_LDS_MIN", lds_min)
    monkeypatch.setenv("OTTOHIP_SPLIT_LDS_T", lds_t)
    monkeypatch.setenv("OTTOHIP_SPLIT_PIPE", pipe)
    monkeypatch.setenv("OTTOHIP_SPLIT_PIPE_MIN", "2")
    L = 3 * 16384 + 5
    ev, fb, ref = _case(L, 3)
    tab = gc.count_co_events_fused(gc.DeviceEvents.from_host(ev, fb), n_items=N_ITEMS)
    for n in NAMES:
        a, b, c, c2 = tab.to_numpy(n)
        ra, rb, rc, rc2 = ref[n][:4]
        np.testing.assert_array_equal(a, ra, err_msg=n)
        np.testing.assert_array_equal(b, rb, err_msg=n)
        np.testing.assert_array_equal(c.astype(np.int64), rc, err_msg=n)
        np.testing.assert_array_equal(c2.astype(np.int64), rc2, err_msg=n)
    tab.free()
