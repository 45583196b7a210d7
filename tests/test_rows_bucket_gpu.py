"""The bucketed rows phase (csrc/covis_kernels.h: k_rows_bucket_count / _keys / _layout / _rank) against the sort path.

Every case is counted twice in one process, with the default rows path and with OTTOHIP_ROWS=sort (read per call), and
both results are compared with the per-file tables of the CPU oracle and with each other: the five tables in
(aid, aid_next) order, all four per-rule statistics and the table digests. Every comparison is bit-exact (integer
work). The bucketed path applies to more than 1024 row entries with keys of at most 23 bits; the cases say on which
side of that they are. The case "unfused" and test_wide_offsets reach the two fallbacks behind the sort: the unfused
layout on one GPU and the 64-bit word offsets."""
import functools
import os

import numpy as np
import pytest

import covis as oracle
import otto_recommender_amd.synth as synth

pytestmark = pytest.mark.gpu
NAMES = list(oracle.REFERENCE_RULES)
CLICK, CART, BUY = 0, 1, 2
DAY = 24 * 60 * 60
N_MAX = 2 ** 21 - 1  # the largest catalogue with 21 aid bits: row keys of 23 bits, the largest hi of a bucket's table


def _merge(parts):
    """Per-file tables [(aid, aid_next, count)] -> merged (aid, aid_next, count, count_ge2, file_rows, file_rows_ge2)."""
    a = np.concatenate([p[0] for p in parts]).astype(np.int64)
    b = np.concatenate([p[1] for p in parts]).astype(np.int64)
    c = np.concatenate([p[2] for p in parts]).astype(np.int64)
    key, inv = np.unique((a << 32) | b, return_inverse=True)
    cnt = np.bincount(inv, weights=c, minlength=len(key)).astype(np.int64)
    ge2 = np.bincount(inv, weights=np.where(c >= 2, c, 0), minlength=len(key)).astype(np.int64)
    return (key >> 32).astype(np.int32), (key & 0xFFFFFFFF).astype(np.int32), cnt, ge2, len(a), int((c >= 2).sum())


def _random_sessions(rng, n_sessions, pool, first=0):
    """Sessions of 2 ... 6 events with aids from pool, all three types, times inside a few hours: rows (s, aid, ts, type)."""
    ln = rng.integers(2, 7, n_sessions)
    s = np.repeat(np.arange(first, first + n_sessions), ln)
    n = len(s)
    return np.stack([s, rng.choice(pool, n), rng.integers(0, 4 * 3600, n), rng.integers(0, 3, n)], axis=1)


def _edge_rows():
    """Aids with low byte 0 and 255, aids 0 and N_MAX - 1, in all three types (the type bits are the top of hi)."""
    rng = np.random.default_rng(1)
    special = np.array([0, 255, 256, 511, 65280, 65535, N_MAX - 1 - 255, N_MAX - 1 - 254, N_MAX - 1])
    assert (special[-3] & 255, special[-2] & 255) == (255, 0)
    pool = np.concatenate([special, special, rng.integers(0, N_MAX, 64)])
    rows = _random_sessions(rng, 3000, pool)
    # every special aid as click, cart and buy with pairs of its own: one session per (aid, type), partner of each type
    extra = []
    for i, a in enumerate(special):
        for t in (CLICK, CART, BUY):
            s = 3000 + 3 * i + t
            extra += [(s, a, 0, t), (s, special[(i + 1) % len(special)], 5, CLICK),
                      (s, special[(i + 2) % len(special)], 9, CART), (s, special[(i + 3) % len(special)], 12, BUY)]
    return np.concatenate([rows, np.array(extra)])


def _hub_rows():
    """One hub click per session in 2048 sessions, each with 256 cart / buy partners of one aid in two clusters a day
    before and a day after it (48 h apart: no pairs across): every hub entry counts 256 words, above the count byte's
    255, grouped or not. 1024 two-click sessions of other aids with the hub's low byte share its bucket, so the hub
    is half of the bucket's entries."""
    hub, partner, ns = 0x1234, 0x0777, 2048
    j = np.arange(128)
    ts = np.concatenate([[0], -DAY + 10 + j, DAY - 10 - j])
    ty = np.concatenate([[CLICK], CART + j % 2, CART + j % 2])
    aid = np.concatenate([[hub], np.full(256, partner)])
    s = np.repeat(np.arange(ns), 257)
    rows = np.stack([s, np.tile(aid, ns), np.tile(ts, ns), np.tile(ty, ns)], axis=1)
    nfill = ns // 2  # two click entries each: as many as the hub's
    k = np.arange(nfill)
    same = hub + 256 * (1 + k % 29)  # the hub's low byte, other hi
    fill = np.stack([np.repeat(ns + k, 2), np.stack([same, same + 256 * 31], 1).ravel(), np.tile([0, 7], nfill),
                     np.zeros(2 * nfill, np.int64)], axis=1)
    sess = np.concatenate([rows, fill])
    new_id = np.random.default_rng(2).permutation(ns + nfill)  # hub and filler sessions interleaved
    sess[:, 0] = new_id[sess[:, 0]]
    return sess[np.argsort(sess[:, 0], kind="stable")]


def _case_rows(name):
    rng = np.random.default_rng(7)
    if name == "edges":  # bucketed; 23-bit keys
        return _edge_rows(), N_MAX, 3
    if name == "small_catalogue":  # bucketed; fewer than 256 aids: the buckets of the low bytes >= 200 are empty
        return _random_sessions(rng, 2500, np.arange(200)), 200, 2
    if name == "one_bucket":  # bucketed; every aid has the low byte 7: one bucket holds every entry
        return _random_sessions(rng, 2500, 7 + 256 * np.arange(32)), 8192, 2
    if name == "hub":  # bucketed; saturated count bytes, one LDS address for most lanes
        return _hub_rows(), 65536, 2
    if name == "few_entries":  # below the floor of 1024 entries: the first pass, then the sort's remaining passes
        return _random_sessions(rng, 60, np.arange(5000)), 8192, 2
    if name == "no_pairs":  # En = 0: single-event sessions
        return np.stack([np.arange(50), np.arange(50), np.zeros(50, np.int64), np.arange(50) % 3], axis=1), 8192, 1
    if name == "one_entry":  # one kept entry: the click has a pair (click -> cart), the cart has none
        return np.array([(0, 3, 0, CLICK), (0, 4, 10, CART), (1, 5, 0, BUY)]), 8192, 1
    if name == "bits24":  # 22 aid bits, 24-bit keys: the sort path
        pool = np.concatenate([[0, 255, 2 ** 21 - 1, 2 ** 21], rng.integers(0, 2 ** 21 + 1, 64)])
        return _random_sessions(rng, 2500, pool), 2 ** 21 + 1, 2
    if name == "unfused":  # 3 * n_items >= 2^24: the rows no longer fit the fused layout's 24-bit row index, so one
        # GPU takes the unfused layout (k_gather_counts, two scans, k_rows); 1 rule + 23 aid + 1 file bits per word
        pool = np.concatenate([[0, 255, 256, 2 ** 23 - 1], rng.integers(0, 2 ** 23, 64)])
        return _random_sessions(rng, 2500, pool), 2 ** 23, 2
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _case(name):
    """Events, file bounds, n_items and the oracle's merged tables and digests (computed once, read-only)."""
    rows, n_items, nf = _case_rows(name)
    ev = synth.events_from_columns(rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3])
    fb = np.linspace(0, ev.n_sessions, nf + 1).astype(np.int64)
    per_file = oracle.count_co_events_files(ev.session_offsets, ev.aid, ev.ts, ev.type, fb)
    ref = {n: _merge([p[n] for p in per_file]) for n in NAMES}
    dig = oracle.files_digest(ev.session_offsets, ev.aid, ev.ts, ev.type, fb, threads=4)
    return ev, fb, n_items, ref, dig


def _count(ev, fb, n_items, env):
    """One GPU count under the environment switches env (None: unset); returns {rule: (tables, stats, digest)}."""
    from otto_recommender_amd import covis as gc
    old = {k: os.environ.get(k) for k in env}
    for k, v in env.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    try:
        tab = gc.count_co_events_fused(gc.DeviceEvents.from_host(ev, fb), n_items=n_items)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    out = {n: (tab.to_numpy(n), tab.stats(n), tab.digest(n)) for n in NAMES}
    tab.free()
    return out


def _check(name, env=None):
    ev, fb, n_items, ref, dig = _case(name)
    env = dict(env or {})
    got = {"default": _count(ev, fb, n_items, {**env, "OTTOHIP_ROWS": None}),
           "sort": _count(ev, fb, n_items, {**env, "OTTOHIP_ROWS": "sort"})}
    for side, res in got.items():
        for n in NAMES:
            (a, b, c, c2), st, d = res[n]
            ra, rb, rc, rc2, fr, fr2 = ref[n]
            np.testing.assert_array_equal(a, ra, err_msg=f"{side} {n}")
            np.testing.assert_array_equal(b, rb, err_msg=f"{side} {n}")
            np.testing.assert_array_equal(c.astype(np.int64), rc, err_msg=f"{side} {n}")
            np.testing.assert_array_equal(c2.astype(np.int64), rc2, err_msg=f"{side} {n}")
            assert (st["n_rows"], st["n_pairs"], st["file_rows"], st["file_rows_ge2"]) == \
                (len(ra), int(rc.sum()), fr, fr2), (side, n)
            for k in ("d_count", "d_count_ge2", "pairs", "pairs_ge2"):
                assert d[k] == dig[n][k], (side, n, k)
            assert d["rows"] == len(ra), (side, n)
    for n in NAMES:
        (ta, sa, da), (tb, sb, db) = got["default"][n], got["sort"][n]
        for x, y in zip(ta, tb):
            np.testing.assert_array_equal(x, y, err_msg=n)
        assert sa == sb and da == db, n
    return ref


@pytest.mark.parametrize("name", ["edges", "small_catalogue", "one_bucket", "few_entries", "no_pairs", "one_entry",
                                  "bits24", "unfused"])
def test_rows_match_sort_and_oracle(gpu, name):
    ref = _check(name)
    if name == "edges":  # the construction: rows of aid 0 and of the largest aid in all three types
        for n in ("click_to_click", "cart_to_cart", "buy_to_buy"):
            assert (ref[n][0] == 0).any() and (ref[n][0] == N_MAX - 1).any(), n
    if name == "no_pairs":
        assert all(len(ref[n][0]) == 0 for n in NAMES)
    if name == "one_entry":
        assert sum(int(ref[n][2].sum()) for n in NAMES) == 1


@pytest.mark.parametrize("group", ["1", "0"])
def test_hub_saturated_counts(gpu, group):
    """The hub's row holds 256 words per entry (more than the count byte's 255), so every hub entry's count is read
    through the link array (grouped entries) or the count array (OTTOHIP_GROUP=0)."""
    ref = _check("hub", {"OTTOHIP_GROUP": group})
    a, _, c = ref["click_to_cart_or_buy"][:3]
    assert int(c[a == 0x1234].sum()) == 256 * 2048 and int((a == 0x1234).sum()) == 1


@pytest.mark.parametrize("switch", ["OTTOHIP_ROWS_DIRECT", "OTTOHIP_ROWS_PART"])
def test_other_outlets(gpu, switch):
    """The outlets kept as A/B switches: the rank pass writes the offsets in event order itself (DIRECT), or they
    take the sort path's partition pass and scatter (PART)."""
    _check("edges", {switch: "1"})
    _check("hub", {switch: "1"})


def test_wide_offsets(gpu):
    """OTTOHIP_POFF32=0 (read per call): 64-bit word offsets from k_rows_tile, through k_link_fix (grouped entries)
    and into the emit, the path of a build with 2^32 words or more. The hub keeps the saturated count byte and the
    link array in play."""
    _check("edges", {"OTTOHIP_POFF32": "0"})
    for g in ("1", "0"):
        _check("hub", {"OTTOHIP_POFF32": "0", "OTTOHIP_GROUP": g})


def test_out_of_range_aid(gpu):
    """An aid outside [0, n_items) among enough entries for the bucketed path: the range error, as on the sort path."""
    from otto_recommender_amd import _lib as L
    rows = _random_sessions(np.random.default_rng(3), 2500, np.arange(1000))
    rows[1234, 1] = 2_000_000
    ev = synth.events_from_columns(rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3])
    fb = np.array([0, ev.n_sessions], np.int64)
    for env in ({"OTTOHIP_ROWS": None}, {"OTTOHIP_ROWS": "sort"}):
        with pytest.raises(L.OttoHipError) as e:
            _count(ev, fb, 1000, env)
        assert e.value.rc == -2  # OTTOHIP_ERANGE
