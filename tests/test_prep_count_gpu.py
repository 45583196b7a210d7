"""The fused prep + count kernel (csrc/covis_kernels.h: k_prep_count2, the default) against its first body
(OTTOHIP_PREP=v1, k_prep_count) and the CPU oracle.

Every case is counted four times in one process: with the default kernel and with OTTOHIP_PREP=v1, each with
OTTOHIP_GROUP 1 and 0 (all read per call). Every result is compared with the per-file tables of the CPU oracle and
with the first one: the five tables in (aid, aid_next) order, all four per-rule statistics and the table digests.
Every comparison is bit-exact (integer work). The cases sit on the boundaries of the segment rule for the window
bounds (gaps of W - 1, W, W + 1; spans of w and w + 1), on the chunk (64 lanes) and batch (64 sessions, 512 events)
geometry, on equal timestamps and duplicates, and on windows other than the reference's. Before anything runs on the
GPU, the oracle's tables are asked for the pairs each construction was built for."""
import functools
import os

import numpy as np
import pytest

import covis as oracle
import otto_recommender_amd.synth as synth
from test_rows_bucket_gpu import _hub_rows

pytestmark = pytest.mark.gpu
CLICK, CART, BUY = 0, 1, 2
H = 3600
DAY = 24 * H
C2C, C2CB, K2K, K2B, B2B = "click_to_click", "click_to_cart_or_buy", "cart_to_cart", "cart_to_buy", "buy_to_buy"
SIDES = [("v2 group", {"OTTOHIP_PREP": None, "OTTOHIP_GROUP": None}), ("v1 group", {"OTTOHIP_PREP": "v1", "OTTOHIP_GROUP": None}),
         ("v2 single", {"OTTOHIP_PREP": None, "OTTOHIP_GROUP": "0"}), ("v1 single", {"OTTOHIP_PREP": "v1", "OTTOHIP_GROUP": "0"})]


# ------------------------------------------------------------------ references
def _rules(min_dt=-DAY, max_dt=DAY, wmax=None):
    """The oracle's rules and window clamp for the config constants (wmax: {name: max |dt|} overrides)."""
    r = {n: (t, nx, (wmax or {}).get(n, w)) for n, (t, nx, w) in oracle.REFERENCE_RULES.items()}
    return r, min_dt, max_dt


def _brute_file(off, aid, ts, ty, rules, min_dt, max_dt, dedup):
    """One file by the definition: per session the (deduplicated) events, every ordered pair (i, j) of events that
    are not the same (ts, aid, type), min_dt <= dt <= max_dt, |dt| <= the rule's maximum, types by the rule."""
    acc = {n: {} for n in rules}
    for s in range(len(off) - 1):
        e = np.stack([ts[off[s]:off[s + 1]], aid[off[s]:off[s + 1]], ty[off[s]:off[s + 1]]], 1).astype(np.int64)
        if dedup:
            e = np.unique(e, axis=0)
        t, a, y = e[:, 0], e[:, 1], e[:, 2]
        dt = t[None, :] - t[:, None]
        same = (dt == 0) & (a[None, :] == a[:, None]) & (y[None, :] == y[:, None])
        base = ~same & (dt >= min_dt) & (dt <= max_dt)
        for n, (this, nxt, w) in rules.items():
            ok = base & (np.abs(dt) <= w) & (y[:, None] == this) & np.isin(y, nxt)[None, :]
            for i, j in zip(*np.nonzero(ok)):
                k = (int(a[i]), int(a[j]))
                acc[n][k] = acc[n].get(k, 0) + 1
    out = {}
    for n, d in acc.items():
        ks = sorted(d)
        out[n] = (np.array([k[0] for k in ks], np.int32), np.array([k[1] for k in ks], np.int32),
                  np.array([d[k] for k in ks], np.uint32))
    return out


def _merge(parts):
    """Per-file tables [(aid, aid_next, count)] -> merged (aid, aid_next, count, count_ge2, file_rows, file_rows_ge2)."""
    a = np.concatenate([p[0] for p in parts]).astype(np.int64)
    b = np.concatenate([p[1] for p in parts]).astype(np.int64)
    c = np.concatenate([p[2] for p in parts]).astype(np.int64)
    key, inv = np.unique((a << 32) | b, return_inverse=True)
    cnt = np.bincount(inv, weights=c, minlength=len(key)).astype(np.int64)
    ge2 = np.bincount(inv, weights=np.where(c >= 2, c, 0), minlength=len(key)).astype(np.int64)
    return (key >> 32).astype(np.int32), (key & 0xFFFFFFFF).astype(np.int32), cnt, ge2, len(a), int((c >= 2).sum())


def _reference(ev, fb, rules, min_dt, max_dt, dedup=True, brute=False):
    """Merged tables per rule from the oracle's per-file tables (brute: from the definition above, the only
    reference without deduplication: the oracle always deduplicates)."""
    off = np.asarray(ev.session_offsets, np.int64)
    per_file = []
    for f in range(len(fb) - 1):
        s0, s1 = int(fb[f]), int(fb[f + 1])
        e0, e1 = int(off[s0]), int(off[s1])
        if brute:
            per_file.append(_brute_file(off[s0:s1 + 1] - e0, ev.aid[e0:e1], ev.ts[e0:e1], ev.type[e0:e1], rules,
                                        min_dt, max_dt, dedup))
        else:
            per_file.append(oracle.count_co_events_file(off[s0:s1 + 1], ev.aid[e0:e1], ev.ts[e0:e1], ev.type[e0:e1],
                                                        rules, min_dt, max_dt))
    return {n: _merge([p[n] for p in per_file]) for n in rules}


def _n(ref, name, a, b):
    """The merged count of row (a, b) of a rule, 0 when it is absent."""
    ra, rb, rc = ref[name][:3]
    hit = (ra == a) & (rb == b)
    return int(rc[hit].sum())


# ------------------------------------------------------------------ cases
def _events(sessions, first=0):
    """[[(aid, ts, type), ...], ...] -> rows (session, aid, ts, type), events in the given order."""
    rows = [(first + s, a, t, y) for s, evs in enumerate(sessions) for a, t, y in evs]
    return np.array(rows, np.int64)


def _filler(rng, n, base_aid, first):
    """n sessions of 2 ... 6 events of all types inside a few hours."""
    ln = rng.integers(2, 7, n)
    s = np.repeat(np.arange(first, first + n), ln)
    m = len(s)
    return np.stack([s, base_aid + rng.integers(0, 50, m), rng.integers(0, 4 * H, m), rng.integers(0, 3, m)], axis=1)


GAP_TYPES = {"clicks": [CLICK] * 4, "carts": [CART] * 4, "orders": [BUY] * 4, "mixed": [CLICK, CART, BUY, BUY]}


def _gap_sessions():
    """Per W in (12 h, 24 h) and type composition one session of four events with gaps W - 1, W and W + 1; session q has
    the aids 10 q ... 10 q + 3."""
    out = []
    for W in (12 * H, DAY):
        for comp in GAP_TYPES.values():
            q = len(out)
            ts = np.cumsum([1000, W - 1, W, W + 1])
            out.append([(10 * q + i, int(ts[i]), comp[i]) for i in range(4)])
    return out


def _span_sessions():
    """Segments of three gaps, each below W, with span w and w + 1 (w = W here): clicks with 4 h gaps under the 12 h
    rule, carts with 8 h gaps under the 24 h rule; the long gap last (the first event's upper bound and the last
    event's lower bound fall back to the search) and, mirrored, first. Session q has the aids 100 + 10 q ..."""
    out = []
    for ty, g in ((CLICK, 4 * H), (CART, 8 * H)):
        for gaps in ([g, g, g], [g, g, g + 1], [g + 1, g, g]):
            q = len(out)
            ts = np.cumsum([-5000] + gaps)
            out.append([(100 + 10 * q + i, int(ts[i]), ty) for i in range(4)])
    return out


def _long_session(n, aid0, step, breaks=(), ty=None, t0=0):
    """n events step seconds apart, with gaps of 13 h before the events in breaks; types cycle click, click, cart,
    click, order unless ty is given."""
    cyc = [CLICK, CLICK, CART, CLICK, BUY]
    t, evs = t0, []
    for i in range(n):
        t += 13 * H if i in breaks else step
        evs.append((aid0 + i % 37, t, cyc[i % 5] if ty is None else ty))
    return evs


def _case_rows(name):
    rng = np.random.default_rng(11)
    if name == "gap_edges":
        return _events(_gap_sessions()), {}
    if name == "span_edges":
        return _events(_span_sessions()), {}
    if name == "breaks_200":  # segment breaks on both sides of the chunk boundaries 64 and 128
        return np.concatenate([_events([_long_session(200, 0, 60, breaks=(63, 64, 65, 127, 128))]),
                               _filler(rng, 30, 500, 1)]), {}
    if name == "start_63":  # the second session starts at index 63 of its batch
        return _events([_long_session(63, 0, 500), _long_session(150, 100, 700, breaks=(1, 66))]), {}
    if name in ("sessions_64", "sessions_65"):  # a batch of exactly 64 two-event sessions; one more
        n = int(name[-2:])
        return _events([[(s % 7, 0, CLICK), (s % 5 + 10, 30, s % 3)] for s in range(n)]), {}
    if name == "batch_512":  # sessions of 255 and 257 events: the second starts in the first block, the batch has 512
        return _events([_long_session(255, 0, 300), _long_session(257, 50, 400, breaks=(100,))]), {}
    if name == "lcap":  # 512 events: the LDS path; 513: the long-session kernels
        return _events([_long_session(512, 0, 100), _long_session(513, 40, 100), _long_session(5, 90, 100)]), {}
    if name == "equal_ts":
        # 60 ordered events, then ten of one ts with descending aids over the indices 60 ... 69 (the run crosses
        # 63 / 64), then ordered events; a second session with three events of one ts, so that of the batch's last
        # two chunks one has equal ts and the other has none
        run = [(300 - i, 60 * 61, CLICK if i % 2 else CART) for i in range(10)]
        s0 = _long_session(60, 0, 60) + run + _long_session(40, 400, 60, t0=60 * 61)
        s1 = _long_session(64, 0, 45) + [(7, 64 * 45 + 45, CLICK), (5, 64 * 45 + 45, CLICK), (6, 64 * 45 + 45, BUY)] + \
            _long_session(30, 20, 45, t0=64 * 45 + 45)
        return _events([s0, s1]), {}
    if name == "twins":
        # the equal-ts run again, with exact duplicates inside it: aid 295 twice, aid 293 three times
        run = [(300 - i, 60 * 61, CLICK) for i in range(10)]
        run = run[:5] + [(295, 60 * 61, CLICK)] + run[5:7] + [(293, 60 * 61, CLICK)] * 2 + run[7:]
        s0 = _long_session(58, 0, 60) + run + _long_session(40, 400, 60, t0=60 * 61)
        return _events([s0, [(1, 5, CART), (1, 5, CART), (2, 9, CART)]]), {}
    if name == "unordered":  # a ts decrease in the middle session of a batch
        mid = _long_session(80, 200, 50)
        mid[40], mid[41] = mid[41], mid[40]
        return _events([_long_session(70, 0, 50), mid, _long_session(70, 300, 50)]), {}
    if name == "ts_range":
        lo, hi = -2 ** 31, 2 ** 31 - 1
        return _events([[(1, lo, CLICK), (2, lo, CLICK), (3, lo + 12 * H, CLICK), (4, lo + 12 * H + 1, CART)],
                        [(5, -12 * H, CLICK), (6, -1, CLICK), (7, 0, CART), (8, 1, CLICK), (9, 12 * H - 1, CLICK),
                         (10, 12 * H, BUY), (11, DAY, BUY)],
                        [(12, hi - DAY, CART), (13, hi - 12 * H, CLICK), (14, hi - 1, CLICK), (15, hi, CLICK),
                         (16, hi, CART)]]), {}
    if name == "typical":
        return None, {}
    if name == "hub":
        return _hub_rows(), {}
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _case(name, dedup=True, min_dt=-DAY, c2c=12 * H):
    """Events, file bounds, n_items, the rules, the reference's merged tables and digests (computed once, read-only)."""
    base = name.split("+")[0]
    if base == "typical":
        ev = synth.generate(3000)
    elif base == "windows":  # the boundary sessions and a typical mix, for the other windows
        g = synth.generate(400, first_session=50)
        rows = np.concatenate([_events(_gap_sessions() + _span_sessions()),
                               np.stack([g.session.astype(np.int64) + 1000, g.aid % 4000 + 1000, g.ts, g.type], 1)])
        ev = synth.events_from_columns(rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3])
    else:
        rows, _ = _case_rows(base)
        ev = synth.events_from_columns(rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3])
    n_items = synth_items(ev)
    nf = 2 if ev.n_sessions >= 4 else 1
    fb = np.linspace(0, ev.n_sessions, nf + 1).astype(np.int64)
    rules, lo, hi = _rules(min_dt, DAY, {C2C: c2c})
    ref = _reference(ev, fb, rules, lo, hi, dedup, brute=not dedup)
    return ev, fb, n_items, rules, ref


def synth_items(ev):
    return max(8192, int(ev.aid.max()) + 1) if len(ev.aid) else 8192


def _count(ev, fb, n_items, env, dedup):
    """One GPU count under the environment switches env (None: unset); returns {rule: (tables, stats, digest)}."""
    from otto_recommender_amd import covis as gc
    old = {k: os.environ.get(k) for k in env}
    for k, v in env.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    try:
        tab = gc.count_co_events_fused(gc.DeviceEvents.from_host(ev, fb), n_items=n_items, dedup=dedup)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    out = {n: (tab.to_numpy(n), tab.stats(n), tab.digest(n)) for n in oracle.REFERENCE_RULES}
    tab.free()
    return out


def _check(request, monkeypatch, name, dedup=True, min_dt=-DAY, c2c=12 * H):
    """All four sides against the reference and the first side. The GPU fixture is taken here, after the caller's
    checks of the construction."""
    ev, fb, n_items, rules, ref = _case(name, dedup, min_dt, c2c)
    request.getfixturevalue("gpu")
    from otto_recommender_amd import config
    monkeypatch.setattr(config, "MIN_TIME_TO_NEXT", min_dt)
    monkeypatch.setitem(config.MAP_MAX_TIME_TO_NEXT, C2C, c2c)
    monkeypatch.setattr(oracle, "MIN_TIME_TO_NEXT", min_dt)
    dig = oracle.files_digest(ev.session_offsets, ev.aid, ev.ts, ev.type, fb, threads=4, rules=rules) if dedup else None
    got = {side: _count(ev, fb, n_items, env, dedup) for side, env in SIDES}
    for side, res in got.items():
        for n in rules:
            (a, b, c, c2), st, d = res[n]
            ra, rb, rc, rc2, fr, fr2 = ref[n]
            np.testing.assert_array_equal(a, ra, err_msg=f"{side} {n}")
            np.testing.assert_array_equal(b, rb, err_msg=f"{side} {n}")
            np.testing.assert_array_equal(c.astype(np.int64), rc, err_msg=f"{side} {n}")
            np.testing.assert_array_equal(c2.astype(np.int64), rc2, err_msg=f"{side} {n}")
            assert (st["n_rows"], st["n_pairs"], st["file_rows"], st["file_rows_ge2"]) == \
                (len(ra), int(rc.sum()), fr, fr2), (side, n)
            if dig is not None:
                for k in ("d_count", "d_count_ge2", "pairs", "pairs_ge2"):
                    assert d[k] == dig[n][k], (side, n, k)
            assert d["rows"] == len(ra), (side, n)
    first = got[SIDES[0][0]]
    for side, res in got.items():
        for n in rules:
            (ta, sa, da), (tb, sb, db) = first[n], res[n]
            for x, y in zip(ta, tb):
                np.testing.assert_array_equal(x, y, err_msg=f"{side} {n}")
            assert sa == sb and da == db, (side, n)


# ------------------------------------------------------------------ tests
def test_gaps_at_the_window_edge(request, monkeypatch):
    ref = _case("gap_edges")[4]
    # sessions in _gap_sessions order: (12 h | 24 h) x (clicks, carts, orders, mixed); aids 10 q + 0 ... 3
    for q, rule in ((0, C2C), (5, K2K), (6, B2B)):  # the rule whose window is the session's W, one type throughout
        a = 10 * q
        assert (_n(ref, rule, a, a + 1), _n(ref, rule, a + 1, a + 2), _n(ref, rule, a + 2, a + 3)) == (1, 1, 0), rule
        assert _n(ref, rule, a, a + 2) == 0  # W - 1 + W apart
    a = 10 * 7  # 24 h, click, cart, order, order
    assert (_n(ref, C2CB, a, a + 1), _n(ref, K2B, a + 1, a + 2), _n(ref, B2B, a + 2, a + 3)) == (1, 1, 0)
    a = 10 * 4  # 24 h, clicks: beyond the 12 h of click_to_click everywhere
    assert sum(_n(ref, C2C, a + i, a + j) for i in range(4) for j in range(4)) == 0
    _check(request, monkeypatch, "gap_edges")


def test_span_at_the_window_edge(request, monkeypatch):
    ref = _case("span_edges")[4]
    for q0, rule in ((0, C2C), (3, K2K)):
        for q, outer in ((q0, 1), (q0 + 1, 0), (q0 + 2, 0)):  # span w: the outer pair counts; w + 1: it does not
            a = 100 + 10 * q
            assert (_n(ref, rule, a, a + 3), _n(ref, rule, a + 3, a)) == (outer, outer), (rule, q)
            assert (_n(ref, rule, a, a + 2), _n(ref, rule, a + 1, a + 3)) == (1, 1), (rule, q)
            assert all(_n(ref, rule, a + i, a + i + 1) == 1 for i in range(3)), (rule, q)
    _check(request, monkeypatch, "span_edges")


@pytest.mark.parametrize("name", ["breaks_200", "start_63", "sessions_64", "sessions_65", "batch_512", "lcap"])
def test_chunk_and_batch_geometry(request, monkeypatch, name):
    ev = _case(name)[0]
    ln = np.diff(ev.session_offsets)
    if name == "start_63":
        assert ev.session_offsets[1] == 63
    if name in ("sessions_64", "sessions_65"):
        assert len(ln) == int(name[-2:]) and (ln == 2).all()
    if name == "batch_512":
        assert list(ln) == [255, 257] and ev.session_offsets[1] < 256
    if name == "lcap":
        assert list(ln[:2]) == [512, 513]
    if name == "breaks_200":
        ts = ev.ts[:200].astype(np.int64)
        assert ln[0] == 200 and list(np.flatnonzero(np.diff(ts) > 12 * H) + 1) == [63, 64, 65, 127, 128]
    _check(request, monkeypatch, name)


def test_equal_ts(request, monkeypatch):
    ev, _, _, _, ref = _case("equal_ts")
    ts = ev.ts[:ev.session_offsets[1]]
    assert (ts[60:70] == ts[60]).all() and ts[59] < ts[60] < ts[70] and (np.diff(ev.aid[60:70]) < 0).all()
    s1 = ev.ts[ev.session_offsets[1]:ev.session_offsets[2]]
    # the batch's chunk 2 (events 128 ... 191) has the second session's equal ts, chunk 3 (from 192) has none
    o1 = int(ev.session_offsets[1])
    assert (s1[64:67] == s1[64]).all() and 128 <= o1 + 64 < o1 + 67 <= 192 and (np.diff(s1[191 - o1:]) > 0).all()
    assert _n(ref, C2C, 299, 297) == 1 and _n(ref, K2K, 300, 298) == 1  # inside the run, by type
    _check(request, monkeypatch, "equal_ts")


@pytest.mark.parametrize("dedup", [True, False])
def test_exact_duplicates(request, monkeypatch, dedup):
    ref = _case("twins", dedup)[4]
    ref_d = _case("twins", True)[4]
    if not dedup:
        # a twin pairs with every other event once more per copy, never with its copies: rows of 295 (twice) and
        # 293 (three times) grow by these factors, (295, 293) by both, and (295, 295), (293, 293) stay absent
        assert _n(ref_d, C2C, 295, 300) == 1 and _n(ref, C2C, 295, 300) == 2 and _n(ref, C2C, 293, 300) == 3
        assert _n(ref, C2C, 295, 293) == 6 and _n(ref, C2C, 295, 295) == 0 and _n(ref, C2C, 293, 293) == 0
        assert _n(ref, K2K, 1, 2) == 2 and _n(ref, K2K, 1, 1) == 0
        # the definition used for this reference agrees with the oracle where the oracle applies (dedup on)
        ev, fb, _, rules, _ = _case("twins", True)
        br = _reference(ev, fb, rules, -DAY, DAY, True, brute=True)
        for n in rules:
            for x, y in zip(br[n], ref_d[n]):
                np.testing.assert_array_equal(x, y, err_msg=n)
    else:
        assert _n(ref, C2C, 295, 300) == 1 and _n(ref, C2C, 295, 293) == 1 and _n(ref, K2K, 1, 2) == 1
    _check(request, monkeypatch, "twins", dedup)


def test_unordered_session(request, monkeypatch):
    ev = _case("unordered")[0]
    o = ev.session_offsets
    dec = [bool((np.diff(ev.ts[o[s]:o[s + 1]].astype(np.int64)) < 0).any()) for s in range(3)]
    assert dec == [False, True, False]
    _check(request, monkeypatch, "unordered")


def test_timestamp_range(request, monkeypatch):
    ev, _, _, _, ref = _case("ts_range")
    assert ev.ts.min() == -2 ** 31 and ev.ts.max() == 2 ** 31 - 1
    assert (_n(ref, C2C, 1, 3), _n(ref, C2C, 1, 2), _n(ref, C2CB, 1, 4), _n(ref, C2CB, 3, 4)) == (1, 1, 1, 1)
    assert (_n(ref, C2C, 5, 6), _n(ref, C2C, 5, 8), _n(ref, C2C, 6, 8), _n(ref, C2C, 8, 9)) == (1, 0, 1, 1)  # across 0
    assert (_n(ref, C2C, 6, 9), _n(ref, C2C, 13, 15), _n(ref, C2CB, 15, 16), _n(ref, C2CB, 15, 12)) == (1, 1, 1, 1)
    _check(request, monkeypatch, "ts_range")


@pytest.mark.parametrize("kw", [{"min_dt": -6 * H}, {"min_dt": 1}, {"c2c": 0}], ids=["min-6h", "min+1", "c2c=0"])
def test_other_windows(request, monkeypatch, kw):
    ref = _case("windows", True, kw.get("min_dt", -DAY), kw.get("c2c", 12 * H))[4]
    a = 100  # the first span session: clicks 4 h apart, aids 100 ... 103
    if kw.get("min_dt") == -6 * H:  # W = 12 h, w = 6 h: forwards up to 12 h, backwards up to 6 h
        assert (_n(ref, C2C, a, a + 3), _n(ref, C2C, a + 3, a), _n(ref, C2C, a + 1, a), _n(ref, C2C, a + 2, a)) == (1, 0, 1, 0)
    if kw.get("min_dt") == 1:  # the window does not contain 0: only later events, never the same ts
        assert (_n(ref, C2C, a, a + 1), _n(ref, C2C, a + 1, a)) == (1, 0)
    if kw.get("c2c") == 0:  # only equal ts pair under click_to_click; the 24 h rules are as before
        assert _n(ref, C2C, a, a + 1) == 0 and _n(ref, K2K, 130, 131) == 1
        assert int(ref[C2C][2].sum()) > 0  # the typical mix has clicks of equal ts
    _check(request, monkeypatch, "windows", True, kw.get("min_dt", -DAY), kw.get("c2c", 12 * H))


def test_saturated_counts(request, monkeypatch):
    """The hub's entries count 256 words each, above the row key's count byte, on both kernels."""
    ref = _case("hub")[4]
    a, _, c = ref[C2CB][:3]
    assert int(c[a == 0x1234].sum()) == 256 * 2048 and int((a == 0x1234).sum()) == 1
    _check(request, monkeypatch, "hub")


def test_typical_mix(request, monkeypatch):
    ev = _case("typical")[0]
    ln = np.diff(ev.session_offsets)
    assert ln.min() >= 2 and ln.max() <= 500 and (ln > 64).any()
    _check(request, monkeypatch, "typical")
