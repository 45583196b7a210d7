"""The emit flush that expands groups of Q consecutive partners of one record per lane (csrc/covis_kernels.h:
emit_flushq, pass 3 of k_emit) at the edges of its groups.

Every table is compared bit-exactly with the per-file tables of the CPU oracle (oracle.count_co_events_files),
merged as in tests/test_reduce_fold_gpu.py: rows, count, count_ge2 and the four per-rule statistics. The twin test
runs with dedup off, where the oracle (which removes exact twins first) is not the specification: its reference is
the pandas restatement without the unique step, as in test_dedup_off_matches_pandas_without_unique, one file.
The record lengths and the per-lane written counts the cases are built for are asserted on the CPU from a
restatement of pass 3's records (per event and (rule, next type): the window of that type's (ts, aid)-ordered
list without the event's own run), for groups of 4 and of 8."""
import functools

import numpy as np
import pytest

import covis as oracle
import covis_pandas
import otto_recommender_amd.synth as synth

pytestmark = pytest.mark.gpu
NAMES = list(oracle.REFERENCE_RULES)
N_ITEMS = 1 << 16
CLICK, CART, ORDER = 0, 1, 2
HOUR = 3600


def _events(sessions):
    """[[(aid, ts, type)]] -> Events (session ids 0, 1, ...)."""
    rows = [(s, a, t, y) for s, ev in enumerate(sessions) for a, t, y in ev]
    a = np.array(rows, np.int64)
    return synth.events_from_columns(a[:, 0], a[:, 1], a[:, 2], a[:, 3])


def _records(sessions, dedup=True):
    """Pass 3's records: (rule, symmetric, own aid, partner aids in list order) per event and (rule, next type)."""
    out = []
    for ev in sessions:
        ev = sorted(set(ev) if dedup else ev, key=lambda e: (e[1], e[0], e[2]))
        for a, t, y in ev:
            for name, (this, nxt, w) in oracle.REFERENCE_RULES.items():
                if y != this:
                    continue
                w = min(w, oracle.MAX_TIME_TO_NEXT)
                for ty in nxt:
                    part = [pa for pa, pt, py in ev if py == ty and abs(pt - t) <= w and (pa, pt, py) != (a, t, y)]
                    if part:
                        out.append((name, tuple(nxt) == (this,), a, part))
    return out


def _lane_counts(records, q):
    """Written words per lane: per group of q consecutive partners, those a symmetric record keeps (aid >= own)."""
    counts = set()
    for _, sym, a, part in records:
        for g in range(0, len(part), q):
            counts.add(sum(1 for p in part[g:g + q] if not sym or p >= a))
    return counts


def _merge(parts):
    """Per-file tables [(aid, aid_next, count)] -> merged (aid, aid_next, count, count_ge2, file_rows, file_rows_ge2)."""
    a = np.concatenate([p[0] for p in parts]).astype(np.int64)
    b = np.concatenate([p[1] for p in parts]).astype(np.int64)
    c = np.concatenate([p[2] for p in parts]).astype(np.int64)
    key, inv = np.unique((a << 32) | b, return_inverse=True)
    cnt = np.bincount(inv, weights=c, minlength=len(key)).astype(np.int64)
    ge2 = np.bincount(inv, weights=np.where(c >= 2, c, 0), minlength=len(key)).astype(np.int64)
    return (key >> 32).astype(np.int32), (key & 0xFFFFFFFF).astype(np.int32), cnt, ge2, len(a), int((c >= 2).sum())


def _oracle_ref(ev, nf):
    fb = np.linspace(0, ev.n_sessions, nf + 1).astype(np.int64)
    per_file = oracle.count_co_events_files(ev.session_offsets, ev.aid, ev.ts, ev.type, fb)
    return fb, {n: _merge([p[n] for p in per_file]) for n in NAMES}


def _assert_tables(tab, ref):
    for n in NAMES:
        a, b, c, c2 = tab.to_numpy(n)
        ra, rb, rc, rc2, fr, fr2 = ref[n]
        np.testing.assert_array_equal(a, ra, err_msg=n)
        np.testing.assert_array_equal(b, rb, err_msg=n)
        np.testing.assert_array_equal(c.astype(np.int64), rc, err_msg=n)
        np.testing.assert_array_equal(c2.astype(np.int64), rc2, err_msg=n)
        st = tab.stats(n)
        assert (st["n_rows"], st["n_pairs"], st["file_rows"], st["file_rows_ge2"]) == (len(ra), int(rc.sum()), fr, fr2), n


def _run(ev, fb, dedup=True):
    from otto_recommender_amd import covis as gc
    return gc.count_co_events_fused(gc.DeviceEvents.from_host(ev, fb), n_items=N_ITEMS, dedup=dedup)


# ---- the cases: sessions as [(aid, ts, type)]

def _group_edge_sessions():
    """One session per n = 2 ... 18 clicks of distinct aids inside an hour, plus a cart and an order: every click's
    click_to_click record has n - 1 partners (every remainder mod 4 and mod 8, the own-run gap at every offset of a
    group) and two click_to_cart_or_buy records of length 1."""
    rng = np.random.default_rng(7)
    out = []
    for n in range(2, 19):
        aids = rng.choice(60_000, n + 2, replace=False)
        ts = np.sort(rng.choice(HOUR, n + 2, replace=False))
        ty = [CLICK] * n + [CART, ORDER]
        out.append([(int(a), int(t), y) for a, t, y in zip(aids, ts, ty)])
    return out


def _symmetric_sessions():
    """Clicks whose aids ascend / descend / alternate high and low in ts order, and one aid at several ts among
    others: a symmetric record keeps the partners with aid >= its own, so the lanes of these records write every
    count from 0 to Q, and an event that keeps nothing sits beside one that keeps every partner."""
    n = 41
    asc = [(100 + 3 * i, 10 * i, CLICK) for i in range(n)]
    desc = [(5000 - 3 * i, 10 * i, CLICK) for i in range(n)]
    alt = [((9000 + i) if i % 2 else (8000 - i), 10 * i, CLICK) for i in range(n)]
    alt2 = [((12000 + i) if (i // 3) % 2 else (11000 - i), 10 * i, CLICK) for i in range(n)]  # runs of three
    rep = [(20_000 if i % 4 == 1 else 20_000 + (i * 37) % 29 - 14, 10 * i, CLICK) for i in range(n)]
    return [asc, desc, alt, alt2, rep]


def _twin_sessions():
    """12 clicks of distinct aids, the click at position p given m = 2 or 3 times (exact twins, kept with dedup off):
    the exclusion gap of xlen = m starts at every offset of a group."""
    out = []
    for m in (2, 3):
        for p in range(12):
            base = 1000 * (len(out) + 1)
            ev = [(base + (i * 7) % 12, 5 * i, CLICK) for i in range(12)]
            out.append(ev[:p] + [ev[p]] * m + ev[p + 1:])
    return out


def _spanning_sessions(n):
    """A few short sessions, then one of n clicks within 12 h (n - 1 partners per click_to_click record: more than
    one round of 64 groups, the first such record starting in the middle of a round)."""
    rng = np.random.default_rng(n)
    short = [[(int(a), 60 * i, CLICK) for i, a in enumerate(rng.choice(60_000, 3, replace=False))] for _ in range(3)]
    aids = rng.choice(60_000, n, replace=False)
    ts = np.sort(rng.choice(12 * HOUR, n, replace=False))
    return short + [[(int(a), int(t), CLICK) for a, t in zip(aids, ts)]]


def _dense_sessions():
    """60 sessions of 62 clicks, a cart and a buy within an hour (the shape of test_emit_record_guard_dense_sessions):
    every event opens a record in every round of pass 3, so every flush is full."""
    rng = np.random.default_rng(5)
    out = []
    for _ in range(60):
        ty = np.zeros(64, np.int64)
        ty[rng.choice(64, 2, replace=False)] = [CART, ORDER]
        aids = rng.choice(50_000, 64, replace=False)
        ts = np.sort(rng.integers(0, HOUR, 64))
        out.append([(int(a), int(t), int(y)) for a, t, y in zip(aids, ts, ty)])
    return out


SESSIONS = {"edges": _group_edge_sessions, "symmetric": _symmetric_sessions,
            "span300": lambda: _spanning_sessions(300), "span500": lambda: _spanning_sessions(500),
            "dense": _dense_sessions}


@functools.lru_cache(maxsize=None)
def _case(name, nf=1):
    """Events, file bounds and the merged oracle tables of a case (computed once, read-only)."""
    sessions = SESSIONS[name]()
    ev = _events(sessions)
    fb, ref = _oracle_ref(ev, nf)
    return sessions, ev, fb, ref


@functools.lru_cache(maxsize=None)
def _twin_case():
    sessions = _twin_sessions()
    ev = _events(sessions)
    df = ev.to_pandas()
    tabs = covis_pandas.as_arrays(covis_pandas.count_co_events(covis_pandas.self_merge_big_df(df)))
    return sessions, ev, np.array([0, ev.n_sessions], np.int64), {n: _merge([tabs[n]]) for n in NAMES}


def test_group_edges(gpu):
    sessions, ev, fb, ref = _case("edges")
    recs = _records(sessions)
    assert {len(p) for n, _, _, p in recs if n == "click_to_click"} == set(range(1, 18))
    assert {len(p) for n, _, _, p in recs if n == "click_to_cart_or_buy"} == {1}
    tab = _run(ev, fb)
    _assert_tables(tab, ref)
    tab.free()


def test_symmetric_lane_counts(gpu):
    sessions, ev, fb, ref = _case("symmetric")
    recs = [r for r in _records(sessions) if r[1]]
    for q in (4, 8):
        assert _lane_counts(recs, q) == set(range(q + 1)), q
    kept = [sum(1 for p in part if p >= a) for _, _, a, part in recs]
    full = [k == len(r[3]) for k, r in zip(kept, recs)]
    assert any((x == 0 and fy) or (fx and y == 0)  # a record that keeps nothing beside one that keeps all
               for x, y, fx, fy in zip(kept, kept[1:], full, full[1:]))
    assert any(a == p for _, _, a, part in recs for p in part)  # equal aids at distinct ts: both orders are kept
    tab = _run(ev, fb)
    _assert_tables(tab, ref)
    tab.free()


def test_exact_twins_dedup_off(gpu):
    sessions, ev, fb, ref = _twin_case()
    # every event of a session is a click inside the window: a record holds all of them but the event's own run
    runs = {len(s) - len(p) for s in sessions for _, _, _, p in _records([s], dedup=False)}
    assert runs == {1, 2, 3}
    tab = _run(ev, fb, dedup=False)
    _assert_tables(tab, ref)
    tab.free()


@pytest.mark.parametrize("name", ["span300", "span500"])
def test_spanning_record(gpu, name):
    sessions, ev, fb, ref = _case(name)
    n = len(sessions[-1])
    assert max(len(p) for _, _, _, p in _records(sessions[-1:])) == n - 1 and (n - 1 + 3) // 4 > 64
    tab = _run(ev, fb)
    _assert_tables(tab, ref)
    tab.free()


@pytest.mark.parametrize("nf", [1, 3])
def test_full_flushes(gpu, nf):
    _, ev, fb, ref = _case("dense", nf)
    tab = _run(ev, fb)
    _assert_tables(tab, ref)
    tab.free()


def test_full_flushes_guard(gpu, monkeypatch):
    """OTTOHIP_DEBUG: the instantiation that checks every record index against the flush's records (err bit 8)."""
    monkeypatch.setenv("OTTOHIP_DEBUG", "1")
    _, ev, fb, ref = _case("dense", 3)
    tab = _run(ev, fb)
    _assert_tables(tab, ref)
    tab.free()


@pytest.mark.parametrize("name", ["edges", "symmetric", "twins", "span300", "span500", "dense"])
def test_two_pair_flush_parity(gpu, monkeypatch, name):
    """OTTOHIP_EMIT_FLUSHQ=0 (emit_flush2, for A/B runs): identical tables from the same inputs."""
    if name == "twins":
        _, ev, fb, ref = _twin_case()
    else:
        _, ev, fb, ref = _case(name, 3 if name == "dense" else 1)
    new = _run(ev, fb, dedup=name != "twins")
    monkeypatch.setenv("OTTOHIP_EMIT_FLUSHQ", "0")
    old = _run(ev, fb, dedup=name != "twins")
    _assert_tables(old, ref)
    for n in NAMES:
        for x, y in zip(new.to_numpy(n), old.to_numpy(n)):
            np.testing.assert_array_equal(x, y, err_msg=n)
        assert new.stats(n) == old.stats(n), n
    new.free()
    old.free()
