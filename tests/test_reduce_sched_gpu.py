"""The reduce's level schedule (csrc/abi.hip: sched_levels; csrc/covis_kernels.h: k_agg_hash, push_task_block).

The hash leaves of a level run on the third stream with a grid of resident blocks that take their tasks from a
device counter (OTTOHIP_HASH_GRID forces the block count; 0: the strided launch), a task that overflows its LDS table
is deferred to the next level's split, and the host reads one counter set per level, with the split's chunk, digit
and count-matrix totals summed by whoever pushes a split task. OTTOHIP_REDUCE_SCHED=1 selects it (the tests here
set it unless they say otherwise); 0, the default, is the loop of blocking reads, which takes the same hash grid.
Every case is compared bit-exactly with the per-file tables of the CPU oracle: rows, count, count_ge2 and the four
per-rule statistics. The debug listing (OTTOHIP_DEBUG) of the level schedule names each level's deferred overflow
tasks ("overflow n"); the other loop's listing does not."""
import functools
import re

import numpy as np
import pytest

import covis as oracle
import otto_recommender_amd.synth as synth
import test_covis_gpu as base
from test_split_lds_gpu import _merge

pytestmark = pytest.mark.gpu
NAMES = list(oracle.REFERENCE_RULES)
N_HUBS = 12
STRIDE = 1 << 16  # hub h (aid h) has the one partner 16 + h * STRIDE
HUB_ITEMS = 16 + N_HUBS * STRIDE
# words per hub row, 1700 .. 5000: from five digits on (> 1680 words) one bucket holding the whole row is above four
# times the expected bucket and goes to the hash leaf; a shorter row's bucket would be split again
HUB_LEN = [1700 + 300 * h for h in range(N_HUBS)]


@pytest.fixture(autouse=True)
def level_schedule(monkeypatch):
    monkeypatch.setenv("OTTOHIP_REDUCE_SCHED", "1")


LEVEL = re.compile(r"level (\d+): sort (\d+)/(\d+)/(\d+)/(\d+)/(\d+) hash (\d+) split (\d+) lds (\d+)(?: overflow (\d+))?")


def _levels(err):
    """The debug listing: per level (hash tasks, split-list tasks, deferred overflow tasks or None)."""
    out = {}
    for m in LEVEL.finditer(err):
        out[int(m.group(1))] = (int(m.group(7)), int(m.group(8)), None if m.group(10) is None else int(m.group(10)))
    return out


def _reference(ev, fb, names=None):
    rules = {n: oracle.REFERENCE_RULES[n] for n in (names or NAMES)}
    per_file = oracle.count_co_events_files(ev.session_offsets, ev.aid, ev.ts, ev.type, fb, rules=rules)
    return per_file, {n: _merge([p[n] for p in per_file]) for n in rules}


def _assert_tables(tab, ref):
    for n in ref:
        a, b, c, c2 = tab.to_numpy(n)
        ra, rb, rc, rc2, fr, fr2 = ref[n]
        np.testing.assert_array_equal(a, ra, err_msg=n)
        np.testing.assert_array_equal(b, rb, err_msg=n)
        np.testing.assert_array_equal(c.astype(np.int64), rc, err_msg=n)
        np.testing.assert_array_equal(c2.astype(np.int64), rc2, err_msg=n)
        st = tab.stats(n)
        assert (st["n_rows"], st["n_pairs"], st["file_rows"], st["file_rows_ge2"]) == (len(ra), int(rc.sum()), fr, fr2), n


def _build_and_check(ev, fb, ref, n_items, names=None, **kw):
    from otto_recommender_amd import covis as gc
    tab = gc.count_co_events_fused(gc.DeviceEvents.from_host(ev, fb), names, n_items=n_items, **kw)
    _assert_tables(tab, ref)
    return tab


def _files(ev, nf):
    return np.linspace(0, ev.n_sessions, nf + 1).astype(np.int64)


# ---------------------------------------------------------------- hash grid edges
@functools.lru_cache(maxsize=None)
def _hubs(nf):
    """Twelve hub aids, hub h clicked in HUB_LEN[h] two-event sessions with its one partner: its clicks row of
    HUB_LEN[h] words is split at level 0 into one bucket, far above the expected size, so one hash task at level 1."""
    h = np.concatenate([np.full(L, k) for k, L in enumerate(HUB_LEN)])
    h = h[np.random.default_rng(3).permutation(len(h))]  # deals every hub's sessions over the files
    n = len(h)
    ev = synth.events_from_columns(np.repeat(np.arange(n), 2), np.stack([h, 16 + h * STRIDE], 1).ravel(),
                                   np.tile([0, 10], n), np.zeros(2 * n, np.int64))
    fb = _files(ev, nf)
    _, ref = _reference(ev, fb)
    a, _, c = ref["click_to_click"][:3]
    for k, L in enumerate(HUB_LEN):
        assert int(c[a == k].sum()) == L
    return ev, fb, ref


@pytest.mark.parametrize("nf", [1, 3])
@pytest.mark.parametrize("grid", ["1", "2", "5", "12", "13", None, "0"])
def test_hash_grid_edges(gpu, monkeypatch, grid, nf):
    """Fewer blocks than hash tasks, as many, more, the resident grid and the strided launch."""
    if grid is None:
        monkeypatch.delenv("OTTOHIP_HASH_GRID", raising=False)
    else:
        monkeypatch.setenv("OTTOHIP_HASH_GRID", grid)
    ev, fb, ref = _hubs(nf)
    _build_and_check(ev, fb, ref, HUB_ITEMS).free()


@pytest.mark.parametrize("sched", ["1", "0"])
def test_hub_rows_are_hash_tasks(gpu, monkeypatch, capfd, sched):
    """The construction of test_hash_grid_edges: level 1 holds at least a dozen hash tasks (both loops list it)."""
    monkeypatch.setenv("OTTOHIP_DEBUG", "1")
    monkeypatch.setenv("OTTOHIP_REDUCE_SCHED", sched)
    monkeypatch.setenv("OTTOHIP_HASH_GRID", "5")
    ev, fb, ref = _hubs(3)
    capfd.readouterr()
    _build_and_check(ev, fb, ref, HUB_ITEMS).free()
    lv = _levels(capfd.readouterr().err)
    assert lv[1][0] >= N_HUBS, lv
    assert (lv[1][2] is not None) == (sched == "1"), lv  # the level schedule's listing names the overflow


# ---------------------------------------------------------------- deferred overflow
@functools.lru_cache(maxsize=None)
def _hot_row(nf):
    """The hot row of test_hot_row_overflow_resplit (tests/test_covis_gpu.py) with the hot aid's share lowered until a
    hash task overflows: that test's 60 k partners leave ~120 distinct keys in the hot key's bucket, far below the
    table's limit of 1024 keys. Here aid 7 is clicked once in each of 376,000 sessions beside three partners that
    occur nowhere else (1.128 M distinct keys, one word each), and twelve times in each of 300 sessions dealt evenly
    among the others (39,600 words of key (7, 7), 3.4 % of the row). Row (click, 7) is split at level 0 into 512
    buckets of ~2,200 distinct keys; the bucket of key (7, 7) is far above the expected size, so it is a hash task
    at level 1, and it passes 1024 keys before half of its words are in: it overflows. The other buckets (~2,200
    words) are split once more at level 1 into register-sort sizes, so level 2's own split list is empty: its
    split consists of the deferred task alone."""
    n_p, k, n_hot, m = 376_000, 3, 300, 12
    sess = np.concatenate([np.repeat(np.arange(n_p), k + 1), np.repeat(n_p + np.arange(n_hot), m)])
    aid = np.concatenate([np.concatenate([np.full((n_p, 1), 7), 1000 + np.arange(n_p * k).reshape(n_p, k)], 1).ravel(),
                          np.full(n_hot * m, 7)])
    ts = np.concatenate([np.tile(np.arange(k + 1) * 10, n_p), np.tile(np.arange(m) * 10, n_hot)])
    sess = np.random.default_rng(4).permutation(n_p + n_hot)[sess]
    o = np.lexsort((ts, sess))
    ev = synth.events_from_columns(sess[o], aid[o], ts[o], np.zeros(len(o), np.int64))
    fb = _files(ev, nf)
    _, ref = _reference(ev, fb, ["click_to_click"])
    a_, b_, c_ = ref["click_to_click"][:3]
    assert int(c_[a_ == 7].sum()) == n_p * k + n_hot * m * (m - 1)  # the row's words
    return ev, fb, ref


@pytest.mark.parametrize("nf", [1, 3])
@pytest.mark.parametrize("grid", ["1", None])
def test_deferred_overflow(gpu, monkeypatch, capfd, grid, nf):
    monkeypatch.setenv("OTTOHIP_DEBUG", "1")
    if grid is None:
        monkeypatch.delenv("OTTOHIP_HASH_GRID", raising=False)
    else:
        monkeypatch.setenv("OTTOHIP_HASH_GRID", grid)
    ev, fb, ref = _hot_row(nf)
    capfd.readouterr()
    _build_and_check(ev, fb, ref, 1_855_603, names=["click_to_click"]).free()
    err = capfd.readouterr().err
    lv = _levels(err)
    assert all(v[2] is not None for v in lv.values()), lv  # the level schedule ran
    assert any(v[2] > 0 for v in lv.values()), lv  # a hash task overflowed
    assert any(v[1] == 0 and v[2] > 0 for v in lv.values()), lv  # a level whose split is deferred tasks only


# ---------------------------------------------------------------- both loops, degenerate loops
@pytest.mark.parametrize("sched", ["1", "0"])
def test_heavy_rows_both_loops(gpu, monkeypatch, sched):
    monkeypatch.setenv("OTTOHIP_REDUCE_SCHED", sched)
    base.test_heavy_rows_split_and_hash_paths(gpu)


def test_no_split_no_hash(gpu, monkeypatch, capfd):
    """synth.generate(400): every row fits a register sort, so the loop is its first level."""
    monkeypatch.setenv("OTTOHIP_DEBUG", "1")
    ev = synth.generate(400)
    fb = _files(ev, 1)
    _, ref = _reference(ev, fb)
    capfd.readouterr()
    _build_and_check(ev, fb, ref, 1_855_603).free()
    lv = _levels(capfd.readouterr().err)
    assert lv == {0: (0, 0, 0)}, lv


def test_no_pairs(gpu):
    """A stream of single-event sessions emits no pair."""
    n = 3000
    ev = synth.events_from_columns(np.arange(n), np.arange(n) % 500, np.arange(n), np.zeros(n, np.int64))
    fb = _files(ev, 3)
    _, ref = _reference(ev, fb)
    assert all(len(ref[k][0]) == 0 for k in ref)
    _build_and_check(ev, fb, ref, 1_855_603).free()


# ---------------------------------------------------------------- file options
@pytest.mark.parametrize("case", ["split_hash", "overflow"])
def test_file_cuts_through_the_schedule(gpu, monkeypatch, capfd, case):
    """Part mode (with its mirror rows), key cuts and per-file rows of tests/test_covis_gpu.py's file-cut test: the
    k_agg_hash variants with file options, on the level schedule."""
    monkeypatch.setenv("OTTOHIP_DEBUG", "1")
    capfd.readouterr()
    base.test_file_cuts_hot_rows(gpu, case)
    lv = _levels(capfd.readouterr().err)
    assert lv and all(v[2] is not None for v in lv.values()), lv
    assert any(v[0] > 0 for v in lv.values()), lv  # hash tasks


def test_per_file_rule_two_blocks(gpu, monkeypatch):
    """per_file_rule: the leaves that also histogram the rule's per-file rows (each block's share flushed at its
    end), two blocks sharing the twelve hash tasks of the hub rows."""
    monkeypatch.setenv("OTTOHIP_HASH_GRID", "2")
    ev, fb, ref = _hubs(3)
    per_file, _ = _reference(ev, fb)
    n = "click_to_click"
    tab = _build_and_check(ev, fb, ref, HUB_ITEMS, per_file_rule=n)
    np.testing.assert_array_equal(tab.file_rows_per_file, [len(p[n][0]) for p in per_file])
    np.testing.assert_array_equal(tab.file_rows_ge2_per_file, [int((p[n][2] >= 2).sum()) for p in per_file])
    tab.free()


# ---------------------------------------------------------------- two builds on one context
def test_two_builds_one_context(gpu, monkeypatch):
    """A build with deferred overflow and several levels, then a much smaller one on the same context: counter
    sets, the pinned level buffer and the overflow lists of the first must not reach the second."""
    ev, fb, ref = _hot_row(3)
    _build_and_check(ev, fb, ref, 1_855_603, names=["click_to_click"]).free()
    ev2 = synth.generate(400)
    fb2 = _files(ev2, 2)
    _, ref2 = _reference(ev2, fb2)
    _build_and_check(ev2, fb2, ref2, 1_855_603).free()
    ev3, fb3, ref3 = _hubs(1)
    _build_and_check(ev3, fb3, ref3, HUB_ITEMS).free()
