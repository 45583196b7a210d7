"""Host-side checks of tests/prims_oracle.py (no GPU): (a) every numpy reference against an independent
formulation (np.lexsort, Python loops) on small inputs, and (b) that the inputs of tests/test_prims_gpu.py
discriminate: wrong results computed in numpy (32-bit partial sums, a lost cross-wave or cross-tile prefix, an
unstable sort, a sort by bits [0, bits) only, one that ignores bit 31, a histogram that counts the padding lanes, a
skip pass that keeps the dropped keys, a run histogram that ignores lo, ...) go through the same check_* functions
that the GPU results go through and have to be turned down."""
import functools

import numpy as np
import pytest

import prims_oracle as O


# ------------------------------------------------------------------------- (a) the references
def test_exclusive_scan_vs_python_loop():
    x = np.array([0xFFFFFFFF, 1, 0, 0xFFFFFFFF, 7] * 3, np.uint32)
    out, tot = O.exclusive_scan(x)
    acc, ref = 0, []
    for v in x.tolist():
        ref.append(acc)
        acc += v
    assert out.dtype == np.uint64 and out.tolist() == ref and tot == acc and acc > 1 << 32
    assert O.exclusive_scan(np.zeros(0, np.uint64)) [1] == 0 and len(O.exclusive_scan(np.zeros(0, np.uint64))[0]) == 0
    big = np.full(5, (1 << 40) - 1, np.uint64)
    assert O.exclusive_scan(big)[0].tolist() == [i * ((1 << 40) - 1) for i in range(5)]


def test_scan_levels():
    """the sizes of the GPU test reach one, two and three levels; 2048^2 + 1 gives the second level 2 tiles"""
    assert O.scan_levels(2048) == [1] and O.scan_levels(2049) == [2, 1]
    assert O.scan_levels(4_194_303) == [2048, 1] and O.scan_levels(4_194_304) == [2048, 1]
    assert O.scan_levels(4_194_305) == [2049, 2, 1]


@pytest.mark.parametrize("bits,shift0", [(1, 0), (7, 0), (8, 0), (9, 0), (17, 0), (25, 0), (32, 0), (17, 8), (32, 8),
                                         (32, 24)])
def test_sort_reference_vs_lexsort_and_loop(bits, shift0):
    rng = np.random.default_rng(bits)
    k = rng.integers(0, 1 << 32, 300, dtype=np.uint64).astype(np.uint32)
    k[::3] = k[1]                                   # ties
    v = O.values(300)
    top = O.top_bit(bits)
    assert top % 8 == 0 and top - 8 < bits <= top
    field = [((int(x) >> shift0) << shift0) % (1 << top) for x in k]
    assert O.sort_field(k, bits, shift0).tolist() == field
    order = np.lexsort((np.arange(300), np.array(field)))
    rk, rv = O.sort_pairs(k, v, bits, shift0)
    np.testing.assert_array_equal(rk, k[order]); np.testing.assert_array_equal(rv, v[order])
    # LSD passes in a Python loop: whole bytes from shift0 up
    pairs = list(zip(k.tolist(), v.tolist()))
    for s in range(shift0, bits, 8):
        pairs = [p for d in range(256) for p in pairs if (p[0] >> s) & 255 == d]
    assert [p[0] for p in pairs] == rk.tolist() and [p[1] for p in pairs] == rv.tolist()


def test_shift0_finishes_a_presorted_input():
    k = O.key_pattern("uniform", 1000); v = O.values(1000)
    o = np.argsort(k & np.uint32(255), kind="stable")
    rk, rv = O.sort_pairs(k[o], v[o], 32, 8)
    fk, fv = O.sort_pairs(k, v, 32)
    np.testing.assert_array_equal(rk, fk); np.testing.assert_array_equal(rv, fv)


def test_skip_and_pass_references_vs_loop():
    mask, inv = O.skip_params(8)
    k = O.skip_input(8, "half", 500)
    rk, rv, rn = O.skip_sort(k, 8, mask, inv)
    kept = [(int(x), i) for i, x in enumerate(k) if int(x) & mask != inv]
    kept.sort(key=lambda p: p[0] & 0xFF)            # list.sort is stable
    assert rn == len(kept) and 100 < rn < 400
    assert rk.tolist() == [p[0] for p in kept] and rv.tolist() == [p[1] for p in kept]
    pk, pv, pn = O.skip_pass(k, mask, inv)
    assert (pk.tolist(), pv.tolist(), pn) == (rk.tolist(), rv.tolist(), rn)   # one byte: the first pass is the sort
    v = O.values(500)
    for shift in (0, 8, 24):
        ok, ov = O.radix_pass(k, v, shift)
        ref = sorted(zip(k.tolist(), v.tolist(), range(500)), key=lambda p: ((p[0] >> shift) & 255, p[2]))
        assert ok.tolist() == [p[0] for p in ref] and ov.tolist() == [p[1] for p in ref]


@pytest.mark.parametrize("n", [1, 16384, 16385, 40000])
def test_digit_start_vs_loop(n):
    k = O.key_pattern("uniform", n)
    keep = O.skip_keep(k, 0xF, 0x3)
    for kp in (None, keep):
        nt = O.n_tiles(n)
        cnt = [[0] * nt for _ in range(256)]
        for i, x in enumerate(k.tolist()):
            if kp is None or kp[i]:
                cnt[(x >> 8) & 255][i // O.RADIX_TILE_KEYS] += 1
        acc, ref = 0, []
        for d in range(256):
            for t in range(nt):
                ref.append(acc)
                acc += cnt[d][t]
        ds = O.digit_start(k, 8, kp)
        assert ds.shape == (256, nt) and ds.reshape(-1).tolist() == ref
        assert acc == (n if kp is None else int(keep.sum()))


def test_run_hist_reference_vs_loop():
    for n, (shift, mask, nb) in [(257, O.RUN_HIST_FIELDS[0]), (257, O.RUN_HIST_FIELDS[1]), (600, O.RUN_HIST_FIELDS[2])]:
        x = O.run_hist_input(n, shift, mask, nb)
        lo, hi = 30, n - 11
        ref = [0] * nb
        for i in range(lo, hi):
            ref[((int(x[i]) & 0xFFFFFFFF) >> shift) & mask] += 1
        assert O.run_hist(x, lo, hi, shift, mask, nb).tolist() == ref
        if mask == 0xFFFF:
            assert (x < 0).any() and (x >= 0).any()          # bit 31: negative int32
        f = (x.view(np.uint32) >> np.uint32(shift)) & np.uint32(mask)
        starts = np.concatenate([[0], np.nonzero(np.diff(f))[0] + 1])
        assert len(set(f[starts].tolist())) < len(starts)      # a key has two separate runs
    assert O.run_hist(np.array([5, 301], np.int32), 0, 2, 0, 0xFFFFFFFF, 300) is None


def test_lds_reference_is_accepted_by_its_check():
    for case in O.LDS_CASES:
        nv, p = case
        d, start = O.lds_digits(p), O.lds_start()
        assert len(d) == 64 and int(d.max()) < 256
        O.check_lds(case, O.lds_ranks_lane_order(d, nv, start), O.lds_hist(d, nv, start))
    # the check does not ask for lane order across separated runs: the two runs of digit 5 may swap
    case = (64, "separated_runs")
    d, start = O.lds_digits("separated_runs"), O.lds_start()
    r = O.lds_ranks_lane_order(d, 64, start)
    r2 = r.copy()
    r2[0:10] = r[17:27] + np.uint32(10)   # first run (10 lanes) after the second (20 lanes)
    r2[17:37] = start[5] + np.arange(20, dtype=np.uint32)
    r2[0:10] = start[5] + np.uint32(20) + np.arange(10, dtype=np.uint32)
    O.check_lds(case, r2, O.lds_hist(d, 64, start))


def test_key_patterns_are_what_they_say():
    n = 5 * 16384 + 777
    k = O.key_pattern("uniform", n)
    assert 0.48 < float((k >> np.uint32(31)).mean()) < 0.52           # bit 31 on about half the keys
    for s in (0, 8, 16, 24):
        assert len(np.unique((k >> np.uint32(s)) & np.uint32(255))) == 256
    assert len(np.unique(O.key_pattern("equal", n))) == 1
    a = O.key_pattern("ascending", n).astype(np.int64)
    assert (np.diff(a) > 0).all() and a[-1] >= 1 << 31
    assert (np.diff(O.key_pattern("descending", n).astype(np.int64)) < 0).all()
    alt = O.key_pattern("alternating", n)
    for s in (0, 8, 16, 24):
        d = (alt >> np.uint32(s)) & np.uint32(255)
        assert d[0] != d[1] and (d[::2] == d[0]).all() and (d[1::2] == d[1]).all()
    for L in (63, 64, 65, 1500):
        r = O.key_pattern(f"runs{L}", n)
        cut = np.nonzero(np.diff(r.astype(np.int64)))[0] + 1
        assert (np.diff(cut) == L).all() and cut[0] == L
    d255 = O.key_pattern("digit255", n)
    assert ((d255 & np.uint32(0xFFFF00FF)) == np.uint32(0xFFFF00FF)).all() and len(np.unique(d255)) == 256
    t0 = O.key_pattern("tail0", n)
    assert n % 64 and (t0[n - n % 64:] == 0).all() and t0[n - n % 64 - 1] != 0
    for bits in (1, 9, 17):
        p = O.key_pattern("payload", n, bits)
        top = O.top_bit(bits)
        assert len(np.unique(p >> np.uint32(top))) > 100 and len(np.unique(O.sort_field(p, bits))) <= min(1 << top, n // 4 + 1)


def test_skip_inputs_drop_what_they_say():
    for c, sc, n in O.SKIP_CASES:
        mask, inv = O.skip_params(c)
        assert inv & ~mask == 0 and mask == (1 << c) - 1 and c % 8 == 0
        k, rk, rv, rn = O.skip_reference(c, sc, n)
        drop = ~O.skip_keep(k, mask, inv)
        want = {"none": 0, "all": n, "subtile": 4096, "block": 16384, "tail": n % 16384, "one_kept": 0,
                "one_dropped": 1}.get(sc)
        if want is None:
            assert 0.45 < drop.mean() < 0.55
        else:
            assert int(drop.sum()) == want and rn == n - want
        if c < 32 and n > 1:
            assert len(np.unique(k >> np.uint32(c))) > 1      # a count rides above the key


# ------------------------------------------------------------------------- (b) the inputs discriminate
def _rejects(check, *args):
    try:
        check(*args)
    except AssertionError:
        return True
    return False


def _scan_result(case, out, tot):
    buf = out if len(out) == case[1] + 1 else np.append(out, np.uint64(O.SENTINEL64))
    return buf, (tot if case[3] else None)


@functools.lru_cache(maxsize=None)
def _scan_kills():
    kills = {}
    for case in O.SCAN_CASES:
        x, out, tot = O.scan_reference(*case[:3])
        O.check_scan(case, *_scan_result(case, out, tot))
        kills[case] = {m for m, f in O.SCAN_MUTANTS.items() if _rejects(O.check_scan, case, *_scan_result(case, *f(x, out, tot)))}
    return kills


@functools.lru_cache(maxsize=None)
def _sort_kills():
    kills = {}
    for case in O.SORT_CASES + O.SHIFT0_CASES + [(n, 32, "uniform") for n in O.XCD_N]:
        k, v, rk, rv = O.sort_reference(*case)
        O.check_sort(case, rk, rv)
        kills[case] = {m for m, f in O.SORT_MUTANTS.items() if _rejects(O.check_sort, case, *f(k, v, case[1]))}
    return kills


@functools.lru_cache(maxsize=None)
def _iota_kills():
    kills = {}
    for case in O.IOTA_CASES:
        n, bits, p = case
        k, v = O.key_pattern(p, n, bits), np.arange(n, dtype=np.uint32)
        O.check_iota(case, *O.sort_pairs(k, v, bits))
        kills[case] = {m for m, f in O.SORT_MUTANTS.items() if _rejects(O.check_iota, case, *f(k, v, bits))}
    return kills


@functools.lru_cache(maxsize=None)
def _skip_kills():
    kills = {}
    for case in O.SKIP_CASES + [(16, "half", n) for n in O.XCD_N]:
        k, rk, rv, rn = O.skip_reference(*case)
        O.check_skip(case, *O._skip_result(k, rk, rv))
        kills[case] = {m for m, f in O.SKIP_MUTANTS.items() if _rejects(O.check_skip, case, *f(k, case[0]))}
    return kills


@functools.lru_cache(maxsize=None)
def _pass_kills():
    kills = {}
    for case in O.PASS_CASES:
        _, _, rk, rv, rn, rd = O.pass_reference(*case)
        O.check_pass(case, *O._pass_result(case, rk, rv, rn, rd))
        kills[case] = {m for m, f in O.PASS_MUTANTS.items() if _rejects(O.check_pass, case, *f(case))}
    return kills


@functools.lru_cache(maxsize=None)
def _lds_kills():
    return {case: {m for m, f in O.LDS_MUTANTS.items()
                   if _rejects(O.check_lds, case, *f(O.lds_digits(case[1]), case[0], O.lds_start()))}
            for case in O.LDS_CASES}


@functools.lru_cache(maxsize=None)
def _run_hist_kills():
    kills = {}
    for case in O.RUN_HIST_CASES:
        n, shift, mask, nb, lo, hi = case
        x = O.run_hist_input(n, shift, mask, nb)
        O.check_run_hist(case, O.run_hist(x, lo, hi, shift, mask, nb))
        kills[case] = {m for m, f in O.RUN_HIST_MUTANTS.items()
                       if _rejects(O.check_run_hist, case, f(x, lo, hi, shift, mask, nb))}
    return kills


FAMILIES = {
    # name: (kills, mutants, pattern of a case, cases too small for any wrong result of the list to differ)
    "scan": (_scan_kills, O.SCAN_MUTANTS, lambda c: c[2], lambda c: False),
    "sort": (_sort_kills, O.SORT_MUTANTS, lambda c: c[2], lambda c: c[0] < 2),
    "iota": (_iota_kills, O.SORT_MUTANTS, lambda c: c[2], lambda c: c[0] < 2),
    "skip": (_skip_kills, O.SKIP_MUTANTS, lambda c: c[1], lambda c: False),
    "pass": (_pass_kills, O.PASS_MUTANTS, lambda c: c[3], lambda c: False),
    "lds": (_lds_kills, O.LDS_MUTANTS, lambda c: c[1], lambda c: False),
    "run_hist": (_run_hist_kills, O.RUN_HIST_MUTANTS, lambda c: (c[1], c[2]), lambda c: False),
}


@pytest.mark.parametrize("family", list(FAMILIES))
def test_every_wrong_result_is_rejected_somewhere(family):
    kills, mutants, _, _ = FAMILIES[family]
    hit = set().union(*kills().values())
    assert hit == set(mutants), set(mutants) - hit


@pytest.mark.parametrize("family", list(FAMILIES))
def test_every_pattern_rejects_a_wrong_result(family):
    kills, _, pattern, _ = FAMILIES[family]
    by = {}
    for case, k in kills().items():
        by.setdefault(pattern(case), set()).update(k)
    assert all(by.values()), [p for p, k in by.items() if not k]


@pytest.mark.parametrize("family", list(FAMILIES))
def test_every_case_rejects_a_wrong_result(family):
    """every GPU case turns down at least one of the wrong results, bar the cases with nothing to get wrong in
    these ways (a sort of fewer than two keys)"""
    kills, _, _, trivial = FAMILIES[family]
    blind = [c for c, k in kills().items() if not k and not trivial(c)]
    assert not blind, blind


def test_the_wrong_results_of_the_issue_hit_where_expected():
    sk = _scan_kills()
    assert "wrap32" in sk[(32, 9, "uniform", 1, 0)] and "wrap32" in sk[(64, 513, "single_first", 0, 0)]
    assert "no_wave_prefix" in sk[(32, 513, "single_first", 0, 0)] and "no_wave_prefix" not in sk[(32, 512, "single_first", 0, 0)]
    assert "no_tile_prefix" in sk[(64, 2049, "single_first", 0, 0)] and "no_tile_prefix" not in sk[(64, 2048, "single_first", 0, 0)]
    assert "no_tile_prefix" in sk[(64, 4_194_305, "uniform", 1, 1)]
    assert all("not_written" in k for c, k in sk.items() if c[1] or c[3])   # the poisoned output shows with zeros too
    assert all("unguarded_store" in k for k in sk.values())
    so = _sort_kills()
    big = 5 * 16384 + 777
    assert "unstable" in so[(big, 32, "equal")] and "unstable" in so[(2, 32, "runs1500")]
    assert "low_bits_only" in so[(4097, 17, "uniform")] and "low_bits_only" not in so[(4097, 16, "uniform")]
    assert "ignores_bit31" in so[(4097, 32, "uniform")] and "ignores_bit31" in so[(4097, 25, "ascending")]
    assert "whole_key" in so[(16385, 9, "payload")] and "whole_key" in so[(16385, 24, "uniform")]
    assert all("padding_as_digit0" in k for c, k in _pass_kills().items())   # no pass size is a whole tile
    assert all("keeps_dropped" in k for c, k in _pass_kills().items() if c[0] and c[1] > 1)
    assert all("keeps_dropped" in k for c, k in _skip_kills().items() if c[1] not in ("none", "one_kept"))
    assert all("counts_padding" in k for c, k in _skip_kills().items() if c[2] % O.RADIX_TILE_KEYS)
    assert all("ignores_lo" in k for c, k in _run_hist_kills().items() if c[4] > 0)
    lk = _lds_kills()
    assert "runs_restart" in lk[(64, "separated_runs")] and "run_past_valid" in lk[(41, "digit0_tail")]
    assert "counts_padding" in lk[(0, "digit0")] and "counts_padding" in lk[(63, "all_equal")]
