"""numpy references, named inputs and result checks for the device primitives of csrc/prims.h: the exclusive scans,
the stable LSD radix sort with its options (bits, shift0, generated values, the compacting skip pass), one radix pass
with its digit_start matrix, lds_add_runs on one wave, and the run histogram ottohip_run_hist.

Everything is integer and exact. tests/test_prims_gpu.py runs the library on the cases listed here and hands the
results to the check_* functions; tests/test_prims_cpu.py hands the same functions deliberately wrong results (the
*_MUTANTS below) and requires that they are turned down, so an input that cannot tell a broken kernel from a correct
one shows up without a GPU."""
import functools

import numpy as np

RADIX_TILE_KEYS = 16384   # prims.h: keys per column of digit_start
SUB_TILE = 4096           # keys a block stages at once
SCAN_TILE = 2048          # 256 threads x 8 items
SCAN_WAVE = 512           # 64 lanes x 8 items
U32 = np.uint32
U64 = np.uint64
SENTINEL64 = 0xA5A5A5A5A5A5A5A5
SENTINEL32 = 0xA5A5A5A5


def assert_same(got, ref, what=""):
    """exact equality of two integer arrays; names the first difference (no full diff of millions of words)"""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if not np.array_equal(got, ref):
        i = int(np.flatnonzero(got.reshape(-1) != ref.reshape(-1))[0])
        raise AssertionError(f"{what}: first difference at {i}: got {int(got.reshape(-1)[i])}, "
                             f"expected {int(ref.reshape(-1)[i])}; {int((got != ref).sum())} of {ref.size} differ")


# ---------------------------------------------------------------------------------------------- references
def exclusive_scan(x):
    """(out, total) in uint64: out[i] = sum(x[:i])"""
    x = np.asarray(x).astype(U64)
    inc = np.cumsum(x, dtype=U64)
    out = np.empty(len(x), U64)
    if len(x):
        out[0] = 0
        out[1:] = inc[:-1]
    return out, int(inc[-1]) if len(x) else 0


def scan_levels(n):
    """tile counts of the recursive scan, top level first (a level with one tile ends the recursion)"""
    lv = []
    while n > 0:
        nb = -(-n // SCAN_TILE)
        lv.append(nb)
        if nb == 1:
            break
        n = nb
    return lv


def top_bit(bits):
    """the passes run in whole bytes: first bit that does not take part in the order"""
    return 8 * (-(-bits // 8))


def sort_field(keys, bits, shift0=0):
    m = (1 << top_bit(bits)) - 1
    return (((np.asarray(keys, U32).astype(U64) >> U64(shift0)) << U64(shift0)) & U64(m)).astype(U32)


def sort_order(keys, bits, shift0=0):
    return np.argsort(sort_field(keys, bits, shift0), kind="stable")


def sort_pairs(keys, vals, bits, shift0=0):
    o = sort_order(keys, bits, shift0)
    return keys[o], vals[o]


def skip_keep(keys, mask, inv):
    return (keys & U32(mask)) != U32(inv)


def skip_sort(keys, bits, mask, inv):
    """the skip filter followed by the sort of the kept (key, index) pairs: (keys, vals, n_out)"""
    idx = np.nonzero(skip_keep(keys, mask, inv))[0]
    k = keys[idx]
    o = sort_order(k, bits)
    return k[o], idx[o].astype(U32), len(idx)


def radix_pass(keys, vals, shift):
    o = np.argsort((keys >> U32(shift)) & U32(255), kind="stable")
    return keys[o], vals[o]


def skip_pass(keys, mask, inv):
    idx = np.nonzero(skip_keep(keys, mask, inv))[0]
    k = keys[idx]
    o = np.argsort(k & U32(255), kind="stable")
    return k[o], idx[o].astype(U32), len(idx)


def n_tiles(n):
    return -(-n // RADIX_TILE_KEYS)


def digit_counts(keys, shift, keep=None):
    """[256, n_tiles] counts of digit (key >> shift) & 255 per tile of RADIX_TILE_KEYS input keys (kept keys only)"""
    nt = n_tiles(len(keys))
    d = ((keys >> U32(shift)) & U32(255)).astype(np.int64)
    t = np.arange(len(keys), dtype=np.int64) // RADIX_TILE_KEYS
    cell = d * nt + t
    if keep is not None:
        cell = cell[keep]
    return np.bincount(cell, minlength=256 * nt).reshape(256, nt)


def digit_start(keys, shift, keep=None, counts=None):
    """the exclusive scan, in (digit, tile) order, of digit_counts: uint64 [256, n_tiles]"""
    c = digit_counts(keys, shift, keep) if counts is None else counts
    return exclusive_scan(c.reshape(-1))[0].reshape(c.shape)


def run_hist(x, lo, hi, shift, mask, n_bins):
    """np.bincount of the masked field of x[lo:hi]; None where a key >= n_bins (OTTOHIP_ERANGE)"""
    k = ((x.view(U32)[lo:hi] >> U32(shift)) & U32(mask)).astype(np.int64)
    if len(k) and int(k.max()) >= n_bins:
        return None
    return np.bincount(k, minlength=n_bins).astype(U64)


def lds_hist(digits, nv, start):
    return (start.astype(np.int64) + np.bincount(digits[:nv].astype(np.int64), minlength=256)).astype(U32)


def lds_ranks_lane_order(digits, nv, start):
    """one valid answer of lds_add_runs: every digit's words ranked in lane order"""
    seen = start.astype(np.int64).copy()
    r = np.zeros(64, U32)
    for l in range(nv):
        r[l] = seen[digits[l]]
        seen[digits[l]] += 1
    return r


# ---------------------------------------------------------------------------------------------- named inputs
def _mix32(i):
    """a fixed 32-bit mix of an index array (all four bytes vary)"""
    x = (np.asarray(i).astype(U64) + U64(0x9E3779B9)) & U64(0xFFFFFFFF)
    x = ((x ^ (x >> U64(16))) * U64(0x85EBCA6B)) & U64(0xFFFFFFFF)
    x = ((x ^ (x >> U64(13))) * U64(0xC2B2AE35)) & U64(0xFFFFFFFF)
    return (x ^ (x >> U64(16))).astype(U32)


def _seed(name):
    return sum((i + 1) * ord(c) for i, c in enumerate(name))


def key_pattern(name, n, bits=32):
    """the named key patterns of the sort tests (uint32[n])"""
    rng = np.random.default_rng([_seed(name), n, bits])
    i = np.arange(n, dtype=np.int64)
    if name == "uniform":        # all 32 bits, whatever `bits`: the bits above the last pass are payload
        return rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(U32)
    if name == "equal":          # no byte is 0 (the padding digit) or 255
        return np.full(n, 0x9C3A5E71, U32)
    if name == "ascending":      # spread over the whole range, so bit 31 is set on the upper half
        return ((i * ((1 << 32) // max(n, 1))) & 0xFFFFFFFF).astype(U32)
    if name == "descending":
        return key_pattern("ascending", n, bits)[::-1].copy()
    if name == "alternating":    # two digit values lane by lane, in every byte
        return np.where(i & 1, 0xC4D2E1F3, 0x3B2D1E0C).astype(U32)
    if name.startswith("runs"):  # equal keys (so equal digits in every pass) in runs of the given length
        return _mix32(i // int(name[4:]))
    if name == "digit255":       # passes 0, 2 and 3 see digit 255 only; byte 1 varies
        return (U32(0xFFFF00FF) | (rng.integers(0, 256, n, dtype=np.int64).astype(U32) << U32(8))).astype(U32)
    if name == "tail0":          # the last n % 64 keys are 0: the digit that the padding lanes of a tile carry
        k = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(U32)
        if n % 64:
            k[n - n % 64:] = 0
        return k
    if name == "payload":        # few distinct sort fields, random bits above the last pass
        top = top_bit(bits)
        f = _mix32(rng.integers(0, n // 4 + 1, n)).astype(U64) & U64((1 << top) - 1)
        p = rng.integers(0, 1 << 32, n, dtype=np.uint64) >> U64(top) << U64(top) if top < 32 else U64(0)
        return ((f | p) & U64(0xFFFFFFFF)).astype(U32)
    raise KeyError(name)


KEY_PATTERNS = ("uniform", "equal", "ascending", "descending", "alternating", "runs63", "runs64", "runs65", "runs1500",
                "digit255", "tail0", "payload")


def values(n, tag=0):
    """arbitrary u32 values (not their own indices)"""
    return np.random.default_rng([77, n, tag]).integers(0, 1 << 32, n, dtype=np.uint64).astype(U32)


# ---- scan
SCAN_SMALL_N = (0, 1, 8, 9, 511, 512, 513, 2047, 2048, 2049)
SCAN_LARGE_N = (4_194_303, 4_194_304, 4_194_305)
SCAN_PATTERNS = ("uniform", "zeros", "ones32", "single_first", "single_last", "single_2048")


def scan_input(width, n, pattern):
    """u32: full-range values (a thread's 8-sum is about 2^34, so the carry past 2^32 is taken at every level);
    u64: values below 2^40"""
    dt = U32 if width == 32 else U64
    big = 0xFFFFFFFF if width == 32 else (1 << 40) - 1
    x = np.zeros(n, dt)
    if pattern == "uniform":
        x = np.random.default_rng([5, width, n]).integers(0, big + 1, n, dtype=np.uint64).astype(dt)
    elif pattern == "ones32":
        x[:] = 0xFFFFFFFF
    elif pattern == "single_first" and n:
        x[0] = big
    elif pattern == "single_last" and n:
        x[n - 1] = big
    elif pattern == "single_2048" and n > 2048:
        x[2048] = big
    elif pattern not in SCAN_PATTERNS:
        raise KeyError(pattern)
    return x


def _scan_cases():
    out = []
    for width in (32, 64):
        for n in SCAN_SMALL_N:
            for p in SCAN_PATTERNS:
                if (p == "ones32" and width == 64) or (p == "single_2048" and n <= 2048):
                    continue
                for want_total in (1, 0):
                    out.append((width, n, p, want_total, 0))
        for n in SCAN_LARGE_N:   # the third level: the uniform pattern and one other
            for p in ("uniform", "ones32" if width == 32 else "single_first"):
                for want_total in (1, 0):
                    out.append((width, n, p, want_total, 0))
    out += [(64, 2049, "uniform", 1, 1), (64, 4_194_305, "uniform", 1, 1)]   # in place, out == in
    return out


SCAN_CASES = _scan_cases()   # (width, n, pattern, want_total, in_place)


def scan_id(c):
    return f"u{c[0]}-n{c[1]}-{c[2]}-{'total' if c[3] else 'nototal'}{'-inplace' if c[4] else ''}"


@functools.lru_cache(maxsize=2)
def scan_reference(width, n, pattern):
    x = scan_input(width, n, pattern)
    out, tot = exclusive_scan(x)
    return x, out, tot


def check_scan(case, out_buf, total):
    """out_buf: the n + 1 u64 the scan wrote into, filled with SENTINEL64 before (one guard word behind the output);
    total: the returned total, or None when none was requested"""
    width, n, pattern, want_total, _ = case
    _, ref, tot = scan_reference(width, n, pattern)
    assert len(out_buf) == n + 1
    assert int(out_buf[n]) == SENTINEL64, "the word behind the output was written"
    assert_same(out_buf[:n], ref)
    if want_total:
        assert total == tot, (total, tot)
    else:
        assert total is None


def _scan_grouped(x, out, tot, group):
    """prefix restarted at every `group` items, plus the true prefix of the enclosing tile when group < tile"""
    if not len(x):
        return out, tot
    idx = np.arange(len(x))
    res = out - out[idx // group * group]
    if group < SCAN_TILE:
        res += out[idx // SCAN_TILE * SCAN_TILE]
    return res, tot


# wrong scans, from the input and the true (out, total); an `out` of n + 1 words also holds the word behind the output
SCAN_MUTANTS = {
    "wrap32": lambda x, out, tot: (out & U64(0xFFFFFFFF), tot & 0xFFFFFFFF),      # partial sums kept in 32 bits
    "no_wave_prefix": lambda x, out, tot: _scan_grouped(x, out, tot, SCAN_WAVE),  # the cross-wave hop is lost
    "no_tile_prefix": lambda x, out, tot: _scan_grouped(x, out, tot, SCAN_TILE),  # the block sums are lost
    "total_wrap32": lambda x, out, tot: (out, tot & 0xFFFFFFFF),
    "not_written": lambda x, out, tot: (np.full(len(x), SENTINEL64, U64), SENTINEL64),
    "unguarded_store": lambda x, out, tot: (np.append(out, U64(tot)), tot),       # out[n] is written too
}


# ---- sort
SORT_N = (0, 1, 2, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 16383, 16384, 16385, 5 * 16384 + 777,
          11 * 16384 - 5)
SORT_BITS = (1, 7, 8, 9, 16, 17, 24, 25, 32)


def _sort_cases():
    out = []
    for n in SORT_N:             # every size at 32 and 17 bits
        for bits in (32, 17):
            for p in ("uniform", "runs1500", "tail0"):
                out.append((n, bits, p))
    for n in (4097, 16385):      # every width and every pattern
        for bits in SORT_BITS:
            for p in KEY_PATTERNS:
                if (n, bits, p) not in out:
                    out.append((n, bits, p))
    for p in KEY_PATTERNS:       # every pattern across blocks, sub-tiles and a ragged tail
        if (SORT_N[-2], 32, p) not in out:
            out.append((SORT_N[-2], 32, p))
    return out


SORT_CASES = _sort_cases()       # (n, bits, pattern)
BIG = SORT_N[-2]
# generated values (iota_vals): checked against the sort of (key, arange)
IOTA_CASES = [(n, bits, p) for n in (1, 2, 4097, 16385, BIG) for bits in (32, 17, 8) for p in ("uniform", "runs1500")]
# pairs ordered by the low byte on the host and finished from shift0 = 8: checked against the full sort
SHIFT0_CASES = [(4097, 32, "uniform"), (16385, 17, "payload"), (BIG, 32, "runs1500"), (BIG, 24, "uniform"),
                (16385, 32, "tail0"), (2, 32, "uniform")]
# the XCD tile order: 3 blocks (fewer than 8), 8 blocks, 11 blocks (8 + 3) with a ragged tail; uniform keys at 32
# bits, and the skip input (16, "half", n)
XCD_N = (3 * 16384, 8 * 16384, 11 * 16384 - 5)


def sort_id(c):
    return f"n{c[0]}-b{c[1]}-{c[2]}"


@functools.lru_cache(maxsize=8)
def sort_reference(n, bits, pattern):
    k = key_pattern(pattern, n, bits)
    v = values(n, bits)
    rk, rv = sort_pairs(k, v, bits)
    return k, v, rk, rv


def check_sort(case, keys, vals):
    _, _, rk, rv = sort_reference(*case)
    assert_same(keys, rk)
    assert_same(vals, rv)   # vals == vals_in[stable order]


def check_iota(case, keys, vals):
    n, bits, pattern = case
    k = key_pattern(pattern, n, bits)
    rk, rv = sort_pairs(k, np.arange(n, dtype=U32), bits)
    assert_same(keys, rk, "keys")
    assert_same(vals, rv, "vals")


def _by(k, v, field, reverse_ties=False):
    """sorted by field; reverse_ties: equal fields come out in reversed input order"""
    o = np.lexsort((-np.arange(len(k)), field)) if reverse_ties else np.argsort(field, kind="stable")
    return k[o], v[o]


SORT_MUTANTS = {
    "unstable": lambda k, v, bits: _by(k, v, sort_field(k, bits), reverse_ties=True),
    "low_bits_only": lambda k, v, bits: _by(k, v, k & U32((1 << bits) - 1)),          # [0, bits), not whole bytes
    "ignores_bit31": lambda k, v, bits: _by(k, v, sort_field(k, bits) & U32(0x7FFFFFFF)),
    "whole_key": lambda k, v, bits: _by(k, v, k),                                      # the payload orders too
    "values_left": lambda k, v, bits: (sort_pairs(k, v, bits)[0], v),                  # keys move, values do not
}


# ---- skip (the engine's form: mask = (1 << c) - 1 for a byte-aligned c, inv inside it, a count riding above c)
SKIP_N = 5 * 16384 + 777
SKIP_SCENARIOS = ("none", "all", "subtile", "block", "tail", "half", "one_kept", "one_dropped")


def skip_params(c):
    return (1 << c) - 1, 3 << (c - 2)


def skip_input(c, scenario, n):
    mask, inv = skip_params(c)
    rng = np.random.default_rng([9, c, n, _seed(scenario)])
    f = rng.integers(0, 1 << c, n, dtype=np.uint64)
    f[f == inv] ^= 1                                     # no key is dropped by chance
    drop = np.zeros(n, bool)
    if scenario == "all" or scenario == "one_dropped":
        drop[:] = True
    elif scenario == "subtile":                          # the second sub-tile of the second block
        drop[16384 + 4096:16384 + 8192] = True
    elif scenario == "block":
        drop[2 * 16384:3 * 16384] = True
    elif scenario == "tail":                             # the ragged last block
        drop[(n // 16384) * 16384:] = True
    elif scenario == "half":
        drop = rng.random(n) < 0.5
    f[drop] = inv
    count = rng.integers(0, 1 << (32 - c), n, dtype=np.uint64) << U64(c)
    return ((f | count) & U64(0xFFFFFFFF)).astype(U32)


def _skip_cases():
    out = []
    for c in (8, 16, 24):
        for sc in SKIP_SCENARIOS:
            n = 1 if sc.startswith("one_") else SKIP_N
            out.append((c, sc, n))
        out.append((c, "half", 4097))
    return out


SKIP_CASES = _skip_cases()       # (c, scenario, n); bits = c


def skip_id(c):
    return f"c{c[0]}-{c[1]}-n{c[2]}"


@functools.lru_cache(maxsize=8)
def skip_reference(c, scenario, n):
    k = skip_input(c, scenario, n)
    mask, inv = skip_params(c)
    return (k,) + skip_sort(k, c, mask, inv)


def check_skip(case, keys_buf, vals_buf, n_out):
    """keys_buf / vals_buf: the caller's n-entry buffers after the call (keys_buf held the input, vals_buf
    SENTINEL32): the first n_out entries are the result, the rest is as it was"""
    k, rk, rv, rn = skip_reference(*case)
    assert n_out == rn, (n_out, rn)
    assert_same(keys_buf[:rn], rk)
    assert_same(vals_buf[:rn], rv)   # the original indices
    assert_same(keys_buf[rn:], k[rn:])
    assert (vals_buf[rn:] == U32(SENTINEL32)).all()


def _skip_result(k, kk, vv):
    n = len(k)
    kb = k.copy(); vb = np.full(n, SENTINEL32, U32)
    m = min(len(kk), n)
    kb[:m] = kk[:m]; vb[:m] = vv[:m]
    return kb, vb, len(kk)


def _skip_keeps_dropped(k, c):
    o = sort_order(k, c)
    return _skip_result(k, k[o], o.astype(U32))


def _skip_counts_padding(k, c):
    """the histogram counts the padding of the last tile: n_out grows by it, the pairs are the right ones"""
    rk, rv, rn = skip_sort(k, c, *skip_params(c))
    kb, vb, _ = _skip_result(k, rk, rv)
    return kb, vb, rn + (-len(k)) % RADIX_TILE_KEYS


def _skip_unstable(k, c):
    mask, inv = skip_params(c)
    idx = np.nonzero(skip_keep(k, mask, inv))[0]
    kk = k[idx]
    o = np.lexsort((-np.arange(len(kk)), sort_field(kk, c)))
    return _skip_result(k, kk[o], idx[o].astype(U32))


def _skip_count_orders(k, c):
    """the count above the key takes part in the order"""
    mask, inv = skip_params(c)
    idx = np.nonzero(skip_keep(k, mask, inv))[0]
    kk = k[idx]
    o = np.argsort(kk, kind="stable")
    return _skip_result(k, kk[o], idx[o].astype(U32))


SKIP_MUTANTS = {"keeps_dropped": _skip_keeps_dropped, "counts_padding": _skip_counts_padding,
                "unstable": _skip_unstable, "count_orders": _skip_count_orders}


# ---- one pass (radix_pass at a shift, radix_skip_pass) with its digit_start matrix
PASS_N = (1, 4097, 16385, 5 * 16384 + 777)
PASS_PATTERNS = ("uniform", "runs1500", "equal")
PASS_SKIP = (1 << 16) - 1, 3 << 14   # the skip pass' (mask, inv)


def pass_input(skip, n, pattern):
    k = key_pattern(pattern, n)
    if skip and n > 1:           # about a third of the keys are dropped, in runs of 1 to 99
        mask, inv = PASS_SKIP
        rng = np.random.default_rng([13, n, _seed(pattern)])
        run = np.repeat(rng.random(n // 50 + 1) < 0.33, rng.integers(1, 100, n // 50 + 1))
        drop = np.resize(run, n)
        k = np.where(drop, (k & ~U32(mask)) | U32(inv), k).astype(U32)
        k[~drop & ((k & U32(mask)) == U32(inv))] ^= U32(1)
    return k


PASS_CASES = ([(0, n, s, p) for n in PASS_N for s in (0, 8, 24) for p in PASS_PATTERNS] +
              [(1, n, 0, p) for n in PASS_N for p in PASS_PATTERNS])   # (skip, n, shift, pattern)


def pass_id(c):
    return f"{'skip' if c[0] else 'pass'}-n{c[1]}-s{c[2]}-{c[3]}"


@functools.lru_cache(maxsize=8)
def pass_reference(skip, n, shift, pattern):
    """(keys, vals or None, out keys, out vals, n_out, digit_start)"""
    k = pass_input(skip, n, pattern)
    if skip:
        rk, rv, rn = skip_pass(k, *PASS_SKIP)
        return k, None, rk, rv, rn, digit_start(k, 0, skip_keep(k, *PASS_SKIP))
    v = values(n, shift)
    rk, rv = radix_pass(k, v, shift)
    return k, v, rk, rv, n, digit_start(k, shift)


def check_pass(case, kout, vout, n_out, nt, dstart):
    """kout / vout: the n-entry output buffers, filled with SENTINEL32 before; dstart: uint64 [256, nt]"""
    _, _, rk, rv, rn, rd = pass_reference(*case)
    assert n_out == rn, (n_out, rn)
    assert nt == n_tiles(case[1]), nt
    assert_same(np.asarray(dstart).reshape(256, -1), rd)
    assert_same(kout[:rn], rk)
    assert_same(vout[:rn], rv)
    assert (kout[rn:] == U32(SENTINEL32)).all() and (vout[rn:] == U32(SENTINEL32)).all()


def _pass_result(case, rk, rv, rn, dstart):
    n = case[1]
    kb = np.full(n, SENTINEL32, U32); vb = np.full(n, SENTINEL32, U32)
    kb[:rn] = rk[:rn]; vb[:rn] = rv[:rn]
    return kb, vb, rn, n_tiles(n), dstart


def _pass_padding_as_digit0(case):
    """the histogram counts the padding lanes of the last tile as digit 0"""
    k, _, rk, rv, rn, _ = pass_reference(*case)
    keep = skip_keep(k, *PASS_SKIP) if case[0] else None
    c = digit_counts(k, case[2], keep)
    c[0, -1] += (-len(k)) % RADIX_TILE_KEYS
    return _pass_result(case, rk, rv, rn, digit_start(k, case[2], counts=c))


def _pass_keeps_dropped(case):
    k = pass_reference(*case)[0]
    o = np.argsort((k >> U32(case[2])) & U32(255), kind="stable")
    v = np.arange(len(k), dtype=U32) if case[0] else pass_reference(*case)[1]
    return _pass_result(case, k[o], v[o], len(k), digit_start(k, case[2]))


def _pass_unstable(case):
    k, v, rk, rv, rn, rd = pass_reference(*case)
    o = np.lexsort((-np.arange(rn), (rk >> U32(case[2])) & U32(255)))
    return _pass_result(case, rk[o], rv[o], rn, rd)


def _pass_tile_major(case):
    """digit_start scanned in (tile, digit) order"""
    k, _, rk, rv, rn, _ = pass_reference(*case)
    c = digit_counts(k, case[2], skip_keep(k, *PASS_SKIP) if case[0] else None)
    d = exclusive_scan(c.T.reshape(-1))[0].reshape(c.T.shape).T
    return _pass_result(case, rk, rv, rn, np.ascontiguousarray(d))


PASS_MUTANTS = {"padding_as_digit0": _pass_padding_as_digit0, "keeps_dropped": _pass_keeps_dropped,
                "unstable": _pass_unstable, "tile_major_offsets": _pass_tile_major}


# ---- lds_add_runs on one wave
LDS_NV = (0, 1, 63, 64)


def lds_digits(pattern):
    l = np.arange(64)
    if pattern == "all_equal":
        d = np.full(64, 7)
    elif pattern == "all_distinct":
        d = (l * 4 + 3) % 256
    elif pattern == "runs_1_2_31_32":          # lengths 1, 2, 31 (ends at lane 33), then lanes 34..63: 30 (a 32 cut)
        d = np.repeat([200, 17, 255, 1], [1, 2, 31, 30])
    elif pattern == "runs_32_32":
        d = np.repeat([9, 250], [32, 32])
    elif pattern == "separated_runs":          # digit 5 in two runs with another digit between them
        d = np.repeat([5, 99, 5, 0, 5], [10, 7, 20, 3, 24])
    elif pattern == "digit0":                  # the digit of the padding lanes, valid and not
        d = np.zeros(64, np.int64)
    elif pattern == "digit0_tail":             # the valid prefix ends in digit 0 and the lanes behind it carry 0 too
        d = np.where(l < 40, 31, 0)
    else:
        raise KeyError(pattern)
    return d.astype(U32)


LDS_PATTERNS = ("all_equal", "all_distinct", "runs_1_2_31_32", "runs_32_32", "separated_runs", "digit0", "digit0_tail")
LDS_CASES = [(nv, p) for p in LDS_PATTERNS for nv in LDS_NV] + [(41, "digit0_tail"), (12, "separated_runs")]


def lds_id(c):
    return f"nv{c[0]}-{c[1]}"


def lds_start():
    return np.random.default_rng(21).integers(1, 1 << 20, 256).astype(U32)


def check_lds(case, ranks, hist):
    nv, pattern = case
    d, start = lds_digits(pattern), lds_start()
    assert_same(hist, lds_hist(d, nv, start))
    assert (ranks[nv:] == 0).all(), "an invalid lane returned a rank"
    for g in np.unique(d[:nv]):
        lanes = np.nonzero(d[:nv] == g)[0]
        r = np.sort(ranks[lanes].astype(np.int64))
        assert_same(r, int(start[g]) + np.arange(len(lanes)))   # start .. start + count - 1, once each
    for l in range(1, nv):
        if d[l] == d[l - 1]:
            assert int(ranks[l]) == int(ranks[l - 1]) + 1, l   # ascending by one inside a run


def _lds_runs_restart(d, nv, start):
    r = lds_ranks_lane_order(d, nv, start)
    for l in range(nv):
        s = l
        while s > 0 and d[s - 1] == d[l]:
            s -= 1
        r[l] = start[d[l]] + (l - s)
    return r, lds_hist(d, nv, start)


def _lds_counts_padding(d, nv, start):
    return lds_ranks_lane_order(d, nv, start), lds_hist(d, 64, start)


def _lds_invalid_ranked(d, nv, start):
    return lds_ranks_lane_order(d, 64, start), lds_hist(d, nv, start)


def _lds_run_past_valid(d, nv, start):
    """the last run is added with its whole length, not cut at nv"""
    h = lds_hist(d, nv, start)
    e = nv
    while 0 < nv and e < 64 and d[e] == d[nv - 1]:
        e += 1
    if nv:
        h[d[nv - 1]] += U32(e - nv)
    return lds_ranks_lane_order(d, nv, start), h


def _lds_ignores_start(d, nv, start):
    return lds_ranks_lane_order(d, nv, np.zeros(256, U32)), lds_hist(d, nv, start)


LDS_MUTANTS = {"runs_restart": _lds_runs_restart, "counts_padding": _lds_counts_padding,
               "invalid_ranked": _lds_invalid_ranked, "run_past_valid": _lds_run_past_valid,
               "ignores_start": _lds_ignores_start}


# ---- run histogram
RUN_HIST_N = (1, 255, 256, 257, 100_003)
RUN_HIST_FIELDS = ((16, 0xFFFF, 1 << 16), (0, 0xFFFF, 1 << 16), (0, 0xFFFFFFFF, 300))   # (shift, mask, n_bins)


def run_hist_input(n, shift, mask, n_bins):
    """int32[n] whose masked field forms runs (lengths 1..9, one of 60 where it fits); some key comes back in a
    later run; the bits outside the field are random, so bit 31 is set on about half the values where the field
    leaves it free, and the 16-bit fields reach 0x8000 and above"""
    rng = np.random.default_rng([31, n, shift, mask & 0xFFFF, n_bins])
    lens = rng.integers(1, 10, n)
    if n > 100:
        lens[3] = 60
    keys = rng.integers(0, min(n_bins, 40 if n < 1000 else n_bins), n, dtype=np.int64)
    if n_bins > 0x8000:
        keys[::2] |= 0x8000
    keys[5:6] = keys[1:2]                      # the same key in two separate runs
    for j in range(1, n):                      # neighbours differ, so the runs are the ones laid out
        if keys[j] == keys[j - 1]:
            keys[j] = (keys[j] + 1) % n_bins
    f = np.repeat(keys, lens)[:n].astype(U64)
    other = rng.integers(0, 1 << 32, n, dtype=np.uint64) & ~(U64(mask) << U64(shift)) & U64(0xFFFFFFFF)
    return ((f << U64(shift)) | other).astype(U32).view(np.int32)


def _run_hist_cases():
    out = []
    for n in RUN_HIST_N:
        for shift, mask, nb in RUN_HIST_FIELDS:
            out.append((n, shift, mask, nb, 0, n))
            if n >= 255:   # lo and hi inside runs (index 3 starts a run of 60 when n > 100), lo > 0; and hi == lo
                x = run_hist_input(n, shift, mask, nb)
                f = (x.view(U32) >> U32(shift)) & U32(mask)
                lo = int(np.nonzero(np.diff(f))[0][2]) + 1 + 20
                hi = n - 1
                while hi > lo and f[hi] != f[hi - 1]:
                    hi -= 1
                assert lo > 0 and f[lo] == f[lo - 1] and f[hi] == f[hi - 1] and hi > lo
                out += [(n, shift, mask, nb, lo, hi), (n, shift, mask, nb, lo, lo)]
    return out


RUN_HIST_CASES = _run_hist_cases()   # (n, shift, mask, n_bins, lo, hi)


def run_hist_id(c):
    return f"n{c[0]}-s{c[1]}-m{c[2]:x}-b{c[3]}-{c[4]}-{c[5]}"


@functools.lru_cache(maxsize=4)
def _run_hist_input_cached(n, shift, mask, n_bins):
    return run_hist_input(n, shift, mask, n_bins)


def check_run_hist(case, hist):
    n, shift, mask, nb, lo, hi = case
    ref = run_hist(_run_hist_input_cached(n, shift, mask, nb), lo, hi, shift, mask, nb)
    assert ref is not None
    assert_same(hist, ref)


def _rh_runs_once(x, lo, hi, shift, mask, nb):
    """a key's second run overwrites its first"""
    k = ((x.view(U32)[lo:hi] >> U32(shift)) & U32(mask)).astype(np.int64)
    h = np.zeros(nb, U64)
    if len(k):
        s = np.concatenate([[0], np.nonzero(np.diff(k))[0] + 1, [len(k)]])
        h[k[s[:-1]]] = np.diff(s).astype(U64)
    return h


RUN_HIST_MUTANTS = {
    "ignores_lo": lambda x, lo, hi, s, m, nb: run_hist(x, 0, hi, s, m, nb),          # the run that lo cuts counts whole
    "whole_runs": lambda x, lo, hi, s, m, nb: run_hist(x, _run_start(x, lo, hi, s, m), hi, s, m, nb),
    "runs_once": _rh_runs_once,
    "misses_last": lambda x, lo, hi, s, m, nb: run_hist(x, lo, max(lo, hi - 1), s, m, nb),   # the end at hi - 1 is lost
}


def _run_start(x, lo, hi, shift, mask):
    f = (x.view(U32) >> U32(shift)) & U32(mask)
    while lo > 0 and lo < hi and f[lo - 1] == f[lo]:
        lo -= 1
    return lo
