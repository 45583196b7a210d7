"""GPU parity tests of the device primitives (csrc/prims.h, lds_add_runs of csrc/common.h, ottohip_run_hist) over
their whole interface, through the ottohip_test_* hooks: bit-exact against the numpy references of
tests/prims_oracle.py, on the named inputs whose power to tell a broken kernel apart tests/test_prims_cpu.py proves."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import prims_oracle as O

pytestmark = pytest.mark.gpu
EINVAL, ERANGE = -1, -2


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    signed = {np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}.get(a.dtype)
    return torch.from_numpy(a.view(signed) if signed else a).cuda()


def _host(t, dtype):
    return t.cpu().numpy().view(dtype)


def _filled(n, dtype):
    return _dev(np.full(n, O.SENTINEL64 if dtype == np.uint64 else O.SENTINEL32, dtype))


def _lib():
    import otto_recommender_amd._lib as L
    return L, L.load()


# ------------------------------------------------------------------------------------------------ scans
@pytest.mark.parametrize("case", O.SCAN_CASES, ids=O.scan_id)
def test_scan(gpu, case):
    """exclusive_scan_u32 / _u64 with and without a total, in place for u64; values whose partial sums pass 2^32
    at every level (thread, wave, tile, block sums, the recursive levels)"""
    import torch
    L, lib = _lib()
    width, n, pattern, want_total, in_place = case
    x = O.scan_reference(width, n, pattern)[0]
    if in_place:
        buf = _dev(np.append(x, np.uint64(O.SENTINEL64)))
        xin = buf
    else:
        buf, xin = _filled(n + 1, np.uint64), _dev(x)
    tot = ctypes.c_uint64(0xDEAD)
    L.check(lib.ottohip_test_scan(gpu.h, L.ptr(xin), L.ptr(buf), n, width, want_total,
                                  ctypes.byref(tot) if want_total else None, L.stream_handle()))
    torch.cuda.synchronize()
    O.check_scan(case, _host(buf, np.uint64), tot.value if want_total else None)


# ------------------------------------------------------------------------------------------------ sort
def _sort(gpu, k, v, bits, shift0=0, iota=0, skip=None, n=None):
    """ottohip_test_sort_pairs on copies of k / v (v None: a SENTINEL32 buffer): (rc, keys, vals, n_out)"""
    import torch
    L, lib = _lib()
    n = len(k) if n is None else n
    kt = _dev(k)
    vt = _filled(len(k), np.uint32) if v is None else _dev(v)
    n_out = ctypes.c_int64(-7)
    mask, inv = skip if skip else (0, 0)
    rc = lib.ottohip_test_sort_pairs(gpu.h, L.ptr(kt), L.ptr(vt), n, bits, shift0, iota, 1 if skip else 0, mask, inv,
                                     ctypes.byref(n_out), L.stream_handle())
    torch.cuda.synchronize()
    return rc, _host(kt, np.uint32), _host(vt, np.uint32), n_out.value


@pytest.mark.parametrize("case", O.SORT_CASES, ids=O.sort_id)
def test_sort_pairs(gpu, case):
    """stable order by the bits [0, 8 * ceil(bits / 8)), arbitrary values, keys over all 32 bits"""
    L, _ = _lib()
    k, v, _, _ = O.sort_reference(*case)
    if case[2] == "uniform" and case[0] >= 1023:
        assert 0.45 < float((k >> np.uint32(31)).mean()) < 0.55   # bit 31 is set on about half the keys
    rc, gk, gv, n_out = _sort(gpu, k, v, case[1])
    L.check(rc)
    assert n_out == case[0]
    O.check_sort(case, gk, gv)


@pytest.mark.parametrize("case", O.IOTA_CASES, ids=O.sort_id)
def test_sort_iota_vals(gpu, case):
    """generated values: the same result as the sort given arange, and the reference's order"""
    L, _ = _lib()
    n, bits, p = case
    k = O.key_pattern(p, n, bits)
    idx = np.arange(n, dtype=np.uint32)
    rc, gk, gv, n_out = _sort(gpu, k, None, bits, iota=1)
    L.check(rc)
    rc2, ek, ev, _ = _sort(gpu, k, idx, bits)
    L.check(rc2)
    O.assert_same(gk, ek, "keys"); O.assert_same(gv, ev, "vals")
    O.check_iota(case, gk, gv)
    assert n_out == n


def test_sort_iota_refusals(gpu):
    k = O.key_pattern("uniform", 100)
    assert _sort(gpu, k, None, 0, iota=1)[0] == EINVAL            # bits == 0 with n > 1: no pass to generate in
    assert _sort(gpu, k, None, 32, shift0=8, iota=1)[0] == EINVAL  # the first digit is not sorted
    assert _sort(gpu, k, None, 8, shift0=8, iota=1)[0] == EINVAL


@pytest.mark.parametrize("case", O.SKIP_CASES, ids=O.skip_id)
def test_sort_skip(gpu, case):
    """the compacting first pass as the engine forms it: n_out, the kept keys in stable order with their indices,
    nothing written behind them"""
    L, _ = _lib()
    c, _, n = case
    k = O.skip_reference(*case)[0]
    rc, gk, gv, n_out = _sort(gpu, k, None, c, iota=1, skip=O.skip_params(c))
    L.check(rc)
    O.check_skip(case, gk, gv, n_out)


def test_sort_skip_refusals(gpu):
    k = O.key_pattern("uniform", 5000)
    rc, _, _, _ = _sort(gpu, k, O.values(5000), 16, iota=0, skip=O.skip_params(16))
    assert rc == EINVAL                                             # skip without generated values
    # inv outside mask: refused before anything is launched (the padding would be counted and never written)
    rc, _, _, n_out = _sort(gpu, k, None, 16, iota=1, skip=(0xFF, 0x100))
    assert rc == EINVAL and n_out == 0
    rc, _, _, n_out = _sort(gpu, k, None, 16, iota=1, skip=(0xFFFF, 0x10000), n=0)
    assert rc == EINVAL and n_out == 0


def test_skip_pass_refuses_inv_outside_mask(gpu):
    L, lib = _lib()
    kt = _dev(O.key_pattern("uniform", 5000))
    ko, vo = _filled(5000, np.uint32), _filled(5000, np.uint32)
    n_out, nt = ctypes.c_int64(-7), ctypes.c_int(-7)
    rc = lib.ottohip_test_radix_skip_pass(gpu.h, L.ptr(kt), L.ptr(ko), L.ptr(vo), 5000, 0xFFFF, 0x30000,
                                          ctypes.byref(n_out), None, 0, ctypes.byref(nt), L.stream_handle())
    assert rc == EINVAL and n_out.value == 0
    with pytest.raises(L.OttoHipError, match="outside mask"):
        L.check(rc)


@pytest.mark.parametrize("case", O.SHIFT0_CASES, ids=O.sort_id)
def test_sort_shift0_finishes_presorted_pairs(gpu, case):
    """pairs ordered by the low byte in numpy, then the passes from bit 8: the full sort"""
    L, _ = _lib()
    k, v, _, _ = O.sort_reference(*case)
    o = np.argsort(k & np.uint32(255), kind="stable")
    rc, gk, gv, _ = _sort(gpu, k[o], v[o], case[1], shift0=8)
    L.check(rc)
    O.check_sort(case, gk, gv)


def _skip_pass(gpu, k, mask, inv):
    import torch
    L, lib = _lib()
    n = len(k)
    kt, ko, vo = _dev(k), _filled(n, np.uint32), _filled(n, np.uint32)
    ds = _filled(256 * O.n_tiles(n), np.uint64)
    n_out, nt = ctypes.c_int64(-7), ctypes.c_int(-7)
    L.check(lib.ottohip_test_radix_skip_pass(gpu.h, L.ptr(kt), L.ptr(ko), L.ptr(vo), n, mask, inv, ctypes.byref(n_out),
                                             L.ptr(ds), ds.numel(), ctypes.byref(nt), L.stream_handle()))
    torch.cuda.synchronize()
    return _host(ko, np.uint32), _host(vo, np.uint32), n_out.value, nt.value, _host(ds, np.uint64)


@pytest.mark.parametrize("case", [c for c in O.SKIP_CASES if c[2] > 1], ids=O.skip_id)
def test_skip_pass_then_shift0_equals_the_single_call(gpu, case):
    """radix_skip_pass + radix_sort_pairs(shift0 = 8), the bucketed rows' fallback, bit for bit the one call"""
    L, _ = _lib()
    c, _, n = case
    k = O.skip_reference(*case)[0]
    mask, inv = O.skip_params(c)
    rc, ek, ev, e_out = _sort(gpu, k, None, c, iota=1, skip=(mask, inv))
    L.check(rc)
    pk, pv, n_out, _, _ = _skip_pass(gpu, k, mask, inv)
    assert n_out == e_out
    rc, gk, gv, _ = _sort(gpu, pk[:n_out], pv[:n_out], c, shift0=8)
    L.check(rc)
    O.assert_same(gk, ek[:n_out], "keys"); O.assert_same(gv, ev[:n_out], "vals")


# ------------------------------------------------------------------------------------------------ one pass
@pytest.mark.parametrize("case", O.PASS_CASES, ids=O.pass_id)
def test_radix_pass(gpu, case):
    """radix_pass at a shift / radix_skip_pass: the output pairs, n_tiles and the whole digit_start matrix (k_rs_hist
    with lds_add_runs inside, the scan of the counts, the scatter)"""
    import torch
    L, lib = _lib()
    skip, n, shift, _ = case
    k, v = O.pass_reference(*case)[:2]
    if skip:
        ko, vo, n_out, nt, ds = _skip_pass(gpu, k, *O.PASS_SKIP)
    else:
        kt, vt, kot, vot = _dev(k), _dev(v), _filled(n, np.uint32), _filled(n, np.uint32)
        dst = _filled(256 * O.n_tiles(n), np.uint64)
        ntc = ctypes.c_int(-7)
        L.check(lib.ottohip_test_radix_pass(gpu.h, L.ptr(kt), L.ptr(vt), L.ptr(kot), L.ptr(vot), n, shift, L.ptr(dst),
                                            dst.numel(), ctypes.byref(ntc), L.stream_handle()))
        torch.cuda.synchronize()
        ko, vo, n_out, nt, ds = _host(kot, np.uint32), _host(vot, np.uint32), n, ntc.value, _host(dst, np.uint64)
    O.check_pass(case, ko, vo, n_out, nt, ds.reshape(256, -1))


# ------------------------------------------------------------------------------------------------ lds_add_runs
@pytest.mark.parametrize("case", O.LDS_CASES, ids=O.lds_id)
def test_lds_add_runs(gpu, case):
    import torch
    L, lib = _lib()
    nv, pattern = case
    d, h0 = _dev(O.lds_digits(pattern)), _dev(O.lds_start())
    ranks, hist = _filled(64, np.uint32), _filled(256, np.uint32)
    L.check(lib.ottohip_test_lds_add_runs(L.ptr(d), nv, L.ptr(h0), L.ptr(ranks), L.ptr(hist), L.stream_handle()))
    torch.cuda.synchronize()
    O.check_lds(case, _host(ranks, np.uint32), _host(hist, np.uint32))


# ------------------------------------------------------------------------------------------------ run histogram
def _run_hist(gpu, x, lo, hi, shift, mask, n_bins, hist="own"):
    import torch
    L, lib = _lib()
    xt = None if x is None else _dev(x)
    ht = _filled(max(n_bins, 1), np.uint64) if hist == "own" else hist
    rc = lib.ottohip_run_hist(gpu.h, L.ptr(xt), lo, hi, shift, mask, n_bins, L.ptr(ht), L.stream_handle())
    torch.cuda.synchronize()
    return rc, None if ht is None else _host(ht, np.uint64)


@pytest.mark.parametrize("case", O.RUN_HIST_CASES, ids=O.run_hist_id)
def test_run_hist(gpu, case):
    L, _ = _lib()
    n, shift, mask, nb, lo, hi = case
    rc, hist = _run_hist(gpu, O.run_hist_input(n, shift, mask, nb), lo, hi, shift, mask, nb)
    L.check(rc)
    O.check_run_hist(case, hist)


def test_run_hist_refusals(gpu):
    L, lib = _lib()
    x = np.array([5, 5, 301, 7], np.int32)
    assert O.run_hist(x, 0, 4, 0, 0xFFFFFFFF, 300) is None
    assert _run_hist(gpu, x, 0, 4, 0, 0xFFFFFFFF, 300)[0] == ERANGE      # a key >= n_bins
    rc, h = _run_hist(gpu, x, 0, 2, 0, 0xFFFFFFFF, 300)                    # not inside the window: fine
    assert rc == 0 and h[5] == 2 and h.sum() == 2
    assert _run_hist(gpu, x, -1, 4, 0, 0xFF, 512)[0] == EINVAL
    assert _run_hist(gpu, x, 3, 2, 0, 0xFF, 512)[0] == EINVAL
    assert _run_hist(gpu, None, 0, 4, 0, 0xFF, 512)[0] == EINVAL
    assert _run_hist(gpu, x, 0, 4, -1, 0xFF, 512)[0] == EINVAL
    assert _run_hist(gpu, x, 0, 4, 32, 0xFF, 512)[0] == EINVAL
    assert _run_hist(gpu, x, 0, 4, 0, 0xFF, 0)[0] == EINVAL
    assert _run_hist(gpu, x, 0, 4, 0, 0xFF, 512, hist=None)[0] == EINVAL
    ht = _filled(512, np.uint64)
    assert lib.ottohip_run_hist(None, L.ptr(_dev(x)), 0, 4, 0, 0xFF, 512, L.ptr(ht), L.stream_handle()) == EINVAL


# ------------------------------------------------------------------------------------------------ XCD tile order
_XCD_CHILD = r"""
import ctypes, sys
import numpy as np
import torch
import prims_oracle as O
import otto_recommender_amd._lib as L

ctx, lib = L.context(0), L.load()
dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).cuda()
bad = 0
for n in O.XCD_N:       # nb < 8, nb % 8 == 0, nb % 8 == 3 with a ragged tail
    k, v = O.key_pattern("uniform", n), O.values(n)
    mask, inv = O.skip_params(16)
    ks = O.skip_input(16, "half", n)
    for skip in (0, 1):
        kt = dev(ks if skip else k)
        vt = dev(np.full(n, O.SENTINEL32, np.uint32) if skip else v)
        n_out = ctypes.c_int64(-7)
        L.check(lib.ottohip_test_sort_pairs(ctx.h, L.ptr(kt), L.ptr(vt), n, 16 if skip else 32, 0, skip, skip, mask, inv,
                                            ctypes.byref(n_out), L.stream_handle()))
        torch.cuda.synchronize()
        gk, gv = kt.cpu().numpy().view(np.uint32), vt.cpu().numpy().view(np.uint32)
        rk, rv, rn = O.skip_sort(ks, 16, mask, inv) if skip else O.sort_pairs(k, v, 32) + (n,)
        ok = n_out.value == rn and np.array_equal(gk[:rn], rk) and np.array_equal(gv[:rn], rv)
        print("n", n, "skip", skip, "n_out", n_out.value, "expected", rn, "ok" if ok else "MISMATCH", flush=True)
        bad += not ok
sys.exit(1 if bad else 0)
"""


def test_sort_xcd_tile_order(gpu):
    """OTTOHIP_RS_XCD=1 (read once per process): a fresh child interpreter sorts 3, 8 and 11 blocks, plain and with
    skip, and compares with numpy itself"""
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, OTTOHIP_RS_XCD="1")
    env["PYTHONPATH"] = os.pathsep.join([os.path.dirname(here), here] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    r = subprocess.run([sys.executable, "-c", _XCD_CHILD], env=env, timeout=180, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    assert r.stdout.count(" ok") == 6, r.stdout
