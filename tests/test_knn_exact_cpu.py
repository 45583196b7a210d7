"""CPU tests of the exact kNN mode (csrc/knn.hip: ottohip_knn_index_create_ex, ottohip_knn_topk_exact): the
entry points exist, and an emulation of the centred packing (fp32 subtraction of the column mean, RNE bf16
factors, hi/lo norm columns, fp32 sums) stays within the bound E of tests/knn_edges.py and obeys the margin rule
the exact search rests on: every oracle top-20 row has a key above kappa24 - delta, with

    Emax(q) = 1.01 * 2^-7 * |q'| N + 2^-15 * (N^2 + |q'| N) + 2^-144,   N = max_w |w'|,
    delta(q) = 2 * Emax(q) * (1 + 2^-20)

(the device adds a rounding guard to delta, so its margin set contains this one). A key replaces the 5 low mantissa
bits of a score by the row slot; the test takes the lowest key a top-20 row can carry and the highest the others
can, so it does not depend on where a row sits in its block."""
import functools

import numpy as np
import pytest
import torch

import knn as oracle
import knn_edges as K

KN_BCAP = 512  # csrc/knn.hip


def test_entry_points_are_declared_and_exported():
    import otto_recommender_amd._lib as L
    lib = L.load()
    for name in ("ottohip_knn_index_create_ex", "ottohip_knn_topk_exact"):
        assert name in L.SIGNATURES, name
        assert hasattr(lib, name), name
    assert len(L.SIGNATURES["ottohip_knn_index_create_ex"][1]) == 7
    assert len(L.SIGNATURES["ottohip_knn_topk_exact"][1]) == 9


def _centred(emb: np.ndarray) -> np.ndarray:
    """v - mean as k_knn_pack forms it: the mean summed in double and rounded to fp32, the subtraction in fp32."""
    mean = emb.astype(np.float64).mean(0).astype(np.float32)
    return emb - mean[None, :]


def _key_range(em: torch.Tensor):
    """(lowest, highest) key of an fp32 score: the 5 low mantissa bits all zero or all one."""
    bits = em.numpy().view(np.int32)
    a = torch.from_numpy((bits & ~np.int32(31)).view(np.float32).copy())
    b = torch.from_numpy((bits | np.int32(31)).view(np.float32).copy())
    return torch.minimum(a, b), torch.maximum(a, b)


@functools.lru_cache(maxsize=None)
def _margin(name: str, centre: bool, chunk: int = 125):
    """(max excess over E, share of oracle top-20 rows inside the margin, smallest and largest margin set)."""
    emb, rows = K.case(name)
    packed = _centred(emb) if centre else emb
    oi, _ = oracle.topk_exact(emb, rows, 20)  # the truth: distances of the rows as given
    e64 = torch.from_numpy(packed).double()
    N = float((e64 * e64).sum(1).max().sqrt())
    excess, inside, total, small, large = 0.0, 0, 0, 1 << 30, 0
    for a in range(0, len(rows), chunk):
        r = rows[a:a + chunk]
        s, err = K.scores64(packed, r)
        em = K.emulated_scores(packed, r)
        lo, hi = _key_range(em)
        excess = max(excess, float((torch.maximum((lo.double() - s).abs(), (hi.double() - s).abs()) / err).max()))
        qn = (e64[torch.from_numpy(r)] ** 2).sum(1).sqrt()
        emax = 1.01 * 2.0 ** -7 * qn * N + 2.0 ** -15 * (N * N + qn * N) + 2.0 ** -144
        delta = 2.0 * emax * (1.0 + 2.0 ** -20)
        k24 = torch.topk(hi.double(), K.KN_C, dim=1).values[:, -1]
        cut = (k24 - delta)[:, None]
        top = torch.from_numpy(oi[a:a + chunk])
        ok = lo.double().gather(1, top) > cut
        inside += int(ok.sum())
        total += ok.numel()
        n = (hi.double() > cut).sum(1)
        small, large = min(small, int(n.min())), max(large, int(n.max()))
    return excess, inside / total, small, large


@pytest.mark.parametrize("name", ["offset8", "clusters0.1", "normal_d100"])
def test_centred_packing_stays_within_the_bound_and_the_margin_holds_the_top20(name):
    excess, share, small, large = _margin(name, True)
    print(f"{name} centred: max |key - s| / E = {excess:.4f}, top-20 rows inside the margin {share:.4f}, "
          f"margin set {small}..{large} rows")
    assert excess <= 1.0
    assert share == 1.0
    assert large <= KN_BCAP  # the rows the rerank must look at fit the buffer


def test_uncentred_offset8_margin_set_exceeds_the_buffer():
    """The reason for centring: with 8 on every component |q||v| is ~6500, delta ~ 100 against distance gaps of a
    few units, and every query's margin set is larger than the 512-entry buffer (the search stays correct through
    the fp32 scan; it is just a scan)."""
    excess, share, small, large = _margin("offset8", False)
    print(f"offset8 uncentred: max |key - s| / E = {excess:.4f}, inside {share:.4f}, margin set {small}..{large} rows")
    assert excess <= 1.0
    assert share == 1.0
    assert small > KN_BCAP
