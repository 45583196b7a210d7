"""KMeans (csrc/popularity.hip, stage C2) across the dispatch of launch_km_assign, against float64.

A. One exact E-step (ottohip_kmeans_partial / _assign: the MFMA kernel at dim % 4 == 0, the VALU kernel
   otherwise) against float64 scores on rows next to decision boundaries (tests/kmeans_estep.py): the only
   tolerance is the kernel's own stated score error e(x) = 2e-5 cmax (|x| + cmax).
B. Every E-step path of KMeans.fit (bf16 split pass, distance bounds, f16 rows, move lists, k_km_split16,
   lock-step runs) bit-identical to the exact steps at the dims and k no other test reaches, and the exact
   steps against the float64 restatement (oracle/popularity.py) with the existing tolerances.
C. The near-tie lists of the split passes past their LDS capacity (the spill to the global list).
D. The small kernels around the E-step, exactly or to a bound worked out from their arithmetic.
E. The documented limits, refused before any launch."""
import ctypes

import numpy as np
import pytest

import kmeans_estep as ke
from test_popularity_gpu import _check_kmeans

pytestmark = pytest.mark.gpu

OTTOHIP_EINVAL, OTTOHIP_ERANGE, OTTOHIP_ELIMIT = -1, -2, -5  # include/ottohip.h
KM_ENV = ("OTTOHIP_KM_SPLIT", "OTTOHIP_KM_H16", "OTTOHIP_KM_BOUNDS", "OTTOHIP_KM_MV", "OTTOHIP_KM_S16",
          "OTTOHIP_KM_GROUP", "OTTOHIP_KM_LANES", "OTTOHIP_KM_EGRID")


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _n_cu():
    import torch
    return int(torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count)


def _set_env(monkeypatch, env):
    for name in KM_ENV:
        monkeypatch.delenv(name, raising=False)
    for name, v in env.items():
        monkeypatch.setenv("OTTOHIP_KM_" + name, v)


# ---------------------------------------------------------------- A. one E-step against float64

def _partial(gpu, Xd, Cd, labels_in):
    """ottohip_kmeans_partial: (labels, sums [k, dim], counts, inertia, n_changed) as numpy / Python values."""
    import torch
    from otto_recommender_amd import _lib
    n, dim = Xd.shape
    k = Cd.shape[0]
    labels = _dev(labels_in.astype(np.int32))
    sums = torch.full((k * dim,), -7, dtype=torch.int64, device="cuda")  # overwritten, not accumulated
    counts = torch.full((k,), -7, dtype=torch.int64, device="cuda")
    inr, chg = ctypes.c_double(), ctypes.c_int64()
    _lib.check(_lib.load().ottohip_kmeans_partial(gpu.h, _lib.ptr(Xd), n, dim, _lib.ptr(Cd), k, _lib.ptr(labels),
                                                  _lib.ptr(sums), _lib.ptr(counts), ctypes.byref(inr),
                                                  ctypes.byref(chg), _lib.stream_handle()))
    return labels.cpu().numpy(), sums.cpu().numpy().reshape(k, dim), counts.cpu().numpy(), inr.value, chg.value


def _estep_case(gpu, dim, k, n):
    X, C = ke.boundary_fixture(dim, k, n, ke.fixture_seed(dim, k, n))
    Xd, Cd = _dev(X), _dev(C)
    ref = ke.ref_scores(X, C).argmin(1)
    first = None
    for lin in ke.label_inputs(ref, k, 3):
        lab, sums, counts, inertia, n_changed = _partial(gpu, Xd, Cd, lin)
        if first is None:
            first = lab
            st = ke.check_labels(X, C, lab)
        np.testing.assert_array_equal(lab, first)  # the labels do not depend on the labels passed in
        ke.check_sums(X, lab, sums, counts, k)
        ke.check_changed(lin, lab, n_changed)
        ir = ke.check_inertia(X, C, lab, inertia)
    print(f"estep dim={dim} k={k} n={n}: undecidable {st['undecidable']:.4f}, worst (s_label - min s) / 2e "
          f"{st['worst']:.2e}, tightest gap / 2e resolved as float64 {st['tightest']:.2e}, |inertia - f64| / sum e "
          f"{ir:.4f}")
    if k >= 2:
        Xt, Ct, dup_hi, dup_rows = ke.tie_fixture(dim, k, n, ke.fixture_seed(dim, k, n) + 7)
        lab, sums, counts, inertia, n_changed = _partial(gpu, _dev(Xt), _dev(Ct), np.full(n, -1))
        ke.check_ties(Xt, Ct, lab, dup_hi, dup_rows)
        ke.check_sums(Xt, lab, sums, counts, k)
        ke.check_inertia(Xt, Ct, lab, inertia)
        assert n_changed == n


@pytest.mark.parametrize("dim,k", ke.shapes())
def test_estep_matches_float64(gpu, dim, k):
    """The exact E-step at every (dim, k) of the dispatch: decidable rows get the float64 argmin, the others a
    label within 2 e(x) of the minimum, equal scores the lowest index; sums, counts and n_changed exact under
    the device's own labels; inertia within sum e(x)."""
    _estep_case(gpu, dim, k, ke.N_ROWS)


@pytest.mark.parametrize("n", ke.SMALL_N)
def test_estep_matches_float64_few_rows(gpu, n):
    """Less than a tile, a tile, a tile and a row, n = k (dim 100, k 9)."""
    _estep_case(gpu, 100, 9, n)


@pytest.mark.parametrize("dim,k", [(116, 33), (30, 9), (4, 64)])
def test_assign_equals_partial(gpu, dim, k):
    """ottohip_kmeans_assign (labels and inertia only: no sums in LDS) gives partial's labels."""
    import torch
    from otto_recommender_amd import _lib
    n = ke.N_ROWS
    X, C = ke.boundary_fixture(dim, k, n, ke.fixture_seed(dim, k, n))
    Xd, Cd = _dev(X), _dev(C)
    lab_p = _partial(gpu, Xd, Cd, np.full(n, -1))[0]
    labels = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    inr = ctypes.c_double()
    _lib.check(_lib.load().ottohip_kmeans_assign(gpu.h, _lib.ptr(Xd), n, dim, _lib.ptr(Cd), k, _lib.ptr(labels),
                                                 ctypes.byref(inr), _lib.stream_handle()))
    np.testing.assert_array_equal(labels.cpu().numpy(), lab_p)
    ke.check_inertia(X, C, lab_p, inr.value)


# ---------------------------------------------------------------- B. every E-step path at the new shapes

def _blobs(dim, k, n=6007):
    rng = np.random.default_rng(1000 * dim + k)
    kb = k + (k + 4) // 5
    centers = rng.normal(scale=3, size=(kb, dim))
    return (centers[rng.integers(0, kb, n)] + rng.normal(size=(n, dim))).astype(np.float32)


STEP_SHAPES = [(128, 63), (116, 32),  # KS = 8 (dim > 112), NB = 2 / 1
               (112, 33),             # the last KS = 7 dim, the last dim of the lock-step kernel
               (104, 50), (108, 50),  # nq = 13 / 14: the two instantiations of the exact kernel
               (124, 64),             # k (dim + 1) = 8000 of 8192: the LDS limit
               (8, 2), (4, 64), (100, 1)]
STEP_PATHS = {
    "bf16": {"SPLIT": "1", "H16": "0", "BOUNDS": "0"},
    "bf16_bounds": {"H16": "0", "BOUNDS": "1"},
    "h16": {"H16": "1", "BOUNDS": "0"},
    "h16_bounds": {"H16": "1", "BOUNDS": "1", "MV": "0"},
    "h16_moves": {"H16": "1", "MV": "1", "S16": "0"},
    "defaults": {},
    "lockstep": {"GROUP": "4"},  # 32 < k <= 64 and dim <= 112 only
}
_EXACT_FITS = {}


def _fit(monkeypatch, X, k, env):
    from otto_recommender_amd import popularity as gp
    _set_env(monkeypatch, {"GROUP": "1", **env})
    km = gp.KMeans(n_clusters=k, random_state=42, n_init=2).fit(X)
    return km.labels_.cpu().numpy(), km.cluster_centers_.cpu().numpy(), km.inertia_, km.n_iter_


def _exact_fit(monkeypatch, dim, k):
    if (dim, k) not in _EXACT_FITS:
        _EXACT_FITS[(dim, k)] = _fit(monkeypatch, _blobs(dim, k), k, {"SPLIT": "0"})
    return _EXACT_FITS[(dim, k)]


STEP_CASES = [(dim, k, path) for dim, k in STEP_SHAPES for path in STEP_PATHS
              if path != "lockstep" or (32 < k <= 64 and dim <= 112)]  # what the lock-step kernel takes


@pytest.mark.parametrize("dim,k,path", STEP_CASES)
def test_step_paths_equal_exact_steps(gpu, monkeypatch, dim, k, path):
    """KMeans.fit through each E-step path gives the exact f32 steps' (OTTOHIP_KM_SPLIT=0) labels, centres,
    inertia and iterations bit for bit."""
    base = _exact_fit(monkeypatch, dim, k)
    got = _fit(monkeypatch, _blobs(dim, k), k, STEP_PATHS[path])
    np.testing.assert_array_equal(got[0], base[0])
    np.testing.assert_array_equal(got[1], base[1])
    assert got[2] == base[2] and got[3] == base[3]


@pytest.mark.parametrize("dim,k", STEP_SHAPES + [(30, 9), (101, 17)])
def test_exact_steps_match_restatement(gpu, monkeypatch, dim, k):
    """The exact steps against the float64 restatement of sklearn 1.2 (oracle/popularity.py) with the tolerances
    of tests/test_popularity_gpu.py; dim 30 and 101 take the VALU kernel through ottohip_kmeans_lloyd_iter."""
    _set_env(monkeypatch, {"GROUP": "1", "SPLIT": "0"})
    _check_kmeans(_blobs(dim, k), k, n_init=2)


def test_valu_steps_empty_cluster_relocation(gpu, monkeypatch):
    """A third of the rows identical at dim 30 (VALU kernel, lloyd_iter): empty clusters relocated; the figures
    of test_kmeans_empty_cluster_relocation."""
    _set_env(monkeypatch, {})
    rng = np.random.default_rng(77)
    centers = rng.normal(scale=3, size=(9, 30))
    X = (centers[rng.integers(0, 9, 6007)] + rng.normal(size=(6007, 30))).astype(np.float32)
    X[:2000] = X[0]
    _check_kmeans(X, 12, agree=0.995, rel=1e-4)


# ---------------------------------------------------------------- C. near-tie lists past their LDS capacity

KMS_AMB, KMH_AMB = 1024, 8192  # mirror csrc/popularity.hip KMS_AMB / KMH_AMB: near-tie rows a block stages in LDS
TIE_PATHS = {  # E-step path: (LDS capacity, f16 rows attached, environment)
    "bf16": (KMS_AMB, False, {"H16": "0", "BOUNDS": "0"}),
    "bf16_bounds": (KMS_AMB, False, {"H16": "0", "BOUNDS": "1"}),
    "h16_bounds": (KMH_AMB, True, {"MV": "0"}),
    "h16_split16": (KMH_AMB, True, {}),
}
_TIE_ROWS = {}
_TIE_EXACT = {}


def _tie_rows(amb):
    """n = n_cu * amb * 5 / 4 + 77 rows of dim 4: with one block per CU at least one block (every block, the
    tiles going round-robin) meets more than `amb` rows. (X numpy, X device, rint(x 2^24) int64)."""
    if amb not in _TIE_ROWS:
        n = _n_cu() * amb * 5 // 4 + 77
        X = np.random.default_rng(amb).normal(size=(n, 4)).astype(np.float32)
        _TIE_ROWS[amb] = (X, _dev(X), np.rint(X.astype(np.float64) * ke.FX).astype(np.int64))
    return _TIE_ROWS[amb]


def _two_centres(kind):
    c0 = np.random.default_rng(5).normal(size=4).astype(np.float32)
    c1 = c0.copy()
    if kind == "close":
        c1[0] += np.float32(2.0 ** -12)
        assert c1[0] != c0[0]
    return np.stack([c0, c1])


def _lloyd_steps(gpu, Xd, C, max_steps):
    """ottohip_kmeans_lloyd_steps from labels -1: (labels, centres, sums [k, dim], counts, out[0..5])."""
    import torch
    from otto_recommender_amd import _lib
    n, dim = Xd.shape
    k = C.shape[0]
    Cd = _dev(C)
    labels = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    sums = torch.zeros(k * dim, dtype=torch.int64, device="cuda")
    counts = torch.zeros(k, dtype=torch.int64, device="cuda")
    out = (ctypes.c_double * 6)()
    _lib.check(_lib.load().ottohip_kmeans_lloyd_steps(gpu.h, _lib.ptr(Xd), n, dim, _lib.ptr(Cd), k, _lib.ptr(labels),
                                                      _lib.ptr(sums), _lib.ptr(counts), max_steps, 0.0, out,
                                                      _lib.stream_handle()))
    torch.cuda.synchronize()
    return labels.cpu().numpy(), Cd.cpu().numpy(), sums.cpu().numpy().reshape(k, dim), counts.cpu().numpy(), list(out)


def _two_cluster_sums(fx, labels):
    s1 = fx[labels == 1].sum(0)
    return np.stack([fx.sum(0) - s1, s1]), np.array([np.sum(labels == 0), np.sum(labels == 1)], np.int64)


@pytest.mark.parametrize("centres", ["identical", "close"])
@pytest.mark.parametrize("path", list(TIE_PATHS))
def test_near_tie_lists_past_lds_capacity(gpu, monkeypatch, path, centres):
    """More near-tie rows per block than the split passes stage in LDS (k_km_assign_split, k_km_split16): the
    rows past the capacity go to the global list one by one, and none is lost or scored twice.
    identical: two equal centres, every row is a tie: all labels 0, the sums are the exact column sums, the step
    stops on the empty cluster with the centres untouched. close: c_1 = c_0 + 2^-12 e_0, three steps (the first
    almost all near ties, the others ordinary): bit-identical to the exact steps (OTTOHIP_KM_SPLIT=0)."""
    from otto_recommender_amd import _lib
    amb, half, env = TIE_PATHS[path]
    X, Xd, fx = _tie_rows(amb)
    n = X.shape[0]
    assert n > _n_cu() * amb
    C = _two_centres(centres)
    steps = 1 if centres == "identical" else 3
    if (amb, centres) not in _TIE_EXACT:
        _set_env(monkeypatch, {"SPLIT": "0"})
        _TIE_EXACT[(amb, centres)] = _lloyd_steps(gpu, Xd, C, steps)
    base = _TIE_EXACT[(amb, centres)]
    _set_env(monkeypatch, env)
    lib = _lib.load()
    if half:
        _lib.check(lib.ottohip_kmeans_attach_half(gpu.h, _lib.ptr(Xd), n, 4, _lib.stream_handle()))
    try:
        labels, Cn, sums, counts, out = _lloyd_steps(gpu, Xd, C, steps)
    finally:
        if half:
            lib.ottohip_kmeans_detach_half(gpu.h)
    rs, rc = _two_cluster_sums(fx, labels)
    np.testing.assert_array_equal(counts, rc)
    np.testing.assert_array_equal(sums, rs)
    if centres == "identical":
        assert not labels.any()
        assert counts.tolist() == [n, 0]
        np.testing.assert_array_equal(sums[0], fx.sum(0))
        assert out[1] == n and out[3] == 1 and out[4] == 1 and out[5] == 3, out
        np.testing.assert_array_equal(Cn, C)
    else:
        assert out[4] == 3 and out[5] == 0 and counts.min() > 0, (out, counts)
    np.testing.assert_array_equal(labels, base[0])
    np.testing.assert_array_equal(Cn, base[1])
    np.testing.assert_array_equal(sums, base[2])
    np.testing.assert_array_equal(counts, base[3])
    assert out[1:] == base[4][1:], (out, base[4])


# ---------------------------------------------------------------- D. the small kernels

SMALL_DIMS = (1, 3, 100, 127, 128)


def _small_rows(n, dim, seed=0):
    return (np.random.default_rng(1000 * dim + n + seed).normal(size=(n, dim)) * 2 + 0.5).astype(np.float32)


@pytest.mark.parametrize("center", [False, True])
@pytest.mark.parametrize("dim", SMALL_DIMS)
def test_col_sums_exact(gpu, dim, center):
    """sum_x[d] = sum rint(x 2^24), sum_sq[d] = sum rint(fl32(t t) 2^24) with t = fl32(x - c): exact."""
    import torch
    from otto_recommender_amd import _lib
    for n in (0, 1, _n_cu() * 16 + 5):
        X = _small_rows(n, dim)
        c = np.random.default_rng(dim).normal(size=dim).astype(np.float32) if center else np.zeros(dim, np.float32)
        Xd, cd = _dev(X), _dev(c)
        s1 = torch.full((dim,), 3, dtype=torch.int64, device="cuda")
        s2 = torch.full((dim,), 3, dtype=torch.int64, device="cuda")
        _lib.check(_lib.load().ottohip_col_sums(gpu.h, _lib.ptr(Xd) if n else None, n, dim,
                                                _lib.ptr(cd) if center else None, _lib.ptr(s1), _lib.ptr(s2),
                                                _lib.stream_handle()))
        t = X - c[None, :]
        q = t * t
        assert t.dtype == np.float32 and q.dtype == np.float32
        np.testing.assert_array_equal(s1.cpu().numpy(), np.rint(X.astype(np.float64) * ke.FX).astype(np.int64).sum(0))
        np.testing.assert_array_equal(s2.cpu().numpy(), np.rint(q.astype(np.float64) * ke.FX).astype(np.int64).sum(0))


@pytest.mark.parametrize("dim", SMALL_DIMS)
def test_center_rows_exact(gpu, dim):
    import torch
    from otto_recommender_amd import _lib
    for n in (0, 1, _n_cu() * 16 + 5):
        X = _small_rows(n, dim)
        mean = np.random.default_rng(dim).normal(size=dim).astype(np.float32)
        Xd, md = _dev(X), _dev(mean)
        out = torch.full((max(n, 1), dim), 9.0, dtype=torch.float32, device="cuda")
        _lib.check(_lib.load().ottohip_center_rows(gpu.h, _lib.ptr(Xd) if n else None, n, dim, _lib.ptr(md),
                                                   _lib.ptr(out), _lib.stream_handle()))
        got = out.cpu().numpy()
        np.testing.assert_array_equal(got[:n].view(np.uint32), (X - mean[None, :]).view(np.uint32))
        assert n > 0 or np.all(got == 9.0)


@pytest.mark.parametrize("k", [1, 64])
@pytest.mark.parametrize("dim", SMALL_DIMS)
def test_update_exact(gpu, dim, k):
    """centres = float32(float64(sum) / 2^24 / count), empty clusters keep theirs; shift^2 to rel 1e-12 (one
    float64 sum of k dim <= 8192 squares in another order: 8192 2^-53 = 9e-13)."""
    from otto_recommender_amd import _lib
    rng = np.random.default_rng(100 * dim + k)
    n = 3000
    X = _small_rows(n, dim)
    labels = rng.integers(0, k, n)
    if k > 1:
        labels[np.isin(labels, (0, 17, k - 1))] = 5  # three empty clusters
    sums, counts = ke.fixed_sums(X, labels, k)
    C = rng.normal(size=(k, dim)).astype(np.float32)
    Cd, sd, cd = _dev(C), _dev(sums), _dev(counts)
    shift = ctypes.c_double()
    _lib.check(_lib.load().ottohip_kmeans_update(gpu.h, _lib.ptr(Cd), _lib.ptr(sd), _lib.ptr(cd), k, dim,
                                                 ctypes.byref(shift), _lib.stream_handle()))
    ref = C.copy()
    nz = counts > 0
    ref[nz] = (sums[nz].astype(np.float64) / ke.FX / counts[nz, None].astype(np.float64)).astype(np.float32)
    np.testing.assert_array_equal(Cd.cpu().numpy().view(np.uint32), ref.view(np.uint32))
    assert k == 1 or (~nz).sum() == 3
    sh = float(((ref.astype(np.float64) - C.astype(np.float64)) ** 2).sum())
    assert abs(shift.value - sh) <= 1e-12 * sh, (shift.value, sh)


def test_relocate_exact(gpu):
    """Several moves, two of them out of one cluster, against int64 arithmetic; an index outside [0, k) is
    refused (ERANGE) and nothing is written."""
    from otto_recommender_amd import _lib
    lib = _lib.load()
    for dim in SMALL_DIMS:
        k, n = 8, 500
        rng = np.random.default_rng(dim)
        X = _small_rows(n, dim)
        labels = rng.integers(0, 5, n)  # clusters 5, 6, 7 empty
        sums, counts = ke.fixed_sums(X, labels, k)
        rows = np.concatenate([np.flatnonzero(labels == 0)[:2], np.flatnonzero(labels == 3)[:1]])
        moves = np.array([[0, 5], [0, 6], [3, 7]], np.int32)
        rs, rc = sums.copy(), counts.copy()
        fx = np.rint(X[rows].astype(np.float64) * ke.FX).astype(np.int64)
        for j, (oc, nc) in enumerate(moves):
            rs[oc] -= fx[j]
            rs[nc] = fx[j]
            rc[oc] -= 1
            rc[nc] = 1
        sd, cd, vd = _dev(sums), _dev(counts), _dev(X[rows])
        mv = (ctypes.c_int32 * 6)(*moves.ravel().tolist())
        bad = (ctypes.c_int32 * 6)(0, 5, 0, k, 3, 7)
        neg = (ctypes.c_int32 * 6)(0, 5, -1, 6, 3, 7)
        for b in (bad, neg):
            rc_ = lib.ottohip_kmeans_relocate(gpu.h, _lib.ptr(sd), _lib.ptr(cd), k, dim, _lib.ptr(vd), b, 3,
                                              _lib.stream_handle())
            assert rc_ == OTTOHIP_ERANGE and b"relocate" in lib.ottohip_last_error()
            np.testing.assert_array_equal(sd.cpu().numpy(), sums)
            np.testing.assert_array_equal(cd.cpu().numpy(), counts)
        _lib.check(lib.ottohip_kmeans_relocate(gpu.h, _lib.ptr(sd), _lib.ptr(cd), k, dim, _lib.ptr(vd), mv, 3,
                                               _lib.stream_handle()))
        np.testing.assert_array_equal(sd.cpu().numpy(), rs)
        np.testing.assert_array_equal(cd.cpu().numpy(), rc)


def _farthest(gpu, Xd, Cd, ld, n, dim, m):
    from otto_recommender_amd import _lib
    rows = (ctypes.c_int64 * max(m, 1))(*([7] * max(m, 1)))
    d2 = (ctypes.c_float * max(m, 1))(*([7.0] * max(m, 1)))
    _lib.check(_lib.load().ottohip_kmeans_farthest(gpu.h, _lib.ptr(Xd) if n else None, n, dim, _lib.ptr(Cd),
                                                   _lib.ptr(ld) if n else None, m, rows, d2, _lib.stream_handle()))
    return np.array(rows[:], np.int64), np.array(d2[:], np.float32)


@pytest.mark.parametrize("dim", SMALL_DIMS)
def test_farthest_rows(gpu, dim):
    """The m rows farthest from their labelled centre: each distance within 128 2^-24 (relative) of float64,
    descending, no row that float64 puts clearly behind the m-th; equal distances (identical rows) by row."""
    REL = 128 * 2.0 ** -24
    k, m = 6, 9
    n = _n_cu() * 16 + 5
    rng = np.random.default_rng(dim + 40)
    X = _small_rows(n, dim)
    C = rng.normal(size=(k, dim)).astype(np.float32)
    labels = rng.integers(0, k, n).astype(np.int32)
    far = np.sort(rng.permutation(n)[:3])  # three identical rows, the farthest of all
    X[far] = C[2] + np.float32(40.0)
    labels[far] = 2
    Xd, Cd, ld = _dev(X), _dev(C), _dev(labels)
    rows, d2 = _farthest(gpu, Xd, Cd, ld, n, dim, m)
    d64 = ((X.astype(np.float64) - C.astype(np.float64)[labels]) ** 2).sum(1)
    np.testing.assert_array_equal(rows[:3], far)
    assert d2[0] == d2[1] == d2[2]
    assert len(set(rows.tolist())) == m and rows.min() >= 0 and rows.max() < n
    assert np.all(np.diff(d2) <= 0)
    assert np.all(np.abs(d2.astype(np.float64) - d64[rows]) <= REL * d64[rows]), (d2, d64[rows])
    mth = np.sort(d64)[-m]
    assert np.all(d64[rows] >= mth * (1 - 2 * REL))
    # more rows asked for than there are; none asked for
    rows, d2 = _farthest(gpu, Xd, Cd, ld, 3, dim, 5)
    assert rows[3:].tolist() == [-1, -1] and d2[3:].tolist() == [-1.0, -1.0]
    assert sorted(rows[:3].tolist()) == [0, 1, 2]
    rows, d2 = _farthest(gpu, Xd, Cd, ld, n, dim, 0)
    assert rows.tolist() == [7] and d2.tolist() == [7.0]
    rows, d2 = _farthest(gpu, None, Cd, None, 0, dim, 2)
    assert rows.tolist() == [-1, -1]


@pytest.mark.parametrize("dim", SMALL_DIMS)
def test_inertia_of_given_labels(gpu, dim):
    """Within rel 1e-6 of float64 (per row an f32 sum of at most 128 squares: 128 2^-24 = 7.6e-6 at worst, the
    rows' errors independent; accumulated in float64); the same bits on a second call."""
    from otto_recommender_amd import _lib
    k = 7
    for n in (0, 1, _n_cu() * 16 + 5):
        rng = np.random.default_rng(dim + n)
        X = _small_rows(n, dim)
        C = rng.normal(size=(k, dim)).astype(np.float32)
        labels = rng.integers(0, k, n).astype(np.int32)
        Xd, Cd, ld = _dev(X), _dev(C), _dev(labels)
        got = []
        for _ in range(2):
            inr = ctypes.c_double(-1.0)
            _lib.check(_lib.load().ottohip_kmeans_inertia(gpu.h, _lib.ptr(Xd) if n else None, n, dim, _lib.ptr(Cd),
                                                          _lib.ptr(ld) if n else None, ctypes.byref(inr),
                                                          _lib.stream_handle()))
            got.append(inr.value)
        ref = float(((X.astype(np.float64) - C.astype(np.float64)[labels]) ** 2).sum())
        assert got[0] == got[1]
        assert abs(got[0] - ref) <= 1e-6 * ref, (got[0], ref)


# ---------------------------------------------------------------- E. limits

def _estep_calls(gpu, n, dim, k):
    """partial, lloyd_iter and lloyd_steps on buffers of the full size: [(name, return code, last error)]."""
    import torch
    from otto_recommender_amd import _lib
    lib = _lib.load()
    Xd = torch.zeros((n, dim), dtype=torch.float32, device="cuda")
    Cd = torch.zeros((k, dim), dtype=torch.float32, device="cuda")
    labels = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    sums = torch.zeros(k * dim, dtype=torch.int64, device="cuda")
    counts = torch.zeros(k, dtype=torch.int64, device="cuda")
    inr, chg = ctypes.c_double(), ctypes.c_int64()
    out = (ctypes.c_double * 6)()
    sh = _lib.stream_handle()
    a = (gpu.h, _lib.ptr(Xd), n, dim, _lib.ptr(Cd), k, _lib.ptr(labels), _lib.ptr(sums), _lib.ptr(counts))
    res = []
    for name, call in (("kmeans_partial", lambda: lib.ottohip_kmeans_partial(*a, ctypes.byref(inr), ctypes.byref(chg), sh)),
                       ("kmeans_lloyd_iter", lambda: lib.ottohip_kmeans_lloyd_iter(*a, out, sh)),
                       ("kmeans_lloyd_steps", lambda: lib.ottohip_kmeans_lloyd_steps(*a, 2, 0.0, out, sh))):
        rc = call()
        res.append((name, rc, lib.ottohip_last_error()))
    torch.cuda.synchronize()
    assert torch.all(labels == -1) and not sums.any() and not counts.any()  # refused before any launch
    return res


@pytest.mark.parametrize("dim,k,code", [(100, 65, OTTOHIP_EINVAL), (129, 9, OTTOHIP_EINVAL), (128, 64, OTTOHIP_ELIMIT)])
def test_estep_limits(gpu, dim, k, code):
    """k <= 64 and dim <= 128 (EINVAL), k (dim + 1) <= 8192 (ELIMIT: the per-block sums in LDS)."""
    for name, rc, msg in _estep_calls(gpu, 64, dim, k):
        assert rc == code, (name, rc)
        assert name.encode() in msg, (name, msg)


def test_attach_half_and_fit_limits(gpu):
    import torch
    from otto_recommender_amd import _lib, popularity as gp
    lib = _lib.load()
    Xd = torch.zeros((64, 30), dtype=torch.float32, device="cuda")
    assert lib.ottohip_kmeans_attach_half(gpu.h, _lib.ptr(Xd), 64, 30, _lib.stream_handle()) == OTTOHIP_EINVAL
    assert b"kmeans_attach_half" in lib.ottohip_last_error()
    with pytest.raises(ValueError):
        gp.KMeans(n_clusters=9, n_init=1).fit(np.zeros((8, 4), np.float32))
