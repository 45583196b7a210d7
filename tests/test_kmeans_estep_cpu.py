"""The float64 checkers of tests/kmeans_estep.py must be able to fail: numpy stand-ins of the KMeans E-step
(no GPU). A float32 restatement passes every check; an E-step that is subtly wrong (a centre column lost, the
last four dims dropped, centres rounded to bf16, ties to the highest index, a row missing from the sums) is
rejected. The fixtures' validity (at most 1 % of the rows undecidable) is asserted here for every shape the GPU
test uses, so it does not rest on a GPU run."""
import numpy as np
import pytest

import kmeans_estep as ke

STANDIN_SHAPES = [(100, 50), (128, 63), (8, 9)]


seed_of = ke.fixture_seed


def estep_f32(X, C, Cs=None, last=False):
    """One E-step in float32 as the kernels state it: labels = argmin |c|^2 - 2 x.c (ties to the lowest index,
    `last`: to the highest), fixed-point sums and counts under those labels, inertia = sum max(|x|^2 + s, 0).
    Cs: the centres the scores are computed from (a wrong kernel's view of C)."""
    Cs = C if Cs is None else Cs
    k = C.shape[0]
    s = (Cs * Cs).sum(1, dtype=np.float32)[None, :] - np.float32(2) * (X[:, :Cs.shape[1]] @ Cs.T)
    assert s.dtype == np.float32
    lab = k - 1 - s[:, ::-1].argmin(1) if last else s.argmin(1)
    xn = (X * X).sum(1, dtype=np.float32)
    inertia = float(np.maximum(xn + s[np.arange(len(lab)), lab], np.float32(0)).astype(np.float64).sum())
    sums, counts = ke.fixed_sums(X, lab, k)
    return lab.astype(np.int32), sums, counts, inertia


def bf16(a):
    u = a.view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) >> 16 << 16
    return u.astype(np.uint32).view(np.float32)


@pytest.mark.parametrize("dim,k", STANDIN_SHAPES)
def test_float32_restatement_passes(dim, k):
    X, C = ke.boundary_fixture(dim, k, ke.N_ROWS, seed_of(dim, k))
    lab, sums, counts, inertia = estep_f32(X, C)
    st = ke.check_labels(X, C, lab)
    assert st["wrong"] == 0 and st["worst"] < 1.0
    ke.check_sums(X, lab, sums, counts, k)
    assert ke.check_inertia(X, C, lab, inertia) < 1.0
    for lin in ke.label_inputs(st["ref"], k, 3):
        ke.check_changed(lin, lab, int(np.sum(lin != lab)))
    Xt, Ct, dup_hi, dup_rows = ke.tie_fixture(dim, k, ke.N_ROWS, seed_of(dim, k) + 7)
    ke.check_ties(Xt, Ct, estep_f32(Xt, Ct)[0], dup_hi, dup_rows)


@pytest.mark.parametrize("dim,k", STANDIN_SHAPES)
@pytest.mark.parametrize("fault", ["column_zeroed", "last_4_dims_dropped", "bf16_centres"])
def test_wrong_scores_are_rejected(dim, k, fault):
    X, C = ke.boundary_fixture(dim, k, ke.N_ROWS, seed_of(dim, k))
    if fault == "column_zeroed":
        Cs = C.copy()
        Cs[:, dim // 2] = 0
    elif fault == "last_4_dims_dropped":
        Cs = np.ascontiguousarray(C[:, :dim - 4])
    else:
        Cs = bf16(C)
    lab = estep_f32(X, C, Cs)[0]
    st = ke.label_stats(X, C, lab)
    assert st["wrong"] >= 50, st  # far from a borderline rejection
    with pytest.raises(AssertionError):
        ke.check_labels(X, C, lab)


@pytest.mark.parametrize("dim,k", STANDIN_SHAPES)
def test_ties_to_the_highest_index_are_rejected(dim, k):
    X, C, dup_hi, dup_rows = ke.tie_fixture(dim, k, ke.N_ROWS, seed_of(dim, k) + 7)
    lab = estep_f32(X, C, last=True)[0]
    assert np.isin(lab, dup_hi).sum() >= 50
    with pytest.raises(AssertionError):
        ke.check_ties(X, C, lab, dup_hi, dup_rows)


@pytest.mark.parametrize("dim,k", STANDIN_SHAPES)
def test_a_row_missing_from_the_sums_is_rejected(dim, k):
    X, C = ke.boundary_fixture(dim, k, ke.N_ROWS, seed_of(dim, k))
    lab, sums, counts, inertia = estep_f32(X, C)
    s2, c2 = ke.fixed_sums(X[1:], lab[1:], k)
    with pytest.raises(AssertionError):
        ke.check_sums(X, lab, s2, c2, k)
    with pytest.raises(AssertionError):  # the counts right, one row's vector lost
        ke.check_sums(X, lab, s2, counts, k)
    with pytest.raises(AssertionError):
        ke.check_changed(np.full(len(lab), -1), lab, len(lab) - 1)
    with pytest.raises(AssertionError):  # one row's distance counted twice
        ke.check_inertia(X, C, lab, inertia * (1 + 2.0 / len(lab)))


def test_fixtures_keep_the_undecidable_cap():
    """Every fixture of tests/test_kmeans_shapes_gpu.py: at most 1 % of the rows within 2 e(x) of a tie (the
    float64 labels themselves pass every label check), and an E-step that loses one centre column mislabels at
    least 50 decidable rows at every shape with k > 1 (the fewest: 337 at dim 124, k 2)."""
    cases = [(dim, k, ke.N_ROWS) for dim, k in ke.shapes()] + [(100, 9, n) for n in ke.SMALL_N]
    assert len(ke.shapes()) == 113
    for dim, k, n in cases:
        X, C = ke.boundary_fixture(dim, k, n, seed_of(dim, k, n))
        ref = ke.ref_scores(X, C).argmin(1)
        st = ke.check_labels(X, C, ref)
        assert st["worst"] == 0.0
        if k >= 2 and n == ke.N_ROWS:  # the fixture sees a lost centre column at every shape, not only the three above
            Cs = C.copy()
            Cs[:, dim // 2] = 0
            assert ke.label_stats(X, C, estep_f32(X, C, Cs)[0])["wrong"] >= 50, (dim, k)
        if k >= 2:
            Xt, Ct, dup_hi, dup_rows = ke.tie_fixture(dim, k, n, seed_of(dim, k, n) + 7)
            s = ke.ref_scores(Xt, Ct)
            s[:, list(dup_hi)] = np.inf
            ke.check_ties(Xt, Ct, s.argmin(1), dup_hi, dup_rows)
