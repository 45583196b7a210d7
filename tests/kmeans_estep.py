"""Float64 checks of one KMeans E-step (csrc/popularity.hip, stage C2): fixtures and checkers, numpy only.

The exact f32 E-step (k_km_assign_mfma, k_km_assign) scores s_j = |c_j|^2 - 2 x.c_j. The comment above
KMB_SKIP states its error: every score is within e(x) = 2e-5 cmax (|x| + cmax) of the real value, cmax = max_j
|c_j|; the distance-bound filter relies on it. Everything here is derived from that one statement:
  - a row whose two smallest float64 scores differ by more than 2 e(x) is *decidable*: two scores, each off by
    at most e(x), cannot swap, so its label must be the float64 argmin;
  - any other row's label j must still satisfy s_j - min s <= 2 e(x);
  - among exactly equal scores (duplicated centres) the lowest index wins.
The fixture puts half of its rows next to decision boundaries, where a wrong or missing term of the dot
product changes the label; on well-separated blobs alone it would not. The checkers are plain functions so
that tests/test_kmeans_estep_cpu.py can show, without a GPU, that they reject subtly wrong E-steps."""
import numpy as np

FX = float(1 << 24)  # fixed-point scale of the device sums (csrc/popularity.hip KM_FX)
SCORE_ERR = 2e-5     # e(x) = SCORE_ERR * cmax * (|x| + cmax): the comment above KMB_SKIP
UNDECIDABLE_CAP = 0.01  # a fixture whose rows are mostly undecidable checks nothing: at most 1 % may be

N_ROWS = 4129  # no multiple of 32 (MFMA tile), 64 (wave) or 256 (VALU block)
MFMA_DIMS = (4, 8, 52, 100, 104, 108, 112, 116, 124, 128)  # dim % 4 == 0: nq 13 / 14..16, KS 7 / 8
VALU_DIMS = (1, 3, 30, 101, 127)                           # dim % 4 != 0: k_km_assign<8q>
K_VALUES = (1, 2, 8, 9, 32, 33, 63, 64)                    # every KP = 8q of the VALU kernel, NB = 1 / 2
SMALL_N = (1, 31, 32, 33, 9)                               # at dim 100, k 9 (the last one is n = k)


def shapes():
    """(dim, k) of part A: every pair within the LDS limit k (dim + 1) <= 8192; dim 1 with k in {2, 8} only
    (with k >= 32 centres on a line more than 1 % of the rows are undecidable)."""
    out = []
    for dim in MFMA_DIMS + VALU_DIMS:
        for k in K_VALUES:
            if dim == 1 and k not in (2, 8):
                continue
            if k * (dim + 1) > 8192:
                continue
            out.append((dim, k))
    return out


def fixture_seed(dim, k, n=N_ROWS):
    """One seed per case, shared by the CPU test of the fixtures and the GPU test that uses them."""
    return 100_000 * n + 100 * dim + k


def _norm(a):
    return np.sqrt((a * a).sum(axis=-1))


def err_bound(X, C):
    """e(x) per row, float64."""
    cmax = _norm(C.astype(np.float64)).max()
    return SCORE_ERR * cmax * (_norm(X.astype(np.float64)) + cmax)


def ref_scores(X, C):
    """s_j = |c_j|^2 - 2 x.c_j in float64 from the float32 inputs: [n, k]."""
    X64, C64 = X.astype(np.float64), C.astype(np.float64)
    return (C64 * C64).sum(1)[None, :] - 2.0 * (X64 @ C64.T)


def _rows(C, distinct, n, rng):
    """n rows for the centres C (float32): the first n - n // 2 are blob rows C[j] + normal (j over every
    centre), the others lie near the bisecting hyperplane of a random pair (a, b) of `distinct` centres:
    x = (c_a + c_b) / 2 + w + tau d_hat with w normal and orthogonal to d_hat = (c_a - c_b) / |c_a - c_b| and
    2 |tau| |c_a - c_b|, the float64 score gap of a and b, log-uniform in [2, 1000] times 2 e(x). Without w every
    dimension's share of the gap vanishes at the midpoint and a kernel that drops one would pass. Shuffled, so
    every tile holds both kinds."""
    k, dim = C.shape
    C64 = C.astype(np.float64)
    cmax = _norm(C64).max()
    nb = n // 2 if len(distinct) >= 2 else 0
    X = np.empty((n, dim))
    X[:n - nb] = C64[rng.integers(0, k, n - nb)] + rng.normal(size=(n - nb, dim))
    if nb:
        distinct = np.asarray(distinct)
        ia = rng.integers(0, len(distinct), nb)
        ib = (ia + rng.integers(1, len(distinct), nb)) % len(distinct)
        a, b = distinct[ia], distinct[ib]
        d = C64[a] - C64[b]
        dn = _norm(d)
        dh = d / dn[:, None]
        w = rng.normal(size=(nb, dim))
        w -= (w * dh).sum(1)[:, None] * dh
        x0 = (C64[a] + C64[b]) / 2 + w
        ratio = np.exp(rng.uniform(np.log(2.0), np.log(1000.0), nb))
        sign = np.where(rng.random(nb) < 0.5, -1.0, 1.0)
        tau = sign * ratio * 2.0 * SCORE_ERR * cmax * (_norm(x0) + cmax) / (2.0 * dn)
        X[n - nb:] = x0 + tau[:, None] * dh
    return X[rng.permutation(n)].astype(np.float32)


def boundary_fixture(dim, k, n, seed):
    """(X [n, dim] f32, C [k, dim] f32): C = normal, half blob rows and (k >= 2) half boundary rows (_rows)."""
    rng = np.random.default_rng(seed)
    C = rng.normal(size=(k, dim)).astype(np.float32)
    return _rows(C, np.arange(k), n, rng), C


def tie_fixture(dim, k, n, seed):
    """boundary_fixture with exact ties planted (k >= 2): one or two centres are copies of a lower-indexed one
    (their scores are equal in float64 and, computed alike, in the kernel), blob rows sit around the copies as
    around every centre, and a few rows are copies of other rows. Returns (X, C, dup_hi, dup_rows): dup_hi the
    indices of the copies (no row may get them), dup_rows [m, 2] pairs of identical rows."""
    rng = np.random.default_rng(seed)
    C = rng.normal(size=(k, dim)).astype(np.float32)
    pairs = [(0, k - 1)] if k < 4 else [(0, k - 1), (1, k // 2)]
    for lo, hi in pairs:
        C[hi] = C[lo]
    dup_hi = tuple(hi for _, hi in pairs)
    X = _rows(C, np.setdiff1d(np.arange(k), dup_hi), n, rng)
    m = min(8, n // 2)
    dup_rows = rng.permutation(n)[:2 * m].reshape(m, 2)
    X[dup_rows[:, 1]] = X[dup_rows[:, 0]]
    return X, C, dup_hi, dup_rows


def label_stats(X, C, labels, dup_hi=()):
    """The float64 comparison of an E-step's labels; dup_hi: centres that are copies of a lower index (their
    scores are left out: the lowest index must win). Returns a dict:
      ref          float64 argmin (lowest index among equals)
      undecidable  share of rows whose two smallest scores are within 2 e(x)
      wrong        decidable rows whose label is not the float64 argmin
      excess       rows (of any kind) whose label's score exceeds the minimum by more than 2 e(x)
      worst        max over rows of (s_label - min s) / (2 e(x))
      tightest     min over the rows labelled as float64 labels them of gap / (2 e(x)): how close a tie the
                   E-step still resolved as float64 does (a measurement, nothing is asserted on it)"""
    labels = np.asarray(labels).astype(np.int64)
    n, k = X.shape[0], C.shape[0]
    assert labels.shape == (n,)
    assert n == 0 or (labels.min() >= 0 and labels.max() < k), (labels.min(), labels.max())
    s = ref_scores(X, C)
    if len(dup_hi):
        s[:, list(dup_hi)] = np.inf
    e2 = 2.0 * err_bound(X, C)
    ref = s.argmin(1)
    smin = s.min(1) if n else np.zeros(0)
    gap = np.partition(s, 1, axis=1)[:, 1] - smin if k - len(dup_hi) >= 2 else np.full(n, np.inf)
    decidable = gap > e2
    over = s[np.arange(n), labels] - smin
    same = labels == ref
    return {"ref": ref, "tightest": float((gap[same] / e2[same]).min()) if same.any() else np.inf, "undecidable": float(np.mean(~decidable)) if n else 0.0,
            "wrong": int(np.sum(decidable & (labels != ref))), "excess": int(np.sum(over > e2)),
            "worst": float((over / e2).max()) if n else 0.0}


def check_labels(X, C, labels, dup_hi=()):
    """Asserts the fixture's cap and both label conditions; returns label_stats."""
    st = label_stats(X, C, labels, dup_hi)
    assert st["undecidable"] <= UNDECIDABLE_CAP, f"fixture: {st['undecidable']:.4f} of the rows undecidable"
    assert st["wrong"] == 0, f"{st['wrong']} decidable rows off the float64 argmin (worst ratio {st['worst']:.3g})"
    assert st["excess"] == 0, f"{st['excess']} labels more than 2 e(x) above the minimum ({st['worst']:.3g})"
    return st


def check_ties(X, C, labels, dup_hi, dup_rows):
    """Equal scores go to the lowest index, identical rows get one label, and check_labels holds."""
    labels = np.asarray(labels)
    n_hi = int(np.isin(labels, dup_hi).sum())
    assert n_hi == 0, f"{n_hi} rows labelled with the higher index of two equal centres"
    np.testing.assert_array_equal(labels[dup_rows[:, 0]], labels[dup_rows[:, 1]])
    return check_labels(X, C, labels, dup_hi)


def fixed_sums(X, labels, k):
    """(sums [k, dim], counts [k]) int64: sum of rint(x 2^24) and the row count per label."""
    labels = np.asarray(labels).astype(np.int64)
    fx = np.rint(X.astype(np.float64) * FX).astype(np.int64)
    sums = np.zeros((k, X.shape[1]), np.int64)
    np.add.at(sums, labels, fx)
    return sums, np.bincount(labels, minlength=k).astype(np.int64)


def check_sums(X, labels, sums, counts, k):
    """The device's fixed-point sums and counts equal those of its own labels, exactly."""
    rs, rc = fixed_sums(X, labels, k)
    np.testing.assert_array_equal(np.asarray(counts).astype(np.int64), rc)
    np.testing.assert_array_equal(np.asarray(sums).astype(np.int64).reshape(k, -1), rs)


def check_changed(labels_in, labels_out, n_changed):
    assert int(n_changed) == int(np.sum(np.asarray(labels_in) != np.asarray(labels_out))), n_changed


def check_inertia(X, C, labels, inertia):
    """|inertia - sum (|x|^2 + s_label)| <= sum e(x): every row's score is within e(x)."""
    labels = np.asarray(labels).astype(np.int64)
    X64 = X.astype(np.float64)
    ref = float(((X64 * X64).sum(1) + ref_scores(X, C)[np.arange(len(labels)), labels]).sum())
    tol = float(err_bound(X, C).sum())
    assert abs(float(inertia) - ref) <= tol, (float(inertia), ref, tol)
    return abs(float(inertia) - ref) / tol if tol else 0.0


def label_inputs(ref, k, seed):
    """The labels passed into an E-step for the n_changed check: none (-1), the float64 labels, and a copy with
    half of the rows relabelled at random."""
    rng = np.random.default_rng(seed)
    half = ref.copy()
    pick = rng.random(len(ref)) < 0.5
    half[pick] = rng.integers(0, k, int(pick.sum()))
    return [np.full(len(ref), -1, np.int32), ref.astype(np.int32), half.astype(np.int32)]
