"""A plain numpy float64 restatement of the k-means that specenh.cluster runs
(include/specenh_kmeans.h), shared by the CPU and GPU tests, with the kernel's rules:

    score    s_j = |c_j|^2 - 2 x.c_j            (|x|^2 left out), lowest j among equal scores
    update   C_new[j] = mean of cluster j;  an empty cluster keeps its previous centre, count 0
    inertia  sum_p |x_p - c_label(p)|^2 against the centres the labels were taken from
    lloyd    stop after an iteration whose labels equal the previous one's or whose centres
             moved by sum |C_new - C|^2 <= tol mean(var(X, axis=0)); then one final assignment

and the error bounds of the float32 kernels, counted from their order of operations:

    c_s(d)    = max(min(d, 32) + ceil(d / 32), ceil(d / 64) + 6) + 2     roundings of a score
    c_u(n, m) = min(m, L + S), L the slab length, S = ceil(n / L)        of a cluster sum
    c_i(n, d) = 16 + ceil(min(L, n) / 2) + ceil(S ceil(d / 32) / 256)    of the inertia

    label:   s_l - min_j s_j <= c_s eps (T_l + T_j*),  T_j = |c_j|^2 + 2 sum_i |x_i c_ji|
    sums:    |sum - sum64| <= c_u eps sum_members |x|   per entry; centres one rounding further
    inertia: |I - I64| <= c_i eps I64                   (non-negative terms only)
"""
import numpy as np

EPS = 2.0 ** -24
MAX_K, MAX_D = 256, 65536
TILE, CHUNK, SLAB = 64, 32, 1024


def _ceil(a, b):
    return -(-a // b)


def c_s(d):
    return max(min(d, CHUNK) + _ceil(d, CHUNK), _ceil(d, 64) + 6) + 2


def slab_len(n):
    L = SLAB
    while _ceil(n, L) > 1024:
        L *= 2
    return L


def c_u(n, m):
    L = slab_len(n)
    return min(int(m), L + _ceil(n, L))


def c_i(n, d):
    L = slab_len(n)
    return 16 + _ceil(min(L, n), 2) + _ceil(_ceil(n, L) * _ceil(d, 32), 256)


# ---------------------------------------------------------------- the restatement
def scores64(X, C):
    """(s, T) float64 [n, k]: the scores and their magnitudes T_j = |c_j|^2 + 2 sum |x_i c_ji|."""
    X = np.asarray(X, dtype=np.float64)
    C = np.asarray(C, dtype=np.float64)
    cn = (C * C).sum(axis=1)
    s = cn[None, :] - 2.0 * (X @ C.T)
    T = cn[None, :] + 2.0 * (np.abs(X) @ np.abs(C).T)
    return s, T


def assign64(X, C):
    """Labels int32 [n]: np.argmin takes the first of equal scores, the lowest index."""
    return np.argmin(scores64(X, C)[0], axis=1).astype(np.int32)


def update64(X, labels, C):
    """(C_new, counts, sums, inertia) in float64 for the given labels and input centres."""
    X = np.asarray(X, dtype=np.float64)
    C = np.asarray(C, dtype=np.float64)
    k = C.shape[0]
    counts = np.bincount(labels, minlength=k).astype(np.int32)
    sums = np.zeros_like(C)
    np.add.at(sums, labels, X)
    C_new = C.copy()
    full = counts > 0
    C_new[full] = sums[full] / counts[full, None]
    inertia = float(((X - C[labels]) ** 2).sum())
    return C_new, counts, sums, inertia


def abs_sums64(X, labels, k):
    """sum_members |x| per cluster and column, float64 [k, d]: the scale of the sums' bound."""
    X = np.asarray(X, dtype=np.float64)
    out = np.zeros((k, X.shape[1]))
    np.add.at(out, labels, np.abs(X))
    return out


def lloyd64(X, C0, max_iter=300, tol=1e-4):
    """(centers, labels, inertia, n_iter, history): specenh.cluster.kmeans for one item in
    float64; history holds every iteration's (labels, inertia, counts)."""
    X = np.asarray(X, dtype=np.float64)
    C = np.asarray(C0, dtype=np.float64).copy()
    thr = tol * X.var(axis=0).mean()
    prev, history, n_iter = None, [], 0
    for it in range(max_iter):
        labels = assign64(X, C)
        C_new, counts, _, inertia = update64(X, labels, C)
        history.append((labels, inertia, counts))
        shift = ((C_new - C) ** 2).sum()
        C = C_new
        n_iter = it + 1
        if (prev is not None and np.array_equal(labels, prev)) or shift <= thr:
            break
        prev = labels
    labels = assign64(X, C)
    inertia = float(((X - C[labels]) ** 2).sum())
    return C, labels, inertia, n_iter, history


# ---------------------------------------------------------------- bounds
def label_slack(X, C, labels):
    """(excess, bound, gap) float64 [n]: s_l - min_j s_j of the given labels, the bound
    c_s eps (T_l + T_j*) it must not exceed, and the oracle's gap between its best and its
    second best score (inf for k = 1)."""
    s, T = scores64(X, C)
    n, k = s.shape
    rows = np.arange(n)
    star = np.argmin(s, axis=1)
    excess = s[rows, labels] - s[rows, star]
    bound = c_s(X.shape[1]) * EPS * (T[rows, labels] + T[rows, star])
    if k == 1:
        gap = np.full(n, np.inf)
    else:
        part = np.partition(s, 1, axis=1)
        gap = part[:, 1] - part[:, 0]
    return excess, bound, gap


def margin_ok(X, C):
    """True where the oracle's gap exceeds twice the label bound of its own choice against
    the runner-up, so that a float32 argmin must agree with it."""
    s, T = scores64(X, C)
    n, k = s.shape
    if k == 1:
        return np.ones(n, dtype=bool)
    order = np.argsort(s, axis=1, kind="stable")
    rows = np.arange(n)
    gap = s[rows, order[:, 1]] - s[rows, order[:, 0]]
    worst = c_s(X.shape[1]) * EPS * (T.max(axis=1) + T[rows, order[:, 0]])
    return gap > 2.0 * worst


# ---------------------------------------------------------------- data, seeded, float32
def blobs(n, d, k, seed, dtype=np.float32):
    """(X [n, d], centres [k, d], labels [n]): k separated blobs in [-1, 1]^d. The centres are
    uniform, except that their first coordinates are a shuffled lattice of spacing delta =
    2 / k, so any two are at least delta apart whatever d; a point lies within 0.1 delta of its
    centre, so its gap between the best and the second best score is at least 0.8 delta^2.
    Cluster j gets the points j, j + k, ...: none is empty for n >= k."""
    rng = np.random.default_rng(seed)
    delta = 2.0 / k
    cent = rng.uniform(-1.0, 1.0, size=(k, d))
    cent[:, 0] = (rng.permutation(k) + 0.5) * delta - 1.0
    lab = (np.arange(n) % k).astype(np.int32)
    X = cent[lab] + rng.uniform(-1.0, 1.0, size=(n, d)) * (0.1 * delta / np.sqrt(d))
    return X.astype(dtype), cent.astype(dtype), lab


def noise(n, d, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, size=(n, d)).astype(np.float32)


def two_level_image(rows, cols, seed, lo=0.2, hi=0.8, amp=0.02):
    """(image float32 [rows, cols], mask bool): a band of `hi` pixels on a `lo` background
    plus uniform noise of amplitude `amp`; both levels occur for rows * cols >= 2."""
    rng = np.random.default_rng(seed)
    mask = rng.uniform(size=(rows, cols)) < 0.3
    mask.flat[0], mask.flat[-1] = True, False
    img = np.where(mask, hi, lo) + rng.uniform(-amp, amp, size=(rows, cols))
    return img.astype(np.float32), mask


def duplicates(n, d, seed, distinct=3):
    """n points drawn from only `distinct` different rows: exact ties between points."""
    rng = np.random.default_rng(seed)
    base = rng.uniform(-1.0, 1.0, size=(distinct, d)).astype(np.float32)
    return base[rng.integers(0, distinct, size=n)]
