"""k-means on the GPU (csrc/kmeans.hip, specenh.cluster) against the float64 restatement of
tests/kmeans_local.py, at the smallest shapes at which each mechanism can break: the 64-point
tile (n = 1, 63, 64, 65, 257, 1000), the chunks of 32 of the dot products and the 32-column
blocks of the update (d = 1, 2, 3, 31, 32, 33, 130, 1025), the 32-centre blocks and their
split over the waves (k = 1, 2, 3, 31, 32, 33, 64, 256), rows and batch items with padding
(ld = d + 4 for even d, d + 5 for odd d; the padding holds NaN), more slabs than one (n > 1024).

The bounds are include/specenh_kmeans.h's, counted from the kernels' order of operations:
c_s roundings of a score, c_u of a cluster sum, c_i of the inertia; none is fitted to results."""
import functools

import numpy as np
import pytest
import torch

import kmeans_local as kl
import specenh  # noqa: F401  (registers torch.ops.specenh.*)

pytestmark = pytest.mark.gpu
EPS = kl.EPS

# (n, d, k, batch, padded): a pruned product of the edges
CASES = (
    [(n, 3, 3, 1, n % 2 == 1) for n in (1, 63, 64, 65, 257, 1000)]
    + [(65, d, 3, 1, d % 2 == 0) for d in (1, 2, 31, 32, 33, 130, 1025)]
    + [(257, 3, k, 1, k % 2 == 0) for k in (1, 2, 31, 32, 33, 64, 256)]
    + [(1000, 130, 64, 1, True), (257, 33, 256, 3, True), (65, 1025, 33, 3, False),
       (1000, 1, 256, 1, False), (63, 32, 32, 3, True), (64, 2, 2, 3, True),
       (1, 1, 1, 3, False), (3, 5, 7, 1, True), (2500, 31, 3, 1, True), (1100, 1, 2, 3, True)]
)
IDS = [f"n{n}-d{d}-k{k}-B{B}{'-pad' if pad else ''}" for n, d, k, B, pad in CASES]


def dev(a):
    return torch.tensor(a, device="cuda:0")


def on_device(X, pad):
    """X float32 [B, n, d] as a device tensor; padded: rows d + 4 (even d) or d + 5 (odd d)
    apart, items n * ld + 7 apart, NaN in every gap."""
    B, n, d = X.shape
    if not pad:
        return dev(X)
    ld = d + (4 if d % 2 == 0 else 5)
    buf = torch.full((B, n * ld + 7), float("nan"), device="cuda:0")
    view = torch.as_strided(buf, (B, n, d), (n * ld + 7, ld, 1))
    view.copy_(dev(X))
    return view


@functools.lru_cache(maxsize=None)
def data(n, d, k, B, kind):
    """(X [B, n, d], C [B, k, d]) float32, read-only: blobs around C, or uniform noise."""
    if kind == "blobs":
        made = [kl.blobs(n, d, k, seed=17 + b) for b in range(B)]
        X, C = np.stack([m[0] for m in made]), np.stack([m[1] for m in made])
    else:
        X = np.stack([kl.noise(n, d, seed=31 + b) for b in range(B)])
        C = np.stack([kl.noise(k, d, seed=57 + b) for b in range(B)])
    X.setflags(write=False)
    C.setflags(write=False)
    return X, C


def step(X, C, pad=False):
    """kmeans_step on numpy [B, n, d], [B, k, d] -> numpy (labels, C_new, counts, inertia)."""
    out = torch.ops.specenh.kmeans_step(on_device(X, pad), dev(C))
    return tuple(o.cpu().numpy() for o in out)


def check_labels(X, C, labels, tag):
    """The label criterion at every point; returns the worst excess / bound."""
    excess, bound, _ = kl.label_slack(X, C, labels)
    assert labels.min() >= 0 and labels.max() < C.shape[0]
    ratio = float((excess / np.maximum(bound, 1e-300)).max())   # a centre at 0: 0 <= 0
    bad = int((excess > bound).sum())
    assert bad == 0, f"{tag}: {bad} points beyond the bound, worst ratio {ratio:.3f}"
    return ratio


def check_update(X, C, labels, C_new, counts, inertia, tag):
    """Counts, centres and inertia of one item against float64 for the kernel's own labels."""
    n, d = X.shape
    k = C.shape[0]
    C64, counts64, _, inertia64 = kl.update64(X, labels, C)
    assert counts.dtype == np.int32 and np.array_equal(counts, counts64), tag
    empty = counts == 0
    assert np.array_equal(C_new[empty].view(np.uint32), C[empty].view(np.uint32)), tag
    A = kl.abs_sums64(X, labels, k)
    worst = 0.0
    for j in np.flatnonzero(~empty):
        bound = (kl.c_u(n, counts[j]) + 1) * EPS * A[j] / counts[j]
        err = np.abs(C_new[j].astype(np.float64) - C64[j])
        assert (err <= bound).all(), f"{tag}: centre {j} off by {(err / bound).max():.3f} bounds"
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
    ibound = kl.c_i(n, d) * EPS * inertia64
    assert abs(float(inertia) - inertia64) <= ibound, (tag, float(inertia), inertia64, ibound)
    return worst, abs(float(inertia) - inertia64) / max(ibound, 1e-300)


# ---------------------------------------------------------------- one iteration
@pytest.mark.parametrize("kind", ["blobs", "noise"])
@pytest.mark.parametrize("n,d,k,B,pad", CASES, ids=IDS)
def test_step_against_float64(n, d, k, B, pad, kind):
    X, C = data(n, d, k, B, kind)
    if kind == "blobs":   # the maker's margin: a float32 argmin has to agree with the oracle
        for b in range(B):
            assert kl.margin_ok(X[b], C[b]).all()
    labels, C_new, counts, inertia = step(X, C, pad)
    assert labels.shape == (B, n) and labels.dtype == np.int32
    assert C_new.shape == (B, k, d) and counts.shape == (B, k) and inertia.shape == (B,)
    ratios = []
    for b in range(B):
        tag = f"{kind} n={n} d={d} k={k} item {b}"
        ratios.append(check_labels(X[b], C[b], labels[b], tag))
        if kind == "blobs":
            assert np.array_equal(labels[b], kl.assign64(X[b], C[b])), tag
        worst_c, worst_i = check_update(X[b], C[b], labels[b], C_new[b], counts[b], inertia[b],
                                        tag)
        ratios.append(max(worst_c, worst_i))
        if k > n:
            assert (counts[b] == 0).sum() >= k - n
    print(f"\n[kmeans step {kind} n={n} d={d} k={k} B={B}] worst label excess / bound = "
          f"{max(ratios[0::2]):.3f}, worst update error / bound = {max(ratios[1::2]):.3f}")


@pytest.mark.parametrize("n,d,k,twin,of", [(1000, 3, 5, 3, 1), (257, 33, 256, 200, 7),
                                           (65, 1, 64, 63, 0), (300, 130, 40, 39, 2)])
def test_a_duplicated_centre_never_wins(n, d, k, twin, of):
    """C[twin] = C[of], of < twin: identical rows get identical score bits, whatever block or
    wave holds them, and the lower index takes the tie."""
    X = kl.noise(n, d, seed=5).copy()
    C = kl.noise(k, d, seed=6).copy()
    C[twin] = C[of]
    X[:10] = C[of] + 1e-3 * X[:10]          # points for which the pair is (nearly always) best
    labels, _, counts, _ = step(X[None], C[None])
    assert not (labels[0] == twin).any() and counts[0, twin] == 0
    check_labels(X, C, labels[0], "twin")
    # all points equal to one centre, all centres equal: everything ties, label 0
    X1 = np.repeat(C[:1], 70, axis=0)
    C1 = np.repeat(C[:1], 33, axis=0)
    assert not step(X1[None], C1[None])[0].any()


def test_empty_clusters_keep_their_centres():
    X, C = data(3, 5, 7, 1, "noise")        # k > n
    labels, C_new, counts, _ = step(X, C)
    assert counts.sum() == 3 and (counts[0] == 0).sum() >= 4
    for j in np.flatnonzero(counts[0] == 0):
        assert C_new[0, j].tobytes() == C[0, j].tobytes()
    far = np.concatenate([kl.noise(4, 33, seed=1), np.full((1, 33), 50.0, np.float32)])
    labels, C_new, counts, _ = step(kl.noise(1000, 33, seed=2)[None], far[None])
    assert counts[0, 4] == 0 and C_new[0, 4].tobytes() == far[4].tobytes()


# ---------------------------------------------------------------- determinism
@pytest.mark.parametrize("n,d,k", [(1000, 33, 33), (2500, 3, 256), (257, 1025, 5)])
def test_bits_do_not_depend_on_the_run_the_batch_or_the_stride(n, d, k):
    X, C = data(n, d, k, 3, "noise")
    first = step(X, C, pad=False)
    again = step(X, C, pad=False)
    padded = step(X, C, pad=True)
    for a, b, c in zip(first, again, padded):
        assert a.tobytes() == b.tobytes() == c.tobytes()
    for b in (0, 2):
        alone = step(X[b:b + 1], C[b:b + 1], pad=(b == 0))
        for a, s in zip(first, alone):
            assert a[b].tobytes() == s[0].tobytes()
    Xd, Cd = dev(X), dev(C)
    assert np.array_equal(torch.ops.specenh.kmeans_assign(Xd, Cd).cpu().numpy(), first[0])
    # the two-dimensional forms are the batch of one
    lab2, C2, cnt2, ine2 = torch.ops.specenh.kmeans_step(Xd[1], Cd[1])
    assert lab2.shape == (n,) and C2.shape == (k, d) and cnt2.shape == (k,) and ine2.shape == ()
    assert np.array_equal(lab2.cpu().numpy(), first[0][1])
    assert C2.cpu().numpy().tobytes() == first[1][1].tobytes()
    assert float(ine2) == float(first[3][1])
    assert np.array_equal(torch.ops.specenh.kmeans_assign(Xd[1], Cd[1]).cpu().numpy(), first[0][1])


def test_graph_capture():
    X, C = data(1000, 33, 33, 3, "noise")
    Xd, Cd = dev(X), dev(C)
    eager = torch.ops.specenh.kmeans_step(Xd, Cd)
    xs, cs = torch.zeros_like(Xd), torch.zeros_like(Cd)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):      # the outputs and the workspace come from the graph's pool
        captured = torch.ops.specenh.kmeans_step(xs, cs)
    xs.copy_(Xd), cs.copy_(Cd)
    g.replay()
    torch.cuda.synchronize()
    for e, c in zip(eager, captured):
        assert torch.equal(e, c)


def test_opcheck():
    X, C = data(65, 3, 3, 1, "noise")
    Xd, Cd = dev(X), dev(C)
    for op, args in ((torch.ops.specenh.kmeans_assign, (Xd, Cd)),
                     (torch.ops.specenh.kmeans_step, (Xd[0], Cd[0]))):
        torch.library.opcheck(op, args)


# ---------------------------------------------------------------- fit
@pytest.mark.parametrize("n,d,k", [(1000, 2, 5), (257, 33, 12), (1000, 1, 3)])
@pytest.mark.parametrize("as_numpy", [True, False], ids=["numpy", "device"])
def test_fit_on_blobs_follows_the_float64_iteration(n, d, k, as_numpy):
    from specenh.cluster import KMeans

    X, cent, lab = kl.blobs(n, d, k, seed=9)
    rng = np.random.default_rng(9)
    C0 = (cent + rng.uniform(-1, 1, size=cent.shape) * (0.3 / k)).astype(np.float32)
    C64, labels64, inertia64, n_iter64, history = kl.lloyd64(X, C0)
    # every iteration of the oracle has the margin, so float32 must take the same path
    Ct = C0.astype(np.float64)
    for labels_t, _, _ in history:
        assert kl.margin_ok(X, Ct).all()
        Ct = kl.update64(X, labels_t, Ct)[0]
    assert kl.margin_ok(X, C64).all()
    km = KMeans(n_clusters=k, init=C0, n_init=1)
    km.fit(X if as_numpy else dev(X))
    labels, centers = km.labels_, km.cluster_centers_
    if as_numpy:
        assert isinstance(labels, np.ndarray) and isinstance(centers, np.ndarray)
        assert centers.dtype == np.float32 and labels.dtype == np.int32
    else:
        assert labels.is_cuda and centers.is_cuda
        labels, centers = labels.cpu().numpy(), centers.cpu().numpy()
    assert np.array_equal(labels, labels64) and np.array_equal(labels, lab)
    assert km.n_iter_ == n_iter64
    counts = np.bincount(labels64, minlength=k)
    A = kl.abs_sums64(X, labels64, k)
    for j in range(k):
        bound = (kl.c_u(n, counts[j]) + 1) * EPS * A[j] / counts[j]
        assert (np.abs(centers[j] - C64[j]) <= bound).all()
    assert abs(km.inertia_ - inertia64) <= 2 * kl.c_i(n, d) * EPS * inertia64 + 1e-30
    assert np.array_equal(km.predict(X), labels64)
    # float64 in: computed in float32, centres returned as float64
    km64 = KMeans(n_clusters=k, init=C0.astype(np.float64), n_init=1).fit(X.astype(np.float64))
    assert km64.cluster_centers_.dtype == np.float64
    assert np.array_equal(km64.cluster_centers_.astype(np.float32), centers)
    assert np.array_equal(km64.labels_, labels64)


def test_iterations_on_noise_keep_lloyds_properties():
    """No margin here, so properties only: the inertia does not rise from one iteration to
    the next by more than the rounding allows. Exactly, I(C', l') <= I(C', l) <= I(C, l); in
    float32 the labels l' may miss the optimum by their bound, the centres C' the means by
    theirs (which costs m_j |dC_j|^2), and each inertia carries its own relative error."""
    n, d, k = 1000, 3, 8
    X = kl.noise(n, d, seed=3)
    Xd = dev(X)
    C = dev(X[:k])
    prev, rel = None, kl.c_i(n, d) * EPS
    for it in range(12):
        labels, C_new, counts, inertia = torch.ops.specenh.kmeans_step(Xd, C)
        Cn, ln, cn = C.cpu().numpy(), labels.cpu().numpy(), counts.cpu().numpy()
        inertia = float(inertia)
        if prev is not None:
            _, lbound, _ = kl.label_slack(X, Cn, ln)
            A = kl.abs_sums64(X, prev[1], k)
            m = np.maximum(prev[2], 1)[:, None]
            dC = (np.array([kl.c_u(n, c) for c in prev[2]])[:, None] + 1) * EPS * A / m
            allowed = prev[0] * (1 + rel) / (1 - rel) ** 2 + lbound.sum() + (m * dC ** 2).sum()
            print(f"\n[kmeans noise iteration {it}] inertia {inertia:.6f} after {prev[0]:.6f}")
            assert inertia <= allowed, (it, inertia, prev[0], allowed)
        prev = (inertia, ln, cn)
        C = C_new


@pytest.mark.parametrize("n,d,k", [(1000, 2, 5), (300, 33, 4)])
def test_fit_on_noise_ends_at_a_fixed_point(n, d, k):
    from specenh.cluster import KMeans

    X = kl.noise(n, d, seed=21)
    km = KMeans(n_clusters=k, init=X[:k].copy(), n_init=1, tol=0.0, max_iter=300).fit(X)
    assert 1 <= km.n_iter_ < 300          # stopped on unchanged labels
    labels, centers = km.labels_, km.cluster_centers_
    ratio = check_labels(X, centers, labels, "fit noise")
    print(f"\n[kmeans fit noise n={n} d={d} k={k}] n_iter {km.n_iter_}, inertia "
          f"{km.inertia_:.6f}, worst label excess / bound {ratio:.3f}")
    # every centre is the mean of its members; the inertia is theirs
    C64, counts, _, inertia64 = kl.update64(X, labels, centers)
    A = kl.abs_sums64(X, labels, k)
    for j in range(k):
        if counts[j]:
            bound = (kl.c_u(n, counts[j]) + 1) * EPS * A[j] / counts[j]
            assert (np.abs(centers[j] - C64[j]) <= bound).all()
    assert abs(km.inertia_ - inertia64) <= kl.c_i(n, d) * EPS * inertia64
    assert np.array_equal(km.predict(X), labels)
    assert np.array_equal(km.fit_predict(X), labels)


@pytest.mark.parametrize("init", ["random", "k-means++"])
def test_the_same_random_state_gives_the_same_fit(init):
    from specenh.cluster import KMeans

    X = kl.blobs(500, 4, 6, seed=4)[0]
    fits = [KMeans(n_clusters=6, init=init, n_init=2, random_state=7).fit(X) for _ in range(2)]
    assert fits[0].cluster_centers_.tobytes() == fits[1].cluster_centers_.tobytes()
    assert np.array_equal(fits[0].labels_, fits[1].labels_)
    assert fits[0].inertia_ == fits[1].inertia_ and fits[0].n_iter_ == fits[1].n_iter_
    assert fits[0].cluster_centers_.shape == (6, 4) and fits[0].labels_.shape == (500,)
    assert len(np.unique(fits[0].cluster_centers_, axis=0)) == 6    # k distinct starting rows
    with pytest.raises(ValueError, match="n_samples=5 should be >= n_clusters=6"):
        KMeans(n_clusters=6, init=init).fit(X[:5])


def test_batched_kmeans_equals_the_single_runs():
    from specenh import cluster

    n, d, k = 700, 3, 6
    X = np.stack([kl.noise(n, d, seed=40), kl.blobs(n, d, k, seed=41)[0], kl.noise(n, d, seed=42)])
    Xd = dev(X)
    init = Xd[:, :k].contiguous()
    C, labels, inertia, n_iter = cluster.kmeans(Xd, init, max_iter=100, tol=1e-4)
    assert C.shape == (3, k, d) and labels.shape == (3, n) and labels.dtype == torch.int32
    assert inertia.shape == (3,) and n_iter.shape == (3,)
    assert len(set(n_iter.tolist())) > 1      # the items do stop at different iterations
    for b in range(3):
        Cb, lb, ib, nb = cluster.kmeans(Xd[b:b + 1], init[b:b + 1], max_iter=100, tol=1e-4)
        assert torch.equal(Cb[0], C[b]) and torch.equal(lb[0], labels[b])
        assert torch.equal(ib[0], inertia[b]) and int(nb[0]) == int(n_iter[b])


# ---------------------------------------------------------------- segment
def test_segment():
    from specenh import cluster

    made = [kl.two_level_image(r, c, seed=s) for (r, c), s in (((40, 70), 1), ((40, 70), 2))]
    imgs = np.stack([m[0] for m in made] + [np.full((40, 70), 0.3, np.float32)])
    labels, centers = cluster.segment(imgs, n_clusters=2)
    assert labels.shape == (3, 40, 70) and labels.dtype == np.int32 and centers.shape == (3, 2)
    for b in range(2):
        assert np.array_equal(labels[b] == 1, made[b][1])
        assert abs(centers[b, 0] - 0.2) < 0.01 and abs(centers[b, 1] - 0.8) < 0.01
    assert not labels[2].any()                 # a constant image
    assert (np.diff(centers, axis=1) >= 0).all()
    for b in range(3):                         # a batch is its single images
        lb, cb = cluster.segment(imgs[b], n_clusters=2)
        assert lb.shape == (40, 70) and np.array_equal(lb, labels[b])
        assert cb.tobytes() == centers[b].tobytes()
    # three clusters on a device tensor: ascending centres, the top label is the mode mask
    img3 = np.where(made[0][1], 0.9, np.where(made[1][1], 0.5, 0.1)).astype(np.float32)
    lab3, cen3 = cluster.segment(dev(img3), n_clusters=3)
    assert lab3.is_cuda and cen3.is_cuda and lab3.dtype == torch.int32
    assert (cen3[1:] > cen3[:-1]).all()
    assert np.array_equal(lab3.cpu().numpy() == 2, made[0][1])
    odd, mask = kl.two_level_image(33, 131, seed=3)     # one image, more than one slab
    assert np.array_equal(cluster.segment(odd)[0] == 1, mask)
