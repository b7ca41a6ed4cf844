"""The `from sklearn.cluster import KMeans` of the reference files on the GPU:

    from specenh.cluster import KMeans
    km = KMeans(n_clusters=4, random_state=0).fit(latent)        # numpy in, numpy out
    mask = cluster.segment(spectrograms, n_clusters=2)[0] == 1   # mode / background pixels

One Lloyd iteration is ``torch.ops.specenh.kmeans_step`` (csrc/kmeans.hip: assignment and
update on the fp32 matrix cores, no floating-point atomics; include/specenh_kmeans.h has the
arithmetic). Everything here around it is plumbing: initialisation, the stopping rule and
the bookkeeping of a batch. Results are bit-reproducible: from run to run, and an item of a
batch equals its single run.

Differences from scikit-learn: the arithmetic is fp32 (float64 input is cast and the centres
are returned as float64); an empty cluster keeps its previous centre instead of being
relocated; a final assignment always follows the loop, so ``labels_`` and ``inertia_`` belong to
``cluster_centers_``; only Lloyd's algorithm, no sample weights.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib

__all__ = ["KMeans", "kmeans", "segment"]


def _ops():
    from .ops import ops
    return ops


def _device():
    if not torch.cuda.is_available():
        raise RuntimeError("specenh requires a ROCm GPU (HIP); there is no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


def _to_device(X, what="X"):
    """(fp32 device tensor, was_numpy, original floating dtype or None)."""
    if isinstance(X, torch.Tensor):
        if X.device.type != "cuda":
            raise RuntimeError("specenh.cluster runs on the GPU only (no CPU fallback)")
        return X.float(), False, X.dtype if X.dtype == torch.float64 else None
    a = np.asarray(X)
    if a.dtype.kind not in "fiu":
        raise TypeError(f"{what} must be numeric")
    t = torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=_device())
    return t, True, torch.float64 if a.dtype == np.float64 else None


def kmeans(X, init, max_iter=300, tol=1e-4):
    """Lloyd's k-means of every item of a batch: X [B, n, d] and init [B, k, d], float32 device
    tensors. Returns (centers [B, k, d], labels [B, n] int32, inertia [B], n_iter [B]).

    Every item stops on its own criterion, scikit-learn's: after an iteration whose labels
    equal the previous iteration's, or whose centres moved by sum |C_new - C|^2 <= tol *
    mean(var(X, axis=0)); at most max_iter iterations. A finished item's centres are frozen
    while the others go on (one host read an iteration decides whether any is left), and a
    final assignment gives the labels and the inertia of the returned centres. Item b equals
    its single run bit for bit."""
    ops = _ops()
    if X.dim() != 3 or init.dim() != 3:
        raise ValueError("X must be [B, n, d] and init [B, k, d]")
    if X.shape[1] < init.shape[1]:
        raise ValueError(f"n_samples={X.shape[1]} should be >= n_clusters={init.shape[1]}.")
    max_iter = int(max_iter)
    if max_iter < 1:
        raise ValueError("max_iter must be at least 1")
    B = X.shape[0]
    C = init.float().contiguous().clone()
    # thresholds and centre shifts in fp64: their bits do not depend on how a batch is reduced
    thr = float(tol) * X.double().var(dim=1, unbiased=False).mean(dim=1)
    done = torch.zeros(B, dtype=torch.bool, device=X.device)
    n_iter = torch.zeros(B, dtype=torch.int64, device=X.device)
    prev = None
    for _ in range(max_iter):
        labels, C_new, _, _ = ops.kmeans_step(X, C)
        active = ~done
        shift = (C_new.double() - C.double()).square().sum(dim=(1, 2))
        stop = shift <= thr
        if prev is not None:
            stop = stop | (labels == prev).all(dim=1)
        C = torch.where(active[:, None, None], C_new, C)
        n_iter += active
        done = done | stop
        prev = labels
        if bool(done.all()):
            break
    labels, _, _, inertia = ops.kmeans_step(X, C)
    return C, labels, inertia, n_iter


class KMeans:
    """sklearn.cluster.KMeans on the GPU: ``fit``, ``predict``, ``fit_predict`` and the
    attributes ``cluster_centers_``, ``labels_``, ``inertia_``, ``n_iter_``. numpy in, numpy out
    (float64 is computed in fp32, its centres returned as float64); device tensors stay on the
    device. ``init``: "k-means++" (D^2 sampling), "random" (k distinct rows) or an array [k, d];
    both random inits draw from a torch.Generator seeded with ``random_state``. ``n_init``
    "auto" is 1; the run of lowest inertia wins."""

    _ACCEPTED = {"algorithm": ("lloyd", "auto"), "copy_x": (True, False), "verbose": (0, False)}

    def __init__(self, n_clusters=8, init="k-means++", n_init="auto", max_iter=300, tol=1e-4,
                 random_state=None, **kwargs):
        for name, value in kwargs.items():
            if name not in self._ACCEPTED or value not in self._ACCEPTED[name]:
                raise NotImplementedError(f"KMeans: {name}={value!r} is not implemented "
                                          "(Lloyd's algorithm, no sample weights)")
        if isinstance(init, str) and init not in ("k-means++", "random"):
            raise ValueError(f"init must be 'k-means++', 'random' or an array, not {init!r}")
        if callable(init):
            raise NotImplementedError("KMeans: a callable init is not implemented")
        if n_init != "auto" and (not isinstance(n_init, (int, np.integer)) or n_init < 1):
            raise ValueError("n_init must be 'auto' or a positive int")
        if int(n_clusters) < 1 or int(n_clusters) > _lib.KMEANS_MAX_K:
            raise (ValueError if int(n_clusters) < 1 else NotImplementedError)(
                f"n_clusters must be in [1, {_lib.KMEANS_MAX_K}]")
        self.n_clusters = int(n_clusters)
        self.init = init
        self.n_init = n_init
        self.max_iter = int(max_iter)
        self.tol = float(tol)
        self.random_state = random_state

    # ------------------------------------------------------------ initial centres
    def _generator(self, device):
        g = torch.Generator(device=device)
        if self.random_state is None:
            g.seed()
        else:
            g.manual_seed(int(self.random_state))
        return g

    def _init_centers(self, X, g):
        n, d = X.shape
        k = self.n_clusters
        if not isinstance(self.init, str):
            C, _, _ = _to_device(self.init, "init")
            if tuple(C.shape) != (k, d):
                raise ValueError(f"init has shape {tuple(C.shape)}, expected ({k}, {d})")
            return C.to(X.device)
        if self.init == "random":
            return X[torch.randperm(n, generator=g, device=X.device)[:k]].contiguous()
        # k-means++: the next centre is drawn with probability proportional to the squared
        # distance to the nearest centre so far
        ops = _ops()
        C = torch.empty((k, d), dtype=torch.float32, device=X.device)
        C[0] = X[torch.randint(n, (1,), generator=g, device=X.device)[0]]
        for i in range(1, k):
            near = C[:i][ops.kmeans_assign(X, C[:i].contiguous()).long()]
            d2 = (X - near).square().sum(dim=1)
            d2 = torch.where(d2.sum() > 0, d2, torch.ones_like(d2))  # all points are centres
            C[i] = X[torch.multinomial(d2, 1, generator=g)[0]]
        return C

    # ------------------------------------------------------------ sklearn's methods
    def fit(self, X, y=None, sample_weight=None):
        if sample_weight is not None:
            raise NotImplementedError("KMeans.fit: sample_weight is not implemented")
        shape = tuple(X.shape) if isinstance(X, torch.Tensor) else np.shape(X)
        if len(shape) != 2:
            raise ValueError("X must be [n_samples, n_features]")
        if shape[0] < self.n_clusters:
            raise ValueError(f"n_samples={shape[0]} should be >= n_clusters={self.n_clusters}.")
        Xd, was_numpy, wide = _to_device(X)
        g = self._generator(Xd.device)
        runs = 1 if self.n_init == "auto" or not isinstance(self.init, str) else int(self.n_init)
        best = None
        for _ in range(runs):
            C0 = self._init_centers(Xd, g)
            C, labels, inertia, n_iter = kmeans(Xd[None], C0[None], self.max_iter, self.tol)
            res = (float(inertia[0]), C[0], labels[0], int(n_iter[0]))
            if best is None or res[0] < best[0]:
                best = res
        self.inertia_, self._centers, labels, self.n_iter_ = best
        centers = self._centers if wide is None else self._centers.to(wide)
        self.cluster_centers_ = centers.cpu().numpy() if was_numpy else centers
        self.labels_ = labels.cpu().numpy() if was_numpy else labels
        return self

    def predict(self, X):
        if not hasattr(self, "_centers"):
            raise RuntimeError("this KMeans instance is not fitted yet")
        Xd, was_numpy, _ = _to_device(X)
        if Xd.dim() != 2 or Xd.shape[1] != self._centers.shape[1]:
            raise ValueError(f"X must be [n_samples, {self._centers.shape[1]}]")
        labels = _ops().kmeans_assign(Xd, self._centers.to(Xd.device))
        return labels.cpu().numpy() if was_numpy else labels

    def fit_predict(self, X, y=None, sample_weight=None):
        return self.fit(X, y, sample_weight).labels_


def segment(images, n_clusters=2, max_iter=50):
    """Pixel k-means of every image, a data-driven alternative to ``quantfilt``'s fixed
    quantile: images [B, rows, cols] (or one [rows, cols]) -> (labels int32 of the same
    shape, centers [B, k] ascending). The initial centres are evenly spaced between an image's
    minimum and maximum (no random numbers); clusters are numbered by ascending centre, so
    ``labels == n_clusters - 1`` is the mask of the brightest pixels (the modes). A constant image
    gets all-zero labels. numpy in, numpy out; device tensors stay on the device."""
    k = int(n_clusters)
    if k < 1 or k > _lib.KMEANS_MAX_K:
        raise ValueError(f"n_clusters must be in [1, {_lib.KMEANS_MAX_K}]")
    t, was_numpy, wide = _to_device(images, "images")
    if t.dim() not in (2, 3) or t.shape[-1] < 1 or t.shape[-2] < 1:
        raise ValueError("images must be [rows, cols] or [batch, rows, cols]")
    single = t.dim() == 2
    t3 = t[None] if single else t
    B, rows, cols = t3.shape
    X = t3.reshape(B, rows * cols, 1)
    lo, hi = X.amin(dim=1), X.amax(dim=1)                       # [B, 1]
    frac = torch.arange(k, dtype=torch.float32, device=X.device) / max(k - 1, 1)
    init = (lo + (hi - lo) * frac[None, :]).unsqueeze(2)        # [B, k, 1]
    C, labels, _, _ = kmeans(X, init, max_iter, 1e-4)
    C, order = torch.sort(C[:, :, 0], dim=1, stable=True)       # equal centres keep their order
    rank = torch.empty_like(order)
    rank.scatter_(1, order, torch.arange(k, device=X.device).expand(B, k))
    labels = torch.gather(rank, 1, labels.long()).to(torch.int32)
    # a constant image is one cluster by definition: the mean of equal pixels need not be
    # their value in fp32, which would otherwise decide between k equal centres
    flat = hi == lo                                             # [B, 1]
    labels = torch.where(flat, torch.zeros_like(labels), labels).reshape(B, rows, cols)
    C = torch.where(flat, lo.expand(B, k), C)
    if wide is not None:
        C = C.to(wide)
    if single:
        labels, C = labels[0], C[0]
    return (labels.cpu().numpy(), C.cpu().numpy()) if was_numpy else (labels, C)
