"""Time k-means (csrc/kmeans.hip) in one process, at three sizes:

  pixels  4096 x (16384 pixels, d = 1, k = 3)   the C5 label case of cluster.segment
  strips  n = 4096, d = 16384, k = 64           the 128 x 128 strips
  points  n = 2^20, d = 32, k = 256

  step        torch.ops.specenh.kmeans_step: one Lloyd iteration (assignment and update)
  assign      torch.ops.specenh.kmeans_assign alone
  fit         specenh.cluster.kmeans, FIT_ITERS iterations (tol = 0) and the final assignment
  torch       what they replace, in float32: cdist -> argmin -> index_add_ of the points and of
              ones, one division (the [n, k] distances are materialised, the sums are atomic)
  torch_fit   that step FIT_ITERS + 1 times

HIP events around each route, 3 warm-ups, interleaved rounds, median (and min). With each
time: the fraction of the fp32 matrix peak (157.3 Tflop/s) on the 2 n d k flops of the step's
two products (4 n d k in all) and the fraction of HBM (8 TB/s spec; 6.3 TB/s is what a copy
reaches) on the algorithmic traffic 2 n d 4 bytes. No counter profile is taken here.
    python tools/kmeans_bench.py [--json PATH] [--rounds N]"""
import json

from benchlib import measure, parse_args, resources, write_json  # puts the package on sys.path

import torch
from specenh import cluster

path, ROUNDS, _ = parse_args(5)
WARM = 3
FIT_ITERS = 10
MFMA_PEAK = 157.3e12
HBM_PEAK = 8.0e12
# (label, batch, n, d, k, items of the torch route)
SHAPES = [("pixels", 4096, 16384, 1, 3, 256), ("strips", 1, 4096, 16384, 64, 1),
          ("points", 1, 1 << 20, 32, 256, 1)]
ops = torch.ops.specenh


def torch_step(X, C):
    """X [B, n, d], C [B, k, d] -> (labels, C_new), the composition the kernels replace."""
    B, n, d = X.shape
    k = C.shape[1]
    labels = torch.cdist(X, C).argmin(dim=2)
    sums = torch.zeros_like(C)
    counts = torch.zeros((B, k), device=X.device)
    if B == 1:
        sums[0].index_add_(0, labels[0], X[0])
        counts[0].index_add_(0, labels[0], torch.ones(n, device=X.device))
    else:       # index_add_ of every item at once
        sums.scatter_add_(1, labels[:, :, None].expand(B, n, d), X)
        counts.scatter_add_(1, labels, torch.ones((B, n), device=X.device))
    return labels, torch.where(counts[:, :, None] > 0, sums / counts[:, :, None].clamp(min=1), C)


def torch_fit(X, C):
    for _ in range(FIT_ITERS):
        _, C = torch_step(X, C)
    return torch_step(X, C)[0], C


res = {"rounds": ROUNDS, "warmups": WARM, "fit_iterations": FIT_ITERS,
       "fp32_matrix_peak_flops": MFMA_PEAK, "hbm_peak_bytes_per_s": HBM_PEAK,
       "counter_profile": "not taken", "note": "a first version; no counter profile taken",
       "kernel_resources": resources("kmeans.hip"), "shapes": {}}
print(json.dumps(res["kernel_resources"]), flush=True)
for label, B, n, d, k, Bt in SHAPES:
    g = torch.Generator("cuda").manual_seed(1)
    # k levels plus noise: clusters that exist, as in the use cases
    level = torch.randint(k, (B, n, 1), device="cuda", generator=g).float() / k
    X = level + 0.3 / k * torch.randn((B, n, d), device="cuda", generator=g)
    del level
    init = X[:, :k].contiguous()
    runs = {"step": lambda: ops.kmeans_step(X, init),
            "assign": lambda: ops.kmeans_assign(X, init),
            "fit": lambda: cluster.kmeans(X, init, max_iter=FIT_ITERS, tol=0.0),
            "torch": lambda: torch_step(X[:Bt], init[:Bt]),
            "torch_fit": lambda: torch_fit(X[:Bt], init[:Bt])}
    entry = {"batch": B, "n": n, "d": d, "k": k, "torch_batch": Bt}
    entry.update(measure(runs, ROUNDS, WARM))
    entry["fit_iterations_run"] = cluster.kmeans(X, init, max_iter=FIT_ITERS, tol=0.0)[3].tolist()[:8]
    flops = 2.0 * B * n * d * k
    traffic = 2.0 * B * n * d * 4
    t = entry["step_ms_median"] * 1e-3
    entry["step_flops_2ndk_over_mfma_peak"] = flops / t / MFMA_PEAK
    entry["step_flops_both_products_over_mfma_peak"] = 2 * flops / t / MFMA_PEAK
    entry["step_traffic_2nd4_over_hbm_peak"] = traffic / t / HBM_PEAK
    ta = entry["assign_ms_median"] * 1e-3
    entry["assign_flops_2ndk_over_mfma_peak"] = flops / ta / MFMA_PEAK
    entry["assign_traffic_nd4_over_hbm_peak"] = traffic / 2 / ta / HBM_PEAK
    entry["torch_over_step_per_item"] = (entry["torch_ms_median"] / Bt) / (entry["step_ms_median"] / B)
    entry["torch_fit_over_fit_per_item"] = ((entry["torch_fit_ms_median"] / Bt)
                                            / (entry["fit_ms_median"] / B))
    lab = ops.kmeans_step(X[:Bt], init[:Bt])[0]
    entry["labels_differing_from_torch"] = int((lab != torch_step(X[:Bt], init[:Bt])[0]).sum())
    entry["labels_compared"] = int(lab.numel())
    print(f"{label:7s} " + "  ".join(f"{m} {entry[m + '_ms_median']:9.3f} ms" for m in runs)
          + f" (torch: {Bt} of {B} items)  step: {entry['step_flops_2ndk_over_mfma_peak']:.4f} of "
          f"the fp32 MFMA peak on 2ndk, {entry['step_traffic_2nd4_over_hbm_peak']:.4f} of HBM on "
          f"2nd4; torch / step per item {entry['torch_over_step_per_item']:.1f}, fit "
          f"{entry['torch_fit_over_fit_per_item']:.1f}; labels differing from torch "
          f"{entry['labels_differing_from_torch']} of {entry['labels_compared']}", flush=True)
    res["shapes"][label] = entry
    del X, init, runs, lab
    torch.cuda.empty_cache()
write_json(res, path)
