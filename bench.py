"""Benchmark of the spectrogram-enhancement hot path on 1..N MI355X GPUs.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--batch B] [--dump-outputs DIR]
    python bench.py --full [--no-cpu-baseline] [--no-stages] ...
    python -m torch.distributed.run --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

A plain run sets up, warms up, times the K steps and prints the result line (metric, value,
unit, higher_is_better, dtype, ms_per_step, config): nothing else runs. --full adds the
roofline, stages, cpu_baseline and accuracy legs described below (null in a plain run).
--dump-outputs DIR writes what the last timed step returned (DIR/reconstructions.npy,
float32; a fixed seeded sample of the shots when the batch exceeds DUMP_MAX_SHOTS). The
inputs are seeded, so two builds run with the same arguments compare output for output.

BASELINE.json's metric is "spectrograms/s (STFT+VAE-denoise fwd) ... PSNR vs CPU ref":
the end-to-end inference stream of SURVEY.md §8(d) C5, per GPU. One step = one batch of
B shots resident in HBM (default 4096 x 16,512 fp16 samples of synthetic plasma chirps):

    specgr: spectrogram 256-pt hann / hop 128, linear detrend, density, log, min-max,
            drop Nyquist -> [B, 128, 128] fp32          (stft_psd_kernel<256, fp16 in>)
            (the fp16 samples are widened to fp32 on load: no conversion pass)
    denoiseSignal default (drop the top singular component) -> [B, 128, 128] fp32
                                                        (gram / subspace / recon kernels)
    (the SVD stores its reconstruction as the fp16 NHWC autoencoder input)
    conv autoencoder forward (manual_scan_3layers.py:186-199 layout, 16/32/64 filters, 5x5,
            trained weights) -> [B, 128, 128, 1] fp32
            (conv_c1_mfma + pool, conv_patch + pool x2, conv_patch convT x2, fused tail)

The batch splits over --streams HIP streams (default 2) with staggered chains.

Shots shard across ranks (each rank owns its B shots; no collective in the data path;
weak scaling); value = all ranks' spectrograms / max-over-ranks wall time.

Rank 0 prints ONE JSON line with, besides the contract fields (the rest under --full):
  roofline      the dominant kernel of a step: the autoencoder layer launch with the largest
                measured time (HIP events around every launch, on its stream). Its bound is
                whichever floor is higher: algorithmic HBM bytes (activations read once and
                written once + weights, ae_layer_costs) / 8 TB/s, or useful FLOPs (SURVEY §8
                A7 MACs x 2) / the unit's peak (MFMA 2.5 PFLOP/s dense fp16 for every layer of
                the fused forward; an unfused 1-output-channel conv would run on the VALU,
                v_dot2 314.6 TFLOP/s). traffic = measured HBM
                bytes of that launch from profiles/pmc_r06.json (rocprofv3 --pmc passes of
                tools/pmc_refresh.sh at the same shapes, keyed by the exact kernel symbol: null
                with a warning when the timed launch ran a different kernel); stages.ae_layers
                has every layer.
  stages        per-stage ms of one slice (stages.shots_per_launch shots: the launch shape
                of the timed step, which splits the batch over --streams HIP streams;
                default 2), and the C2 STFT-only configuration (4096 x
                65,536 fp32, nperseg 1024 / hop 256) with its HBM roofline.
  cpu_baseline  the same chain on the host CPU (scipy.signal.spectrogram + log/min-max,
                numpy SVD, torch-CPU autoencoder with the same weights) on a bounded
                sample, timed before the GPU is touched.
  accuracy      GPU output vs the fp64 CPU chain on sample shots, with the trained
                reference-model weights (tests/golden/ae_c4_trained.npz: outputs that carry
                a signal): out_rel = ||y - y_ref|| / ||y_ref - mean(y_ref)|| per shot (max),
                psnr_db = 10 log10(var(y_ref) / mse), pass = out_rel within the fp16
                tolerance of oracle/checks.py (a dropped MFMA k-step fails it).
"""
from __future__ import annotations

import argparse
import ctypes
import json
import multiprocessing as mp
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [REPO, os.path.join(REPO, "spectrogram-enhancement_amd")]

METRIC = "spectrograms/s (STFT+VAE-denoise fwd) at 1/2/4/8 GPUs; PSNR vs CPU ref"
# C5 (SURVEY.md §8 d): C1 spectrogram parameters on 16,512-sample shots -> 128 x 128
L5 = 16512
SPEC5 = {"nperseg": 256, "noverlap": 128, "fs": 500000, "window": "hann",
         "scaling": "density", "detrend": "linear", "eps": 1e-11}
HW5 = 128
AE_FILTERS, AE_K = (16, 32, 64), 5
# C2 STFT stage
L2 = 65536
SPEC2 = {"nperseg": 1024, "noverlap": 768, "fs": 500000, "window": "hamm",
         "scaling": "density", "detrend": "linear", "eps": 1e-11}
F2, T2 = 512, (L2 - 1024) // 256 + 1
ALG_BYTES_C2 = 4 * L2 + 4 * F2 * T2  # 780,288 B per spectrogram (SURVEY §8 d)
HBM_PEAK_GBPS = 8000.0               # MI355X_MICROARCH.md: HBM3E 8 TB/s
MFMA_PEAK_TFLOPS = 2500.0            # dense fp16/bf16 (256 CU x 4 SIMD x 1024 FLOP/clk x 2.4 GHz)


def ae_layers():
    c1, c2, c3 = AE_FILTERS
    k = AE_K
    return [("conv", 1, c1, k, "relu"), ("pool",), ("conv", c1, c2, k, "relu"), ("pool",),
            ("conv", c2, c3, k, "relu"), ("pool",), ("convT", c3, c3, k, "relu"),
            ("convT", c3, c2, k, "relu"), ("convT", c2, c1, k, "relu"),
            ("conv", c1, 1, k, "sigmoid")]


AE_WEIGHTS = os.path.join(REPO, "tests", "golden", "ae_c4_trained.npz")


def ae_weights():
    """The reference model's weights after 400 Keras-Adam steps on C4-style synthetic data
    (tests/golden/make_ae_weights.py; no real checkpoint exists): the outputs span the
    sigmoid, so the accuracy leg measures a real signal. Compute is weight-independent."""
    with np.load(AE_WEIGHTS, allow_pickle=False) as d:
        return [d[k] for k in sorted(d.files)]


def ae_flops_per_sample(h=HW5, w=HW5):
    """2 x useful MACs (no padding or dilation holes counted) of the 7 convolutions."""
    macs, hh, ww = 0, h, w
    for lay in ae_layers():
        if lay[0] == "pool":
            hh, ww = hh // 2, ww // 2
            continue
        kind, cin, cout, k, _ = lay
        if kind == "convT":
            macs += hh * ww * cin * cout * k * k  # each input pixel scatters k*k taps
            hh, ww = 2 * hh, 2 * ww
        else:
            macs += hh * ww * cin * cout * k * k
    return 2 * macs


VALU_DOT2_PEAK_TFLOPS = 314.6         # v_dot2_f32_f16: 4 FLOP/lane/instr, 128 lanes/clk/CU
LAYER_NAMES = ["conv1+pool", "conv2+pool", "conv3+pool", "convT1", "convT2", "convT3",
               "conv_out"]
LAYER_NAMES_TAIL = LAYER_NAMES[:5] + ["convT3+conv_out"]
LAYER_NAMES_DEC3 = LAYER_NAMES[:4] + ["convT2+convT3+conv_out"]


def layer_names(eng):
    """Names of the forward's launches (the engine's fusions: encoder2 / decoder3 / tail)."""
    names = LAYER_NAMES_DEC3 if eng.dec3 else (LAYER_NAMES_TAIL if eng.tail else LAYER_NAMES)
    if getattr(eng, "enc2", False):
        names = ["conv1+pool+conv2+pool"] + names[2:]
    return names


def ae_layer_costs(h=HW5, w=HW5, act_bytes=2, out_bytes=4, tail=False, dec3=False, enc2=False):
    """Per launch of the fused forward (conv+pool fused; with ``tail`` the last
    Conv2DTranspose + Conv2D(1) are one launch, csrc/decoder_tail.hip): useful FLOPs and
    algorithmic HBM bytes per sample (activations read once + written once), the weights
    read once per launch, and the units that do the arithmetic: every layer is on the
    matrix cores (the 1-input-channel conv in csrc/conv_c1_mfma.hip, the fused tail's
    Conv2D(1) as per-row MFMAs + diagonal sums) except an unfused 1-output-channel conv
    (VALU dot2, csrc/conv_narrow.hip). ``mfma_flops`` is the part on the matrix cores."""
    lays = ae_layers()
    res, hh, ww, i = [], h, w, 0
    while i < len(lays):
        kind, cin, cout, k, _ = lays[i]
        pool = i + 1 < len(lays) and lays[i + 1][0] == "pool"
        oh, ow = (2 * hh, 2 * ww) if kind == "convT" else (hh, ww)
        macs = hh * ww * cin * cout * k * k
        sh, sw = (oh // 2, ow // 2) if pool else (oh, ow)
        last = i + (2 if pool else 1) >= len(lays)
        nbytes = hh * ww * cin * act_bytes + sh * sw * cout * (out_bytes if last else act_bytes)
        unit = "valu" if cout == 1 else "mfma"
        res.append({"flops": 2 * macs, "mfma_flops": 2 * macs if unit == "mfma" else 0,
                    "bytes": nbytes, "weight_bytes": k * k * cin * cout * act_bytes + 4 * cout,
                    "unit": unit})
        hh, ww = sh, sw
        i += 2 if pool else 1
    if tail or dec3:  # convT3 + conv_out, both on MFMA: the 16-channel map is not HBM traffic
        a, b = res[-2], res[-1]
        res = res[:-2] + [{"flops": a["flops"] + b["flops"], "mfma_flops": a["flops"] + b["flops"],
                           "bytes": (h // 2) * (w // 2) * AE_FILTERS[1] * act_bytes +
                           h * w * out_bytes,
                           "weight_bytes": a["weight_bytes"] + b["weight_bytes"],
                           "unit": "mfma"}]
    if dec3:  # + convT2 in front: its 32-channel map is not HBM traffic either
        a, b = res[-2], res[-1]
        res = res[:-2] + [{"flops": a["flops"] + b["flops"], "mfma_flops": a["flops"] + b["flops"],
                           "bytes": (h // 4) * (w // 4) * AE_FILTERS[2] * act_bytes +
                           h * w * out_bytes,
                           "weight_bytes": a["weight_bytes"] + b["weight_bytes"],
                           "unit": "mfma"}]
    if enc2:  # conv1+pool and conv2+pool as one launch: the pooled 16-channel map stays in LDS
        a, b = res[0], res[1]
        res = [{"flops": a["flops"] + b["flops"], "mfma_flops": a["mfma_flops"] + b["mfma_flops"],
                "bytes": h * w * act_bytes + (h // 4) * (w // 4) * AE_FILTERS[1] * act_bytes,
                "weight_bytes": a["weight_bytes"] + b["weight_bytes"], "unit": "mfma"}] + res[2:]
    return res


PMC_FILE = os.path.join(REPO, "profiles", "pmc_r06.json")


def load_pmc():
    """Per-stage PMC records of tools/pmc_fold.py: {target: {stage: {"symbol", "batch",
    "fetch_bytes", "write_bytes", "hbm_bytes", ...}}} (rocprofv3 --pmc passes of
    tools/pmc_refresh.sh at the bench's launch shapes)."""
    try:
        with open(PMC_FILE) as fh:
            return json.load(fh)
    except (OSError, ValueError):
        return {}


def pmc_traffic(pmc, target, stage, symbols, launch_batch):
    """HBM bytes of one run of ``stage`` (its launches, ``symbols`` in order) at
    ``launch_batch`` shots from the PMC record, or (None, reason) when there is no record or
    it was taken on different kernels than the ones just timed (symbol mismatch: the
    counters would describe code that no longer runs)."""
    if isinstance(symbols, str):
        symbols = [symbols]
    rec = pmc.get(target, {}).get(stage)
    if rec is None:
        return None, f"no PMC record for {target}/{stage}"
    if list(rec.get("symbols", [])) != list(symbols):
        rs = list(rec.get("symbols", []))
        uniq = lambda xs: sorted(set(xs), key=xs.index)  # noqa: E731
        msg = (f"PMC record for {target}/{stage} is of {len(rs)} launches {uniq(rs)}, the timed "
               f"run made {len(symbols)} launches {uniq(list(symbols))}: traffic withheld "
               f"(rerun tools/pmc_refresh.sh)")
        print(f"[bench] WARNING: {msg}", file=sys.stderr)
        return None, msg
    return rec["hbm_bytes"] * launch_batch / rec["batch"], None


# ------------------------------------------------------------------ CPU baseline
def _cpu_worker(shots):
    os.environ["OMP_NUM_THREADS"] = "1"
    os.environ["OPENBLAS_NUM_THREADS"] = "1"
    import torch

    torch.set_num_threads(1)
    from oracle import autoencoder as ora
    from oracle import svd as osvd
    from oracle.spectrogram import specgr_scipy

    spec = ae_layers()
    params, it = [], iter(ae_weights())
    for lay in spec:
        params.append(None if lay[0] == "pool" else
                      {"W": torch.from_numpy(next(it)), "b": torch.from_numpy(next(it))})
    for x in shots:
        S, _, _ = specgr_scipy(x, SPEC5)
        D = osvd.denoiseSignal(S)
        with torch.no_grad():
            ora.forward(spec, params, torch.from_numpy(D.astype(np.float32))[None, :, :, None])
    return len(shots)


def host_cpu_share():
    """(worker count, where it came from): the CPU bandwidth this job may use — the cgroup
    quota (v2 cpu.max or v1 cfs_quota_us / cfs_period_us), capped by the affinity mask and
    by OMP_NUM_THREADS when the launcher sets it (the GPU box: 16 per GPU) — never the whole
    machine that sched_getaffinity alone reports there."""
    affinity = len(os.sched_getaffinity(0))
    share, src = affinity, f"sched_getaffinity ({affinity})"
    quota = None
    try:
        with open("/sys/fs/cgroup/cpu.max") as fh:
            q, per = fh.read().split()[:2]
            if q != "max":
                quota = float(q) / float(per)
    except (OSError, ValueError):
        try:
            with open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us") as fh:
                q = float(fh.read())
            with open("/sys/fs/cgroup/cpu/cpu.cfs_period_us") as fh:
                per = float(fh.read())
            if q > 0:
                quota = q / per
        except (OSError, ValueError):
            pass
    if quota is not None and int(quota) < share:
        share, src = max(1, int(quota)), f"cgroup cpu quota ({quota:g} CPUs)"
    omp = os.environ.get("OMP_NUM_THREADS", "")
    if omp.isdigit() and 0 < int(omp) < share:
        share, src = int(omp), f"OMP_NUM_THREADS={omp} (launcher's per-job CPU share)"
    return share, src


def cpu_baseline(n_shots: int) -> dict:
    """The C5 chain on the host: one shot per task, one thread per worker, all cores."""
    from specenh.synthetic import plasma_chirps

    cores, cores_src = host_cpu_share()
    x = plasma_chirps(n_shots, L5, seed0=0, dtype=np.float16).astype(np.float64)
    chunks = [x[i::cores] for i in range(cores)]
    # one BLAS/OpenMP thread per worker, set before the workers import numpy/torch
    saved = {k: os.environ.get(k) for k in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS",
                                             "MKL_NUM_THREADS")}
    os.environ.update({k: "1" for k in saved})
    ctx = mp.get_context("spawn")  # fresh interpreters: never touch the GPU
    try:
        pool = ctx.Pool(cores)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    with pool:
        pool.map(_cpu_worker, [c[:1] for c in chunks])  # warm imports
        t0 = time.perf_counter()
        done = sum(pool.map(_cpu_worker, chunks))
        dt = time.perf_counter() - t0
    return {"value": done / dt, "unit": "spectrograms/s", "cores": cores, "kind": "port",
            "cores_source": cores_src,
            "sample": f"{done} shots x {L5} fp16 samples: scipy.signal.spectrogram (256 hann/"
                      f"hop 128, linear detrend) + log + min-max + drop row, numpy SVD "
                      f"denoiseSignal default, torch-CPU fp32 autoencoder forward; {cores} "
                      f"worker processes x 1 thread, {dt:.2f} s wall"}


# ------------------------------------------------------------------ C3 / C4 stages
FP32_MFMA_PEAK_TFLOPS = 157.3        # v_mfma_f32_16x16x4_f32 / 32x32x2 (= the FP32 vector rate)


def c3_matrices(dev, B=4096, m=513, n=256, k=16, seed=3):
    """B gapped m x n fp32 matrices: 16 components 10 * 0.8^i along random orthonormal
    directions (QR of Gaussian matrices, on the host: the device QR library does not run
    under rocprofv3 --pmc) + Gaussian noise (singular values ~0.003-0.017)."""
    import torch
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    gh = torch.Generator()
    gh.manual_seed(seed)
    A = torch.empty((B, m, n), dtype=torch.float32, device=dev)
    s_sig = 10.0 * 0.8 ** torch.arange(k, device=dev, dtype=torch.float32)
    for b0 in range(0, B, 512):
        b1 = min(B, b0 + 512)
        U = torch.linalg.qr(torch.randn((b1 - b0, m, k), generator=gh)).Q.to(dev)
        V = torch.linalg.qr(torch.randn((b1 - b0, n, k), generator=gh)).Q.to(dev)
        A[b0:b1] = (U * s_sig) @ V.transpose(1, 2) + \
            (0.01 / m ** 0.5) * torch.randn((b1 - b0, m, n), generator=g, device=dev)
        del U, V
    return A


def svd_c3_stage(dev, B=4096, m=513, n=256, k=16, reps=5, pmc=None):
    """BASELINE config 3: denoiseSignal on 4096 gapped 513 x 256 fp32 matrices, rank-16
    (start 0, stop 16) and the default (1, r). Matrices: 16 signal components 10 * 0.8^i
    along random orthonormal directions + Gaussian noise of
    singular values ~0.003-0.017 (SURVEY.md §8 d: the gap sits at the cut; orthonormal
    directions from a QR of Gaussian matrices, so the signal spectrum is exact). Roofline
    (SURVEY §8 d C3): 2mn^2 + 4mnk = 75.6 MFLOP per matrix at the fp32 MFMA peak; HBM floor
    8mn bytes (read A, write the reconstruction)."""
    import torch
    from specenh import _lib, svd
    A = c3_matrices(dev, B, m, n, k)
    out = torch.empty_like(A)
    st = torch.cuda.current_stream(dev)
    res = {"workload": f"{B} x {m} x {n} fp32 gapped matrices (rank 16 + noise)"}
    flop = 2.0 * m * n * n + 4.0 * m * n * k
    for name, (lo, hi) in {"rank16": (0, 16), "default": (None, None)}.items():
        for _ in range(2):
            c0 = _lib.launch_count()
            svd.denoise_batch(A, lo, hi, out=out)
            syms = _lib.kernel_names(c0, _lib.launch_count())
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(reps):
            svd.denoise_batch(A, lo, hi, out=out)
        e1.record(st)
        e1.synchronize()
        ms = e0.elapsed_time(e1) / reps
        fl = flop if name == "rank16" else 2.0 * m * n * n + 4.0 * m * n  # K = 1
        ach = fl * B / (ms * 1e-3) / 1e12
        # accuracy on sampled matrices of the timed batch: the notebook's arithmetic
        # (numpy thin SVD in float64, components [lo, hi); denoising_by_svd.ipynb:209-228)
        # on the same fp32 matrices vs the output of the last timed launch
        rels = []
        for b in np.linspace(0, B - 1, 6).astype(int):
            a64 = A[b].double().cpu().numpy()
            u, sv, vh = np.linalg.svd(a64, full_matrices=False)
            l0, h0 = (0, 16) if name == "rank16" else (1, len(sv))
            ref = (u[:, l0:h0] * sv[l0:h0]) @ vh[l0:h0]
            rels.append(float(np.linalg.norm(out[b].double().cpu().numpy() - ref) /
                              np.linalg.norm(ref)))
        acc = {"rel_fro_max": max(rels), "tol": 1e-5, "pass": max(rels) <= 1e-5,
               "matrices": 6, "reference": "numpy float64 thin SVD of the same fp32 matrices"}
        if not acc["pass"]:
            print(f"[bench] C3 {name} ACCURACY CHECK FAILED: {max(rels):.3e}", file=sys.stderr)
        # measured HBM bytes of the whole denoise call (tools/pmc_refresh.sh c3), vs the
        # 8 m n B floor of reading A and writing the reconstruction
        tr, why = pmc_traffic(pmc or {}, "c3", f"svd_c3_{name}", syms, B)
        res[name] = {"ms": ms, "matrices_per_s": B / (ms * 1e-3), "accuracy": acc,
                     "kernels": sorted(set(syms), key=syms.index),
                     "traffic": tr, "traffic_floor": 8.0 * m * n * B,
                     **({"traffic_note": why} if why else {}),
                     "roofline": {"bound": "mfma_fp32", "achieved": ach,
                                  "peak": FP32_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
                                  "frac": ach / FP32_MFMA_PEAK_TFLOPS,
                                  "flops_per_matrix": fl,
                                  "hbm_floor_ms": 8.0 * m * n * B / (HBM_PEAK_GBPS * 1e9) * 1e3}}
    del A, out
    return res


def ae_ops():
    from specenh import ae
    return [ae.PoolOp() if lay[0] == "pool" else
            ae.ConvOp(lay[0], lay[1], lay[2], lay[3], lay[4], stride=2 if lay[0] == "convT" else 1)
            for lay in ae_layers()]


def make_c5_engine(dev, dtype="float16", out_fp16=True):
    """The C5 model (manual_scan_3layers.py:186-199) with the trained weights. Inference
    output: fp16 reconstructions (32,768 B out per shot), stored by the
    fused three-layer decoder."""
    import torch
    from specenh import ae
    eng = ae.AutoencoderEngine(ae_ops(), (HW5, HW5, 1), compute_dtype=dtype, device=dev)
    eng.set_keras_weights(ae_weights())
    if out_fp16 and eng.dec3:
        eng.set_inference_output_dtype(torch.float16)
    return eng


def c4_engine_and_batch(dev, batch=128, n=None, seed=4):
    """A mixed_bfloat16 engine of the reference model and one C4 batch (device pairs,
    specenh.synthetic.c4_pairs_torch), plus the whole device set when ``n`` is given."""
    import torch
    from specenh.synthetic import c4_pairs_torch
    eng = make_c5_engine(dev, "mixed_bfloat16")
    X, Y = c4_pairs_torch(n or batch, seed=seed, device=dev, dtype=torch.bfloat16)
    if n is None:
        return eng, X, Y
    return eng, X, Y, X[:batch], Y[:batch]


def ae_train_c4_stage(dev, dist=None, batch=128, steps=20, n_local=4096, seed=4, make=None,
                      sync=None):
    """BASELINE config 4: Keras fit() steps of the 3-layer model on the C4 workload (SURVEY
    §8 d: C1 spectrograms of seeded noisy chirps -> the noise-free chirps' spectrograms,
    generated on the device), mixed_bfloat16 (bf16 MFMA, fp32 master weights + Adam):
    forward, BCE from logits, backward (dgrad + deterministic wgrad), Adam. Each step draws
    the next ``batch`` samples of a per-epoch permutation of this rank's ``n_local`` pairs.

    Under torch.distributed (``dist``: every rank runs this stage) the flat fp32 gradient is
    SUM-all-reduced over RCCL in two buckets before Adam (specenh.ae.dp_backward, SURVEY §8
    E2), in two modes: per-GPU batch ``batch`` (global batch = batch x world: the scaling
    configuration) and global batch ``batch`` (batch / world per rank: Keras parity).
    Reported: global samples/s (all ranks' samples / max-over-ranks time), ms per step, and
    the standalone all-reduce time of the gradient buffer with its share of the step.
    1.494 GFLOP per sample (SURVEY §8 d C4: forward x 3) at the dense bf16 MFMA peak.

    ``make(rank) -> (engine, X, Y)`` and ``sync()`` replace the HIP engine / C4 pairs and
    torch.cuda.synchronize (tests/test_bench_dist_cpu.py runs this orchestration on gloo
    with the oracle's CPU engine)."""
    import torch
    world = dist.get_world_size() if dist else 1
    rank = dist.get_rank() if dist else 0
    group = dist.group.WORLD if dist else None
    if make is None:
        eng, X, Y, _, _ = c4_engine_and_batch(dev, batch, n=n_local, seed=seed + 7919 * rank)
    else:
        eng, X, Y = make(rank)
    n_local = X.shape[0]
    sync = sync or torch.cuda.synchronize
    if dist:
        eng.sync_state(group)
    g = torch.Generator(device=dev)
    g.manual_seed(seed)  # the same permutation sequence on every rank (own data)

    def run(per_rank, nsteps):
        perm = torch.randperm(n_local, generator=g, device=dev)
        pos = 0
        for _ in range(nsteps):
            if pos + per_rank > n_local:
                perm = torch.randperm(n_local, generator=g, device=dev)
                pos = 0
            idx = perm[pos:pos + per_rank]
            pos += per_rank
            eng.train_step(X.index_select(0, idx), Y.index_select(0, idx), process_group=group)

    def timed(per_rank):
        run(per_rank, 3)
        if dist:
            dist.barrier()
        sync()
        t0 = time.perf_counter()
        run(per_rank, steps)
        sync()
        el = max_over_ranks(time.perf_counter() - t0, dist, dev)
        return el / steps

    fl = 3.0 * ae_flops_per_sample()
    modes = {"per_gpu_batch": batch}
    if dist and world > 1 and batch % world == 0:
        modes["global_batch"] = batch // world
    res = {"workload": f"fit steps on {n_local} device C4 pairs per rank (128x128x1 noisy "
                       f"chirp spectrogram -> clean), mixed_bfloat16, Adam, world {world}",
           "world": world}
    for mode, per in modes.items():
        sec = timed(per)
        ach = fl * per * world / sec / 1e12
        res[mode] = {"samples_per_rank": per, "global_batch": per * world,
                     "ms_per_step": sec * 1e3, "samples_per_s": per * world / sec,
                     "roofline": {"bound": "mfma", "achieved": ach,
                                  "peak": MFMA_PEAK_TFLOPS * world, "unit": "TFLOP/s",
                                  "frac": ach / (MFMA_PEAK_TFLOPS * world),
                                  "flops_per_step": fl * per * world}}
    if dist:  # the gradient exchange alone (both buckets, the flat fp32 buffer)
        for _ in range(3):
            dist.all_reduce(eng.g)
        sync()
        t0 = time.perf_counter()
        for _ in range(20):
            dist.all_reduce(eng.g)
        sync()
        ar = max_over_ranks(time.perf_counter() - t0, dist, dev) / 20
        res["allreduce"] = {"bytes": eng.g.numel() * 4, "ms": ar * 1e3,
                            "share_of_step": ar * 1e3 / res["per_gpu_batch"]["ms_per_step"]}
    del X, Y
    return res


def c5_host_stream_stage(dev, make_engine, shots=32768, chunk=2048, slots=4):
    """BASELINE config 5 as a stream from host memory (SURVEY.md §7 item 7, §8 d C5: "1M
    shots streamed"): fp16 samples in pinned host memory -> H2D -> specgr -> denoiseSignal
    -> fp16 autoencoder -> D2H of the fp32 reconstructions into pinned host memory.
    ``slots`` HIP streams each own one chunk's device buffers and run H2D, the chain and D2H
    in order, so one slot's copies (the two DMA directions) overlap the other slots' kernels.
    This is the PCIe-inclusive rate; the headline ``value`` keeps the inputs in HBM."""
    import torch
    from specenh import pipeline_data, svd
    from specenh.synthetic import plasma_chirps_torch

    n_chunks = shots // chunk
    shots = n_chunks * chunk
    host_x = torch.empty((shots, L5), dtype=torch.float16, pin_memory=True)
    probe = make_engine()
    host_y = torch.empty((shots, HW5, HW5, 1), dtype=probe.infer_out_dtype, pin_memory=True)
    del probe
    for c in range(n_chunks):  # distinct seeded shots, synthesised on the device
        host_x[c * chunk:(c + 1) * chunk].copy_(
            plasma_chirps_torch(chunk, L5, seed=5000 + c, device=dev).to(torch.float16))
    torch.cuda.synchronize()
    sl = []
    for _ in range(slots):
        sl.append({"s": torch.cuda.Stream(dev), "eng": make_engine(),
                   "x": torch.empty((chunk, L5), dtype=torch.float16, device=dev),
                   "S": torch.empty((chunk, HW5, HW5), dtype=torch.float32, device=dev),
                   "A": torch.empty((chunk, HW5, HW5, 1), dtype=torch.float16, device=dev)})

    def run(n):
        for c in range(n):
            s = sl[c % slots]
            rows = slice(c * chunk, (c + 1) * chunk)
            with torch.cuda.stream(s["s"]):
                s["x"].copy_(host_x[rows], non_blocking=True)
                pipeline_data.specgr_batch(s["x"], SPEC5, out=s["S"])
                svd.denoise_batch(s["S"], out=s["A"].view(chunk, HW5, HW5))
                y = s["eng"].forward(s["A"])
                host_y[rows].copy_(y, non_blocking=True)

    run(min(n_chunks, 2 * slots))  # warm-up (engine buffers, plans)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run(n_chunks)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0

    # the two copy directions alone, for the PCIe context of the figure above
    dx = torch.empty((chunk * 4, L5), dtype=torch.float16, device=dev)
    dy = torch.empty((chunk * 4, HW5 * HW5), dtype=host_y.dtype, device=dev)
    bw = {}
    for name, (dst, src) in {"h2d": (dx, host_x[:chunk * 4]),
                             "d2h": (host_y[:chunk * 4].view(chunk * 4, -1), dy)}.items():
        dst.copy_(src, non_blocking=True)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for _ in range(5):
            dst.copy_(src, non_blocking=True)
        torch.cuda.synchronize()
        bw[name] = 5 * src.numel() * src.element_size() / (time.perf_counter() - t1) / 1e9
    # both directions at once on two streams (the stream's real copy ceiling: the shots'
    # H2D and D2H bytes move concurrently)
    in_b, out_b = 2 * L5, host_y.element_size() * HW5 * HW5
    s_in, s_out = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    hx, hy = host_x[:chunk * 4], host_y[:chunk * 4].view(chunk * 4, -1)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    for _ in range(5):
        with torch.cuda.stream(s_in):
            dx.copy_(hx, non_blocking=True)
        with torch.cuda.stream(s_out):
            hy.copy_(dy, non_blocking=True)
    torch.cuda.synchronize()
    t_bi = (time.perf_counter() - t1) / 5
    bw["h2d_with_d2h"] = hx.numel() * hx.element_size() / t_bi / 1e9
    bw["d2h_with_h2d"] = hy.numel() * hy.element_size() / t_bi / 1e9
    ceiling = chunk * 4 / t_bi  # shots/s the copies alone allow, both directions concurrent
    rate = shots / dt
    del sl, dx, dy
    return {"workload": f"{shots} shots streamed from pinned host memory in {chunk}-shot "
                        f"chunks over {slots} HIP streams (H2D fp16 samples, chain, D2H "
                        f"{str(host_y.dtype).replace('torch.', '')} reconstructions)",
            "spectrograms_per_s": rate, "ms": dt * 1e3,
            "h2d_bytes_per_shot": in_b, "d2h_bytes_per_shot": out_b,
            "h2d_GBps_achieved": rate * in_b / 1e9, "d2h_GBps_achieved": rate * out_b / 1e9,
            "copy_only_GBps": bw, "copy_ceiling_shots_per_s": ceiling,
            "frac_of_copy_ceiling": rate / ceiling}


# ------------------------------------------------------------------ multi-GPU plumbing
def shard(world: int, rank: int, batch: int) -> dict:
    """Weak scaling: every rank owns `batch` shots of its own, the global
    shot ids [rank * batch, (rank + 1) * batch), synthesised from a per-rank seed. Shots are
    independent, so there is no collective in the data path."""
    return {"seed": 1000 + rank, "first_shot": rank * batch, "shots": batch}


def max_over_ranks(elapsed: float, dist=None, device=None) -> float:
    """The slowest rank's wall time of the timed region (the job is done when it is)."""
    if dist is None:
        return elapsed
    import torch
    t = torch.tensor([elapsed], dtype=torch.float64, device=device)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t.item())


def throughput(world: int, batch: int, steps: int, elapsed: float) -> float:
    """Whole-job spectrograms/s: every rank's shots of every timed step / the max time."""
    return world * batch * steps / elapsed


# ------------------------------------------------------------------ --dump-outputs
DUMP_MAX_SHOTS = 512  # x 128 x 128 float32 = 32 MiB per file (one file per rank)


def dump_outputs(dirname, Y, rank=0):
    """Write the reconstructions the last timed step returned (``Y``: the step's tensor, or
    its per-stream slices in shot order) as float32 [n, 128, 128, 1]: every shot of a batch
    up to DUMP_MAX_SHOTS, else the sorted shots of a fixed seeded draw (the same shots in
    every run with the same --batch). Rank 0 writes reconstructions.npy, rank r > 0
    reconstructions_rank<r>.npy (its own shard)."""
    import torch
    if isinstance(Y, (list, tuple)):
        Y = torch.cat(list(Y))
    n = Y.shape[0]
    if n > DUMP_MAX_SHOTS:
        pick = np.sort(np.random.default_rng(20240).choice(n, DUMP_MAX_SHOTS, replace=False))
        Y = Y.index_select(0, torch.as_tensor(pick, device=Y.device))
    os.makedirs(dirname, exist_ok=True)
    name = "reconstructions.npy" if rank == 0 else f"reconstructions_rank{rank}.npy"
    np.save(os.path.join(dirname, name), Y.float().cpu().numpy())


# ------------------------------------------------------------------ GPU
def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--cpu-shots", type=int, default=1024)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-stages", action="store_true")
    ap.add_argument("--streams", type=int, default=2,
                    help="HIP streams the batch is split over (staggered chains; 1 = serial)")
    ap.add_argument("--full", action="store_true",
                    help="also run the CPU baseline, the per-layer roofline, the C2/C3/C4/"
                         "host-stream stages and the accuracy check (a plain run only times "
                         "the steps)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's reconstructions to DIR/*.npy (float32)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))

    # rank 0 times the CPU reference at every world size, before anything touches the GPU
    # (the other ranks wait in the process-group rendezvous), so a scaling line at N > 1
    # carries the same baseline as N = 1
    cpu = None
    if args.full and rank == 0 and not args.no_cpu_baseline:
        cpu = cpu_baseline(args.cpu_shots)

    import torch
    import torch.distributed as dist

    from specenh import _lib, ae, pipeline_data, svd
    from specenh.synthetic import plasma_chirps_torch

    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    # launched by torch.distributed.run (any world size, 1 included): RCCL process group
    use_dist = world > 1 or ("MASTER_ADDR" in os.environ and "RANK" in os.environ)
    if use_dist:
        dist.init_process_group("nccl", device_id=dev)
    L = _lib.lib()

    B = args.batch
    mine = shard(world, rank, B)
    x16 = plasma_chirps_torch(B, L5, seed=mine["seed"], device=dev).to(torch.float16)
    S = torch.empty((B, HW5, HW5), dtype=torch.float32, device=dev)
    A = torch.empty((B, HW5, HW5, 1), dtype=torch.float16, device=dev)
    eng = make_c5_engine(dev)
    torch.cuda.synchronize()

    NS = max(1, args.streams) if B % max(1, args.streams) == 0 else 1
    Hs = B // NS  # shots per launch in the timed step (one slice per stream)

    # One slice (Hs shots) through each stage: the launch configuration of the timed step,
    # used for the per-layer roofline and the stage breakdown, so that every launch of the
    # run has one shape and rocprofv3's per-kernel averages match the fields below.
    def stage_stft():
        pipeline_data.specgr_batch(x16[:Hs], SPEC5, out=S[:Hs])

    def stage_svd():  # fp32 SVD, reconstruction stored as the autoencoder's fp16 input
        svd.denoise_batch(S[:Hs], out=A[:Hs].view(Hs, HW5, HW5))

    def stage_ae(timing=None, kernels=None):
        return eng.forward(A[:Hs], timing=timing, kernels=kernels)

    # The timed step: the batch splits into NS slices, each running the whole chain on its
    # own HIP stream with its own autoencoder buffers. Slice h > 0 starts once slice h-1's
    # SVD is done, so its latency-bound STFT/SVD kernels co-run with the conv layers of
    # the slice ahead (and, with no sync between steps, the next step's head overlaps this
    # step's tail). Every shot still goes through every stage inside the step.
    if NS > 1:
        sstreams = [torch.cuda.Stream(dev) for _ in range(NS)]
        sengs = [eng] + [make_c5_engine(dev) for _ in range(NS - 1)]
        sdone = [torch.cuda.Event() for _ in range(NS)]

    def step():
        if NS == 1:
            stage_stft()
            stage_svd()
            return stage_ae()
        outs = []
        for h in range(NS):
            s_h = sstreams[h]
            if h > 0:
                s_h.wait_event(sdone[h - 1])
            with torch.cuda.stream(s_h):
                sl = slice(h * Hs, (h + 1) * Hs)
                pipeline_data.specgr_batch(x16[sl], SPEC5, out=S[sl])
                svd.denoise_batch(S[sl], out=A[sl].view(Hs, HW5, HW5))
                sdone[h].record(s_h)
                outs.append(sengs[h].forward(A[sl]))
        # no join with the current stream here: step i+1's slices queue behind step i's on
        # their own streams; the barrier (device-wide synchronize) closes the timed region
        return outs

    for _ in range(args.warmup):
        step()

    def barrier():
        if use_dist:
            dist.barrier()
        torch.cuda.synchronize()

    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        last = step()
    barrier()
    elapsed = max_over_ranks(time.perf_counter() - t0, dist if use_dist else None, dev)

    # the last timed step's reconstructions, before any other leg reuses the engines' buffers
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, last, rank)
    del last

    res = {
        "metric": METRIC,
        "value": throughput(world, B, args.steps, elapsed),
        "unit": "spectrograms/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": 1e3 * elapsed / args.steps,
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "fp16",
        "full": args.full,
        "data": "synthetic (seeded plasma chirps + noise + drift, generated on device, fp16); "
                "autoencoder weights trained on synthetic C4 data by the CPU oracle "
                "(tests/golden/ae_c4_trained.npz; no reference checkpoint exists)",
        "config": {"workload": "BASELINE config 5 per GPU: end-to-end STFT -> SVD -> "
                               "autoencoder-denoise inference stream, 16,512-sample fp16 "
                               "shots -> specgr 128x128 (256 hann / hop 128) -> "
                               "denoiseSignal default -> 3-layer conv AE (16/32/64, 5x5) "
                               "fp16 forward -> fp16 reconstructions (32,768 B per shot)",
                   "shots_per_step": B, "shots_per_launch": Hs, "samples": L5, "stft_dtype": "fp32",
                   "svd_dtype": "fp32 (fp64 small algebra)", "ae_dtype": "fp16",
                   "parallelism": f"shot-sharded x{world}", "streams_per_gpu": NS},
    }
    if not args.full:  # a plain run ends here: the legs below are --full's
        if use_dist:
            dist.barrier()
            dist.destroy_process_group()
        if rank == 0:
            res.update({"roofline": None, "cpu_baseline": None, "psnr_db": None,
                        "accuracy": None, "stages": None})
            print(json.dumps(res))
        return

    # ---- dominant kernel: conv_fwd_kernel, every conv launch bracketed by HIP events on
    # the stream it is launched on ----
    reps = max(3, args.steps)
    conv_ms = []
    for _ in range(reps):
        stage_stft()
        stage_svd()
        timing, kernels = [], []
        stage_ae(timing, kernels)
        torch.cuda.synchronize()
        conv_ms.append([a.elapsed_time(b) for a, b in timing])
    conv_ms = np.array(conv_ms)                       # [reps, launches]
    layer_ms = np.median(conv_ms, axis=0)
    pmc = load_pmc()
    layers = []
    names = layer_names(eng)
    out_bytes = torch.empty((), dtype=eng.infer_out_dtype).element_size()
    for name, c, ms, sym in zip(names, ae_layer_costs(out_bytes=out_bytes, tail=eng.tail,
                                                      dec3=eng.dec3,
                                                      enc2=getattr(eng, "enc2", False)), layer_ms,
                                kernels):
        # compute floor: MFMA FLOPs at the dense fp16 MFMA peak + VALU FLOPs at the dot2 peak
        t_c = c["mfma_flops"] * Hs / (MFMA_PEAK_TFLOPS * 1e12) + \
            (c["flops"] - c["mfma_flops"]) * Hs / (VALU_DOT2_PEAK_TFLOPS * 1e12)
        nb = c["bytes"] * Hs + c["weight_bytes"]
        t_m = nb / (HBM_PEAK_GBPS * 1e9)
        if t_m >= t_c:
            ach = nb / (ms * 1e-3) / 1e9
            rl = {"bound": "hbm", "achieved": ach, "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                  "frac": ach / HBM_PEAK_GBPS}
        else:
            # the FLOP-mix peak: this launch's FLOPs over its compute floor (= the MFMA peak
            # for a pure-MFMA layer, the dot2 peak for a pure-VALU one)
            peak_c = c["flops"] * Hs / t_c / 1e12
            ach = c["flops"] * Hs / (ms * 1e-3) / 1e12
            rl = {"bound": "mfma" if c["mfma_flops"] else "valu", "achieved": ach,
                  "peak": peak_c, "unit": "TFLOP/s", "frac": ach / peak_c}
        tr, why = pmc_traffic(pmc, "c5", name, sym, Hs)
        rl.update({"layer": name, "kernel": sym, "kernel_ms": float(ms),
                   "alg_bytes_per_launch": nb, "flops_per_launch": c["flops"] * Hs,
                   "mfma_flops_per_launch": c["mfma_flops"] * Hs,
                   # PMC passes (tools/pmc_refresh.sh) ran the same kernel at the bench's
                   # launch shape; traffic is per launch of Hs shots
                   "traffic": tr, "traffic_ratio": tr / nb if tr else None})
        if why:
            rl["traffic_note"] = why
        layers.append(rl)
    dom = layers[int(np.argmax(layer_ms))]

    # ---- BASELINE config 4 (training) on every rank: data-parallel over RCCL under
    # torchrun, rank-local otherwise ----
    c4 = None
    if not args.no_stages:
        c4 = ae_train_c4_stage(dev, dist if use_dist else None)

    # ---- per-stage breakdown of one step (events between stages) ----
    stages = None
    if rank == 0 and not args.no_stages:
        st = torch.cuda.current_stream(dev)
        evs = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        acc = np.zeros(3)
        for _ in range(reps):
            evs[0].record(st); stage_stft()
            evs[1].record(st); stage_svd()
            evs[2].record(st); stage_ae()
            evs[3].record(st)
            evs[3].synchronize()
            acc += [evs[i].elapsed_time(evs[i + 1]) for i in range(3)]
        acc /= reps
        stages = {"shots_per_launch": Hs,
                  "ms": dict(zip(["stft_specgr_f16in", "svd_denoise_to_f16",
                                  "ae_forward"], acc.round(4).tolist())),
                  "conv_ms_per_layer": layer_ms.round(4).tolist(),
                  "ae_layers": layers}
        # C2: the STFT-only configuration (BASELINE config 2) and its HBM roofline
        B2 = 4096
        x2 = plasma_chirps_torch(B2, L2, seed=7, device=dev)
        o2 = torch.empty((B2, F2, T2), dtype=torch.float32, device=dev)
        for _ in range(2):
            c0 = _lib.launch_count()
            pipeline_data.specgr_batch(x2, SPEC2, out=o2)
            syms2 = _lib.kernel_names(c0, _lib.launch_count())
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(5):
            pipeline_data.specgr_batch(x2, SPEC2, out=o2)
        e1.record(st)
        e1.synchronize()
        k_ms = e0.elapsed_time(e1) / 5
        ach2 = ALG_BYTES_C2 * B2 / (k_ms * 1e-3) / 1e9
        tr2, why2 = pmc_traffic(pmc, "c2", "stft_c2", syms2, B2)
        stages["stft_c2"] = {
            "workload": "4096 x 65536 fp32, nperseg 1024 hop 256 hamm, linear, density, "
                        "log + min-max + drop Nyquist -> 4096 x 512 x 253",
            "spectrograms_per_s": B2 / (k_ms * 1e-3), "kernels": syms2,
            "kernel_ms": k_ms, "roofline": {"bound": "hbm", "achieved": ach2,
                                            "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                                            "frac": ach2 / HBM_PEAK_GBPS,
                                            "alg_bytes_per_launch": ALG_BYTES_C2 * B2,
                                            "traffic": tr2, "traffic_note": why2}}
        del o2
        # §8 A4 / f3: cross-power amplitude spectrogram of shot pairs at the C2 geometry
        from specenh import cross
        Bc = B2 // 2
        xa, xb_ = x2[:Bc], x2[Bc:]
        for _ in range(2):
            c0 = _lib.launch_count()
            _, _, oc = cross.cross_spectrogram_batch(xa, xb_, 5e5, "hamm", 1024, 768, "linear",
                                                     "density", amplitude=True)
            symsc = _lib.kernel_names(c0, _lib.launch_count())
        e0.record(st)
        for _ in range(5):
            _, _, oc = cross.cross_spectrogram_batch(xa, xb_, 5e5, "hamm", 1024, 768, "linear",
                                                     "density", amplitude=True)
        e1.record(st)
        e1.synchronize()
        c_ms = e0.elapsed_time(e1) / 5
        algc = (2 * 4 * L2 + 4 * (F2 + 1) * T2) * Bc
        achc = algc / (c_ms * 1e-3) / 1e9
        trc, whyc = pmc_traffic(pmc, "csd", "csd_c2", symsc, Bc)
        stages["csd_c2"] = {
            "workload": f"{Bc} signal pairs x 65536 fp32, nperseg 1024 hop 256 hamm, linear, "
                        "density -> |Pxy| amplitude [pairs, 513, 253] (crosspowerspec.py:39)",
            "pairs_per_s": Bc / (c_ms * 1e-3), "kernels": symsc, "kernel_ms": c_ms,
            "roofline": {"bound": "hbm", "achieved": achc, "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                         "frac": achc / HBM_PEAK_GBPS, "alg_bytes_per_launch": algc,
                         "traffic": trc, "traffic_note": whyc}}
        del x2, oc
        stages["svd_c3"] = svd_c3_stage(dev, pmc=pmc)
        stages["ae_train_c4"] = c4
        stages["c5_host_stream"] = c5_host_stream_stage(dev, lambda: make_c5_engine(dev))

    # ---- accuracy vs the fp64 CPU chain on sample shots ----
    accuracy = None
    if rank == 0:
        from oracle import autoencoder as ora
        from oracle import checks
        from oracle import svd as osvd
        from oracle.spectrogram import specgr_arrays

        Y = step()
        torch.cuda.synchronize()
        if isinstance(Y, list):  # per-stream slices, in shot order
            Y = torch.cat(Y)
        spec = ae_layers()
        params, it = [], iter(ae_weights())
        for lay in spec:
            params.append(None if lay[0] == "pool" else
                          {"W": torch.from_numpy(next(it)).double(),
                           "b": torch.from_numpy(next(it)).double()})
        rels, got_all, ref_all = [], [], []
        for b in np.linspace(0, B - 1, 8).astype(int):
            Sx, _, _ = specgr_arrays(x16[b].double().cpu().numpy(), SPEC5)
            Dx = osvd.denoiseSignal(Sx)
            with torch.no_grad():
                ref = ora.forward(spec, params, torch.from_numpy(Dx)[None, :, :, None]).numpy()[0]
            got = Y[b].double().cpu().numpy()
            rels.append(checks.out_rel(got, ref))
            got_all.append(got)
            ref_all.append(ref)
        tol = checks.TOL["float16"]["out_rel"]
        accuracy = {"out_rel_max": max(rels), "out_rel_tol": tol, "pass": max(rels) <= tol,
                    "psnr_db": checks.signal_psnr_db(np.stack(got_all), np.stack(ref_all)),
                    "ref_output_std": float(np.std(np.stack(ref_all))),
                    "shots": 8, "reference": "fp64 CPU chain: scipy-semantics specgr -> numpy "
                                             "SVD denoiseSignal -> fp64 autoencoder restatement"}
        if not accuracy["pass"]:
            print(f"[bench] ACCURACY CHECK FAILED: out_rel {max(rels):.3e} > {tol}",
                  file=sys.stderr)

    if use_dist:
        dist.barrier()
        dist.destroy_process_group()
    if rank != 0:
        return

    res.update({
        "roofline": {k: dom[k] for k in ("bound", "achieved", "peak", "unit", "frac",
                                           "traffic")} |
                    {"layer": f"{dom['layer']} launch of the autoencoder forward",
                     "kernel": dom["kernel"],
                     "kernel_ms": dom["kernel_ms"], "alg_bytes_per_launch":
                     dom["alg_bytes_per_launch"], "flops_per_launch": dom["flops_per_launch"],
                     "traffic_ratio": dom["traffic_ratio"],
                     "traffic_source": os.path.relpath(PMC_FILE, REPO) + " (tools/pmc_refresh.sh: "
                                       "rocprofv3 --pmc FETCH_SIZE x2 + WRITE_SIZE, separate "
                                       "passes, the same kernel symbol at the same launch shape)"}
                    | ({"traffic_note": dom["traffic_note"]} if "traffic_note" in dom else {}),
        "cpu_baseline": cpu,
        "psnr_db": accuracy["psnr_db"] if accuracy else None,
        "accuracy": accuracy,
        "stages": stages,
    })
    print(json.dumps(res))


if __name__ == "__main__":
    main()
