"""Time the array mode decomposition (csrc/herm_eig.hip: batched Hermitian Jacobi, one wave
per matrix) on the shapes of profiles/csm.json (nperseg 1024 / noverlap 768 hamm, linear
detrend, density), for k = 1 and k = 4 leading modes, in one process:

  herm_eig     torch.ops.specenh.herm_eig_out alone on the resident cross-spectral matrices
  array_modes  specenh.spectral.array_modes whole (CSM + eigensolver per batch slice)
  csm          specenh.spectral.cross_spectral_matrix(want=("csm",)) alone
  eigh         the baseline, torch.linalg.eigh on the same CSM tensor (all C eigenvectors)

HIP events around each route, 3 warm-ups, interleaved rounds, median (and min). The baseline
does not depend on k and runs beside the k = 1 routes. When torch.linalg.eigh raises (or runs
out of memory) at a shape the message is recorded and the baseline is timed on the largest
leading slice that runs (halving). The baseline is also far slower than anything else here
(about 0.8 ms a matrix at C = 40), so a slice is halved as well while one call, projected from
a timed probe of 512 matrices, would take more than EIGH_CALL_S seconds, and a baseline call
above 1 s is timed over 1 warm-up and 3 rounds instead of 3 and --rounds. Nothing is scaled:
herm_eig is timed on that same slice too, and the ratio is formed on equal work only.
Also recorded: mean and max sweeps, the agreement of the two routes (eigenvalues over
lambda_1; where it exceeds 1e-5, both routes' error on the worst matrix against
numpy.linalg.eigh in complex128) and the kernel's resource usage
(-Rpass-analysis=kernel-resource-usage).
    python tools/modes_bench.py [--json PATH] [--rounds N]"""
import json
import statistics
import time

from benchlib import parse_args, resources, timed, write_json  # puts the package on sys.path

import torch
from specenh import _lib, spectral
from specenh.synthetic import plasma_chirps_torch

path, ROUNDS, _ = parse_args(11)
N, NOV, WIN, FS = 1024, 768, "hamm", 500000.0
WARM = 3
EIGH_CALL_S = 4.0
KW = dict(fs=FS, window=WIN, nperseg=N, noverlap=NOV, detrend="linear", scaling="density")
ops = torch.ops.specenh
# (label, B, C, L, navg)
SHAPES = [("B8 C40 L65536 navg0", 8, 40, 65536, 0),
          ("B8 C40 L65536 navg8", 8, 40, 65536, 8),
          ("B1 C40 L1048576 navg0", 1, 40, 1 << 20, 0),
          ("B8 C4 L65536 navg0", 8, 4, 65536, 0)]


def baseline_slice(S):
    """The largest leading slice (halving) of the flattened matrices on which
    torch.linalg.eigh runs within EIGH_CALL_S, the messages of the ones on which it raises,
    and the wall time of that call."""
    flat = S.reshape(-1, S.shape[-2], S.shape[-1])
    count, errors = flat.shape[0], []
    probe = min(512, count)
    try:
        torch.linalg.eigh(flat[:probe])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        torch.linalg.eigh(flat[:probe])
        torch.cuda.synchronize()
        each = (time.perf_counter() - t0) / probe
        while count > probe and count * each > EIGH_CALL_S:
            count //= 2
    except Exception as e:
        errors.append({"matrices": probe, "message": f"{type(e).__name__}: {str(e)[:300]}"})
    while count >= 1:
        try:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            torch.linalg.eigh(flat[:count])
            torch.cuda.synchronize()
            return flat[:count], errors, time.perf_counter() - t0
        except Exception as e:  # recorded, then a smaller slice
            errors.append({"matrices": count, "message": f"{type(e).__name__}: {str(e)[:300]}"})
            torch.cuda.empty_cache()
            count //= 2
    return None, errors, 0.0


res = {"plan": {"nperseg": N, "noverlap": NOV, "window": WIN, "detrend": "linear",
                "scaling": "density"}, "rounds": ROUNDS, "warmups": WARM,
       "max_sweeps": _lib.HERM_EIG_MAX_SWEEPS, "kernel_resources": resources("herm_eig.hip"),
       "shapes": {}}
print(json.dumps(res["kernel_resources"]), flush=True)
for label, B, C, L, navg in SHAPES:
    x = plasma_chirps_torch(B * C, L, seed=1, device="cuda").reshape(B, C, L)
    _, _, est = spectral.cross_spectral_matrix(x, navg=navg, want=("csm",), **KW)
    S = est["csm"]
    del est
    lead = tuple(S.shape[:-2])
    count = S.numel() // (C * C)
    w = torch.empty(lead + (C,), device="cuda")
    sw = torch.empty(lead, dtype=torch.int32, device="cuda")
    base, errors, first = baseline_slice(S)
    base_rounds = ROUNDS if first <= 1.0 else min(3, ROUNDS)
    print(f"{label:24s} {count} matrices; eigh on {0 if base is None else base.shape[0]}, "
          f"{first:.2f} s a call", flush=True)
    entry = {"batch": B, "channels": C, "length": L, "navg": navg, "groups": S.shape[2],
             "matrices": count, "csm_bytes": S.numel() * 8,
             "eigh_matrices": 0 if base is None else base.shape[0], "eigh_errors": errors,
             "eigh_rounds": base_rounds, "k": {}}
    for k in (1, 4):
        v = torch.empty(lead + (k, C), dtype=torch.complex64, device="cuda")
        runs = {"herm_eig": lambda: ops.herm_eig_out(S, k, w, v, None),
                "array_modes": lambda: spectral.array_modes(x, k=k, navg=navg, **KW),
                "csm": lambda: spectral.cross_spectral_matrix(x, navg=navg, want=("csm",), **KW)}
        if base is not None and k == 1:
            wsl = w.reshape(-1, C)[:base.shape[0]]
            vsl = v.reshape(-1, k, C)[:base.shape[0]]
            runs["herm_eig_on_eigh_slice"] = lambda: ops.herm_eig_out(base, 1, wsl, vsl, None)
            runs["eigh"] = lambda: torch.linalg.eigh(base)
        for name, fn in runs.items():
            for _ in range(WARM if name != "eigh" or base_rounds == ROUNDS else 1):
                fn()
        torch.cuda.synchronize()
        times = {name: [] for name in runs}
        for rnd in range(ROUNDS):  # interleaved: the routes see the same clock / thermal state
            for name, fn in runs.items():
                if name != "eigh" or rnd < base_rounds:
                    times[name].append(timed(fn))
        med = {name: statistics.median(t) for name, t in times.items()}
        ek = {f"{name}_ms_median": med[name] for name in runs}
        ek.update({f"{name}_ms_min": min(times[name]) for name in runs})
        ek["output_bytes"] = w.numel() * 4 + v.numel() * 8
        ek["herm_eig_over_csm"] = med["herm_eig"] / med["csm"]
        if "eigh" in runs:  # the same matrices on both sides
            ek["eigh_over_herm_eig_on_eigh_slice"] = med["eigh"] / med["herm_eig_on_eigh_slice"]
        entry["k"][str(k)] = ek
        print(f"{label:24s} k {k}  " + "  ".join(f"{n} {med[n]:9.3f} ms" for n in runs), flush=True)
        del v
    ops.herm_eig_out(S, 0, w, None, sw)
    entry["sweeps_mean"] = float(sw.float().mean())
    entry["sweeps_max"] = int(sw.max())
    if base is not None:
        wb = torch.linalg.eigh(base)[0].flip(-1)
        wf = w.reshape(-1, C)[:base.shape[0]]
        dis = (wf - wb).abs().amax(-1) / wb[:, 0]
        entry["eigenvalue_agreement_over_lambda1"] = float(dis.max())
        if not float(dis.max()) <= 1e-5:  # which route is off: numpy in complex128 decides
            import numpy as np
            worst = int(torch.nan_to_num(dis, nan=float("inf")).argmax())
            wn = np.linalg.eigvalsh(base[worst].cpu().numpy().astype(np.complex128))[::-1]
            entry["worst_matrix"] = {
                "index": worst, "lambda1": float(wn[0]),
                "matrices_above_1e-5": int((~(dis <= 1e-5)).sum()),
                "herm_eig_error_over_lambda1":
                    float(np.abs(wf[worst].cpu().numpy() - wn).max() / wn[0]),
                "eigh_error_over_lambda1":
                    float(np.abs(wb[worst].cpu().numpy() - wn).max() / wn[0])}
            print(f"{label:24s} worst matrix {entry['worst_matrix']}", flush=True)
        del wb
    print(f"{label:24s} sweeps mean {entry['sweeps_mean']:.2f} max {entry['sweeps_max']}  "
          f"agreement {entry.get('eigenvalue_agreement_over_lambda1')}  eigh on "
          f"{entry['eigh_matrices']} of {count} matrices, errors {errors}", flush=True)
    res["shapes"][label] = entry
    del x, S, w, sw, base
    torch.cuda.empty_cache()
write_json(res, path)
