"""What the tools/*_bench.py scripts share: the --json / --rounds arguments, the compiler's
resource usage of a source file's kernels, HIP-event timing of interleaved routes and the JSON
result. Importing it puts the repository and the package on sys.path."""
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "spectrogram-enhancement_amd")]


def parse_args(rounds=None):
    """(json path or None, rounds, the other arguments) of `tool [ARGS] [--json PATH]
    [--rounds N]`; rounds None: the tool has no --rounds."""
    args, path = list(sys.argv[1:]), None
    for flag in ("--json", "--rounds") if rounds is not None else ("--json",):
        if flag in args:
            i = args.index(flag)
            if flag == "--json":
                path = args[i + 1]
            else:
                rounds = int(args[i + 1])
            del args[i:i + 2]
    return path, rounds, args


def resources(source_name):
    """VGPRs, SGPRs, scratch, LDS and occupancy of every kernel of csrc/<source_name> (or of a
    path), from the compiler: {kernel: {remark: value}}."""
    import build  # spectrogram-enhancement_amd/build.py: the flags the library is built with
    src = os.path.join(build.CSRC, source_name)
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([build.HIPCC, *build.CFLAGS, "-Rpass-analysis=kernel-resource-usage",
                            "-c", src, "-o", os.path.join(tmp, "kernels.o")],
                           capture_output=True, text=True)
    out, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+(?:Function Name: (\S+)|"
                      r"([A-Za-z][^:\[]*?)(?: \[[^\]]*\])?: (\S+))", line)
        if not m:
            continue
        if m.group(1):
            name = m.group(1)
            out[name] = {}
        elif name:
            out[name][m.group(2).strip()] = m.group(3)
    return out or {"error": r.stderr[-500:]}


def timed(fn):
    """Milliseconds of fn() between two HIP events."""
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def sample(runs, rounds, warm):
    """{name: [ms of each round]} of the routes {name: fn}: `warm` warm-ups each, then `rounds`
    interleaved rounds, so that the routes see the same clock / thermal state."""
    import torch
    for fn in runs.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in runs}
    for _ in range(rounds):
        for name, fn in runs.items():
            times[name].append(timed(fn))
    return times


def measure(runs, rounds, warm):
    """sample() as {<name>_ms_median, <name>_ms_min}."""
    times = sample(runs, rounds, warm)
    out = {f"{name}_ms_median": statistics.median(t) for name, t in times.items()}
    out.update({f"{name}_ms_min": min(t) for name, t in times.items()})
    return out


def write_json(res, path):
    """Prints the result as one JSON line; with a path, writes it there too."""
    print(json.dumps(res))
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as fh:
            json.dump(res, fh, indent=1)
