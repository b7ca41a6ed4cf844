"""The call contract the five averaging entries of the C ABI share (no GPU): the same fault
gives the same code and the same ``specenh_last_error()`` text from every entry that can have
it, and from the entry's ``*_workspace_bytes`` function where that sees the fault too.

Validation happens before the device is touched: the plan is a host-side stand-in (the fields
the validation reads lead the struct), the pointers are never followed. One table holds a valid
call of every entry and what an entry does not share; one table holds the faults."""
import ctypes

import pytest


class PlanHead(ctypes.Structure):  # csrc/stft_plan.hpp: int nperseg, noverlap, hop; ...
    _fields_ = [("nperseg", ctypes.c_int), ("noverlap", ctypes.c_int), ("hop", ctypes.c_int),
                ("rest", ctypes.c_byte * 256)]


def plan_ptr(plan):
    return ctypes.cast(ctypes.pointer(plan), ctypes.c_void_p)


PLAN, ODD = PlanHead(256, 128, 128), PlanHead(200, 100, 100)
# non-null pointers that are never followed
P, Q, R = ctypes.c_void_p(4096), ctypes.c_void_p(8192), ctypes.c_void_p(12288)
L = 16512  # T = 128 frames, four chunks of 32: every entry needs its workspace
COMMON = dict(plan=plan_ptr(PLAN), batch=2, length=L, navg=0, workspace=P,
              workspace_bytes=1 << 40, stream=None)

# order: the C argument list. valid: what COMMON lacks. bytes: the *_workspace_bytes function and
# its argument list. strides: the *_stride arguments compared with length. null_at_batch0: the
# pointers that may be null when there is nothing to do. lacks: faults the entry cannot have.
# texts: where the entry words a fault for itself.
ENTRIES = {
    "specenh_spectral_mean": dict(
        order=("plan", "x", "y", "batch", "length", "x_stride", "y_stride", "navg", "pxx", "pyy",
               "pxy", "coh", "workspace", "stream"),
        valid=dict(x=P, y=Q, x_stride=L, y_stride=L, pxx=P, pyy=None, pxy=None, coh=None),
        bytes=("specenh_spectral_workspace_bytes", ("plan", "batch", "length", "navg")),
        strides=("x_stride", "y_stride"), null_at_batch0=("y", "workspace"),
        # no byte count in its ABI; every nperseg the plan has is served
        lacks=("misaligned workspace", "workspace too small", "nperseg = 200")),
    "specenh_csm": dict(
        order=("plan", "x", "batch", "channels", "length", "channel_stride", "batch_stride",
               "navg", "csm", "coh", "workspace", "workspace_bytes", "stream"),
        valid=dict(x=P, channels=5, channel_stride=L, batch_stride=5 * L, csm=P, coh=None),
        bytes=("specenh_csm_workspace_bytes", ("plan", "batch", "channels", "length", "navg")),
        strides=("channel_stride",), null_at_batch0=("coh", "workspace")),
    "specenh_bispectrum": dict(
        order=("plan", "x", "y", "z", "batch", "length", "x_stride", "y_stride", "z_stride",
               "navg", "nbins", "bispec", "bicoh", "workspace", "workspace_bytes", "stream"),
        valid=dict(x=P, y=Q, z=R, x_stride=L, y_stride=L, z_stride=L, nbins=0, bispec=P,
                   bicoh=None, nsignals=3),
        bytes=("specenh_bispectrum_workspace_bytes",
               ("plan", "batch", "nsignals", "length", "navg")),
        strides=("x_stride", "y_stride", "z_stride"),
        null_at_batch0=("y", "z", "bicoh", "workspace")),
    "specenh_wavenumber_spectrum": dict(
        order=("plan", "x", "y", "batch", "length", "x_stride", "y_stride", "navg", "nk", "skf",
               "workspace", "workspace_bytes", "stream"),
        valid=dict(x=P, y=Q, x_stride=L, y_stride=L, nk=64, skf=P, nsignals=2),
        bytes=("specenh_wavenumber_workspace_bytes",
               ("plan", "batch", "nsignals", "length", "navg")),
        strides=("x_stride", "y_stride"), null_at_batch0=("workspace",)),
    "specenh_correlation": dict(
        order=("plan", "x", "y", "batch", "length", "x_stride", "y_stride", "navg", "maxlag",
               "mode", "out", "energies", "workspace", "workspace_bytes", "stream"),
        valid=dict(x=P, y=Q, x_stride=L, y_stride=L, maxlag=40, mode=1, out=P, energies=None),
        bytes=("specenh_correlation_workspace_bytes",
               ("plan", "batch", "length", "navg", "maxlag")),
        strides=("x_stride", "y_stride"), null_at_batch0=("energies", "workspace"),
        # its padded transform halves the range
        texts={"nperseg = 200": "correlation: nperseg must be a power of two in [64, 2048]"}),
}

EINVAL, EUNSUPPORTED = "SPECENH_EINVAL", "SPECENH_EUNSUPPORTED"
# fault: (what changes in the valid call, code, text, whether *_workspace_bytes sees it too)
FAULTS = {
    "null plan": (dict(plan=None), EINVAL, "null plan", True),
    "batch = -1": (dict(batch=-1), EINVAL, "batch must be >= 0", True),
    "signal shorter than nperseg": (dict(length=255), EINVAL, "signal shorter than nperseg", True),
    "navg > T": (dict(navg=129), EINVAL, "navg exceeds the number of frames", True),
    "null workspace": (dict(workspace=None), EINVAL, "null workspace", False),
    "misaligned workspace": (dict(workspace=ctypes.c_void_p(4104)), EINVAL,
                             "workspace must be 16-byte aligned", False),
    "workspace too small": ("need - 1", EINVAL, "workspace too small", False),
    "nperseg = 200": (dict(plan=plan_ptr(ODD)), EUNSUPPORTED,
                      "nperseg must be a power of two in [64, 4096]", True),
}


def run(name, names, **change):
    """(return value, last error) of function `name` on the entry's valid call with `change`."""
    from specenh import _lib

    values = dict(COMMON, **change)
    rc = getattr(_lib.lib(), name)(*(values[n] for n in names))
    return rc, _lib.last_error()


def entry_call(name, **change):
    e = ENTRIES[name]
    return run(name, e["order"], **dict(e["valid"], **change))


def bytes_call(name, **change):
    e = ENTRIES[name]
    return run(e["bytes"][0], e["bytes"][1], **dict(e["valid"], **change))


def test_the_valid_calls_are_valid_up_to_the_launch():
    """Every fault below is the only fault of its call: the same call with batch = 0 is OK, and
    the workspace the byte count asks for is not empty."""
    from specenh import _lib

    for name, e in ENTRIES.items():
        assert entry_call(name, batch=0)[0] == _lib.SPECENH_OK, name
        assert bytes_call(name)[0] > 0, name
        assert bytes_call(name, batch=0)[0] == 0, name


@pytest.mark.parametrize("fault", list(FAULTS))
def test_a_fault_reads_the_same_from_every_entry(fault):
    from specenh import _lib

    change, code, text, in_bytes = FAULTS[fault]
    seen = {}
    for name, e in ENTRIES.items():
        if fault in e.get("lacks", ()):
            continue
        want = (getattr(_lib, code), e.get("texts", {}).get(fault, text))
        ch = dict(workspace_bytes=bytes_call(name)[0] - 1) if change == "need - 1" else change
        assert entry_call(name, **ch) == want, name
        if in_bytes:
            assert bytes_call(name, **ch) == (0, want[1]), name
        seen[name] = want
    assert len(seen) >= 4 and len(set(seen.values())) <= 2  # one wording, correlation's nperseg


def test_every_stride_is_compared_with_the_length_under_its_own_name():
    from specenh import _lib

    for name, e in ENTRIES.items():
        for stride in e["strides"]:
            assert entry_call(name, **{stride: L - 1}) == (_lib.SPECENH_EINVAL,
                                                           f"{stride} < length"), (name, stride)


def test_nothing_to_do_is_ok_with_every_pointer_null_that_may_be():
    from specenh import _lib

    for name, e in ENTRIES.items():
        nulls = {n: None for n in e["null_at_batch0"]}
        assert entry_call(name, batch=0, **nulls)[0] == _lib.SPECENH_OK, name
        # a fault of the call is still a fault when there is nothing to do
        assert entry_call(name, batch=0, navg=129, **nulls)[0] == _lib.SPECENH_EINVAL, name
