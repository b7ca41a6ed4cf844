"""LDS access patterns of top1_kernel_reg (svd_denoise.hip) through the bank model of
tools/lds_banks.py: one line per wave-instruction pattern, extra cycles from bank conflicts
against the conflict-free cycle count (DESIGN 6.1 carries the table).

    python tools/top1_reg_banks.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from lds_banks import conflicts  # noqa: E402

N, ZP = 128, 136


def zt(p, k):
    return p * ZP + k + 4 * (k >> 6)


def uoff(k):
    return 4 * (k + (k >> 4))


def ppos(i):
    return i ^ ((i >> 3) & 7)


# byte offsets of the regions inside the kernel's LDS block
ZT, U, P = 0, 4 * ZP * 4, 4 * ZP * 4 + uoff(N) * 4


def lane_map(tid):
    lane = tid & 63
    return dict(lane=lane, w=tid >> 6, a=tid >> 4, c=tid & 15,
                i0=64 * (lane >> 5) + 4 * (tid & 15) + 2 * ((lane >> 4) & 1))


def patterns():
    """(name, instruction, wave -> (64 byte addresses, 64 active flags or None))."""
    def per_wave(f, active=None):
        def g(w):
            lm = [lane_map(64 * w + l) for l in range(64)]
            return [f(m, 64 * w + l) for l, m in enumerate(lm)], \
                (None if active is None else [active(m, 64 * w + l) for l, m in enumerate(lm)])
        return g

    out = []
    for h in (0, 1):
        out.append((f"X Z: basis chunk h={h} (p=0)", "ds_read_b128",
                    per_wave(lambda m, t, h=h: ZT + 4 * zt(0, 4 * m["c"] + 64 * h))))
    out.append(("X Z: U rows written (float2)", "ds_write_b64",
                per_wave(lambda m, t: U + 4 * (uoff(m["a"] + 16 * (m["c"] >> 1)) + 2 * (m["c"] & 1)))))
    out.append(("X^T U: U row a + 16 m (m=0)", "ds_read_b128",
                per_wave(lambda m, t: U + 4 * uoff(m["a"]))))
    for e in (0, 1):
        out.append((f"X^T U: wave partial sums, column i0+{e}", "ds_write_b128",
                    per_wave(lambda m, t, e=e: P + 4 * (m["w"] * 4 * N + 4 * ppos(m["i0"] + e)))))
    out.append(("Y: the four waves' sums read (wave 0's)", "ds_read_b128",
                per_wave(lambda m, t: P + 16 * ppos(t & 127))))
    out.append(("Y: row written / read back", "ds_read_b128", per_wave(lambda m, t: P + 16 * (t & 127))))
    out.append(("Z: row read back (p=0)", "ds_read_b32", per_wave(lambda m, t: ZT + 4 * zt(0, t & 127))))
    for i in (0, 1):
        out.append((f"Gram sums: padded U, step i={i}", "ds_read_b32",
                    per_wave(lambda m, t, i=i: U + 4 * (uoff(8 * i + (t & 7)) + ((t >> 3) & 3)))))
    out.append(("fp64: v chunk (double2)", "ds_read_b128",
                per_wave(lambda m, t: P + 8 * (4 * m["c"]))))
    out.append(("fp64: u row written", "ds_write_b64",
                per_wave(lambda m, t: P + 8 * (N + m["a"] + 16 * (m["c"] >> 1)),
                         lambda m, t: not (m["c"] & 1))))
    out.append(("fp64: u row a + 16 m (m=0)", "ds_read_b64",
                per_wave(lambda m, t: P + 8 * (N + m["a"]))))
    out.append(("fp64: X^T u wave partial sums (double2)", "ds_write_b128",
                per_wave(lambda m, t: P + 8 * (2 * N + m["w"] * N + m["i0"]))))
    out.append(("fp64: X^T u sums read", "ds_read_b64", per_wave(lambda m, t: P + 8 * (2 * N + (t & 127)))))
    return out


def table():
    rows = []
    for name, instr, f in patterns():
        extra = cycles = 0
        for w in range(4):
            addrs, active = f(w)
            e, c = conflicts(instr, addrs, active)
            extra, cycles = max(extra, e), max(cycles, c)
        rows.append((name, instr, extra, cycles))
    return rows


if __name__ == "__main__":
    for name, instr, extra, cycles in table():
        print(f"{name:48s} {instr:14s} extra {extra:2d} of {cycles:2d} cycles")
