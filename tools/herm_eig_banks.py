"""LDS bank model (tools/lds_banks.py) of the two passes of csrc/herm_eig.hip for candidate
row strides: mean LDS cycles per wave-instruction over every round of a sweep (8-byte
elements: ds_read_b64 / ds_write_b64).

    python tools/herm_eig_banks.py [P ...]

The mapping is the kernel's: P / 2 pairs a round, L = min(64 / (P / 2), P) lanes per pair,
lane (pair, sub) touching elements sub, sub + L, ... of rows (a, b) (row pass) and of columns
(a, b) (column pass). The conflict-free count is 2 (ds_read_b64) and 4 (ds_write_b64)
cycles."""
import sys

from lds_banks import conflicts


def rounds(P):
    """The (a, b) of every pair j in every round of the tournament."""
    for rnd in range(P - 1):
        pos = lambda k: 0 if k == 0 else 1 + (k - 1 + rnd) % (P - 1)  # noqa: E731
        yield [tuple(sorted((pos(j), pos(P - 1 - j)))) for j in range(P // 2)]


def model(P, S, elem=8):
    NP = P // 2
    L = min(64 // NP, P)
    rd, wr = "ds_read_b64", "ds_write_b64"
    tot = {"row read": 0, "row write": 0, "col read": 0, "col write": 0}
    cnt = 0
    for pairs in rounds(P):
        for u in range((P + L - 1) // L):
            active = [l // L < NP and l % L + L * u < P for l in range(64)]
            for which in (0, 1):  # row / column a, then b
                row = [0] * 64
                col = [0] * 64
                for l in range(64):
                    if active[l]:
                        k, ab = l % L + L * u, pairs[l // L][which]
                        row[l] = (ab * S + k) * elem
                        col[l] = (k * S + ab) * elem
                tot["row read"] += conflicts(rd, row, active)[1]
                tot["row write"] += conflicts(wr, row, active)[1]
                tot["col read"] += conflicts(rd, col, active)[1]
                tot["col write"] += conflicts(wr, col, active)[1]
                cnt += 1
    return {k: v / cnt for k, v in tot.items()}


def best_pad(P):
    """The pad in 1 .. 4 with the fewest modelled cycles a round: the row pass touches A, the
    column pass A and V."""
    def cost(S):
        m = model(P, S)
        return m["row read"] + m["row write"] + 2 * (m["col read"] + m["col write"])
    return min(range(1, 5), key=lambda pad: (cost(P + pad), pad))


if __name__ == "__main__":
    if sys.argv[1:] == ["--table"]:  # the PAD table of csrc/herm_eig.hip
        print(", ".join(str(best_pad(P)) for P in range(2, 65, 2)))
        sys.exit(0)
    sizes = [int(a) for a in sys.argv[1:]] or [16, 32, 40, 64]
    print("mean LDS cycles per wave-instruction")
    for P in sizes:
        for S in range(P, P + 5):
            m = model(P, S)
            print(f"  P {P:2d} S {S:2d}  " + "  ".join(f"{k} {v:5.2f}" for k, v in m.items()))
