"""CPU model of conv_rows_pool_kernel's step timeline (csrc/conv_rows.hip, schedules 0 and 1).

A persistent workgroup streams the rows of its images through an 8-row LDS ring, two rows per
step. The kernel's timeline is restated here and checked for every step:

  prologue   fills of steps 0 .. LEAD - 1, vmcnt(0), barrier (schedule 1: the fragments of
             step 0 are read after it)
  step s     the DMA waves fill the slots of step s + LEAD (an LDS-DMA for rows inside the
             image, a zero write otherwise); every wave stores pooled pair s - 2; the
             fragments of step s + PF are read (PF = 0: schedule 0, PF = 1: schedule 1); the
             DMA waves wait for the DMA issued in step s - 1; barrier

Checked: a slot that a working step consumes holds that step's rows and was covered by a wait
and a barrier before it is read; no slot is refilled before the barrier that follows its last
read; and the vmcnt count of schedule 1's ledger (ops issued after the awaited DMA) is what an
in-order queue of the wave's vector-memory ops needs, never more than the three the kernel's
steady state allows for. The constants are read back from the kernel source as well."""
import os
import re

import pytest

RING, ROWS, LEAD, PF = 8, 2, 3, 1
SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                   "spectrogram-enhancement_amd", "csrc", "conv_rows.hip")


def test_constants_are_the_kernels():
    txt = open(SRC).read()
    rc = txt[txt.index("struct RC {"):txt.index("struct CRArgs")]
    for name, val in (("RING", RING), ("LEAD", LEAD), ("PF", PF)):
        m = re.search(r"static constexpr int %s = (\d+);" % name, rc)
        assert m and int(m.group(1)) == val, name
    assert "tests/test_conv_rows_sched_model.py" in rc


def slots(t):
    """ring slots of step t's two rows"""
    return [(ROWS * t + j) % RING for j in range(ROWS)]


def timeline(spi, nimg, pf, lead=LEAD, dma_wave=True):
    """Run the restated timeline; returns (steps, waits) where waits lists the vmcnt count of
    every wait the ledger issued. Raises AssertionError on a hazard."""
    S = nimg * spi + 1
    ph = spi - 1  # pooled rows per image = input row pairs per image

    def working(t):  # step t has input rows (not the bubble between images, not past the end)
        return 0 <= t and t // spi < nimg and t % spi < ph

    def in_image(t):  # step t's rows are DMA'd (else zero-written)
        return t < S and working(t)

    def pair_valid(t):  # pooled pair of step t is an output row
        return t >= 0 and t // spi < nimg and t % spi < ph

    content = [None] * RING    # step whose rows the slot holds (as filled last)
    visible = [False] * RING   # the fill was waited for and a barrier has passed since
    landed = [False] * RING    # the fill has completed (wait or zero write + barrier)
    last_read = [-10] * RING   # last step in which the slot was read (used or not)
    queue = []                 # in-order vector-memory ops of this wave: ("dma", t) / ("st", t)
    done = 0                   # ops [0, done) have completed
    vmn, mk0, mk1 = 0, -1, -1  # the kernel's ledger
    waits = []

    def fill(t, s_now):
        nonlocal vmn
        for sl in slots(t):
            assert last_read[sl] < s_now, f"slot {sl} refilled in step {s_now}, read in {last_read[sl]}"
            content[sl], visible[sl], landed[sl] = t, False, False
        if dma_wave and in_image(t):
            queue.append(("dma", t))
            vmn += 1
            return vmn
        for sl in slots(t):  # zero write: an LDS write, complete at this wave's next barrier
            landed[sl] = True
        return -1

    def read(t, s_now):
        for sl in slots(t):
            last_read[sl] = s_now
            if working(t):  # the fragments are consumed: they must be step t's, and visible
                assert content[sl] == t, f"step {s_now} reads slot {sl}: holds {content[sl]}, wants {t}"
                assert visible[sl], f"step {s_now} reads slot {sl} before its wait and barrier"

    def barrier():
        for sl in range(RING):
            if landed[sl]:
                visible[sl] = True

    def complete_upto(n_left):
        nonlocal done
        done = max(done, len(queue) - n_left)
        for kind, t in queue[:done]:
            if kind == "dma":
                for sl in slots(t):
                    if content[sl] == t:
                        landed[sl] = True

    for t in range(lead):
        fill(t, -1)
    complete_upto(0)
    barrier()
    vmn = 0
    queue.clear()
    done = 0
    if pf:
        read(0, -1)
    for s in range(S):
        mk1 = fill(s + lead, s)
        if pair_valid(s - 2):
            queue.append(("st", s - 2))
            vmn += 1
        read(s + pf, s)
        if pf == 0 and not dma_wave:
            pass  # (schedule 0 waits on every wave; modelled for the DMA waves below)
        if pf:
            # schedule 1: the ledger's count, checked against the queue
            if mk0 >= 0:
                n = vmn - mk0
                idx = max(i for i, op in enumerate(queue) if op == ("dma", s - 1 + lead))
                assert n == len(queue) - idx - 1, (s, n, queue[idx:])
                assert 0 <= n <= 3
                waits.append(n)
                complete_upto(n)
                assert done > idx
                if mk1 >= 0:  # the DMA just issued stays in flight
                    assert n >= 1
        else:
            # schedule 0: vmcnt(1) when this step issued a DMA, vmcnt(0) otherwise
            complete_upto(1 if mk1 >= 0 else 0)
        mk0 = mk1
        barrier()
    return S, waits


@pytest.mark.parametrize("nimg", [1, 2, 3])
@pytest.mark.parametrize("spi", range(2, 10))
@pytest.mark.parametrize("pf", [0, PF])
def test_timeline_has_no_hazard(spi, nimg, pf):
    S, waits = timeline(spi, nimg, pf)
    assert S == nimg * spi + 1
    if pf:
        # one wait per step that follows a step with a DMA: the in-image steps LEAD ahead
        assert len(waits) == sum(1 for s in range(1, S) if (s - 1 + LEAD) // spi < nimg and
                                 (s - 1 + LEAD) % spi < spi - 1 and s - 1 + LEAD < S)
        if spi >= 4 and nimg >= 2:
            assert max(waits) == 3  # the steady state: two stores and the next DMA are younger


@pytest.mark.parametrize("nimg", [1, 3])
@pytest.mark.parametrize("spi", range(2, 10))
def test_store_only_waves_never_wait(spi, nimg):
    """Waves 4-7 move no rows: their ledger never records a DMA, so they never wait."""
    _, waits = timeline(spi, nimg, PF, dma_wave=False)
    assert waits == []


def test_model_sees_a_deeper_prefetch_and_a_longer_lead():
    """The checks have teeth: fragments two steps ahead are read before their wait, and a
    four-step DMA lead refills the slots schedule 0 is reading."""
    with pytest.raises(AssertionError):
        timeline(6, 2, 2)
    with pytest.raises(AssertionError):
        timeline(6, 2, 0, lead=4)
