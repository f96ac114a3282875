"""CPU-only checks of the per-walker scalar layout of the resident sweep k_sweep_r8 (csrc/pqa_res8_tab.hpp: PQA_R8_WS): the AO phase
reads the proposals of the block's eight walkers, wsc[pt * PQA_R8_WS + d] for point pt = lane % 8, in one LDS instruction per coordinate.
The LDS serves a 64-bit read in two groups of 32 lanes, bank = (byte address / 4) mod 64, and a 128-bit read in four groups of 16 lanes
(MI355X); lanes that read the same address broadcast.  The stride must put the eight addresses on disjoint banks, keep every walker's
slice 16-byte aligned and hold the slots the kernel uses (0..29)."""
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
TAB = os.path.join(HERE, "..", "pyqmc_amd", "csrc", "pqa_res8_tab.hpp")
NW = 8  # walkers per block (PQA_R8_NW)
READ_B128_GROUPS = [
    list(range(0, 4)) + list(range(12, 16)) + list(range(20, 28)),
    list(range(4, 12)) + list(range(16, 20)) + list(range(28, 32)),
]
READ_B128_GROUPS += [[l + 32 for l in g] for g in READ_B128_GROUPS]


def header_define(name):
    m = re.search(r"#define\s+" + name + r"\s+(\d+)", open(TAB).read())
    assert m, name
    return int(m.group(1))


def extra_cycles(stride, dwords, groups):
    """Conflict cycles of one wave-wide read of wsc[pt * stride + 0 .. dwords / 2) (lane = pt + 8 slot) under the banking model above."""
    extra = 0
    for g in groups:
        per_bank = {}
        for lane in g:
            base = 2 * (lane % 8) * stride  # dword address of the lane's double
            for k in range(dwords):
                per_bank.setdefault((base + k) % 64, set()).add(base)
        extra += max(len(a) for a in per_bank.values()) - 1
    return extra


def test_proposal_reads_of_the_eight_walkers_are_conflict_free():
    ws = header_define("PQA_R8_WS")
    assert extra_cycles(ws, 2, [list(range(32)), list(range(32, 64))]) == 0
    assert extra_cycles(ws, 4, READ_B128_GROUPS) == 0
    # the model itself: the former stride of 32 doubles puts all eight walkers on one bank pair (8-way, 7 extra cycles per group)
    assert extra_cycles(32, 2, [list(range(32)), list(range(32, 64))]) == 14


def test_scalar_slices_are_disjoint_aligned_and_hold_every_slot():
    ws = header_define("PQA_R8_WS")
    assert ws >= 30 and ws % 2 == 0  # slots 0..29 (r8_jas_dual's hand-over at 28, 29); 16-byte aligned slices
    cells = [w * ws + k for w in range(NW) for k in range(30)]
    assert len(set(cells)) == len(cells)
