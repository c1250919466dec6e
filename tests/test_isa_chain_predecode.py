"""Build-quality guard (CPU: hipcc cross-compiles gfx950 without a GPU) for the scheduling of decode_chain_wc_k's coded path (csrc/chain.hip: operand
lookahead in the coded K loops, pre-decode ahead of the down_proj -> QKV seam), with the helpers of tests/test_isa_wcode.py on the assembly of
chain.hip compiled with build.py's own flags:

  * in every coded K loop (a K loop that holds v_perm_b32) the waits that drain the LDS counter, lgkmcnt(0), are at most one per coded chunk of the
    trip: the four activation fragments of a chunk are read ahead of its decodes and waited for with lgkmcnt(3..0). Before, there was one drain per
    fragment, four times as many;
  * decode work stands in front of the workgroup barrier of the hand-off wait: a v_perm_b32 (the last instruction of a fragment's decode) comes before
    the first barrier that follows the poll loop's nap, and before any MFMA;
  * what the change must not touch compiles as it did on the commit before it: the raw chained kernels and the o_proj role's kernel to the same number
    of VGPRs, the int4 chained kernel to the same number of VGPRs and of instructions in each of its K loops (numbers taken from that commit's chain.hip
    with the same compiler flags).
"""
import os
import re

import pytest

from test_isa_entry import HIPCC, _bodies, _descriptors
from test_isa_wcode import _k_loops, chain_asm      # noqa: F401  (fixture)

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")

WC = "_ZN3rdx17decode_chain_wc_kEPKvS1_iiiiNS_9ChainArgsE"
W4 = "_ZN3rdx17decode_chain_w4_kEPKvS1_iiiiNS_9ChainArgsE"
# VGPRs on the parent commit
PARENT_VGPRS = {
    "_ZN3rdx14decode_chain_kIDF16bLb0EEEvPKvS2_iiiiNS_9ChainArgsE": 88,
    "_ZN3rdx14decode_chain_kIDF16bLb1EEEvPKvS2_iiiiNS_9ChainArgsE": 60,
    r"_ZN3rdx14attn_oproj16_kIDF16bLb0EEEv\w+": 108,
    W4: 60,
}
PARENT_W4_LOOPS = [45, 45, 1069, 1069]       # instructions per K loop (labels included): the raw loop of a flagged tile and the int4 loop, per role


def _ins(body):
    return [l.split(";")[0].strip() for l in body]


def test_coded_k_loops_drain_the_lds_counter_once_per_chunk(chain_asm):      # noqa: F811
    bodies = _bodies(chain_asm)
    coded = [l for l in _k_loops(bodies[WC]) if any(x.startswith("v_perm_b32") for x in l)]
    assert len(coded) >= 2, len(coded)                                           # the coded loop of either role
    for loop in coded:
        mfma = sum(x.startswith("v_mfma") for x in loop)
        assert mfma and mfma % 4 == 0, mfma
        drains = sum(bool(re.match(r"^s_waitcnt\b.*lgkmcnt\(0\)", x)) for x in loop)
        print(f"coded K loop: {mfma} MFMAs = {mfma // 4} chunks per trip, {drains} lgkmcnt(0)")
        assert drains <= mfma // 4, (drains, mfma)


def test_decode_stands_in_front_of_the_handoff_barrier(chain_asm):      # noqa: F811
    # A build-quality guard on the kernel TEXT, not on control flow: it reads the linear order of the emitted blocks (nap -> next barrier; no MFMA
    # anywhere earlier in the text, i.e. the role laid out first is the QKV role and its K loops come behind its hand-off). A compiler that lays the
    # blocks out differently can fail it, or pass it, with no change of behaviour: then re-read the assembly and re-pin the scan.
    ins = _ins(_bodies(chain_asm)[WC])
    naps = [i for i, x in enumerate(ins) if x.startswith("s_sleep")]
    assert naps, "no poll loop found: the scan no longer matches the assembly"
    found = False
    for nap in naps:
        bar = next((i for i in range(nap, len(ins)) if ins[i].startswith("s_barrier")), None)
        if bar is None:
            continue
        head = ins[:bar]
        if any(x.startswith("v_perm_b32") for x in head) and not any(x.startswith("v_mfma") for x in head):
            found = True
    assert found, "no decode (v_perm_b32) in front of a hand-off barrier"


def test_untouched_kernels_compile_as_on_the_parent_commit(chain_asm):      # noqa: F811
    bodies, desc = _bodies(chain_asm), _descriptors(chain_asm)
    for pat, vgprs in PARENT_VGPRS.items():
        names = [n for n in desc if re.fullmatch(pat, n)]
        assert len(names) == 1, (pat, names)
        assert desc[names[0]]["next_free_vgpr"] == vgprs, (names[0], desc[names[0]]["next_free_vgpr"], vgprs)
    assert sorted(len(l) for l in _k_loops(bodies[W4])) == PARENT_W4_LOOPS
