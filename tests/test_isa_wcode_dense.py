"""Build-quality guard (CPU: hipcc cross-compiles gfx950 without a GPU) for the dense twin of the coded K loops (csrc/skinny_body.h, csrc/chain.hip:
a tile whose dense word is set is decoded without the zero test, csrc/rdx_common.h wc_hi4 DENSE), with the helpers of tests/test_isa_entry.py and
tests/test_isa_wcode.py on the assembly of gemm.hip and chain.hip compiled with build.py's own flags:

  * every skinny_gemm_wc_k instantiation holds at least three single-block K loops (dense, general, raw), decode_chain_wc_k at least six (both roles);
    each waits with counted vmcnt, none with vmcnt(0);
  * among the coded loops of one ring depth (same number of MFMAs per trip) the one with the fewest VALU instructions per MFMA has strictly fewer than
    the general loop, the one with the most; the counts are printed (profiles/r14_dense_decode.md has them), not fixed here;
  * no scratch; the 4-wave GEMV stays at most 64 VGPRs, the chained kernel at most 128;
  * what the change must not touch: the int4 kernels and the raw bf16 GEMV keep their VGPRs and the instruction count of each of their K loops
    (numbers taken from the commit before the dense decode, same compiler flags; tests/test_isa_chain_predecode.py pins the chained int4 kernel and
    the raw chained kernels the same way).
"""
import os
import re

import pytest

from test_isa_entry import HIPCC, _bodies, _descriptors
from test_isa_wcode import CHAIN, PAT, N_INST, _k_loops, chain_asm, gemm_asm      # noqa: F401  (fixtures)

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")

W4_PAT = r"_ZN3rdx16skinny_gemm_w4_kILi[034]ELb[01]ELi(?:4|8|16)EEEv"
RAW_PAT = r"_ZN3rdx13skinny_gemm_kIDF16bLi1ELi[0-5]ELb([01])ELi(4|8|16)ELb1ELb0EEEv"
# on the commit before the dense decode: VGPRs of every skinny_gemm_w4_k instantiation and the instructions (labels included) of its two K loops -- the
# raw loop of a flagged tile and the int4 loop
PARENT_W4_VGPRS = 58
PARENT_W4_LOOPS = {4: [45, 1070], 8: [45, 1069], 16: [45, 1069]}       # by waves per workgroup
# the raw bf16 GEMV on LDS-staged activations (skinny_gemm_k<bf16, 1, EPI, NORM, WAVES, true, false>, the kernel the coded one falls back on and shares
# skinny_tile with), on that commit: (fused RMSNorm, waves) -> (VGPRs, instructions of its one K loop); no scratch
PARENT_RAW = {(0, 4): (50, 85), (1, 4): (62, 85), (0, 8): (82, 165), (1, 8): (94, 165), (0, 16): (82, 165), (1, 16): (94, 165)}


def _valu(loop):
    return sum(1 for x in loop if x.startswith("v_") and not x.startswith("v_mfma"))


def _mfma(loop):
    return sum(1 for x in loop if x.startswith("v_mfma"))


def _check_loops(name, loops, want):
    assert len(loops) >= want, (name, len(loops), want)
    for loop in loops:
        assert any(re.match(r"^s_waitcnt\b.*vmcnt\(\d+\)", x) for x in loop), (name, "a K loop without a vmcnt wait: the scan no longer matches")
        assert not [x for x in loop if re.match(r"^s_waitcnt\b.*vmcnt\(0\)", x)], (name, "vmcnt(0) inside a K loop")


def _dense_is_cheaper(name, loops, show):
    """Coded loops (those that assemble fragments with v_perm_b32), grouped by MFMAs per trip = ring depth = role."""
    coded = [l for l in loops if any(x.startswith("v_perm_b32") for x in l)]
    groups = {}
    for l in coded:
        groups.setdefault(_mfma(l), []).append(_valu(l))
    assert groups, (name, "no coded K loop found")
    for m, valu in sorted(groups.items()):
        assert len(valu) >= 2, (name, m, valu)                       # a dense and a general loop per ring depth
        if show:
            print(f"{name}: {m} MFMAs per trip, VALU per trip dense {min(valu)} / general {max(valu)} = {min(valu) / m:.2f} / {max(valu) / m:.2f} per MFMA")
        assert min(valu) < max(valu), (name, m, valu)


def test_every_coded_gemv_has_a_dense_a_general_and_a_raw_k_loop(gemm_asm):      # noqa: F811
    bodies, desc = _bodies(gemm_asm), _descriptors(gemm_asm)
    names = sorted(n for n in bodies if re.match(PAT, n))
    assert len(names) == N_INST
    for i, n in enumerate(names):
        d = desc[n]
        assert d["private_segment_fixed_size"] == 0 and "scratch_" not in "\n".join(bodies[n]), n
        if re.search(r"Li4EEEv", n):
            assert d["next_free_vgpr"] <= 64, (n, d["next_free_vgpr"])
        loops = list(_k_loops(bodies[n]))
        _check_loops(n, loops, 3)
        _dense_is_cheaper(n, loops, show=i == 0)


def test_the_coded_chained_kernel_has_three_k_loops_per_role(chain_asm):      # noqa: F811
    bodies, desc = _bodies(chain_asm), _descriptors(chain_asm)
    d = desc[CHAIN]
    assert d["private_segment_fixed_size"] == 0 and "scratch_" not in "\n".join(bodies[CHAIN])
    assert d["next_free_vgpr"] <= 128, d["next_free_vgpr"]
    print(f"decode_chain_wc_k: {d['next_free_vgpr']} VGPRs")
    loops = list(_k_loops(bodies[CHAIN]))
    _check_loops(CHAIN, loops, 6)
    _dense_is_cheaper("decode_chain_wc_k", loops, show=True)


def test_int4_and_raw_gemv_k_loops_are_those_of_the_parent_commit(gemm_asm):      # noqa: F811
    bodies, desc = _bodies(gemm_asm), _descriptors(gemm_asm)
    w4 = sorted(n for n in bodies if re.match(W4_PAT, n))
    assert len(w4) == 18, len(w4)                                   # 3 epilogues x fused RMSNorm or not x 4 / 8 / 16 waves
    for n in w4:
        assert desc[n]["next_free_vgpr"] == PARENT_W4_VGPRS, (n, desc[n]["next_free_vgpr"])
        waves = int(re.search(r"Li(4|8|16)EEEv", n).group(1))
        assert sorted(len(l) for l in _k_loops(bodies[n])) == PARENT_W4_LOOPS[waves], n
    raw = sorted(n for n in bodies if re.match(RAW_PAT, n))
    assert len(raw) == 36, len(raw)                                 # 6 epilogues x fused RMSNorm or not x 4 / 8 / 16 waves
    for n in raw:                                                    # the raw GEMV: one K loop, no decode in it, the parent's registers and length
        m = re.match(RAW_PAT, n)
        vgprs, length = PARENT_RAW[(int(m.group(1)), int(m.group(2)))]
        loops = list(_k_loops(bodies[n]))
        assert len(loops) == 1 and not any(x.startswith("v_perm_b32") for x in loops[0]), n
        assert (desc[n]["next_free_vgpr"], len(loops[0])) == (vgprs, length), (n, desc[n]["next_free_vgpr"], len(loops[0]))
        assert desc[n]["private_segment_fixed_size"] == 0, n
        _check_loops(n, loops, 1)
