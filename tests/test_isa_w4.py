"""Build-quality guard (CPU: hipcc cross-compiles gfx950 without a GPU) for the kernels on int4 group-quantised weights, skinny_gemm_w4_k (gemm.hip)
and decode_chain_w4_k (chain.hip): what tests/test_isa_wcode.py holds the coded kernels to, with its helpers and fixtures' recipe, on the assembly of
gemm.hip / chain.hip compiled with build.py's own flags:

  * the 8 dwords of leading arguments (int4 stream, X, K, N, header words) are covered by the kernarg preload;
  * no private (scratch) segment -- the 4-wave form is built at 64 VGPRs, eight workgroups per CU; the chained kernel at <= 128;
  * on every path from the entry the first 16-byte global load (the non-temporal nibble ring) stands in front of any scalar load;
  * the K loops -- the int4 one and the raw one of a flagged tile (the LoRA-A rows of the fused QKV weight) -- wait with counted vmcnt only;
  * the int4 loop rounds to bf16 with the packed conversion (v_cvt_pk_bf16_f32), four per fragment: no integer rounding sequence.
"""
import os
import re

import pytest

from test_isa_entry import HIPCC, _bodies, _descriptors, first_loads
from test_isa_wcode import _k_loops, chain_asm, gemm_asm      # noqa: F401  (fixtures)

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")

PAT = r"_ZN3rdx16skinny_gemm_w4_kILi[034]ELb[01]ELi(?:4|8|16)EEEv"
N_INST = 18          # 3 epilogues (none, +residual, SwiGLU) x fused RMSNorm or not x 4 / 8 / 16 waves
LEAD = 8
CHAIN = "_ZN3rdx17decode_chain_w4_kEPKvS1_iiiiNS_9ChainArgsE"


def _names(bodies):
    names = sorted(n for n in bodies if re.match(PAT, n))
    assert len(names) == N_INST, f"{len(names)} instantiations of skinny_gemm_w4_k found, {N_INST} expected: the scan no longer matches the assembly"
    return names


def test_w4_kernels_preload_their_leading_arguments_and_hold_no_scratch(gemm_asm):      # noqa: F811
    bodies, desc = _bodies(gemm_asm), _descriptors(gemm_asm)
    bad = []
    for n in _names(bodies):
        d = desc[n]
        if d["user_sgpr_kernarg_preload_length"] < LEAD:
            bad.append((n, "preload length", d["user_sgpr_kernarg_preload_length"]))
        if d["private_segment_fixed_size"] != 0:
            bad.append((n, "scratch bytes", d["private_segment_fixed_size"]))
        if re.search(r"Li4EEEv", n) and d["next_free_vgpr"] > 64:
            bad.append((n, "VGPRs of the 4-wave form", d["next_free_vgpr"]))
        if "scratch_" in "\n".join(bodies[n]):
            bad.append((n, "scratch instructions", None))
    assert not bad, bad


def test_w4_ring_stands_in_front_of_every_scalar_load(gemm_asm):      # noqa: F811
    bodies = _bodies(gemm_asm)
    bad = []
    for n in _names(bodies):
        sites, offenders = first_loads(bodies[n])
        if offenders:
            bad.append((n, "in front of a path's first load", offenders[:3]))
        if len(sites) < 1 or sum(sites.values()) < len(sites):
            bad.append((n, "first-load sites (non-temporal)", (len(sites), sum(sites.values()))))
    assert not bad, bad


def _check_loops(name, loops, want, bad):
    if len(loops) < want:
        bad.append((name, "K loops found", len(loops)))
    for loop in loops:
        if not any(re.match(r"^s_waitcnt\b.*vmcnt\(\d+\)", x) for x in loop):
            bad.append((name, "a K loop without a vmcnt wait: the scan no longer matches", None))
        drains = [x for x in loop if re.match(r"^s_waitcnt\b.*vmcnt\(0\)", x)]
        if drains:
            bad.append((name, "vmcnt(0) inside a K loop", len(drains)))
    # the int4 loops: those that convert. Four packed conversions per fragment, one fragment per MFMA
    dec = [l for l in loops if any(x.startswith("v_cvt_pk_bf16_f32") for x in l)]
    if not dec:
        bad.append((name, "no K loop with v_cvt_pk_bf16_f32", None))
    for l in dec:
        cv, mf = sum(x.startswith("v_cvt_pk_bf16_f32") for x in l), sum(x.startswith("v_mfma") for x in l)
        if cv != 4 * mf:
            bad.append((name, "packed conversions / MFMAs in the int4 loop", (cv, mf)))


def test_w4_k_loops_wait_with_counted_vmcnt(gemm_asm):      # noqa: F811
    bodies = _bodies(gemm_asm)
    bad = []
    for n in _names(bodies):
        _check_loops(n, list(_k_loops(bodies[n])), 2, bad)          # int4 and raw
    assert not bad, bad


def test_w4_chain_kernel_head_scratch_and_waits(chain_asm):      # noqa: F811
    bodies, desc = _bodies(chain_asm), _descriptors(chain_asm)
    assert CHAIN in bodies, sorted(n for n in bodies if "chain" in n)
    d = desc[CHAIN]
    assert d["user_sgpr_kernarg_preload_length"] >= 8
    assert d["private_segment_fixed_size"] == 0 and "scratch_" not in "\n".join(bodies[CHAIN])
    assert d["next_free_vgpr"] <= 128
    sites, offenders = first_loads(bodies[CHAIN])
    assert not offenders, offenders[:3]
    assert len(sites) >= 2 and sum(sites.values()) == len(sites), sites          # both roles' int4 rings, non-temporal
    bad = []
    _check_loops(CHAIN, list(_k_loops(bodies[CHAIN])), 4, bad)                    # int4 and raw loop of either role
    assert not bad, bad
