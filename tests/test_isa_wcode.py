"""Build-quality guard (CPU: hipcc cross-compiles gfx950 without a GPU) for the kernels on coded bf16 weights, skinny_gemm_wc_k (gemm.hip) and
decode_chain_wc_k (chain.hip: down_proj and QKV roles, 8 leading dwords, <= 128 VGPRs, two first-load sites, a coded and a raw K loop per role): what
tests/test_isa_entry.py and tests/test_isa_waits.py hold the raw kernels to, with their helpers, on the assembly of gemm.hip compiled with build.py's
own flags:

  * the 8 dwords of leading arguments (coded planes, X, K, N, header words) are covered by the kernarg preload;
  * no private (scratch) segment -- the 4-wave form is built at 64 VGPRs, eight workgroups per CU;
  * on every path from the entry the first 16-byte global load (the non-temporal coded ring) stands in front of any scalar load and of any wait on the
    scalar counter: the tile's header word and the argument struct are read behind it;
  * the K loops -- every loop that holds MFMAs and non-temporal loads: the coded one and the raw one of a flagged tile -- wait with counted vmcnt only.
"""
import os
import re
import subprocess

import pytest

from radialog_amd import build
from test_isa_entry import CSRC, HIPCC, _bodies, _descriptors, first_loads

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")

PAT = r"_ZN3rdx16skinny_gemm_wc_kILi[0345]ELb[01]ELi(?:4|8|16)EEEv"
N_INST = 24          # 4 epilogues x fused RMSNorm or not x 4 / 8 / 16 waves
LEAD = 8


@pytest.fixture(scope="module")
def gemm_asm(tmp_path_factory):
    d = tmp_path_factory.mktemp("isa_wcode")
    o = d / "gemm.s"
    flags = [f for f in build.unit_flags("gemm.hip") if not f.startswith("-W")]
    p = subprocess.run([HIPCC] + flags + ["-S", "--cuda-device-only", "-I" + CSRC, os.path.join(CSRC, "gemm.hip"), "-o", str(o)],
                       capture_output=True, text=True, cwd=str(d))
    assert p.returncode == 0 and o.exists(), p.stderr[-2000:]
    return o.read_text()


@pytest.fixture(scope="module")
def chain_asm(tmp_path_factory):
    d = tmp_path_factory.mktemp("isa_wcode_chain")
    o = d / "chain.s"
    flags = [f for f in build.unit_flags("chain.hip") if not f.startswith("-W")]
    p = subprocess.run([HIPCC] + flags + ["-S", "--cuda-device-only", "-I" + CSRC, os.path.join(CSRC, "chain.hip"), "-o", str(o)],
                       capture_output=True, text=True, cwd=str(d))
    assert p.returncode == 0 and o.exists(), p.stderr[-2000:]
    return o.read_text()


def _names(bodies):
    names = sorted(n for n in bodies if re.match(PAT, n))
    assert len(names) == N_INST, f"{len(names)} instantiations of skinny_gemm_wc_k found, {N_INST} expected: the scan no longer matches the assembly"
    return names


def test_coded_kernels_preload_their_leading_arguments_and_hold_no_scratch(gemm_asm):
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


def test_coded_ring_stands_in_front_of_every_scalar_load(gemm_asm):
    bodies = _bodies(gemm_asm)
    bad = []
    for n in _names(bodies):
        sites, offenders = first_loads(bodies[n])
        if offenders:
            bad.append((n, "in front of a path's first load", offenders[:3]))
        if len(sites) < 1 or sum(sites.values()) < len(sites):
            bad.append((n, "first-load sites (non-temporal)", (len(sites), sum(sites.values()))))
    assert not bad, bad


def _k_loops(body):
    ins = [l.split(";")[0].strip() for l in body]
    labels = {l[:-1]: i for i, l in enumerate(ins) if re.match(r"^\.LBB\d+_\d+:$", l)}
    for i, l in enumerate(ins):
        m = re.match(r"^s_c?branch\w*\s+(\.LBB\d+_\d+)", l)
        if m and m.group(1) in labels and labels[m.group(1)] < i:
            loop = ins[labels[m.group(1)]:i]
            # a K loop is ONE basic block (no branch inside it: a split block is what made these loops wait vmcnt(0) on every trip); backward jumps
            # of the tail code span several blocks and are no loops
            if sum(1 for x in loop if re.match(r"^\.LBB\d+_\d+:$", x)) != 1 or any(re.match(r"^s_c?branch", x) for x in loop):
                continue
            if any(x.startswith("v_mfma") for x in loop) and any(x.startswith("global_load_dwordx4") and re.search(r"\bnt\b", x) for x in loop):
                yield loop


def test_k_loops_wait_with_counted_vmcnt(gemm_asm):
    bodies = _bodies(gemm_asm)
    bad = []
    for n in _names(bodies):
        loops = list(_k_loops(bodies[n]))
        if len(loops) < 2:
            bad.append((n, "K loops found (coded and raw expected)", len(loops)))
        for loop in loops:
            if not any(re.match(r"^s_waitcnt\b.*vmcnt\(\d+\)", x) for x in loop):
                bad.append((n, "a K loop without a vmcnt wait: the scan no longer matches", None))
            drains = [x for x in loop if re.match(r"^s_waitcnt\b.*vmcnt\(0\)", x)]
            if drains:
                bad.append((n, "vmcnt(0) inside a K loop", len(drains)))
    assert not bad, bad


CHAIN = "_ZN3rdx17decode_chain_wc_kEPKvS1_iiiiNS_9ChainArgsE"


def test_coded_chain_kernel_head_scratch_and_waits(chain_asm):
    bodies, desc = _bodies(chain_asm), _descriptors(chain_asm)
    assert CHAIN in bodies, sorted(n for n in bodies if "chain" in n)
    d = desc[CHAIN]
    assert d["user_sgpr_kernarg_preload_length"] >= 8
    assert d["private_segment_fixed_size"] == 0 and "scratch_" not in "\n".join(bodies[CHAIN])
    assert d["next_free_vgpr"] <= 128
    sites, offenders = first_loads(bodies[CHAIN])
    assert not offenders, offenders[:3]
    assert len(sites) >= 2 and sum(sites.values()) == len(sites), sites          # both roles' coded rings, non-temporal
    loops = list(_k_loops(bodies[CHAIN]))
    assert len(loops) >= 4, len(loops)                                            # coded and raw loop of either role
    for loop in loops:
        assert any(re.match(r"^s_waitcnt\b.*vmcnt\(\d+\)", x) for x in loop)
        assert not [x for x in loop if re.match(r"^s_waitcnt\b.*vmcnt\(0\)", x)], "vmcnt(0) inside a K loop"
