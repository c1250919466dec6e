"""Build-quality guard (CPU: hipcc cross-compiles gfx950 without a GPU) for the 3-16-row kernels on int4 group-quantised weights, xstat16_w4_k and
xrow16_w4_k (xs16.hip), on the assembly of the unit compiled with build.py's own flags -- what tests/test_isa_w4.py holds the batch <= 2 int4 kernels to,
with its helpers:

  * the expected instantiations exist (xstat16_w4_k for EPI_NONE and EPI_SILU_MUL, one xrow16_w4_k);
  * no private (scratch) segment;
  * the K loops wait with counted vmcnt only. xrow16_w4_k has a loop in the sense of test_isa_wcode._k_loops (one basic block, MFMAs and non-temporal
    16-byte loads: its unguarded trips). The production down_proj (K = 11008) never reaches that loop -- it runs the guarded first trip and the tail --
    so the blocks of the guarded first trip are held to counted waits as well. xstat16_w4_k's K loop is unrolled inside a trip of two tiles; what stands for it here is every basic block that
    decodes, multiplies AND refills (non-temporal 16-byte loads) -- the prefetching trips, the peeled first one and the loop's: none may hold
    vmcnt(0), each holds 2 tiles x 16 MFMAs, and its waits are vmcnt(14): eight chunks of two loads in flight, less the one being consumed;
  * the loops round to bf16 with the packed conversion (v_cvt_pk_bf16_f32), four per fragment, one fragment per MFMA.
The VGPR counts are printed (pytest -s) for profiles/r16_w4_rows.md.
"""
import os
import re
import subprocess

import pytest

from radialog_amd import build
from test_isa_entry import CSRC, HIPCC, _bodies, _descriptors
from test_isa_wcode import _k_loops

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")

XSTAT = r"_ZN3rdx12xstat16_w4_kILi[04]EEEvNS_8GemmArgsE"
XROW = "_ZN3rdx11xrow16_w4_kENS_8GemmArgsE"


@pytest.fixture(scope="module")
def xs16_asm(tmp_path_factory):
    d = tmp_path_factory.mktemp("isa_w4_rows")
    o = d / "xs16.s"
    flags = [f for f in build.unit_flags("xs16.hip") if not f.startswith("-W")]
    p = subprocess.run([HIPCC] + flags + ["-S", "--cuda-device-only", "-I" + CSRC, os.path.join(CSRC, "xs16.hip"), "-o", str(o)],
                       capture_output=True, text=True, cwd=str(d))
    assert p.returncode == 0 and o.exists(), p.stderr[-2000:]
    return o.read_text()


def _names(bodies):
    xs = sorted(n for n in bodies if re.match(XSTAT, n))
    assert len(xs) == 2, f"{len(xs)} instantiations of xstat16_w4_k found, 2 expected (EPI_NONE, EPI_SILU_MUL): the scan no longer matches the assembly"
    assert XROW in bodies, sorted(n for n in bodies if "w4" in n)
    return xs, XROW


def _blocks(body):
    """the kernel's basic blocks: instruction lines split at labels and behind branches"""
    blk, out = [], []
    for l in body:
        x = l.split(";")[0].strip()
        if not x:
            continue
        if re.match(r"^\.LBB\d+_\d+:$", x):
            out.append(blk)
            blk = []
            continue
        blk.append(x)
        if re.match(r"^s_c?branch", x):
            out.append(blk)
            blk = []
    out.append(blk)
    return [b for b in out if b]


def _is_nt_load(x):
    return x.startswith("global_load_dwordx4") and re.search(r"\bnt\b", x) is not None


def test_w4_rows_kernels_exist_and_hold_no_scratch(xs16_asm):
    bodies, desc = _bodies(xs16_asm), _descriptors(xs16_asm)
    xs, xr = _names(bodies)
    for n in xs + [xr]:
        d = desc[n]
        assert d["private_segment_fixed_size"] == 0, (n, d["private_segment_fixed_size"])
        assert "scratch_" not in "\n".join(bodies[n]), n
        print(f"{n}: next_free_vgpr {d['next_free_vgpr']}")
    assert all(desc[n]["next_free_vgpr"] <= 256 for n in xs) and desc[xr]["next_free_vgpr"] <= 128      # 2 / 4 waves per SIMD


def test_xrow16_w4_k_loop_waits_counted_and_converts_packed(xs16_asm):
    bodies = _bodies(xs16_asm)
    _, xr = _names(bodies)
    loops = list(_k_loops(bodies[xr]))
    assert len(loops) >= 1, "no K loop found in xrow16_w4_k: the scan no longer matches"
    for loop in loops:
        assert any(re.match(r"^s_waitcnt\b.*vmcnt\(\d+\)", x) for x in loop)
        assert not [x for x in loop if re.match(r"^s_waitcnt\b.*vmcnt\(0\)", x)], "vmcnt(0) inside the K loop"
        cv, mf = sum(x.startswith("v_cvt_pk_bf16_f32") for x in loop), sum(x.startswith("v_mfma") for x in loop)
        assert mf == 16 and cv == 4 * mf, (cv, mf)          # a trip of four chunks, four fragments each


def test_xrow16_w4_guarded_first_trip_waits_counted(xs16_asm):
    """At the production down_proj (K = 11008: six or seven int4 chunks per wave) the unguarded loop above never runs: a wave takes the guarded first trip
    (four chunks, each fragment behind its wave-uniform test, the ring refilled) and the tail. The first trip's blocks are those that decode, multiply
    and stand in front of the loop; its refills (non-temporal 16-byte loads) stand in blocks of their own or beside the MFMAs. None of the blocks between
    the prologue's loads and the loop may drain the queue: every wait there is counted, vmcnt(6) at the least (the refill of the chunk just consumed is
    in flight: two weight loads and four activation fragments)."""
    bodies = _bodies(xs16_asm)
    _, xr = _names(bodies)
    blocks = _blocks(bodies[xr])
    loop = next(iter(_k_loops(bodies[xr])))
    n_loop = sum(x.startswith("v_mfma") for x in loop)
    # the blocks in front of the loop's block, from the first one that refills (the prologue's loads stand in blocks without MFMAs or conversions)
    idx_loop = next(i for i, b in enumerate(blocks) if sum(x.startswith("v_mfma") for x in b) == n_loop and any(_is_nt_load(x) for x in b))
    first = [b for b in blocks[:idx_loop] if any(x.startswith("v_mfma") or x.startswith("v_cvt_pk_bf16_f32") for x in b)]
    assert sum(sum(x.startswith("v_mfma") for x in b) for b in first) == 16, "the guarded first trip: 16 MFMAs in front of the loop expected"
    span = blocks[blocks.index(first[0]):idx_loop]
    assert sum(sum(_is_nt_load(x) for x in b) for b in span) == 4, "the first trip refills its four chunks"
    waits = [int(m.group(1)) for b in span for x in b for m in [re.match(r"^s_waitcnt\b.*vmcnt\((\d+)\)", x)] if m]
    assert waits and min(waits) >= 6, waits


def test_xstat16_w4_prefetching_trips_wait_counted_and_convert_packed(xs16_asm):
    bodies = _bodies(xs16_asm)
    xs, _ = _names(bodies)
    for n in xs:
        trips = [b for b in _blocks(bodies[n]) if any(x.startswith("v_mfma") for x in b) and any(x.startswith("v_cvt_pk_bf16_f32") for x in b)
                 and any(_is_nt_load(x) for x in b)]
        assert len(trips) >= 2, (n, len(trips), "prefetching trips (the peeled first one and the loop's) expected")
        for b in trips:
            waits = [int(m.group(1)) for x in b for m in [re.match(r"^s_waitcnt\b.*vmcnt\((\d+)\)", x)] if m]
            mf, cv = sum(x.startswith("v_mfma") for x in b), sum(x.startswith("v_cvt_pk_bf16_f32") for x in b)
            assert (mf, cv) == (32, 128), (n, mf, cv)
            assert sum(_is_nt_load(x) for x in b) == 8, n                      # the eight chunks refilled
            assert waits and 0 not in waits, (n, waits)
            assert waits.count(14) >= 8 and min(waits) >= 13, (n, waits)       # (13: the first trip's bias load, where there is a bias)
