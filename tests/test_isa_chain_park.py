"""Build-quality guard (CPU: hipcc cross-compiles gfx950 without a GPU) for the parked pre-decode of decode_chain_wc_k's QKV role (csrc/chain.hip,
chain_tile PARK), with the helpers of tests/test_isa_entry.py and tests/test_isa_wcode.py on the assembly of chain.hip compiled with build.py's own flags:

  * no scratch and at most 128 VGPRs;
  * a ds_write_b128 (a parked fragment) and a v_perm_b32 (the last instruction of a fragment's decode) stand in front of the hand-off barrier that
    follows the poll loop's nap, and no MFMA does;
  * in the QKV role's text no global_load_dwordx4 stands between the last load of the ring and that barrier: from the role's first load to the barrier
    there are exactly the ring's loads, three 16-byte loads for each of its four coded chunks. This is what the parked pre-decode exists for: a refill
    in front of the hand-off puts its bytes ahead of the activation row, which returns behind them.

Like tests/test_isa_chain_predecode.py this reads the linear order of the emitted text (the QKV role is laid out first, its K loops behind its
hand-off): a compiler that lays the blocks out differently can fail it with no change of behaviour; then re-read the assembly and re-pin the scan."""
import os

import pytest

from test_isa_entry import HIPCC, _bodies, _descriptors, first_loads
from test_isa_wcode import CHAIN, chain_asm      # noqa: F401  (fixture)

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")

RING_LOADS = 4 * 3          # the QKV role's ring: four coded chunks of three 16-byte loads (and one 4-byte load) each


def _ins(body):
    return [l.split(";")[0].strip() for l in body]


def _handoff_barrier(ins):
    """Index of the barrier of the hand-off wait: the first barrier behind the first nap of the poll loop."""
    naps = [i for i, x in enumerate(ins) if x.startswith("s_sleep")]
    assert naps, "no poll loop found: the scan no longer matches the assembly"
    bar = next((i for i in range(naps[0], len(ins)) if ins[i].startswith("s_barrier")), None)
    assert bar is not None, "no barrier behind the poll loop"
    return bar


def test_no_scratch_and_at_most_128_vgprs(chain_asm):      # noqa: F811
    bodies, desc = _bodies(chain_asm), _descriptors(chain_asm)
    d = desc[CHAIN]
    print(f"decode_chain_wc_k: {d['next_free_vgpr']} VGPRs, {d['private_segment_fixed_size']} bytes of scratch")
    assert d["private_segment_fixed_size"] == 0 and "scratch_" not in "\n".join(bodies[CHAIN])
    assert d["next_free_vgpr"] <= 128, d["next_free_vgpr"]


def test_fragments_are_decoded_and_parked_in_front_of_the_handoff_barrier(chain_asm):      # noqa: F811
    ins = _ins(_bodies(chain_asm)[CHAIN])
    head = ins[:_handoff_barrier(ins)]
    assert any(x.startswith("ds_write_b128") for x in head), "no 16-byte LDS store in front of the hand-off barrier"
    assert any(x.startswith("v_perm_b32") for x in head), "no decode (v_perm_b32) in front of the hand-off barrier"
    assert not any(x.startswith("v_mfma") for x in head), "an MFMA in front of the hand-off barrier: the QKV role is no longer laid out first"


def test_no_weight_load_between_the_ring_and_the_handoff_barrier(chain_asm):      # noqa: F811
    body = _bodies(chain_asm)[CHAIN]
    ins = _ins(body)
    bar = _handoff_barrier(ins)
    sites, _ = first_loads(body)
    qkv = [i for i in sites if i < bar]
    assert len(qkv) == 1, (sorted(sites), bar)                 # the QKV role's first load; the down_proj role's lies behind the barrier in the text
    loads = [i for i in range(qkv[0], bar) if ins[i].startswith("global_load_dwordx4")]
    assert len(loads) == RING_LOADS, f"{len(loads)} 16-byte loads between the QKV role's first load and its hand-off barrier, the ring is {RING_LOADS}"
    assert loads[-1] - loads[0] < 40, "the ring's loads are not issued together: the scan no longer matches the assembly"
