"""Build-quality guard (CPU: hipcc cross-compiles gfx950 without a GPU) for the kernels of the fp8 KV cache (csrc/attn.hip): the unit compiled with
build.py's own flags holds the three decode-attention builds on the fp8 cache for both model dtypes, the prompt's quantiser and the read-back kernel,
and none of them has a private (scratch) segment. The 16- and 4-wave builds run under a 128-register cap; a spill there would put a scratch round trip
into the kernel's dependent chain. The VGPR counts are printed (pytest -s)."""
import os
import re
import subprocess

import pytest

from radialog_amd import build
from test_isa_entry import CSRC, HIPCC, _descriptors

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


@pytest.fixture(scope="module")
def attn_asm(tmp_path_factory):
    d = tmp_path_factory.mktemp("isa_kv8")
    o = d / "attn.s"
    flags = [f for f in build.unit_flags("attn.hip") if not f.startswith("-W")]
    p = subprocess.run([HIPCC] + flags + ["-S", "--cuda-device-only", "-I" + CSRC, os.path.join(CSRC, "attn.hip"), "-o", str(o)], capture_output=True, text=True, cwd=str(d))
    assert p.returncode == 0 and o.exists(), p.stderr[-2000:]
    return o.read_text()


def test_kv8_kernels_exist_and_hold_no_scratch(attn_asm):
    desc = _descriptors(attn_asm)
    att = sorted(n for n in desc if re.match(r"_ZN3rdx22decode_attention_kv8_kI(DF16_|DF16b)Li(16|8|4)EEE", n))
    assert len(att) == 6, (att, "three builds (16, 8, 4 waves) x two model dtypes expected")
    quant = sorted(n for n in desc if re.match(r"_ZN3rdx16kv8_quant_rows_kI", n))
    read = sorted(n for n in desc if re.match(r"_ZN3rdx10kv8_read_kI", n))
    assert len(quant) == 2 and len(read) == 2, (quant, read)
    for n in att + quant + read:
        assert f".amdhsa_private_segment_fixed_size 0" in _directive_lines(attn_asm, n), n
        assert desc[n]["private_segment_fixed_size"] == 0, (n, desc[n]["private_segment_fixed_size"])
        print(f"{n}: next_free_vgpr {desc[n]['next_free_vgpr']}")


def _directive_lines(asm, name):
    """The .amdhsa_ directives of one kernel's descriptor block."""
    m = re.search(r"\.amdhsa_kernel " + re.escape(name) + r"\n(.*?)\.end_amdhsa_kernel", asm, re.S)
    assert m, name
    return [l.strip() for l in m.group(1).split("\n")]
