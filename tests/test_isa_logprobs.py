"""Build-quality guard (CPU: hipcc cross-compiles gfx950 without a GPU) for the kernel of the generation log-probs (csrc/logprob.hip): the unit compiled
with build.py's own flags holds logprob_step_k for both model dtypes, neither build has a private (scratch) segment -- the kernel runs behind every decode
step, and a spill would put a scratch round trip into each of its nine passes over the LDS row -- and the unit is part of the library and of its source
hash. The VGPR counts are printed (pytest -s)."""
import os
import re
import subprocess

import pytest

from radialog_amd import build
from test_isa_entry import CSRC, HIPCC, _descriptors
from test_isa_kv8 import _directive_lines

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


@pytest.fixture(scope="module")
def logprob_asm(tmp_path_factory):
    d = tmp_path_factory.mktemp("isa_logprobs")
    o = d / "logprob.s"
    flags = [f for f in build.unit_flags("logprob.hip") if not f.startswith("-W")]
    p = subprocess.run([HIPCC] + flags + ["-S", "--cuda-device-only", "-I" + CSRC, os.path.join(CSRC, "logprob.hip"), "-o", str(o)], capture_output=True, text=True, cwd=str(d))
    assert p.returncode == 0 and o.exists(), p.stderr[-2000:]
    return o.read_text()


def test_logprob_unit_is_built_and_hashed():
    assert "logprob.hip" in build.SOURCES and "logprob.hip" not in build.HOOK_SOURCES


def test_logprob_step_kernels_exist_and_hold_no_scratch(logprob_asm):
    desc = _descriptors(logprob_asm)
    ks = sorted(n for n in desc if re.match(r"_ZN3rdx14logprob_step_kI(DF16_|DF16b)EE", n))
    assert len(ks) == 2, (ks, "one build per model dtype expected")
    for n in ks:
        assert ".amdhsa_private_segment_fixed_size 0" in _directive_lines(logprob_asm, n), n
        assert desc[n]["private_segment_fixed_size"] == 0, (n, desc[n]["private_segment_fixed_size"])
        print(f"{n}: next_free_vgpr {desc[n]['next_free_vgpr']}")
