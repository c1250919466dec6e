"""Build-quality guard (CPU: hipcc cross-compiles gfx950 without a GPU) for the kernel of prompt-lookup decoding (csrc/lookup.hip): the unit compiled with
build.py's own flags holds lookup_accept_k for both model dtypes, and neither build has a private (scratch) segment -- the kernel sits on the serial path
of every forward of rdx_generate_lookup. The register counts are printed (pytest -s)."""
import os
import re
import subprocess

import pytest

from radialog_amd import build
from test_isa_entry import CSRC, HIPCC, _descriptors

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


@pytest.fixture(scope="module")
def lookup_asm(tmp_path_factory):
    d = tmp_path_factory.mktemp("isa_lookup")
    o = d / "lookup.s"
    flags = [f for f in build.unit_flags("lookup.hip") if not f.startswith("-W")]
    p = subprocess.run([HIPCC] + flags + ["-S", "--cuda-device-only", "-I" + CSRC, os.path.join(CSRC, "lookup.hip"), "-o", str(o)], capture_output=True, text=True, cwd=str(d))
    assert p.returncode == 0 and o.exists(), p.stderr[-2000:]
    return o.read_text()


def test_lookup_accept_kernel_exists_and_holds_no_scratch(lookup_asm):
    desc = _descriptors(lookup_asm)
    ks = sorted(n for n in desc if re.match(r"_ZN3rdx15lookup_accept_kI(DF16_|DF16b)EE", n))
    assert len(ks) == 2, (sorted(desc), "one build per model dtype expected")
    for n in ks:
        assert desc[n]["private_segment_fixed_size"] == 0, (n, desc[n]["private_segment_fixed_size"])
        print(f"{n}: next_free_vgpr {desc[n]['next_free_vgpr']}")


def test_the_units_are_part_of_the_product_library():
    assert "lookup.hip" in build.SOURCES and "lookup.hip" not in build.HOOK_SOURCES
    assert "api_lookup.hip" in build.SOURCES and "api_lookup.hip" not in build.HOOK_SOURCES
