"""Build-quality guard (CPU: hipcc cross-compiles gfx950 without a GPU) for the entry blocks of the batch-1/2 decode step's kernels. Every launch of the
step pays its head before its weight stream starts, 97 times per token; these kernels therefore take what their first loads are addressed from as LEADING
scalar arguments, which kernarg preloading (radialog_amd/build.py UNIT_FLAGS) has in SGPRs when the first wave starts, and read everything else behind
those loads (csrc/rdx_common.h late_kernarg). Nothing fails functionally when that is lost -- an argument moved behind the struct, a field read early, a
flag dropped from one unit -- so it is pinned here, on the assembly of the units compiled with build.py's own per-unit flags:

  * `.amdhsa_user_sgpr_kernarg_preload_length` covers the dwords of the declared leading arguments;
  * behind the compatibility header (the scalar loads a firmware without preloading runs instead), on EVERY path from the kernel's entry the first
    16-byte global load comes before any scalar load and before any wait on the scalar/LDS counter -- per role: the weight roles' first load is the
    non-temporal ring, the attention role's are wave 0's qkv row and the cache waves' K fragments (plain loads: that role streams no weight);
  * no kernel has a private (scratch) segment.
"""
import os
import re
import subprocess

import pytest

from radialog_amd import build

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "radialog_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")

# kernel family -> (unit, regex on the mangled name, instantiations expected, dwords of the leading arguments, first-load sites, of which non-temporal)
#   decode_chain_k(const void*, const void*, int x 4, ChainArgs)                      8 dwords; roles: down_proj, QKV (both weight rings)
#   attn_oproj16_k(const void* x 2, void* x 2, int x 6, DecAttnArgs, ChainGemm, ..)  14 dwords; o_proj (ring), attention wave 0 and its cache waves
#   skinny_gemm_k(const void*, const void*, int, int, GemmArgs)                       6 dwords; the instantiations of the batch-1/2 step: one M tile, fused
#       RMSNorm, LDS-staged activations, 4 waves (more than 512 tiles: QKV = EPI 0, gate/up = EPI 4, lm_head = EPI 5), model-dtype and fp8 weights
T_ = r"(?:DF16_|DF16b)"          # f16 | bf16
FAMILIES = {
    "decode_chain_k": ("chain.hip", rf"_ZN3rdx14decode_chain_kI{T_}Lb[01]EEEv", 4, 8, 2, 2),
    "attn_oproj16_k": ("chain.hip", rf"_ZN3rdx14attn_oproj16_kI{T_}Lb[01]EEEv", 4, 14, 3, 1),
    "skinny_gemm_k": ("gemm.hip", rf"_ZN3rdx13skinny_gemm_kI{T_}Li1ELi[045]ELb1ELi4ELb1ELb[01]EEEv", 12, 6, 1, 1),
}


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    out = {}
    d = tmp_path_factory.mktemp("isa_entry")
    procs = []
    for unit in sorted({f[0] for f in FAMILIES.values()}):
        o = d / (unit + ".s")
        flags = [f for f in build.unit_flags(unit) if not f.startswith("-W")]
        cmd = [HIPCC] + flags + ["-S", "--cuda-device-only", "-I" + CSRC, os.path.join(CSRC, unit), "-o", str(o)]
        procs.append((unit, o, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=str(d))))
    for unit, o, p in procs:
        _, err = p.communicate()
        assert p.returncode == 0 and o.exists(), err[-2000:]
        out[unit] = o.read_text()
    return out


def test_units_carry_the_preload_flag():
    for unit in {f[0] for f in FAMILIES.values()}:
        assert any("amdgpu-kernarg-preload-count" in f for f in build.unit_flags(unit)), unit
    # the encoder and the batch >= 3 units keep their code
    for unit in ("xstat32.hip", "xs16.hip", "gemm8.hip", "gemm_dma.hip", "pconv.hip", "attn.hip"):
        assert build.unit_flags(unit) == build.FLAGS, unit


def test_source_hash_covers_the_unit_flags(monkeypatch):
    h = build.source_hash()
    monkeypatch.setattr(build, "UNIT_FLAGS", {})
    assert build.source_hash() != h, "a library built without the per-unit flags would pass for this tree's"


def _bodies(text):
    """mangled name -> the kernel's instruction lines (from its label to its .Lfunc_end)"""
    lines = text.split("\n")
    out = {}
    for i, l in enumerate(lines):
        m = re.match(r"^(_Z\w+):", l)
        if m:
            j = i + 1
            while j < len(lines) and not lines[j].startswith(".Lfunc_end"):
                j += 1
            out[m.group(1)] = lines[i + 1:j]
    return out


def _descriptors(text):
    """mangled name -> {directive: int} of its .amdhsa_kernel block"""
    out = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", text, re.S):
        out[m.group(1)] = {k: int(v) for k, v in re.findall(r"\.amdhsa_(\w+) (\d+)\s*$", m.group(2), re.M)}
    return out


SCALAR_LOAD = re.compile(r"^s_(?:buffer_)?load_")
LGKM_WAIT = re.compile(r"^s_waitcnt\b.*lgkmcnt")
BRANCH = re.compile(r"^s_(c?branch\w*)\s+(\.LBB\d+_\d+)")


def first_loads(body):
    """Walks every path from the first instruction behind the compatibility header (it ends in `.p2align 8`) until the path's first 16-byte global load.
    Returns (sites, offenders): sites = {line index of a first load: is it non-temporal}, offenders = [(line index, text)] of scalar loads / scalar-counter
    waits met before one. A path that ends (s_endpgm) without a load counts for neither."""
    ins = [l.split(";")[0].strip() for l in body]
    labels = {l[:-1]: i for i, l in enumerate(ins) if re.match(r"^\.LBB\d+_\d+:$", l)}
    aligns = [i for i, l in enumerate(ins) if re.match(r"^\.p2align\s+8$", l)]
    assert aligns, "no compatibility header: the kernel is not compiled for kernarg preloading"
    sites, offenders, seen, todo = {}, [], set(), [aligns[0] + 1]
    while todo:
        i = todo.pop()
        while i < len(ins) and i not in seen:
            seen.add(i)
            l = ins[i]
            if l.startswith("global_load_dwordx4"):
                sites[i] = bool(re.search(r"\bnt\b", l))
                break
            if SCALAR_LOAD.match(l) or LGKM_WAIT.match(l):
                offenders.append((i, l))
                break
            if l.startswith("s_endpgm"):
                break
            m = BRANCH.match(l)
            if m:
                assert m.group(2) in labels, l
                if m.group(1) == "branch":
                    i = labels[m.group(2)]
                    continue
                todo.append(labels[m.group(2)])
            i += 1
    return sites, offenders


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_first_loads_stand_in_front_of_every_scalar_load(family, asm):
    unit, pat, n_inst, lead, n_sites, n_nt = FAMILIES[family]
    text = asm[unit]
    bodies, desc = _bodies(text), _descriptors(text)
    names = sorted(n for n in bodies if re.match(pat, n))
    assert len(names) >= n_inst, f"{family}: {len(names)} instantiations found, {n_inst} named: the scan no longer matches the assembly"
    bad = []
    for n in names:
        d = desc[n]
        if d["user_sgpr_kernarg_preload_length"] < lead:
            bad.append((n, "preload length", d["user_sgpr_kernarg_preload_length"]))
        if d["private_segment_fixed_size"] != 0:
            bad.append((n, "scratch bytes", d["private_segment_fixed_size"]))
        sites, offenders = first_loads(bodies[n])
        if offenders:
            bad.append((n, "in front of a path's first load", offenders[:3]))
        if len(sites) < n_sites or sum(sites.values()) < n_nt:
            bad.append((n, f"first-load sites (non-temporal) found, {n_sites} ({n_nt}) expected", (len(sites), sum(sites.values()))))
    assert not bad, bad
    assert "scratch_" not in "\n".join("\n".join(bodies[n]) for n in names)
