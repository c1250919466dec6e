"""The decode step, family by family, computes the bits it computed before its host code was rebuilt around one argument builder per unit
(csrc/api_dispatch.hip: dec_attn_args, unit_args and the per-family decorators; csrc/api_llama.hip: one function per row family).

That change touched no kernel, no launch geometry and no kernel argument, so the bar is equality of bits. tests/golden/step_bits.json holds
SHA-256 digests of the greedy tokens and of every step's logits, recorded on the commit BEFORE the change (`python
tests/test_gpu_step_bits.py --write FILE [KEY ...]` run from the root of the tree to record: it imports radialog_amd from the working
directory; with KEYs only those cases are recorded and merged into FILE). Every case was recorded twice there and the two recordings were
equal. One case per edge of every family the step chooses from: the chained launch (batch <= 2) with its un-fused and un-chained legs, xs16
(3 and 16 rows), the 32-row family (4 rows with xs16 off, 17 and 32 rows: K-split slabs pending into the next and into the final RMSNorm;
fp8 activations at 4 and 32 rows), the row-block family (33 rows: a ragged third row tile; 128 rows; RDX_BLK_DOWN=0: the weight-stationary
down_proj) and its fp8 form (40 and 128 rows), and the small config, whose widths the activation-stationary kernels refuse (the generic GEMV
behind a stand-alone RMSNorm). The prompts' prefill variants (wstat / row-block kernels at 72 rows, the K-split prompt down_proj, the tile
GEMMs above 384 rows, gemm8) ride along in the same digests.

The cases on an int4 engine ("weights_w4", with and without the "w4" option), plain bf16 at 2 rows and "wcode=0" were recorded the same way, on the
commit before the choice of which copy of a weight each unit streams moved into one table (csrc/api_dispatch.hip stream_wants): host code again.

(The commit the digests come from read RDX_BLK_DOWN once per PROCESS, in a function-local static: there the RDX_BLK_DOWN=0 case had to be
recorded by a run of its own.)"""
import hashlib
import json
import os
import sys

if __name__ == "__main__":          # recording run (--write): the tree in the working directory is the one that is recorded
    sys.path.insert(0, os.getcwd())

import pytest
import torch

from radialog_amd import synth
from radialog_amd.config import LlamaCfg, RaDialogCfg, small_cfg

pytestmark = pytest.mark.gpu

T_PROMPT, N_NEW = 72, 8
ENV_SWITCHES = ("RDX_FUSE_AO", "RDX_CHAIN", "RDX_BLK_DOWN")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "step_bits.json")

# (widths, batch, dtype, fp8 weights, setting): setting = "default", an environment switch "NAME=0" read at rdx_create, an option "name=0", or
# "weights_w4" (an int4 engine, RdxEngine(weights_w4=True)), alone or with an option behind a comma
CASES = [("prod2", 1, "bf16", False, "default"), ("prod2", 1, "f16", False, "default"),
         ("prod2", 1, "bf16", False, "RDX_FUSE_AO=0"), ("prod2", 1, "bf16", False, "RDX_CHAIN=0"), ("prod2", 1, "bf16", False, "prompt_blk=0"),
         ("prod2", 2, "bf16", True, "default"),
         ("prod2", 3, "bf16", False, "default"), ("prod2", 16, "bf16", False, "default"),
         ("prod2", 4, "bf16", False, "xs16=0"),
         ("prod2", 17, "bf16", False, "default"), ("prod2", 17, "f16", False, "default"), ("prod2", 32, "bf16", False, "default"),
         ("prod2", 4, "bf16", True, "default"), ("prod2", 32, "bf16", True, "default"),
         ("prod2", 33, "bf16", False, "default"), ("prod2", 33, "f16", False, "default"), ("prod2", 128, "bf16", False, "default"),
         ("prod2", 33, "bf16", False, "RDX_BLK_DOWN=0"),
         ("prod2", 40, "bf16", True, "default"), ("prod2", 128, "bf16", True, "default"),
         ("small", 1, "bf16", False, "default"), ("small", 1, "f16", False, "default"),
         ("small", 4, "bf16", False, "default"), ("small", 18, "bf16", False, "default"),
         # which copy of a weight each unit streams (api_dispatch.hip unit_stream): int4 in the chained family (1, 2), in xs16 (3, 16) and not beyond (17),
         # the packed copy with "w4" off; plain bf16: the coded copies at 2 rows, the raw ones with "wcode" off
         ("prod2", 1, "bf16", False, "weights_w4"), ("prod2", 2, "bf16", False, "weights_w4"), ("prod2", 3, "bf16", False, "weights_w4"),
         ("prod2", 16, "bf16", False, "weights_w4"), ("prod2", 17, "bf16", False, "weights_w4"),
         ("prod2", 1, "bf16", False, "weights_w4,w4=0"), ("prod2", 3, "bf16", False, "weights_w4,w4=0"),
         ("prod2", 2, "bf16", False, "default"), ("prod2", 1, "bf16", False, "wcode=0")]


def _key(which, B, dtype, fp8, setting):
    return f"{which}-B{B}-{dtype}-fp8{int(fp8)}-{setting}"


def _case_digests(env, which, B, dtype, fp8, setting):
    """{"eager": digest, "graph": digest} of one case: one two-layer engine, 8 eager steps and 8 replayed ones from the same prompt."""
    from radialog_amd import _lib
    from radialog_amd.engine import RdxEngine, synth_getter
    cfg = small_cfg() if which == "small" else RaDialogCfg(llama=LlamaCfg(layers=2, qformer_dim=192))
    for name in ENV_SWITCHES:
        env.delenv(name, raising=False)
    _, w4, setting = setting.rpartition("weights_w4")
    name, _, value = (setting.lstrip(",") or "default").partition("=")
    if name in ENV_SWITCHES:
        env.setenv(name, value)
    eng = RdxEngine(cfg, dtype=dtype, device=0, max_batch=B, max_len=128, lora=True, vision=False, weights_fp8=fp8, weights_w4=bool(w4))
    eng.load_weights(synth_getter(cfg, eng.device, lora=True), vision=False)
    if name != "default" and name not in ENV_SWITCHES:
        eng.set_option(name, int(value))
    ids = synth.synth_prompt_ids(B, T_PROMPT, vocab=cfg.llama.vocab, img_offset=6, pad_rows=False, seed=33)
    if B > 1:                                  # left-pad row 1 by 5 (pad id 0), keep 32 <IMG> inside
        ids[1] = torch.cat([torch.zeros(5, dtype=torch.long), ids[1, : T_PROMPT - 5]])
    qf = synth.synth("t.qf2", (B, 32, cfg.llama.qformer_dim), -1.0, 1.0)
    got = {}
    for mode, use_graph in (("eager", False), ("graph", True)):
        toks, scores, n = eng.generate(ids, qf, max_new=N_NEW, eos_id=-1, output_scores=True, use_graph=use_graph)
        assert n == N_NEW
        h = hashlib.sha256()
        h.update(toks.cpu().long().contiguous().numpy().tobytes())
        h.update(scores.cpu().contiguous().view(torch.int16).numpy().tobytes())
        got[mode] = h.hexdigest()
    if B <= 2:                  # which family ran: rdx_time(7) brackets the chained launch and fails where the step has none
        if name in ("RDX_FUSE_AO", "RDX_CHAIN"):
            with pytest.raises(_lib.RdxError, match="not active"):
                eng.time_unit(7, 1)
        else:
            assert eng.time_unit(7, 1) > 0.0
    eng.close()
    return got


@pytest.mark.parametrize("which,B,dtype,fp8,setting", CASES, ids=[_key(*c) for c in CASES])
def test_decode_step_computes_the_recorded_bits(monkeypatch, which, B, dtype, fp8, setting):
    """Tokens and the logits of all 8 steps, eager and as a replayed graph, are bit for bit what the step computed before its host code was
    rebuilt."""
    with open(GOLDEN) as f:
        want = json.load(f)[_key(which, B, dtype, fp8, setting)]
    got = _case_digests(monkeypatch, which, B, dtype, fp8, setting)
    print(f"{_key(which, B, dtype, fp8, setting)}: eager {got['eager'][:16]} graph {got['graph'][:16]} (recorded {want['eager'][:16]} {want['graph'][:16]})")
    assert got == want


if __name__ == "__main__":
    class _Env:
        def setenv(self, k, v): os.environ[k] = v
        def delenv(self, k, raising=False): os.environ.pop(k, None)
    path = sys.argv[sys.argv.index("--write") + 1]
    only = sys.argv[sys.argv.index("--write") + 2:]
    got = {}
    if only and os.path.exists(path):
        with open(path) as f:
            got = json.load(f)
    for c in CASES:
        if not only or _key(*c) in only:
            got[_key(*c)] = _case_digests(_Env(), *c)
            print(_key(*c), got[_key(*c)], flush=True)
    with open(path, "w") as f:
        json.dump(got, f, indent=1, sort_keys=True)
        f.write("\n")
