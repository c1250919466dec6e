"""The chained down_proj(l) -> RMSNorm + QKV(l+1) launch of the batch <= 2 step (csrc/chain.hip: decode_chain_k) after the QKV role's weight
ring went from 8 to 16 fragments per wave (profiles/r07_chain_seam.md), and the in-situ timeline hook that measured the seam
(rdx_gemv_trace 7).

A deeper ring only changes WHEN a chunk is fetched: every wave still multiplies the same chunks in the same order and the partial sums are
added in the same order, so the bar is equality of bits with the kernel as it was. tests/golden/chain_seam_bits.json holds SHA-256 digests
of the greedy tokens and of the logits of all 24 steps, recorded with the 8-fragment kernel (`python tests/test_gpu_chain_seam.py --write
FILE` run from the root of the tree to record: it imports radialog_amd from the working directory) on the small config and on two
production-width layers (4096 / 11008), batch 1 and 2, fp16 and bf16, model-dtype and fp8 weights. (One kernel per unit, RDX_CHAIN=0, is no
bit-exact reference: its down_proj and gate/up take other kernels with other K splits; measured, 363 431 of 768 024 logits differ by an ulp.)"""
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

T_PROMPT, N_STEPS = 72, 24


def _prompt(cfg, B):
    ids = synth.synth_prompt_ids(B, T_PROMPT, vocab=cfg.llama.vocab, img_offset=6, pad_rows=False, seed=33)
    if B > 1:                                  # left-pad row 1 by 5 (pad id 0), keep 32 <IMG> inside
        ids[1] = torch.cat([torch.zeros(5, dtype=torch.long), ids[1, : T_PROMPT - 5]])
    return ids


def _engine(monkeypatch, cfg, chain, dtype, fp8):
    from radialog_amd.engine import RdxEngine, synth_getter
    if chain is None:
        monkeypatch.delenv("RDX_CHAIN", raising=False)
    else:
        monkeypatch.setenv("RDX_CHAIN", str(chain))
    eng = RdxEngine(cfg, dtype=dtype, device=0, max_batch=2, max_len=128, lora=True, vision=False, weights_fp8=fp8)
    eng.load_weights(synth_getter(cfg, eng.device, lora=True), vision=False)
    return eng


def _run(eng, cfg, B):
    ids = _prompt(cfg, B)
    qf = synth.synth("t.qf2", (B, 32, cfg.llama.qformer_dim), -1.0, 1.0)
    out = {}
    for use_graph in (False, True):
        toks, scores, n = eng.generate(ids, qf, max_new=N_STEPS, eos_id=-1, output_scores=True, use_graph=use_graph)
        assert n == N_STEPS
        out[use_graph] = (toks.cpu().clone(), scores.cpu().clone())
    return out


def _same(a, b, what):
    for g in (False, True):
        for h in (False, True):
            assert torch.equal(a[g][0], b[h][0]), f"{what}: greedy tokens differ (graph {g} vs {h})"
            assert torch.equal(a[g][1].view(torch.int16), b[h][1].view(torch.int16)), \
                f"{what}: logits differ in {(a[g][1] != b[h][1]).sum().item()} places (graph {g} vs {h})"


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "chain_seam_bits.json")
CASES = [(w, B, dt, fp8) for w in ("small", "prod2") for B in (1, 2) for dt in ("f16", "bf16") for fp8 in (False, True)]


def _cfg(which):
    return small_cfg() if which == "small" else RaDialogCfg(llama=LlamaCfg(layers=2, qformer_dim=192))


def _digest(out):
    toks, scores = out
    h = hashlib.sha256()
    h.update(toks.long().contiguous().numpy().tobytes())
    h.update(scores.contiguous().view(torch.int16).numpy().tobytes())
    return h.hexdigest()


def _case_digest(monkeypatch, which, B, dtype, fp8):
    cfg = _cfg(which)
    eng = _engine(monkeypatch, cfg, None, dtype, fp8)
    out = _run(eng, cfg, B)
    assert eng.time_unit(7, 1) > 0.0            # the chained launch is what this context runs (rdx_time 7 fails where it is not active)
    eng.close()
    _same(out, out, "chained launch, eager vs graph")
    return _digest(out[True])


@pytest.mark.parametrize("which,B,dtype,fp8", CASES)
def test_chained_step_computes_the_recorded_bits(monkeypatch, which, B, dtype, fp8):
    """Tokens and the logits of all 24 steps, eager and as a replayed graph, are bit for bit what the chained launch computed with the
    8-fragment ring."""
    with open(GOLDEN) as f:
        want = json.load(f)[f"{which}-B{B}-{dtype}-fp8{int(fp8)}"]
    assert _case_digest(monkeypatch, which, B, dtype, fp8) == want


@pytest.mark.parametrize("B,dtype,fp8", [(1, "bf16", False), (2, "f16", False), (1, "f16", True)])
def test_seam_timeline_is_causal_and_leaves_the_step_alone(monkeypatch, B, dtype, fp8):
    """rdx_gemv_trace(7): one eager decode step with per-workgroup timestamps of one chained launch. Every down_proj workgroup stamps its
    stages in order; every QKV workgroup sees its inputs ready only after EVERY down_proj tile has been stored (the hand-off is what orders
    them, not luck); and tokens generated after traced steps are those generated before."""
    cfg = small_cfg()
    eng = _engine(monkeypatch, cfg, None, dtype, fp8)
    ids = _prompt(cfg, B)
    qf = synth.synth("t.qf2", (B, 32, cfg.llama.qformer_dim), -1.0, 1.0)
    first, _, _ = eng.generate(ids, qf, max_new=N_STEPS, eos_id=-1, use_graph=True)
    nwg = cfg.llama.hidden // 16
    nqkv = ((3 * cfg.llama.hidden + 16 + 15) // 16 + 3) // 4
    for _ in range(2):
        eng.generate(ids, qf, max_new=8, eos_id=-1, use_graph=False)
        tr = eng.gemv_trace(7, 0)
        d, q = tr[:nwg], tr[nwg:nwg + nqkv]
        assert (tr[nwg + nqkv:] == 0).all() and (d[:, 0] > 0).all() and (q[:, 0] > 0).all()
        for rec, order in ((d, (0, 5, 3, 6, 1, 7, 2)), (q, (0, 5, 3, 6, 1, 7))):       # entry, first KiB, inputs, first MFMA, K loop, end(, arrival)
            for a, b in zip(order, order[1:]):
                assert (rec[:, a] <= rec[:, b]).all(), f"slot {a} after slot {b}"
        assert int(q[:, 3].min()) >= int(d[:, 7].max()), "a QKV workgroup saw its inputs ready before the last down_proj tile was stored"
    again, _, _ = eng.generate(ids, qf, max_new=N_STEPS, eos_id=-1, use_graph=True)
    assert torch.equal(first.cpu(), again.cpu())
    eng.close()


def test_seam_timeline_reports_a_step_without_the_chained_launch(monkeypatch):
    from radialog_amd import _lib
    cfg = small_cfg()
    eng = _engine(monkeypatch, cfg, 0, "f16", False)
    ids = _prompt(cfg, 1)
    qf = synth.synth("t.qf2", (1, 32, cfg.llama.qformer_dim), -1.0, 1.0)
    eng.generate(ids, qf, max_new=8, eos_id=-1)
    with pytest.raises(_lib.RdxError, match="not active"):
        eng.gemv_trace(7, 0)
    eng.close()


if __name__ == "__main__":
    class _Env:
        def setenv(self, k, v): os.environ[k] = v
        def delenv(self, k, raising=False): os.environ.pop(k, None)
    got = {f"{w}-B{B}-{dt}-fp8{int(fp8)}": _case_digest(_Env(), w, B, dt, fp8) for w, B, dt, fp8 in CASES}
    with open(sys.argv[sys.argv.index("--write") + 1], "w") as f:
        json.dump(got, f, indent=1, sort_keys=True)
        f.write("\n")
