"""The decoder on int4 group-quantised weights (RdxEngine(weights_w4=True): RDX_W_GEMM_W4, radialog_amd/w4.py). int4 is a storage format of the
batch <= 2 step's weight stream, not an arithmetic: engine A (weights_w4) must compute, bit for bit, what engine B computes -- a plain bf16 engine
whose getter hands it dequantize(quantize(w)) for the seven projections. Tokens and every step's scores are compared at batch 1 and 2 (the int4
kernels), eager and as a replayed graph, and at batch 3 and in one score() call (the packed copy of the dequantised weight: no int4 kernel runs).

WHICH kernels ran is seen through the launch counters (rdx_w4_stats): a dispatch that quietly fell back to the bf16 kernels would pass every
comparison of bits. Per eager step of the batch <= 2 chained family (api_llama.hip step_chained) with "w4" on:
    int4 GEMVs           = 1 (layer 0's stand-alone QKV) + layers (every gate/up)      -- o_proj is inside the fused attention launch, the lm_head is bf16
    int4 chained launches = layers                                                      -- down_proj(l) -> QKV(l + 1), one launch per layer
A generate of N_NEW tokens launches N_NEW - 1 steps (the prefill selects the first token); a graph is captured once and counts once."""
import numpy as np
import pytest
import torch

from radialog_amd import synth, w4
from radialog_amd.config import LlamaCfg, RaDialogCfg, small_cfg
from radialog_amd.engine import LogitsRules, Sampling

pytestmark = pytest.mark.gpu

T_PROMPT, N_NEW, MAX_B = 40, 12, 3
PROJ = tuple(f"{p}_proj.weight" for p in ("q", "k", "v", "o", "gate", "up", "down"))


def _cfg(which):
    return small_cfg() if which == "small" else RaDialogCfg(llama=LlamaCfg(layers=2, qformer_dim=192))


def _engines(which):
    from radialog_amd.engine import RdxEngine, synth_getter
    cfg = _cfg(which)
    a = RdxEngine(cfg, dtype="bf16", device=0, max_batch=MAX_B, max_len=128, lora=True, vision=False, weights_w4=True)
    a.load_weights(synth_getter(cfg, a.device, lora=True), vision=False)
    b = RdxEngine(cfg, dtype="bf16", device=0, max_batch=MAX_B, max_len=128, lora=True, vision=False)
    inner = synth_getter(cfg, b.device, lora=True)

    def get(name):
        t = inner(name)
        if name.endswith(PROJ):          # (the LoRA tensors end in lora_A.weight / lora_B.weight)
            t = torch.from_numpy(w4.dequantize(w4.quantize(t.float().cpu().numpy()))).to(t.device)
        return t
    b.load_weights(get, vision=False)
    return cfg, a, b


@pytest.fixture(scope="module", params=["small", "prod2"])
def pair(request):
    cfg, a, b = _engines(request.param)
    yield cfg, a, b
    a.close()
    b.close()


def _inputs(cfg, B):
    ids = synth.synth_prompt_ids(B, T_PROMPT, vocab=cfg.llama.vocab, img_offset=6, pad_rows=False, seed=41)
    if B > 1:
        ids[1] = torch.cat([torch.zeros(3, dtype=torch.long), ids[1, : T_PROMPT - 3]])
    qf = synth.synth("t.w4.qf", (B, 32, cfg.llama.qformer_dim), -1.0, 1.0)
    return ids, qf


def _generate(cfg, eng, B, use_graph, **kw):
    ids, qf = _inputs(cfg, B)
    toks, scores, n = eng.generate(ids, qf, max_new=N_NEW, eos_id=-1, output_scores=True, use_graph=use_graph, **kw)
    assert n == N_NEW
    return toks.cpu().clone(), scores.cpu().contiguous().view(torch.int16).clone()


def _launches(eng):
    return eng.w4_stats()[3:]


@pytest.mark.parametrize("B", [1, 2])
def test_w4_step_equals_the_bf16_step_on_the_dequantised_weights(pair, B):
    cfg, a, b = pair
    L = cfg.llama.layers
    assert b.w4_stats() == (0, 0, 0, 0, 0)
    for use_graph in (False, True):
        a.set_option("w4", 1)
        n0 = _launches(a)
        t1, s1 = _generate(cfg, a, B, use_graph)
        n1 = _launches(a)
        a.set_option("w4", 0)
        t0, s0 = _generate(cfg, a, B, use_graph)
        n2 = _launches(a)
        a.set_option("w4", 1)
        t2, s2 = _generate(cfg, a, B, use_graph)
        n3 = _launches(a)
        tb, sb = _generate(cfg, b, B, use_graph)
        steps = (N_NEW - 1) if not use_graph else 1          # a graph: captured once (the option dropped the old one)
        want = (steps * (L + 1), steps * L)
        assert (n1[0] - n0[0], n1[1] - n0[1]) == want, f"int4 launches with the option on (graph={use_graph})"
        assert n2 == n1, f"int4 launches with the option off (graph={use_graph})"
        assert (n3[0] - n2[0], n3[1] - n2[1]) == want, f"the option dropped the graph and switched back (graph={use_graph})"
        assert torch.equal(t1, tb) and torch.equal(s1, sb), f"int4 stream != bf16 engine on W' (graph={use_graph})"
        assert torch.equal(t0, tb) and torch.equal(s0, sb), f"packed W' copy != bf16 engine on W' (graph={use_graph})"
        assert torch.equal(t2, t1) and torch.equal(s2, s1), f"the option does not switch back (graph={use_graph})"
    assert b.w4_stats() == (0, 0, 0, 0, 0)
    assert a.time_unit(7, 1) > 0.0         # the chained family is the one that ran


def test_batch_3_and_score_run_no_int4_kernel(pair):
    cfg, a, b = pair
    n0 = _launches(a)
    ta, sa = _generate(cfg, a, 3, False)
    tb, sb = _generate(cfg, b, 3, False)
    assert torch.equal(ta, tb) and torch.equal(sa, sb)
    ids, qf = _inputs(cfg, 2)
    labels = ids.clone().to(torch.int32)
    labels[:, :8] = -100
    la = a.score(ids, qf, labels, want_top1=True)
    lb = b.score(ids, qf, labels, want_top1=True)
    assert torch.equal(la[0].cpu().view(torch.int32), lb[0].cpu().view(torch.int32)) and torch.equal(la[1].cpu(), lb[1].cpu())
    assert _launches(a) == n0 and _launches(b) == (0, 0)


def test_tile_counts(pair):
    cfg, a, _ = pair
    L = cfg.llama
    qkv_pad = (3 * L.hidden + 2 * L.lora_r + 15) // 16 * 16
    raw = L.layers * (qkv_pad - 3 * L.hidden) // 16                                       # exactly the LoRA-A tiles
    int4 = L.layers * (3 * L.hidden // 16 + 2 * L.inter // 16 + L.hidden // 16)           # q / k / v rows, gate/up, down_proj (o_proj: no stream)
    chunk = lambda rows, k: (rows // 16) * (k // 128) * w4.CHUNK_BYTES + (rows // 16) * 4
    nbytes = L.layers * (chunk(qkv_pad, L.hidden) + chunk(2 * L.inter, L.hidden) + chunk(L.hidden, L.inter))
    tiles, rawt, got_bytes = a.w4_stats()[:3]
    assert (tiles, rawt, got_bytes) == (int4, raw, nbytes) and raw == L.layers * 1
    assert a.wcode_stats()[0] == (L.vocab + 15) // 16           # of the coded copies only the lm_head's is left


def test_sampling_and_logits_rules_compose(pair):
    cfg, a, b = pair
    for kw in (dict(sampling=Sampling(temperature=0.8, top_k=50, top_p=0.9, seed=1234)), dict(logits_rules=LogitsRules(1.3, 3, 4))):
        n0 = _launches(a)
        ta, sa = _generate(cfg, a, 2, False, **kw)
        tb, sb = _generate(cfg, b, 2, False, **kw)
        assert torch.equal(ta, tb) and torch.equal(sa, sb), kw
        n1 = _launches(a)
        assert (n1[0] - n0[0], n1[1] - n0[1]) == ((N_NEW - 1) * (cfg.llama.layers + 1), (N_NEW - 1) * cfg.llama.layers)
    a.set_sampling(None)
    b.set_sampling(None)
    a.set_logits_rules(None)
    b.set_logits_rules(None)
