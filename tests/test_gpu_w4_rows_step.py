"""The 3-16-row decode step on int4 group-quantised weights (RdxEngine(weights_w4=True); api_llama.hip step_xs16 with xstat16_w4_k / xrow16_w4_k). int4
is a storage format: engine A (weights_w4) must compute, bit for bit, what engine B computes -- a plain bf16 engine whose getter hands it
dequantize(quantize(w)) for the seven projections (the engine pair of tests/test_gpu_w4_step.py, here with room for 17 rows: 17 is the first batch
beyond the family).

WHICH kernels ran is seen through the launch counters (rdx_w4_rows_stats): per eager step of the 3-16-row family with "w4" on
    int4 xstat16 launches = 2 * layers (QKV and gate/up)        int4 xrow16 launches = layers (down_proj; o_proj has no int4 stream)
A generate of N_NEW tokens launches N_NEW - 1 steps (the prefill selects the first token); a graph is captured once and counts once. At batch 2 (the
chained family), 17 (the 32-row family) and at a hidden size other than 4096 (no 3-16-row family) the counters stand still."""
import pytest
import torch

from radialog_amd import synth, w4
from radialog_amd.config import LlamaCfg, RaDialogCfg, small_cfg

pytestmark = pytest.mark.gpu

T_PROMPT, N_NEW, MAX_B = 40, 6, 17
PROJ = tuple(f"{p}_proj.weight" for p in ("q", "k", "v", "o", "gate", "up", "down"))


def _engines(cfg):
    from radialog_amd.engine import RdxEngine, synth_getter
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
    return a, b


@pytest.fixture(scope="module")
def pair():
    cfg = RaDialogCfg(llama=LlamaCfg(layers=2, qformer_dim=192))
    a, b = _engines(cfg)
    yield cfg, a, b
    a.close()
    b.close()


def _inputs(cfg, B):
    ids = synth.synth_prompt_ids(B, T_PROMPT, vocab=cfg.llama.vocab, img_offset=6, pad_rows=False, seed=43)
    ids[1] = torch.cat([torch.zeros(3, dtype=torch.long), ids[1, : T_PROMPT - 3]])
    qf = synth.synth("t.w4rows.qf", (B, 32, cfg.llama.qformer_dim), -1.0, 1.0)
    return ids, qf


def _generate(cfg, eng, B, use_graph):
    ids, qf = _inputs(cfg, B)
    toks, scores, n = eng.generate(ids, qf, max_new=N_NEW, eos_id=-1, output_scores=True, use_graph=use_graph)
    assert n == N_NEW
    return toks.cpu().clone(), scores.cpu().contiguous().view(torch.int16).clone()


def _delta(n1, n0):
    return (n1[0] - n0[0], n1[1] - n0[1])


@pytest.mark.parametrize("B", [3, 12, 16])
def test_w4_rows_step_equals_the_bf16_step_on_the_dequantised_weights(pair, B):
    cfg, a, b = pair
    L = cfg.llama.layers
    assert b.w4_rows_stats() == (0, 0)
    for use_graph in (False, True):
        a.set_option("w4", 1)
        n0 = a.w4_rows_stats()
        t1, s1 = _generate(cfg, a, B, use_graph)
        n1 = a.w4_rows_stats()
        a.set_option("w4", 0)
        t0, s0 = _generate(cfg, a, B, use_graph)
        n2 = a.w4_rows_stats()
        a.set_option("w4", 1)
        t2, s2 = _generate(cfg, a, B, use_graph)
        n3 = a.w4_rows_stats()
        tb, sb = _generate(cfg, b, B, use_graph)
        steps = (N_NEW - 1) if not use_graph else 1          # a graph: captured once (the option dropped the old one)
        want = (steps * 2 * L, steps * L)
        assert _delta(n1, n0) == want, f"int4 launches with the option on (graph={use_graph})"
        assert n2 == n1, f"int4 launches with the option off (graph={use_graph})"
        assert _delta(n3, n2) == want, f"the option dropped the graph and switched back (graph={use_graph})"
        assert torch.equal(t1, tb) and torch.equal(s1, sb), f"int4 stream != bf16 engine on W' (graph={use_graph})"
        assert torch.equal(t0, tb) and torch.equal(s0, sb), f"packed W' copy != bf16 engine on W' (graph={use_graph})"
        assert torch.equal(t2, t1) and torch.equal(s2, s1), f"the option does not switch back (graph={use_graph})"
    assert b.w4_rows_stats() == (0, 0)


@pytest.mark.parametrize("B", [2, 17])
def test_other_families_do_not_move_the_counters(pair, B):
    cfg, a, b = pair
    n0 = a.w4_rows_stats()
    ta, sa = _generate(cfg, a, B, False)
    tb, sb = _generate(cfg, b, B, False)
    assert torch.equal(ta, tb) and torch.equal(sa, sb)
    assert a.w4_rows_stats() == n0 and b.w4_rows_stats() == (0, 0)


def test_small_config_has_no_3_to_16_row_family():
    cfg = small_cfg()
    a, b = _engines(cfg)
    try:
        ta, sa = _generate(cfg, a, 4, False)
        tb, sb = _generate(cfg, b, 4, False)
        assert torch.equal(ta, tb) and torch.equal(sa, sb)
        assert a.w4_rows_stats() == (0, 0) and b.w4_rows_stats() == (0, 0)
    finally:
        a.close()
        b.close()


def test_row_session_on_int4_weights(pair):
    """generate_queue with 4 rows and 6 short prompts: the tokens of generate per prompt (one batch of 6: the same family, and a row's bits do not
    depend on its neighbours), on the int4 kernels."""
    cfg, a, b = pair
    caps = [4, 7, 5, 9, 6, 8]
    ids = synth.synth_prompt_ids(6, T_PROMPT, vocab=cfg.llama.vocab, img_offset=6, pad_rows=False, seed=47)
    qf = synth.synth("t.w4rows.queue.qf", (6, 32, cfg.llama.qformer_dim), -1.0, 1.0)
    reqs = [(ids[i], qf[i], caps[i]) for i in range(6)]
    n0 = a.w4_rows_stats()
    out = a.generate_queue(reqs, rows=4, stage=2, eos_id=-1)
    n1 = a.w4_rows_stats()
    assert n1[0] > n0[0] and n1[1] > n0[1] and (n1[0] - n0[0]) == 2 * (n1[1] - n0[1])
    toks, _, _ = a.generate(ids, qf, max_new=max(caps), eos_id=-1)
    toks = toks.cpu()
    for i, cap in enumerate(caps):
        assert len(out[i]) == cap and torch.equal(out[i].cpu().long(), toks[i, :cap].long()), f"request {i}"
    outb = b.generate_queue(reqs, rows=4, stage=2, eos_id=-1)
    assert all(torch.equal(x.cpu(), y.cpu()) for x, y in zip(out, outb)) and b.w4_rows_stats() == (0, 0)
