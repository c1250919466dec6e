"""The batch <= 2 decode step on coded bf16 weights (rdx_set_option "wcode", on by default: every gate/up, down_proj and QKV and the lm_head stream
their 13-bit coded copy; csrc/skinny_body.h, csrc/chain.hip) computes the bits it computes on the raw packed weights: tokens and every step's
logits are compared with the option switched between two generates of ONE engine, eager and as a replayed graph. Where no coded copy exists
(f16, fp8 weights) the option is inert. WHICH kernels ran is seen through the context's launch counters (rdx_wcode_stats: launches of
skinny_gemm_wc_k and of decode_chain_wc_k; a captured graph counts once, at capture): per eager step with the option on exactly layers + 1 coded
GEMVs (every gate/up, the lm_head; layer 0's stand-alone QKV stays raw) and `layers` coded chained launches, none with it off, none ever in an f16 or fp8 engine --
a dispatch that quietly fell back to the raw kernels would pass every bitwise comparison and fail these counts."""
import pytest
import torch

from radialog_amd import synth
from radialog_amd.config import LlamaCfg, RaDialogCfg, small_cfg

pytestmark = pytest.mark.gpu

T_PROMPT, N_NEW = 40, 12


def _cfg(which):
    return small_cfg() if which == "small" else RaDialogCfg(llama=LlamaCfg(layers=2, qformer_dim=192))


def _engine(which, B, dtype="bf16", fp8=False, plant=None):
    from radialog_amd.engine import RdxEngine, synth_getter
    cfg = _cfg(which)
    eng = RdxEngine(cfg, dtype=dtype, device=0, max_batch=B, max_len=128, lora=True, vision=False, weights_fp8=fp8)
    get = synth_getter(cfg, eng.device, lora=True)
    if plant:
        inner = get

        def get(name):
            t = inner(name)
            if any(name.endswith(s) for s in plant):
                t = t.clone()
                t[21, 77] = 1e-30          # 70 binades under its tile's largest weight: outside the window
            return t
    eng.load_weights(get, vision=False)
    return cfg, eng


def _generate(cfg, eng, B, use_graph):
    ids = synth.synth_prompt_ids(B, T_PROMPT, vocab=cfg.llama.vocab, img_offset=6, pad_rows=False, seed=41)
    if B > 1:
        ids[1] = torch.cat([torch.zeros(3, dtype=torch.long), ids[1, : T_PROMPT - 3]])
    qf = synth.synth("t.wcode.qf", (B, 32, cfg.llama.qformer_dim), -1.0, 1.0)
    toks, scores, n = eng.generate(ids, qf, max_new=N_NEW, eos_id=-1, output_scores=True, use_graph=use_graph)
    assert n == N_NEW
    return toks.cpu().clone(), scores.cpu().contiguous().view(torch.int16).clone()


def _launches(eng):
    return eng.wcode_stats()[3:]


def _on_equals_off(cfg, eng, B, coded=True):
    L = cfg.llama.layers
    for use_graph in (False, True):
        eng.set_option("wcode", 1)
        n0 = _launches(eng)
        t1, s1 = _generate(cfg, eng, B, use_graph)
        n1 = _launches(eng)
        eng.set_option("wcode", 0)
        t0, s0 = _generate(cfg, eng, B, use_graph)
        n2 = _launches(eng)
        eng.set_option("wcode", 1)
        t2, s2 = _generate(cfg, eng, B, use_graph)
        # the first token comes from the prefill; eager: N_NEW - 1 steps are launched, a graph: the step is captured once (the option dropped the old one)
        steps = (N_NEW - 1) if not use_graph else 1
        want = (steps * (L + 1), steps * L) if coded else (0, 0)
        assert (n1[0] - n0[0], n1[1] - n0[1]) == want, f"coded launches with the option on (graph={use_graph})"
        assert n2 == n1, f"coded launches with the option off (graph={use_graph})"
        assert torch.equal(t1, t0) and torch.equal(s1, s0), f"coded != raw (graph={use_graph})"
        assert torch.equal(t2, t1) and torch.equal(s2, s1), f"the option does not switch back (graph={use_graph})"


@pytest.mark.parametrize("which,B", [("small", 1), ("small", 2), ("prod2", 1), ("prod2", 2)])
def test_coded_step_equals_raw_step_bitwise(which, B):
    cfg, eng = _engine(which, B)
    try:
        tiles, fallback, nbytes = eng.wcode_stats()[:3]
        L = cfg.llama
        want = ((L.vocab + 15) // 16) + L.layers * (2 * L.inter // 16 + L.hidden // 16) + (L.layers - 1) * ((3 * L.hidden + 2 * L.lora_r + 15) // 16)
        print(f"{which} B={B}: {tiles} coded tiles, {fallback} fall back, {nbytes / 2**20:.1f} MiB of coded copies")
        assert tiles == want
        assert fallback <= tiles // 100          # expected 0 on the synthetic weights (uniform: 23 binades at most under a tile's top)
        _on_equals_off(cfg, eng, B)
        assert eng.time_unit(7, 1) > 0.0         # the chained family is the one that ran (rdx_time 7 fails where the step has no chained launch)
    finally:
        eng.close()


@pytest.mark.parametrize("B", [1, 2])
def test_fallback_tiles_inside_the_step(B):
    """An out-of-window weight in layer 1's down_proj and q_proj (the fused QKV weight: the fallback inside decode_chain_wc_k, in the down_proj role of
    layer 1's launch and in the QKV role of layer 0's) and in layer 1's gate_proj and the lm_head (skinny_gemm_wc_k): the four tiles are flagged and
    stream their raw bytes, next to coded ones."""
    cfg, eng = _engine("prod2", B, plant=("layers.1.mlp.down_proj.weight", "layers.1.self_attn.q_proj.weight", "layers.1.mlp.gate_proj.weight", "lm_head.weight"))
    try:
        assert eng.wcode_stats()[1] == 4
        _on_equals_off(cfg, eng, B)
    finally:
        eng.close()


@pytest.mark.parametrize("dtype,fp8", [("f16", False), ("bf16", True)])
def test_option_is_inert_without_a_coded_copy(dtype, fp8):
    cfg, eng = _engine("small", 1, dtype=dtype, fp8=fp8)
    try:
        assert eng.wcode_stats() == (0, 0, 0, 0, 0)
        _on_equals_off(cfg, eng, 1, coded=False)
        assert eng.wcode_stats() == (0, 0, 0, 0, 0)
    finally:
        eng.close()
