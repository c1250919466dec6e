"""The coded chained launch (decode_chain_wc_k, csrc/chain.hip) decodes the first coded chunks of a wave's ring ahead of its role's seam -- one chunk in
the QKV role (in front of the hand-off wait; wave 0, which polls, behind it), two in the down_proj role (under the flight of its activation loads) --
and takes the first trip of its K loop unconditionally. tests/test_gpu_wcode_step.py compares coded and raw steps on slices of 4 and 8 coded chunks per
QKV wave; this file makes the same comparison -- one engine, option "wcode" on / off / on, tokens and every step's logits torch.equal, eager and as a
replayed graph, batch 1 and 2, the launch counts of rdx_wcode_stats -- on the slice lengths at which the pre-decode and the unconditional first trip
take their other paths. The reference is the raw chained kernel (decode_chain_k), which the pre-decode does not touch.

    hidden  512 ( 4 heads): a QKV wave's slice is exactly the 1 pre-decoded chunk: ring slots 1..3 and all four refills are clamped duplicates of it, whose
                            fragments multiply the zero line;
    hidden 1536 (12 heads): 3 chunks, between the pre-decode and the ring depth RC = 4: two chunks behind the pre-decoded one, one duplicate;
    hidden 2560 (20 heads): 5 chunks, one past RC: the slot the pre-decode refilled holds the slice's last chunk, consumed by the tail.

`inter` = 1408, 2816, 4224 puts the down_proj slices off the coded-chunk grid (2.75, 5.5 and 8.25 packed chunks per wave = 1-2, 2-3 and 3-4 coded
chunks around the role's ring of 2, all of it pre-decoded: first and last coded chunks shared with the neighbours, guard and zero line in the pre-decoded
multiply and in the tail). A last case plants out-of-window weights in rows 5 and 21 of layer 1's q_proj and down_proj: tile 0 -- the tile the polling
wave belongs to -- and tile 1 stream their raw bytes and pre-decode nothing, next to coded tiles of the same QKV workgroup."""
import pytest
import torch

from radialog_amd import synth
from radialog_amd.config import LlamaCfg, RaDialogCfg

pytestmark = pytest.mark.gpu

T_PROMPT, N_NEW = 40, 8
WIDTHS = {"exactly_pre": (512, 4, 1408), "between_pre_and_ring": (1536, 12, 2816), "one_past_ring": (2560, 20, 4224)}


def _cfg(which):
    hidden, heads, inter = WIDTHS[which]
    return RaDialogCfg(llama=LlamaCfg(vocab=8001, hidden=hidden, inter=inter, layers=3, heads=heads, qformer_dim=192))


def _engine(which, B, plant=None):
    from radialog_amd.engine import RdxEngine, synth_getter
    cfg = _cfg(which)
    assert cfg.llama.head_dim == 128
    eng = RdxEngine(cfg, dtype="bf16", device=0, max_batch=B, max_len=128, lora=True, vision=False)
    get = synth_getter(cfg, eng.device, lora=True)
    if plant:
        inner = get

        def get(name):
            t = inner(name)
            if any(name.endswith(s) for s in plant):
                t = t.clone()
                t[5, 77] = 1e-30           # 70 binades under its tile's largest weight: outside the window (tile 0)
                t[21, 77] = 1e-30          # tile 1
            return t
    eng.load_weights(get, vision=False)
    return cfg, eng


def _generate(cfg, eng, B, use_graph):
    ids = synth.synth_prompt_ids(B, T_PROMPT, vocab=cfg.llama.vocab, img_offset=6, pad_rows=False, seed=43)
    if B > 1:
        ids[1] = torch.cat([torch.zeros(3, dtype=torch.long), ids[1, : T_PROMPT - 3]])
    qf = synth.synth("t.predecode.qf", (B, 32, cfg.llama.qformer_dim), -1.0, 1.0)
    toks, scores, n = eng.generate(ids, qf, max_new=N_NEW, eos_id=-1, output_scores=True, use_graph=use_graph)
    assert n == N_NEW
    return toks.cpu().clone(), scores.cpu().contiguous().view(torch.int16).clone()


def _on_equals_off(cfg, eng, B):
    L = cfg.llama.layers
    for use_graph in (False, True):
        eng.set_option("wcode", 1)
        n0 = eng.wcode_stats()[3:]
        t1, s1 = _generate(cfg, eng, B, use_graph)
        n1 = eng.wcode_stats()[3:]
        eng.set_option("wcode", 0)
        t0, s0 = _generate(cfg, eng, B, use_graph)
        n2 = eng.wcode_stats()[3:]
        eng.set_option("wcode", 1)
        t2, s2 = _generate(cfg, eng, B, use_graph)
        # eager: N_NEW - 1 steps are launched; a graph: the step is captured once. Per step L + 1 coded GEMVs (gate/up, lm_head) and L coded chained launches
        steps = (N_NEW - 1) if not use_graph else 1
        assert (n1[0] - n0[0], n1[1] - n0[1]) == (steps * (L + 1), steps * L), f"coded launches with the option on (graph={use_graph})"
        assert n2 == n1, f"coded launches with the option off (graph={use_graph})"
        assert torch.equal(t1, t0) and torch.equal(s1, s0), f"coded != raw (graph={use_graph})"
        assert torch.equal(t2, t1) and torch.equal(s2, s1), f"the option does not switch back (graph={use_graph})"


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("which", sorted(WIDTHS))
def test_coded_step_equals_raw_step_bitwise_on_short_and_wrapping_slices(which, B):
    cfg, eng = _engine(which, B)
    try:
        assert eng.wcode_stats()[0] > 0 and eng.wcode_stats()[1] == 0           # coded copies exist, no tile falls back on the synthetic weights
        _on_equals_off(cfg, eng, B)
        assert eng.time_unit(7, 1) > 0.0         # the chained family is the one that ran
    finally:
        eng.close()


@pytest.mark.parametrize("B", [1, 2])
def test_fallback_tiles_of_the_polling_wave(B):
    """Rows 5 and 21 of layer 1's q_proj (QKV role of layer 0's launch) and down_proj (down_proj role of layer 1's): tiles 0 and 1 of both weights are
    flagged -- four fallback tiles -- and stream their raw bytes; QKV workgroup 0 holds both next to two coded tiles."""
    cfg, eng = _engine("one_past_ring", B, plant=("layers.1.mlp.down_proj.weight", "layers.1.self_attn.q_proj.weight"))
    try:
        assert eng.wcode_stats()[1] == 4
        _on_equals_off(cfg, eng, B)
    finally:
        eng.close()
