"""The data-tagged hand-off from attention to o_proj inside the fused batch <= 2 launch (csrc/handoff.h: WaitTagged; csrc/chain.hip:
attn_oproj16_k) and the in-situ timeline hook that measured the seam (rdx_gemv_trace 8, profiles/r08_attn_oproj_handoff.md).

The attention workgroups publish their output as 8-byte {two elements, tag} granules into ONE buffer shared by every layer and every step; nothing
is ever zeroed, so what keeps an o_proj workgroup from accepting an old row is the tag alone (step epoch * layers + layer + 1). The transport moves
the same elements into the same registers, so the bar everywhere is equality of bits: with a fresh engine (whose buffer holds no old row at all),
across eager steps and graph replays, batch sizes, prompts and restarts."""
import dataclasses

import pytest
import torch

from radialog_amd import _lib, synth
from radialog_amd.config import LlamaCfg, RaDialogCfg, small_cfg

pytestmark = pytest.mark.gpu

T_PROMPT, N_STEPS = 72, 12


def _cfg(which):
    if which == "small":
        return small_cfg()
    if which == "prod2":
        return RaDialogCfg(llama=LlamaCfg(layers=2, qformer_dim=192))
    # one decoder layer at the small widths: tag = epoch + 1, the case in which a tag counted per step of a prompt would repeat
    return dataclasses.replace(small_cfg(), llama=LlamaCfg(vocab=32001, hidden=512, inter=1408, layers=1, heads=4, qformer_dim=192))


def _engine(cfg, dtype, fp8=False):
    from radialog_amd.engine import RdxEngine, synth_getter
    eng = RdxEngine(cfg, dtype=dtype, device=0, max_batch=2, max_len=128, lora=True, vision=False, weights_fp8=fp8)
    eng.load_weights(synth_getter(cfg, eng.device, lora=True), vision=False)
    return eng


def _prompt(cfg, B, seed):
    ids = synth.synth_prompt_ids(B, T_PROMPT, vocab=cfg.llama.vocab, img_offset=6, pad_rows=False, seed=seed)
    if B > 1:                                  # left-pad row 1 by 5 (pad id 0), keep 32 <IMG> inside
        ids[1] = torch.cat([torch.zeros(5, dtype=torch.long), ids[1, : T_PROMPT - 5]])
    qf = synth.synth(f"t.qf{seed}", (B, 32, cfg.llama.qformer_dim), -1.0, 1.0)
    return ids, qf


def _gen(eng, cfg, B, seed, max_new, use_graph):
    ids, qf = _prompt(cfg, B, seed)
    toks, scores, n = eng.generate(ids, qf, max_new=max_new, eos_id=-1, output_scores=True, use_graph=use_graph)
    assert n == max_new
    return toks.cpu().clone(), scores.cpu().clone()


def _assert_same(got, want, what):
    assert torch.equal(got[0], want[0]), f"{what}: greedy tokens differ"
    assert torch.equal(got[1].view(torch.int16), want[1].view(torch.int16)), f"{what}: logits differ in {(got[1] != want[1]).sum().item()} places"


SEED_A, SEED_B = 33, 34
# (prompt, batch, max_new, use_graph): two batch sizes, two prompts, restarts after two tokens, eager steps and graph replays on ONE granule buffer
SEQUENCE = [(SEED_A, 2, N_STEPS, True), (SEED_B, 1, N_STEPS, False), (SEED_A, 1, 2, False), (SEED_A, 1, 2, True), (SEED_B, 2, N_STEPS, True)]


@pytest.mark.parametrize("which,dtype,fp8", [("small", "f16", False), ("small", "bf16", False), ("prod2", "f16", False), ("prod2", "bf16", False),
                                             ("small", "f16", True)])
def test_no_stale_row_is_ever_accepted(which, dtype, fp8):
    """Runs of different batch sizes, prompts and lengths follow one another on one engine; each must compute, bit for bit, what the same run
    computes on a fresh engine. A row of an earlier launch accepted as this launch's would change the logits."""
    cfg = _cfg(which)
    want = {}
    for seed, B, n, _ in SEQUENCE:
        if (seed, B, n) not in want:
            fresh = _engine(cfg, dtype, fp8)
            want[(seed, B, n)] = _gen(fresh, cfg, B, seed, n, True)
            fresh.close()
    eng = _engine(cfg, dtype, fp8)
    for i, (seed, B, n, graph) in enumerate(SEQUENCE):
        _assert_same(_gen(eng, cfg, B, seed, n, graph), want[(seed, B, n)], f"run {i} (prompt {seed}, batch {B}, {n} tokens, graph {graph})")
    eng.close()


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_one_layer_model_restarted_after_two_tokens(dtype):
    """One layer, max_new = 2, four times: every fused launch of the engine's life follows another fused launch of the SAME layer at the SAME step
    of a prompt; only the epoch tells them apart."""
    cfg = _cfg("one")
    fresh = _engine(cfg, dtype)
    want = _gen(fresh, cfg, 1, SEED_A, 2, True)
    fresh.close()
    eng = _engine(cfg, dtype)
    for i in range(4):
        _assert_same(_gen(eng, cfg, 1, SEED_A, 2, i % 2 == 1), want, f"restart {i}")
    eng.close()


def test_graph_replays_alone_then_a_fresh_generate():
    """The captured step graph replayed on its own (rdx_time 0), then eager steps (rdx_time 7), then a generate: the epoch moves with every step
    whoever launched it, no wait times out (a timeout makes the next call fail with -5) and the tokens are the first generate's."""
    cfg = small_cfg()
    eng = _engine(cfg, "bf16")
    ids, qf = _prompt(cfg, 1, SEED_A)
    first, _, _ = eng.generate(ids, qf, max_new=2 * N_STEPS, eos_id=-1, use_graph=True)
    assert eng.time_unit(0, 10) > 0.0
    assert eng.time_unit(7, 2) > 0.0
    again, _, _ = eng.generate(ids, qf, max_new=2 * N_STEPS, eos_id=-1, use_graph=True)
    assert torch.equal(first.cpu(), again.cpu())
    eng.close()


@pytest.mark.parametrize("B", [1, 2])
def test_teacher_forced_steps_compute_the_generated_logits(B):
    """The caller-driven path (rdx_decode_step_ids) runs the same step behind an embedding gather of its own: fed the tokens of a generate, it
    returns that generate's logits bit for bit, step by step."""
    cfg = small_cfg()
    eng = _engine(cfg, "bf16")
    ids, qf = _prompt(cfg, B, SEED_B)
    toks, scores, n = eng.generate(ids, qf, max_new=N_STEPS, eos_id=-1, output_scores=True, use_graph=True)
    toks, scores = toks.cpu().clone(), scores.cpu().clone()
    _, lg = eng.prefill(ids, qf, max_new=N_STEPS, eos_id=-1)
    assert torch.equal(lg.cpu().view(torch.int16), scores[0].view(torch.int16))
    for s in range(1, N_STEPS):
        _, lg = eng.decode_step(input_ids=toks[:, s - 1])
        assert torch.equal(lg.cpu().view(torch.int16), scores[s].view(torch.int16)), f"step {s}"
    eng.close()


@pytest.mark.parametrize("B,dtype,fp8", [(1, "bf16", False), (2, "f16", False), (1, "f16", True)])
def test_seam_timeline_is_causal_and_leaves_the_step_alone(B, dtype, fp8):
    """rdx_gemv_trace(8): one eager decode step with per-workgroup timestamps of one fused launch. Every workgroup stamps its stages in order; every
    o_proj workgroup sees its inputs ready only after EVERY attention workgroup has issued its output stores; tokens generated after traced steps
    are those generated before."""
    cfg = small_cfg()
    eng = _engine(cfg, dtype, fp8)
    ids, qf = _prompt(cfg, B, SEED_A)
    first, _, _ = eng.generate(ids, qf, max_new=N_STEPS, eos_id=-1, use_graph=True)
    n_attn = cfg.llama.heads * B
    n_o = (cfg.llama.hidden // 16 + 1) // 2
    for layer in (0, 1):
        eng.generate(ids, qf, max_new=8, eos_id=-1, use_graph=False)
        tr = eng.gemv_trace(_lib.TRACE_ATTN_OPROJ, layer)
        a, o = tr[:n_attn], tr[n_attn:n_attn + n_o]
        assert (tr[n_attn + n_o:] == 0).all() and (a[:, :7] > 0).all() and (o[:, 0] > 0).all()
        for rec, order in ((a, (0, 1, 2, 3, 4, 5, 6)), (o, (0, 5, 3, 6, 1, 7))):
            for x, y in zip(order, order[1:]):
                assert (rec[:, x] <= rec[:, y]).all(), f"layer {layer}: slot {x} after slot {y}"
        assert int(o[:, 3].min()) >= int(a[:, 5].max()), "an o_proj workgroup saw its inputs ready before the last attention output was stored"
    again, _, _ = eng.generate(ids, qf, max_new=N_STEPS, eos_id=-1, use_graph=True)
    assert torch.equal(first.cpu(), again.cpu())
    eng.close()


def test_seam_timeline_reports_a_step_without_the_fused_launch(monkeypatch):
    monkeypatch.setenv("RDX_FUSE_AO", "0")
    cfg = small_cfg()
    eng = _engine(cfg, "f16")
    ids, qf = _prompt(cfg, 1, SEED_A)
    eng.generate(ids, qf, max_new=8, eos_id=-1)
    with pytest.raises(_lib.RdxError, match="not active"):
        eng.gemv_trace(_lib.TRACE_ATTN_OPROJ, 0)
    eng.close()
