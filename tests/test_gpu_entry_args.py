"""The batch-1/2 decode step after its kernels took their layer's pointers BY VALUE (csrc/chain.hip, csrc/gemm.hip): decode_chain_k no longer looks its
weights up in a device table, and skinny_gemm_k / decode_chain_k / attn_oproj16_k take what their first loads are addressed from as leading kernel
arguments (preloaded into SGPRs) and read the rest of their arguments late, from the kernarg segment (rdx_common.h late_kernarg).

What can go wrong with that is not arithmetic: it is a launch bound to the wrong layer or to the wrong role (down_proj of l with QKV of l, the last launch
reading a QKV weight that is not there), a struct read at the wrong offset of the argument list, or a captured graph that kept something a later step or
a later engine must not see. Three decoder layers at production width (4096 / 11008, 32 heads) are the smallest model with a first, a middle and a last
chained launch; prompt 24, 6 new tokens; batch 1 and 2; bf16, f16 and fp8 weights.

  * eager steps and graph replays from the same prompt give the same tokens and logits, bit for bit;
  * a second engine, created after the first is closed, gives the same bits (nothing of a launch's arguments outlives its engine);
  * tokens and logits are within the bar of tests/_parity.py of the oracle (the bars of test_gpu_parity.py's production-width test: accumulation-order noise
    per layer; fp8: the e4m3 grid's). Legs of 6 / 12 (row, step) pairs carry no percentage bar of their own: the identical-token share is asserted over
    the sum of the model-dtype legs, per dtype, by the last test of this module. A free-running comparison ends a row at its first accepted token flip,
    and on these random-init weights the ORACLE's margins go down to 0.09 (its own run, no GPU involved) against an e4m3 noise bar of 0.87: an fp8 row may
    not survive its first step, and the comparison of the W8 kernels would be empty. So every case is ALSO decoded teacher-forced (tests/_parity.py
    teacher_forced: the oracle's tokens are fed, every (row, step) pair is compared -- logits under the bar at every step, the engine's argmax the oracle's
    token unless the oracle's margin is within twice the measured error); that is the leg that holds the fp8 weights, by value, to their layer;
  * the engine's hand-off error word is 0: rdx_generate reads it after the last step and fails the call when it is set, so a generation that returns is
    that assertion."""
import pytest
import torch

from radialog_amd import synth
from radialog_amd.config import LlamaCfg, RaDialogCfg
from _parity import Cover, check_greedy, teacher_forced

pytestmark = pytest.mark.gpu

DT = {"f16": torch.float16, "bf16": torch.bfloat16}
LAYERS, T_PROMPT, N_NEW = 3, 24, 6
PROD_TOL = {"f16": 1e-2, "bf16": 8e-2}       # tests/test_gpu_parity.py: logits within 1e-2 in fp16 per layer^(1/2); bf16 has 8x the ulp
FP8_TOL = 0.5                                # ... and the e4m3 grid's noise with fp8 weights
MIN_COVER = {"f16": 0.9, "bf16": 0.75}
KINDS = [("bf16", False), ("f16", False), ("bf16", True)]
COVER = {"f16": Cover(), "bf16": Cover()}


@pytest.fixture(scope="module")
def model():
    """config, fp32 weights for the oracle, the two-row text prompt (row 1 left-padded by 5) and a cache of oracle runs per (dtype, fp8)."""
    cfg = RaDialogCfg(llama=LlamaCfg(layers=LAYERS, qformer_dim=192))
    W = synth.make_weights(synth.llama_specs(cfg.llama, lora=True))
    # a text-only prompt: 24 tokens cannot hold the 32 <IMG> positions, so they become ordinary ids and no image embedding is spliced in
    ids = synth.synth_prompt_ids(2, T_PROMPT, vocab=cfg.llama.vocab, img_offset=4, pad_rows=False, seed=41)
    ids = torch.where(ids == synth.IMG_TOKEN_ID, 100 + 37 * torch.arange(T_PROMPT).expand(2, -1), ids)
    ids[1] = torch.cat([torch.zeros(5, dtype=torch.long), ids[1, : T_PROMPT - 5]])
    qf = None
    refs = {}
    yield cfg, W, ids, qf, refs
    refs.clear()
    W.clear()


def _oracle(model, dtype, fp8):
    """ONE oracle run per weight kind, on both rows; batch 1 is its row 0 (rows are independent)."""
    from oracle import ref_cpu
    cfg, W, ids, qf, refs = model
    if (dtype, fp8) not in refs:
        with torch.no_grad():
            refs[(dtype, fp8)] = ref_cpu.LlamaOracle(W, cfg.llama, DT[dtype], lora=True, fp8=fp8).generate_greedy(ids, qf, max_new=N_NEW, eos_id=-1, pad_id=0)
    return refs[(dtype, fp8)]


def _rows(ref, B):
    return {"tokens": ref["tokens"][:B], "scores": [s[:B] for s in ref["scores"]], "margins": ref["margins"][:, :B]}


def _engine(cfg, dtype, fp8):
    from radialog_amd.engine import RdxEngine, synth_getter
    eng = RdxEngine(cfg, dtype=dtype, device=0, max_batch=2, max_len=128, lora=True, vision=False, weights_fp8=fp8)
    eng.load_weights(synth_getter(cfg, eng.device, lora=True), vision=False)
    return eng


def _run(eng, ids, qf):
    out = {}
    for use_graph in (False, True):
        toks, scores, n = eng.generate(ids, qf, max_new=N_NEW, eos_id=-1, pad_id=0, output_scores=True, use_graph=use_graph)      # raises when err != 0
        assert n == N_NEW
        out[use_graph] = (toks.cpu().clone(), scores.cpu().clone())
    assert eng.time_unit(7, 1) > 0.0             # the chained launch is what this engine runs (rdx_time 7 fails where it is not active)
    return out


def _same(a, b, what):
    assert torch.equal(a[0], b[0]), f"{what}: greedy tokens differ"
    assert torch.equal(a[1].view(torch.int16), b[1].view(torch.int16)), f"{what}: logits differ in {(a[1] != b[1]).sum().item()} places"


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("dtype,fp8", KINDS)
def test_three_layer_step_binds_every_launch_to_its_layer(model, dtype, fp8, B):
    cfg, _, ids2, qf2, _ = model
    ids, qf = ids2[:B], qf2
    eng = _engine(cfg, dtype, fp8)
    first = _run(eng, ids, qf)
    eng.close()
    _same(first[False], first[True], "eager steps vs graph replay")
    eng = _engine(cfg, dtype, fp8)
    second = _run(eng, ids, qf)
    tol = (FP8_TOL if fp8 else PROD_TOL[dtype]) * LAYERS ** 0.5
    ref = _rows(_oracle(model, dtype, fp8), B)
    tf = teacher_forced(eng, ref, ids, qf, N_NEW, tol, f"teacher-forced B={B} {dtype} fp8={fp8} layers={LAYERS}")       # all B x 6 pairs compared
    assert tf[1] == B * N_NEW
    eng.close()
    for g in (False, True):
        _same(first[g], second[g], f"second engine (graph {g})")
    toks, scores = first[True]
    leg = check_greedy(toks, scores, ref, tol, 0.0, f"B={B} {dtype} fp8={fp8} layers={LAYERS}")
    if not fp8:
        COVER[dtype].add(leg)
    print(f"entry args B={B} {dtype} fp8={fp8}: free-running compared {leg[0]}/{leg[1]}, |hip-oracle| {leg[2]:.4g}; teacher-forced {tf[0]}/{tf[1]} tokens "
          f"the oracle's, |hip-oracle| {tf[2]:.4g} (bar {tol:.4g})")


def test_token_identity_coverage_of_the_legs_above():
    for dtype, c in COVER.items():
        c.check(MIN_COVER[dtype], f"three-layer entry-argument legs, {dtype}")
