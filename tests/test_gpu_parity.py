"""GPU parity tests proper: librdx (through its C ABI, via RdxEngine) against the CPU oracle on the same seeded
inputs, at sizes the oracle finishes in seconds. Bars:
  * decoder: same dtype on both sides, same rounding points -> logits within 1e-2 (fp16, the tolerance north_star
    states) / 6e-2 (bf16: one bf16 ulp at |logit|~4 is 3e-2), greedy token ids IDENTICAL wherever the oracle's
    top-1/top-2 margin exceeds 4x that tolerance.
  * encoder / Q-Former: the reference runs them in fp32; the HIP path computes in the model dtype with fp32
    accumulation -> relative L2 error <= 5e-3 (fp16) / 3e-2 (bf16).
"""
import numpy as np
import pytest
import torch

from radialog_amd import synth
from radialog_amd.config import small_cfg
from _parity import Cover, check_greedy, teacher_forced as _teacher_forced

pytestmark = pytest.mark.gpu

DT = {"f16": torch.float16, "bf16": torch.bfloat16}
LOGIT_TOL = {"f16": 1e-2, "bf16": 6e-2}
ENC_TOL = {"f16": 5e-3, "bf16": 3e-2}
# share of (row, step) pairs that must have been compared with IDENTICAL tokens (tests/_parity.py). fp16 is the reference's
# dtype (torch_dtype=float16, demo.py:225) and the parity dtype; bf16 (the bench dtype) rounds 8x coarser, so oracle near-ties
# within two ulps -- the only place a token may legitimately differ -- are 8x more frequent and end a row's comparison earlier.
MIN_COVER = {"f16": 0.9, "bf16": 0.75}
# Legs of fewer than 48 (row, step) pairs (production-width batch 1: 5 pairs) cannot carry a percentage bar on their own: ONE legitimate
# near-tie flip at an early step ends the row. Their logit tolerance and margin rule are asserted per leg; their identical-token counts
# are summed here per dtype and the bar is applied to the sum by test_small_leg_token_identity_coverage at the end of this module.
SMALL_LEGS = {"f16": Cover(), "bf16": Cover()}


def _cpu_weights(cfg, lora=True):
    specs = {}
    specs.update(synth.vision_specs(cfg.vision))
    specs.update(synth.qformer_specs(cfg.qformer))
    specs.update(synth.llama_specs(cfg.llama, lora=lora))
    return synth.make_weights(specs)


@pytest.fixture(scope="module")
def cfg():
    return small_cfg()


@pytest.fixture(scope="module")
def cpu_w(cfg):
    return _cpu_weights(cfg)


@pytest.fixture(scope="module", params=["f16", "bf16"])
def engine(request, cfg):
    from radialog_amd.engine import RdxEngine, synth_getter
    eng = RdxEngine(cfg, dtype=request.param, device=0, max_batch=4, max_len=256, lora=True)
    eng.load_weights(synth_getter(cfg, eng.device, lora=True))
    yield eng
    eng.close()


def _rel_l2(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def test_encode_image_matches_oracle(engine, cfg, cpu_w):
    from oracle import ref_cpu
    img = synth.synth_images(2, cfg.vision.img)
    with torch.no_grad():
        ref_q, ref_emb = ref_cpu.forward_image(img, cpu_w, cfg)
    q, emb = engine.encode_image(img.to(engine.device))
    tol = ENC_TOL[engine.dtype]
    assert q.shape == ref_q.shape and emb.shape == ref_emb.shape
    assert torch.isfinite(q).all() and torch.isfinite(emb).all()
    assert _rel_l2(emb.cpu(), ref_emb) < tol, "image_embeds (ResNet trunk + projector + scramble + ln_vision)"
    assert _rel_l2(q.cpu(), ref_q) < tol, "Q-Former last_hidden_state"


def test_two_image_mode_vit_pooler_matches_oracle(engine, cfg, cpu_w):
    """Optional BioViL-T two-image branch: both images through the trunk, ViT pooler difference features, full projector."""
    from oracle import ref_cpu
    img = synth.synth_images(2, cfg.vision.img)
    prev = synth.synth_images(2, cfg.vision.img, seed=77)
    with torch.no_grad():
        ref_q, ref_emb = ref_cpu.forward_image(img, cpu_w, cfg, previous=prev)
        single_q, _ = ref_cpu.forward_image(img, cpu_w, cfg)
    q, emb = engine.encode_image(img.to(engine.device), previous_image=prev.to(engine.device))
    tol = ENC_TOL[engine.dtype]
    assert _rel_l2(emb.cpu(), ref_emb) < tol and _rel_l2(q.cpu(), ref_q) < tol
    assert _rel_l2(q.cpu(), single_q) > 0.1                 # and it really is a different function of the inputs


def _prompt(cfg, B, T, seed):
    ids = synth.synth_prompt_ids(B, T, vocab=cfg.llama.vocab, img_offset=6, pad_rows=False, seed=seed)
    if B > 1:                                  # left-pad row 1 by 5 (pad id 0), keep 32 <IMG> inside
        ids[1] = torch.cat([torch.zeros(5, dtype=torch.long), ids[1, : T - 5]])
    if B > 2:                                  # row 2 has no <IMG>: the drop-32-tokens quirk
        ids[2][ids[2] == 32000] = 99
    return ids


def test_prefill_logits_and_kv_match_oracle(engine, cfg, cpu_w):
    from oracle import ref_cpu
    dt = DT[engine.dtype]
    B, T = 3, 72
    ids = _prompt(cfg, B, T, seed=21)
    qf = synth.synth("t.qf", (B, 32, cfg.llama.qformer_dim), -1.0, 1.0)
    orc = ref_cpu.LlamaOracle(cpu_w, cfg.llama, dt, lora=True)
    km = ids.ne(0).long()
    with torch.no_grad():
        logits, past, _ = orc.forward(orc.embed(ids, qf), km, ref_cpu.positions_from_mask(km))
    toks, lg = engine.prefill(ids, qf, max_new=4)
    k0 = engine.kv_read(0, 0, B)[:, :, :T].float().cpu()
    v1 = engine.kv_read(1, 1, B)[:, :, :T].float().cpu()
    rk, rv = past[0][0].float(), past[1][1].float()
    valid = km.bool()[:, None, :, None]        # pad-query rows of the reference are garbage that nothing reads
    tol = LOGIT_TOL[engine.dtype]
    assert float(((k0 - rk) * valid).abs().max()) < tol, "layer-0 K cache (QKV GEMM + RoPE)"
    assert float(((v1 - rv) * valid).abs().max()) < 4 * tol, "layer-1 V cache (whole layer 0 + LoRA on v)"
    ref_last = logits[:, -1].float()
    err = (lg.float().cpu() - ref_last).abs().max()
    assert float(err) < tol, f"last-position logits differ by {float(err)}"
    t0, am = toks[:, 0].cpu().long(), ref_last.argmax(-1)
    gaps = ref_last.topk(2).values.diff().abs()[:, 0]
    for b in range(B):
        assert int(t0[b]) == int(am[b]) or float(gaps[b]) <= 2 * float(err), f"row {b}: first token differs at margin {float(gaps[b])}"


def test_greedy_tokens_identical_to_oracle(engine, cfg, cpu_w):
    from oracle import ref_cpu
    dt = DT[engine.dtype]
    B, T, N = 3, 72, 12
    ids = _prompt(cfg, B, T, seed=33)
    qf = synth.synth("t.qf2", (B, 32, cfg.llama.qformer_dim), -1.0, 1.0)
    orc = ref_cpu.LlamaOracle(cpu_w, cfg.llama, dt, lora=True)
    with torch.no_grad():
        ref = orc.generate_greedy(ids, qf, max_new=N, eos_id=-1, pad_id=0)
    cover = Cover()
    for use_graph in (False, True):
        toks, scores, n = engine.generate(ids, qf, max_new=N, eos_id=-1, pad_id=0, output_scores=True, use_graph=use_graph)
        assert n == N
        cover.add(check_greedy(toks, scores, ref, LOGIT_TOL[engine.dtype], 0.0, f"{engine.dtype} graph={use_graph}"))
    cover.check(MIN_COVER[engine.dtype], f"{engine.dtype} eager + graph")


@pytest.mark.parametrize("T", [72, 200, 520])
def test_flash_prefill_attention_matches_oracle_and_the_16_query_kernel(cfg, cpu_w, monkeypatch, T):
    """csrc/flash.hip (64-query blocks, a wave owns 16 queries over their whole key range, V transposed through LDS once per
    workgroup) is what the batched prefill runs (>= 512 workgroups); RDX_FLASH_MIN=1 forces it onto these small prompts: left-padded
    row, a row without <IMG>, T = 72 (two ragged query blocks), T = 200 (four blocks, 7 key chunks, an odd last chunk), T = 520 (a multi-turn
    sized prompt, test.py:440-674: nine blocks, the causal chunk skip over up to eight whole chunks), and a
    multi-turn continuation (Tk > Tq: the causal offset). Prefill logits and the K / V cache against the oracle
    (modeling_llama_imgemb.py:187-250), greedy tokens through 8 steps, and against attention_k (RDX_FLASH_MIN=0) within one ulp-ish."""
    from oracle import ref_cpu
    from radialog_amd.engine import RdxEngine, synth_getter
    B, N = 3, 8
    ids = _prompt(cfg, B, T, seed=71)
    qf = synth.synth("t.qfflash", (B, 32, cfg.llama.qformer_dim), -1.0, 1.0)
    km = ids.ne(0).long()
    for dtype in ("f16", "bf16"):
        dt = DT[dtype]
        orc = ref_cpu.LlamaOracle(cpu_w, cfg.llama, dt, lora=True)
        with torch.no_grad():
            logits, past, _ = orc.forward(orc.embed(ids, qf), km, ref_cpu.positions_from_mask(km))
            ref = orc.generate_greedy(ids, qf, max_new=N, eos_id=-1, pad_id=0)
        eng = RdxEngine(cfg, dtype=dtype, device=0, max_batch=B, max_len=max(256, (T + 127) // 64 * 64), lora=True, vision=False)
        eng.load_weights(synth_getter(cfg, eng.device, lora=True), vision=False)
        out = {}
        for flash in (1, 0):
            eng.set_option("flash_min", flash)
            toks, lg = eng.prefill(ids, qf, max_new=4)
            out[flash] = (lg.float().cpu().clone(), eng.kv_read(cfg.llama.layers - 1, 1, B)[:, :, :T].float().cpu().clone())
        eng.set_option("flash_min", 1)
        tol = LOGIT_TOL[dtype]
        valid = km.bool()[:, None, :, None]
        err = float((out[1][0] - logits[:, -1].float()).abs().max())
        assert err < tol, f"{dtype} T={T}: flash prefill logits differ from the oracle by {err}"
        assert float(((out[1][1] - past[-1][1].float()) * valid).abs().max()) < 4 * tol, "last layer's V cache (every attention output feeds it)"
        ab = float((out[1][0] - out[0][0]).abs().max())
        assert ab < tol / 2, f"{dtype} T={T}: flash vs 16-query kernel logits differ by {ab}"
        toks, scores, n = eng.generate(ids, qf, max_new=N, eos_id=-1, pad_id=0, output_scores=True)
        SMALL_LEGS[dtype].add(check_greedy(toks, scores, ref, tol, 0.0, f"flash {dtype} T={T}"))
        # continuation turn: Tq = 17 new tokens behind the cached prompt + answer (causal offset Tk - Tq > 0)
        t1, _, _ = eng.generate(ids, qf, max_new=5, eos_id=-1, pad_id=0, reuse_prefix=True)
        follow = torch.randint(3, 31999, (B, 17), generator=torch.Generator().manual_seed(9))
        ids2 = torch.cat([ids, t1.cpu().long(), follow], dim=1)
        t2, s2, _ = eng.generate(ids2, qf, max_new=4, eos_id=-1, pad_id=0, output_scores=True, reuse_prefix=True)
        assert eng.last_kept_prefix == T + 4
        with torch.no_grad():
            ref2 = orc.generate_greedy(ids2, qf, max_new=4, eos_id=-1, pad_id=0)
        SMALL_LEGS[dtype].add(check_greedy(t2, s2, ref2, tol, 0.0, f"flash continuation {dtype} T={T}"))
        eng.close()


def test_eos_and_padding_rule(engine, cfg, cpu_w):
    """Finished rows emit pad; generation stops early once every row has produced EOS (HF 4.28.1 greedy_search)."""
    from oracle import ref_cpu
    dt = DT[engine.dtype]
    B, T, N = 2, 48, 24
    ids = _prompt(cfg, B, T, seed=5)
    qf = synth.synth("t.qf3", (B, 32, cfg.llama.qformer_dim), -1.0, 1.0)
    orc = ref_cpu.LlamaOracle(cpu_w, cfg.llama, dt, lora=True)
    with torch.no_grad():
        free = orc.generate_greedy(ids, qf, max_new=6, eos_id=-1, pad_id=0)
    eos = int(free["tokens"][0, 2])             # make the 3rd token of row 0 the EOS id
    with torch.no_grad():
        ref = orc.generate_greedy(ids, qf, max_new=N, eos_id=eos, pad_id=0)
    toks, _, n = engine.generate(ids, qf, max_new=N, eos_id=eos, pad_id=0)
    toks = toks.cpu().long()
    nref = ref["tokens"].shape[1]
    # the engine checks for "all finished" every 16 steps, so it may run past the reference; extra tokens are pad
    assert n >= nref
    # the subject here is the EOS / pad rule; the few pairs in front of the stop feed the per-dtype aggregate
    SMALL_LEGS[engine.dtype].add(check_greedy(toks, None, ref, LOGIT_TOL[engine.dtype], 0.0, f"{engine.dtype} eos"))
    if torch.equal(toks[0, :3], ref["tokens"][0, :3]):
        assert int(toks[0, 3:].abs().sum()) == 0      # row 0 finished at step 2 -> pads afterwards
    assert int(toks[:, nref:].abs().sum()) == 0       # everything behind the reference's stop is padding


@pytest.mark.parametrize("fused", [1, 0])
def test_fused_attention_oproj_launch_matches_oracle(cfg, cpu_w, monkeypatch, fused):
    """Batch <= 2: decode attention and o_proj in ONE launch of 16-wave workgroups with a fence-free hand-off (write-through stores,
    sharded arrival counter; csrc/chain.hip: attn_oproj16_k) -- the default -- against RDX_FUSE_AO=0, one kernel per unit. Both must
    be exactly as accurate."""
    from oracle import ref_cpu
    from radialog_amd.engine import RdxEngine, synth_getter
    monkeypatch.setenv("RDX_FUSE_AO", str(fused))
    eng = RdxEngine(cfg, dtype="f16", device=0, max_batch=4, max_len=256, lora=True, vision=False)
    eng.load_weights(synth_getter(cfg, eng.device, lora=True), vision=False)
    B, T, N = 2, 72, 24
    ids = _prompt(cfg, B, T, seed=33)
    qf = synth.synth("t.qf2", (B, 32, cfg.llama.qformer_dim), -1.0, 1.0)
    with torch.no_grad():
        ref = ref_cpu.LlamaOracle(cpu_w, cfg.llama, torch.float16, lora=True).generate_greedy(ids, qf, max_new=N, eos_id=-1)
    for use_graph in (False, True):
        toks, scores, n = eng.generate(ids, qf, max_new=N, eos_id=-1, use_graph=use_graph, output_scores=True)
        check_greedy(toks, scores, ref, LOGIT_TOL["f16"], MIN_COVER["f16"], f"fused attention+o_proj {fused} graph={use_graph}")
    eng.close()


@pytest.mark.parametrize("B,chain", [(1, 1), (2, 1), (1, 0), (2, 0)])
def test_chained_down_qkv_launch_matches_oracle(cfg, cpu_w, monkeypatch, B, chain):
    """Batch <= 2: down_proj(l) -> RMSNorm + QKV(l+1) as one chained launch per layer (csrc/chain.hip: decode_chain_k, fence-free
    hand-off; the default) against RDX_CHAIN=0, one kernel per unit; attention + o_proj in the fused 16-wave launch."""
    from oracle import ref_cpu
    from radialog_amd.engine import RdxEngine, synth_getter
    monkeypatch.setenv("RDX_CHAIN", str(chain))
    T, N = 72, 24
    ids = _prompt(cfg, B, T, seed=33)
    qf = synth.synth("t.qf2", (B, 32, cfg.llama.qformer_dim), -1.0, 1.0)
    for dtype in ("f16", "bf16"):
        eng = RdxEngine(cfg, dtype=dtype, device=0, max_batch=2, max_len=256, lora=True, vision=False)
        eng.load_weights(synth_getter(cfg, eng.device, lora=True), vision=False)
        with torch.no_grad():
            ref = ref_cpu.LlamaOracle(cpu_w, cfg.llama, DT[dtype], lora=True).generate_greedy(ids, qf, max_new=N, eos_id=-1)
        tol = LOGIT_TOL[dtype]
        cover = Cover()
        for use_graph in (False, True):
            toks, scores, n = eng.generate(ids, qf, max_new=N, eos_id=-1, output_scores=True, use_graph=use_graph)
            cover.add(check_greedy(toks, scores, ref, tol, 0.0, f"{dtype} chain={chain} graph={use_graph}"))
        cover.check(MIN_COVER[dtype], f"{dtype} chain={chain}")
        eng.close()


def test_step_graph_replays_after_generate_keep_the_handoff_sound(engine, cfg):
    """Regression: encode -> generate twice, then replay the captured step graph on its own (rdx_time) and generate
    again. The fused attention + o_proj launch waits on arrival counters; they are cleared by the last kernel of every
    step, so no replay may time out (a timeout makes the next rdx_generate fail with -5)."""
    B, T, N = 1, 72, 16
    ids = _prompt(cfg, B, T, seed=33)
    img = synth.synth_images(B, cfg.vision.img).to(engine.device)
    first = None
    for _ in range(2):
        q, _ = engine.encode_image(img, want_image_embeds=False)
        toks, _, n = engine.generate(ids, q, max_new=N, eos_id=-1, use_graph=True)
        first = toks.clone() if first is None else first
        assert torch.equal(first, toks)
    ms = engine.time_unit(0, 10)
    assert ms < 50.0, f"step graph replay took {ms} ms: a hand-off wait timed out"
    toks, _, n = engine.generate(ids, q, max_new=N, eos_id=-1, use_graph=True)
    assert torch.equal(first, toks)


@pytest.mark.parametrize("kperm", [1, 0])
def test_batch18_greedy_tokens_match_oracle(cfg, cpu_w, kperm, monkeypatch):
    """16 < batch <= 32 at widths the activation-stationary kernels do not cover (they are built for K = 4096): the generic two-row-tile
    GEMV family for every decode projection and the lm_head, and the 4-wave throughput attention; tokens and logits must match the
    oracle row by row."""
    from oracle import ref_cpu
    from radialog_amd.engine import RdxEngine, synth_getter
    # K cache layout (read at rdx_create): 16-position fragment order (small contexts) / row-major (what batch * heads > 256 gets)
    monkeypatch.setenv("RDX_KPERM", str(kperm))
    B, T, N = 18, 96, 8
    ids = synth.synth_prompt_ids(B, T, vocab=cfg.llama.vocab, img_offset=6, pad_rows=True, seed=3)
    qf = synth.synth("t.qf18", (B, 32, cfg.llama.qformer_dim), -1.0, 1.0)
    for dtype in ("f16", "bf16"):
        eng = RdxEngine(cfg, dtype=dtype, device=0, max_batch=B, max_len=128, lora=True, vision=False)
        eng.load_weights(synth_getter(cfg, eng.device, lora=True), vision=False)
        with torch.no_grad():
            ref = ref_cpu.LlamaOracle(cpu_w, cfg.llama, DT[dtype], lora=True).generate_greedy(ids, qf, max_new=N, eos_id=-1, pad_id=0)
        toks, scores, n = eng.generate(ids, qf, max_new=N, eos_id=-1, pad_id=0, output_scores=True, use_graph=True)
        tol = LOGIT_TOL[dtype]
        check_greedy(toks, scores, ref, tol, MIN_COVER[dtype], f"{dtype}")
        eng.close()


_PROD_W = {}


def _production_width_weights(layers):
    from radialog_amd.config import LlamaCfg, RaDialogCfg
    if layers not in _PROD_W:
        cfg = RaDialogCfg(llama=LlamaCfg(layers=layers, qformer_dim=192))     # 2 layers: the down_proj -> next layer's QKV seam as well
        _PROD_W.clear()                                                        # one set (1.9-2.7 GB of fp32) at a time
        _PROD_W[layers] = (cfg, synth.make_weights(synth.llama_specs(cfg.llama, lora=True)))
    return _PROD_W[layers]


PROD_TOL = {"f16": 1e-2, "bf16": 8e-2}      # north_star: logits within 1e-2 in fp16; bf16 has 8x the ulp
# fp8 x fp8 path (BASELINE configs[4]; the oracle is this repo's own fake-quantised restatement, the reference has no fp8 mode): the e4m3
# quantiser is discontinuous -- an activation that differs by one model-dtype ulp between the two sides (accumulation order) can land on
# the next e4m3 code, 2^-3 of its magnitude away, whatever the model dtype -- so the logit noise is set by the e4m3 grid, not by fp16 / bf16:
# measured 0.17-0.26 per step at production width (one layer), 0.45 over 48 x 32 x 32 001 logits, 0.21-0.24 on the small config in fp16.
# A wrong scale, group boundary or layout shows up as O(1-10); the token margin rule applies unchanged.
FP8_TOL = 0.5


def _prefix_err(scores, ref_scores, tok_a, tok_b, N):
    """max |a - b| over the steps whose inputs are still the same on both sides (tokens equal so far), per row."""
    worst = 0.0
    B = tok_a.shape[0]
    for b in range(B):
        for s in range(N):
            worst = max(worst, float((scores[s][b].float().cpu() - ref_scores[s][b].float()).abs().max()))
            if int(tok_a[b, s]) != int(tok_b[b, s]):
                break
    return worst


@pytest.mark.parametrize("B,fp8,layers,dtypes", [
    (32, False, 1, ("f16", "bf16")), (32, True, 1, ("bf16",)), (32, False, 2, ("f16",)),        # BASELINE configs[2] / [4] per-GPU batch
    (20, False, 1, ("bf16",)), (20, True, 1, ("bf16",)), (8, False, 1, ("bf16",)), (16, True, 1, ("bf16",)),
    (5, False, 1, ("bf16",)), (3, False, 1, ("f16",)), (4, True, 1, ("bf16",)), (1, False, 1, ("f16", "bf16")),
    (2, False, 1, ("f16",)), (1, True, 1, ("bf16",)), (20, False, 2, ("bf16",)), (1, False, 2, ("f16",)),
    (12, False, 1, ("f16", "bf16")), (16, False, 2, ("f16",)),       # round 5: the reference's eval batch (test.py:279,:344) and a full row tile on xs16.hip
    (64, False, 1, ("bf16",)), (40, False, 2, ("bf16",)),       # round 5: 33-128 rows, the row-block family (ragged last block at 40),
    (88, False, 1, ("bf16",)), (128, False, 1, ("f16",)),                                       # three (one workgroup slot in four idle) and four row blocks per tile walker
    (40, True, 1, ("bf16",)), (96, True, 1, ("bf16",)), (128, True, 1, ("bf16",))])               # ... and its fp8 x fp8 form (the 32-row fp8 kernels per row block)
def test_production_width_layers_match_oracle(B, fp8, layers, dtypes):
    """Every decode kernel family at the production widths (hidden 4096, inter 11008, vocab 32001; one or two decoder layers so
    that the oracle finishes in seconds; two layers add the down_proj -> next QKV seam): batch 1-2 fused / chained GEMV launches,
    batch 3-32 activation-stationary (xstat32.hip) and K-split (xsplit32_k) kernels with fragment-packed hand-offs, batch 32 with
    the row-major K cache and the full 32-row block, hipGraph replay. Per-step logits within the north_star tolerance of the oracle,
    tokens identical (tests/_parity.py), and -- accumulation-order noise being what separates any two fp16 implementations -- the
    HIP logits must be no further from the exactly-accumulated (fp64) evaluation of the same rounding points than the torch-CPU
    oracle is, up to a factor 2 (round 3: tightened from 3; measured ratios 0.7 ... 1.45. Cause: the MFMA pipeline's fp32 accumulation leaves ~1 % of the bf16-rounded K / V elements one ulp
off the exact value where torch's CPU FMA chain leaves 0.03 %, tests/diag/mfma_round.py; the worst of 5 million logits then sits
2-3 ulps out instead of 1). fp8 = BASELINE configs[4]: e4m3 weights everywhere, e4m3 activations on the fp8 MFMAs (f8f6f4 shapes in the prefill, 16x16x32_fp8 in the decode) in the
prefill (gemm8.hip) and from batch 3 in decode (xstat32.hip); the oracle runs the reference math on the same fake-quantised operands
(LlamaOracle(fp8=True))."""
    from oracle import ref_cpu
    from radialog_amd.engine import RdxEngine, synth_getter
    cfg, cpu_w = _production_width_weights(layers)
    T, N = 96, 5
    ids = synth.synth_prompt_ids(B, T, vocab=cfg.llama.vocab, img_offset=6, pad_rows=(B > 1), seed=5)
    qf = synth.synth("t.qf20", (B, 32, cfg.llama.qformer_dim), -1.0, 1.0)
    for dtype in dtypes:
        eng = RdxEngine(cfg, dtype=dtype, device=0, max_batch=B, max_len=128, lora=True, vision=False, weights_fp8=fp8)
        eng.load_weights(synth_getter(cfg, eng.device, lora=True), vision=False)
        with torch.no_grad():
            ref = ref_cpu.LlamaOracle(cpu_w, cfg.llama, DT[dtype], lora=True, fp8=fp8).generate_greedy(ids, qf, max_new=N, eos_id=-1, pad_id=0)
            # the exactly-accumulated evaluation costs as much again: on the legs that span the kernel families (batch 1, 20, 32)
            with_exact = (not fp8) and layers == 1 and B in (1, 12, 20, 32)
            # (round 6: the fp64 arbiter runs on this GPU -- oracle/ref_cpu.py LlamaOracle(device=...): fp64 contractions are order-independent wherever they run)
            truth = (ref_cpu.LlamaOracle(cpu_w, cfg.llama, DT[dtype], lora=True, exact=True, device=eng.device).generate_greedy(ids, qf, max_new=N, eos_id=-1, pad_id=0)
                     if with_exact else None)
        toks, scores, n = eng.generate(ids, qf, max_new=N, eos_id=-1, pad_id=0, output_scores=True, use_graph=True)
        tol = PROD_TOL[dtype] * layers ** 0.5        # accumulation-order noise adds up layer by layer (two layers: 1.4e-2 in fp16)
        if fp8:     # e4m3 activations (prefill; decode from batch 3): the noise is the e4m3 grid's (FP8_TOL above)
            tol = FP8_TOL * layers ** 0.5           # (per layer, like the model-dtype noise: bench.py's full-depth bar is FP8_TOL sqrt(32))
        leg = check_greedy(toks, scores, ref, tol, MIN_COVER[dtype] if B * N >= 48 else 0.0, f"B={B} {dtype} fp8={fp8} layers={layers}")
        if B * N < 48:
            SMALL_LEGS[dtype].add(leg)
        cmp_, tot, e_ho = leg
        tk = toks.cpu().long()
        if truth is None:
            print(f"production width B={B} {dtype} fp8={fp8} layers={layers}: compared {cmp_}/{tot}, |hip-oracle| {e_ho:.4g}")
            eng.close()
            continue
        e_ht = _prefix_err(scores, truth["scores"], tk, truth["tokens"], N)
        e_ot = _prefix_err(ref["scores"], truth["scores"], ref["tokens"], truth["tokens"], N)
        print(f"production width B={B} {dtype} fp8={fp8} layers={layers}: compared {cmp_}/{tot}, |hip-oracle| {e_ho:.4g}, "
              f"|hip-exact| {e_ht:.4g}, |oracle-exact| {e_ot:.4g}")
        if not fp8:
            ulp = 2.0 ** -8 if dtype == "f16" else 2.0 ** -5                 # one ulp at |logit| in [4, 8)
            assert e_ht <= 2.0 * e_ot + ulp, f"{dtype}: HIP is {e_ht:.4g} from the exact evaluation, the torch-CPU oracle only {e_ot:.4g}"
        eng.close()


@pytest.mark.parametrize("B", [4, 12])
def test_batch_3_16_decode_families_agree_and_match_oracle(B):
    """Round 5: batch 3-16 decodes on the one-row-tile family (xs16.hip: RMSNorm as the prologue of QKV / gate-up / lm_head, un-split o_proj /
    down_proj with the residual epilogue: 5 launches per layer); `rdx_set_option("xs16", 0)` puts the same engine back on the 32-row family of
    rounds 1-4 (xstat32_k / xsplit32_k + stand-alone rmsnorm4096_k: 7 launches). Both against the oracle at production width, two layers (the
    down_proj -> next layer's norm-prologue seam), teacher-forced over 24 steps, hipGraph and eager; and against each other."""
    from oracle import ref_cpu
    from radialog_amd.engine import RdxEngine, synth_getter
    cfg, cpu_w = _production_width_weights(2)
    T, N = 160, 24
    ids = synth.synth_prompt_ids(B, T, vocab=cfg.llama.vocab, pad_rows=True, seed=23)
    qf = synth.synth("t.qf_xs16", (B, 32, cfg.llama.qformer_dim), -1.0, 1.0)
    for dtype in ("f16", "bf16"):
        with torch.no_grad():
            ref = ref_cpu.LlamaOracle(cpu_w, cfg.llama, DT[dtype], lora=True).generate_greedy(ids, qf, max_new=N, eos_id=-1, pad_id=0)
        eng = RdxEngine(cfg, dtype=dtype, device=0, max_batch=B, max_len=224, lora=True, vision=False)
        eng.load_weights(synth_getter(cfg, eng.device, lora=True), vision=False)
        logit_rows = {}
        for fam in (1, 0):
            eng.set_option("xs16", fam)
            same, total, worst = _teacher_forced(eng, ref, ids, qf, N, PROD_TOL[dtype] * 2 ** 0.5, f"B={B} {dtype} xs16={fam}")
            assert same >= MIN_COVER[dtype] * total, f"B={B} {dtype} xs16={fam}: only {same}/{total} steps chose the oracle's token"
            toks, scores, n = eng.generate(ids, qf, max_new=6, eos_id=-1, pad_id=0, output_scores=True, use_graph=True)      # the captured step graph
            logit_rows[fam] = scores[:n].float().cpu()
            print(f"batch {B} {dtype} xs16={fam}: teacher-forced {same}/{total} identical, worst logit error {worst:.4g}")
        # the two families differ in fp32 accumulation order only
        d = float((logit_rows[1] - logit_rows[0]).abs().max())
        assert d <= 2 * PROD_TOL[dtype] * 2 ** 0.5, f"B={B} {dtype}: the two decode families are {d:.4g} apart"
        eng.close()


def test_fp8_row_blocks_equal_the_32_row_kernels_row_by_row():
    """fp8 weights at 33-128 rows run the 32-row fp8 kernels once per 32-row block (xstat32_k<.., A8, BLK> fp8 x fp8 behind rmsnorm4096_k into e4m3 blocks (ACT_BLK64_E4M3); the K-split
    o_proj / down_proj xsplit32_k<.., BLK> W8A16, the only form since the fp8 x fp8 K-split leg was removed): a row's arithmetic -- its own e4m3 scales, the K groups of o_proj /
    down_proj, every accumulation order -- is what the 32-row family computes for that row.
    So 40 rows in one pass (a full block + a ragged one) must reproduce, BIT FOR BIT, the tokens and logits of rows 0-31 and of rows 8-39 run as two
    32-row calls on the same engine (production width, two layers, hipGraph step; 32 rows each so that both sides take the same decode-attention
    variant -- below 9 rows the 16-wave latency form sums P.V in another order)."""
    from radialog_amd.engine import RdxEngine, synth_getter
    cfg, _ = _production_width_weights(2)
    B, T, N = 40, 96, 6
    ids = synth.synth_prompt_ids(B, T, vocab=cfg.llama.vocab, img_offset=6, pad_rows=True, seed=31)
    qf = synth.synth("t.qf8blk", (B, 32, cfg.llama.qformer_dim), -1.0, 1.0)
    eng = RdxEngine(cfg, dtype="bf16", device=0, max_batch=B, max_len=128, lora=True, vision=False, weights_fp8=True)
    eng.load_weights(synth_getter(cfg, eng.device, lora=True), vision=False)
    toks, scores, n = eng.generate(ids, qf, max_new=N, eos_id=-1, pad_id=0, output_scores=True, use_graph=True)
    toks, scores = toks.cpu(), scores[:n].float().cpu()
    assert not torch.isnan(scores).any()
    for lo, hi in ((0, 32), (8, 40)):
        t2, s2, n2 = eng.generate(ids[lo:hi], qf[lo:hi], max_new=N, eos_id=-1, pad_id=0, output_scores=True, use_graph=True)
        assert n2 == n and torch.equal(t2.cpu(), toks[lo:hi]), f"rows {lo}..{hi - 1}: tokens differ between the row-block pass and the 32-row family"
        d = float((s2[:n2].float().cpu() - scores[:, lo:hi]).abs().max())
        assert d == 0.0, f"rows {lo}..{hi - 1}: logits differ by {d} between the row-block pass and the 32-row family"
    eng.close()


def test_unplanted_lm_head_teacher_forced_margin_rule(cfg, cpu_w):
    """The identity legs above run on synth.py's planted lm_head (64 decisive rows, so that identical tokens can be DEMANDED). This leg
    uses an ordinary random-init head -- every row std 0.02 like transformers' `_init_weights` (modeling_llama_imgemb.py:349-358), top-2
    gaps of a few 1e-2 -- so that the claim is not tied to the planted margin distribution: teacher-forced through 24 steps, every
    step's logits within the tolerance, and every step whose oracle margin exceeds twice the measured error must pick the oracle's
    token. How many steps that decides is printed, not demanded."""
    from oracle import ref_cpu
    from radialog_amd.engine import RdxEngine, synth_getter
    H = cfg.llama.hidden
    plain = synth.synth("t.plain_lm_head", (cfg.llama.vocab, H), -0.02 * 3 ** 0.5, 0.02 * 3 ** 0.5)
    W = dict(cpu_w)
    W["lm_head.weight"] = plain
    B, T, N = 3, 72, 24
    ids = _prompt(cfg, B, T, seed=61)
    qf = synth.synth("t.qfplain", (B, 32, cfg.llama.qformer_dim), -1.0, 1.0)
    for dtype in ("f16", "bf16"):
        eng = RdxEngine(cfg, dtype=dtype, device=0, max_batch=B, max_len=128, lora=True, vision=False)
        base = synth_getter(cfg, eng.device, lora=True)
        eng.load_weights(lambda name: plain.to(eng.device) if name == "lm_head.weight" else base(name), vision=False)
        with torch.no_grad():
            ref = ref_cpu.LlamaOracle(W, cfg.llama, DT[dtype], lora=True).generate_greedy(ids, qf, max_new=N, eos_id=-1, pad_id=0)
        same, total, worst = _teacher_forced(eng, ref, ids, qf, N, LOGIT_TOL[dtype], f"plain head {dtype}")
        decided = int((ref["margins"] > 2 * worst).sum())
        print(f"unplanted lm_head {dtype}: {same}/{total} argmax tokens identical, {decided}/{total} steps have a margin above 2 x the worst "
              f"logit error {worst:.4g} (median oracle margin {float(ref['margins'].median()):.4g})")
        assert same >= decided                       # every decided step was identical (the helper asserted it step by step)
        eng.close()


@pytest.mark.parametrize("B,N,dtypes,fp8,layers", [(1, 256, ("f16", "bf16"), False, 1), (32, 64, ("f16", "bf16"), False, 1), (4, 64, ("bf16",), False, 1),
                                                   (64, 32, ("f16",), False, 1), (32, 48, ("bf16",), True, 1), (1, 64, ("bf16",), True, 1),
                                                   (40, 12, ("bf16",), True, 2)])      # fp8 x fp8 row blocks: ragged second block, the K-split slabs across the layer seam
def test_production_width_decode_over_the_bench_positions_teacher_forced(B, N, dtypes, fp8, layers):
    """The positions bench.py decodes through -- 160 -> 416 at batch 1 (256 steps), 160 -> 224 at batch 32 and 4 -- at production
    width (hidden 4096, inter 11008, vocab 32001; one layer so that the oracle finishes in seconds), every step compared
    (teacher forcing through rdx_decode_step_ids; modeling_llama_imgemb.py:187-250,:705-793): decode attention's register window and
    tail loops, the RoPE rows and the KV appends at every one of those positions, the batch-1 chained launches / batch 3-32
    activation-stationary kernels in eager mode. fp8 = the configs[4] weight path (e4m3 weights; fp8 x fp8 prefill and batch-32 decode)
    against LlamaOracle(fp8=True)."""
    from oracle import ref_cpu
    from radialog_amd.engine import RdxEngine, synth_getter
    cfg, cpu_w = _production_width_weights(layers)
    T = 160
    ids = synth.synth_prompt_ids(B, T, vocab=cfg.llama.vocab, pad_rows=(B > 1), seed=7)
    qf = synth.synth("t.qftf", (B, 32, cfg.llama.qformer_dim), -1.0, 1.0)
    for dtype in dtypes:
        with torch.no_grad():
            ref = ref_cpu.LlamaOracle(cpu_w, cfg.llama, DT[dtype], lora=True, fp8=fp8).generate_greedy(ids, qf, max_new=N, eos_id=-1, pad_id=0)
        eng = RdxEngine(cfg, dtype=dtype, device=0, max_batch=B, max_len=(T + N + 31) // 32 * 32, lora=True, vision=False, weights_fp8=fp8)
        eng.load_weights(synth_getter(cfg, eng.device, lora=True), vision=False)
        same, total, worst = _teacher_forced(eng, ref, ids, qf, N, (FP8_TOL if fp8 else PROD_TOL[dtype]) * layers ** 0.5, f"B={B} {dtype} fp8={fp8}")
        eng.close()
        print(f"teacher-forced production width B={B} {dtype} fp8={fp8} layers={layers}: {same}/{total} argmax tokens identical over positions {T}..{T + N - 1}, "
              f"worst logit error {worst:.4g}")
        assert same >= MIN_COVER[dtype] * total, f"B={B} {dtype}: only {same}/{total} steps chose the oracle's token"


@pytest.mark.parametrize("B,tp", [(1, 0), (3, 0), (3, 1), (3, 2)])
def test_long_context_decode_streams_past_the_register_window(cfg, cpu_w, B, tp, monkeypatch):
    """Multi-turn prompts (test.py:440-674: report + follow-up question, 400-700 tokens) put the context beyond the 480
    positions decode attention holds in registers; the rest streams through the MFMA / dot2 tail loops. T = 600 here.
    tp = 1 forces the 4-wave throughput variant that batch-32 decode uses (128-position window), tp = 2 the 8-wave variant of 9-16 rows (336)."""
    from oracle import ref_cpu
    if tp:
        monkeypatch.setenv("RDX_ATT_TP", str(tp))
    from radialog_amd.engine import RdxEngine, synth_getter
    T, N = 600, 6
    ids = synth.synth_prompt_ids(B, T, vocab=cfg.llama.vocab, img_offset=6, pad_rows=False, seed=11)
    qf = synth.synth("t.qfL", (B, 32, cfg.llama.qformer_dim), -1.0, 1.0)
    for dtype in ("f16", "bf16"):
        eng = RdxEngine(cfg, dtype=dtype, device=0, max_batch=B, max_len=640, lora=True, vision=False)
        eng.load_weights(synth_getter(cfg, eng.device, lora=True), vision=False)
        with torch.no_grad():
            ref = ref_cpu.LlamaOracle(cpu_w, cfg.llama, DT[dtype], lora=True).generate_greedy(ids, qf, max_new=N, eos_id=-1, pad_id=0)
        toks, scores, n = eng.generate(ids, qf, max_new=N, eos_id=-1, pad_id=0, output_scores=True, use_graph=True)
        tol = LOGIT_TOL[dtype]
        SMALL_LEGS[dtype].add(check_greedy(toks, scores, ref, tol, 0.0, f"{dtype} T={T} B={B}"))
        eng.close()


@pytest.mark.parametrize("tp,lens", [(1, (47, 48, 49, 64, 65, 96, 97, 112, 113, 128, 129)),
                                     (0, (60, 61, 120, 121, 240, 241, 300, 301, 420, 421, 480, 481)),
                                     (2, (47, 56, 57, 84, 85, 112, 113, 223, 224, 225, 335, 336, 337, 400))])      # 8 waves: 7 cache waves x 3 groups x 16 (lower part 224), V rows 28 apart
def test_decode_attention_context_lengths_around_the_register_window_edges(cfg, cpu_w, tp, lens, monkeypatch):
    """Context lengths on either side of every boundary of the register window: the halves (loaded unconditionally / once
    `slot` is known), the V row pairs P.V consumes together (16 positions apart in the 4-wave variant, 60 in the 16-wave
    one -- an unloaded odd row of a pair once produced NaN x 0), the window end where the tail loops take over. Three
    decode steps from each prompt length, all three attention variants, logits and tokens against the oracle."""
    from oracle import ref_cpu
    if tp:
        monkeypatch.setenv("RDX_ATT_TP", str(tp))
    from radialog_amd.engine import RdxEngine, synth_getter
    B, N = 2, 4
    for dtype in ("f16", "bf16"):
        eng = RdxEngine(cfg, dtype=dtype, device=0, max_batch=B, max_len=512, lora=True, vision=False)
        eng.load_weights(synth_getter(cfg, eng.device, lora=True), vision=False)
        oracle = ref_cpu.LlamaOracle(cpu_w, cfg.llama, DT[dtype], lora=True)
        tol = LOGIT_TOL[dtype]
        cover = Cover()
        for T in lens:
            ids = _prompt(cfg, B, T, seed=100 + T)
            qf = synth.synth(f"t.qfw{T}", (B, 32, cfg.llama.qformer_dim), -1.0, 1.0)
            with torch.no_grad():
                ref = oracle.generate_greedy(ids, qf, max_new=N, eos_id=-1, pad_id=0)
            toks, scores, n = eng.generate(ids, qf, max_new=N, eos_id=-1, pad_id=0, output_scores=True, use_graph=False)
            assert not torch.isnan(scores.float()).any(), f"{dtype} T={T}: NaN logits"
            cover.add(check_greedy(toks, scores, ref, tol, 0.0, f"{dtype} T={T}"))      # 8 pairs per length: the bar is on the sweep
        cover.check(MIN_COVER[dtype], f"{dtype} context-length sweep")
        eng.close()


@pytest.mark.parametrize("B", [1, 2])
def test_multi_turn_prefix_kv_reuse_matches_full_recompute_and_oracle(cfg, cpu_w, B):
    """Multi-turn re-prompting (test.py:440-674, demo.py:277-305): turn 2's prompt = turn 1's prompt + its answer + a
    follow-up question. With reuse_prefix the engine keeps the KV rows of the shared token prefix (rdx_generate_append) and
    prefills only the rest; tokens and logits must be those of the full prompt (oracle on the whole sequence), and the kept
    length must be everything the cache held (prompt + consumed answer tokens)."""
    from oracle import ref_cpu
    from radialog_amd.engine import RdxEngine, synth_getter
    T1, N1, TQ, N2 = 72, 9, 21, 8
    ids1 = _prompt(cfg, B, T1, seed=41)
    if B > 1:
        ids1[1] = _prompt(cfg, 2, T1, seed=43)[1]            # row 1 left-padded (pads sit inside the shared prefix)
    qf = synth.synth("t.qfmt", (B, 32, cfg.llama.qformer_dim), -1.0, 1.0)
    question = torch.randint(3, 31999, (B, TQ), generator=torch.Generator().manual_seed(5))
    for dtype in ("f16", "bf16"):
        eng = RdxEngine(cfg, dtype=dtype, device=0, max_batch=B, max_len=256, lora=True, vision=False)
        eng.load_weights(synth_getter(cfg, eng.device, lora=True), vision=False)
        t1, _, n1 = eng.generate(ids1, qf, max_new=N1, eos_id=-1, pad_id=0, reuse_prefix=True)
        assert eng.last_kept_prefix == 0 and n1 == N1
        ids2 = torch.cat([ids1, t1.cpu().long(), question], dim=1)
        t2, s2, n2 = eng.generate(ids2, qf, max_new=N2, eos_id=-1, pad_id=0, output_scores=True, reuse_prefix=True)
        assert eng.last_kept_prefix == T1 + N1 - 1          # the last selected token of turn 1 was never fed: it is prefilled now
        t2, s2 = t2.cpu().long().clone(), s2.float().cpu().clone()
        # the same prompt from scratch on the same engine
        t2f, s2f, _ = eng.generate(ids2, qf, max_new=N2, eos_id=-1, pad_id=0, output_scores=True)
        assert eng.last_kept_prefix == 0
        with torch.no_grad():
            ref = ref_cpu.LlamaOracle(cpu_w, cfg.llama, DT[dtype], lora=True).generate_greedy(ids2, qf, max_new=N2, eos_id=-1, pad_id=0)
        tol = LOGIT_TOL[dtype]
        SMALL_LEGS[dtype].add(check_greedy(t2, s2, ref, tol, 0.0, f"{dtype} reuse path vs oracle"))
        SMALL_LEGS[dtype].add(check_greedy(t2f, s2f, ref, tol, 0.0, f"{dtype} full prefill vs oracle"))
        same = (t2 == t2f.cpu().long()).long().cumprod(1).bool()           # steps up to the first difference share their inputs
        assert float(((s2 - s2f.float().cpu()).abs().amax(-1).T * same).max()) < tol, f"{dtype}: reuse path vs full prefill"
        # a third turn whose prompt diverges inside the cached part keeps only the common prefix
        ids3 = ids2.clone()
        ids3[:, T1 + 3] = (ids3[:, T1 + 3] + 7) % 31000 + 3
        eng.generate(ids2, qf, max_new=2, eos_id=-1, pad_id=0, reuse_prefix=True)
        eng.generate(ids3, qf, max_new=2, eos_id=-1, pad_id=0, reuse_prefix=True)
        assert eng.last_kept_prefix == T1 + 3
        # other image -> nothing is reused
        eng.generate(ids3, qf + 0.5, max_new=2, eos_id=-1, pad_id=0, reuse_prefix=True)
        assert eng.last_kept_prefix == 0
        eng.close()


@pytest.mark.parametrize("blk", [1, 0])
def test_multi_turn_append_at_production_width_on_the_row_block_prompt_kernels(blk):
    """Round 5: one prompt's K = 4096 projections (and, up to 128 rows, its down_proj) run on row blocks of 32 sharing an XCD's L2
    (xstat32_k / xsplit32_k<.., BLK>; `prompt_blk` 0 = the weight-stationary wstat_k of rounds 2-4). Production width, two layers: a 100-token
    first turn (four row blocks, the last one ragged), then a follow-up whose 48-token tail is prefilled behind the kept prefix
    (rdx_generate_append: two row blocks) -- logits and tokens of both turns against the oracle on the whole sequence."""
    from oracle import ref_cpu
    from radialog_amd.engine import RdxEngine, synth_getter
    cfg, cpu_w = _production_width_weights(2)
    T1, N1, TQ, N2 = 100, 6, 43, 6
    ids1 = synth.synth_prompt_ids(1, T1, vocab=cfg.llama.vocab, seed=91)
    qf = synth.synth("t.qfmtp", (1, 32, cfg.llama.qformer_dim), -1.0, 1.0)
    question = torch.randint(3, 31999, (1, TQ), generator=torch.Generator().manual_seed(9))
    for dtype in ("f16", "bf16"):
        eng = RdxEngine(cfg, dtype=dtype, device=0, max_batch=1, max_len=256, lora=True, vision=False)
        eng.load_weights(synth_getter(cfg, eng.device, lora=True), vision=False)
        eng.set_option("prompt_blk", blk)
        t1, s1, n1 = eng.generate(ids1, qf, max_new=N1, eos_id=-1, pad_id=0, output_scores=True, reuse_prefix=True)
        t1, s1 = t1.cpu().long().clone(), s1.float().cpu().clone()
        ids2 = torch.cat([ids1, t1, question], dim=1)
        t2, s2, n2 = eng.generate(ids2, qf, max_new=N2, eos_id=-1, pad_id=0, output_scores=True, reuse_prefix=True)
        assert eng.last_kept_prefix == T1 + N1 - 1
        with torch.no_grad():
            orc = ref_cpu.LlamaOracle(cpu_w, cfg.llama, DT[dtype], lora=True)
            r1 = orc.generate_greedy(ids1, qf, max_new=N1, eos_id=-1, pad_id=0)
            r2 = orc.generate_greedy(ids2, qf, max_new=N2, eos_id=-1, pad_id=0)
        tol = PROD_TOL[dtype] * 2 ** 0.5
        SMALL_LEGS[dtype].add(check_greedy(t1, s1, r1, tol, 0.0, f"{dtype} prompt_blk={blk} turn 1"))
        SMALL_LEGS[dtype].add(check_greedy(t2.cpu().long(), s2.float().cpu(), r2, tol, 0.0, f"{dtype} prompt_blk={blk} turn 2 (appended tail)"))
        eng.close()


def test_prefill_append_rejects_what_the_cache_does_not_hold(cfg):
    from radialog_amd.engine import RdxEngine, synth_getter
    from radialog_amd._lib import RdxError
    import ctypes as C
    eng = RdxEngine(cfg, dtype="bf16", device=0, max_batch=2, max_len=128, lora=True, vision=False)
    eng.load_weights(synth_getter(cfg, eng.device, lora=True), vision=False)
    tail = torch.full((1, 4), 17, dtype=torch.int32, device=eng.device)
    toks = torch.zeros(1, 4, dtype=torch.int32, device=eng.device)
    n = C.c_int(0)
    call = lambda B, keep: eng.lib.rdx_generate_append(eng.ctx, tail.data_ptr(), B, 4, keep, 4, -1, 0, toks.data_ptr(), None, C.byref(n), 0)
    assert call(1, 10) != 0                                  # nothing cached yet
    ids = _prompt(cfg, 1, 48, seed=9)
    eng.generate(ids, None, max_new=4, eos_id=-1, pad_id=0)
    assert call(1, 52) != 0                                  # 48 + 3 consumed tokens are cached, not 52
    assert call(2, 40) != 0                                  # batch differs from the cached conversation
    assert call(1, 120) != 0                                 # would overflow max_len
    assert call(1, 51) == 0
    eng.close()


@pytest.mark.parametrize("B", [1, 2])
def test_fp8_weight_decode_matches_fake_quantised_oracle(cfg, cpu_w, B):
    """BASELINE configs[4] on the small config: decoder GEMM weights in e4m3 with one scale per output row (LoRA-A rows included), the
    ONLY copy the engine holds. Prefill: fp8 x fp8 (gemm8.hip, e4m3 activations per row and K group -- inter = 1408 gives uneven
    groups); decode at batch <= 2: the GEMV / chained launches stream the e4m3 bytes and keep model-dtype activations. Oracle = the
    reference math on the same fake-quantised operands."""
    from oracle import ref_cpu
    from radialog_amd.engine import RdxEngine, synth_getter
    T, N = 72, 12
    ids = _prompt(cfg, B, T, seed=33)
    qf = synth.synth("t.qf2", (B, 32, cfg.llama.qformer_dim), -1.0, 1.0)
    for dtype in ("f16", "bf16"):
        eng = RdxEngine(cfg, dtype=dtype, device=0, max_batch=2, max_len=256, lora=True, vision=False, weights_fp8=True)
        eng.load_weights(synth_getter(cfg, eng.device, lora=True), vision=False)
        with torch.no_grad():
            ref = ref_cpu.LlamaOracle(cpu_w, cfg.llama, DT[dtype], lora=True, fp8=True).generate_greedy(ids, qf, max_new=N, eos_id=-1, pad_id=0)
        toks, scores, n = eng.generate(ids, qf, max_new=N, eos_id=-1, pad_id=0, output_scores=True, use_graph=True)
        SMALL_LEGS[dtype].add(check_greedy(toks, scores, ref, FP8_TOL, 0.0, f"{dtype} fp8 B={B}"))
        eng.close()


def test_fp8_engine_refuses_batch3_decode_on_shapes_without_an_fp8_kernel(cfg):
    """From batch 3 the fp8 engine multiplies fp8 x fp8 in the activation-stationary kernels, which are built for K = 4096; the small config
    has no such kernel and no model-dtype weight copy to fall back to: the call must fail with an error, not produce numbers."""
    from radialog_amd.engine import RdxEngine, synth_getter
    from radialog_amd._lib import RdxError
    eng = RdxEngine(cfg, dtype="bf16", device=0, max_batch=3, max_len=128, lora=True, vision=False, weights_fp8=True)
    eng.load_weights(synth_getter(cfg, eng.device, lora=True), vision=False)
    ids = _prompt(cfg, 3, 48, seed=3)
    with pytest.raises(RdxError, match="fp8 weights"):
        eng.generate(ids, None, max_new=4, eos_id=-1, pad_id=0)
    eng.close()


def test_decode_step_refuses_to_walk_past_the_reserved_slots(cfg):
    """rdx_decode_step appends a KV row and advances the RoPE position on every call: it must stop at the max_new the prefill
    reserved (and after a completed rdx_generate) instead of writing past the cache (round-1 advisor finding)."""
    from radialog_amd.engine import RdxEngine, synth_getter
    from radialog_amd._lib import RdxError
    eng = RdxEngine(cfg, dtype="bf16", device=0, max_batch=1, max_len=64, lora=True, vision=False)
    eng.load_weights(synth_getter(cfg, eng.device, lora=True), vision=False)
    ids = _prompt(cfg, 1, 40, seed=9)
    eng.prefill(ids, None, max_new=3)                # token 0 selected
    eng.decode_step(); eng.decode_step()             # tokens 1, 2
    with pytest.raises(RdxError, match="max_new"):
        eng.decode_step()
    with pytest.raises(RdxError):                     # 40 + 30 > max_len 64: refused at the prefill already
        eng.prefill(ids, None, max_new=30)
    eng.generate(ids, None, max_new=4, eos_id=-1)
    assert eng.lib.rdx_decode_step(eng.ctx, None) != 0          # a completed generate leaves nothing to step through
    eng.close()


def test_small_leg_token_identity_coverage():
    """Runs last in this module: the identical-token counts of every leg too short for a percentage bar of its own (SMALL_LEGS), summed per
    dtype, against the same bars as the long legs -- 90 % fp16, 75 % bf16. (Running this test alone finds nothing to check and skips.)"""
    if SMALL_LEGS["f16"].total + SMALL_LEGS["bf16"].total == 0:
        pytest.skip("no short legs ran in this session")
    for dtype, cover in SMALL_LEGS.items():
        if cover.total:
            print(f"short legs {dtype}: {cover.compared}/{cover.total} pairs identical")
            cover.check(MIN_COVER[dtype], f"{dtype} short legs")
