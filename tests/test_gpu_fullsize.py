"""Parity at the sizes BASELINE.json's configs are quoted on -- the shapes bench.py actually runs:

  * the FULL-SIZE image encoder (448 px, ResNet-50 3-4-6-3 with a 64-wide stem, 2048 trunk channels, projector 1408, Q-Former
    768 x 12) at batch 1 (split-K over the deep layers' few tiles) and batch 8 (256^2-tile / batched dispatch), against
    oracle/ref_cpu.forward_image (blip2_qformer.py:467-484);
  * the FULL-DEPTH decoder: all 32 Vicuna-7B layers at production width, fp16 (the reference's dtype), batch 1, T = 160, greedy
    tokens and per-step logits against the oracle AND against the exactly-accumulated evaluation of the same rounding points;
  * image -> tokens END TO END: oracle image -> oracle fp32 Q-Former output -> oracle tokens versus HIP image -> HIP Q-Former
    output -> HIP tokens (no hand-over of the GPU's embeddings to the oracle's decoder).
"""
import pytest
import torch

from radialog_amd import synth
from radialog_amd.config import LlamaCfg, RaDialogCfg, full_cfg, small_cfg
from _parity import check_greedy, teacher_forced

pytestmark = pytest.mark.gpu

DT = {"f16": torch.float16, "bf16": torch.bfloat16}
ENC_TOL = {"f16": 5e-3, "bf16": 3e-2}


def _rel_l2(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


@pytest.fixture(scope="module")
def full_vis_w():
    cfg = full_cfg()
    return cfg, synth.make_weights({**synth.vision_specs(cfg.vision), **synth.qformer_specs(cfg.qformer)})


@pytest.fixture(scope="module")
def full_enc_ref(full_vis_w):
    from oracle import ref_cpu
    cfg, W = full_vis_w
    img = synth.synth_images(8, cfg.vision.img)
    with torch.no_grad():
        ref_q, ref_emb = ref_cpu.forward_image(img, W, cfg)
    return img, ref_q, ref_emb


@pytest.mark.parametrize("dtype,trunk", [("f16", "packed"), ("bf16", "packed"), ("f16", "rowmajor")])
def test_full_size_encoder_matches_oracle(full_vis_w, full_enc_ref, dtype, trunk, monkeypatch):
    """trunk = "packed": the round-4 default -- the ResNet trunk on fragment-packed activations (pconv_k); "rowmajor" (RDX_PCONV=0 at
    rdx_create): the LDS-staged row-major kernels of rounds 1-3, kept as the A/B leg. Both against the fp32 oracle, and against each other
    within the same tolerance."""
    from radialog_amd.engine import RdxEngine, synth_getter
    cfg, W = full_vis_w
    img, ref_q, ref_emb = full_enc_ref
    if trunk == "rowmajor":
        monkeypatch.setenv("RDX_PCONV", "0")
    eng = RdxEngine(cfg, dtype=dtype, device=0, llama=False)
    eng.load_weights(synth_getter(cfg, eng.device), llama=False)
    tol = ENC_TOL[dtype]
    for B in (1, 8, 3):                   # 1: few-tile grids; 8: batched tiles; 3 after 8: a smaller batch in the grown workspace
        q, emb = eng.encode_image(img[:B].to(eng.device))
        assert q.shape == (B, 32, 768) and emb.shape == (B, 196, 1408)
        assert torch.isfinite(q).all() and torch.isfinite(emb).all()
        e_emb, e_q = _rel_l2(emb.cpu(), ref_emb[:B]), _rel_l2(q.cpu(), ref_q[:B])
        print(f"full-size encoder {dtype} {trunk} B={B}: rel-L2 image_embeds {e_emb:.3e}, Q-Former out {e_q:.3e}")
        assert e_emb < tol, f"B={B}: image_embeds (ResNet-50 trunk + projector + scramble + ln_vision) rel-L2 {e_emb}"
        assert e_q < tol, f"B={B}: Q-Former last_hidden_state rel-L2 {e_q}"
        # per-image: no row may hide behind the batch norm
        for b in range(B):
            assert _rel_l2(q[b].cpu(), ref_q[b]) < 2 * tol, f"B={B} image {b}"
    eng.close()


def test_image_to_tokens_end_to_end_matches_oracle():
    """Nothing crosses over: the oracle runs image -> fp32 encoder -> fp32 Q-Former -> fp16 decoder -> tokens on the CPU, the engine
    runs the same chain on the GPU (fp16 encoder with fp32 accumulation). The encoder's rounding noise (rel-L2 ~1e-3) reaches the
    decoder through img_proj and the 32 spliced rows; tokens must still be the oracle's and logits within the decoder tolerance
    plus what that input perturbation is worth (measured and asserted: < 2e-2)."""
    from oracle import ref_cpu
    from radialog_amd.engine import RdxEngine, synth_getter
    cfg = small_cfg()
    W = synth.make_weights({**synth.vision_specs(cfg.vision), **synth.qformer_specs(cfg.qformer), **synth.llama_specs(cfg.llama)})
    B, T, N = 3, 64, 12
    img = synth.synth_images(B, cfg.vision.img, seed=31)
    ids = synth.synth_prompt_ids(B, T, vocab=cfg.llama.vocab, img_offset=5, pad_rows=False, seed=17)
    ids[1] = torch.cat([torch.zeros(4, dtype=torch.long), ids[1, : T - 4]])
    with torch.no_grad():
        rq, _ = ref_cpu.forward_image(img, W, cfg)
        ref = ref_cpu.LlamaOracle(W, cfg.llama, torch.float16, lora=True).generate_greedy(ids, rq, max_new=N, eos_id=-1)
    eng = RdxEngine(cfg, dtype="f16", device=0, max_batch=B, max_len=128)
    eng.load_weights(synth_getter(cfg, eng.device))
    q, _ = eng.encode_image(img.to(eng.device), want_image_embeds=False)
    toks, scores, n = eng.generate(ids, q, max_new=N, eos_id=-1, output_scores=True)
    cmp_, tot, worst = check_greedy(toks, scores, ref, 2e-2, 0.9, "image -> tokens")
    print(f"end to end: {cmp_}/{tot} pairs identical, worst logit error {worst:.4g}, encoder rel-L2 {_rel_l2(q.cpu(), rq):.3e}")
    eng.close()


def test_full_size_encoder_into_production_width_decoder_end_to_end(full_vis_w):
    """The same end-to-end identity at the benchmark's shapes: full-size encoder (768-wide Q-Former output) into a production-width
    decoder (hidden 4096, inter 11008, vocab 32001; two layers so that the CPU oracle finishes in seconds), fp16."""
    from oracle import ref_cpu
    from radialog_amd.engine import RdxEngine, synth_getter
    base, Wv = full_vis_w
    cfg = RaDialogCfg(llama=LlamaCfg(layers=2), qformer=base.qformer, vision=base.vision)
    Wl = synth.make_weights(synth.llama_specs(cfg.llama, lora=True))
    B, T, N = 2, 96, 6
    img = synth.synth_images(B, cfg.vision.img, seed=77)
    ids = synth.synth_prompt_ids(B, T, vocab=cfg.llama.vocab, img_offset=20, pad_rows=False, seed=19)
    with torch.no_grad():
        rq, _ = ref_cpu.forward_image(img, Wv, cfg)
        ref = ref_cpu.LlamaOracle(Wl, cfg.llama, torch.float16, lora=True).generate_greedy(ids, rq, max_new=N, eos_id=-1)
    eng = RdxEngine(cfg, dtype="f16", device=0, max_batch=B, max_len=128)
    eng.load_weights(synth_getter(cfg, eng.device))
    q, _ = eng.encode_image(img.to(eng.device), want_image_embeds=False)
    toks, scores, n = eng.generate(ids, q, max_new=N, eos_id=-1, output_scores=True)
    # the full-size encoder's fp16 rounding noise (Q-Former output rel-L2 ~2e-3, twice the small model's) enters through 32 rows
    cmp_, tot, worst = check_greedy(toks, scores, ref, 3e-2, 0.9, "full-size image -> tokens")
    print(f"full-size end to end: {cmp_}/{tot} pairs identical, worst logit error {worst:.4g}, encoder rel-L2 {_rel_l2(q.cpu(), rq):.3e}")
    eng.close()


def _full_depth_engine_and_weights(dtype, B, max_len):
    """All 32 production-width layers: the engine, and the SAME bytes for the oracle -- generated on the GPU (seconds instead of
    minutes), rounded to the model dtype, moved to the host."""
    from radialog_amd.engine import RdxEngine, synth_getter
    cfg = full_cfg()
    dt = DT[dtype]
    eng = RdxEngine(cfg, dtype=dtype, device=0, max_batch=B, max_len=max_len, vision=False)
    eng.load_weights(synth_getter(cfg, eng.device), vision=False)
    specs = synth.llama_specs(cfg.llama, lora=True)
    probe = "model.layers.0.self_attn.q_proj.lora_A.weight"
    assert torch.equal(specs[probe][1](probe, specs[probe][0], "cpu"), specs[probe][1](probe, specs[probe][0], eng.device).cpu())
    W = {name: gen(name, shape, eng.device).to(dt).cpu() for name, (shape, gen) in specs.items()}
    return cfg, eng, W


def _head(ref, n):
    """The first n steps of a LlamaOracle.generate_greedy result (the free-running legs compare a prefix of the long oracle run)."""
    return {"tokens": ref["tokens"][:, :n], "scores": ref["scores"][:n], "margins": ref["margins"][:n]}


FULL_TOL = {"f16": 6e-2, "bf16": 0.45}      # one-layer tolerance x sqrt(32 layers): 1e-2 -> 6e-2 (fp16, north_star's dtype), 8e-2 -> 0.45 (bf16)


def _exact_columns(hip_rows, ref_rows, exact_rows):
    """Per-step distances from the exactly-accumulated evaluation: (|hip - exact|, |oracle - exact|), each the largest of the rows x 32 001 logit
    differences of a step."""
    e_h = [float((h.float() - x.float()).abs().max()) for h, x in zip(hip_rows, exact_rows)]
    e_o = [float((o.float() - x.float()).abs().max()) for o, x in zip(ref_rows, exact_rows)]
    return e_h, e_o


def _stats(v):
    t = torch.tensor(v)
    return float(t.median()), float(t.quantile(0.9)), float(t.max())


@pytest.mark.slow
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_full_depth_32_layer_decoder_matches_oracle(dtype):
    """BASELINE configs[0]/[1] decoder in full: 32 layers at production width, batch 1, the bench's 160-token prompt with the 32 <IMG>
    slots -- in fp16 (the reference's dtype) AND in bf16 (the dtype bench.py times). Three legs on one engine:

    (a) 6 free-running greedy tokens through the hipGraph step against the torch-CPU oracle: tokens identical wherever its margin exceeds twice
        the measured logit error (tests/_parity.py).
    (b) a REPORT-LENGTH horizon -- 64 teacher-forced decode steps (positions 160 .. 223; the oracle's token is fed back through
        rdx_decode_step_ids so a near-tie flip cannot end the comparison) at full depth against the torch-CPU oracle, with an ABSOLUTE backstop
        bar: 99 % of the steps within 1e-2 x sqrt(32) = 6e-2 in fp16 (0.45 in bf16), all within 1.5 x that, every differing argmax at an oracle
        margin <= 2 x the measured error of that step, and >= 90 % (fp16) / 75 % (bf16) argmax identity.
    (c) round 6 (VERDICT r5 "weak" 1): the EXACT evaluation -- the same op sequence and rounding points with every contraction accumulated in
        fp64, LlamaOracle(exact=True) -- arbitrates ALL 64 steps (rounds 3-5: 3 steps; the CPU needs a minute per step to widen 6.6 G
        parameters, so the arbiter now runs on this GPU with its fp64 weights cached in HBM: oracle/ref_cpu.py). HIP, torch-CPU oracle and exact
        evaluation are fed the same tokens; per step e_h = |HIP - exact|, e_o = |oracle - exact| (largest of 32 001 logit differences). Over 32
        layers the accumulation-order noise of ANY two fp32-accumulating implementations is 3-4e-2 in fp16, so the claim that means something is
        relative: HIP is no further from the exact value than torch's own CPU kernels are -- asserted on the horizon's median (x 1.25), 90th
        percentile and maximum (x 1.5), each + 1 ulp at |logit| in [4, 8); the per-step form e_h <= e_o + 1 ulp is counted and printed (two
        independent noises of equal size satisfy it about half of the time, so it cannot be a per-step assertion)."""
    from oracle import ref_cpu
    dt = DT[dtype]
    cfg, eng, W = _full_depth_engine_and_weights(dtype, 1, 256)
    T, N, NTF = 160, 6, 64
    ids = synth.synth_prompt_ids(1, T, vocab=cfg.llama.vocab)
    qf = synth.synth("t.qf_full", (1, 32, cfg.llama.qformer_dim), -1.0, 1.0)
    toks, scores, n = eng.generate(ids, qf, max_new=N, eos_id=-1, output_scores=True)
    toks, scores = toks.cpu().long().clone(), scores.float().cpu().clone()
    with torch.no_grad():
        ref = ref_cpu.LlamaOracle(W, cfg.llama, dt, lora=True).generate_greedy(ids, qf, max_new=NTF, eos_id=-1)
        arb = ref_cpu.LlamaOracle(W, cfg.llama, dt, lora=True, exact=True, device=eng.device)
        del W
        exact_rows = arb.forced_logits(ids, qf, ref["tokens"])
        del arb
    torch.cuda.empty_cache()
    print(f"full depth {dtype}: tokens hip {toks[0].tolist()} oracle {ref['tokens'][0, :N].tolist()}; margins {[round(float(m), 3) for m in ref['margins'][:N, 0]]}")
    check_greedy(toks, scores, _head(ref, N), FULL_TOL[dtype], 0.0, f"full depth {dtype}")
    # leg (b): 64 teacher-forced steps against the torch-CPU oracle (the absolute backstop)
    hip_rows = []
    same, total, worst = teacher_forced(eng, ref, ids, qf, NTF, FULL_TOL[dtype], f"full depth teacher-forced {dtype}", collect=hip_rows)
    eng.close()
    print(f"full depth {dtype}, {NTF} teacher-forced steps (positions {T}..{T + NTF - 1}): {same}/{total} argmax tokens identical, worst logit error "
          f"{worst:.4g} (bar: 99 % < {FULL_TOL[dtype]}, all < {1.5 * FULL_TOL[dtype]:.3g}); median oracle margin {float(ref['margins'].median()):.3g}")
    assert same >= {"f16": 0.9, "bf16": 0.75}[dtype] * total, f"{dtype}: only {same}/{total} full-depth steps chose the oracle's token"
    # leg (c): the exact evaluation over the whole horizon
    e_h, e_o = _exact_columns(hip_rows, ref["scores"], exact_rows)
    ulp = 2.0 ** -8 if dtype == "f16" else 2.0 ** -5
    (mh, ph, xh), (mo, po, xo) = _stats(e_h), _stats(e_o)
    inside = sum(1 for a, b in zip(e_h, e_o) if a <= b + ulp)
    ex_tok = sum(int(r[0].float().argmax()) == int(ref["tokens"][0, s]) for s, r in enumerate(exact_rows))
    print(f"full depth {dtype}, exact arbiter over {NTF} steps: |hip-exact| median {mh:.4g} p90 {ph:.4g} max {xh:.4g}; |oracle-exact| median {mo:.4g} p90 {po:.4g} "
          f"max {xo:.4g}; steps with |hip-exact| <= |oracle-exact| + 1 ulp: {inside}/{NTF}; exact argmax == oracle token on {ex_tok}/{NTF} steps")
    assert mh <= 1.25 * mo + ulp, f"{dtype}: median |hip - exact| {mh:.4g} vs the torch-CPU oracle's {mo:.4g}"
    assert ph <= 1.5 * po + ulp and xh <= 1.5 * xo + ulp, f"{dtype}: |hip - exact| p90 {ph:.4g} / max {xh:.4g} vs the oracle's {po:.4g} / {xo:.4g}"


# batch-32 legs: the oracle runs a subset of the rows (a row's arithmetic does not depend on its neighbours); the subsets of the two dtypes are
# COMPLEMENTARY (rounds 4-5 never compared rows 4-7, 12-15, ... -- lanes e >= 4 of each half row tile -- at full depth)
_B32_ROWS = {"f16": [r for r in range(32) if (r >> 2) % 2 == 0], "bf16": [4, 6, 12, 14, 20, 22, 28, 30]}


@pytest.mark.slow
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_full_depth_batch32_decoder_matches_oracle(dtype):
    """BASELINE configs[2] decoder in full: 32 layers at production width, batch 32 with left-padded rows (prompts as the bench builds them,
    every 4th row padded; T = 96 -- the padded rows' 32-slot image block needs T >= 92 -- because the oracle's batched prefill is most of this
    test's minutes; bench.py's `parity_b32` checks row 0 of the timed T = 160 run at full depth): the activation-stationary / K-split kernels, the
    throughput attention with the row-major K cache and the batched prefill GEMMs at full depth. fp16 (the reference's dtype; 16 oracle rows) and,
    round 6, bf16 (the benchmarked dtype; the 8 rows the fp16 leg leaves out of every second group of four). Two legs on one engine and ONE oracle run:
    (a) 4 free-running tokens through the hipGraph-captured step against the oracle's first 4: logits within the full-depth bar (6e-2 fp16 / 0.45
        bf16), tokens identical wherever the oracle's margin exceeds twice the measured error, >= 90 % / 75 % of the pairs;
    (b) 8 teacher-forced steps, none lost to a near-tie, same absolute bar, >= 90 % / 75 % argmax identity."""
    from oracle import ref_cpu
    cfg, eng, W = _full_depth_engine_and_weights(dtype, 32, 128)
    B, T, N, NTF = 32, 96, 4, 8
    cover = {"f16": 0.9, "bf16": 0.75}[dtype]
    ids = synth.synth_prompt_ids(B, T, vocab=cfg.llama.vocab, pad_rows=True, seed=7)
    qf = synth.synth("t.qf_full32", (B, 32, cfg.llama.qformer_dim), -1.0, 1.0)
    toks, scores, n = eng.generate(ids, qf, max_new=N, eos_id=-1, pad_id=0, output_scores=True, use_graph=True)
    rows = _B32_ROWS[dtype]
    toks, scores = toks.cpu().long()[rows].clone(), scores.float().cpu()[:, rows].clone()
    with torch.no_grad():
        ref = ref_cpu.LlamaOracle(W, cfg.llama, DT[dtype], lora=True).generate_greedy(ids[rows], qf[rows], max_new=NTF, eos_id=-1, pad_id=0)
    del W
    cmp_, tot, worst = check_greedy(toks, scores, _head(ref, N), FULL_TOL[dtype], cover, f"full depth batch 32 {dtype}")
    print(f"full depth batch 32 {dtype} (oracle rows {rows}): {cmp_}/{tot} pairs identical, worst logit error {worst:.4g}, "
          f"smallest oracle margin {float(ref['margins'][:N].min()):.4g}")
    same, total, worst = teacher_forced(eng, ref, ids, qf, NTF, FULL_TOL[dtype], f"full depth batch 32 teacher-forced {dtype}", rows=rows)
    eng.close()
    print(f"full depth batch 32 {dtype}, {NTF} teacher-forced steps: {same}/{total} argmax tokens identical, worst logit error {worst:.4g}")
    assert same >= cover * total


@pytest.mark.slow
def test_full_depth_64_row_block_decoder_fp16_matches_oracle():
    """Round 6 (VERDICT r5 "weak" 3): the 33-128 row family (xstat32_k / xsplit32_k<.., BLK>: two 32-row blocks per tile walker, the batched prefill,
    the throughput attention at 2048 (row, head) pairs) through ALL 32 layers -- rounds 5's legs stopped at two layers. 64 rows, T = 96 with every
    4th row left-padded, fp16; the oracle runs 4 rows -- one padded and one unpadded row of each 32-row block -- 4 teacher-forced steps after the
    prefill, the other 60 rows ride along on their own tokens."""
    from oracle import ref_cpu
    cfg, eng, W = _full_depth_engine_and_weights("f16", 64, 128)
    B, T, NTF = 64, 96, 4
    ids = synth.synth_prompt_ids(B, T, vocab=cfg.llama.vocab, pad_rows=True, seed=9)
    qf = synth.synth("t.qf_full64", (B, 32, cfg.llama.qformer_dim), -1.0, 1.0)
    rows = [3, 17, 38, 63]
    with torch.no_grad():
        ref = ref_cpu.LlamaOracle(W, cfg.llama, torch.float16, lora=True).generate_greedy(ids[rows], qf[rows], max_new=NTF, eos_id=-1, pad_id=0)
    del W
    same, total, worst = teacher_forced(eng, ref, ids, qf, NTF, FULL_TOL["f16"], "full depth 64 rows teacher-forced fp16", rows=rows)
    eng.close()
    print(f"full depth 64 rows fp16 (oracle rows {rows}), {NTF} teacher-forced steps: {same}/{total} argmax tokens identical, worst logit error {worst:.4g}")
    assert same >= 0.9 * total


# ----------------------------------------------------------------------------------------------------------------------------------------
# round 6 (VERDICT r5 "missing" 2, 3): the two optional encoder modes at their REAL shapes
# ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_two_image_mode_at_448px_matches_oracle(full_vis_w, dtype):
    """rdx_encode_image2 at the production shape: both 448 px images through the ResNet-50 trunk, the VisionTransformerPooler at 392 tokens x 256,
    8 heads x 32, 3 blocks (biovil_t/transformer.py:73-119,:163-224; sine position + type embeddings), the 512-wide projector input, scramble,
    ln_vision and the Q-Former -- against oracle/ref_cpu.forward_image(previous=...), whose pooler is pinned by tests/golden/vit_pooler.npz.
    Rounds 2-5 ran this mode at 128 px / 16 tokens x 2 / 2 blocks / 2 heads only."""
    from oracle import ref_cpu
    from radialog_amd.engine import RdxEngine, synth_getter
    cfg, W = full_vis_w
    assert cfg.vision.pool_blocks == 3 and cfg.vision.pool_heads == 8 and cfg.vision.b2v == 256 and cfg.vision.grid == 14
    B = 2
    img = synth.synth_images(B, cfg.vision.img, seed=21)
    prev = synth.synth_images(B, cfg.vision.img, seed=22)
    with torch.no_grad():
        ref_q, ref_emb = ref_cpu.forward_image(img, W, cfg, previous=prev)
        single_q, _ = ref_cpu.forward_image(img[:1], W, cfg)
    eng = RdxEngine(cfg, dtype=dtype, device=0, llama=False)
    eng.load_weights(synth_getter(cfg, eng.device), llama=False)
    q, emb = eng.encode_image(img.to(eng.device), previous_image=prev.to(eng.device))
    eng.close()
    assert q.shape == (B, 32, 768) and emb.shape == (B, 196, 1408) and torch.isfinite(q).all() and torch.isfinite(emb).all()
    e_emb, e_q = _rel_l2(emb.cpu(), ref_emb), _rel_l2(q.cpu(), ref_q)
    print(f"two-image mode 448 px {dtype}: rel-L2 image_embeds {e_emb:.3e}, Q-Former out {e_q:.3e}")
    tol = ENC_TOL[dtype]
    assert e_emb < tol and e_q < tol
    for b in range(B):
        assert _rel_l2(q[b].cpu(), ref_q[b]) < 2 * tol, f"image {b}"
    assert _rel_l2(q[:1].cpu(), single_q) > 0.05                 # and it is a different function of the inputs than the single-image mode


def test_findings_classifier_at_488px_matches_oracle():
    """rdx_classify_findings at the shape demo.py runs it (findings_classifier/chexpert_model.py:15-21, demo.py:155-170,:256-261): 488 px centre crop ->
    16 x 16 grid, stock 128-wide projector, avg_pool2d(4), 2048 -> 512 -> 14 -- logits against oracle/ref_cpu.findings_logits, predicted label sets
    equal wherever the oracle's logit is outside the tolerance of the decision boundary. Rounds 3-5 compared at 136 px only."""
    from oracle import ref_cpu
    from radialog_amd.chexpert_model import ChexpertClassifier
    from radialog_amd.config import classifier_cfg
    cfg = classifier_cfg()
    assert cfg.vision.grid == 16 and cfg.vision.proj == 128 and cfg.cls.hidden == 512
    W = synth.make_weights(synth.classifier_specs(cfg.vision, cfg.cls))
    img = synth.synth_images(3, cfg.vision.img, seed=5)
    with torch.no_grad():
        ref = ref_cpu.findings_logits(img, W, cfg.vision, cfg.cls)
    for dtype, tol in (("f16", 5e-3), ("bf16", 3e-2)):
        m = ChexpertClassifier(num_classes=cfg.cls.classes, cfg=cfg, dtype=dtype)
        m.load_state_dict(W)
        out = m(img.cuda()).float().cpu()
        assert out.shape == ref.shape and torch.isfinite(out).all()
        scale = float(ref.abs().max().clamp_min(1.0))
        err = float((out - ref).abs().max())
        print(f"findings classifier 488 px {dtype}: worst logit error {err:.4g} at logit scale {scale:.3g}")
        assert err < 4 * tol * scale, f"{dtype}: logits differ by {err}"
        far = ref.abs() > 4 * tol * scale
        assert torch.equal((out > 0)[far], (ref > 0)[far])
        m._engine.close()


# ----------------------------------------------------------------------------------------------------------------------------------------
# the encoder at the batches the project runs: 256 (enc_b256, embed_dump's default), 32 (BASELINE configs[2]) and a ragged 33
# ----------------------------------------------------------------------------------------------------------------------------------------
_ORACLE_POS = [0, 3, 16, 127, 128, 201, 254, 255]       # where the 8 oracle images of full_enc_ref sit in the batch of 256
_DUP = (4, 5, 6, 7)                                      # one image four times: the four phases of 196-row images against 16-row tiles
_NOISE_POS = (9, 30)                                     # the distinct-channel noise images inside the batch-32 run


@pytest.fixture(scope="module")
def noise_enc_ref(full_vis_w):
    """Two white-noise images with three DIFFERENT channels through the oracle (every synth_images input repeats one channel)."""
    from oracle import ref_cpu
    cfg, W = full_vis_w
    img = torch.rand(2, 3, cfg.vision.img, cfg.vision.img, generator=torch.Generator().manual_seed(448))
    with torch.no_grad():
        ref_q, _ = ref_cpu.forward_image(img, W, cfg)
    return img, ref_q


def _production_batch(img8, S, device):
    x = synth.synth_images(256, S, device=device, seed=101)
    x[_DUP[1]:_DUP[-1] + 1] = x[_DUP[0]]
    for j, p in enumerate(_ORACLE_POS):
        x[p] = img8[j].to(device)
    return x


def _batch_invariance(run, x, tol, label):
    """run(x) -> per-row output. Twice the same batch: bit-identical; the duplicates: bit-identical to each other (a row's arithmetic does not
    depend on its neighbours within one launch); every row: within tol (relative L2) of the same image run alone at B = 1. Returns
    (batch output, worst B = 1 distance).
    The B = 1 encode is not the same arithmetic as the batched one -- one image's deep stages split K over the waves of a workgroup, the Q-Former's
    32 rows run other tilings -- so the two differ by the rounding noise of two fp32-accumulating evaluations, about the size of either one's
    distance from the oracle (measured: 2.8e-3 fp16 / 2.1e-2 bf16 at B = 256). The bar is ENC_TOL, half the per-image oracle bar."""
    out = run(x)
    assert torch.isfinite(out).all(), label
    assert torch.equal(out, run(x)), f"{label}: the same batch twice gives different bits"
    dups = [b for b in _DUP if b < x.shape[0]]
    for b in dups[1:]:
        assert torch.equal(out[b], out[dups[0]]), f"{label}: duplicate image at {b} differs from the one at {dups[0]}"
    errs = [_rel_l2(out[b].cpu(), run(x[b:b + 1])[0].cpu()) for b in range(x.shape[0])]
    worst = max(errs)
    assert worst < tol, f"{label}: row {errs.index(worst)} is {worst:.3e} (rel-L2) from the same image encoded alone"
    return out, worst


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_full_size_encoder_at_production_batches(full_vis_w, full_enc_ref, noise_enc_ref, dtype):
    """rdx_encode_image at B = 256 (the oracle's 8 images spread over the batch, incl. both ends and both sides of 128), B = 32 (configs[2];
    with the two distinct-channel noise images inside) and B = 33 (a ragged last workgroup), packed trunk, 448 px: the oracle rows meet the
    per-image bar, duplicates are bit-identical, every row is within ENC_TOL of its own B = 1 encode in the same (grown) context."""
    from radialog_amd.engine import RdxEngine, synth_getter
    cfg, W = full_vis_w
    img8, ref_q, _ = full_enc_ref
    nimg, nref = noise_enc_ref
    tol = ENC_TOL[dtype]
    eng = RdxEngine(cfg, dtype=dtype, device=0, llama=False)
    eng.load_weights(synth_getter(cfg, eng.device), llama=False)
    run = lambda x: eng.encode_image(x, want_image_embeds=False)[0]            # noqa: E731
    x = _production_batch(img8, cfg.vision.img, eng.device)
    q, worst = _batch_invariance(run, x, tol, f"{dtype} B=256")
    errs = [_rel_l2(q[p].cpu(), ref_q[j]) for j, p in enumerate(_ORACLE_POS)]
    print(f"encoder {dtype} B=256: oracle rows rel-L2 max {max(errs):.3e} (bar {2 * tol}); worst row vs B=1 {worst:.3e} (bar {tol})")
    assert max(errs) < 2 * tol, errs
    x32 = x[:32].clone()
    for j, p in enumerate(_NOISE_POS):
        x32[p] = nimg[j].to(eng.device)
    q32, worst32 = _batch_invariance(run, x32, tol, f"{dtype} B=32")
    q33, worst33 = _batch_invariance(run, x[:33].contiguous(), tol, f"{dtype} B=33")
    n1 = run(nimg.to(eng.device))
    en = [_rel_l2(n1[j].cpu(), nref[j]) for j in range(2)] + [_rel_l2(q32[p].cpu(), nref[j]) for j, p in enumerate(_NOISE_POS)]
    print(f"encoder {dtype} B=32 / 33: worst row vs B=1 {worst32:.3e} / {worst33:.3e}; distinct-channel noise images vs oracle {max(en):.3e} (bar {tol})")
    assert max(en) < tol, en
    assert _rel_l2(q33[:32].cpu(), q[:32].cpu()) < tol and _rel_l2(q32[:9].cpu(), q[:9].cpu()) < tol
    eng.close()


def test_findings_classifier_at_488px_batch_17():
    """rdx_classify_findings at B = 17, 488 px: ragged stem tiles and pad rows in every packed tensor (17 x 122^2 rows). Duplicates give
    bit-identical logits; every row is within the classifier bar (4 x tol x max(1, |logit|)) of its B = 1 logits."""
    from radialog_amd.chexpert_model import ChexpertClassifier
    from radialog_amd.config import classifier_cfg
    cfg = classifier_cfg()
    W = synth.make_weights(synth.classifier_specs(cfg.vision, cfg.cls))
    x = synth.synth_images(17, cfg.vision.img, seed=55, device="cuda")
    x[_DUP[1]:_DUP[-1] + 1] = x[_DUP[0]]
    for dtype, tol in (("f16", 5e-3), ("bf16", 3e-2)):
        m = ChexpertClassifier(num_classes=cfg.cls.classes, cfg=cfg, dtype=dtype)
        m.load_state_dict(W)
        out = m(x).float()
        assert torch.isfinite(out).all() and torch.equal(out, m(x).float())
        for b in _DUP[1:]:
            assert torch.equal(out[b], out[_DUP[0]]), f"{dtype}: duplicate at {b}"
        worst = 0.0
        for b in range(17):
            one = m(x[b:b + 1]).float()[0]
            e = float((out[b] - one).abs().max()) / float(one.abs().max().clamp_min(1.0))
            worst = max(worst, e)
            assert e < 4 * tol, f"{dtype}: row {b} differs from its B = 1 logits by {e:.3g} x scale"
        print(f"findings classifier 488 px {dtype} B=17: worst row vs B=1 {worst:.3e} x logit scale (bar {4 * tol})")
        m._engine.close()


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_two_image_mode_at_batch_16(full_vis_w, dtype):
    """rdx_encode_image2 at B = 16 (a trunk batch of 32, the ViT pooler at 16 x 392 tokens): duplicates bit-identical, every row within
    ENC_TOL of the same pair encoded alone."""
    from radialog_amd.engine import RdxEngine, synth_getter
    cfg, W = full_vis_w
    eng = RdxEngine(cfg, dtype=dtype, device=0, llama=False)
    eng.load_weights(synth_getter(cfg, eng.device), llama=False)
    img = synth.synth_images(16, cfg.vision.img, seed=61, device=eng.device)
    prev = synth.synth_images(16, cfg.vision.img, seed=62, device=eng.device)
    img[_DUP[1]:_DUP[-1] + 1] = img[_DUP[0]]
    prev[_DUP[1]:_DUP[-1] + 1] = prev[_DUP[0]]
    pair = torch.cat([img, prev], 1)                 # rows carry both images through _batch_invariance's slicing
    run = lambda xp: eng.encode_image(xp[:, :3].contiguous(), want_image_embeds=False, previous_image=xp[:, 3:].contiguous())[0]   # noqa: E731
    _, worst = _batch_invariance(run, pair, ENC_TOL[dtype], f"two-image {dtype} B=16")
    print(f"two-image mode {dtype} B=16: worst row vs B=1 {worst:.3e} (bar {ENC_TOL[dtype]})")
    eng.close()
