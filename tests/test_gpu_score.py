"""Scoring given tokens on the GPU: score_rows_k (radialog_amd/csrc/score.hip) alone through rdx_score_rows_test, rdx_score end to end against the CPU
oracle's all-position logits restated by tests/_score.py, its chunking, its agreement with the prefill + teacher-forced decode path, the state it leaves,
LlamaForCausalLM.forward on top of it, and its refusals.

Bars. The kernel alone: the bar derived in tests/_score.py from the fp32 operations of the definition (tests/test_score_host.py holds an fp32 emulation of
the kernel's order inside it and four planted faults outside it, on these very inputs). End to end: |d logprob| <= |d x_label| + |d logsumexp| <=
2 max |d x|, so TWICE the logit tolerance the teacher-forced leg of the same configuration passes to _parity.teacher_forced in tests/test_gpu_parity.py
(small_cfg: LOGIT_TOL; production width, one layer: PROD_TOL). top1 must be the oracle's argmax wherever the oracle's top-2 margin exceeds that logit
tolerance, and at least 90 % of the scored positions must be that decisive (synth.py's planted lm_head rows; checked on the CPU for these seeds:
seed 63: f16 >= 98 %, bf16 >= 92 % per case; production width 184 of 188)."""
import ctypes as C

import pytest
import torch

import _score as S
from radialog_amd import synth
from radialog_amd.config import small_cfg
from test_gpu_parity import LOGIT_TOL, PROD_TOL

pytestmark = pytest.mark.gpu

DT = {"f16": torch.float16, "bf16": torch.bfloat16}
T_SMALL = 56
MIN_DECISIVE = 0.9


@pytest.fixture(scope="module")
def cfg():
    return small_cfg()


@pytest.fixture(scope="module")
def cpu_w(cfg):
    return synth.make_weights(synth.llama_specs(cfg.llama, lora=True))


@pytest.fixture(scope="module", params=["f16", "bf16"])
def engine(request, cfg):
    from radialog_amd.engine import RdxEngine, synth_getter
    eng = RdxEngine(cfg, dtype=request.param, device=0, max_batch=5, max_len=128, lora=True, vision=False)
    eng.load_weights(synth_getter(cfg, eng.device, lora=True), vision=False)
    yield eng
    eng.close()


def labels_of(ids):
    """labels = ids, with -100 at the pads and at a row's first real token: its predecessor is a pad position, whose hidden state is garbage that nothing
    reads on either side (the oracle's pad-query rows attend nothing)."""
    labels = ids.clone()
    labels[ids == 0] = -100
    labels[:, 1:][ids[:, :-1] == 0] = -100
    return labels


def small_case(cfg, B, T=T_SMALL):
    """ids [B, T] with the 32 <IMG> ids inside; B == 2: row 1 left-padded by 3. labels = ids with the pads ignored."""
    ids = synth.synth_prompt_ids(B, T, vocab=cfg.llama.vocab, img_offset=6, pad_rows=False, seed=63)
    if B == 2:
        ids[1] = torch.cat([torch.zeros(3, dtype=torch.long), ids[1, : T - 3]])
    qf = synth.synth(f"t.score.qf{B}", (B, 32, cfg.llama.qformer_dim), -1.0, 1.0)
    return ids, qf, labels_of(ids)


_REF = {}


def oracle_logits(cpu_w, lcfg, dtype, ids, qf, key):
    """The oracle's logits of every position [B, T, V] (model dtype, CPU), computed once per case."""
    from oracle import ref_cpu
    if key not in _REF:
        orc = ref_cpu.LlamaOracle(cpu_w, lcfg, DT[dtype], lora=True)
        km = ids.ne(0).long()
        with torch.no_grad():
            logits, _, _ = orc.forward(orc.embed(ids, qf), km, ref_cpu.positions_from_mask(km), all_logits=True)
        _REF[key] = logits.cpu()
    return _REF[key]


def decisive(ref_logits, labels, tol):
    """[B, T] bool: scored entries (t >= 1, label != -100) whose predecessor row has an oracle top-2 margin above tol; and the oracle's argmax there."""
    top2 = ref_logits[:, :-1].float().topk(2, dim=-1)
    margin = top2.values[..., 0] - top2.values[..., 1]
    scored = torch.zeros_like(labels, dtype=torch.bool)
    scored[:, 1:] = labels[:, 1:] != -100
    dec = torch.zeros_like(scored)
    dec[:, 1:] = scored[:, 1:] & (margin > tol)
    am = torch.full_like(labels, -1)
    am[:, 1:] = top2.indices[..., 0]
    return scored, dec, am


def check_against_oracle(lp, t1, ref_logits, labels, tol, label):
    want = S.token_logprobs(ref_logits, labels)
    scored, dec, am = decisive(ref_logits, labels, tol)
    lp, t1 = lp.double().cpu(), t1.cpu().long()
    err = (lp - want).abs()
    print(f"{label}: worst |logprob - oracle| {float(err.max()):.4g} (bar {2 * tol}), {int(dec.sum())}/{int(scored.sum())} positions decisive")
    assert not torch.isnan(lp).any() and float(err.max()) <= 2 * tol, f"{label}: logprob differs by {float(err.max()):.4g} (bar {2 * tol}) at flat index {int(err.argmax())}"
    assert bool((lp[~scored] == 0).all()) and bool((t1[~scored] == -1).all()), f"{label}: entries that are not scored must hold (0, -1)"
    assert int(dec.sum()) >= MIN_DECISIVE * int(scored.sum()), f"{label}: only {int(dec.sum())}/{int(scored.sum())} positions are decisive"
    assert torch.equal(t1[dec], am[dec]), f"{label}: top1 differs from the oracle's argmax at {int((t1[dec] != am[dec]).sum())} decisive positions"
    assert bool(((t1[scored] >= 0) & (t1[scored] < ref_logits.shape[-1])).all())


# ---- 1. the kernel alone ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,V", S.KERNEL_CASES)
def test_score_rows_kernel_alone(engine, M, V):
    xp, tgt = S.kernel_case(M, V, DT[engine.dtype])
    x = xp[:, :V]
    want, want_t1, bar = S.row_logprob(x, tgt), S.row_top1(x, tgt), S.score_rows_bar(x, tgt)
    lp, t1 = engine.score_rows_test(xp, tgt, vocab=V)
    lp2, t12 = engine.score_rows_test(xp, tgt, vocab=V)
    lp, t1 = lp.cpu(), t1.cpu().long()
    ok = S.within(lp, want, bar)
    over = ((lp.double() - want).abs() - bar).nan_to_num(nan=0.0, posinf=0.0, neginf=0.0)
    print(f"score_rows_k M={M} V={V} {engine.dtype}: worst |logprob - fp64| - bar = {float(over.max()):.3g}, largest bar {float(bar.max()):.3g}")
    assert bool(ok.all()), f"rows {ok.logical_not().nonzero().flatten().tolist()[:8]} leave the derived bar"
    assert torch.equal(t1, want_t1)
    ign = tgt == -100
    assert bool((lp[ign] == 0).all()) and bool((t1[ign] == -1).all())                  # exactly (0.0, -1), NaN rows included
    assert torch.equal(lp.view(torch.int32), lp2.cpu().view(torch.int32)) and torch.equal(t1, t12.cpu().long())       # the same bits on a second launch


# ---- 2. end to end on the small configuration -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 2, 5])
def test_score_matches_oracle_all_positions_and_last_eight(engine, cfg, cpu_w, B):
    ids, qf, labels = small_case(cfg, B)
    tol = LOGIT_TOL[engine.dtype]
    ref = oracle_logits(cpu_w, cfg.llama, engine.dtype, ids, qf, (engine.dtype, B))
    lp_a, t1_a, _ = engine.score(ids, qf, labels, want_top1=True)
    check_against_oracle(lp_a, t1_a, ref, labels, tol, f"{engine.dtype} B={B} all positions")
    last = torch.full_like(labels, -100)
    last[:, -8:] = labels[:, -8:]
    lp_b, t1_b, _ = engine.score(ids, qf, last, want_top1=True)
    want_b = S.token_logprobs(ref, last)
    assert float((lp_b.double().cpu() - want_b).abs().max()) <= 2 * tol
    assert bool((lp_b[:, :-8] == 0).all()) and bool((t1_b[:, :-8] == -1).all())
    assert float((lp_a[:, -8:] - lp_b[:, -8:]).abs().max()) <= 2 * tol                 # 8 B rows may take another lm_head kernel than all of them
    scored, dec, am = decisive(ref, last, tol)
    assert torch.equal(t1_b.cpu().long()[dec], am[dec])


# ---- 3. production width: gemm_dma on the lm_head, Npad != vocab --------------------------------------------------------------------------------------
def test_score_at_production_width():
    from radialog_amd.config import LlamaCfg, RaDialogCfg
    from radialog_amd.engine import RdxEngine, synth_getter
    pcfg = RaDialogCfg(llama=LlamaCfg(layers=1, qformer_dim=192))
    assert pcfg.llama.vocab % 16 != 0
    w = synth.make_weights(synth.llama_specs(pcfg.llama, lora=True))
    B, T, dtype = 2, 96, "f16"
    tol = PROD_TOL[dtype] * 1 ** 0.5
    ids = synth.synth_prompt_ids(B, T, vocab=pcfg.llama.vocab, img_offset=6, pad_rows=False, seed=51)
    ids[1] = torch.cat([torch.zeros(3, dtype=torch.long), ids[1, : T - 3]])
    qf = synth.synth("t.score.qfp", (B, 32, pcfg.llama.qformer_dim), -1.0, 1.0)
    labels = labels_of(ids)
    ref = oracle_logits(w, pcfg.llama, dtype, ids, qf, ("prod", dtype))
    del w
    eng = RdxEngine(pcfg, dtype=dtype, device=0, max_batch=B, max_len=T, lora=True, vision=False)
    try:
        eng.load_weights(synth_getter(pcfg, eng.device, lora=True), vision=False)
        lp, t1, _ = eng.score(ids, qf, labels, want_top1=True)
        check_against_oracle(lp, t1, ref, labels, tol, "production width f16 B=2 T=96")
    finally:
        eng.close()
        _REF.pop(("prod", dtype), None)


# ---- 4. chunking ----------------------------------------------------------------------------------------------------------------------------------
def test_score_chunks_agree(engine, cfg, cpu_w):
    B = 5
    ids, qf, labels = small_case(cfg, B)
    assert int((labels[:, 1:] != -100).sum()) == 275                                   # several chunks of 64 and a ragged last one
    tol = LOGIT_TOL[engine.dtype]
    ref = oracle_logits(cpu_w, cfg.llama, engine.dtype, ids, qf, (engine.dtype, B))
    lp_d, t1_d, _ = engine.score(ids, qf, labels, want_top1=True)
    engine.set_option("score_chunk", 64)
    try:
        lp_c, t1_c, _ = engine.score(ids, qf, labels, want_top1=True)
    finally:
        engine.set_option("score_chunk", 2048)
    check_against_oracle(lp_c, t1_c, ref, labels, tol, f"{engine.dtype} chunk 64")
    check_against_oracle(lp_d, t1_d, ref, labels, tol, f"{engine.dtype} default chunk")
    assert float((lp_c - lp_d).abs().max()) <= 2 * tol
    with pytest.raises(Exception, match="score_chunk"):
        engine.set_option("score_chunk", -1)


# ---- 5. agreement with prefill + teacher-forced decode steps ----------------------------------------------------------------------------------------
def test_score_agrees_with_prefill_and_forced_decode(engine, cfg):
    B, N = 2, 8
    ids, qf, _ = small_case(cfg, B)
    g = torch.Generator().manual_seed(9)
    toks = torch.randint(3, 31999, (B, N), generator=g)
    rows = []
    _, lg = engine.prefill(ids, qf, max_new=N + 1, eos_id=-1)
    rows.append(lg.cpu())
    for s in range(1, N):
        _, lg = engine.decode_step(input_ids=toks[:, s - 1])
        rows.append(lg.cpu())
    stepwise = torch.stack([S.row_logprob(rows[s], toks[:, s]) for s in range(N)], dim=1)          # [B, N] float64
    full = torch.cat([ids, toks], dim=1)
    labels = torch.full_like(full, -100)
    labels[:, -N:] = toks
    lp, _, _ = engine.score(full, qf, labels)
    err = (lp[:, -N:].double().cpu() - stepwise).abs()
    print(f"score vs prefill + forced decode {engine.dtype}: worst difference {float(err.max()):.4g}")
    assert float(err.max()) <= 2 * LOGIT_TOL[engine.dtype]


# ---- 6. state ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rules", [None, (1.3, 2, 0)])
def test_state_after_score(engine, cfg, rules):
    from radialog_amd.engine import RdxEngine, synth_getter
    B = 2
    ids, qf, labels = small_case(cfg, B)
    if rules is not None:
        engine.set_logits_rules(rules)
    lp1, t11, lg1 = engine.score(ids, qf, labels, want_top1=True, want_logits=True)
    lp2, t12, lg2 = engine.score(ids, qf, labels, want_top1=True, want_logits=True)
    assert torch.equal(lp1.view(torch.int32), lp2.view(torch.int32)) and torch.equal(t11, t12)
    valid = ids.ne(0).to(lg1.device)
    assert torch.equal(lg1.view(torch.int16)[valid], lg2.view(torch.int16)[valid])
    # no conversation behind a scoring pass: single steps and the append calls refuse
    assert engine.lib.rdx_decode_step(engine.ctx, None) == -1
    toks = torch.zeros(B, 4, dtype=torch.int32, device=engine.device)
    tail = ids[:, -4:].to(engine.device, torch.int32).contiguous()
    n = C.c_int(0)
    assert engine.lib.rdx_generate_append(engine.ctx, C.c_void_p(tail.data_ptr()), B, 4, 8, 4, -1, 0, C.c_void_p(toks.data_ptr()), None, C.byref(n), 1) == -1
    # ... and the next generate is the one of an engine that never scored
    N = 6
    toks_a, sc_a, n_a = engine.generate(ids, qf, max_new=N, eos_id=-1, output_scores=True, logits_rules=rules)
    toks_a, sc_a = toks_a.clone(), sc_a.clone()
    fresh = RdxEngine(cfg, dtype=engine.dtype, device=0, max_batch=5, max_len=128, lora=True, vision=False)
    try:
        fresh.load_weights(synth_getter(cfg, fresh.device, lora=True), vision=False)
        toks_f, sc_f, n_f = fresh.generate(ids, qf, max_new=N, eos_id=-1, output_scores=True, logits_rules=rules)
        assert n_a == n_f and torch.equal(toks_a, toks_f)
        assert torch.equal(sc_a.view(torch.int16), sc_f.view(torch.int16))
    finally:
        fresh.close()
        engine.set_logits_rules(None)


# ---- 7. model level ----------------------------------------------------------------------------------------------------------------------------------
def test_model_forward_loss_and_logits(cfg, cpu_w):
    from radialog_amd.modeling_llama_imgemb import LlamaForCausalLM, PeftModelForCausalLM
    dtype, B = "f16", 2
    tol = LOGIT_TOL[dtype]
    ids, qf, labels = small_case(cfg, B)
    ref = oracle_logits(cpu_w, cfg.llama, dtype, ids, qf, (dtype, B))
    lm = LlamaForCausalLM.from_pretrained(None, torch_dtype=torch.float16, synthetic=True, cfg=cfg.llama, max_batch=B, max_len=64)
    try:
        kw = dict(input_ids=ids, attention_mask=ids.ne(0).long(), labels=labels, qformer_embs=qf)
        out = lm(**kw)
        want = float(S.loss(ref, labels))
        print(f"model loss {float(out.loss):.6f}, oracle {want:.6f}")
        assert out.loss.dtype == torch.float32 and abs(float(out.loss) - want) <= 2 * tol
        assert tuple(out.logits.shape) == (B, T_SMALL, cfg.llama.vocab)
        valid = ids.ne(0)
        err = (out.logits.float().cpu() - ref.float()).abs().amax(dim=-1)[valid]
        assert float(err.max()) < tol, f"logits differ by {float(err.max()):.4g}"
        assert float((out.token_logprobs.double().cpu() - S.token_logprobs(ref, labels)).abs().max()) <= 2 * tol
        cheap = lm(return_logits=False, **kw)
        assert cheap.logits is None and torch.equal(cheap.loss.view(torch.int32), out.loss.view(torch.int32))
        tup = lm.forward(return_dict=False, **kw)
        assert isinstance(tup, tuple) and torch.equal(tup[0], out.loss) and tuple(tup[1].shape) == tuple(out.logits.shape)
        assert torch.equal(PeftModelForCausalLM(lm)(**kw).loss, out.loss)
        only = lm(input_ids=ids, attention_mask=ids.ne(0).long(), qformer_embs=qf)
        assert only.loss is None and torch.equal(only.logits.view(torch.int16)[valid.to(only.logits.device)], out.logits.view(torch.int16)[valid.to(out.logits.device)])
    finally:
        lm.close()


# ---- 8. refusals -------------------------------------------------------------------------------------------------------------------------------------
def _raw_score(engine, ids, labels, lp, t1):
    ids32 = ids.to(engine.device, torch.int32).contiguous()
    lab = labels.to("cpu", torch.int32).contiguous()
    B, T = ids.shape
    torch.cuda.synchronize()
    rc = engine.lib.rdx_score(engine.ctx, C.c_void_p(ids32.data_ptr()), None, B, T, None, C.c_void_p(lab.data_ptr()), C.c_void_p(lp.data_ptr()),
                              C.c_void_p(t1.data_ptr()), None)
    torch.cuda.synchronize()
    return rc, (engine.lib.rdx_last_error(engine.ctx) or b"").decode()


def test_refusals_write_nothing(engine, cfg):
    from radialog_amd import _lib
    from radialog_amd.engine import RdxEngine, synth_getter
    B, T = 2, 40
    ids = synth.synth_prompt_ids(B, T, vocab=cfg.llama.vocab, img_offset=4, seed=3)
    lp = torch.full((B, 200), 7.5, dtype=torch.float32, device=engine.device)
    t1 = torch.full((B, 200), 77, dtype=torch.int32, device=engine.device)
    bad = ids.clone()
    bad[1, 7] = cfg.llama.vocab                                                         # 32001
    rc, msg = _raw_score(engine, ids, bad, lp, t1)
    assert rc == -1 and "label" in msg and str(cfg.llama.vocab) in msg
    long_ids = synth.synth_prompt_ids(1, engine.max_len + 1, vocab=cfg.llama.vocab, img_offset=4, seed=3)
    rc, msg = _raw_score(engine, long_ids, long_ids, lp, t1)
    assert rc == -1 and "max_len" in msg
    assert bool((lp == 7.5).all()) and bool((t1 == 77).all())
    with pytest.raises(_lib.RdxError, match="label"):
        engine.score(ids, None, bad)
    f8 = RdxEngine(cfg, dtype=engine.dtype, device=0, max_batch=B, max_len=64, lora=True, vision=False, weights_fp8=True)
    try:
        f8.load_weights(synth_getter(cfg, f8.device, lora=True), vision=False)
        rc, msg = _raw_score(f8, ids, ids, lp, t1)
        assert rc == -1 and "fp8" in msg and "quantisation convention" in msg
        assert bool((lp == 7.5).all()) and bool((t1 == 77).all())
        with pytest.raises(_lib.RdxError, match="fp8"):
            f8.score(ids, None, ids)
    finally:
        f8.close()
