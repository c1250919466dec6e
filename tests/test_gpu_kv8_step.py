"""The engine on the fp8 KV cache (RdxEngine(kv_fp8=True); the format: radialog_amd/kv8.py). kv8 is a storage format: engine A (kv_fp8) must compute, bit for
bit, what a plain twin B computes on a cache that holds A's stored values -- the same weights, dtype and sizes, created under RDX_FUSE_AO=0 so that at 1-2
rows both run the generic family (A never runs the fused attention + o_proj launch), and launched under the same "att_tp".

  prompt      A's logits and token 0 are B's bits (the prompt's own attention reads its unquantised K / V), and A's codes and exponents of every layer are
              kv8.quant of the rows B's prompt wrote, byte for byte;
  every step  B's caches are overwritten with A.kv_read (rdx_kv_write_test), both engines step on the same ids: the logits are bit-identical, and the code
              row and exponent A appended are kv8.quant of the row B appended (a zero K code may have either sign: the kernels' RoPE zeros).
Small config, max_len 128, prompt 72 (row 1 left-padded), 6 teacher-forced steps, rows 1 / 3 / 12 / 17 x RDX_ATT_TP unset / 1 / 2; one production-width
leg (1 layer, 40 rows: the row-block families, bf16 and fp8 weights)."""
import ctypes
import os

import pytest
import torch

from radialog_amd import kv8, synth
from radialog_amd.config import LlamaCfg, RaDialogCfg, small_cfg

pytestmark = pytest.mark.gpu

T_PROMPT, STEPS, MAX_LEN, MAX_B = 72, 6, 128, 17


def _pair(cfg, dtype, max_batch, fp8=False):
    """(A, B): the kv_fp8 engine and its plain twin. Both are created with the fused attention + o_proj launch off."""
    from radialog_amd.engine import RdxEngine, synth_getter
    old = os.environ.get("RDX_FUSE_AO")
    os.environ["RDX_FUSE_AO"] = "0"
    try:
        a = RdxEngine(cfg, dtype=dtype, device=0, max_batch=max_batch, max_len=MAX_LEN, lora=True, vision=False, weights_fp8=fp8, kv_fp8=True)
        b = RdxEngine(cfg, dtype=dtype, device=0, max_batch=max_batch, max_len=MAX_LEN, lora=True, vision=False, weights_fp8=fp8)
    finally:
        if old is None:
            del os.environ["RDX_FUSE_AO"]
        else:
            os.environ["RDX_FUSE_AO"] = old
    for e in (a, b):
        e.load_weights(synth_getter(cfg, e.device, lora=True), vision=False)
    return a, b


@pytest.fixture(scope="module", params=["bf16", "f16"])
def pair(request):
    cfg = small_cfg()
    a, b = _pair(cfg, request.param, MAX_B)
    yield cfg, a, b
    a.close()
    b.close()


def _inputs(cfg, B, seed=43):
    ids = synth.synth_prompt_ids(B, T_PROMPT, vocab=cfg.llama.vocab, img_offset=6, pad_rows=False, seed=seed)
    if B > 1:
        ids[1] = torch.cat([torch.zeros(3, dtype=torch.long), ids[1, : T_PROMPT - 3]])
    qf = synth.synth("t.kv8.qf", (B, 32, cfg.llama.qformer_dim), -1.0, 1.0)
    return ids, qf


def _variant(monkeypatch, tp, *engines):
    """The live engines take the variant as their option "att_tp" (0 too: they are shared); engines created from here on find no RDX_ATT_TP."""
    monkeypatch.delenv("RDX_ATT_TP", raising=False)
    for e in engines:
        e.set_option("att_tp", tp)


def _bits(t):
    return t.cpu().contiguous().view(torch.int16)


def _zero_code(c):
    return (c & 0x7f) == 0


def _twin_run(cfg, a, b, B, steps, what):
    layers = cfg.llama.layers
    ids, qf = _inputs(cfg, B)
    ta, la = a.prefill(ids, qf, max_new=steps + 1, eos_id=-1)
    tb, lb = b.prefill(ids, qf, max_new=steps + 1, eos_id=-1)
    assert torch.equal(_bits(la), _bits(lb)) and torch.equal(ta[:, 0].cpu(), tb[:, 0].cpu()), f"{what}: the prompt's logits / token 0 differ from the plain engine's"
    for l in range(layers):
        for which in (0, 1):
            codes, exps = a.kv_read_codes(l, which, B)
            wc, we = kv8.quant(b.kv_read(l, which, B).cpu()[:, :, :T_PROMPT])
            got = codes.cpu()[:, :, :T_PROMPT]
            diff = (got != wc) & ~(_zero_code(got) & _zero_code(wc) & (which == 0))
            assert not bool(diff.any()) and torch.equal(exps.cpu()[:, :, :T_PROMPT], we), f"{what}: layer {l} {'KV'[which]}: the prompt's codes / exponents are not kv8.quant of the plain rows"
            assert torch.equal(_bits(a.kv_read(l, which, B)), _bits(kv8.dequant(codes.cpu(), exps.cpu(), dtype=a.tdtype))), f"{what}: kv_read is not dequant(kv_read_codes)"
    g = torch.Generator().manual_seed(B)
    for s in range(steps):
        for l in range(layers):
            for which in (0, 1):
                b.kv_write_test(l, which, a.kv_read(l, which, B))
        forced = torch.randint(3, cfg.llama.vocab - 1, (B,), generator=g)
        _, la = a.decode_step(input_ids=forced)
        _, lb = b.decode_step(input_ids=forced)
        assert torch.equal(_bits(la), _bits(lb)), f"{what}: step {s}: {int((_bits(la) != _bits(lb)).sum())} logits differ from the plain twin on the stored values"
        pos = T_PROMPT + s
        for l in range(layers):
            for which in (0, 1):
                codes, exps = a.kv_read_codes(l, which, B)
                wc, we = kv8.quant(b.kv_read(l, which, B).cpu()[:, :, pos])
                got = codes.cpu()[:, :, pos]
                diff = (got != wc) & ~(_zero_code(got) & _zero_code(wc) & (which == 0))
                assert not bool(diff.any()) and torch.equal(exps.cpu()[:, :, pos], we), f"{what}: step {s} layer {l} {'KV'[which]}: the appended row is not kv8.quant of the plain one"


@pytest.mark.parametrize("tp", [0, 1, 2])
@pytest.mark.parametrize("B", [1, 3, 12, 17])
def test_steps_equal_the_plain_twin_on_the_stored_values(pair, monkeypatch, B, tp):
    cfg, a, b = pair
    _variant(monkeypatch, tp, a, b)
    _twin_run(cfg, a, b, B, STEPS, f"{a.dtype}, {B} rows, RDX_ATT_TP {tp}")


def test_generate_with_and_without_the_graph_and_the_flag_is_not_ignored(pair, monkeypatch):
    cfg, a, b = pair
    _variant(monkeypatch, 0, a, b)
    ids, qf = _inputs(cfg, 3)
    out = []
    for use_graph in (False, True):
        toks, scores, n = a.generate(ids, qf, max_new=STEPS + 1, eos_id=-1, output_scores=True, use_graph=use_graph)
        assert n == STEPS + 1
        out.append((toks.cpu().clone(), _bits(scores).clone()))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1]), "the step graph and the eager steps give different tokens / scores"
    tb, sb, _ = b.generate(ids, qf, max_new=STEPS + 1, eos_id=-1, output_scores=True)
    sb = _bits(sb)
    assert torch.equal(out[0][1][0], sb[0]), "token 0's scores are the plain engine's"
    assert not torch.equal(out[0][1][1:], sb[1:]), "the fp8 cache changed no logit within 6 steps: the option is ignored"


def test_score_bytes_and_refusals(pair, monkeypatch):
    from radialog_amd._lib import RdxError
    cfg, a, b = pair
    _variant(monkeypatch, 0, a, b)
    ids, qf = _inputs(cfg, 3)
    labels = ids.clone()
    labels[:, :40] = -100
    la, lb = a.score(ids, qf, labels)[0], b.score(ids, qf, labels)[0]
    assert torch.equal(la.cpu().view(torch.int32), lb.cpu().view(torch.int32)), "rdx_score differs from the plain engine's bits"
    l = cfg.llama
    plain = 2 * l.layers * MAX_B * l.heads * MAX_LEN * 128 * 2
    assert b.kv_cache_bytes() == plain
    assert a.kv_cache_bytes() == plain // 2 + 2 * l.layers * MAX_B * l.heads * MAX_LEN == kv8.cache_bytes(l.layers, MAX_B, l.heads, MAX_LEN)
    with pytest.raises(RdxError, match="kv_fp8"):
        a.set_option("kv_fp8", 0)                                      # after rdx_finalize_weights
    with pytest.raises(RdxError, match="kv_fp8"):
        b.set_option("kv_fp8", 1)
    with pytest.raises(RdxError, match="kv_fp8"):
        b.kv_read_codes(0, 0, 1)
    with pytest.raises(RdxError, match="kv_fp8"):
        a.kv_write_test(0, 0, torch.zeros(1, l.heads, MAX_LEN, 128))
    a.generate(ids, qf, max_new=2, eos_id=-1)
    with pytest.raises(RdxError, match="kv_fp8"):
        a.beam_search(ids[:1], qf[:1], 2, max_new=2)
    with pytest.raises(ValueError, match="kv_fp8"):
        a.generate(ids, qf, max_new=2, eos_id=-1, reuse_prefix=True)
    tail = ids[:, -8:].to(a.device, torch.int32).contiguous()
    toks = torch.zeros(3, 2, dtype=torch.int32, device=a.device)
    n = ctypes.c_int(0)
    torch.cuda.synchronize()
    assert a.lib.rdx_prefill_append(a.ctx, tail.data_ptr(), 3, 8, T_PROMPT - 8, 2, -1, 0, toks.data_ptr(), None) == -1 and "kv_fp8" in a._last_error()
    assert a.lib.rdx_generate_append(a.ctx, tail.data_ptr(), 3, 8, T_PROMPT - 8, 2, -1, 0, toks.data_ptr(), None, ctypes.byref(n), 1) == -1 and "kv_fp8" in a._last_error()
    with pytest.raises(RdxError, match="kv_fp8"):
        with a.row_session(2, 1, 4, eos_id=-1):
            pass
    # the attention timer works on the fp8 cache: it appends the row of the current slot again and again (the same bytes) and touches no cached position
    a.prefill(ids, qf, max_new=4, eos_id=-1)
    before = a.kv_read_codes(0, 0, 3)
    assert a.time_unit(6, 2) > 0
    once = a.kv_read_codes(0, 0, 3)
    assert a.time_unit(6, 3) > 0
    again = a.kv_read_codes(0, 0, 3)
    assert torch.equal(once[0], again[0]) and torch.equal(once[1], again[1])
    assert torch.equal(before[0][:, :, :T_PROMPT], once[0][:, :, :T_PROMPT]) and torch.equal(before[1][:, :, :T_PROMPT], once[1][:, :, :T_PROMPT])
    assert torch.equal(before[0][:, :, T_PROMPT + 1:], once[0][:, :, T_PROMPT + 1:]) and bool(once[0][:, :, T_PROMPT].any())


@pytest.mark.parametrize("fp8", [False, True])
def test_production_width_row_blocks(monkeypatch, fp8):
    """1 layer at the Vicuna-7B widths, 40 rows: the row-block families (attention writes ACT_TILES32, or ACT_BLK64 with fp8 weights), 3 steps."""
    _variant(monkeypatch, 0)
    cfg = RaDialogCfg(llama=LlamaCfg(layers=1, qformer_dim=192))
    a, b = _pair(cfg, "bf16", 40, fp8=fp8)
    try:
        _twin_run(cfg, a, b, 40, 3, f"production width, 40 rows, fp8 weights {fp8}")
    finally:
        a.close()
        b.close()
