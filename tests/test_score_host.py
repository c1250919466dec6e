"""Scoring given tokens, host side: the float64 restatement (tests/_score.py) against torch's cross-entropy and the reference's shift formula, the
derived bar of the kernel test against an fp32 emulation of the kernel's reduction order and against planted faults, LlamaForCausalLM.forward's
validation and the labels a legal call hands the engine, and the new symbols of the two libraries."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import _score as S

DTYPES = {"f16": torch.float16, "bf16": torch.bfloat16}


# ---- the restatement --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_restatement_is_torch_cross_entropy_with_the_reference_shift(dt):
    g = torch.Generator().manual_seed(5)
    B, T, V = 3, 9, 37
    logits = (torch.randn(B, T, V, generator=g) * 4).to(DTYPES[dt])
    labels = torch.randint(0, V, (B, T), generator=g)
    labels[0, :4] = -100
    labels[1, ::2] = -100
    labels[2, -1] = -100
    lp = S.token_logprobs(logits, labels)
    # per token: cross_entropy(reduction="none") on the shifted pair, ignore_index rows give 0
    ce = F.cross_entropy(logits.double()[:, :-1].reshape(-1, V), labels[:, 1:].reshape(-1), ignore_index=-100, reduction="none").view(B, T - 1)
    assert torch.allclose(-lp[:, 1:], ce, rtol=0, atol=1e-12) and bool((lp[:, 0] == 0).all())
    assert bool((lp[:, 1:][labels[:, 1:] == -100] == 0).all())
    # the reference's formula (modeling_llama_imgemb.py:771-781), restated in float64
    shift_logits = logits.double()[..., :-1, :].contiguous().view(-1, V)
    shift_labels = labels[..., 1:].contiguous().view(-1)
    want = torch.nn.CrossEntropyLoss()(shift_logits, shift_labels)
    assert abs(float(S.loss(logits, labels)) - float(want)) < 1e-12


def test_hand_cases_at_vocab_5():
    x = torch.tensor([[1.0, 3.0, 3.0, 0.0, 3.0],                        # a three-way tie: the lowest index
                      [float("-inf"), 2.0, float("-inf"), 2.0, 0.0],    # -inf entries drop out of the sum
                      [0.0, 0.0, 0.0, 0.0, 0.0]], dtype=torch.float16)
    tgt = torch.tensor([2, 0, -100])
    assert S.row_top1(x, tgt).tolist() == [1, 1, -1]
    lp = S.row_logprob(x, tgt)
    import math
    assert abs(float(lp[0]) - (3.0 - math.log(math.exp(1) + 3 * math.exp(3) + 1))) < 1e-12
    assert float(lp[1]) == float("-inf") and float(lp[2]) == 0.0
    assert abs(float(S.row_logprob(x[1:2], torch.tensor([3]))[0]) - (2.0 - math.log(2 * math.exp(2) + 1))) < 1e-12
    # the sequence form: position 0 is never scored, and nothing counted gives NaN like CrossEntropyLoss
    logits = x.view(1, 3, 5)
    labels = torch.tensor([[4, 2, 0]])
    lp = S.token_logprobs(logits, labels)
    assert float(lp[0, 0]) == 0.0 and abs(float(lp[0, 1]) - float(S.row_logprob(x[0:1], torch.tensor([2]))[0])) < 1e-15
    assert float(lp[0, 2]) == float("-inf")
    none = torch.full((1, 3), -100)
    assert torch.isnan(S.loss(logits, none)) and torch.isnan(torch.nn.CrossEntropyLoss()(logits.double()[0, :-1], none[0, 1:]))
    assert bool((S.token_logprobs(logits, none) == 0).all())


# ---- the kernel test's bar: the fp32 emulation stays inside it, every planted fault leaves it ------------------------------------------------------
@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("M,V", S.KERNEL_CASES)
def test_bar_holds_the_emulated_kernel_and_catches_planted_faults(M, V, dt):
    """On the GPU test's own inputs (tests/test_gpu_score.py takes them from _score.kernel_case): an fp32 emulation of score_rows_k's reduction
    order is within the derived bar of the float64 restatement on EVERY row with the exact top1, and each planted fault is caught by the case --
    some row leaves the bar or gets another top1. "pads" and "maxld" exist only where the row has pad columns (ld > vocab)."""
    xp, tgt = S.kernel_case(M, V, DTYPES[dt])
    ld = xp.shape[1]
    assert ld % 64 == 0 and ld >= V and (ld == V or bool(torch.isnan(xp[:, V:].float()).any()))
    x = xp[:, :V]
    want, want_t1, bar = S.row_logprob(x, tgt), S.row_top1(x, tgt), S.score_rows_bar(x, tgt)
    scored = (tgt != -100) & torch.isfinite(want)                                  # a -inf target is -inf exactly: bar 0
    assert float(bar.max()) < 2e-2 and float(bar[scored].min()) > 0                # u (2 x 65504 + ...) at the most
    lp, t1 = S.emulate_kernel(xp, tgt, V)
    assert bool(S.within(lp, want, bar).all()), f"emulation leaves the bar by {float(((lp.double() - want).abs() - bar).nan_to_num().max()):.3g}"
    assert torch.equal(t1, want_t1)
    for fault in ("pads", "drop", "label", "maxld"):
        if fault in ("pads", "maxld") and ld == V:
            continue
        flp, ft1 = S.emulate_kernel(xp, tgt, V, fault=fault)
        caught = (~S.within(flp, want, bar)) | (ft1 != want_t1)
        assert bool(caught.any()), f"planted fault {fault!r} passes M={M} V={V} {dt}"


# ---- LlamaForCausalLM.forward: validation before an engine exists, and what a legal call hands the engine -----------------------------------------
class _Reached(Exception):
    pass


def _model():
    from radialog_amd.modeling_llama_imgemb import LlamaForCausalLM
    return LlamaForCausalLM.from_pretrained(None, torch_dtype=torch.float16, synthetic=True)


def test_forward_refuses_bad_arguments_before_building_an_engine(monkeypatch):
    lm = _model()
    monkeypatch.setattr(lm, "_ensure_engine", lambda: (_ for _ in ()).throw(_Reached()))
    ids = torch.ones(2, 40, dtype=torch.long)
    ok = torch.full((2, 40), 7)
    V = lm.lcfg.vocab
    bad_hi, bad_neg = ok.clone(), ok.clone()
    bad_hi[1, 3] = V
    bad_neg[0, 5] = -1
    for kw in (dict(labels=torch.ones(2, 39, dtype=torch.long)), dict(labels=torch.ones(3, 40, dtype=torch.long)), dict(labels=bad_hi), dict(labels=bad_neg),
               dict(labels=ok, past_key_values=[()]), dict(labels=ok, inputs_embeds=torch.zeros(2, 40, 8))):
        with pytest.raises(ValueError):
            lm(input_ids=ids, **kw)
        with pytest.raises(ValueError):
            lm.forward(input_ids=ids, **kw)
    with pytest.raises(_Reached):
        lm(input_ids=ids, labels=ok)
    with pytest.raises(_Reached):
        lm(input_ids=ids)                              # labels=None: the logits alone
    edge = ok.clone()
    edge[0, 0], edge[1, 1] = V - 1, -100
    with pytest.raises(_Reached):
        lm(input_ids=ids, labels=edge)


def test_legal_call_reaches_the_engine_with_shifted_masked_labels(monkeypatch):
    from radialog_amd.modeling_llama_imgemb import PeftModelForCausalLM
    lm = _model()
    seen = {}
    B, T, V = 2, 6, lm.lcfg.vocab
    lp = torch.zeros(B, T)
    lp[0, 1:] = torch.tensor([-1.0, -2.0, -3.0, -4.0, -5.0])
    lp[1, 3] = -0.5

    class FakeEngine:
        def score(self, ids, embs, labels, mask=None, want_top1=False, want_logits=False):
            seen.update(ids=ids, embs=embs, labels=labels.clone(), mask=mask, want_top1=want_top1, want_logits=want_logits)
            return lp.clone(), None, (torch.zeros(B, T, V, dtype=torch.float16) if want_logits else None)

    monkeypatch.setattr(lm, "_ensure_engine", lambda: setattr(lm, "_engine", FakeEngine()))
    ids = torch.arange(B * T).view(B, T) + 5
    labels = ids.clone()
    labels[1] = -100
    labels[1, 3] = 9
    labels[0, 0] = 11                                  # position 0 has no predecessor: handed over, never counted
    out = lm(input_ids=ids, labels=labels)
    assert seen["labels"].dtype == torch.int32 and torch.equal(seen["labels"].long(), labels) and seen["want_logits"] is True
    assert torch.equal(seen["mask"], torch.ones(B, T, dtype=torch.int32))       # attention_mask=None attends everything, as the reference
    assert out.logits.shape == (B, T, V) and torch.equal(out.token_logprobs, lp)
    assert out.loss.dtype == torch.float32 and out.loss.dim() == 0
    assert abs(float(out.loss) - (1 + 2 + 3 + 4 + 5 + 0.5) / 6) < 1e-6          # the mean over labels[:, 1:] != -100
    cheap = lm(input_ids=ids, labels=labels, return_logits=False, attention_mask=torch.ones(B, T, dtype=torch.long))
    assert seen["want_logits"] is False and cheap.logits is None and torch.equal(cheap.loss, out.loss)
    tup = lm(input_ids=ids, labels=labels, return_dict=False)
    assert isinstance(tup, tuple) and len(tup) == 2 and torch.equal(tup[0], out.loss) and tup[1].shape == (B, T, V)
    only = lm(input_ids=ids)
    assert only.loss is None and only.logits.shape == (B, T, V) and bool((seen["labels"] == -100).all())
    assert lm(input_ids=ids, return_dict=False)[0].shape == (B, T, V)
    nothing = lm(input_ids=ids, labels=torch.full((B, T), -100))
    assert torch.isnan(nothing.loss)
    # the peft wrapper delegates __call__ and forward as it delegates generate
    peft = PeftModelForCausalLM(lm)
    assert torch.equal(peft(input_ids=ids, labels=labels).loss, out.loss) and torch.equal(peft.forward(input_ids=ids, labels=labels).loss, out.loss)


def test_engine_score_keeps_its_contract_without_a_gpu():
    """RdxEngine.score refuses a labels tensor of another shape before it touches the library, and drops the cached conversation."""
    import inspect
    import types
    from radialog_amd.engine import RdxEngine
    eng = types.SimpleNamespace(device="cpu", _conv={"seq": None})
    with pytest.raises(ValueError):
        RdxEngine.score(eng, torch.ones(2, 8, dtype=torch.long), None, torch.ones(2, 7, dtype=torch.long))
    params = inspect.signature(RdxEngine.score).parameters
    assert list(params)[1:] == ["ids", "qformer_embs", "labels", "mask", "want_top1", "want_logits"]
    assert "self._conv = None" in inspect.getsource(RdxEngine.score)


# ---- the libraries ---------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_exported_and_the_hook_only_from_the_hooks_library():
    from radialog_amd import _lib, build
    raw = C.CDLL(_lib.LIB_PATH, mode=C.RTLD_GLOBAL)
    hooks = C.CDLL(_lib.HOOKS_PATH, mode=C.RTLD_GLOBAL)
    assert hasattr(raw, "rdx_score") and not hasattr(raw, "rdx_score_rows_test")
    assert hasattr(hooks, "rdx_score_rows_test")
    assert "rdx_score" in _lib.SYMBOLS and "rdx_score_rows_test" in _lib.DEC_HOOK_SYMBOLS
    assert len(_lib.SYMBOLS["rdx_score"][1]) == 10 and len(_lib.DEC_HOOK_SYMBOLS["rdx_score_rows_test"][1]) == 8
    assert "score.hip" in build.SOURCES and "score.hip" not in build.HOOK_SOURCES
    bound = _lib.load()
    assert list(bound.rdx_score.argtypes) == _lib.SYMBOLS["rdx_score"][1]
