"""Logits rules of the greedy search (repetition penalty, n-gram ban, min-new-tokens), host side: the plain-torch restatement the GPU tests
compare select_step_k with (tests/_logits_rules.py) against hand-computed cases and against the installed transformers' processors, and the
argument checks of LlamaForCausalLM.generate, which run before any engine exists."""
import numpy as np
import pytest
import torch

import _logits_rules as LR

INF = float("inf")


def _bits(t):
    return t.view(torch.int16)


def _row(vals, dtype):
    return torch.tensor([vals], dtype=dtype)


# ---- the restatement against hand-computed cases -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_penalty_half_is_exact_doubling_and_halving(dtype):
    """p = 0.5 is exact in both dtypes: positive logits double (x / 0.5), negative ones halve (x * 0.5), zeros keep their sign, tokens outside
    the history stay."""
    x = _row([3.0, -3.0, 0.0, -0.0, 5.0, -7.0], dtype)
    out, tok = LR.apply_rules(x, [[0, 1, 2, 3]], [0], (0.5, 0, 0))
    want = _row([6.0, -1.5, 0.0, -0.0, 5.0, -7.0], dtype)
    assert torch.equal(_bits(out), _bits(want))
    assert int(tok[0]) == 0
    assert torch.equal(_bits(x), _bits(_row([3.0, -3.0, 0.0, -0.0, 5.0, -7.0], dtype)))        # the input is left alone


def test_penalty_fp16_values_zeros_and_subnormals_against_float32_arithmetic():
    """A positive, a negative, +0, -0 and fp16 subnormals under p = 1.3 and p = 0.5: the expected bits come from numpy's float32 arithmetic and its
    round-to-nearest-even float32 -> float16 conversion, and three of them are spelled out."""
    sub = 2.0 ** -24                                    # the smallest fp16 subnormal
    vals = [2.6, -2.6, 0.0, -0.0, sub, 3 * sub, -3 * sub, 1000 * sub, -sub]
    x = _row(vals, torch.float16)
    for p in (1.3, 0.5):
        out, _ = LR.apply_rules(x, [list(range(len(vals)))], [0], (p, 0, 0))
        x32 = x[0].numpy().astype(np.float32)
        p32 = np.float32(p)
        want = np.where(x32 < 0, x32 * p32, x32 / p32).astype(np.float16)
        assert np.array_equal(out[0].numpy().view(np.int16), want.view(np.int16)), p
        assert np.signbit(out[0].numpy()[3]) and not np.signbit(out[0].numpy()[2])             # -0 stays -0, +0 stays +0
    out13, _ = LR.apply_rules(x, [list(range(len(vals)))], [0], (1.3, 0, 0))
    assert float(out13[0, 4]) == sub                    # 1 / 1.3 = 0.77 ulp -> 1 ulp
    assert float(out13[0, 5]) == 2 * sub                # 3 / 1.3 = 2.31 ulp -> 2 ulp
    assert float(out13[0, 6]) == -4 * sub               # -3 * 1.3 = -3.9 ulp -> -4 ulp
    out05, _ = LR.apply_rules(x, [list(range(len(vals)))], [0], (0.5, 0, 0))
    assert float(out05[0, 4]) == 2 * sub and float(out05[0, 8]) == 0.0 and np.signbit(out05[0].numpy()[8])      # -1 ulp * 0.5 ties to even: -0


def test_a_token_that_occurs_three_times_is_penalised_once():
    x = _row([8.0, 1.0, -4.0, 2.0], torch.float16)
    out, _ = LR.apply_rules(x, [[0, 2, 0, 0, 2]], [0], (2.0, 0, 0))
    assert out[0].tolist() == [4.0, 1.0, -8.0, 2.0]


def test_ngram_ban_cases():
    x = torch.zeros(1, 10, dtype=torch.float16)
    banned = lambda hist, n: sorted(torch.nonzero(LR.apply_rules(x, [hist], [0], (1.0, n, 0))[0][0] == -INF).flatten().tolist())   # noqa: E731
    assert banned([1, 2, 3], 5) == []                           # n larger than L + 1 bans nothing
    assert banned([1, 2, 3], 4) == []                           # L + 1 == n: the only 4-gram would be the history + the new token itself
    assert banned([1, 2, 3, 1, 2], 3) == [3]                    # "1 2" was followed by 3
    assert banned([1, 2, 3, 1, 2], 2) == [3]                    # "2" was followed by 3 (the last 2 has no successor yet)
    assert banned([4, 5, 4, 6, 4], 2) == [5, 6]
    assert banned([7, 8, 7], 1) == [7, 8]                       # n = 1: every token of the history
    assert banned([1, 2, 3], 0) == []
    assert banned([], 1) == []
    assert LR.banned_ngram_tokens([1, 2], 3) == []              # L + 1 == n, nothing earlier to match


def test_min_new_tokens_bans_eos_up_to_m_minus_1():
    x = _row([1.0, 5.0, 2.0], torch.bfloat16)
    out, tok = LR.apply_rules(x.repeat(3, 1), [[0]] * 3, [3, 4, 5], (1.0, 0, 5), eos_id=1)
    assert out[0, 1] == -INF and out[1, 1] == -INF and out[2, 1] == 5.0        # generated = m - 1 still banned, generated = m not
    assert tok.tolist() == [2, 2, 1]
    out, tok = LR.apply_rules(x, [[0]], [0], (1.0, 0, 5), eos_id=-1)           # no EOS id: nothing to ban
    assert torch.equal(_bits(out), _bits(x)) and int(tok[0]) == 1


def test_order_and_argmax_ties():
    """Penalty first, then the bans (a banned token is -inf whatever the penalty made of it); ties go to the lowest index, also ties the
    penalty creates and rows that are all -inf."""
    x = _row([4.0, 2.0, 8.0, 4.0], torch.float16)
    out, tok = LR.apply_rules(x, [[2, 2]], [0], (2.0, 1, 0))
    assert out[0].tolist() == [4.0, 2.0, -INF, 4.0] and int(tok[0]) == 0
    out, tok = LR.apply_rules(x, [[2]], [0], (2.0, 0, 0))                      # 8 / 2 = 4: a three-way tie that only exists after the penalty
    assert out[0].tolist() == [4.0, 2.0, 4.0, 4.0] and int(tok[0]) == 0
    assert int(LR.greedy_argmax(torch.full((1, 5), -INF, dtype=torch.bfloat16))[0]) == 0
    assert torch.equal(LR.apply_rules(x, [[0, 1, 2, 3]], [9], LR.NEUTRAL, eos_id=1)[0], x)


# ---- the restatement against the installed transformers ------------------------------------------------------------------------------------
def _random_rows(B, V, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(B, V, generator=g) * 6).to(dtype)
    x[:, ::7] = (torch.randn(B, len(range(0, V, 7)), generator=g) * 1e-6).to(dtype)       # tiny values: subnormal results in fp16
    x[:, 3::11] = (torch.randn(B, len(range(3, V, 11)), generator=g) * 2).to(dtype) * torch.finfo(dtype).tiny       # around the smallest normal, in both dtypes
    return x


@pytest.mark.parametrize("V", [40, 32001])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_restatement_equals_transformers_processors(dtype, V):
    lp = pytest.importorskip("transformers.generation.logits_process")
    g = torch.Generator().manual_seed(V)
    x = _random_rows(4, V, dtype, seed=V + 1)
    lens = [1, 2, 7, 23]
    hists = []
    for L in lens:
        h = torch.randint(0, min(V, 6), (L,), generator=g).tolist()          # few distinct ids: duplicates and repeated n-grams
        h[0] = V - 1
        hists.append(h)
    for b, h in enumerate(hists):
        row, ids = x[b:b + 1], torch.tensor([h], dtype=torch.long)
        for p in (1.3, 0.5):
            want = lp.RepetitionPenaltyLogitsProcessor(p)(ids, row.clone())
            got, _ = LR.apply_rules(row, [h], [0], (p, 0, 0))
            assert torch.equal(_bits(got), _bits(want)), (b, p)
        for n in (1, 2, 3):
            want = lp.NoRepeatNGramLogitsProcessor(n)(ids, row.clone())
            got, _ = LR.apply_rules(row, [h], [0], (1.0, n, 0))
            assert torch.equal(_bits(got), _bits(want)), (b, n)
        T0 = max(len(h) - 2, 0)                                                # the row has generated len(h) - T0 tokens
        for m in (len(h) - T0, len(h) - T0 + 1):
            want = lp.MinNewTokensLengthLogitsProcessor(T0, m, 3)(ids, row.clone())
            got, _ = LR.apply_rules(row, [h], [len(h) - T0], (1.0, 0, m), eos_id=3)
            assert torch.equal(_bits(got), _bits(want)), (b, m)
        # all three chained in transformers' order
        want = row.clone()
        for proc in (lp.RepetitionPenaltyLogitsProcessor(1.3), lp.NoRepeatNGramLogitsProcessor(2), lp.MinNewTokensLengthLogitsProcessor(T0, 5, 3)):
            want = proc(ids, want)
        got, tok = LR.apply_rules(row, [h], [len(h) - T0], (1.3, 2, 5), eos_id=3)
        assert torch.equal(_bits(got), _bits(want)), b
        assert int(tok[0]) == int(torch.argmax(want.float(), dim=-1)[0])


# ---- LlamaForCausalLM.generate: the checks run before any engine exists -------------------------------------------------------------------------
class _Reached(Exception):
    pass


def _model():
    from radialog_amd.modeling_llama_imgemb import LlamaForCausalLM
    return LlamaForCausalLM.from_pretrained(None, torch_dtype=torch.float16, synthetic=True)


def test_generate_refuses_bad_rules_before_building_an_engine(monkeypatch):
    lm = _model()
    monkeypatch.setattr(lm, "_ensure_engine", lambda: (_ for _ in ()).throw(_Reached()))
    ids = torch.ones(1, 40, dtype=torch.long)
    for kw in (dict(repetition_penalty=0.0), dict(repetition_penalty=-1.5), dict(repetition_penalty=2), dict(repetition_penalty=float("nan")),
               dict(repetition_penalty="1.2"), dict(no_repeat_ngram_size=-1), dict(no_repeat_ngram_size=1.5), dict(min_new_tokens=-2),
               dict(repetition_penalty=1.2, num_beams=2), dict(no_repeat_ngram_size=3, num_beams=3), dict(min_new_tokens=1, num_beams=2)):
        with pytest.raises(ValueError):
            lm.generate(input_ids=ids, max_new_tokens=4, **kw)
    with pytest.raises(NotImplementedError):
        lm.generate(input_ids=ids, max_new_tokens=4, do_sample=True, repetition_penalty=1.2)
    for one in (1, 1.0, np.float32(1.0)):                                      # "off" in any numeric spelling passes, as in transformers
        with pytest.raises(_Reached):
            lm.generate(input_ids=ids, max_new_tokens=4, repetition_penalty=one)
    with pytest.raises(_Reached):                                              # neutral rules with beams are no conflict
        lm.generate(input_ids=ids, max_new_tokens=4, num_beams=2, repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=0)


def test_legal_rules_pass_validation_and_reach_the_engine(monkeypatch):
    """A legal rule goes past the checks (the stubbed _ensure_engine raises its sentinel, not ValueError), and the engine call receives it --
    with `reuse_prefix_kv` set on the model too (the engine drops the prefix reuse for a ruled call itself)."""
    from radialog_amd.engine import LogitsRules, RdxEngine
    lm = _model()
    ids = torch.ones(1, 40, dtype=torch.long)
    monkeypatch.setattr(lm, "_ensure_engine", lambda: (_ for _ in ()).throw(_Reached()))
    with pytest.raises(_Reached):
        lm.generate(input_ids=ids, max_new_tokens=4, repetition_penalty=1.2, no_repeat_ngram_size=3, min_new_tokens=2)
    seen = {}

    class FakeEngine:
        def generate(self, *a, **kw):
            seen.update(kw)
            raise _Reached()

    monkeypatch.setattr(lm, "_ensure_engine", lambda: setattr(lm, "_engine", FakeEngine()))
    lm.reuse_prefix_kv = True
    with pytest.raises(_Reached):
        lm.generate(input_ids=ids, max_new_tokens=4, repetition_penalty=1.2, no_repeat_ngram_size=3, min_new_tokens=2)
    assert seen["logits_rules"] == LogitsRules(1.2, 3, 2) and seen["logits_rules"].active
    lm._engine = None
    seen.clear()
    with pytest.raises(_Reached):
        lm.generate(input_ids=ids, max_new_tokens=4)
    assert not seen["logits_rules"].active
    # the engine's generate takes the rules by that name, and a ruled call never appends to a cached conversation
    import inspect
    for fn in (RdxEngine.generate, RdxEngine.prefill, RdxEngine.decode_step):
        assert "logits_rules" in inspect.signature(fn).parameters
    with pytest.raises(ValueError):
        LogitsRules(0.0, 0, 0)
    assert LogitsRules.of((1.3, 2, 0)) == LogitsRules(1.3, 2, 0) and not LogitsRules.of(None).active


def test_engine_tracks_the_rules_the_context_holds():
    """decode_step re-sets the rules when they differ from what the CONTEXT holds -- whichever call set that last -- not from what the last prefill asked for."""
    import types
    from radialog_amd.engine import LogitsRules, RdxEngine
    calls = []
    lib = types.SimpleNamespace(rdx_set_logits_rules=lambda ctx, r: calls.append(r is not None) or 0)
    eng = types.SimpleNamespace(lib=lib, ctx=None, _rules=LogitsRules())
    set_rules = lambda r: RdxEngine.set_logits_rules(eng, r)      # noqa: E731
    assert set_rules((1.3, 0, 0)).active and eng._rules == LogitsRules(1.3, 0, 0) and calls == [True]
    assert not set_rules(None).active and eng._rules == LogitsRules() and calls == [True, False]       # what generate(rules=None) does
    assert LogitsRules.of((1.3, 0, 0)) != eng._rules              # so a decode_step(logits_rules=(1.3, 0, 0)) sets them again
