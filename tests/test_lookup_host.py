"""Prompt-lookup decoding, the host side (no GPU): the restatement of the draft rule and of the trace (tests/_lookup.py) on hand-written cases, the
validation of `Lookup` and of generate()'s arguments before any engine exists, and the ABI declarations."""
import os
import re

import pytest
import torch

import _lookup as LK
from _lookup import Rule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the draft rule ---------------------------------------------------------------------------------------------------------------------------------
def test_longest_ngram_wins():
    #    0  1  2  3  4  5  6  7  8  9
    H = [1, 2, 3, 9, 7, 2, 3, 8, 2, 3]
    # n = 3 (8 2 3) has no earlier match; n = 2 (2 3) matches at 5 (-> 8) and 1 (-> 9): the most recent
    assert LK.find_draft(H, 2, 3, 1) == [8, 2]
    H2 = [5, 1, 2, 3, 4, 6, 2, 3, 7, 1, 2, 3]
    # n = 3 (1 2 3) matches at 1 -> 4 6; n = 2 alone would have taken the later (2 3) at 6 -> 7
    assert LK.find_draft(H2, 2, 3, 1) == [4, 6]
    assert LK.find_draft(H2, 2, 2, 1) == [7, 1]


def test_most_recent_match_wins():
    H = [4, 1, 5, 4, 2, 6, 4]
    assert LK.find_draft(H, 3, 1, 1) == [2, 6, 4]
    assert LK.find_draft(H, 1, 1, 1) == [2]


def test_a_match_ending_at_the_end_of_H_is_excluded():
    H = [7, 7]
    # the only other occurrence of (7) is at j = 0 with j + 1 < 2: allowed, and its continuation is the last token
    assert LK.find_draft(H, 4, 1, 1) == [7]
    # the last n tokens themselves (j = len - n) never count
    assert LK.find_draft([1, 2, 3], 4, 2, 1) == []
    assert LK.find_draft([3], 4, 3, 1) == []


def test_draft_is_clipped_at_len_H_at_the_budget_and_at_the_slot_bound():
    H = [1, 2, 3, 4, 1, 2]
    assert LK.find_draft(H, 15, 2, 1) == [3, 4, 1, 2]              # stops at len(H)
    assert LK.find_draft(H, 2, 2, 1) == [3, 4]
    assert LK.find_draft(H, 0, 2, 1) == []
    r = Rule(8, 3, 1)
    assert LK.draft_limit(r, emitted=1, max_new=24, slot=48, slot_end=72) == 8
    assert LK.draft_limit(r, emitted=20, max_new=24, slot=67, slot_end=72) == 3       # one token of the pass is the model's own
    assert LK.draft_limit(r, emitted=23, max_new=24, slot=70, slot_end=72) == 0
    assert LK.draft_limit(r, emitted=1, max_new=24, slot=48, slot_end=51) == 2        # slots 48 .. 50 only
    assert LK.draft_limit(r, emitted=1, max_new=24, slot=50, slot_end=51) == 0


def test_a_match_straddling_corpus_and_prompt_and_no_corpus():
    corpus, prompt = [9, 1], [2, 5, 6, 1, 2]
    assert LK.find_draft(corpus + prompt, 3, 2, 2) == [5, 6, 1]     # (1 2) starts in the corpus, ends in the prompt
    assert LK.find_draft(prompt, 3, 2, 2) == []                      # n_corpus = 0: no match
    assert LK.find_draft(prompt, 3, 2, 1) == [5, 6, 1]               # ... until unigrams are allowed
    assert LK.find_draft([1, 2, 3, 4], 3, 3, 1) == []                # no match at all


# ---- the trace simulator ----------------------------------------------------------------------------------------------------------------------------
def test_simulate_full_acceptance_and_a_rejection():
    prompt = [10, 11, 12]
    S = [20, 21, 22, 23, 24, 25]
    # the corpus holds S: token 0 is found, the draft is 21 22 23 (draft_len 3), all accepted, the pass emits 4 tokens; 5 of 6 are out, so the budget
    # max_new - emitted - 1 leaves no room for a draft: a plain step emits the last one
    trace, st = LK.simulate(prompt, S, S, Rule(3, 2, 1), max_new=6)
    assert trace == [(3, 3), (0, 0)] and st == {"passes": 1, "drafted": 3, "accepted": 3, "forwards": 2}
    trace, st = LK.simulate(prompt, S + [26], S + [26], Rule(3, 2, 1), max_new=7)
    assert trace == [(3, 3), (1, 1)] and st == {"passes": 2, "drafted": 4, "accepted": 4, "forwards": 2}
    bad = [20, 21, 99, 23, 24, 25]
    trace, _ = LK.simulate(prompt, bad, S, Rule(3, 2, 1), max_new=6)
    # draft 21 99 23: one accepted, emits 21 22; then (21 22) / (22) has no match in the corpus: a plain step emits 23; then (23) -> 24, clipped to 1 by
    # the budget, accepted: the pass emits 24 25
    assert trace == [(3, 1), (0, 0), (1, 1)]


def test_simulate_eos_inside_an_accepted_run_and_max_new_mid_pass():
    prompt = [10, 11]
    full = [20, 21, 2, 23, 24]
    trace, st = LK.simulate(prompt, full, [20, 21, 2], Rule(4, 2, 1), max_new=8, eos_id=2)
    assert trace == [(4, 2)] and st["accepted"] == 2                 # the EOS is the second draft: the emission ends there
    trace, _ = LK.simulate(prompt, full, [20, 21, 2], Rule(1, 2, 1), max_new=8, eos_id=2)
    assert trace == [(1, 1)]                                         # ... and here it is the pass's own token
    # max_new reached mid-pass: the draft is clipped to max_new - emitted - 1 so that the pass's own token is the last one
    trace, _ = LK.simulate(prompt, full, full[:4], Rule(4, 2, 1), max_new=4)
    assert trace == [(2, 2)]
    with pytest.raises(AssertionError):
        LK.simulate(prompt, full, full[:3], Rule(4, 2, 1), max_new=4)      # a call would not have stopped there


def test_accept_step_restates_one_launch():
    r = LK.accept_step(am=[5, 6, 9, 1], tail=[4, 5, 6, 7], state=(3, 50, 50, 1), hist=[1, 2, 3, 4], corpus=[], rule=Rule(3, 2, 1), max_new=20, slot_end=80)
    assert r["emitted"] == [5, 6, 9] and r["accepted"] == 2 and r["state"] == (6, 53, 53, 1) and r["tail"][0] == 9 and not r["finished"]
    r = LK.accept_step(am=[5, 2, 9, 1], tail=[4, 5, 2, 9], state=(3, 50, 50, 1), hist=[1], corpus=[], rule=Rule(3, 2, 1), max_new=20, slot_end=80, eos_id=2)
    assert r["emitted"] == [5, 2] and r["accepted"] == 2 and r["finished"] and r["state"] == (5, 52, 52, 0)


# ---- argument validation ----------------------------------------------------------------------------------------------------------------------------
def test_lookup_validates_its_fields():
    from radialog_amd.engine import Lookup
    assert Lookup() == Lookup(8, 3, 1) and Lookup.of(5) == Lookup(5, 3, 1) and Lookup.of((4, 2, 2)) == Lookup(4, 2, 2)
    for kw in (dict(draft_len=0), dict(draft_len=16), dict(draft_len=-1), dict(draft_len=2.0), dict(draft_len=True), dict(ngram_max=0), dict(ngram_max=9),
               dict(ngram_min=0), dict(ngram_max=2, ngram_min=3), dict(ngram_min="1")):
        with pytest.raises(ValueError):
            Lookup(**kw)


class _Reached(Exception):
    pass


def _model(**kw):
    from radialog_amd.modeling_llama_imgemb import LlamaForCausalLM
    return LlamaForCausalLM.from_pretrained(None, torch_dtype=torch.bfloat16, synthetic=True, **kw)


def test_generate_refuses_what_the_library_refuses_before_building_an_engine(monkeypatch):
    lm = _model()
    lm.enable_sampling = True
    monkeypatch.setattr(lm, "_ensure_engine", lambda: (_ for _ in ()).throw(_Reached()))
    ids = torch.ones(1, 40, dtype=torch.long)
    for kw in (dict(num_beams=2), dict(do_sample=True), dict(repetition_penalty=1.2), dict(no_repeat_ngram_size=2), dict(min_new_tokens=1),
               dict(output_logprobs=True, return_dict_in_generate=True)):
        with pytest.raises(ValueError, match="prompt_lookup_num_tokens"):
            lm.generate(input_ids=ids, max_new_tokens=4, prompt_lookup_num_tokens=4, **kw)
    with pytest.raises(ValueError, match="batch"):
        lm.generate(input_ids=torch.ones(2, 40, dtype=torch.long), max_new_tokens=4, prompt_lookup_num_tokens=4)
    for kw in (dict(prompt_lookup_num_tokens=16), dict(prompt_lookup_num_tokens=-1), dict(prompt_lookup_num_tokens=4, max_matching_ngram_size=9),
               dict(prompt_lookup_num_tokens=4, max_matching_ngram_size=0), dict(max_matching_ngram_size=2), dict(lookup_corpus=[1, 2])):
        with pytest.raises(ValueError):
            lm.generate(input_ids=ids, max_new_tokens=4, **kw)
    for extra in (dict(kv_fp8=True), dict(weights_fp8=True)):
        lm2 = _model(**extra)
        monkeypatch.setattr(lm2, "_ensure_engine", lambda: (_ for _ in ()).throw(_Reached()))
        with pytest.raises(ValueError, match="fp8"):
            lm2.generate(input_ids=ids, max_new_tokens=4, prompt_lookup_num_tokens=4)
        with pytest.raises(_Reached):
            lm2.generate(input_ids=ids, max_new_tokens=4)


def test_neutral_arguments_take_the_existing_path_and_legal_ones_reach_generate_lookup(monkeypatch):
    from radialog_amd.engine import Lookup
    lm = _model()
    seen = {}

    class FakeEngine:
        def generate(self, *a, **kw):
            seen["generate"] = kw
            raise _Reached()

        def generate_lookup(self, *a, **kw):
            seen["lookup"] = kw
            raise _Reached()

    monkeypatch.setattr(lm, "_ensure_engine", lambda: setattr(lm, "_engine", FakeEngine()))
    ids = torch.ones(1, 40, dtype=torch.long)
    for kw in ({}, dict(prompt_lookup_num_tokens=None), dict(prompt_lookup_num_tokens=0)):
        seen.clear()
        with pytest.raises(_Reached):
            lm.generate(input_ids=ids, max_new_tokens=4, **kw)
        assert "generate" in seen and "lookup" not in seen
    seen.clear()
    with pytest.raises(_Reached):
        lm.generate(input_ids=ids, max_new_tokens=4, prompt_lookup_num_tokens=6, max_matching_ngram_size=2, lookup_corpus=[3, 4, 5])
    assert "generate" not in seen and seen["lookup"]["lookup"] == Lookup(6, 2, 1) and seen["lookup"]["corpus"] == [3, 4, 5]


# ---- ABI --------------------------------------------------------------------------------------------------------------------------------------------
def test_the_new_symbols_are_declared_in_the_headers_and_in_the_binding():
    from radialog_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "rdx.h")).read()
    for name in ("rdx_set_lookup", "rdx_generate_lookup"):
        assert name in _lib.SYMBOLS and re.search(r"\bint " + name + r"\(", hdr), name
    # one ctypes argument per C parameter
    for name, table, path in (("rdx_generate_lookup", _lib.SYMBOLS, "rdx.h"), ("rdx_set_lookup", _lib.SYMBOLS, "rdx.h"),
                              ("rdx_lookup_accept_test", _lib.DEC_HOOK_SYMBOLS, "rdx_dec_hooks.h")):
        text = open(os.path.join(ROOT, "include", path)).read()
        m = re.search(r"\bint " + name + r"\((.*?)\);", text, re.S)
        assert m, name
        assert len(m.group(1).split(",")) == len(table[name][1]), name
    assert [f[0] for f in _lib.RdxLookup._fields_] == ["draft_len", "ngram_max", "ngram_min"]
    assert "typedef struct rdx_lookup { int draft_len; int ngram_max; int ngram_min; } rdx_lookup;" in hdr
