"""Logits rules of the greedy search on the GPU: select_step_k (radialog_amd/csrc/elem.hip) alone through rdx_select_test and inside the decode
step, against the plain-torch restatement of tests/_logits_rules.py (which tests/test_logits_rules_host.py holds to transformers' processors).
Everything here is equality of bits: the rules are elementwise fp32 arithmetic with one rounding, -inf stores and an argmax."""
import ctypes as C

import pytest
import torch

import _logits_rules as LR
from radialog_amd import synth
from radialog_amd.config import small_cfg

pytestmark = pytest.mark.gpu

TDT = {"f16": torch.float16, "bf16": torch.bfloat16}
INF = float("inf")


def _bits(t):
    return t.contiguous().view(torch.int16)


# ---- 1. the kernel alone -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["f16", "bf16"])
def hook_eng(request):
    from radialog_amd.engine import RdxEngine
    e = RdxEngine(small_cfg(), dtype=request.param, device=0, max_batch=1, max_len=32, llama=False, vision=False)
    yield e
    e.close()


LD = 12
LENS = (1, 2, 7, LD)
EOS = 2
RULESETS = [(1.3, 0, 0), (0.5, 0, 0), (1.0, 1, 0), (1.0, 3, 0), (1.0, 0, 5), (1.3, 2, 3)]
N_PLANTS = 6


def _case(dtype, B, V, rules, variant):
    """Inputs of one launch: per row a history of length 1, 2, 7 or LD (a few distinct ids, so that n-grams repeat; id V - 1 and ids at both ends of the
    16-byte pieces among them), n_generated 4 or 5, and one planted situation per row (row + variant picks which)."""
    p, n, m = rules
    g = torch.Generator().manual_seed(1000 * B + V + 17 * variant + int(100 * p) + 7 * n + m)
    x = (torch.randn(B, V, generator=g) * 4).to(dtype)
    tiny = torch.finfo(dtype).tiny
    hist = torch.zeros(B, LD, dtype=torch.int32)
    lens, gens, hists = [], [], []
    few = [3, 5, 9, V - 1, 8, 15, 16, V - 2]
    for b in range(B):
        L = LENS[(b + variant) % 4]
        h = [few[int(i)] for i in torch.randint(0, 3 + (b % 6), (L,), generator=g)]
        if L >= 7:
            h[L - 2:] = h[0:2]                                   # the last tokens repeat an earlier stretch: 2- and 3-gram bans exist
            h[3] = int(torch.randint(0, V, (1,), generator=g))   # ... and one id from anywhere in the vocabulary
        hist[b, :L] = torch.tensor(h, dtype=torch.int32)
        hist[b, L:] = 7                                          # behind the length: must not be read as history
        lens.append(L); gens.append(4 + (b + variant) % 2); hists.append(h)
        # subnormal results in every row: the smallest normal / p, a subnormal * p, and their negatives
        x[b, h[0]] = tiny if b % 2 == 0 else -tiny * 0.75
        if L > 1:
            x[b, h[1]] = tiny * 0.375 if b % 2 else -tiny * 1.25
        banned = [t for t in LR.banned_ngram_tokens(h, n) if 0 <= t < V]
        if m > 0 and gens[-1] < m:
            banned.append(EOS)
        free = [i for i in range(20, 36) if i not in h and i not in banned and i != EOS]
        plant = (b + variant) % N_PLANTS
        if plant == 0:                                           # id V - 1 is the maximum (odd V: the scalar tail must be selectable)
            x[b, V - 1] = 60.0
        elif plant == 1:                                         # two equal maxima: the lower index wins
            x[b, free[3]] = 50.0; x[b, free[1]] = 50.0
        elif plant == 2:                                         # a tie that exists only after the penalty (p = 1: before as well)
            x[b, h[-1]] = 40.0
            after = LR.penalise(x[b], [h[-1]], p)[h[-1]] if p != 1.0 else x[b, h[-1]]
            x[b, free[0]] = after; x[b, free[5]] = after
        elif plant == 3:                                         # the maximum is a token the ban removes
            if banned:
                x[b, banned[0]] = 70.0
        elif plant == 4:                                         # -inf on the way in: inside and outside the history
            x[b, h[-1]] = -INF; x[b, free[2]] = -INF
        else:                                                    # everything but one history token is -inf
            x[b] = -INF
            x[b, h[0]] = -3.0
    return x, hist, torch.tensor(lens, dtype=torch.int32), torch.tensor(gens, dtype=torch.int32), hists, gens


@pytest.mark.parametrize("B,V", [(1, 40), (3, 32001), (33, 32001)])
def test_select_kernel_alone_equals_the_restatement(hook_eng, B, V):
    dtype = hook_eng.tdtype
    for rules in RULESETS:
        for variant in range(max(1, N_PLANTS // B)):
            x, hist, lens, gens, hists, gl = _case(dtype, B, V, rules, variant)
            want, want_tok = LR.apply_rules(x, hists, gl, rules, eos_id=EOS)
            got, tok = hook_eng.select_test(x, hist, lens, gens, rules, eos_id=EOS)
            got, tok = got.cpu(), tok.cpu().long()
            bad = (_bits(got) != _bits(want)).nonzero()
            assert bad.numel() == 0, f"{rules} variant {variant}: processed rows differ at (row, id) {bad[:8].tolist()}"
            assert torch.equal(tok, want_tok), f"{rules} variant {variant}: tokens {tok.tolist()} != {want_tok.tolist()}"
            assert torch.equal(torch.isinf(got), torch.isinf(want))
    # eos_id = -1 with min_new_tokens: nothing is banned, the row comes back as it went in
    x, hist, lens, gens, hists, gl = _case(dtype, B, V, (1.0, 0, 5), 0)
    got, tok = hook_eng.select_test(x, hist, lens, gens, (1.0, 0, 5), eos_id=-1)
    assert torch.equal(_bits(got.cpu()), _bits(x)) and torch.equal(tok.cpu().long(), LR.greedy_argmax(x))


def test_select_hook_refuses_bad_rules(hook_eng):
    from radialog_amd._lib import RdxError
    x = torch.zeros(1, 40, dtype=hook_eng.tdtype)
    one = torch.ones(1, dtype=torch.int32)
    with pytest.raises(ValueError):
        hook_eng.select_test(x, torch.zeros(1, 4, dtype=torch.int32), one * 5, one, (1.3, 0, 0))           # a length beyond the history row
    with pytest.raises(RdxError):
        hook_eng.select_test(torch.zeros(1, 300000, dtype=hook_eng.tdtype), torch.zeros(1, 4, dtype=torch.int32), one, one, (1.3, 0, 0))


# ---- 2.-5. inside the decode step ------------------------------------------------------------------------------------------------------------
T_PROMPT, MAX_NEW = 48, 8


def _engine(B, dtype="f16"):
    from radialog_amd.engine import RdxEngine, synth_getter
    cfg = small_cfg()
    eng = RdxEngine(cfg, dtype=dtype, device=0, max_batch=B, max_len=128, lora=True, vision=False)
    eng.load_weights(synth_getter(cfg, eng.device, lora=True), vision=False)
    return eng, cfg


def _prompt(cfg, B):
    ids = synth.synth_prompt_ids(B, T_PROMPT, vocab=cfg.llama.vocab, img_offset=4, pad_rows=False, seed=21)
    ids[B - 1] = torch.cat([torch.zeros(3, dtype=torch.long), ids[B - 1, : T_PROMPT - 3]])           # one left-padded row (pad id 0)
    qf = synth.synth("t.qf_rules", (B, 32, cfg.llama.qformer_dim), -1.0, 1.0)
    return ids, qf


def _gen(eng, ids, qf, rules, eos=-1, use_graph=True, max_new=MAX_NEW):
    toks, scores, n = eng.generate(ids, qf, max_new=max_new, eos_id=eos, pad_id=0, output_scores=True, use_graph=use_graph, logits_rules=rules)
    return toks[:, :n].cpu().long().clone(), scores[:n].cpu().clone(), n


@pytest.mark.parametrize("B", [1, 4, 32])
def test_ruled_generation_equals_the_restatement_on_the_raw_logits(B):
    """Rules (1.3, 3, 0) through rdx_generate (captured step graph), then the same token path replayed with the rules off (prefill + decode_step on
    the ruled run's tokens: the same kernels on the same inputs) for every step's raw logits. The restatement applied to those, with the
    histories rebuilt here, must give the ruled run's scores bit for bit and its tokens at every (row, step)."""
    eng, cfg = _engine(B)
    try:
        ids, qf = _prompt(cfg, B)
        rules = (1.3, 3, 0)
        toks, scores, n = _gen(eng, ids, qf, rules)
        assert n == MAX_NEW
        raw = [eng.prefill(ids, qf, MAX_NEW, eos_id=-1, pad_id=0)[1].cpu().clone()]
        for s in range(1, MAX_NEW):
            raw.append(eng.decode_step(input_ids=toks[:, s - 1])[1].cpu().clone())
        hists = [ids[b].tolist() for b in range(B)]
        for s in range(MAX_NEW):
            want, want_tok = LR.apply_rules(raw[s], hists, [s] * B, rules, eos_id=-1)
            diff = (_bits(scores[s]) != _bits(want)).nonzero()
            assert diff.numel() == 0, f"step {s}: scores differ from the restatement at (row, id) {diff[:8].tolist()}"
            assert torch.equal(toks[:, s], want_tok), f"step {s}: tokens {toks[:, s].tolist()} != {want_tok.tolist()}"
            if s == 0:                              # the rules did something: the prompt's own tokens were penalised
                for b in range(B):
                    seen = torch.tensor(sorted(set(hists[b])))
                    changed = _bits(scores[0][b, seen]) != _bits(raw[0][b, seen])
                    assert bool(changed.any()), f"row {b}: the scores at the prompt's token ids are the raw logits"
            for b in range(B):
                hists[b].append(int(toks[b, s]))
    finally:
        eng.close()


def test_graph_replay_equals_eager_under_rules_with_eos_and_pad():
    """Rules (1.3, 2, 2) with an EOS id the run reaches: the captured step graph and eager launches give identical tokens and scores, no row
    emits EOS among its first two tokens, and a finished row emits pad from then on."""
    B = 4
    eng, cfg = _engine(B)
    try:
        ids, qf = _prompt(cfg, B)
        rules = (1.3, 2, 2)
        free, _, _ = _gen(eng, ids, qf, rules)
        # an EOS id row 0 reaches: its first token from step 3 on (else step 2) that it has not emitted before -- banning an id the row never
        # selected changes nothing, so row 0 walks the same path up to that step and finishes there
        first = [s for s in (3, 4, 5, 2) if int(free[0, s]) not in free[0, :s].tolist()]
        assert first, f"row 0 repeats itself from step 2 on: {free[0].tolist()}"
        eos = int(free[0, first[0]])
        tg, sg, ng = _gen(eng, ids, qf, rules, eos=eos, use_graph=True)
        te, se, ne = _gen(eng, ids, qf, rules, eos=eos, use_graph=False)
        assert ng == ne and torch.equal(tg, te)
        assert torch.equal(_bits(sg), _bits(se))
        assert not bool((tg[:, :2] == eos).any())
        assert bool((sg[:2, :, eos] == -INF).all())
        finished = 0
        for b in range(B):
            at = (tg[b] == eos).nonzero().flatten()
            if at.numel():
                finished += 1
                assert int(at[0]) >= 2 and bool((tg[b, int(at[0]) + 1:] == 0).all()), f"row {b}: {tg[b].tolist()}"
        assert finished >= 1 and int((tg[0] == eos).nonzero()[0]) == first[0]
    finally:
        eng.close()


def test_neutral_rules_are_off_and_a_rule_change_recaptures_the_graph():
    B = 4
    eng, cfg = _engine(B)
    try:
        ids, qf = _prompt(cfg, B)
        plain_t, plain_s, _ = _gen(eng, ids, qf, None)
        for neutral in ((1.0, 0, 0), None):
            t, s, _ = _gen(eng, ids, qf, neutral)
            assert torch.equal(t, plain_t) and torch.equal(_bits(s), _bits(plain_s))
        # two rule sets back to back on one context, same buffers: the second call must not replay the first one's graph
        a_t, a_s, _ = _gen(eng, ids, qf, (1.3, 0, 0))
        b_t, b_s, _ = _gen(eng, ids, qf, (0.5, 1, 0))
        b_eager_t, b_eager_s, _ = _gen(eng, ids, qf, (0.5, 1, 0), use_graph=False)
        assert torch.equal(b_t, b_eager_t) and torch.equal(_bits(b_s), _bits(b_eager_s))
        assert not torch.equal(_bits(a_s), _bits(b_s))
        assert bool((b_s[1, 0, b_t[0, 0]] == -INF)) and not bool((a_s[1] == -INF).any())        # n = 1 bans token 0 at step 1; the penalty alone bans nothing
        t, s, _ = _gen(eng, ids, qf, None)          # and off again
        assert torch.equal(t, plain_t) and torch.equal(_bits(s), _bits(plain_s))
    finally:
        eng.close()


def test_beam_search_and_append_are_refused_under_rules():
    from radialog_amd._lib import RdxLogitsRules
    B = 2
    eng, cfg = _engine(B)
    try:
        ids, qf = _prompt(cfg, B)
        eng.generate(ids, qf, max_new=4, eos_id=-1, reuse_prefix=True)             # a cached conversation to append to
        lib, ctx = eng.lib, eng.ctx
        dev = eng.device
        tail = torch.full((B, 2), 11, dtype=torch.int32, device=dev)
        toks = torch.zeros(B, 4, dtype=torch.int32, device=dev)
        ids32 = ids[:1].repeat(2, 1).to(dev, torch.int32).contiguous()               # one prompt, expanded to its two beam rows
        qf32 = qf[:1].repeat(2, 1, 1).to(dev, torch.float32).contiguous()
        host_t, host_l, n = torch.zeros(1, 4, dtype=torch.int32), torch.zeros(1, dtype=torch.int32), C.c_int(0)
        p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731

        def calls():
            torch.cuda.synchronize(dev)
            return (lib.rdx_prefill_append(ctx, p(tail), B, 2, T_PROMPT, 4, -1, 0, p(toks), None),
                    lib.rdx_generate_append(ctx, p(tail), B, 2, T_PROMPT, 4, -1, 0, p(toks), None, C.byref(n), 1),
                    lib.rdx_beam_search(ctx, p(ids32), None, 1, 2, T_PROMPT, p(qf32), 4, -1, 0, 1.0, 0, p(host_t), p(host_l), None, None, C.byref(n)))

        assert lib.rdx_set_logits_rules(ctx, C.byref(RdxLogitsRules(1.2, 0, 0))) == 0
        assert calls() == (-1, -1, -1)
        assert b"logits rules" in lib.rdx_last_error(ctx)
        for bad in (RdxLogitsRules(0.0, 0, 0), RdxLogitsRules(float("inf"), 0, 0), RdxLogitsRules(float("nan"), 0, 0), RdxLogitsRules(1.2, -1, 0),
                    RdxLogitsRules(1.2, 0, -1)):
            assert lib.rdx_set_logits_rules(ctx, C.byref(bad)) == -1
        assert calls() == (-1, -1, -1)              # a refused rule set leaves the previous one in force
        assert lib.rdx_set_logits_rules(ctx, None) == 0
        assert calls() == (0, 0, 0)
        eng.sync()
    finally:
        eng.close()


@pytest.mark.parametrize("B", [1, 4])
def test_ruled_generation_without_a_scores_buffer_selects_the_same_tokens(B):
    """No scores asked for (the default generate() call): the lm_head writes into the context's own logits rows and select_step_k processes those.
    Same tokens as with a scores buffer, captured graph and eager; the step timer replays that graph too."""
    eng, cfg = _engine(B)
    try:
        ids, qf = _prompt(cfg, B)
        rules = (1.3, 3, 2)
        want, _, n = _gen(eng, ids, qf, rules)
        plain, _, _ = _gen(eng, ids, qf, None)
        assert not torch.equal(want, plain)                      # the rules change the path, so equal tokens below mean the rules ran
        for use_graph in (True, False):
            toks, scores, m = eng.generate(ids, qf, max_new=MAX_NEW, eos_id=-1, pad_id=0, output_scores=False, use_graph=use_graph, logits_rules=rules)
            assert scores is None and m == n and torch.equal(toks[:, :m].cpu().long(), want), f"graph {use_graph}"
        assert eng.time_unit(0, 2) > 0.0
    finally:
        eng.close()


def test_forced_ids_enter_the_history_under_rules():
    """rdx_decode_step_ids under rules: the caller's token, not the one the previous step selected, is what the history holds. Rules (1.3, 1, 0) ban
    every token of the history, so each forced id is -inf from the step behind it on; the scores equal the restatement on the raw logits of the
    same forced path (replayed with the rules off) with the forced ids in the history."""
    B, steps = 4, 4
    eng, cfg = _engine(B)
    try:
        ids, qf = _prompt(cfg, B)
        rules = (1.3, 1, 0)
        forced = [torch.tensor([900 + 10 * s + b for b in range(B)]) for s in range(steps)]
        toks, lg = eng.prefill(ids, qf, MAX_NEW, eos_id=-1, pad_id=0, logits_rules=rules)
        got = [lg.cpu().clone()]
        for s in range(steps):
            got.append(eng.decode_step(input_ids=forced[s])[1].cpu().clone())
        sel = toks.cpu().long().clone()
        raw = [eng.prefill(ids, qf, MAX_NEW, eos_id=-1, pad_id=0)[1].cpu().clone()]
        for s in range(steps):
            raw.append(eng.decode_step(input_ids=forced[s])[1].cpu().clone())
        hists = [ids[b].tolist() for b in range(B)]
        for s in range(steps + 1):
            want, want_tok = LR.apply_rules(raw[s], hists, [s] * B, rules)
            assert torch.equal(_bits(got[s]), _bits(want)), f"step {s}: scores differ from the restatement"
            assert torch.equal(sel[:, s], want_tok), f"step {s}"
            if s > 0:
                for b in range(B):
                    assert got[s][b, forced[s - 1][b]] == -INF
                    if int(sel[b, s - 1]) not in hists[b]:
                        assert got[s][b, sel[b, s - 1]] != -INF          # the replaced token is not history
            if s < steps:
                for b in range(B):
                    hists[b].append(int(forced[s][b]))
    finally:
        eng.close()
