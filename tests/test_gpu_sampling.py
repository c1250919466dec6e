"""Sampled decoding on the GPU: sample_step_k (radialog_amd/csrc/elem.hip) alone through rdx_sample_test and inside the decode step, against the
fp64 restatement of tests/_sampling.py (which tests/test_sampling_host.py holds to hand cases and to transformers' warpers). The scores row is
compared bit for bit (the kept set and T(x / t) are exact); the token by the restatement's acceptance rule (DELTA = 2^-16 of CDF, derived there).
Kernel-alone rows whose top-p decision lies within MARGIN = 2^-14 of its threshold are redrawn on the CPU before anything is launched."""
import ctypes as C

import pytest
import torch

import _logits_rules as LR
import _sampling as SP
from radialog_amd import synth
from radialog_amd.config import LlamaCfg, RaDialogCfg, small_cfg

pytestmark = pytest.mark.gpu

INF = float("inf")
EOS = 2
RULES = (1.3, 2, 3)                     # penalty 1.3, n-gram 2, min_new 3 with EOS = 2


def _bits(t):
    return t.contiguous().view(torch.int16)


def _settings(V):
    """(temperature, top_k, top_p): the four mixed settings, k = 1, k >= V, p = 1e-6."""
    return [(1.0, 0, 1.0), (0.7, 50, 1.0), (1.3, 0, 0.9), (0.8, 40, 0.95), (1.0, 1, 1.0), (1.0, V + 7, 1.0), (1.0, 0, 1e-6)]


# ---- 1. the kernel alone -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["f16", "bf16"])
def hook_eng(request):
    from radialog_amd.engine import RdxEngine
    e = RdxEngine(small_cfg(), dtype=request.param, device=0, max_batch=1, max_len=32, llama=False, vision=False)
    yield e
    e.close()


def _row(dtype, V, variant, seed):
    """One logits row shaped like a language model's -- a broad tail and a few dozen likely tokens, so that the top-p boundary falls between masses
    far larger than MARGIN -- in one of four variants: plain; duplicated values (the k-th largest among them); -inf where a ban struck; one dominant
    logit."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(V, generator=g) * 2 - 8
    head = torch.randperm(V, generator=g)[: min(44, V // 2)]
    x[head] = torch.randn(head.numel(), generator=g) * 3 + 6
    if variant == 1:
        x = torch.round(x * 2) / 2                                  # half-integer values: groups of equal values everywhere
        order = torch.argsort(x, descending=True)
        for k in (40, 50):
            if k + 1 < V:
                x[order[k - 2]] = x[order[k - 1]]; x[order[k]] = x[order[k - 1]]      # the k-th largest value occurs on both sides of rank k
    elif variant == 2:
        x[torch.randperm(V, generator=g)[: max(2, V // 20)]] = -INF
        x[head[0]] = -INF
    elif variant == 3:
        x[int(torch.randint(0, V, (1,), generator=g))] = 30.0
    return x.to(dtype)


def _history(b, V):
    few = [3, 5, 9, 3, 5, V - 1, 3]      # ends in 3: the bigram (3, 5) bans 5; 3, 5, 9 and V - 1 are penalised
    h = few[b % 3:] if b % 2 else few
    return [min(t + (b % 4), V - 1) if t != V - 1 else t for t in h]


def _launch_inputs(dtype, B, V, n_gen, seed0):
    """Rows, histories and the restated results of every (setting, rules off / on) for one launch. A candidate row with a top-p gap below MARGIN in any
    of them is redrawn from the next seed. Returns (x, hist, hist_len, hists, want {(setting index, ruled): scores [B, V]}, candidates, redraws)."""
    LD = 8
    hists = [_history(b, V) for b in range(B)]
    hist = torch.zeros(B, LD, dtype=torch.int32)
    for b, h in enumerate(hists):
        hist[b, :len(h)] = torch.tensor(h, dtype=torch.int32)
    lens = torch.tensor([len(h) for h in hists], dtype=torch.int32)
    settings = _settings(V)
    x = torch.empty(B, V, dtype=dtype)
    want = {(si, r): torch.empty(B, V, dtype=dtype) for si in range(len(settings)) for r in (False, True)}
    cands = redraws = 0
    for b in range(B):
        seed = seed0 + 131 * b
        while True:
            cands += 1
            row = _row(dtype, V, (b + n_gen[b]) % 4, seed)
            ruled_row = LR.apply_rules(row.unsqueeze(0), [hists[b]], [n_gen[b]], RULES, eos_id=EOS)[0][0]
            res = {(si, r): SP.warp_row(ruled_row if r else row, *settings[si]) for si in range(len(settings)) for r in (False, True)}
            if min(v[2] for v in res.values()) >= SP.MARGIN:
                break
            redraws += 1
            seed += 7919
        x[b] = row
        for key, v in res.items():
            want[key][b] = v[0]
    return x, hist, lens, hists, want, cands, redraws


def _draw_indices(B):
    """The launches of one (B, V): every row meets draw indices 0-7 over them (33 rows: in one launch)."""
    if B >= 8:
        return [[b % 8 for b in range(B)]]
    return [[(B * j + b) % 8 for b in range(B)] for j in range((8 + B - 1) // B)]


@pytest.mark.parametrize("B,V", [(1, 40), (3, 32001), (33, 32001)])
def test_sample_kernel_alone_meets_the_restatement(hook_eng, B, V):
    dtype = hook_eng.tdtype
    settings = _settings(V)
    cands = redraws = 0
    seed = 0x9E3779B97F4A7C15
    for li, n_gen in enumerate(_draw_indices(B)):
        x, hist, lens, hists, want, c, r = _launch_inputs(dtype, B, V, n_gen, 1000 * B + V + 17 * li)
        cands += c; redraws += r
        ng = torch.tensor(n_gen, dtype=torch.int32)
        for si, (t, k, p) in enumerate(settings):
            for ruled in (False, True):
                kw = dict(rules=RULES, hist=hist, hist_len=lens, eos_id=EOS) if ruled else {}
                got, tok = hook_eng.sample_test(x, ng, (t, k, p, seed), **kw)
                got2, tok2 = hook_eng.sample_test(x, ng, (t, k, p, seed), **kw)
                got, tok = got.cpu(), tok.cpu().long()
                tag = f"launch {li} setting {(t, k, p)} rules {ruled}"
                assert torch.equal(_bits(got), _bits(got2.cpu())) and torch.equal(tok, tok2.cpu().long()), f"{tag}: two launches differ"
                w = want[(si, ruled)]
                bad = (_bits(got) != _bits(w)).nonzero()
                assert bad.numel() == 0, f"{tag}: scores differ from the restatement at (row, id) {bad[:8].tolist()}"
                for b in range(B):
                    ok, why = SP.accepts(w[b], int(tok[b]), SP.u24(seed, b, n_gen[b]))
                    assert ok, f"{tag} row {b} draw {n_gen[b]}: outside the acceptance rule: {why}"
                if k == 1:                                          # a single maximum in every row but the duplicated ones: the argmax
                    am = LR.greedy_argmax(w)
                    one_max = (w == w.float().max(dim=1, keepdim=True).values.to(w.dtype)).sum(1) == 1
                    assert torch.equal(tok[one_max], am[one_max])
    assert redraws <= -(-cands // 16), f"{redraws} of {cands} candidate rows needed a redraw (at most 1 in 16, in whole rows)"


def test_seed_and_row_enter_the_draw(hook_eng):
    dtype, B, V = hook_eng.tdtype, 33, 32001
    x = _row(dtype, V, 0, 5).unsqueeze(0).repeat(B, 1)             # identical logits in all 33 rows
    ng = torch.zeros(B, dtype=torch.int32)
    _, a = hook_eng.sample_test(x, ng, (1.0, 0, 1.0, 1))
    _, b = hook_eng.sample_test(x, ng, (1.0, 0, 1.0, 2))
    _, a7 = hook_eng.sample_test(x, ng + 7, (1.0, 0, 1.0, 1))
    a, b, a7 = a.cpu(), b.cpu(), a7.cpu()
    assert len(set(a.tolist())) > 1, "33 rows of identical logits drew one token: the row index is not in the counter"
    assert not torch.equal(a, b), "another seed drew the same 33 tokens"
    assert not torch.equal(a, a7), "another draw index drew the same 33 tokens"
    scores = SP.warp_row(x[0], 1.0, 0, 1.0)[0]
    for r in range(B):
        assert SP.accepts(scores, int(a[r]), SP.u24(1, r, 0))[0] and SP.accepts(scores, int(a7[r]), SP.u24(1, r, 7))[0]


def test_sample_hook_and_set_sampling_refuse_bad_arguments(hook_eng):
    from radialog_amd._lib import RdxError, RdxSampling
    x = torch.zeros(1, 40, dtype=hook_eng.tdtype)
    one = torch.ones(1, dtype=torch.int32)
    with pytest.raises(RdxError):                                   # a row that does not fit the LDS
        hook_eng.sample_test(torch.zeros(1, 300000, dtype=hook_eng.tdtype), one, (1.0, 0, 1.0, 0))
    with pytest.raises(ValueError):                                 # active rules without a history
        hook_eng.sample_test(x, one, (1.0, 0, 1.0, 0), rules=RULES)
    # a context without finalised llama weights cannot sample
    assert hook_eng.lib.rdx_set_sampling(hook_eng.ctx, C.byref(RdxSampling(1, 1.0, 0, 1.0, 0))) == -1
    assert b"not finalized" in hook_eng.lib.rdx_last_error(hook_eng.ctx)
    assert hook_eng.lib.rdx_set_sampling(hook_eng.ctx, None) == 0


# ---- 2. inside the decode step ---------------------------------------------------------------------------------------------------------------
T_PROMPT, MAX_NEW = 48, 12
SAMPLING = (0.8, 50, 0.95, 20240229)


def _engine(B, dtype="f16", cfg=None):
    from radialog_amd.engine import RdxEngine, synth_getter
    cfg = cfg or small_cfg()
    eng = RdxEngine(cfg, dtype=dtype, device=0, max_batch=B, max_len=128, lora=True, vision=False)
    eng.load_weights(synth_getter(cfg, eng.device, lora=True), vision=False)
    return eng, cfg


def _prompt(cfg, B):
    ids = synth.synth_prompt_ids(B, T_PROMPT, vocab=cfg.llama.vocab, img_offset=4, pad_rows=False, seed=23)
    ids[B - 1] = torch.cat([torch.zeros(3, dtype=torch.long), ids[B - 1, : T_PROMPT - 3]])           # one left-padded row (pad id 0)
    qf = synth.synth("t.qf_sampling", (B, 32, cfg.llama.qformer_dim), -1.0, 1.0)
    return ids, qf


def _gen(eng, ids, qf, sampling, rules=None, eos=-1, use_graph=True, max_new=MAX_NEW, scores=True):
    toks, sc, n = eng.generate(ids, qf, max_new=max_new, eos_id=eos, pad_id=0, output_scores=scores, use_graph=use_graph, logits_rules=rules, sampling=sampling)
    return toks[:, :n].cpu().long().clone(), (sc[:n].cpu().clone() if scores else None), n


def _raw_rows(eng, ids, qf, toks, steps):
    """Every step's raw logits on the token path `toks`: the plain context (no rules, no sampling), teacher-forced."""
    raw = [eng.prefill(ids, qf, MAX_NEW, eos_id=-1, pad_id=0)[1].cpu().clone()]
    for s in range(1, steps):
        raw.append(eng.decode_step(input_ids=toks[:, s - 1])[1].cpu().clone())
    return raw


@pytest.mark.parametrize("B,rules", [(1, None), (4, None), (32, None), (4, (1.3, 3, 2))])
def test_sampled_generation_meets_the_restatement_on_the_raw_logits(B, rules):
    """Sampling (0.8, 50, 0.95) through rdx_generate (captured step graph), then the same token path replayed on a plain context for every step's
    raw logits. Rules, warpers and the acceptance rule restated on those must give the run's scores bit for bit and admit its token at every (row, step)."""
    eng, cfg = _engine(B)
    try:
        ids, qf = _prompt(cfg, B)
        toks, scores, n = _gen(eng, ids, qf, SAMPLING, rules=rules)
        assert n == MAX_NEW
        greedy, _, _ = _gen(eng, ids, qf, None, rules=rules)
        assert not torch.equal(toks, greedy)                       # the draw is not the argmax everywhere
        raw = _raw_rows(eng, ids, qf, toks, MAX_NEW)
        hists = [ids[b].tolist() for b in range(B)]
        t, k, p, seed = SAMPLING
        for s in range(MAX_NEW):
            x = LR.apply_rules(raw[s], hists, [s] * B, rules, eos_id=-1)[0] if rules else raw[s]
            for b in range(B):
                want, kept, gap = SP.warp_row(x[b], t, k, p)
                diff = (_bits(scores[s][b]) != _bits(want)).nonzero()
                assert diff.numel() == 0, f"step {s} row {b}: scores differ from the restatement at ids {diff[:8].flatten().tolist()} (top-p gap {gap:.3e})"
                assert 1 <= int(kept.sum()) <= 50 + 150             # top_k = 50; the fp16 ties with the 50th value stay
                ok, why = SP.accepts(want, int(toks[b, s]), SP.u24(seed, b, s))
                assert ok, f"step {s} row {b}: outside the acceptance rule: {why}"
                hists[b].append(int(toks[b, s]))
    finally:
        eng.close()


def test_graph_replay_equals_eager_and_the_step_loop_with_eos_and_pad():
    B = 4
    eng, cfg = _engine(B)
    try:
        ids, qf = _prompt(cfg, B)
        free, _, _ = _gen(eng, ids, qf, SAMPLING)
        # an EOS id row 0 reaches: the first token from step 2 on that it has not emitted before; the path up to there does not depend on it
        first = [s for s in range(2, MAX_NEW) if int(free[0, s]) not in free[0, :s].tolist()]
        assert first, f"row 0 repeats itself from step 2 on: {free[0].tolist()}"
        eos = int(free[0, first[0]])
        tg, sg, ng = _gen(eng, ids, qf, SAMPLING, eos=eos, use_graph=True)
        te, se, ne = _gen(eng, ids, qf, SAMPLING, eos=eos, use_graph=False)
        t2, s2, n2 = _gen(eng, ids, qf, SAMPLING, eos=eos, use_graph=True)                 # the same seed twice
        assert ng == ne == n2 and torch.equal(tg, te) and torch.equal(tg, t2)
        assert torch.equal(_bits(sg), _bits(se)) and torch.equal(_bits(sg), _bits(s2))
        at = (tg[0] == eos).nonzero().flatten()
        assert int(at[0]) == first[0] and bool((tg[0, first[0] + 1:] == 0).all()), tg[0].tolist()
        assert torch.equal(tg[0, :first[0]], free[0, :first[0]])
        # rdx_prefill + rdx_decode_step, no EOS: the loop the caller drives equals rdx_generate, scores included
        toks, lg = eng.prefill(ids, qf, MAX_NEW, eos_id=-1, pad_id=0, sampling=SAMPLING)
        rows = [lg.cpu().clone()]
        for _ in range(1, MAX_NEW):
            rows.append(eng.decode_step()[1].cpu().clone())
        fs = _gen(eng, ids, qf, SAMPLING)[1]
        assert torch.equal(toks.cpu().long(), free)
        assert torch.equal(_bits(torch.stack(rows)), _bits(fs))
    finally:
        eng.close()


def test_a_new_seed_needs_no_new_graph_and_a_new_top_p_gets_one():
    """Back to back on one context with the same buffers, as the neutral-rules test does: a call that replayed a stale graph would repeat the previous
    call's warper arguments (top_p travels as a kernel argument) -- and a seed frozen into the graph would repeat its tokens (the seed is read from memory)."""
    B = 4
    eng, cfg = _engine(B)
    try:
        ids, qf = _prompt(cfg, B)
        t, k, p, seed = SAMPLING
        a_t, a_s, _ = _gen(eng, ids, qf, (t, k, p, seed))
        b_t, b_s, _ = _gen(eng, ids, qf, (t, k, p, seed + 1))
        b_eager_t, b_eager_s, _ = _gen(eng, ids, qf, (t, k, p, seed + 1), use_graph=False)
        assert torch.equal(b_t, b_eager_t) and torch.equal(_bits(b_s), _bits(b_eager_s))
        assert not torch.equal(a_t, b_t)
        c_t, c_s, _ = _gen(eng, ids, qf, (t, k, 0.5, seed + 1))
        c_eager_t, c_eager_s, _ = _gen(eng, ids, qf, (t, k, 0.5, seed + 1), use_graph=False)
        assert torch.equal(c_t, c_eager_t) and torch.equal(_bits(c_s), _bits(c_eager_s))
        assert int(torch.isfinite(c_s[1].float()).sum()) < int(torch.isfinite(b_s[1].float()).sum())       # p = 0.5 keeps fewer than p = 0.95
        # without a scores buffer the lm_head writes into the context's own rows: the same tokens, and the step timer replays that graph
        n_t, _, _ = _gen(eng, ids, qf, (t, k, 0.5, seed + 1), scores=False)
        assert torch.equal(n_t, c_t) and eng.time_unit(0, 2) > 0.0
    finally:
        eng.close()


def _top1_equals_greedy(eng, cfg, B):
    """top_k = 1 keeps the maximum's value group: with a single maximum the draw is the argmax whatever the random bits are. A row whose maximum is
    tied at some step (fp16 logits do tie) may leave the greedy path there, by one of the tied ids; up to that step it must be on it."""
    ids, qf = _prompt(cfg, B)
    g_t, g_s, _ = _gen(eng, ids, qf, None)
    s_t, s_s, _ = _gen(eng, ids, qf, (1.0, 1, 1.0, 99))
    tied = (g_s == g_s.float().max(dim=-1, keepdim=True).values.to(g_s.dtype)).sum(-1) > 1          # [step, row]
    whole = 0
    for b in range(B):
        at = tied[:, b].nonzero().flatten()
        upto = int(at[0]) if at.numel() else g_t.shape[1]
        whole += upto == g_t.shape[1]
        assert torch.equal(s_t[b, :upto], g_t[b, :upto]), f"B = {B} row {b}: top_k = 1 left the greedy path: {s_t[b].tolist()} != {g_t[b].tolist()}"
        for s in range(upto):
            kept = torch.isfinite(s_s[s, b].float())
            assert int(kept.sum()) == 1 and int(kept.nonzero()[0]) == int(g_t[b, s]) and s_s[s, b, g_t[b, s]] == g_s[s, b, g_t[b, s]]
        if upto < g_t.shape[1]:
            assert g_s[upto, b, s_t[b, upto]] == g_s[upto, b].float().max()
    assert whole * 2 >= B, f"only {whole} of {B} rows have untied maxima throughout"
    return ids, qf, g_t, g_s


def test_top_k_1_is_greedy_and_off_is_off_at_32_rows():
    eng, cfg = _engine(32)
    try:
        ids, qf, g_t, g_s = _top1_equals_greedy(eng, cfg, 32)
        # off again (rdx_set_sampling(NULL) behind a sampled call): the plain greedy tokens and scores
        assert eng.lib.rdx_set_sampling(eng.ctx, None) == 0
        o_t, o_s, _ = _gen(eng, ids, qf, None)
        assert torch.equal(o_t, g_t) and torch.equal(_bits(o_s), _bits(g_s))
    finally:
        eng.close()


def test_top_k_1_is_greedy_at_40_rows():
    """The row-block family (33-128 rows) needs the full widths; two layers keep it quick."""
    eng, cfg = _engine(40, cfg=RaDialogCfg(llama=LlamaCfg(layers=2, qformer_dim=192)))
    try:
        _top1_equals_greedy(eng, cfg, 40)
    finally:
        eng.close()


def test_top_k_1_is_greedy_through_generate_append():
    B = 2
    eng, cfg = _engine(B)
    try:
        ids, qf = _prompt(cfg, B)
        ids[B - 1] = ids[0].roll(1)                                # no padded row: the prefix is reusable
        outs = []
        for sampling in (None, (1.0, 1, 1.0, 5)):
            a, _, n = eng.generate(ids, qf, max_new=6, eos_id=-1, pad_id=0, output_scores=True, reuse_prefix=True, sampling=sampling)
            a = a[:, :n].cpu().long().clone()
            turn2 = torch.cat([ids, a, torch.full((B, 3), 11, dtype=torch.long)], dim=1)
            b, sc, m = eng.generate(turn2, qf, max_new=6, eos_id=-1, pad_id=0, output_scores=True, reuse_prefix=True, sampling=sampling)
            assert eng.last_kept_prefix > 0                        # rdx_generate_append ran
            outs.append((a, b[:, :m].cpu().long().clone()))
            eng._conv = None
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    finally:
        eng.close()


def test_beam_search_and_bad_parameters_are_refused_while_sampling():
    from radialog_amd._lib import RdxSampling
    B = 2
    eng, cfg = _engine(B)
    try:
        ids, qf = _prompt(cfg, B)
        lib, ctx, dev = eng.lib, eng.ctx, eng.device
        ids32 = ids[:1].repeat(2, 1).to(dev, torch.int32).contiguous()
        qf32 = qf[:1].repeat(2, 1, 1).to(dev, torch.float32).contiguous()
        host_t, host_l, n = torch.zeros(1, 4, dtype=torch.int32), torch.zeros(1, dtype=torch.int32), C.c_int(0)
        p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731

        def beam():
            torch.cuda.synchronize(dev)
            return lib.rdx_beam_search(ctx, p(ids32), None, 1, 2, T_PROMPT, p(qf32), 4, -1, 0, 1.0, 0, p(host_t), p(host_l), None, None, C.byref(n))

        assert lib.rdx_set_sampling(ctx, C.byref(RdxSampling(1, 0.8, 50, 0.95, 1))) == 0
        assert beam() == -1 and b"sampling" in lib.rdx_last_error(ctx)
        for bad in (RdxSampling(1, 0.0, 0, 1.0, 0), RdxSampling(1, -1.0, 0, 1.0, 0), RdxSampling(1, float("inf"), 0, 1.0, 0), RdxSampling(1, float("nan"), 0, 1.0, 0),
                    RdxSampling(1, 1.0, -1, 1.0, 0), RdxSampling(1, 1.0, 0, 0.0, 0), RdxSampling(1, 1.0, 0, 1.5, 0), RdxSampling(1, 1.0, 0, float("nan"), 0)):
            assert lib.rdx_set_sampling(ctx, C.byref(bad)) == -1
        assert beam() == -1                          # a refused call leaves the previous selection in force
        assert lib.rdx_set_sampling(ctx, C.byref(RdxSampling(0, -5.0, -5, 7.0, 0))) == 0        # do_sample == 0: off, whatever the rest holds
        assert beam() == 0
        eng.sync()
    finally:
        eng.close()


def test_generate_entry_point_samples():
    from radialog_amd.modeling_llama_imgemb import LlamaForCausalLM
    cfg = small_cfg()
    B, N = 2, 6
    lm = LlamaForCausalLM.from_pretrained(None, torch_dtype=torch.float16, cfg=cfg.llama, max_batch=B, max_len=128, synthetic=True).eval()
    lm.enable_sampling = True
    try:
        ids, qf = _prompt(cfg, B)
        kw = dict(input_ids=ids, qformer_embs=qf, max_new_tokens=N, eos_token_id=-1, pad_token_id=0, return_dict_in_generate=True, output_scores=True)
        out = lm.generate(do_sample=True, seed=7, **kw)
        assert out.sequences.shape == (B, T_PROMPT + N) and torch.equal(out.sequences[:, :T_PROMPT].cpu(), ids)
        assert len(out.scores) == N and all(s.shape == (B, cfg.llama.vocab) for s in out.scores)
        kept = torch.isfinite(torch.stack(out.scores).float()).sum(-1)
        assert bool((kept >= 1).all()) and bool((kept <= 50 + 150).all())                        # top_k = 50 by default (fp16 ties with the 50th stay)
        again = lm.generate(do_sample=True, seed=7, **kw)
        other = lm.generate(do_sample=True, seed=8, **kw)
        assert torch.equal(out.sequences, again.sequences) and not torch.equal(out.sequences, other.sequences)
        torch.manual_seed(3)
        a = lm.generate(do_sample=True, **kw).sequences
        torch.manual_seed(3)
        assert torch.equal(a, lm.generate(do_sample=True, **kw).sequences)
        greedy = lm.generate(**kw)
        assert bool(torch.isfinite(torch.stack(greedy.scores).float()).all())                    # and greedy is untouched
    finally:
        lm._engine.close()
