"""Prompt-lookup decoding on the GPU (include/rdx.h: rdx_set_lookup / rdx_generate_lookup; radialog_amd/csrc/lookup.hip, api_lookup.hip).

The contract is not "the tokens of generate()": a verify pass runs the <= 32-row prompt kernels, a plain step the chained batch-1 kernels, their logits differ in
rounding and the synthetic models' greedy margins do not always decide against that. What every call must satisfy instead (check_contracts):
  1. greedy under its own scores, exact: tokens[i] is the lowest-index argmax of scores[i];
  2. the scores are the model's: within LOGIT_TOL / PROD_TOL (tests/test_gpu_parity.py) of the oracle's teacher-forced logits on the call's own emitted prefix;
  3. the draft and accept logic, exact: the host restatement (tests/_lookup.py), given the emitted tokens, reproduces the returned trace and stats;
  4. a call in which no draft is ever found gives generate()'s tokens and scores bit for bit.
Seeds 40, 41 and 43 (small_cfg, T = 48, 24 steps): over their legs with corpus = generate()'s own output, accepted counts of 0 and of the full draft both occur."""
import ctypes as C

import numpy as np
import pytest
import torch

import _lookup as LK
from radialog_amd import synth
from radialog_amd.config import small_cfg
from test_gpu_parity import DT, LOGIT_TOL, PROD_TOL, _cpu_weights, _production_width_weights

pytestmark = pytest.mark.gpu

T, N, MAX_LEN = 48, 24, 128
SEEDS = (40, 41, 43)


@pytest.fixture(scope="module")
def cfg():
    return small_cfg()


@pytest.fixture(scope="module")
def cpu_w(cfg):
    return _cpu_weights(cfg)


def _engine(cfg, dtype, **kw):
    from radialog_amd.engine import RdxEngine, synth_getter
    vision = kw.pop("vision", False)
    eng = RdxEngine(cfg, dtype=dtype, device=0, max_batch=kw.pop("max_batch", 2), max_len=MAX_LEN, lora=True, vision=vision, **kw)
    eng.load_weights(synth_getter(cfg, eng.device, lora=True), vision=vision)
    return eng


@pytest.fixture(scope="module", params=["f16", "bf16"])
def engine(request, cfg):
    eng = _engine(cfg, request.param)
    yield eng
    eng.close()


def _prompt(cfg, seed, T_=T):
    ids = synth.synth_prompt_ids(1, T_, vocab=cfg.llama.vocab, img_offset=6, pad_rows=False, seed=seed)
    qf = synth.synth("t.lk.qf", (1, 32, cfg.llama.qformer_dim), -1.0, 1.0)
    return ids, qf


def _argmax_low(row):
    row = row.float()
    return int((row == row.max()).nonzero()[0])


def check_contracts(out, ids, qf, orc, rule, corpus, max_new, tol, eos=-1, what=""):
    """Contracts 1-3 on what one generate_lookup call returned; returns (emitted tokens, trace as tuples, worst |scores - oracle|)."""
    toks, scores, n, stats, trace = out
    S = toks[0, :n].cpu().tolist()
    assert scores.shape[0] == n
    got = [_argmax_low(scores[i, 0].cpu()) for i in range(n)]
    assert got == S, f"{what}: tokens are not the argmax of their own scores rows"
    with torch.no_grad():
        ref = orc.forced_logits(ids, qf, torch.tensor([S], dtype=torch.long))
    err = max(float((scores[i, 0].float().cpu() - ref[i][0].float()).abs().max()) for i in range(n))
    print(f"{what}: n {n}, |scores - oracle| {err:.4g} (bar {tol}), stats {stats}")
    assert err < tol, f"{what}: scores are {err} from the oracle's teacher-forced logits (bar {tol})"
    tr, st = LK.simulate(ids[0].tolist(), list(corpus or []), S, rule, max_new, eos)
    assert [tuple(r) for r in trace.tolist()] == tr, f"{what}: trace differs from the restatement"
    assert stats == st, (what, stats, st)
    return S, tr, err


def _rule(lk):
    return LK.Rule(lk.draft_len, lk.ngram_max, lk.ngram_min)


# ---- the kernel alone -------------------------------------------------------------------------------------------------------------------------------
def _partials(am, n_tiles=5, tie=None):
    """Argmax partials whose reduction gives am[r] for row r: one winning tile per row among smaller ones; tie = (row, other column): a second tile
    with the SAME value and a higher index, placed in front of the winner."""
    g = torch.Generator().manual_seed(7)
    pv = torch.rand(len(am), n_tiles, generator=g)
    pi = torch.randint(0, 200, (len(am), n_tiles), generator=g, dtype=torch.int32)
    for r, a in enumerate(am):
        pv[r, (r * 2 + 1) % n_tiles] = 2.0
        pi[r, (r * 2 + 1) % n_tiles] = a
    if tie is not None:
        r, other = tie
        assert other > am[r]
        t = (r * 2 + 1) % n_tiles
        pv[r, (t + n_tiles - 1) % n_tiles] = 2.0
        pi[r, (t + n_tiles - 1) % n_tiles] = other
    return pv, pi


def _run_kernel(eng, am, tail, state, hist, rule, corpus=(), eos=-1, max_new=64, slot_end=1 << 20, tie=None, advance=True, logits=None):
    from radialog_amd.engine import Lookup
    pv, pi = _partials(am, tie=tie)
    h = torch.zeros(MAX_LEN, dtype=torch.int32)
    h[: len(hist)] = torch.tensor(hist, dtype=torch.int32)
    got = eng.lookup_accept_test(pv, pi, len(tail) - 1, tail, h, len(hist), state, Lookup(rule.draft_len, rule.ngram_max, rule.ngram_min), corpus=list(corpus),
                                 slot_end=slot_end, advance=advance, eos_id=eos, pad_id=0, max_new=max_new, logits=logits, fwd=2)
    want = LK.accept_step(am, tail, state, hist, corpus, rule, max_new, slot_end, eos_id=eos, pad_id=0, advance=advance)
    step = state[0]
    n = len(want["emitted"])
    out = got["out_tokens"].tolist()
    assert out[step:step + n] == want["emitted"] and out[:step] == [-7] * step, (out[:step + n + 2], want)
    if want["eos"]:
        assert out[step + n:] == [0] * (max_new - step - n)              # pads behind an EOS
    else:
        assert out[step + n:] == [-7] * (max_new - step - n)
    st = got["state"].tolist()
    assert tuple(st[:3]) == want["state"][:3] and st[4] == len(want["hist"])
    if eos >= 0:
        assert st[3] == want["state"][3]
    assert got["hist"].tolist()[: len(want["hist"])] == want["hist"]
    d2 = len(want["tail"]) - 1
    assert got["tail"].tolist()[: d2 + 1] == want["tail"]
    assert got["status"].tolist()[:2] == [d2 | (int(want["finished"]) << 8), want["state"][1]]
    assert got["pos_ids"].tolist()[: d2 + 1] == [want["state"][2] + i for i in range(d2 + 1)]
    if advance:
        assert got["status"].tolist()[2] == 3 and got["trace"][2].tolist() == [len(tail) - 1, want["accepted"]]
    return got, want


def test_accept_kernel_alone_every_accepted_count(engine):
    rule = LK.Rule(8, 3, 1)
    rng = np.random.default_rng(3)
    hist = rng.integers(1, 9, 17).tolist()
    for d in (1, 3, 7, 15):
        for acc in sorted({0, 1, d - 1, d}):
            draft = [20 + i for i in range(d)]
            am = draft[:acc] + [99] + [50 + i for i in range(d - acc)]          # row acc disagrees (or is the pass's own token), later rows are ignored
            _run_kernel(engine, am, [hist[-1]] + draft, (3, 60, 55, 1), hist, rule)


def test_accept_kernel_alone_tie_eos_and_scores(engine):
    rule = LK.Rule(4, 2, 1)
    hist = [1, 2, 3, 4, 1, 2]
    draft = [3, 4, 1]
    # a tie between two columns of one row: the lower index is the row's token, so draft_2 = 4 is accepted
    _run_kernel(engine, [3, 4, 7, 8], [2] + draft, (0, 10, 10, 1), hist, rule, tie=(1, 150))
    # an EOS at the first, a middle and the last emitted position
    for k in (0, 1, 3):
        am = [3, 4, 1, 9]
        eos = am[k]
        _, want = _run_kernel(engine, am, [2] + draft, (5, 20, 18, 1), hist, rule, eos=eos)
        assert len(want["emitted"]) == k + 1 and want["finished"]
    # the token-0 form: no state advance but the step count, no forward recorded
    _run_kernel(engine, [6], [0], (0, 30, 25, 1), hist, rule, advance=False)
    # the emitted rows of the pass's logits land at the emitted steps
    V = engine.cfg.llama.vocab
    lg = torch.randn(4, V).to(DT[engine.dtype])
    got, want = _run_kernel(engine, [3, 4, 7, 8], [2] + draft, (2, 10, 10, 1), hist, rule, logits=lg)
    n = len(want["emitted"])
    assert n == 3
    sc = got["scores"].view(torch.int16)
    assert torch.equal(sc[2:2 + n], lg[:n].view(torch.int16)) and not sc[:2].any() and not sc[2 + n:].any()


def test_accept_kernel_alone_histories_where_many_ngrams_match(engine):
    rng = np.random.default_rng(11)
    for L in (1, 17, MAX_LEN - 1):
        for rule in (LK.Rule(15, 3, 1), LK.Rule(5, 8, 2), LK.Rule(3, 1, 1)):
            hist = rng.integers(1, 9, L).tolist()
            corpus = rng.integers(1, 9, 40).tolist() if L != 17 else []
            # (one emitted token: the history of max_len - 1 entries has room for exactly one more)
            _, want = _run_kernel(engine, [int(rng.integers(1, 9)), 5], [hist[-1], 30], (1, L, L, 1), hist, rule, corpus=corpus)
            _run_kernel(engine, [int(rng.integers(1, 9))], [hist[-1]], (1, L, L, 1), hist, rule, corpus=corpus, slot_end=L + 3)      # the slot bound clips the draft
    # budget: max_new - emitted - 1 tokens may still be drafted
    hist = [1, 2, 3, 4, 5, 6, 7, 8, 1]
    _, want = _run_kernel(engine, [2], [1], (10, 9, 9, 1), hist, LK.Rule(8, 1, 1), max_new=14)
    assert want["tail"] == [2, 3, 4]
    _, want = _run_kernel(engine, [2], [1], (12, 9, 9, 1), hist, LK.Rule(8, 1, 1), max_new=14)
    assert want["tail"] == [2] and not want["finished"]


# ---- contracts 1-3 with injected drafts -------------------------------------------------------------------------------------------------------------
def test_contracts_with_injected_drafts(engine, cfg, cpu_w):
    from oracle import ref_cpu
    from radialog_amd.engine import Lookup
    orc = ref_cpu.LlamaOracle(cpu_w, cfg.llama, DT[engine.dtype], lora=True)
    tol = LOGIT_TOL[engine.dtype]
    zero = full = 0
    for seed in SEEDS:
        ids, qf = _prompt(cfg, seed)
        t0, _, n0 = engine.generate(ids, qf, max_new=N, eos_id=-1)
        S0 = t0[0, :n0].cpu().tolist()
        corrupt = [t if i % 4 else (t + 1) % 1000 + 1 for i, t in enumerate(S0)]
        unrelated = [(7 * i + 3) % 500 + 1000 for i in range(30)]
        for dl in (3, 7, 15):
            lk = Lookup(dl, 3, 1)
            for name, corpus in (("S0", S0), ("corrupted", corrupt), ("unrelated", unrelated)):
                out = engine.generate_lookup(ids, qf, max_new=N, eos_id=-1, lookup=lk, corpus=corpus, output_scores=True)
                assert out[2] == N
                _, tr, _ = check_contracts(out, ids, qf, orc, _rule(lk), corpus, N, tol, what=f"{engine.dtype} seed {seed} draft_len {dl} corpus {name}")
                if name == "S0":
                    zero += sum(1 for d, a in tr if d > 0 and a == 0)
                    full += sum(1 for d, a in tr if d > 0 and a == d)
    assert zero > 0 and full > 0, f"corpus = S0 legs: {zero} passes accepted nothing, {full} their whole draft; both must occur"


def test_natural_drafts_across_cache_groups(engine, cfg, cpu_w):
    from oracle import ref_cpu
    from radialog_amd.engine import Lookup
    orc = ref_cpu.LlamaOracle(cpu_w, cfg.llama, DT[engine.dtype], lora=True)
    ids, qf = _prompt(cfg, 44)
    ids[0, 40:43] = ids[0, 44:47] = torch.tensor([11, 12, 13])          # a repeated 3-gram behind the image block
    lk = Lookup(7, 3, 1)
    out = engine.generate_lookup(ids, qf, max_new=40, eos_id=-1, lookup=lk, output_scores=True)      # slots 48 .. 87: three 16-position K-cache groups
    check_contracts(out, ids, qf, orc, _rule(lk), None, 40, LOGIT_TOL[engine.dtype], what=f"{engine.dtype} natural")
    assert out[2] == 40 and out[3]["drafted"] > 0


def test_production_width_one_layer():
    from oracle import ref_cpu
    from radialog_amd.engine import Lookup
    pcfg, pw = _production_width_weights(1)
    ids = synth.synth_prompt_ids(1, 96, vocab=pcfg.llama.vocab, img_offset=6, pad_rows=False, seed=5)
    qf = synth.synth("t.lk.qfp", (1, 32, pcfg.llama.qformer_dim), -1.0, 1.0)
    for dtype in ("bf16", "f16"):
        eng = _engine(pcfg, dtype, max_batch=1)
        orc = ref_cpu.LlamaOracle(pw, pcfg.llama, DT[dtype], lora=True)
        t0, _, n0 = eng.generate(ids, qf, max_new=12, eos_id=-1)
        S0 = t0[0, :n0].cpu().tolist()
        for lk, corpus in ((Lookup(7, 3, 1), S0), (Lookup(15, 3, 1), [t if i % 4 else 5 for i, t in enumerate(S0)])):
            out = eng.generate_lookup(ids, qf, max_new=12, eos_id=-1, lookup=lk, corpus=corpus, output_scores=True)
            check_contracts(out, ids, qf, orc, _rule(lk), corpus, 12, PROD_TOL[dtype], what=f"production width {dtype} draft_len {lk.draft_len}")
            assert out[3]["passes"] > 0
        eng.close()


# ---- bounds, EOS, contract 4, the state the call leaves ---------------------------------------------------------------------------------------------
def test_full_cache_row_no_slot_beyond_max_len(engine, cfg, cpu_w):
    from oracle import ref_cpu
    from radialog_amd.engine import Lookup
    orc = ref_cpu.LlamaOracle(cpu_w, cfg.llama, DT[engine.dtype], lora=True)
    ids, qf = _prompt(cfg, 41)
    M = MAX_LEN - T                                                  # T + max_new == max_len
    t0, _, _ = engine.generate(ids, qf, max_new=M, eos_id=-1)
    S0 = t0[0].cpu().tolist()
    # row 1 of the cache (the rows behind row 0's last slot) holds a pattern that must survive
    H, D = cfg.llama.heads, 128
    poison = torch.full((2, H, MAX_LEN, D), 3.25, dtype=DT[engine.dtype])
    for which in (0, 1):
        engine.kv_write_test(0, which, poison)
    lk = Lookup(15, 3, 1)
    out = engine.generate_lookup(ids, qf, max_new=M, eos_id=-1, lookup=lk, corpus=S0, output_scores=True)
    S, tr, _ = check_contracts(out, ids, qf, orc, _rule(lk), S0, M, LOGIT_TOL[engine.dtype], what=f"{engine.dtype} full row")
    assert out[2] == M and len(S) == M and max(d for d, _ in tr) == 15
    assert sum((a + 1) for _, a in tr) == M - 1                      # the forwards emit exactly up to max_new
    for which in (0, 1):
        kv = engine.kv_read(0, which, 2)
        assert bool((kv[1].float() == 3.25).all()), "a cache slot at or beyond max_len of row 0 was written"


def test_eos_inside_an_accepted_run(engine, cfg, cpu_w):
    from oracle import ref_cpu
    from radialog_amd.engine import Lookup
    orc = ref_cpu.LlamaOracle(cpu_w, cfg.llama, DT[engine.dtype], lora=True)
    ids, qf = _prompt(cfg, 40)
    t0, _, _ = engine.generate(ids, qf, max_new=N, eos_id=-1)
    S0 = t0[0].cpu().tolist()
    lk = Lookup(7, 3, 1)
    out = engine.generate_lookup(ids, qf, max_new=N, eos_id=-1, lookup=lk, corpus=S0, output_scores=True)
    S, tr, _ = check_contracts(out, ids, qf, orc, _rule(lk), S0, N, LOGIT_TOL[engine.dtype], what="eos base")
    # a position strictly inside an accepted run whose token has not occurred before
    k, pos = None, 1
    for d, a in tr:
        for j in range(1, a):                                        # draft j + 1 of the pass, not the last accepted one
            if k is None and S[pos + j] not in S[:pos + j] and S[pos + j] not in ids[0].tolist():
                k = pos + j
        pos += a + 1
    assert k is not None, (S, tr)
    out = engine.generate_lookup(ids, qf, max_new=N, eos_id=S[k], pad_id=0, lookup=lk, corpus=S0, output_scores=True)
    toks, _, n, _, trace = out
    assert n == k + 1 and toks[0, :n].cpu().tolist() == S[:k + 1] and toks[0, n:].cpu().tolist() == [0] * (N - n)
    check_contracts(out, ids, qf, orc, _rule(lk), S0, N, LOGIT_TOL[engine.dtype], eos=S[k], what="eos inside a run")
    # the state the call leaves: one decode step gives the model's logits for position n, and generate(reuse_prefix) continues the conversation
    _, lg = engine.decode_step(want_logits=True)
    with torch.no_grad():
        ref = orc.forced_logits(ids, qf, torch.tensor([S[:n] + [0]], dtype=torch.long))
    err = float((lg[0].float().cpu() - ref[n][0].float()).abs().max())
    assert err < LOGIT_TOL[engine.dtype], err


def test_generate_append_continues_the_conversation(engine, cfg):
    from radialog_amd.engine import Lookup
    ids, qf = _prompt(cfg, 43)
    t0, _, _ = engine.generate(ids, qf, max_new=N, eos_id=-1)
    toks, _, n, _, _ = engine.generate_lookup(ids, qf, max_new=N, eos_id=-1, lookup=Lookup(7, 3, 1), corpus=t0[0].cpu().tolist())
    turn2 = torch.cat([ids, toks[:, :n - 1].cpu().long(), torch.tensor([[17, 23, 5, 9]])], dim=1)
    a, sa, na = engine.generate(turn2, qf, max_new=6, eos_id=-1, output_scores=True, reuse_prefix=True)
    assert engine.last_kept_prefix == T + n - 1
    a, sa = a.cpu().clone(), sa.float().cpu().clone()
    b, sb, nb = engine.generate(turn2, qf, max_new=6, eos_id=-1, output_scores=True)
    err = float((sa - sb.float().cpu()).abs().max())
    assert err < 2 * LOGIT_TOL[engine.dtype], err                    # the kept rows came from passes and plain steps, the recomputed ones from one prompt


def test_no_drafts_means_generate_bit_for_bit(engine, cfg):
    from radialog_amd.engine import Lookup
    g = torch.Generator().manual_seed(5)
    ids = (torch.randperm(900, generator=g)[:T] + 1).view(1, T)      # distinct ids, no image block, no pad
    # 8-grams only: until 8 tokens are out the last 8 of H hold a (distinct) prompt token, and then the call is over -- no repeat in H is that long
    lk, M = Lookup(8, 8, 8), 8
    t0, s0, n0 = engine.generate(ids, None, max_new=M, eos_id=-1, output_scores=True)
    t0, s0 = t0.cpu().clone(), s0.cpu().view(torch.int16).clone()
    tr, st = LK.simulate(ids[0].tolist(), [], t0[0].tolist(), _rule(lk), M)
    assert st["drafted"] == 0 and len(tr) == M - 1, "the restatement must find no draft for this prompt"
    toks, sc, n, stats, trace = engine.generate_lookup(ids, None, max_new=M, eos_id=-1, lookup=lk, output_scores=True)
    assert n == n0 == M and stats == st and trace.tolist() == [[0, 0]] * (M - 1)
    assert torch.equal(toks.cpu(), t0) and torch.equal(sc.cpu().view(torch.int16), s0)


def test_option_off_leaves_generate_as_on_a_context_that_never_had_it(cfg):
    from radialog_amd.engine import Lookup
    ids, qf = _prompt(cfg, 41)
    a, b = _engine(cfg, "bf16", max_batch=1), _engine(cfg, "bf16", max_batch=1)
    a.generate_lookup(ids, qf, max_new=N, eos_id=-1, lookup=Lookup(7, 3, 1), corpus=[1, 2, 3], output_scores=True)
    a.set_lookup(None)
    ta, sa, _ = a.generate(ids, qf, max_new=N, eos_id=-1, output_scores=True)
    tb, sb, _ = b.generate(ids, qf, max_new=N, eos_id=-1, output_scores=True)
    assert torch.equal(ta.cpu(), tb.cpu()) and torch.equal(sa.cpu().view(torch.int16), sb.cpu().view(torch.int16))
    a.close()
    b.close()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------------
def _raw(eng, ids, max_new, B=1, T_=None):
    """rdx_generate_lookup itself (the engine's wrapper switches rules, sampling and logprobs off first): (rc, message)."""
    ids32 = ids.to(device=eng.device, dtype=torch.int32).contiguous()
    toks = torch.zeros(max(B, 1), max(max_new, 1), dtype=torch.int32, device=eng.device)
    n, stats = C.c_int(0), (C.c_int * 3)()
    torch.cuda.synchronize(eng.device)
    rc = eng.lib.rdx_generate_lookup(eng.ctx, C.c_void_p(ids32.data_ptr()), None, B, ids.shape[1] if T_ is None else T_, None, None, 0, max_new, -1, 0,
                                     C.c_void_p(toks.data_ptr()), None, C.byref(n), stats, None, 0)
    return rc, (eng.lib.rdx_last_error(eng.ctx) or b"").decode()


def test_refusals_name_their_cause_and_leave_the_conversation(engine, cfg):
    from radialog_amd.engine import Lookup
    ids, _ = _prompt(cfg, 40)
    ids[ids == 32000] = 77
    ref, _, _ = engine.generate(ids, None, max_new=10, eos_id=-1)
    ref = ref[0].cpu().tolist()
    engine.set_lookup(None)
    assert _raw(engine, ids, 8)[0] == -1 and "rdx_set_lookup" in _raw(engine, ids, 8)[1]
    engine.set_lookup(Lookup(4, 3, 1))
    toks, _ = engine.prefill(ids, None, max_new=10, eos_id=-1, want_logits=False)
    two = torch.cat([ids, ids])
    for what, rc_msg in (("batch", _raw(engine, two, 8, B=2)), ("max_len", _raw(engine, ids, MAX_LEN - T + 1)), ("max_new", _raw(engine, ids, 0))):
        assert rc_msg[0] == -1 and what in rc_msg[1], (what, rc_msg)
        engine.decode_step(want_logits=False)                        # the previous conversation still decodes
    engine.sync()
    assert toks[0, :4].cpu().tolist() == ref[:4]
    # options that refuse: each is set, a conversation starts under it, the call is refused, the conversation goes on
    for what, kw in (("logits rules", dict(logits_rules=(1.3, 0, 0))), ("sampling", dict(sampling=(0.8, 5, 1.0, 1))), ("logprobs", dict(logprobs=2))):
        engine.prefill(ids, None, max_new=10, eos_id=-1, want_logits=False, **kw)
        rc, msg = _raw(engine, ids, 8)
        assert rc == -1 and what in msg, (what, rc, msg)
        engine.decode_step(want_logits=False)
    engine.set_logits_rules(None), engine.set_sampling(None), engine.set_logprobs(None)
    with engine.row_session(1, 1, 8, eos_id=-1):
        rc, msg = _raw(engine, ids, 8)
        assert rc == -1 and "row session" in msg, msg
    with pytest.raises(ValueError):
        engine.set_lookup((16, 3, 1))
    for bad in ((4, 9, 1), (4, 2, 3)):
        lk = __import__("radialog_amd._lib", fromlist=["RdxLookup"]).RdxLookup(*bad)
        assert engine.lib.rdx_set_lookup(engine.ctx, C.byref(lk)) == -1
    # beam search and row sessions do not look at the option
    engine.beam_search(ids, None, num_beams=2, max_new=4, eos_id=-1)
    out = engine.generate_lookup(ids, None, max_new=10, eos_id=-1, lookup=Lookup(4, 3, 1), output_scores=True)
    assert out[2] == 10


@pytest.mark.parametrize("kw,what", [(dict(kv_fp8=True), "kv_fp8"), (dict(weights_fp8=True), "fp8-weight")])
def test_fp8_contexts_refuse(cfg, kw, what):
    from radialog_amd.engine import Lookup
    eng = _engine(cfg, "bf16", max_batch=1, **kw)
    ids, _ = _prompt(cfg, 40)
    ids[ids == 32000] = 77
    eng.set_lookup(Lookup(4, 3, 1))
    toks, _ = eng.prefill(ids, None, max_new=6, eos_id=-1, want_logits=False)
    rc, msg = _raw(eng, ids, 6)
    assert rc == -1 and what in msg, (rc, msg)
    eng.decode_step(want_logits=False)
    from radialog_amd.modeling_llama_imgemb import LlamaForCausalLM
    lm = LlamaForCausalLM.from_pretrained(None, torch_dtype=torch.bfloat16, synthetic=True, **kw)
    with pytest.raises(ValueError, match="fp8"):
        lm.generate(input_ids=ids, max_new_tokens=4, prompt_lookup_num_tokens=4)
    eng.close()


# ---- int4 weights -----------------------------------------------------------------------------------------------------------------------------------
def test_int4_weight_engine(cfg, cpu_w):
    """The plain steps stream int4, the passes multiply the packed W': the same weights, so the contracts hold against the oracle on W'."""
    from oracle import ref_cpu
    from radialog_amd import w4
    from radialog_amd.engine import Lookup
    proj = tuple(f"{p}_proj.weight" for p in ("q", "k", "v", "o", "gate", "up", "down"))
    wq = {k: (torch.from_numpy(w4.dequantize(w4.quantize(v.float().numpy()))) if k.endswith(proj) else v) for k, v in cpu_w.items()}
    eng = _engine(cfg, "bf16", max_batch=1, weights_w4=True)
    orc = ref_cpu.LlamaOracle(wq, cfg.llama, torch.bfloat16, lora=True)
    ids, qf = _prompt(cfg, 41, T_=40)
    t0, _, _ = eng.generate(ids, qf, max_new=12, eos_id=-1)
    S0 = t0[0].cpu().tolist()
    lk = Lookup(7, 3, 1)
    out = eng.generate_lookup(ids, qf, max_new=12, eos_id=-1, lookup=lk, corpus=S0, output_scores=True)
    check_contracts(out, ids, qf, orc, _rule(lk), S0, 12, LOGIT_TOL["bf16"], what="int4 weights")
    assert out[3]["passes"] > 0
    eng.close()
