"""Generation log-probs on the GPU (include/rdx.h: rdx_set_logprobs / rdx_get_logprobs; radialog_amd/csrc/logprob.hip).

1. logprob_step_k alone through rdx_logprob_step_test, on the inputs of tests/_logprobs.py (tests/test_logprobs_host.py holds an fp32 emulation of the kernel's
   order inside the bar on them, and four planted faults outside it): every entry within the DERIVED bar of the float64 restatement, the ids exactly, the same
   bits on a second launch, and nothing written outside the entries the launch describes.
2. Inside the step, for every decode family: the entries equal the restatement applied to the scores and tokens the same call returned; tokens and scores
   are bit for bit those of the option off; the log-probs are bit for bit the same with and without a scores buffer and with and without the graph. The same
   under logits rules and sampling, on the single-step calls, behind a kept prefix, on an fp8 KV cache and on int4 weights.
3. EOS: the device entries behind a row's EOS describe the pad token, the Python layer masks them. 4. Refusals."""
import ctypes as C

import pytest
import torch

import _logprobs as L
from radialog_amd import synth
from radialog_amd.config import LlamaCfg, RaDialogCfg, small_cfg

pytestmark = pytest.mark.gpu

DT = {"f16": torch.float16, "bf16": torch.bfloat16}
N_NEW, T_PROMPT = 6, 72


def _cfg(which):
    return small_cfg() if which == "small" else RaDialogCfg(llama=LlamaCfg(layers=2, qformer_dim=192))       # "prod2": two layers at the production width


def _engine(which, dtype, max_batch, **kw):
    from radialog_amd.engine import RdxEngine, synth_getter
    cfg = _cfg(which)
    eng = RdxEngine(cfg, dtype=dtype, device=0, max_batch=max_batch, max_len=128, lora=True, vision=False, **kw)
    eng.load_weights(synth_getter(cfg, eng.device, lora=True), vision=False)
    return eng


def _prompt(cfg, B, T=T_PROMPT):
    ids = synth.synth_prompt_ids(B, T, vocab=cfg.llama.vocab, img_offset=6, pad_rows=False, seed=33)
    if B > 1:                                  # left-pad row 1 by 5 (pad id 0), keep 32 <IMG> inside
        ids[1] = torch.cat([torch.zeros(5, dtype=torch.long), ids[1, : T - 5]])
    return ids, synth.synth("t.qf2", (B, 32, cfg.llama.qformer_dim), -1.0, 1.0)


def _last_error(eng):
    return (eng.lib.rdx_last_error(eng.ctx) or b"").decode()


@pytest.fixture(scope="module", params=["f16", "bf16"])
def small_engine(request):
    eng = _engine("small", request.param, 3)
    yield eng
    eng.close()


# ---- 1. the kernel alone ----------------------------------------------------------------------------------------------------------------------------------
_WANT = {}


def _kernel_want(B, V, dtype):
    """The case and its float64 restatement at top_n = 8 (a smaller top_n is its prefix), computed once per case."""
    key = (B, V, dtype)
    if key not in _WANT:
        xp, tok = L.kernel_case(B, V, DT[dtype])
        x = xp[:, :V]
        ids = L.top_ids(x, 8)
        _WANT[key] = (xp, tok, L.chosen(x, tok), ids, L.top_lp(x, ids), L.logprob_bar(x, tok), L.logprob_bar(x, ids))
    return _WANT[key]


@pytest.mark.parametrize("B,V", L.KERNEL_CASES)
def test_logprob_step_kernel_alone(small_engine, B, V):
    eng = small_engine
    xp, tok, w_c, w_i, w_l, b_c, b_l = _kernel_want(B, V, eng.dtype)
    ds = L.d_steps(B)
    step = ds.long() - 1
    live = step < L.MAX_NEW                                                          # the other rows stand at step == max_new: nothing may be written
    tokens = ((tok + 1) % V).view(B, 1).repeat(1, L.MAX_NEW)                         # a wrong token wherever the kernel must not look
    tokens[live, step[live]] = tok[live]
    out_ld = L.MAX_NEW + 1
    for strided in (False, True):
        buf, rs, ss = L.lay_out(xp, V, strided, offset=3 if strided else 0)
        for top_n in (0, 1, 8):
            label = f"logprob_step_k B={B} V={V} {eng.dtype} {'per-step rows' if strided else 'fixed rows'} top_n={top_n}"
            got = [t.cpu() for t in eng.logprob_step_test(buf, ds, tokens, V, top_n, row_stride=rs, step_stride=ss, out_ld=out_ld, offset=3 if strided else 0)]
            again = [t.cpu() for t in eng.logprob_step_test(buf, ds, tokens, V, top_n, row_stride=rs, step_stride=ss, out_ld=out_ld, offset=3 if strided else 0)]
            c, i, l = got
            rows = torch.arange(B)[live]
            gc, gi, gl = c[rows, step[live]], i[rows, step[live]].long(), l[rows, step[live]]
            ok_c = L.within(gc, w_c[live], b_c[live])
            ok_l = L.within(gl[:, :top_n], w_l[live][:, :top_n], b_l[live][:, :top_n])
            over = ((gc.double() - w_c[live]).abs() - b_c[live]).nan_to_num(nan=0.0, posinf=0.0, neginf=0.0)
            print(f"{label}: worst |chosen - fp64| - bar = {float(over.max()):.3g}, largest bar {float(b_c.max()):.3g}")
            assert bool(ok_c.all()), f"{label}: chosen of rows {rows[~ok_c].tolist()[:8]} leaves the derived bar"
            assert bool(ok_l.all()), f"{label}: top log-probs of rows {rows[~ok_l.all(dim=1)].tolist()[:8]} leave the derived bar"
            assert torch.equal(gi[:, :top_n], w_i[live][:, :top_n]), f"{label}: top ids differ"
            # everything else is canary: other steps, step == max_new, the rows at or beyond max_new, slots >= top_n, the guard rows behind row B - 1
            written = torch.zeros(c.shape, dtype=torch.bool)
            written[rows, step[live]] = True
            assert bool(torch.isnan(c[~written]).all()), f"{label}: chosen written outside the launch's entries"
            slot = written.unsqueeze(-1) & (torch.arange(8) < top_n)
            assert bool((i[~slot] == -7).all()) and bool(torch.isnan(l[~slot]).all()), f"{label}: top entries written outside the launch's"
            for a, b in zip(got, again):                                             # the same bits on a second launch
                assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{label}: a second launch gives other bits"


def test_kernel_hook_refusals(small_engine):
    eng = small_engine
    x = torch.zeros(2, 16, dtype=DT[eng.dtype], device=eng.device)
    ds = torch.ones(2, dtype=torch.int32, device=eng.device)
    tk = torch.zeros(2, 2, dtype=torch.int32, device=eng.device)
    c = torch.zeros(2, 2, device=eng.device)
    i = torch.zeros(2, 2, 8, dtype=torch.int32, device=eng.device)
    l = torch.zeros(2, 2, 8, device=eng.device)
    p = lambda t: C.c_void_p(t.data_ptr())                                           # noqa: E731
    call = lambda V, top_n, ld: eng.lib.rdx_logprob_step_test(eng.ctx, p(x), 16, 0, p(ds), p(tk), 2, V, 2, top_n, p(c), p(i), p(l), ld)        # noqa: E731
    assert call(16, 9, 2) == -1 and call(16, -1, 2) == -1 and call(16, 2, 1) == -1 and call(100000, 2, 2) == -1
    assert call(16, 2, 2) == 0


# ---- 2. inside the step -----------------------------------------------------------------------------------------------------------------------------------
def _bits_equal(a, b):
    return all(torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32)) for x, y in zip(a, b))


def _check_entries(lp, scores, toks, n, k, label):
    """The call's log-probs against the restatement applied to the scores and tokens the SAME call returned: every (row, step)."""
    w_c, w_i, w_l, b_c, b_l = L.entries(scores[:n], toks, k)
    c, i, l = lp
    assert tuple(c.shape) == tuple(w_c.shape) and tuple(i.shape) == tuple(w_i.shape) and tuple(l.shape) == tuple(w_l.shape), label
    ok_c, ok_l = L.within(c, w_c, b_c), L.within(l, w_l, b_l)
    over = ((c.double() - w_c).abs() - b_c).nan_to_num(nan=0.0, posinf=0.0, neginf=0.0)
    print(f"{label}: worst |chosen - fp64| - bar = {float(over.max()):.3g} over {c.numel()} entries, mean chosen log-prob {float(c.mean()):.3f}")
    assert bool(ok_c.all()), f"{label}: chosen leaves the bar at (row, step) {ok_c.logical_not().nonzero().tolist()[:6]}"
    assert torch.equal(i.long(), w_i), f"{label}: top ids differ at {(i.long() != w_i).nonzero().tolist()[:6]}"
    assert bool(ok_l.all()), f"{label}: top log-probs leave the bar at {ok_l.logical_not().nonzero().tolist()[:6]}"
    if k:                                                                             # consistency: descending, and the chosen token's entry equals its slot's
        assert bool((l[..., :-1] >= l[..., 1:]).all())


def _step_checks(eng, ids, qf, label, **how):
    """One configuration (greedy, rules or sampling): option off, then on in the four forms -- (scores, graph), (no scores, graph), (scores, eager), (no
    scores, eager) -- and with top_n 0."""
    gen = lambda **kw: eng.generate(ids, qf, max_new=N_NEW, eos_id=-1, **how, **kw)       # noqa: E731
    toks0, sc0, n0 = gen(output_scores=True)
    toks0, sc0 = toks0.clone(), sc0.clone()
    assert n0 == N_NEW
    toks1, sc1, n1, lp1 = gen(output_scores=True, logprobs=8)
    assert n1 == N_NEW and torch.equal(toks1, toks0) and torch.equal(sc1.view(torch.int16), sc0.view(torch.int16)), f"{label}: the option moves tokens or scores"
    _check_entries(lp1, sc1.cpu(), toks1.cpu(), n1, 8, label)
    for kw in (dict(), dict(output_scores=True, use_graph=False), dict(use_graph=False)):
        toks2, _, n2, lp2 = gen(logprobs=8, **kw)
        assert n2 == N_NEW and torch.equal(toks2, toks0), f"{label} {kw}: tokens differ"
        assert _bits_equal(lp2, lp1), f"{label} {kw}: log-probs differ in bits from the (scores, graph) form"
    toks3, _, _, lp3 = gen(logprobs=0)
    assert torch.equal(toks3, toks0) and tuple(lp3[1].shape) == (ids.shape[0], N_NEW, 0) and torch.equal(lp3[0].view(torch.int32), lp1[0].view(torch.int32))
    toks4, sc4, _ = gen(output_scores=True)                                            # and off again: the three-tuple, the same bits
    assert torch.equal(toks4, toks0) and torch.equal(sc4.view(torch.int16), sc0.view(torch.int16))
    return toks0, lp1


@pytest.mark.parametrize("B", [1, 3, 12, 17, 40])
def test_logprobs_inside_the_step_of_every_family(B):
    """1: chained, 3 and 12: the one-row-tile family, 17: the 32-row family, 40: the row blocks. At 3 rows also under logits rules and under sampling."""
    eng = _engine("prod2", "bf16", B)
    try:
        ids, qf = _prompt(eng.cfg, B)
        _step_checks(eng, ids, qf, f"prod2 bf16 B={B} greedy")
        if B == 3:
            _step_checks(eng, ids, qf, "prod2 bf16 B=3 rules (1.3, 2, 0)", logits_rules=(1.3, 2, 0))
            _, lp = _step_checks(eng, ids, qf, "prod2 bf16 B=3 sampling (0.8, 5, 0.9)", sampling=(0.8, 5, 0.9, 1234))
            # the warped row keeps 5 columns (more only where values tie at the fifth): dropped ones (-inf, lowest index first) close a top-8, with log-prob -inf
            assert bool((lp[2][..., 7] == float("-inf")).any()) and bool(torch.isfinite(lp[2][..., 0]).all()) and bool(torch.isfinite(lp[0]).all())
            _step_checks(eng, ids, qf, "prod2 bf16 B=3 rules + sampling", logits_rules=(1.2, 3, 2), sampling=(1.0, 0, 0.95, 7))
    finally:
        eng.close()


@pytest.mark.parametrize("B,dtype", [(1, "f16"), (32, "bf16")])
def test_logprobs_at_production_width(B, dtype):
    eng = _engine("prod2", dtype, B)
    try:
        ids, qf = _prompt(eng.cfg, B)
        _step_checks(eng, ids, qf, f"prod2 {dtype} B={B} greedy")
    finally:
        eng.close()


@pytest.mark.parametrize("kw", [dict(kv_fp8=True), dict(weights_w4=True)], ids=["kv_fp8", "weights_w4"])
def test_logprobs_on_the_fp8_kv_cache_and_on_int4_weights(kw):
    eng = _engine("prod2", "bf16", 3, **kw)
    try:
        ids, qf = _prompt(eng.cfg, 3)
        _step_checks(eng, ids, qf, f"prod2 bf16 B=3 {kw}")
    finally:
        eng.close()


def test_single_step_calls_and_unwritten_entries(small_engine):
    eng = small_engine
    B = 3
    ids, qf = _prompt(eng.cfg, B)
    g = torch.Generator().manual_seed(4)
    forced = torch.randint(3, 31999, (N_NEW, B), generator=g)
    toks, lg = eng.prefill(ids, qf, max_new=N_NEW, eos_id=-1, logprobs=2)
    rows = [lg.cpu()]
    c, i, l = eng.get_logprobs(B, N_NEW)                                               # token 0 only: the other steps read (0.0, -1, 0.0)
    assert bool((c[:, 1:] == 0).all()) and bool((i[:, 1:] == -1).all()) and bool((l[:, 1:] == 0).all()) and bool((c[:, 0] < 0).all()) and bool((i[:, 0] >= 0).all())
    for s in range(1, N_NEW):
        toks, lg = eng.decode_step(input_ids=forced[s] if s >= 3 else None)             # rdx_decode_step, then rdx_decode_step_ids
        rows.append(lg.cpu())
    scores = torch.stack(rows)
    single = eng.get_logprobs(B, N_NEW)
    _check_entries(single, scores, toks.cpu(), N_NEW, 2, f"small {eng.dtype} single steps")
    # the same conversation through rdx_generate: the entries of the free-running steps 0 .. 2 are the same bits
    _, _, _, lp = eng.generate(ids, qf, max_new=N_NEW, eos_id=-1, logprobs=2)
    assert _bits_equal([t[:, :3] for t in single], [t[:, :3] for t in lp])
    # switched on by a decode step: the entries before it keep what the reset left
    eng.prefill(ids, qf, max_new=N_NEW, eos_id=-1, logprobs=0)
    eng.set_logprobs(None)
    eng.decode_step()
    toks, _ = eng.decode_step(logprobs=1)
    c2, i2, _ = eng.get_logprobs(B, N_NEW)
    assert torch.equal(c2[:, 0].view(torch.int32), lp[0][:, 0].view(torch.int32)) and bool((c2[:, 1] == 0).all()) and bool((c2[:, 2] < 0).all())
    assert bool((i2[:, 0] == -1).all()) and torch.equal(i2[:, 2, 0].long(), lp[1][:, 2, 0].long())
    eng.set_logprobs(None)


def test_logprobs_behind_a_kept_prefix(small_engine):
    """rdx_generate_append: the second turn extends the first prompt and its answer, whose KV rows are kept; the entries are those of the full prompt's scores."""
    eng = small_engine
    ids, qf = _prompt(eng.cfg, 1, T=40)
    more = synth.synth_prompt_ids(1, 40, vocab=eng.cfg.llama.vocab, img_offset=50, seed=34)[:, 2:]       # 38 plain tokens: neither BOS, pad nor <IMG>
    answer, _, n, _ = eng.generate(ids, qf, max_new=N_NEW, eos_id=-1, reuse_prefix=True, logprobs=4)
    ids2 = torch.cat([ids, answer[:, :n].cpu().long(), more], dim=1)
    toks, sc, n, lp = eng.generate(ids2, qf, max_new=N_NEW, eos_id=-1, reuse_prefix=True, output_scores=True, logprobs=4)
    assert eng.last_kept_prefix == 40 + N_NEW - 1 and n == N_NEW
    _check_entries(lp, sc.cpu(), toks.cpu(), n, 4, f"small {eng.dtype} append")
    toks_b, _, _, lp_b = eng.generate(ids2, qf, max_new=N_NEW, eos_id=-1, logprobs=4)                      # the whole prompt prefilled
    assert eng.last_kept_prefix == 0 and torch.equal(toks_b, toks)
    tol = 0.05                                                                          # another prompt kernel behind the kept rows: close, not bit-equal
    assert float((lp_b[0] - lp[0]).abs().max()) < tol
    eng.set_logprobs(None)


def test_model_generate_returns_token_and_top_logprobs():
    """LlamaForCausalLM.generate(output_logprobs=True, top_logprobs=3): `.token_logprobs` is compute_transition_scores(normalize_logits=True) of the `.scores`
    the same call returns, `.top_logprobs` the three largest columns of each; sequences and scores are those of a call without the option."""
    from radialog_amd.modeling_llama_imgemb import LlamaForCausalLM
    cfg = small_cfg()
    B = 2
    ids, qf = _prompt(cfg, B, T=56)
    lm = LlamaForCausalLM.from_pretrained(None, torch_dtype=torch.float16, synthetic=True, cfg=cfg.llama, max_batch=2 * B, max_len=128)
    try:
        kw = dict(input_ids=ids, attention_mask=ids.ne(0).long(), qformer_embs=qf, max_new_tokens=N_NEW, return_dict_in_generate=True, output_scores=True, eos_token_id=-1)
        plain = lm.generate(**kw)
        out = lm.generate(output_logprobs=True, top_logprobs=3, **kw)
        assert not hasattr(plain, "token_logprobs") and torch.equal(out.sequences, plain.sequences)
        assert all(torch.equal(a.view(torch.int16), b.view(torch.int16)) for a, b in zip(out.scores, plain.scores))
        n = len(out.scores)
        toks = out.sequences[:, -n:].cpu()
        _check_entries((out.token_logprobs, out.top_logprobs[0], out.top_logprobs[1]), torch.stack(out.scores).cpu(), toks, n, 3, "model f16 B=2")
        only = lm.generate(output_logprobs=True, **{**kw, "output_scores": False})
        assert only.scores is None and torch.equal(only.token_logprobs.view(torch.int32), out.token_logprobs.view(torch.int32)) and only.top_logprobs[0].shape[-1] == 0
        with pytest.raises(ValueError, match="logprobs"):
            lm.generate(output_logprobs=True, num_beams=2, **kw)
        beams = lm.generate(num_beams=2, **kw)                                         # and beam search behind a call that had the option on
        assert beams.sequences.shape[0] == B
    finally:
        lm.close()


# ---- 3. EOS -----------------------------------------------------------------------------------------------------------------------------------------------
def test_entries_behind_eos_are_the_pad_tokens_and_python_masks_them(small_engine):
    eng = small_engine
    B, PAD = 3, 0
    ids, qf = _prompt(eng.cfg, B)
    free, _, _ = eng.generate(ids, qf, max_new=N_NEW, eos_id=-1)
    eos = int(free[0, 3])
    toks, sc, n, lp = eng.generate(ids, qf, max_new=N_NEW, eos_id=eos, pad_id=PAD, output_scores=True, logprobs=8)
    toks, sc = toks.cpu()[:, :n], sc.cpu()[:n]
    first = [(toks[b] == eos).nonzero() for b in range(B)]
    assert len(first[0]) and int(first[0][0]) <= 3 and n > int(first[0][0]) + 1        # row 0 ends, and steps run behind its end
    behind = torch.zeros(B, n, dtype=torch.bool)
    for b in range(B):
        if len(first[b]):
            behind[b, int(first[b][0]) + 1:] = True
    assert bool((toks[behind] == PAD).all())
    raw = eng.get_logprobs(B, n)                                                        # the C level: the pad token's entries, from the scores of those steps
    _check_entries(raw, sc, toks, n, 8, f"small {eng.dtype} EOS (device entries)")
    assert bool((raw[1][behind][:, 0] >= 0).all())
    c, i, l = lp                                                                        # the Python level: masked behind the EOS, untouched up to and including it
    assert bool((c[behind] == 0).all()) and bool((i[behind] == -1).all()) and bool((l[behind] == 0).all())
    assert _bits_equal([t[~behind] for t in lp], [t[~behind] for t in raw])
    eng.set_logprobs(None)


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_logprobs(small_engine):
    eng = small_engine
    lib, ctx = eng.lib, eng.ctx
    ids, qf = _prompt(eng.cfg, 2)
    eng.set_logprobs(None)
    host = torch.zeros(64)
    assert lib.rdx_get_logprobs(ctx, 1, 1, C.c_void_p(host.data_ptr()), None, None) == -1 and "logprobs" in _last_error(eng)      # the option is off
    for bad in (9, -2):
        assert lib.rdx_set_logprobs(ctx, bad) == -1 and "logprobs" in _last_error(eng)
    assert eng._logprobs is None and lib.rdx_get_logprobs(ctx, 1, 1, C.c_void_p(host.data_ptr()), None, None) == -1                # ... and stays off
    with pytest.raises(ValueError, match="logprobs"):
        eng.generate(ids, qf, max_new=4, logprobs=9)
    eng.generate(ids, qf, max_new=4, eos_id=-1, logprobs=2)
    assert lib.rdx_get_logprobs(ctx, 3, 4, C.c_void_p(host.data_ptr()), None, None) == -1 and "logprobs" in _last_error(eng)      # 3 rows of a 2-row conversation
    assert lib.rdx_get_logprobs(ctx, 2, 5, C.c_void_p(host.data_ptr()), None, None) == -1
    assert lib.rdx_get_logprobs(ctx, 2, 4, C.c_void_p(host.data_ptr()), None, None) == 0                                            # the top pointers are nullable
    # beam search and a row session under the option
    assert lib.rdx_beam_search(ctx, None, None, 1, 2, 8, None, 4, -1, 0, 1.0, 0, None, None, None, None, None) == -1
    assert "logprobs" in _last_error(eng) and "rdx_beam_search" in _last_error(eng)
    out = torch.zeros(1, 8, dtype=torch.int32, device=eng.device)
    assert lib.rdx_rows_begin(ctx, 1, 1, 8, -1, 0, C.c_void_p(out.data_ptr())) == -1
    assert "logprobs" in _last_error(eng) and "rdx_rows_begin" in _last_error(eng)
    # setting the option inside a session
    eng.set_logprobs(None)
    assert lib.rdx_rows_begin(ctx, 1, 1, 8, -1, 0, C.c_void_p(out.data_ptr())) == 0
    try:
        assert lib.rdx_set_logprobs(ctx, 2) == -1
        assert "logprobs" in _last_error(eng) and "rdx_rows_end first" in _last_error(eng)
        assert lib.rdx_set_logprobs(ctx, -1) == 0
    finally:
        assert lib.rdx_rows_end(ctx) == 0
    # the Python layer switches the option off where the library would refuse
    eng.set_logprobs(3)
    toks, lens, _, _, _ = eng.beam_search(ids[:1], qf[:1], num_beams=2, max_new=4, eos_id=-1)
    assert eng._logprobs is None and 1 <= int(lens[0]) <= 4
