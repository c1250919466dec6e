"""Row sessions (include/rdx.h rdx_rows_*: continuous batching) on the GPU. A refill is the prompt path into staging rows plus two copy kernels
(csrc/rows.hip), a step is the unchanged decode step: everything here but the oracle legs is an equality of bits (logits compared as int16).

Engines: small_cfg() in f16 and bf16 (rows = 2: the chained / fused launches; rows = 4: the generic family), the 2-layer Vicuna-width config of
tests/test_gpu_w4_step.py in bf16 (rows = 4: the xs16 family) and the same with fp8 weights (small_cfg has no fp8 kernel from 3 rows). max_len 128.
Prompts: T = 40 with the image splice (a refill group of two or more has one row left-padded by 3) and T = 24 without an image -- the splice needs
T >= 32, so the short prompt cannot carry one. A row refilled with T = 40 at step 0 crosses a 16-position boundary at step 8, one refilled with
T = 24 at step 5 at step 13."""
import ctypes as C

import pytest
import torch

from radialog_amd import _lib, synth
from radialog_amd.config import LlamaCfg, RaDialogCfg, small_cfg
from radialog_amd.engine import RowSession
from radialog_amd.rowqueue import chunked_steps
from _parity import Cover, check_greedy
from test_rowqueue_host import QUEUE_LIST

pytestmark = pytest.mark.gpu

DT = {"f16": torch.float16, "bf16": torch.bfloat16}
# the bars of the small-config greedy legs of tests/test_gpu_parity.py (LOGIT_TOL, MIN_COVER on the sum of the legs), not new ones
LOGIT_TOL = {"f16": 1e-2, "bf16": 6e-2}
MIN_COVER = {"f16": 0.9, "bf16": 0.75}
MAX_LEN, MAX_B, CAP, N = 128, 8, 16, 16
T_IMG, T_TXT = 40, 24
ENGINES = [("small", "f16", False), ("small", "bf16", False), ("prod2", "bf16", False), ("prod2", "bf16", True)]


def _cfg(which):
    return small_cfg() if which == "small" else RaDialogCfg(llama=LlamaCfg(layers=2, qformer_dim=192))


def _make(which, dtype, fp8):
    from radialog_amd.engine import RdxEngine, synth_getter
    cfg = _cfg(which)
    eng = RdxEngine(cfg, dtype=dtype, device=0, max_batch=MAX_B, max_len=MAX_LEN, lora=True, vision=False, weights_fp8=fp8)
    eng.load_weights(synth_getter(cfg, eng.device, lora=True), vision=False)
    return cfg, eng


@pytest.fixture(scope="module", params=ENGINES, ids=lambda p: f"{p[0]}-{p[1]}{'-fp8' if p[2] else ''}")
def any_engine(request):
    cfg, eng = _make(*request.param)
    yield cfg, eng
    eng.close()


@pytest.fixture(scope="module", params=["f16", "bf16"])
def small(request):
    cfg, eng = _make("small", request.param, False)
    yield cfg, eng
    eng.close()


def _img_prompts(cfg, n, seed):
    """n prompts of T_IMG tokens with the <IMG> block, every odd row left-padded by 3 (one in each refill pair), and their image embeddings."""
    ids = synth.synth_prompt_ids(n, T_IMG, vocab=cfg.llama.vocab, img_offset=6, pad_rows=False, seed=seed)
    for b in range(1, n, 2):
        ids[b] = torch.cat([torch.zeros(3, dtype=torch.long), ids[b, : T_IMG - 3]])
    return ids, synth.synth(f"t.rows.qf{seed}", (n, 32, cfg.llama.qformer_dim), -1.0, 1.0)


def _txt_prompt(cfg, seed):
    ids = synth.synth_prompt_ids(1, T_TXT, vocab=cfg.llama.vocab, img_offset=6, pad_rows=False, seed=seed)
    ids[ids == 32000] = 99
    return ids


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16).clone()


def _drive(eng, rows, stage, plan, n_steps, use_graph=True, eos_id=-1, hook=None):
    """One session: plan = {step index: [(ids, qf, target rows), ...]} refills enqueued in front of that step, then n_steps single steps with logits.
    Returns (tokens [rows][CAP], rec) with rec[r] = the logits bits row r produced since its last refill (the refill's own first), and the KV of every layer."""
    rec = {r: [] for r in range(rows)}
    with eng.row_session(rows, stage, CAP, eos_id=eos_id, use_graph=use_graph) as ses:
        for s in range(n_steps):
            for ids, qf, tgt in plan.get(s, []):
                lg = _bits(ses.refill(ids, None, qf, tgt, want_logits=True))
                for k, r in enumerate(tgt):
                    rec[r] = [lg[k]]
            if hook is not None:
                hook(ses, s)
            lg = _bits(ses.step(1, want_logits=True))
            for r in range(rows):
                rec[r].append(lg[r])
        eng.sync()
        toks = ses.tokens.cpu().clone()
        L = eng.cfg.llama.layers
        kv = [(_bits(eng.kv_read(l, 0, rows)), _bits(eng.kv_read(l, 1, rows))) for l in range(L)]
    return toks, rec, kv


@pytest.mark.parametrize("rows", [2, 4])
def test_refilling_all_rows_at_once_is_a_fresh_generate(any_engine, rows):
    cfg, eng = any_engine
    ids, qf = _img_prompts(cfg, rows, seed=51)
    for use_graph in (False, True):
        toks, scores, n = eng.generate(ids, qf, max_new=N, eos_id=-1, output_scores=True, use_graph=use_graph)
        assert n == N
        t_ref, s_ref = toks.cpu().clone(), _bits(scores)
        t, rec, _ = _drive(eng, rows, rows, {0: [(ids, qf, list(range(rows)))]}, N - 1, use_graph=use_graph)
        assert torch.equal(t[:, :N], t_ref), f"tokens (graph={use_graph})"
        for r in range(rows):
            assert len(rec[r]) == N
            for s in range(N):
                assert torch.equal(rec[r][s], s_ref[s, r]), f"row {r} step {s} logits (graph={use_graph})"


def test_refill_is_the_prefill(small):
    cfg, eng = small
    _, other = _make("small", eng.dtype, False)
    try:
        ids, qf = _img_prompts(cfg, 2, seed=52)
        with eng.row_session(4, 2, CAP, eos_id=-1) as ses:
            lg = _bits(ses.refill(ids, None, qf, [3, 1], want_logits=True))
            eng.sync()
            t0 = ses.tokens.cpu()[[3, 1], 0]
            assert bool((ses.tokens.cpu()[[3, 1], 1:] == 0).all())
            kv = [[_bits(eng.kv_read(l, w, 4))[[3, 1], :, :T_IMG] for w in (0, 1)] for l in range(cfg.llama.layers)]
        toks, lg2 = other.prefill(ids, qf, max_new=CAP, eos_id=-1)
        assert torch.equal(t0, toks.cpu()[:, 0]) and torch.equal(lg, _bits(lg2))
        for l in range(cfg.llama.layers):
            for w in (0, 1):
                assert torch.equal(kv[l][w], _bits(other.kv_read(l, w, 2))[:, :, :T_IMG]), f"layer {l} {'KV'[w]}"
    finally:
        other.close()


# ---- legs 3, 4, 6: one set of sessions per engine, shared ------------------------------------------------------------
R_ROW, S_A, S_B = 2, 5, 9        # the refilled row, and the step in front of which it is refilled in sessions B and C


def _first(pr, rows):
    """the refills that fill every row at step 0, two prompts (one staging pair) at a time"""
    return [(pr[0][i:i + 2], pr[1][i:i + 2], list(range(i, min(i + 2, rows)))) for i in range(0, rows, 2)]


def _session_c(cfg, eng, rows):
    """leg 4's second session: the text prompt P into row r in front of step S_B, next to the neighbours of seed 54"""
    r = min(R_ROW, rows - 1)
    return _drive(eng, rows, 2, {0: _first(_img_prompts(cfg, rows, seed=54), rows), S_B: [(_txt_prompt(cfg, seed=55), None, [r])]}, N)


def _sessions(cfg, eng, rows):
    r = min(R_ROW, rows - 1)
    base = _img_prompts(cfg, rows, seed=53)
    A = _drive(eng, rows, 2, {0: _first(base, rows)}, N)
    B = _drive(eng, rows, 2, {0: _first(base, rows), S_A: [(_txt_prompt(cfg, seed=55), None, [r])]}, N)
    return r, A, B, _session_c(cfg, eng, rows)


@pytest.fixture(scope="module")
def runs(any_engine):
    cfg, eng = any_engine
    return {rows: _sessions(cfg, eng, rows) for rows in (2, 4)}


def test_live_rows_are_undisturbed_by_a_refill(runs):
    for rows, (r, A, B, _) in runs.items():
        for q in range(rows):
            if q == r:
                continue
            assert torch.equal(A[0][q], B[0][q]), f"rows={rows}: tokens of row {q}"
            assert len(A[1][q]) == len(B[1][q]) == N + 1
            for s in range(N + 1):
                assert torch.equal(A[1][q][s], B[1][q][s]), f"rows={rows}: logits of row {q} at step {s}"
            for l, ((ka, va), (kb, vb)) in enumerate(zip(A[2], B[2])):
                assert torch.equal(ka[q, :, :T_IMG + N], kb[q, :, :T_IMG + N]) and torch.equal(va[q, :, :T_IMG + N], vb[q, :, :T_IMG + N]), f"rows={rows}: KV of row {q}, layer {l}"
        assert not torch.equal(A[0][r], B[0][r])        # and the refill did happen


def test_a_refilled_row_depends_neither_on_its_neighbours_nor_on_when_it_arrived(runs):
    for rows, (r, _, B, Cc) in runs.items():
        n = N - S_B + 1                               # what session C saw of the request: the refill and N - S_B steps
        assert len(B[1][r]) == N - S_A + 1 and len(Cc[1][r]) == n
        for s in range(n):
            assert torch.equal(B[1][r][s], Cc[1][r][s]), f"rows={rows}: logits {s} steps behind the refill"
        assert torch.equal(B[0][r][:n], Cc[0][r][:n])
        assert not torch.equal(B[0][0], Cc[0][0])       # next to different neighbours


def test_one_refilled_row_matches_the_oracle(small):
    from oracle import ref_cpu
    cfg, eng = small
    W = synth.make_weights(synth.llama_specs(cfg.llama, lora=True))
    orc = ref_cpu.LlamaOracle(W, cfg.llama, DT[eng.dtype], lora=True)
    cover = Cover()
    for seed, row in ((56, 2), (57, 0)):
        ids, qf = _img_prompts(cfg, 1, seed=seed)
        with torch.no_grad():
            ref = orc.generate_greedy(ids, qf, max_new=N, eos_id=-1, pad_id=0)
        toks, rec, _ = _drive(eng, 4, 2, {0: [(ids, qf, [row])]}, N - 1)
        scores = torch.stack([x.view(DT[eng.dtype]) for x in rec[row]])[:, None, :]
        cover.add(check_greedy(toks[row:row + 1, :N], scores, ref, LOGIT_TOL[eng.dtype], 0.0, f"{eng.dtype} row {row}"))
    cover.check(MIN_COVER[eng.dtype], f"{eng.dtype}: a refilled row against the oracle")


@pytest.mark.parametrize("rows", [2, 4])
def test_eos_and_parking(small, rows):
    cfg, eng = small
    r = min(R_ROW, rows - 1)
    ids, qf = _img_prompts(cfg, 1, seed=58)
    P = _txt_prompt(cfg, seed=55)
    free, _, _ = _drive(eng, rows, 2, {0: [(ids, qf, [0])]}, N - 1)
    want = _session_c(cfg, eng, rows)      # leg 4's session: the bits row r must keep producing for P
    p_toks = want[0][r][: N - S_B + 1].tolist()
    k = next(i for i in range(2, N) if int(free[0][i]) not in p_toks)
    eos = int(free[0][k])
    k = free[0].tolist().index(eos)                    # the first time row 0 emits it
    with eng.row_session(rows, 2, CAP, eos_id=eos) as ses:
        ses.refill(ids, None, qf, [0])
        for j in range(1, N):
            unf, steps = ses.poll()
            # (a row the poll has seen finished is parked from then on: its count stays at the k + 1 tokens it had selected)
            assert steps[0] == min(j, k + 1) and unf[0] == (1 if j <= k else 0), f"{j} tokens generated, EOS is token {k}"
            assert all(u == 0 for u in unf[1:])        # parked rows
            ses.step(1)
        eng.sync()
        got = ses.tokens.cpu()[0].tolist()
        assert got[: k + 1] == free[0][: k + 1].tolist() and got[k + 1:] == [0] * (CAP - k - 1)
        # row 0 has finished, the others are parked: 3 x max_len steps while row r is refilled with P again and again
        total, it = 0, 0
        while total < 3 * MAX_LEN:
            lg = [_bits(ses.refill(P, None, None, [r], want_logits=True))[0]]
            check_bits = it in (0, 1, 5)
            n_lg = N - S_B if check_bits else 0
            for _ in range(n_lg):
                lg.append(_bits(ses.step(1, want_logits=True))[r])
            ses.step(64 - n_lg)                        # T_TXT + 64 < max_len; tokens behind the cap are not written
            total += 64
            unf, steps = ses.poll()                    # raises when the sticky hand-off error flag is set
            assert steps[r] == 65 and unf[0] == 0
            if check_bits:
                for s, x in enumerate(lg):
                    assert torch.equal(x, want[1][r][s]), f"iteration {it}: logits {s} steps behind the refill"
                assert ses.tokens.cpu()[r][: n_lg + 1].tolist() == want[0][r][: n_lg + 1].tolist()
            it += 1
        assert ses.tokens.cpu()[0].tolist() == got     # the finished row's tokens stayed


def _refused(eng, match, fn):
    with pytest.raises(_lib.RdxError, match=match) as e:
        fn()
    assert "(-1)" in str(e.value), str(e.value)


def test_refusals_leave_the_state_unchanged(small):
    cfg, eng = small
    lib, ctx = eng.lib, eng.ctx
    ids, qf = _img_prompts(cfg, 2, seed=59)
    host = torch.zeros(8, dtype=torch.int32)
    hp = C.c_void_p(host.data_ptr())
    raw = lambda name, rc: _lib.check(ctx, rc, name)        # noqa: E731
    # outside a session
    for name, call in (("rdx_rows_refill", lambda: lib.rdx_rows_refill(ctx, hp, None, 1, 8, None, hp, None)), ("rdx_rows_step", lambda: lib.rdx_rows_step(ctx, 1, 0, None)),
                       ("rdx_rows_poll", lambda: lib.rdx_rows_poll(ctx, hp, hp)), ("rdx_rows_park", lambda: lib.rdx_rows_park(ctx, hp, 1)),
                       ("rdx_rows_end", lambda: lib.rdx_rows_end(ctx))):
        _refused(eng, "no row session", lambda: raw(name, call()))
    eng.set_logits_rules((1.2, 0, 0))
    _refused(eng, "logits rules", lambda: RowSession(eng, 4, 2, CAP, -1, 0))
    eng.set_logits_rules(None)
    eng.set_sampling((0.8, 50, 0.9, 1))
    _refused(eng, "sampling", lambda: RowSession(eng, 4, 2, CAP, -1, 0))
    eng.set_sampling(None)
    _refused(eng, "max_batch", lambda: RowSession(eng, 6, 3, CAP, -1, 0))
    _refused(eng, "cap", lambda: RowSession(eng, 4, 2, MAX_LEN, -1, 0))
    plan = {0: [(ids, qf, [0, 1]), (ids.flip(0), qf.flip(0), [2, 3])]}
    clean = _drive(eng, 4, 2, plan, N)

    def misuse(ses, s):
        if s != 5:
            return
        _refused(eng, "already open", lambda: RowSession(eng, 4, 2, CAP, -1, 0))
        for fn in (lambda: eng.prefill(ids, qf, 4), lambda: eng.generate(ids, qf, 4), lambda: eng.score(ids, qf, ids.to(torch.int32)),
                   lambda: eng.beam_search(ids, qf, 2, 4), lambda: raw("rdx_decode_step", lib.rdx_decode_step(ctx, None)),
                   lambda: raw("rdx_decode_step_ids", lib.rdx_decode_step_ids(ctx, hp, None)),
                   lambda: raw("rdx_prefill_append", lib.rdx_prefill_append(ctx, hp, 4, 2, 8, 4, -1, 0, hp, None)),
                   lambda: raw("rdx_generate_append", lib.rdx_generate_append(ctx, hp, 4, 2, 8, 4, -1, 0, hp, None, None, 0)),
                   lambda: eng.set_logits_rules((1.2, 0, 0)), lambda: eng.set_sampling((0.8, 50, 0.9, 1))):
            _refused(eng, "rdx_rows_end first", fn)
        eng._rules, eng._sampling = type(eng._rules)(), None
        one = ids[:1]
        _refused(eng, r"outside \[1, stage", lambda: ses.refill(torch.cat([ids, one]), None, None, [0, 1, 2]))
        _refused(eng, "listed twice", lambda: ses.refill(ids, None, qf, [1, 1]))
        _refused(eng, "target row 4 outside", lambda: ses.refill(one, None, qf[:1], [4]))
        _refused(eng, "exceeds max_len", lambda: ses.refill(torch.ones(1, MAX_LEN - CAP + 1, dtype=torch.int32), None, None, [0]))
        _refused(eng, "T >= 32", lambda: ses.refill(torch.ones(1, 8, dtype=torch.int32), None, qf[:1], [0]))
        _refused(eng, "steps outside", lambda: ses.step(0))
        _refused(eng, "steps outside", lambda: ses.step(MAX_LEN))
        _refused(eng, "single step only", lambda: raw("rdx_rows_step", lib.rdx_rows_step(ctx, 2, 0, hp)))
        _refused(eng, "full", lambda: ses.step(MAX_LEN - T_IMG - 5 + 1))
        _refused(eng, "outside", lambda: ses.park([7]))
    dirty = _drive(eng, 4, 2, plan, N, hook=misuse)
    assert torch.equal(clean[0], dirty[0])
    for r in range(4):
        assert len(clean[1][r]) == len(dirty[1][r]) and all(torch.equal(a, b) for a, b in zip(clean[1][r], dirty[1][r])), f"row {r}"
    # and the session left no conversation behind
    _refused(eng, "no prefill has run", lambda: raw("rdx_decode_step", lib.rdx_decode_step(ctx, None)))
    toks, _, n = eng.generate(ids, qf, max_new=4, eos_id=-1)
    assert n == 4


def test_generate_queue_end_to_end(small):
    from oracle import ref_cpu
    cfg, eng = small
    reqs = []
    for i, (T, cap) in enumerate(QUEUE_LIST):
        ids = synth.synth_prompt_ids(1, T, vocab=cfg.llama.vocab, img_offset=1, pad_rows=False, seed=70 + i)[0]
        if T < 33:
            ids[ids == 32000] = 99
            reqs.append((ids, None, cap))
        else:
            reqs.append((ids, synth.synth(f"t.rows.q{i}", (32, cfg.llama.qformer_dim), -1.0, 1.0), cap))
    caps = [c for _, c in QUEUE_LIST]
    out1, sch1 = eng.generate_queue(reqs, rows=4, stage=2, eos_id=-1, return_scheduler=True)
    out2, sch2 = eng.generate_queue(reqs, rows=4, stage=2, eos_id=-1, return_scheduler=True)
    assert [len(o) for o in out1] == caps                                    # request order, cut at each request's own cap
    assert all(torch.equal(a, b) for a, b in zip(out1, out2)) and sch1.groups == sch2.groups
    assert sch1.n_steps < chunked_steps(caps, 4)
    W = synth.make_weights(synth.llama_specs(cfg.llama, lora=True))
    orc = ref_cpu.LlamaOracle(W, cfg.llama, DT[eng.dtype], lora=True)
    cover = Cover()
    for i, (ids, qf, cap) in enumerate(reqs):
        with torch.no_grad():
            ref = orc.generate_greedy(ids[None], None if qf is None else qf[None], max_new=cap, eos_id=-1, pad_id=0)
        cover.add(check_greedy(out1[i][None], None, ref, LOGIT_TOL[eng.dtype], 0.0, f"{eng.dtype} request {i}"))
    cover.check(MIN_COVER[eng.dtype], f"{eng.dtype}: generate_queue against the oracle")
