"""Generation log-probs without a GPU: the float64 restatement of tests/_logprobs.py against torch's log_softmax / topk on hand cases and against
transformers' compute_transition_scores, the fp32 emulation of logprob_step_k's reduction order inside the derived bar and four planted faults outside it (on
the very inputs tests/test_gpu_logprobs.py gives the kernel), LlamaForCausalLM's refusals before any engine exists, the Python layer's EOS masking, and the C ABI."""
import ctypes as C
import inspect
import os
import re
from types import SimpleNamespace

import pytest
import torch

import _logprobs as L

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = {"f16": torch.float16, "bf16": torch.bfloat16}
INF = float("inf")


# ---- the restatement -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_hand_cases(dtype):
    dt = DT[dtype]
    # ties: by value, then the lowest index
    x = torch.tensor([[1.0, 3.0, 3.0, -2.0, 3.0, 0.5]]).to(dt)
    assert L.top_ids(x, 4).tolist() == [[1, 2, 4, 0]]
    lsm = torch.log_softmax(x.double(), -1)
    assert torch.equal(L.top_lp(x, L.top_ids(x, 4)), lsm[:, [1, 2, 4, 0]]) and torch.equal(L.chosen(x, torch.tensor([3])), lsm[:, 3])
    # all equal: the first n columns, each log(1 / V)
    x = torch.full((1, 5), 1.25).to(dt)
    assert L.top_ids(x, 5).tolist() == [[0, 1, 2, 3, 4]]
    assert float((L.top_lp(x, L.top_ids(x, 5)) + torch.log(torch.tensor(5.0, dtype=torch.float64))).abs().max()) < 1e-15
    # -inf columns follow the finite ones, lowest index first, with log-prob -inf; a chosen -inf token has log-prob -inf
    x = torch.tensor([[-INF, 2.0, -INF, 1.0]]).to(dt)
    assert L.top_ids(x, 4).tolist() == [[1, 3, 0, 2]]
    lp = L.top_lp(x, L.top_ids(x, 4))
    assert torch.isfinite(lp[0, :2]).all() and bool((lp[0, 2:] == -INF).all()) and float(L.chosen(x, torch.tensor([2]))) == -INF
    assert bool((L.logprob_bar(x, L.top_ids(x, 4))[0, 2:] == 0).all())
    # +-60000 in f16 (bf16: the nearest values): the low columns underflow to probability 0, log-prob = -(the gap) exactly
    x = torch.tensor([[60000.0, -60000.0, 60000.0, -60000.0]]).to(dt)
    assert L.top_ids(x, 3).tolist() == [[0, 2, 1]]
    lp = L.top_lp(x, L.top_ids(x, 3))
    gap = float(x[0, 0].double() - x[0, 1].double())
    assert abs(float(lp[0, 0]) + 0.6931471805599453) < 1e-12 and abs(float(lp[0, 2]) + gap + 0.6931471805599453) < 1e-9
    # NaN never enters the top-n; slots without a candidate hold (-1, 0.0)
    x = torch.tensor([[float("nan"), 1.0, float("nan")]]).to(dt)
    assert L.top_ids(x, 3).tolist() == [[1, -1, -1]] and L.top_lp(x, L.top_ids(x, 3))[0, 1:].tolist() == [0.0, 0.0]
    assert L.top_ids(x, 0).shape == (1, 0)


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_restatement_equals_torch_log_softmax_and_topk(dtype):
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(6, 4099, generator=g) * 3).to(DT[dtype])
    tok = torch.randint(0, 4099, (6,), generator=g)
    lsm = torch.log_softmax(x.double(), -1)
    assert torch.equal(L.chosen(x, tok), lsm[torch.arange(6), tok])
    ids = L.top_ids(x, 8)
    tk = torch.topk(x.double(), 8, dim=-1)
    assert torch.equal(x.double().gather(-1, ids), tk.values)                      # the same values; among equal ones the restatement fixes the order
    for r in range(6):
        for k in range(7):
            a, b = x[r, ids[r, k]], x[r, ids[r, k + 1]]
            assert a > b or (a == b and ids[r, k] < ids[r, k + 1])
    assert torch.equal(L.top_lp(x, ids), lsm.gather(-1, ids))


def test_chosen_equals_transformers_compute_transition_scores():
    transformers = pytest.importorskip("transformers")
    fn = getattr(transformers.GenerationMixin, "compute_transition_scores", None)
    if fn is None:
        pytest.skip("this transformers has no compute_transition_scores")
    g = torch.Generator().manual_seed(11)
    n, B, V, T = 5, 3, 101, 4
    scores = (torch.randn(n, B, V, generator=g) * 2).to(torch.float16)
    scores[2, 1, ::3] = -INF                                                       # a processed row: banned columns
    toks = torch.randint(0, V, (B, n), generator=g)
    toks[1, 2] = 1                                                                 # not a banned column
    cfg = SimpleNamespace(vocab_size=V)
    cfg.get_text_config = lambda: cfg
    seq = torch.cat([torch.zeros(B, T, dtype=torch.long), toks], dim=1)
    want = fn(SimpleNamespace(config=cfg), seq, tuple(scores[i].double() for i in range(n)), normalize_logits=True)
    got = L.entries(scores, toks, 0)[0]
    assert float((got - want.double()).abs().max()) < 1e-12


# ---- the emulation of the kernel's order, on the GPU test's inputs --------------------------------------------------------------------------------------
def _check(em, want, bars):
    (c, i, l), (wc, wi, wl), (bc, bl) = em, want, bars
    return bool(L.within(c, wc, bc).all()) and torch.equal(i, wi) and bool(L.within(l, wl, bl).all())


def _want(x, tok, n):
    ids = L.top_ids(x, n)
    return (L.chosen(x, tok), ids, L.top_lp(x, ids)), (L.logprob_bar(x, tok), L.logprob_bar(x, ids))


@pytest.mark.parametrize("B,V", [(B, V) for B in (1, 9) for V in (32001, 32000, 4099, 8)])
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_emulated_kernel_order_stays_inside_the_derived_bar(B, V, dtype):
    xp, tok = L.kernel_case(B, V, DT[dtype])
    want, bars = _want(xp[:, :V], tok, 8)
    em = L.emulate_kernel(xp, tok, V, 8)
    (c, i, l), (wc, wi, wl), (bc, bl) = em, want, bars
    over = max(float(((c.double() - wc).abs() - bc).nan_to_num(nan=0.0, posinf=0.0, neginf=0.0).max()), float(((l.double() - wl).abs() - bl).nan_to_num(nan=0.0, posinf=0.0, neginf=0.0).max()))
    print(f"emulated logprob_step_k B={B} V={V} {dtype}: worst |error| - bar = {over:.3g}, largest bar {float(bc.max()):.3g}, n_ser {L.n_ser(V)}")
    assert _check(em, want, bars)
    assert L.n_ser(32001) == 128 and L.n_ser(8) == 8 and L.n_ser(4099) == 24


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_planted_faults_leave_the_bar_or_change_an_id(dtype):
    V = 4099
    xp, tok = L.kernel_case(9, V, DT[dtype])
    want, bars = _want(xp[:, :V], tok, 8)
    assert _check(L.emulate_kernel(xp, tok, V, 8, elem0=3), want, bars)            # the alignment alone changes nothing
    for fault, rows in (("drop", range(9)), ("label", (0, 1, 6)), ("pads", range(9))):
        c, i, l = L.emulate_kernel(xp, tok, V, 8, elem0=3, fault=fault)
        for r in rows:
            if r == 5:
                continue                                                             # the NaN row: NaN / -1 whatever happens
            one = lambda t: t[r: r + 1]                                              # noqa: E731
            ok = _check((one(c), one(i), one(l)), tuple(one(t) for t in want), tuple(one(t) for t in bars))
            assert not ok, f"fault {fault!r} goes unnoticed in row {r}"
    # the scalar head of an odd-start row skipped: row 1's token is column 0 (inside the head), row 6's top ties include columns 0 and 1
    c, i, l = L.emulate_kernel(xp, tok, V, 8, elem0=3, fault="head")
    assert int(tok[1]) == 0 and not bool(L.within(c[1:2], want[0][1:2], bars[0][1:2]).all())
    assert not torch.equal(i[6], want[1][6])
    # equal logits: a dropped piece moves S by 8 / V, far outside the bar
    flat = torch.full((1, L.S.pad_ld(V)), 1.25).to(DT[dtype])
    w, b = _want(flat[:, :V], torch.tensor([V - 1]), 0)
    c, _, _ = L.emulate_kernel(flat, torch.tensor([V - 1]), V, 0, fault="drop")
    assert abs(float(c[0]) - float(w[0][0])) > 100 * float(b[0][0])


# ---- LlamaForCausalLM: the checks run before any engine exists ---------------------------------------------------------------------------------------------
class _Reached(Exception):
    pass


def _model():
    from radialog_amd.modeling_llama_imgemb import LlamaForCausalLM
    return LlamaForCausalLM.from_pretrained(None, torch_dtype=torch.float16, synthetic=True)


def test_generate_refuses_logprobs_with_beams_and_in_generate_many(monkeypatch):
    lm = _model()
    monkeypatch.setattr(lm, "_ensure_engine", lambda: (_ for _ in ()).throw(_Reached()))
    ids = torch.ones(1, 40, dtype=torch.long)
    with pytest.raises(ValueError, match="logprobs"):
        lm.generate(input_ids=ids, max_new_tokens=4, num_beams=2, output_logprobs=True)
    with pytest.raises(ValueError, match="logprobs"):
        lm.generate(input_ids=ids, max_new_tokens=4, num_beams=2, output_logprobs=True, top_logprobs=3)
    for bad in (9, -1, 2.0, True):
        with pytest.raises(ValueError, match="logprobs"):
            lm.generate(input_ids=ids, max_new_tokens=4, output_logprobs=True, top_logprobs=bad)
    with pytest.raises(ValueError, match="logprobs"):
        lm.generate(input_ids=ids, max_new_tokens=4, top_logprobs=3)                # alternatives without the option
    with pytest.raises(ValueError, match="logprobs"):
        lm.generate_many([ids[0]], max_new_tokens=4, output_logprobs=True)
    with pytest.raises(ValueError, match="logprobs"):
        lm.generate_many([ids[0]], max_new_tokens=4, top_logprobs=2)
    for kw in (dict(), dict(output_logprobs=True), dict(output_logprobs=True, top_logprobs=8), dict(num_beams=2)):
        with pytest.raises(_Reached):                                               # legal: past the checks
            lm.generate(input_ids=ids, max_new_tokens=4, **kw)


def test_generate_hands_the_engine_its_logprobs_and_returns_them(monkeypatch):
    from radialog_amd.engine import RdxEngine
    lm = _model()
    ids = torch.ones(2, 40, dtype=torch.long)
    seen = []
    toks = torch.tensor([[5, 2, 0, 0], [7, 8, 9, 2]], dtype=torch.int32)
    lp = (torch.full((2, 4), -0.5), torch.zeros(2, 4, 3, dtype=torch.int32), torch.full((2, 4, 3), -1.5))

    class FakeEngine:
        def generate(self, *a, **kw):
            seen.append(kw)
            return (toks, None, 4, lp) if "logprobs" in kw else (toks, None, 4)

    monkeypatch.setattr(lm, "_ensure_engine", lambda: setattr(lm, "_engine", FakeEngine()))
    out = lm.generate(input_ids=ids, max_new_tokens=4, return_dict_in_generate=True, eos_token_id=2, pad_token_id=0)
    assert "logprobs" not in seen[-1] and not hasattr(out, "token_logprobs")      # the call of a model that never heard of the option
    out = lm.generate(input_ids=ids, max_new_tokens=4, return_dict_in_generate=True, eos_token_id=2, pad_token_id=0, output_logprobs=True, top_logprobs=3)
    assert seen[-1]["logprobs"] == 3
    assert tuple(out.token_logprobs.shape) == (2, 4) and tuple(out.top_logprobs[0].shape) == (2, 4, 3) and tuple(out.top_logprobs[1].shape) == (2, 4, 3)
    out = lm.generate(input_ids=ids, max_new_tokens=4, return_dict_in_generate=True, eos_token_id=2, pad_token_id=0, output_logprobs=True)
    assert seen[-1]["logprobs"] == 0
    for fn in (RdxEngine.generate, RdxEngine.prefill, RdxEngine.decode_step):
        assert "logprobs" in inspect.signature(fn).parameters
    assert callable(RdxEngine.set_logprobs) and callable(RdxEngine.get_logprobs)


def test_engine_argument_check_and_eos_masking():
    from radialog_amd.engine import check_top_logprobs, mask_logprobs_after_eos, mean_token_logprob
    assert check_top_logprobs(None) is None and check_top_logprobs(0) == 0 and check_top_logprobs(8) == 8
    for bad in (9, -1, 1.0, "3", True):
        with pytest.raises(ValueError, match="logprobs"):
            check_top_logprobs(bad)
    toks = torch.tensor([[5, 2, 0, 0], [7, 8, 9, 2], [2, 2, 0, 0], [4, 4, 4, 4]])
    c = torch.arange(16, dtype=torch.float32).view(4, 4) - 20.0
    i = torch.arange(32, dtype=torch.int32).view(4, 4, 2)
    l = -torch.arange(32, dtype=torch.float32).view(4, 4, 2) - 1.0
    mc, mi, ml = mask_logprobs_after_eos(toks, 2, c, i, l)
    done = torch.tensor([[0, 0, 1, 1], [0, 0, 0, 0], [0, 1, 1, 1], [0, 0, 0, 0]], dtype=torch.bool)
    assert bool((mc[done] == 0).all()) and bool((mi[done] == -1).all()) and bool((ml[done] == 0).all())
    assert torch.equal(mc[~done], c[~done]) and torch.equal(mi[~done], i[~done]) and torch.equal(ml[~done], l[~done])       # the EOS entry itself stays
    assert c[0, 2] == -18.0                                                          # the inputs are left alone
    for eos in (-1, None):
        uc, ui, ul = mask_logprobs_after_eos(toks, eos, c, i, l)
        assert torch.equal(uc, c) and torch.equal(ui, i) and torch.equal(ul, l)
    k0 = mask_logprobs_after_eos(toks, 2, c, i[:, :, :0], l[:, :, :0])
    assert k0[1].shape == (4, 4, 0) and torch.equal(k0[0], mc)
    m = mean_token_logprob(toks, 2, c)
    assert m.tolist() == [(-20.0 - 19.0) / 2, (-16.0 - 15.0 - 14.0 - 13.0) / 4, -12.0, (-8.0 - 7.0 - 6.0 - 5.0) / 4]


def test_the_entry_points_declare_the_logprobs_flag():
    for name in ("test.py", "demo.py", os.path.join("tools", "step_time.py")):
        assert '"--logprobs"' in open(os.path.join(REPO, name)).read(), name
    text = open(os.path.join(REPO, "test.py")).read()
    assert "output_logprobs=args.logprobs is not None" in text and 'res["mean_logprob"]' in text


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------------------------------
def test_abi_of_the_logprobs_calls():
    from radialog_amd import _lib, build
    raw = C.CDLL(_lib.LIB_PATH, mode=C.RTLD_GLOBAL)
    assert hasattr(raw, "rdx_set_logprobs") and hasattr(raw, "rdx_get_logprobs") and not hasattr(raw, "rdx_logprob_step_test")
    hooks = C.CDLL(_lib.HOOKS_PATH, mode=C.RTLD_GLOBAL)
    assert hasattr(hooks, "rdx_logprob_step_test")
    assert "rdx_logprob_step_test" in _lib.DEC_HOOK_SYMBOLS and "rdx_logprob_step_test" not in _lib.HOOK_SYMBOLS
    text = open(os.path.join(REPO, "include", "rdx.h")).read()
    assert re.search(r"#define RDX_MAX_TOP_LOGPROBS 8\b", text) and _lib.RDX_MAX_TOP_LOGPROBS == 8 == L.MAX_TOP
    assert re.search(r"int rdx_set_logprobs\(rdx_ctx\* ctx, int top_n\);", text)
    assert re.search(r"int rdx_get_logprobs\(rdx_ctx\* ctx, int batch, int n_steps, float\* chosen_host, int32_t\* top_ids_host, float\* top_lp_host\);", text)
    assert "logprob.hip" in build.SOURCES
    # without a context both calls fail cleanly
    lib = _lib.load()
    assert lib.rdx_set_logprobs(None, 3) == -1 and lib.rdx_get_logprobs(None, 1, 1, None, None, None) == -1
