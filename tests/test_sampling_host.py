"""Sampled decoding on the host: the Philox generator against its published known answers and against the library's own host export, the
restatement of tests/_sampling.py against hand-computed cases and transformers' warpers, its draw frequencies, LlamaForCausalLM.generate's
argument checks (no engine is built) and the C ABI of rdx_set_sampling. tests/test_gpu_sampling.py holds the kernel to the restatement."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import _sampling as SP

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")


# ---- Philox -------------------------------------------------------------------------------------------------------------------------------------
KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd))]


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox_known_answers(ctr, key, want):
    assert SP.philox4x32_10(ctr, key) == want


def test_library_host_export_equals_the_restated_philox():
    from radialog_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(5)
    triples = [(0, 0, 0), (2 ** 64 - 1, 2 ** 32 - 1, 2 ** 32 - 1), (1 << 32, 0, 1), (7, 32, 299)]
    triples += [(int(rng.integers(0, 2 ** 64, dtype=np.uint64)), int(rng.integers(0, 128)), int(rng.integers(0, 512))) for _ in range(996)]
    out = C.c_uint32(0)
    for seed, row, draw in triples:
        assert lib.rdx_sample_u24_host(seed, row, draw, C.byref(out)) == 0
        assert out.value == SP.u24(seed, row, draw) and out.value < 1 << 24, (seed, row, draw)
    assert lib.rdx_sample_u24_host(1, 2, 3, None) == -1
    # the key is the seed's two halves, the counter (row, draw, 0, 0), the result word 0 without its low byte
    assert SP.u24((0x299f31d0 << 32) | 0xa4093822, 5, 9) == SP.philox4x32_10((5, 9, 0, 0), (0xa4093822, 0x299f31d0))[0] >> 8


# ---- the warpers: hand-computed cases ---------------------------------------------------------------------------------------------------------------
def _row(vals, dtype=torch.float16):
    return torch.tensor(vals, dtype=torch.float32).to(dtype)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_hand_cases(dtype):
    x = _row([1.0, 3.0, -2.0, 3.0, 0.5, 2.0, -INF, 2.0], dtype)
    V = x.numel()
    # k = 1: the argmax's value group (here two equal maxima: ties with the k-th value stay)
    out, kept, gap = SP.warp_row(x, 1.0, 1, 1.0)
    assert kept.tolist() == [False, True, False, True, False, False, False, False] and gap == INF
    assert out[kept].tolist() == [3.0, 3.0] and bool((out[~torch.from_numpy(kept)] == -INF).all())
    # a single maximum: k = 1 is the argmax
    y = x.clone(); y[3] = 2.5
    assert SP.warp_row(y, 1.0, 1, 1.0)[1].nonzero()[0].tolist() == [1]
    # k >= V is off, k = 0 is off: the row comes back as it went in (the -inf it held included)
    for k in (0, V, V + 5):
        out, kept, _ = SP.warp_row(x, 1.0, k, 1.0)
        assert kept.all() and torch.equal(out.view(torch.int16), x.view(torch.int16))
    # the whole group of the k-th value stays: k = 3 -> 3, 3 and both 2s
    assert SP.warp_row(x, 1.0, 3, 1.0)[1].tolist() == [False, True, False, True, False, True, False, True]
    # p -> 0 keeps the maximum's value group, and only it
    assert SP.warp_row(x, 1.0, 0, 1e-6)[1].tolist() == [False, True, False, True, False, False, False, False]
    # top-p by hand: w = e^(s - 3); ascending cumulative mass decides
    w = np.exp(np.array([1.0, 3.0, -2.0, 3.0, 0.5, 2.0, -np.inf, 2.0]) - 3.0)
    tot = w.sum()
    M_half, M_one, M_two = (w[2] + w[4]) / tot, (w[2] + w[4] + w[0]) / tot, (w[2] + w[4] + w[0] + w[5] + w[7]) / tot
    p = 1.0 - (M_one + M_two) / 2                                   # the boundary between the value 1 and the value-2 group
    out, kept, gap = SP.warp_row(x, 1.0, 0, p)
    assert kept.tolist() == [False, True, False, True, False, True, False, True]
    assert abs(gap - (M_two - M_one) / 2) < 1e-6 and M_half < M_one
    # temperature: fp32 division, one rounding; dropped elements are -inf, kept ones the scaled values
    out, kept, _ = SP.warp_row(x, 0.7, 2, 1.0)
    want = (x.float() / torch.tensor(0.7, dtype=torch.float32)).to(dtype)
    assert torch.equal(out[torch.from_numpy(kept)], want[torch.from_numpy(kept)]) and bool((out[torch.from_numpy(~kept)] == -INF).all())
    assert torch.equal(SP.scale(x, 1.0).view(torch.int16), x.view(torch.int16))


def _llm_like_rows(B, V, seed, dtype=torch.float32):
    """A broad tail and a few dozen likely tokens, as a language model's rows are."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, V, generator=g) * 2 - 8
    for b in range(B):
        head = torch.randperm(V, generator=g)[: min(40, V // 2)]
        x[b, head] = torch.randn(head.numel(), generator=g) * 3 + 6
    return x.to(dtype)


def test_kept_sets_equal_transformers_warpers():
    lp = pytest.importorskip("transformers.generation.logits_process")
    ids = torch.zeros(1, 1, dtype=torch.long)
    checked = 0
    for V in (61, 1000, 32001):
        x = _llm_like_rows(6, V, seed=V)
        for t, k, p in ((1.0, 0, 1.0), (0.7, 50, 1.0), (1.3, 0, 0.9), (0.8, 40, 0.95), (1.0, 1, 1.0), (1.0, V + 3, 1.0), (2.0, 0, 0.5)):
            for b in range(x.shape[0]):
                out, kept, gap = SP.warp_row(x[b], t, k, p)
                if gap < 1e-4:                                      # transformers sums fp32 probabilities: a row this close to the boundary proves nothing
                    continue
                want = x[b:b + 1].clone()
                if t != 1.0:
                    want = lp.TemperatureLogitsWarper(t)(ids, want)
                if k > 0:
                    want = lp.TopKLogitsWarper(k)(ids, want)
                if p < 1.0:
                    want = lp.TopPLogitsWarper(p)(ids, want)
                assert torch.equal(torch.isfinite(want[0]), torch.from_numpy(kept) & torch.isfinite(x[b])), (V, t, k, p, b)
                assert torch.allclose(out[torch.from_numpy(kept)], want[0][torch.from_numpy(kept)], rtol=1e-6, atol=0)
                checked += 1
    assert checked >= 100


def test_draw_frequencies_follow_the_probabilities():
    x = _row([0.0, 1.5, -1.0, 2.0, 0.25, -3.0, 1.0, 0.5], torch.float16).unsqueeze(0)
    N = 20000
    scores, _, _ = SP.warp_row(x[0], 0.9, 6, 1.0)
    F = SP.cdf(scores)
    prob = np.diff(np.concatenate([[0.0], F]))
    counts = np.zeros(8)
    for n in range(N):
        counts[SP.draw(scores, SP.u24(1234, 0, n))] += 1
    assert counts[prob == 0].sum() == 0 and (prob == 0).sum() == 2
    sigma = np.sqrt(N * prob * (1 - prob))
    assert bool((np.abs(counts - N * prob) <= 4 * sigma + 1e-9).all()), (counts, N * prob)
    # the draw is the first index whose inclusive mass exceeds the target, and it obeys the acceptance rule it will be held to
    for n in range(200):
        u = SP.u24(99, 3, n)
        assert SP.accepts(scores, SP.draw(scores, u), u)[0]


def test_sample_rows_uses_row_and_draw_index():
    x = _llm_like_rows(5, 61, seed=3, dtype=torch.float16)
    x[1:] = x[0]
    a = SP.sample_rows(x, [0] * 5, (1.0, 0, 1.0, 11))
    assert a[2] == [SP.u24(11, b, 0) for b in range(5)] and len(set(a[2])) == 5
    assert SP.sample_rows(x, [3] * 5, (1.0, 0, 1.0, 11))[2] != a[2] and SP.sample_rows(x, [0] * 5, (1.0, 0, 1.0, 12))[2] != a[2]


# ---- LlamaForCausalLM.generate: the checks run before any engine exists -------------------------------------------------------------------------
class _Reached(Exception):
    pass


def _model(enable_sampling=True):
    from radialog_amd.modeling_llama_imgemb import LlamaForCausalLM
    lm = LlamaForCausalLM.from_pretrained(None, torch_dtype=torch.float16, synthetic=True)
    if enable_sampling:
        lm.enable_sampling = True
    return lm


def test_sampling_is_a_switch_on_the_model(monkeypatch):
    """A model nobody switched over refuses do_sample=True as before; with `enable_sampling = True` -- set on the model or on its peft wrapper --
    the same call goes past the checks (the stubbed _ensure_engine raises its sentinel) without NotImplementedError."""
    from radialog_amd.modeling_llama_imgemb import PeftModelForCausalLM
    ids = torch.ones(1, 40, dtype=torch.long)
    lm = _model(enable_sampling=False)
    monkeypatch.setattr(lm, "_ensure_engine", lambda: (_ for _ in ()).throw(_Reached()))
    with pytest.raises(NotImplementedError, match="enable_sampling"):
        lm.generate(input_ids=ids, max_new_tokens=4, do_sample=True, seed=7)
    with pytest.raises(_Reached):
        lm.generate(input_ids=ids, max_new_tokens=4)
    PeftModelForCausalLM(lm).enable_sampling = True
    with pytest.raises(_Reached):
        lm.generate(input_ids=ids, max_new_tokens=4, do_sample=True)
    lm.enable_sampling = False
    with pytest.raises(NotImplementedError):
        lm.generate(input_ids=ids, max_new_tokens=4, do_sample=True)


def test_generate_refuses_bad_sampling_arguments_before_building_an_engine(monkeypatch):
    lm = _model()
    monkeypatch.setattr(lm, "_ensure_engine", lambda: (_ for _ in ()).throw(_Reached()))
    ids = torch.ones(1, 40, dtype=torch.long)
    for kw in (dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=2), dict(temperature="0.7"), dict(temperature=float("nan")),
               dict(top_k=-1), dict(top_k=2.5), dict(top_k="5"), dict(top_p=-0.1), dict(top_p=1.5), dict(top_p=float("nan")),
               dict(typical_p=0.9), dict(epsilon_cutoff=3e-4), dict(eta_cutoff=1e-3), dict(num_beams=2), dict(seed=-1), dict(seed=1.5)):
        with pytest.raises(ValueError):
            lm.generate(input_ids=ids, max_new_tokens=4, do_sample=True, **kw)
    for kw in (dict(), dict(temperature=1), dict(temperature=0.7, top_k=0, top_p=0.9), dict(top_p=1), dict(top_p=0.0), dict(typical_p=1.0, epsilon_cutoff=0.0),
               dict(repetition_penalty=1.2, no_repeat_ngram_size=3), dict(seed=2 ** 64 - 1)):
        with pytest.raises(_Reached):                               # legal: past the checks, and no NotImplementedError
            lm.generate(input_ids=ids, max_new_tokens=4, do_sample=True, **kw)
    with pytest.raises(_Reached):                                   # greedy search ignores the warper arguments, as transformers does
        lm.generate(input_ids=ids, max_new_tokens=4, temperature=0.0, top_k=-3)


def test_generate_hands_the_engine_its_sampling(monkeypatch):
    from radialog_amd.engine import RdxEngine, Sampling
    import inspect
    lm = _model()
    ids = torch.ones(1, 40, dtype=torch.long)
    seen = []

    class FakeEngine:
        def generate(self, *a, **kw):
            seen.append(kw)
            raise _Reached()

    monkeypatch.setattr(lm, "_ensure_engine", lambda: setattr(lm, "_engine", FakeEngine()))

    def call(**kw):
        with pytest.raises(_Reached):
            lm.generate(input_ids=ids, max_new_tokens=4, **kw)
        return seen[-1]["sampling"]

    assert call() is None and call(do_sample=False, temperature=0.5) is None
    s = call(do_sample=True, seed=7)
    assert s == Sampling(1.0, 50, 1.0, 7)                           # top_k = 50: transformers' GenerationConfig default
    assert call(do_sample=True, temperature=0.7, top_k=0, top_p=0.9, seed=3) == Sampling(0.7, 0, 0.9, 3)
    assert 0 < call(do_sample=True, top_p=0.0, seed=3).top_p < 1e-30
    # seed=None: 63 bits from torch's default CPU generator -- reproducible under torch.manual_seed, different from draw to draw
    torch.manual_seed(1234)
    a, a2 = call(do_sample=True), call(do_sample=True)
    torch.manual_seed(1234)
    b = call(do_sample=True)
    assert a == b and a.seed != a2.seed and 0 <= a.seed < 2 ** 63
    for fn in (RdxEngine.generate, RdxEngine.prefill, RdxEngine.decode_step):
        assert "sampling" in inspect.signature(fn).parameters
    assert Sampling.of((0.8, 50, 0.95, 1)) == Sampling(0.8, 50, 0.95, 1) and Sampling.of(None) is None
    for bad in ((0.0, 0, 1.0, 0), (float("inf"), 0, 1.0, 0), (1.0, -1, 1.0, 0), (1.0, 0, 0.0, 0), (1.0, 0, 1.1, 0), (1.0, 0, 1.0, -1), (1.0, 0, 1.0, 1 << 64)):
        with pytest.raises(ValueError):
            Sampling(*bad)


def test_the_report_tool_declares_the_sampling_flags():
    text = open(os.path.join(REPO, "test.py")).read()
    for flag in ("--do_sample", "--temperature", "--seed"):
        assert f'"{flag}"' in text
    assert "lang_model.enable_sampling = args.do_sample" in text and "do_sample=args.do_sample" in text and "temperature=args.temperature" in text and "seed=args.seed" in text


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------------------------
def test_abi_of_rdx_set_sampling():
    from radialog_amd import _lib
    raw = C.CDLL(_lib.LIB_PATH, mode=C.RTLD_GLOBAL)
    assert hasattr(raw, "rdx_set_sampling") and not hasattr(raw, "rdx_sample_test") and not hasattr(raw, "rdx_sample_u24_host")
    hooks = C.CDLL(_lib.HOOKS_PATH, mode=C.RTLD_GLOBAL)
    assert hasattr(hooks, "rdx_sample_test") and hasattr(hooks, "rdx_sample_u24_host")
    # the ctypes mirror against the header's declaration, laid out by the C rules for these types on x86-64
    text = open(os.path.join(REPO, "include", "rdx.h")).read()
    m = re.search(r"typedef struct rdx_sampling \{([^}]*)\} rdx_sampling;", text)
    fields = [f.split() for f in m.group(1).split(";") if f.strip()]
    assert fields == [["int", "do_sample"], ["float", "temperature"], ["int", "top_k"], ["float", "top_p"], ["uint64_t", "seed"]]
    S = _lib.RdxSampling
    assert [n for n, _ in S._fields_] == [f[1] for f in fields]
    assert C.sizeof(S) == 24 and [getattr(S, n).offset for n, _ in S._fields_] == [0, 4, 8, 12, 16]
    assert re.search(r"int rdx_set_sampling\(rdx_ctx\* ctx, const rdx_sampling\* s\);", text)
    lib = _lib.load()
    assert lib.rdx_set_sampling(None, None) == -1 and lib.rdx_set_sampling(None, C.byref(S(1, 1.0, 0, 1.0, 0))) == -1        # no context
