"""The prompt path, family by family, computes the bits it computed before its host code was rebuilt around one plan, one argument builder per
unit and one layer loop per kernel family (csrc/api_dispatch.hip: prompt_plan, prompt_unit, prompt_attention; csrc/api_llama.hip: prompt_rows,
prompt_tiles, prompt_fp8).

That change touched no kernel, no launch geometry and no kernel argument, so the bar is equality of bits. tests/golden/prompt_bits.json holds
SHA-256 digests recorded on the commit BEFORE the change, dbc9de3 "Decode: opt-in fp8 KV cache" (`python tests/test_gpu_prompt_bits.py --write
FILE [KEY ...]` run from the root of the tree to record: it imports radialog_amd from the working directory; with KEYs only those engines are
recorded and merged into FILE). Every case was recorded twice there and the two recordings were equal. A prompt's digest covers the tokens and
all score rows of three eagerly generated tokens and, for both layers, K and V of the prompt's rows and slots as the cache stores them (the
model dtype's bits; on an fp8 KV cache the e4m3 codes and the row exponents). The caches start as zeros and every digested slot is written.

The prompt shapes are the smallest at each edge of the dispatch: the <= 32-row kernels, the tiles family with a ragged last row tile, the
K-split down_proj and its pending slabs, the 24-pad-row threshold (104 / 105 rows), the 128-row edge, the 12-tile limit of the row-block
kernels (192 / 193), the pad edge below 384 rows (360 / 361) and the tile GEMMs above it; two and three prompts, a left-padded row, no image;
the `prompt_blk` and `flash_min` switches; append behind kept slots, a row session's refill into row 1, the scoring pass; f16; fp8 weights
(gemm8); the fp8 KV cache (T no multiple of 16: the staging stride differs from T); int4 weights; and the small config, whose widths the
weight-stationary kernel refuses, so that the rows family runs at every M.

A second test holds the prompt path to refusing BEFORE it has any effect: a refused prefill leaves the conversation it refused to replace
as it was."""
import hashlib
import json
import os
import sys

if __name__ == "__main__":          # recording run (--write): the tree in the working directory is the one that is recorded
    sys.path.insert(0, os.getcwd())

import pytest
import torch

from radialog_amd import synth
from radialog_amd.config import LlamaCfg, RaDialogCfg, small_cfg

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "prompt_bits.json")
N_NEW = 3

# engine key -> (widths, constructor arguments, prompts); a prompt = (B, T, variant)
PLAIN = [(1, 32, ""), (1, 33, ""), (1, 104, ""), (1, 105, ""), (1, 128, ""), (1, 129, ""), (1, 192, ""), (1, 193, ""), (1, 360, ""), (1, 361, ""),
         (1, 385, ""), (2, 72, ""), (3, 120, ""), (1, 40, "noimg"), (1, 33, "prompt_blk=0"), (1, 129, "prompt_blk=0"), (2, 72, "flash_min=1")]
ENGINES = {
    "prod2-bf16": ("prod2", dict(dtype="bf16", max_batch=3), PLAIN + [(1, 72, "append"), (1, 40, "rows"), (2, 72, "score")]),
    "prod2-f16": ("prod2", dict(dtype="f16", max_batch=2), [(1, 33, ""), (1, 128, ""), (2, 72, "")]),
    "prod2-bf16-w8": ("prod2", dict(dtype="bf16", max_batch=2, weights_fp8=True), [(1, 32, ""), (1, 33, ""), (2, 72, ""), (1, 385, "")]),
    "prod2-bf16-kv8": ("prod2", dict(dtype="bf16", max_batch=2, kv_fp8=True), [(1, 33, ""), (1, 128, ""), (2, 72, "")]),
    "prod2-bf16-w8-kv8": ("prod2", dict(dtype="bf16", max_batch=1, weights_fp8=True, kv_fp8=True), [(1, 40, "")]),
    "prod2-bf16-w4": ("prod2", dict(dtype="bf16", max_batch=1, weights_w4=True), [(1, 33, "")]),
    "small-bf16": ("small", dict(dtype="bf16", max_batch=4), [(1, 40, ""), (4, 72, "")]),
}


def _case(B, T, variant):
    return f"B{B}-T{T}" + (f"-{variant}" if variant else "")


def _engine(which, max_len=512, **kw):
    from radialog_amd.engine import RdxEngine, synth_getter
    cfg = small_cfg() if which == "small" else RaDialogCfg(llama=LlamaCfg(layers=2, qformer_dim=192))
    eng = RdxEngine(cfg, device=0, max_len=max_len, lora=True, vision=False, **kw)
    eng.load_weights(synth_getter(cfg, eng.device, lora=True), vision=False)
    return eng, cfg


def _prompt(cfg, B, T):
    ids = synth.synth_prompt_ids(B, T, vocab=cfg.llama.vocab, img_offset=6, pad_rows=False, seed=33)
    if B > 1:                                  # left-pad row 1 by 5 (pad id 0), keep 32 <IMG> inside
        ids[1] = torch.cat([torch.zeros(5, dtype=torch.long), ids[1, : T - 5]])
    return ids, synth.synth("t.qf2", (B, 32, cfg.llama.qformer_dim), -1.0, 1.0)


def _bits(h, t):
    t = t.detach().cpu().contiguous()
    h.update((t.view(torch.int16) if t.dtype in (torch.float16, torch.bfloat16) else t).numpy().tobytes())


def _generate_digest(eng, cfg, ids, qf, **kw):
    """Tokens, all score rows, then K and V of both layers at rows [:B], slots [:T], as the cache stores them."""
    B, T = ids.shape
    toks, scores, n = eng.generate(ids, qf, max_new=N_NEW, eos_id=-1, output_scores=True, use_graph=False, **kw)
    assert n == N_NEW
    h = hashlib.sha256()
    _bits(h, toks.long())
    _bits(h, scores)
    for layer in range(cfg.llama.layers):
        for which in (0, 1):
            if eng.kv_fp8:
                codes, exps = eng.kv_read_codes(layer, which, B)
                _bits(h, codes[:, :, :T])
                _bits(h, exps[:, :, :T])
            else:
                _bits(h, eng.kv_read(layer, which, B)[:, :, :T])
    return h.hexdigest(), toks[:, :n].cpu().long().clone()


def _append_digest(eng, cfg, B, T):
    """Two turns with reuse_prefix: turn 2 appends 41 prompt tokens (the tiles family) behind the kept slots."""
    ids, qf = _prompt(cfg, B, T)
    _, answer = _generate_digest(eng, cfg, ids, qf, reuse_prefix=True)
    more = synth.synth_prompt_ids(B, 40, vocab=cfg.llama.vocab, img_offset=50, seed=34)[:, 2:]       # 38 plain tokens: neither BOS, pad nor <IMG>
    digest, _ = _generate_digest(eng, cfg, torch.cat([ids, answer, more], dim=1), qf, reuse_prefix=True)
    assert eng.last_kept_prefix == T + N_NEW - 1
    return digest


def _rows_digest(eng, cfg, T):
    """A row session of two rows: one prompt refilled into row 1 through the staging row, then two steps."""
    ids, qf = _prompt(cfg, 1, T)
    h = hashlib.sha256()
    with eng.row_session(rows=2, stage=1, cap=8, eos_id=-1) as ses:
        _bits(h, ses.refill(ids, None, qf, [1], want_logits=True))
        for _ in range(2):
            _bits(h, ses.step(1, want_logits=True))
        _bits(h, ses.read_tokens(1).long())
    return h.hexdigest()


def _score_digest(eng, cfg, B, T):
    ids, qf = _prompt(cfg, B, T)
    labels = ids.clone()
    labels[:, :40] = -100
    logprob, top1, _ = eng.score(ids, qf, labels, want_top1=True)
    eng.sync()
    h = hashlib.sha256()
    _bits(h, logprob)
    _bits(h, top1)
    return h.hexdigest()


def _engine_digests(key):
    """{case: digest} of one engine's prompts, run in the listed order."""
    which, kw, prompts = ENGINES[key]
    eng, cfg = _engine(which, **kw)
    got = {}
    for B, T, variant in prompts:
        name, _, value = variant.partition("=")
        if variant == "append":
            got[_case(B, T, variant)] = _append_digest(eng, cfg, B, T)
        elif variant == "rows":
            got[_case(B, T, variant)] = _rows_digest(eng, cfg, T)
        elif variant == "score":
            got[_case(B, T, variant)] = _score_digest(eng, cfg, B, T)
        else:
            if value:
                eng.set_option(name, int(value))
            ids, qf = _prompt(cfg, B, T)
            got[_case(B, T, variant)], _ = _generate_digest(eng, cfg, ids, None if variant == "noimg" else qf)
            if value:                              # back to the default for the prompts behind it
                eng.set_option(name, {"prompt_blk": 1, "flash_min": 512}[name])
    eng.close()
    return got


@pytest.mark.parametrize("key", list(ENGINES))
def test_prompt_computes_the_recorded_bits(key):
    """Every prompt of the engine: tokens, scores and the K / V rows the prompt wrote are bit for bit what the prompt path computed before its
    host code was rebuilt."""
    with open(GOLDEN) as f:
        want = json.load(f)[key]
    got = _engine_digests(key)
    for case in got:
        print(f"{key} {case}: {got[case][:16]} (recorded {want.get(case, '?')[:16]}){'' if got[case] == want.get(case) else '  DIFFERS'}")
    assert got == want


def _conversation(eng, ids, qf, refused_call=None):
    """Prefill + 5 decode steps; `refused_call` runs after the first step. Returns (tokens, [logits of the prefill and of every step])."""
    toks, lg = eng.prefill(ids, qf, max_new=6, eos_id=-1)
    logits = [lg.clone()]
    for step in range(5):
        toks, lg = eng.decode_step()
        logits.append(lg.clone())
        if step == 0 and refused_call:
            refused_call()
    return toks.clone(), logits


@pytest.mark.parametrize("kv_fp8", [False, True], ids=["rows33", "kv8-append"])
def test_refused_prefill_leaves_the_conversation_alone(kv_fp8):
    """A prefill that is refused changes nothing: the conversation it would have replaced goes on to the tokens and logits it reaches without
    the refused call in between. rows33: rdx_prefill of 33 prompts on widths without the row-block family. kv8-append: a raw rdx_prefill_append
    on an fp8 KV cache (-1, refused by its entry point).

    rows33 was asked for on a context of max_batch 33, where the prompt path's own refusal (-8, "more than 32 rows per context need the Vicuna-7B
    widths") would answer. No such context exists: rdx_finalize_weights refuses max_batch > 32 on these widths, and on the production widths
    every batch up to max_batch has the row-block family, so that refusal is a guard no public call reaches (like the prompt path's kv_fp8
    one, which the append and row-session entry points pre-empt). The context here holds the 32 rows its widths allow, and the 33-prompt
    call gets the refusal that such a call gets today: -1, batch outside [1, 32]."""
    from radialog_amd._lib import check, RdxError
    from radialog_amd.engine import _ptr
    eng, cfg = _engine("small", max_len=128, dtype="bf16", max_batch=32, kv_fp8=kv_fp8)
    ids, qf = _prompt(cfg, 1, 40)
    big, big_qf = _prompt(cfg, 33, 40)
    big32 = big.to(device=eng.device, dtype=torch.int32).contiguous()
    big_qf = big_qf.to(device=eng.device, dtype=torch.float32).contiguous()
    out = torch.zeros(33, 6, dtype=torch.int32, device=eng.device)
    torch.cuda.synchronize(eng.device)

    def refused():
        if kv_fp8:
            with pytest.raises(RdxError, match=r"rdx_prefill_append failed \(-1\): rdx_prefill_append: not built for the fp8 KV cache \(kv_fp8\): "
                                               "the kept prefix is not held in the model dtype"):
                check(eng.ctx, eng.lib.rdx_prefill_append(eng.ctx, _ptr(big32[:1, :8].contiguous()), 1, 8, 40, 6, -1, 0, _ptr(out), None), "rdx_prefill_append")
        else:
            with pytest.raises(RdxError, match=r"rdx_prefill failed \(-1\): rdx_prefill: batch 33 outside \[1, 32\]"):
                check(eng.ctx, eng.lib.rdx_prefill(eng.ctx, _ptr(big32), None, 33, 40, _ptr(big_qf), 6, -1, 0, _ptr(out), None), "rdx_prefill")

    want_toks, want_logits = _conversation(eng, ids, qf)
    got_toks, got_logits = _conversation(eng, ids, qf, refused)
    eng.close()
    assert torch.equal(got_toks, want_toks)
    for step, (got, want) in enumerate(zip(got_logits, want_logits)):
        assert torch.equal(got, want), f"logits of step {step} differ behind the refused call"


if __name__ == "__main__":
    path = sys.argv[sys.argv.index("--write") + 1]
    only = sys.argv[sys.argv.index("--write") + 2:]
    got = {}
    if only and os.path.exists(path):
        with open(path) as f:
            got = json.load(f)
    for key in ENGINES:
        if not only or key in only:
            got[key] = _engine_digests(key)
            print(key, got[key], flush=True)
    with open(path, "w") as f:
        json.dump(got, f, indent=1, sort_keys=True)
        f.write("\n")
