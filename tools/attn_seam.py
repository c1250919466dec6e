#!/usr/bin/env python
"""Timeline across the attention -> o_proj seam of ONE fused launch (attn_oproj16_k) inside a real batch-1/2 decode step on the Vicuna-7B shapes
(rdx_gemv_trace 8; per-workgroup s_memrealtime stamps, 100 MHz):   python tools/attn_seam.py [B = 1] [layers = 5 20] [--ctx 170 400]
Prints a markdown table of min / median / max per event, in us from the launch's first workgroup entry, for every (context, layer), and the three
gaps of the seam. 64 graph steps run in front of every traced step. Wave 0 of a traced o_proj workgroup waits for its first weight KiB (that is
how it is observed), which a product launch never does: read the table for the order and size of the gaps, and rocprofv3 for the launch's duration."""
import os
import sys

os.environ.setdefault("RDX_DEBUG_HOOKS", "1")      # this tool drives the trace hooks of librdx_hooks.so (include/rdx_hooks.h)
import numpy as np  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from radialog_amd import _lib, synth  # noqa: E402
from radialog_amd.config import full_cfg  # noqa: E402
from radialog_amd.engine import RdxEngine, synth_getter  # noqa: E402

argv = sys.argv[1:]
ctxs = [170, 400]
if "--ctx" in argv:
    i = argv.index("--ctx")
    ctxs = [int(x) for x in argv[i + 1:]]
    argv = argv[:i]
B = int(argv[0]) if argv else 1
layers = [int(x) for x in argv[1:]] or [5, 20]
STEPS = 64
cfg = full_cfg()
n_attn = cfg.llama.heads * B
eng = RdxEngine(cfg, dtype="bf16", device=0, max_batch=B, max_len=512, lora=True, vision=False)
eng.load_weights(synth_getter(cfg, eng.device, lora=True), vision=False)
qf = synth.synth("u.qf", (B, 32, cfg.llama.qformer_dim), -1.0, 1.0).to(eng.device)


def row(name, v):
    v = v[v > 0]
    return f"| {name} | {v.min():.2f} | {np.median(v):.2f} | {v.max():.2f} |" if len(v) else f"| {name} | - | - | - |"


for ctx in ctxs:
    ids = synth.synth_prompt_ids(B, ctx - STEPS, vocab=cfg.llama.vocab, pad_rows=(B > 1), seed=7).to(eng.device)
    for layer in layers:
        eng.generate(ids, qf, max_new=STEPS, eos_id=-1, pad_id=0, use_graph=True)     # a warm, mid-answer state; the traced step follows it
        eng.gemv_trace(_lib.TRACE_ATTN_OPROJ, layer)                                  # first traced step: warms the eager launch path
        eng.generate(ids, qf, max_new=STEPS, eos_id=-1, pad_id=0, use_graph=True)
        raw = eng.gemv_trace(_lib.TRACE_ATTN_OPROJ, layer).numpy().astype(np.float64)
        live = raw[raw[:, 0] > 0]
        t0 = live[:, 0].min()
        us = np.where(raw > 0, (raw - t0) / 100.0, 0.0)
        a, o = us[:n_attn], us[n_attn:][raw[n_attn:, 0] > 0]
        print(f"\n### context {ctx}, layer {layer}, batch {B}: {n_attn} attention workgroups + {len(o)} o_proj workgroups\n")
        print("| event (us from the first entry) | min | median | max |\n|---|---|---|---|")
        print(row("attn: workgroup entry", a[:, 0]))
        print(row("attn: qkv row loaded (new token done, wave 0)", a[:, 1]))
        print(row("attn: scores done", a[:, 2]))
        print(row("attn: softmax done", a[:, 3]))
        print(row("attn: P.V reduced", a[:, 4]))
        print(row("attn: output stored (stores issued)", a[:, 5]))
        print(row("attn: arrival (stores acknowledged)", a[:, 6]))
        print(row("o_proj: workgroup entry", o[:, 0]))
        print(row("o_proj: first weight KiB back (wave 0)", o[:, 5]))
        print(row("o_proj: inputs ready", o[:, 3]))
        print(row("o_proj: first MFMA (row staged)", o[:, 6]))
        print(row("o_proj: K loop done (wave 0)", o[:, 1]))
        print(row("o_proj: end of the workgroup", o[:, 7]))
        last = a[:, 5].max()
        print(f"\nlast output stored {last:.2f} us -> inputs ready +{np.median(o[:, 3]) - last:.2f} (median; max +{o[:, 3].max() - last:.2f}); "
              f"inputs ready -> first MFMA +{np.median(o[:, 6] - o[:, 3]):.2f} (median); first MFMA -> end +{np.median(o[:, 7] - o[:, 6]):.2f} (median); "
              f"launch span {us[:, 7].max():.2f} us")
eng.close()
