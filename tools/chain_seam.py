#!/usr/bin/env python
"""Timeline across the down_proj -> QKV seam of ONE chained launch inside a real batch-1/2 decode step on the Vicuna-7B shapes
(rdx_gemv_trace 7; per-workgroup s_memrealtime stamps, 100 MHz):   python tools/chain_seam.py [B = 1] [layers to trace = 5 6 20]
Prints a markdown table of min / median / max per event, in us from the launch's first workgroup entry. Wave 0 of a traced workgroup waits for
its first weight KiB (that is how it is observed), which a product launch never does: read the table for the order and size of the gaps, and
rdx_time(7) / rocprofv3 for the duration of the launch."""
import os
import sys

os.environ.setdefault("RDX_DEBUG_HOOKS", "1")      # this tool drives the trace hooks of librdx_hooks.so (include/rdx_hooks.h)
import numpy as np  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from radialog_amd import synth  # noqa: E402
from radialog_amd.config import full_cfg  # noqa: E402
from radialog_amd.engine import RdxEngine, synth_getter  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 1
layers = [int(x) for x in sys.argv[2:]] or [5, 6, 20]
cfg = full_cfg()
nwg = cfg.llama.hidden // 16
eng = RdxEngine(cfg, dtype="bf16", device=0, max_batch=B, max_len=512, lora=True, vision=False)
eng.load_weights(synth_getter(cfg, eng.device, lora=True), vision=False)
ids = synth.synth_prompt_ids(B, 160, vocab=cfg.llama.vocab, pad_rows=(B > 1), seed=7).to(eng.device)
qf = synth.synth("u.qf", (B, 32, cfg.llama.qformer_dim), -1.0, 1.0).to(eng.device)


def row(name, v):
    v = v[v > 0]
    return f"| {name} | {v.min():.2f} | {np.median(v):.2f} | {v.max():.2f} |" if len(v) else f"| {name} | - | - | - |"


for layer in layers:
    eng.generate(ids, qf, max_new=64, eos_id=-1, pad_id=0, use_graph=True)     # a warm, mid-answer state; the traced step follows it
    eng.gemv_trace(7, layer)                                                    # first traced step: warms the eager launch path
    eng.generate(ids, qf, max_new=64, eos_id=-1, pad_id=0, use_graph=True)
    raw = eng.gemv_trace(7, layer).numpy().astype(np.float64)
    t0 = raw[:nwg, 0].min()
    us = np.where(raw > 0, (raw - t0) / 100.0, 0.0)
    d, q = us[:nwg], us[nwg:][us[nwg:, 0] > 0]
    print(f"\n### layer {layer} -> {layer + 1}, batch {B}: {nwg} down_proj workgroups + {len(q)} QKV workgroups\n")
    print("| event (us from the first entry) | min | median | max |\n|---|---|---|---|")
    print(row("down: workgroup entry", d[:, 0]))
    print(row("down: last weight chunk consumed (K loop done, wave 0)", d[:, 1]))
    print(row("down: tile stored", d[:, 7]))
    print(row("down: arrival (stores drained, counter bumped)", d[:, 2]))
    print(row("QKV: workgroup entry", q[:, 0]))
    print(row("QKV: first weight KiB back (wave 0)", q[:, 5]))
    print(row("QKV: inputs ready (all arrivals seen)", q[:, 3]))
    print(row("QKV: first MFMA (row normalised and staged)", q[:, 6]))
    print(row("QKV: K loop done (wave 0)", q[:, 1]))
    print(row("QKV: end of the workgroup", q[:, 7]))
    print(f"\nlast arrival {d[:, 2].max():.2f} us -> inputs ready (median) {np.median(q[:, 3]):.2f} -> first MFMA (median) {np.median(q[:, 6]):.2f}; "
          f"launch span {us[:, 7].max():.2f} us")
eng.close()
