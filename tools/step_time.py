#!/usr/bin/env python
"""Decode-step time per batch size (README's batch table, VERDICT r4 "next" 4): Vicuna-7B shapes, bf16 (or --dtype f16), prompt 160 tokens,
(a) the hipGraph step replayed at context ~168 (rdx_time unit 0), (b) the mean step of a 256-token greedy decode (contexts 160 .. 415, what
bench.py averages), with the HBM fraction (weights + KV of SURVEY 8d over 8 TB/s). `--ab` repeats every batch with the one-row-tile family
off (rdx_set_option xs16 0: the 32-row kernels of xstat32.hip). python tools/step_time.py [--batches 1,2,4,8,12,16,32] [--ab] [--fp8 | --w4] [--kv8] [--logprobs N]
(--kv8: the fp8 KV cache, RdxEngine(kv_fp8=True); the HBM fraction then prices KV at 1 + 1/128 bytes per element instead of 2, and 1-2 rows run the generic family)
(--logprobs N: every step also computes the generation log-probs, RdxEngine.generate(logprobs=N): logprob_step_k behind the selection, the lm_head writing its rows)
(--w4: int4 group-quantised projections, RdxEngine(weights_w4=True); the HBM fraction then prices the int4 units at 4.125 bits at 1-16 rows, o_proj and the lm_head at 16, and everything at 16 from 17 rows)."""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from radialog_amd import synth  # noqa: E402
from radialog_amd.config import full_cfg  # noqa: E402
from radialog_amd.engine import RdxEngine, synth_getter  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,2,3,4,8,12,16,32")
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--ab", action="store_true")
    ap.add_argument("--fp8", action="store_true")
    ap.add_argument("--w4", action="store_true")
    ap.add_argument("--kv8", action="store_true")
    ap.add_argument("--logprobs", type=int, default=None)
    ap.add_argument("--new", type=int, default=256)
    a = ap.parse_args()
    cfg = full_cfg()
    lc = cfg.llama
    T, N = 160, a.new
    wb16 = bench.llama_param_bytes(lc, lambda n, k: 1 if a.fp8 else 2)
    # int4: QKV, gate/up and down_proj stream 4.125 bits per weight at 1-16 rows (the LoRA-A rows, o_proj and the lm_head their bf16 bytes); from 17 rows
    # every kernel reads the packed bf16 copy of the dequantised weight
    wb4 = wb16 - lc.layers * (3 * lc.hidden * lc.hidden + 3 * lc.hidden * lc.inter) * (2 - 4.125 / 8)
    print(f"| batch | family | step at ctx {T + 8} (ms) | mean step over {N} tokens (ms) | HBM frac (weights + KV) | prefill ms |")
    print("|---|---|---|---|---|---|")
    for B in [int(x) for x in a.batches.split(",")]:
        eng = RdxEngine(cfg, dtype=a.dtype, device=0, max_batch=B, max_len=(T + N + 64 + 31) // 32 * 32, lora=True, vision=False, weights_fp8=a.fp8, weights_w4=a.w4, kv_fp8=a.kv8)
        eng.load_weights(synth_getter(cfg, eng.device, lora=True), vision=False)
        ids = synth.synth_prompt_ids(B, T, vocab=lc.vocab, pad_rows=(B > 1), seed=7).to(eng.device)
        qf = synth.synth("t.qf_step", (B, 32, lc.qformer_dim), -1.0, 1.0).to(eng.device)
        for fam in ([1, 0] if (a.ab and 3 <= B <= 16) else [1]):
            eng.set_option("xs16", fam)
            eng.generate(ids, qf, max_new=8, eos_id=-1, pad_id=0, logprobs=a.logprobs)
            step = eng.time_unit(0, 20)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(3):
                eng.generate(ids, qf, max_new=1, eos_id=-1, pad_id=0, logprobs=a.logprobs)
            torch.cuda.synchronize()
            pre = (time.perf_counter() - t0) / 3
            eng.generate(ids, qf, max_new=N, eos_id=-1, pad_id=0, logprobs=a.logprobs)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(2):
                toks, _, n, *_lp = eng.generate(ids, qf, max_new=N, eos_id=-1, pad_id=0, logprobs=a.logprobs)
            torch.cuda.synchronize()
            avg = ((time.perf_counter() - t0) / 2 - pre) / (N - 1) * 1e3
            kv_pos = 524288 * ((1 + 1 / 128) / 2 if a.kv8 else 1)         # bytes of one cached position of one row: K and V, 32 layers x 4096 elements
            kv = B * (T + N / 2.0) * kv_pos + B * kv_pos
            wb = wb4 if (a.w4 and B <= 16 and (fam or B <= 2)) else wb16
            frac = (wb + kv) / (avg * 1e-3) / 1e9 / bench.HBM_PEAK_GBS
            name = ("" if a.logprobs is None else f"logprobs {a.logprobs}, ") + ("kv8, " if a.kv8 else "") + ("fp8 x fp8: " if a.fp8 else "int4: " if a.w4 else "") + ("xs16 (5 launches / layer)" if (fam and not a.fp8 and 3 <= B <= 16) else "generic (GEMV, 5 / layer)" if (B <= 2 and a.kv8) else "chained (3 / layer)" if B <= 2 else
                    "row blocks (33-128 rows, 7 / layer)" if B > 32 else "xstat32 (7 launches / layer)")
            print(f"| {B} | {name} | {step:.3f} | {avg:.3f} | {frac * 100:.1f} % | {pre * 1e3:.1f} |", flush=True)
        eng.close()


if __name__ == "__main__":
    main()
