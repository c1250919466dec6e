#!/usr/bin/env python
"""What sampled decoding costs per decode step (profiles/sampling_step.md): Vicuna-7B shapes, bf16, prompt 160 tokens, the captured step graph
replayed at context ~168 (rdx_time unit 0), batch 1 and 32 -- greedy (greedy_step_k: the default path), rules (1.2, 0, 0) (select_step_k) and
sampling (0.8, 50, 0.95) (sample_step_k), the legs interleaved --runs times (A-B-C-A-B-C) on one engine. A tree without sampling (the parent
commit) reports the first two legs. python tools/sampling_step.py [--batches 1,32] [--runs 3] [--iters 20] [--legs greedy,rules,sampling]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from radialog_amd import synth  # noqa: E402
from radialog_amd.config import full_cfg  # noqa: E402
from radialog_amd.engine import RdxEngine, synth_getter  # noqa: E402

RULES = (1.2, 0, 0)
SAMPLING = (0.8, 50, 0.95, 12345)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,32")
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--legs", default="greedy,rules,sampling")
    a = ap.parse_args()
    cfg = full_cfg()
    T = 160
    has_sampling = hasattr(RdxEngine, "set_sampling")
    legs = {"greedy": {}, "rules": {"logits_rules": RULES}}
    if has_sampling:
        legs["sampling"] = {"sampling": SAMPLING}
    legs = {k: v for k, v in legs.items() if k in a.legs.split(",")}
    print("| batch | leg | step at ctx 168 (ms), one figure per run |")
    print("|---|---|---|")
    for B in [int(x) for x in a.batches.split(",")]:
        eng = RdxEngine(cfg, dtype=a.dtype, device=0, max_batch=B, max_len=512, lora=True, vision=False)
        eng.load_weights(synth_getter(cfg, eng.device, lora=True), vision=False)
        ids = synth.synth_prompt_ids(B, T, vocab=cfg.llama.vocab, pad_rows=(B > 1), seed=7).to(eng.device)
        qf = synth.synth("t.qf_step", (B, 32, cfg.llama.qformer_dim), -1.0, 1.0).to(eng.device)
        ms = {k: [] for k in legs}
        for _ in range(a.runs):
            for name, kw in legs.items():
                eng.generate(ids, qf, max_new=8, eos_id=-1, pad_id=0, **kw)          # the state the replays continue: context 160 + 8
                ms[name].append(eng.time_unit(0, a.iters))
        for name in legs:
            print(f"| {B} | {name} | {' / '.join(f'{m:.3f}' for m in ms[name])} |", flush=True)
        eng.close()


if __name__ == "__main__":
    main()
