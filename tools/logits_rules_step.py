#!/usr/bin/env python
"""What the logits rules cost per decode step (profiles/logits_rules_step.md): Vicuna-7B shapes, bf16, prompt 160 tokens, the captured step graph
replayed at context ~168 (rdx_time unit 0), batch 1 and 32 -- with the rules off (greedy_step_k: the default path) and with rules (1.2, 3, 0)
(select_step_k on the step's logits). Every figure is taken --runs times. A tree without logits rules (the parent commit) reports the
rules-off leg alone. python tools/logits_rules_step.py [--batches 1,32] [--runs 2] [--iters 20]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from radialog_amd import synth  # noqa: E402
from radialog_amd.config import full_cfg  # noqa: E402
from radialog_amd.engine import RdxEngine, synth_getter  # noqa: E402

RULES = (1.2, 3, 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,32")
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    cfg = full_cfg()
    T = 160
    has_rules = hasattr(RdxEngine, "set_logits_rules")
    print("| batch | rules | step at ctx 168 (ms), one figure per run |")
    print("|---|---|---|")
    for B in [int(x) for x in a.batches.split(",")]:
        eng = RdxEngine(cfg, dtype=a.dtype, device=0, max_batch=B, max_len=512, lora=True, vision=False)
        eng.load_weights(synth_getter(cfg, eng.device, lora=True), vision=False)
        ids = synth.synth_prompt_ids(B, T, vocab=cfg.llama.vocab, pad_rows=(B > 1), seed=7).to(eng.device)
        qf = synth.synth("t.qf_step", (B, 32, cfg.llama.qformer_dim), -1.0, 1.0).to(eng.device)
        for rules in ([None, RULES] if has_rules else [None]):
            ms = []
            for _ in range(a.runs):
                kw = {"logits_rules": rules} if has_rules else {}
                eng.generate(ids, qf, max_new=8, eos_id=-1, pad_id=0, **kw)          # the state the replays continue: context 160 + 8
                ms.append(eng.time_unit(0, a.iters))
            print(f"| {B} | {'off' if rules is None else rules} | {' / '.join(f'{m:.3f}' for m in ms)} |", flush=True)
        eng.close()


if __name__ == "__main__":
    main()
