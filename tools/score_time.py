#!/usr/bin/env python
"""What scoring given tokens costs (profiles/r11_score.md): Vicuna-7B shapes at full depth, random-init weights, bf16, a 160-token prompt followed by a
128-token report of which only the report is scored, batch 1 and 12. Three legs, alternated --runs times (A-B-C-A-B-C) on one engine per batch:
  score    RdxEngine.score() on prompt + report (one pass, the lm_head on the 128 B scored rows)
  prefill  the plain prefill of the same 288 tokens (what the layers cost; score - prefill = the tail)
  loop     what the same numbers cost without rdx_score: prefill of the prompt, then one decode_step(input_ids=...) per further report token with the
           logits row downloaded (127 steps: the prefill's own logits score the first token), then torch's log_softmax + gather on the rows
Every figure is host wall clock around work that ends in a device synchronise, in ms, the mean of --iters calls after one warm-up call.
Then, at batch 12 with every position scored, the sweep of the "score_chunk" option (0 = all rows at once).
python tools/score_time.py [--batches 1,12] [--runs 3] [--iters 3] [--chunks 128,512,2048,0]"""
import argparse
import dataclasses
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from radialog_amd import synth  # noqa: E402
from radialog_amd.config import full_cfg  # noqa: E402
from radialog_amd.engine import RdxEngine, synth_getter  # noqa: E402

T_PROMPT, N_REPORT = 160, 128


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,12")
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--chunks", default="128,512,2048,0")
    ap.add_argument("--layers", type=int, default=0, help="fewer layers than the full 32 (rehearsals)")
    a = ap.parse_args()
    cfg = full_cfg()
    if a.layers:
        cfg = dataclasses.replace(cfg, llama=dataclasses.replace(cfg.llama, layers=a.layers))
    V = cfg.llama.vocab
    T = T_PROMPT + N_REPORT
    print(f"layers {cfg.llama.layers}, {a.dtype}, prompt {T_PROMPT} + report {N_REPORT}; lm_head {2 * cfg.llama.hidden * V / 1e9:.3f} GFLOP per row")
    print("| batch | leg | ms per call, one figure per run |")
    print("|---|---|---|")
    for B in [int(x) for x in a.batches.split(",")]:
        eng = RdxEngine(cfg, dtype=a.dtype, device=0, max_batch=B, max_len=512, lora=True, vision=False)
        eng.load_weights(synth_getter(cfg, eng.device, lora=True), vision=False)
        prompt = synth.synth_prompt_ids(B, T_PROMPT, vocab=V, pad_rows=(B > 1), seed=7)
        g = torch.Generator().manual_seed(11)
        report = torch.randint(3, 31999, (B, N_REPORT), generator=g)
        full = torch.cat([prompt, report], dim=1)
        labels = torch.full_like(full, -100)
        labels[:, T_PROMPT:] = report
        qf = synth.synth("t.qf_score", (B, 32, cfg.llama.qformer_dim), -1.0, 1.0).to(eng.device)
        full_d, prompt_d, report_d = full.to(eng.device), prompt.to(eng.device), report.to(eng.device)
        out = {}

        def leg_score():
            out["score"] = eng.score(full_d, qf, labels)[0]

        def leg_prefill():
            eng.prefill(full_d, qf, max_new=1, eos_id=-1, want_logits=False)

        def leg_loop():
            rows = [eng.prefill(prompt_d, qf, max_new=N_REPORT + 1, eos_id=-1)[1]]
            for s in range(1, N_REPORT):
                rows.append(eng.decode_step(input_ids=report_d[:, s - 1])[1])
            lg = torch.stack(rows, dim=1).float()                                         # [B, N, V]
            out["loop"] = torch.log_softmax(lg, dim=-1).gather(-1, report_d.unsqueeze(-1)).squeeze(-1)
            torch.cuda.synchronize()

        legs = {"score": leg_score, "prefill": leg_prefill, "loop": leg_loop}
        ms = {k: [] for k in legs}
        for _ in range(a.runs):
            for name, fn in legs.items():
                ms[name].append(timed(fn, a.iters if name != "loop" else 1))
        for name in legs:
            print(f"| {B} | {name} | {' / '.join(f'{m:.2f}' for m in ms[name])} |", flush=True)
        diff = float((out["score"][:, T_PROMPT:] - out["loop"]).abs().max())
        spread = max(max(v) - min(v) for v in (ms["score"], ms["loop"]))
        gaps = [l - s for s, l in zip(ms["score"], ms["loop"])]
        tail = [s - p for s, p in zip(ms["score"], ms["prefill"])]
        print(f"| {B} | score - prefill (the tail; lm_head {B * N_REPORT * 2 * cfg.llama.hidden * V / 1e9:.1f} GFLOP) | {' / '.join(f'{m:.2f}' for m in tail)} |")
        print(f"| {B} | loop / score | {' / '.join(f'{l / s:.1f}x' for s, l in zip(ms['score'], ms['loop']))} |")
        print(f"batch {B}: loop - score per pair {[round(x, 2) for x in gaps]} ms, larger run-to-run spread {spread:.2f} ms, "
              f"faster in every pair by more than the spread: {min(gaps) > spread}; the two paths' logprobs differ by at most {diff:.4g}", flush=True)
        if B == max(int(x) for x in a.batches.split(",")) and a.chunks:
            all_labels = full.clone()
            all_labels[full == 0] = -100
            n_rows = int((all_labels[:, 1:] != -100).sum())
            chunks = [int(x) for x in a.chunks.split(",")]
            cms = {c: [] for c in chunks}
            for _ in range(a.runs):
                for c in chunks:
                    eng.set_option("score_chunk", c)
                    cms[c].append(timed(lambda: eng.score(full_d, qf, all_labels), a.iters))
            eng.set_option("score_chunk", 2048)
            print(f"| batch {B}, every position scored ({n_rows} rows) | score_chunk | ms per call, one figure per run |")
            print("|---|---|---|")
            for c in chunks:
                print(f"| {B} | {c if c else 'all'} | {' / '.join(f'{m:.2f}' for m in cms[c])} |", flush=True)
        eng.close()


if __name__ == "__main__":
    main()
