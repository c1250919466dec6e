#!/usr/bin/env python
"""Continuous batching against chunked batches (profiles/r15_queue.md): one MI355X, Vicuna-7B shapes, synthetic weights, bf16, 96 requests of T = 160 with
the image splice, eos_id = -1, per-request caps from a fixed seeded list spread over 40-300.
  A  the existing way: generate() in chunks of `rows` requests, each with max_new = the chunk's largest cap
  B  generate_queue() with the same `rows`, stage = 4, min_refill 1 / 2 / 4
at rows = 12 and 32, A and the three Bs interleaved three times (median reported); one more pass of every B with a drained, timed refill gives the time
spent in refills. python tools/queue_time.py [out.md]"""
import os
import random
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N_REQ, T, STAGE, SEED = 96, 160, 4, 15
_rng = random.Random(SEED)
CAPS = [_rng.randint(40, 300) for _ in range(N_REQ)]


class TimedRefills:
    """A row session whose refills are drained and timed (the other four methods pass through)."""

    def __init__(self, ses, eng):
        self._s, self._e, self.ms = ses, eng, 0.0

    def __getattr__(self, name):
        return getattr(self._s, name)

    def refill(self, *a, **k):
        self._e.sync()
        t0 = time.perf_counter()
        self._s.refill(*a, **k)
        self._e.sync()
        self.ms += (time.perf_counter() - t0) * 1e3


def main(out_path=None):
    from radialog_amd import synth
    from radialog_amd.config import full_cfg
    from radialog_amd.engine import RdxEngine, synth_getter
    from radialog_amd.rowqueue import RowScheduler, chunked_steps
    cfg = full_cfg()
    cap = max(CAPS)
    eng = RdxEngine(cfg, dtype="bf16", device=0, max_batch=32 + STAGE, max_len=(T + cap + 31) // 32 * 32, lora=True, vision=False)
    eng.load_weights(synth_getter(cfg, eng.device, lora=True), vision=False)
    ids = synth.synth_prompt_ids(N_REQ, T, vocab=cfg.llama.vocab, pad_rows=False, seed=7)
    qf = synth.synth("t.qf_queue", (N_REQ, 32, cfg.llama.qformer_dim), -1.0, 1.0)
    reqs = [(ids[i], qf[i], CAPS[i]) for i in range(N_REQ)]
    ids_d, qf_d = ids.to(eng.device), qf.to(eng.device)

    def run_a(rows):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for s in range(0, N_REQ, rows):
            eng.generate(ids_d[s:s + rows], qf_d[s:s + rows], max_new=max(CAPS[s:s + rows]), eos_id=-1, pad_id=0)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def run_b(rows, min_refill, timed=False):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with eng.row_session(rows, STAGE, cap, eos_id=-1, pad_id=0) as ses:
            s = TimedRefills(ses, eng) if timed else ses
            sch = RowScheduler(s, rows, STAGE, poll=4, min_refill=min_refill)
            out = sch.run(reqs)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        assert [len(o) for o in out] == CAPS
        return ms, sch, (s.ms if timed else None)

    lines = [f"96 requests, T = {T}, bf16, Vicuna-7B shapes, synthetic weights, eos_id = -1, stage = {STAGE}, poll = 4; sum(caps) = {sum(CAPS)}.",
             "", f"caps (random.Random({SEED}).randint(40, 300), 96 draws): {CAPS}", "",
             "| rows | schedule | ms / request (median of 3) | runs (ms / request) | decode steps | refill groups | ms in refills |", "|---|---|---|---|---|---|---|"]
    for rows in (12, 32):
        print(f"rows = {rows} ...", file=sys.stderr, flush=True)
        run_a(rows)
        run_b(rows, 1)                      # warm-up: workspaces, the step graphs of both keys
        a, b = [], {m: [] for m in (1, 2, 4)}
        info = {}
        for _ in range(3):
            a.append(run_a(rows) / N_REQ)
            for m in b:
                ms, sch, _ = run_b(rows, m)
                b[m].append(ms / N_REQ)
                info[m] = sch
        fmt = lambda v: ", ".join(f"{x:.1f}" for x in v)       # noqa: E731
        lines.append(f"| {rows} | A: chunks of {rows} | {statistics.median(a):.1f} | {fmt(a)} | {chunked_steps(CAPS, rows)} | {-(-N_REQ // rows)} prefills of {rows} | - |")
        for m in b:
            _, _, rms = run_b(rows, m, timed=True)
            sch = info[m]
            lines.append(f"| {rows} | B: queue, min_refill {m} | {statistics.median(b[m]):.1f} | {fmt(b[m])} | {sch.n_steps} | {sch.n_refills} | {rms:.0f} |")
    text = "\n".join(lines)
    print(text)
    if out_path:
        with open(out_path, "w") as f:
            f.write(text + "\n")
    eng.close()


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
