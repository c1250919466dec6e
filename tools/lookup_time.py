#!/usr/bin/env python
"""Prompt-lookup decoding on the full-size synthetic bf16 engine, batch 1 (profiles/r20_lookup.md): python tools/lookup_time.py [N = 64]

(a) One verify pass by tail length. A corpus of blocks [S0[i], junk x d] (S0 = the plain greedy output, junk = an id the model never emits) makes EVERY
    forward a pass over d + 1 rows that accepts nothing: the call's time minus the time of the same call with max_new = 1 (the prefill), divided by the
    passes, is one pass -- layers, final norm, lm_head over d + 1 rows, lookup_accept_k, the 8-byte status copy and its sync. Forwards that found no draft
    (the pass's own token left S0) are counted and charged at the plain step's time; the last d forwards of a call run shorter tails (the budget
    max_new - emitted - 1 clips their draft) and are counted as passes, which flatters the 16-row figure by up to a quarter of its passes.
(b) ms per emitted token for corpus = S0, S0 corrupted at every 4th token, and no drafts at all (8-grams only, no corpus), against generate().
(c) The break-even accepted tokens per pass: pass / step - 1.
Every figure is the median of three legs, the legs of the compared configurations alternating."""
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    from radialog_amd import synth
    from radialog_amd.config import full_cfg
    from radialog_amd.engine import Lookup, RdxEngine, synth_getter
    N = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    cfg = full_cfg()
    eng = RdxEngine(cfg, dtype="bf16", device=0, max_batch=1, max_len=512, lora=True, vision=False)
    eng.load_weights(synth_getter(cfg, eng.device, lora=True), vision=False)
    qf = synth.synth("t.qf_step", (1, 32, cfg.llama.qformer_dim), -1.0, 1.0).to(eng.device)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        eng.sync()
        return (time.perf_counter() - t0) * 1e3, out

    def med(fns, legs=3):
        """fns: {name: callable}; the legs alternate between the configurations. Returns {name: (median ms, last output)}."""
        ts, outs = {k: [] for k in fns}, {}
        for k, f in fns.items():
            f()                                                        # warm: graphs, workspaces
        for _ in range(legs):
            for k, f in fns.items():
                t, outs[k] = timed(f)
                ts[k].append(t)
        return {k: (statistics.median(v), outs[k]) for k, v in ts.items()}

    print("# Prompt-lookup decoding: full-size synthetic bf16 engine, batch 1\n")
    junk = cfg.llama.vocab - 2
    step_ms = {}
    print("## (a) one verify pass by tail length\n")
    print("| context | tail rows | forwards (passes, of full length) | ms per pass | plain step ms | pass / step |")
    print("|---|---|---|---|---|---|")
    for T in (136, 376):
        M = 64
        ids = synth.synth_prompt_ids(1, T, vocab=cfg.llama.vocab, pad_rows=False, seed=7).to(eng.device)
        r = med({"gen": lambda: eng.generate(ids, qf, max_new=M, eos_id=-1), "gen1": lambda: eng.generate(ids, qf, max_new=1, eos_id=-1)})
        S0 = r["gen"][1][0][0, :M].cpu().tolist()
        step = (r["gen"][0] - r["gen1"][0]) / (M - 1)
        step_ms[T] = step
        for rows in (2, 4, 8, 16):
            d = rows - 1
            corpus = [t for s in S0 for t in [s] + [junk] * d]
            lk = Lookup(d, 1, 1)
            r = med({"run": lambda: eng.generate_lookup(ids, qf, max_new=M, eos_id=-1, lookup=lk, corpus=corpus),
                     "one": lambda: eng.generate_lookup(ids, qf, max_new=1, eos_id=-1, lookup=lk, corpus=corpus)})
            trace = r["run"][1][4].tolist()
            passes = [x for x in trace if x[0] > 0]
            full = [x for x in passes if x[0] == d]
            other = len(trace) - len(passes)
            ms = (r["run"][0] - r["one"][0] - other * step) / max(len(passes), 1)
            print(f"| ~{T + M // 2} | {rows} | {len(trace)} ({len(passes)}, {len(full)}) | {ms:.3f} | {step:.3f} | {ms / step:.2f} |")
    print("\n## (b) ms per emitted token\n")
    print("| context | draft_len | corpus | tokens | forwards | passes | accepted / drafted | ms per token | generate() ms per token |")
    print("|---|---|---|---|---|---|---|---|---|")
    for T in (160,):
        ids = synth.synth_prompt_ids(1, T, vocab=cfg.llama.vocab, pad_rows=False, seed=7).to(eng.device)
        g = med({"gen": lambda: eng.generate(ids, qf, max_new=N, eos_id=-1), "gen1": lambda: eng.generate(ids, qf, max_new=1, eos_id=-1)})
        S0 = g["gen"][1][0][0, :N].cpu().tolist()
        pre = g["gen1"][0]
        gen_tok = (g["gen"][0] - pre) / (N - 1)
        bad = [t if i % 4 else junk for i, t in enumerate(S0)]
        for dl in (3, 7, 15):
            legs = {"own output": (Lookup(dl, 3, 1), S0), "corrupted every 4th": (Lookup(dl, 3, 1), bad)}
            if dl == 7:
                legs["no drafts"] = (Lookup(dl, 8, 8), None)
            fns = {k: (lambda lk=lk, cp=cp: eng.generate_lookup(ids, qf, max_new=N, eos_id=-1, lookup=lk, corpus=cp)) for k, (lk, cp) in legs.items()}
            fns["one"] = lambda: eng.generate_lookup(ids, qf, max_new=1, eos_id=-1, lookup=Lookup(dl, 3, 1), corpus=S0)
            r = med(fns)
            for k in legs:
                ms, out = r[k]
                st = out[3]
                print(f"| ~{T + N // 2} | {dl} | {k} | {out[2]} | {st['forwards']} | {st['passes']} | {st['accepted']} / {st['drafted']} | "
                      f"{(ms - r['one'][0]) / max(out[2] - 1, 1):.3f} | {gen_tok:.3f} |")
    print("\n## (c) break-even\n")
    print("A pass of r rows costs what `pass / step` plain steps cost (table (a)) and emits 1 + accepted tokens: it pays from a mean of "
          "`pass / step - 1` accepted tokens per pass.")
    eng.close()


if __name__ == "__main__":
    main()
