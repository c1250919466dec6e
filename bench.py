#!/usr/bin/env python
"""bench.py -- RaDialog hot-path benchmark on MI355X (contract: see the task statement / DESIGN.md "Measurement").

A "step" is one pass of the hot path over one batch of synthetic input on each rank:
    BioViL-T encode (448x448 synthetic CXR) -> Q-Former -> img_proj + <IMG> splice -> Vicuna-7B prefill (160-token
    prompt with 32 <IMG> slots) -> 256 greedy tokens (eos disabled so every report is exactly 256 tokens).
Default workload = BASELINE.json configs[1]: 1 x MI355X, batch 1, bf16, random-init weights of the real architecture.
`--batch 32` gives configs[2] (batch-32 decode, hipGraph step). With N > 1 ranks (one process per GPU, launched by
torch.distributed.run) every rank runs the same per-GPU batch on its own shard of images (weak scaling) and the
generated token ids are gathered with ONE RCCL all-gather issued by librdx itself (rdx_allgather_tokens) at the end of each
step -- the only collective on the path; torch.distributed (a gloo group on the host) carries the 128-byte RCCL id, the barrier and
the max-over-ranks clock.

`python bench.py --gpus N` without a launcher (no RANK / WORLD_SIZE in the environment) starts the N ranks itself: it runs
`python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1` as a child (one process per GPU, LOCAL_RANK -> device)
and exits with its status; it fails loudly when fewer than N GPUs are visible. Launched by torch.distributed.run directly (the driver's form) it reads
RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* from the environment; WORLD_SIZE must equal --gpus.

A plain run (`--gpus N --steps K --warmup W`) does only what the headline needs: set up, W warm-up steps, K timed steps, the outputs of the
last timed step if `--dump-outputs DIR` is given (DIR/tokens.npy: the gathered greedy token ids, DIR/qformer_out.npy: rank 0's Q-Former output,
both float32), and ONE JSON line with the contract's fields. `value` = reports/s of the whole job with inputs resident in HBM, `ms_per_step` = the
milliseconds one timed step took (the max over ranks).

`--full` adds everything else below. Rank 0 then prints ONE JSON line of < 4 KB (round 6: compact_line() -- the contract's fields, `roofline` /
`cpu_baseline` with scalars only, every sub-run as `<key>_value` / `_decode_ms` / `_frac` scalars, every parity leg as {ok, same, n, worst, bar}) and
writes the full record described below to bench_detail.json beside this script (RDX_BENCH_DETAIL overrides the path). The full record:
  roofline     bound "hbm": the kernel rocprofv3 ranks first in the decode loop -- at batch <= 2 the chained down(l) -> QKV(l+1)
               launch `decode_chain_k` (profiles/r03_bench_b1_kernel_stats.md), at batch 3-32 the gate/up SwiGLU `xstat32_k`:
               algorithmic bytes per launch / its average launch duration measured live with HIP events on the library's stream
               (rdx_time; the chained launch is bracketed in situ inside real decode steps); `traffic` = HBM bytes per launch
               from the rocprofv3 PMC passes of this same command (profiles/r04_pmc.json; counters cannot be read in-process).
               Also the whole-step fractions and the MFMA-side fractions north_star targets (`mfma`: encode and prefill
               TFLOP/s over the 2.5 PFLOP/s dense bf16 peak).
  b32          (batch-1 runs) BASELINE configs[2] / [3] timed in the same process at every world size: per-GPU batch 32, hipGraph step.
  fp8_b32      (batch-1 runs) BASELINE configs[4]: e4m3 decoder weights AND activations on the fp8 MFMA, per-GPU batch 32.
  b64 / b128 / fp8_b128   (batch-1 runs, one rank) 64 and 128 reports per GPU on the row-block decode family (33-128 rows), the last with fp8 weights.
  token_check  the first 8 greedy tokens of row 0 of every timed configuration against tests/golden/bench_tokens.json (exit 3 on a miss).
  cpu_baseline the CPU oracle (oracle/ref_cpu.py, kind "port") running BASELINE configs[0] for real on the host cores: one
               448 px image through the full-size encoder, the 160-token prefill and 32 greedy tokens through all 32 layers.
"""
import argparse
import json
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

HBM_PEAK_GBS = 8000.0        # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec (6.29 TB/s measured float4 copy)
MFMA_PEAK_TFLOPS = 2500.0    # dense bf16 / fp16 MFMA peak (the 5 PFLOP/s headline includes 2:1 sparsity)
MFMA_FP8_PEAK_TFLOPS = 5000.0    # dense fp8 MFMA peak (MX-scaled K = 128 instruction; MI355X_MICROARCH.md) -- what the fp8 prefill is priced against


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=None, help="ranks (one per GPU); default: the launcher's WORLD_SIZE, or 1 without a launcher")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batch", type=int, default=1, help="reports per GPU per step (1 = configs[1], 32 = configs[2])")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f16"])
    ap.add_argument("--new-tokens", type=int, default=256)
    ap.add_argument("--prompt-len", type=int, default=160)
    ap.add_argument("--fp8", action="store_true", help="decoder GEMM weights in e4m3 + per-row scale (BASELINE configs[4] weight path); "
                    "not the parity configuration: its oracle is the reference math on the fake-quantised weights")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-b32", action="store_true", help="skip the configs[2] (batch 32) sub-run of a batch-1 single-GPU bench")
    ap.add_argument("--no-fp8", action="store_true", help="skip the configs[4] (fp8 weights, batch 32) sub-run of a batch-1 bench")
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--no-b64", action="store_true", help="skip the 64-reports-per-GPU sub-run of a batch-1 bench")
    ap.add_argument("--no-f16", action="store_true", help="skip the fp16 (the reference's dtype) timed run of a batch-1 bf16 bench (value_f16)")
    ap.add_argument("--no-enc256", action="store_true", help="skip the batch-256 image-encode timing (enc_b256)")
    ap.add_argument("--full", action="store_true", help="also the per-phase / roofline detail, the sub-runs, the token fixture check, the CPU oracle "
                    "baseline and its parity legs, and bench_detail.json (the --no-* options select among these)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write the last timed step's outputs to DIR/<name>.npy (float32)")
    args = ap.parse_args(argv)
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    return args


# ----------------------------------------------------------------------------------------------------------------------
# algorithmic work, from the shapes
# ----------------------------------------------------------------------------------------------------------------------
def encode_flops(cfg):
    """FLOPs (2 x MAC) of one image through ResNet-50 trunk, backbone_to_vit, projector, Q-Former query path."""
    v, q = cfg.vision, cfg.qformer
    s = v.img // 2
    mac = s * s * v.stem * 3 * 49
    s, cin = v.img // 4, v.stem
    for li, (pl, nb) in enumerate(zip(v.planes, v.blocks)):
        for b in range(nb):
            so = (s - 1) // 2 + 1 if (b == 0 and li > 0) else s
            mac += s * s * pl * cin + so * so * pl * pl * 9 + so * so * 4 * pl * pl
            if b == 0:
                mac += so * so * 4 * pl * cin
            cin, s = 4 * pl, so
    P = s * s
    mac += P * v.b2v * cin + P * v.proj * 2 * v.b2v + P * v.proj * v.proj
    H, I, NQ = q.hidden, q.inter, q.n_query
    for l in range(q.layers):
        mac += NQ * 4 * H * H + 2 * NQ * NQ * H + 2 * NQ * H * I
        if q.has_cross(l):
            mac += 2 * NQ * H * H + 2 * P * H * q.enc_width + 2 * NQ * P * H
    return 2.0 * mac


def llama_param_bytes(lc, wbytes):
    """bytes of one decode step's weight stream: every GEMM weight once (+ LoRA-A rows fused into QKV), norms, LoRA-B."""
    H, I = lc.hidden, lc.inter
    per_layer = ((3 * H + 2 * lc.lora_r) * H * wbytes(3 * H + 2 * lc.lora_r, H) + H * H * wbytes(H, H) + 2 * I * H * wbytes(2 * I, H)
                 + H * I * wbytes(H, I) + 2 * H * 2 + 2 * H * lc.lora_r * 2)
    return lc.layers * per_layer + lc.vocab * H * wbytes(lc.vocab, H) + H * 2


def prefill_flops(lc, T, B):
    H, I = lc.hidden, lc.inter
    per_tok = 2.0 * lc.layers * ((3 * H + 2 * lc.lora_r) * H + H * H + 3 * H * I)
    attn = lc.layers * 4.0 * T * T * H / 2
    return B * (per_tok * T + attn + 2.0 * lc.vocab * H + 2.0 * 32 * lc.qformer_dim * H)


PMC_FILES = ("r06_pmc.json", "r05_pmc.json", "r04_pmc.json", "r03_pmc.json")


def pmc_traffic(kernel_key):
    """HBM bytes per launch of the dominant kernel from the rocprofv3 PMC passes (FETCH_SIZE / WRITE_SIZE in separate runs of
    this command, FETCH doubled per the gfx950 correction; profiles/rNN_pmc_hbm_traffic.md, machine-readable twin rNN_pmc.json written by
    tools/pmc_to_json.py; newest round first). Only for configurations that were profiled -> null otherwise. The figure is a REPLAY of a
    committed profile, not a measurement of this run (counters cannot be read in-process): pmc_source() says which file and whether the
    kernel sources it was taken on are the ones running now."""
    for name in PMC_FILES:
        try:
            with open(os.path.join(REPO, "profiles", name)) as f:
                v = json.load(f).get(kernel_key, {}).get("traffic_bytes")
            if v is not None:
                return v
        except Exception:
            continue
    return None


def pmc_source(kernel_key):
    """{"file", "tree", "tree_now", "stale"} of the PMC file pmc_traffic(kernel_key) read: `tree` = radialog_amd.build.source_hash() of the
    kernel sources the profile was taken on (stamped by tools/pmc_to_json.py from round 5; absent in older files -> stale = null)."""
    from radialog_amd import build as _b
    now = _b.source_hash()
    for name in PMC_FILES:
        try:
            with open(os.path.join(REPO, "profiles", name)) as f:
                d = json.load(f)
            if d.get(kernel_key, {}).get("traffic_bytes") is not None:
                tree = d.get("_tree")
                # `algorithmic_bytes`: the algorithmic bytes per launch AT THE STATE THE PROFILE WAS TAKEN IN (e.g. the decode attention's
                # context), so that traffic / algorithmic is meaningful even when this run prices the kernel at another context
                return {"file": f"profiles/{name}", "tree": tree, "tree_now": now, "stale": None if tree is None else tree != now,
                        "algorithmic_bytes": d[kernel_key].get("algorithmic_bytes"), "note": d[kernel_key].get("note")}
        except Exception:
            continue
    return None


def _pick_threads():
    """torch's intra-op pool at os.cpu_count() threads can be far slower than a smaller pool on many-core hosts
    (sync overhead on decode-sized ops); calibrate on a decode-shaped matmul and use the fastest setting."""
    ncpu = os.cpu_count() or 1
    cands = sorted({c for c in (8, 16, 32, 64, 128, ncpu) if c <= ncpu})
    w = torch.randn(4096, 4096).to(torch.bfloat16)
    x = torch.randn(1, 4096).to(torch.bfloat16)
    best, best_t = cands[0], float("inf")
    for c in cands:
        torch.set_num_threads(c)
        torch.nn.functional.linear(x, w)
        t0 = time.time()
        for _ in range(3):
            torch.nn.functional.linear(x, w)
        t = time.time() - t0
        if t < best_t:
            best, best_t = c, t
    torch.set_num_threads(best)
    return best


def _oracle_decode(orc, ref_cpu, ids, q, n_tok):
    """Prefill + n_tok greedy tokens on the CPU oracle -> (tokens, per-step fp32 logit rows, s_prefill, s_per_token)."""
    km = ids.ne(0).long()
    t0 = time.time()
    logits, past, _ = orc.forward(orc.embed(ids, q), km, ref_cpu.positions_from_mask(km))
    t_prefill = time.time() - t0
    E = orc.W["model.embed_tokens.weight"]
    toks, rows, t0 = [], [], time.time()
    for s in range(n_tok):
        rows.append(logits[0, -1].float().clone())
        nxt = logits[:, -1].argmax(-1)
        toks.append(int(nxt))
        if s == n_tok - 1:
            break
        km = torch.cat([km, km.new_ones(1, 1)], -1)
        logits, past, _ = orc.forward(torch.nn.functional.embedding(nxt[:, None], E), km, ref_cpu.positions_from_mask(km)[:, -1:], past)
    return toks, rows, t_prefill, (time.time() - t0) / max(n_tok - 1, 1)


def cpu_baseline(cfg, dtype_name, prompt_len, new_tokens, device, hip_tf=None, b32_tf=None, fp8_tf=None, e2e_tf=None):
    """BASELINE configs[0], for real: the CPU oracle encodes ONE 448 px image, prefills the 160-token prompt and decodes 32 greedy
    tokens through all 32 production-width layers on the host cores (the weights are the engine's: generated on the GPU tensor by
    tensor, rounded to the model dtype, copied to the host -- not part of the timed work). The metric is quoted on 256-token
    reports: reports/s = 1 / (encode + prefill + 256 x the measured per-token time).

    `hip_tf(dtype, oracle_tokens, oracle_q) -> (argmax tokens int[32], logits [32, V], encoder rel-L2)` runs the ENGINE on the same image
    and prompt (rank 0, row 0, outside the timed region), teacher-forced with the oracle's tokens (rdx_decode_step_ids), so the oracle is
    also the CHECKER of what was just timed, at full depth, all 32 steps compared. Round 4: with an absolute logit bar per dtype
    (oracle_check) and in BOTH dtypes -- `parity` = the benchmarked dtype on the timed engine, `parity_f16` = the reference's dtype (fp16,
    where north_star states its 1e-2 tolerance) on a second engine; the fp16 oracle pass is not part of the timed CPU sample. The two halves
    are checked separately so that the decoder's bar applies to IDENTICAL inputs, as in tests/test_gpu_fullsize.py: the decoder is fed the
    oracle's own fp32 Q-Former output, and the engine's encoder output is compared with it by relative L2 (`encoder_rel_l2`, bar 5e-3 fp16 /
    3e-2 bf16 = tests' ENC_TOL) -- end to end the encoder's rounding noise enters through 32 spliced rows and moves full-depth logits by up to
    0.1 (fp16) / 0.95 (bf16), which says nothing about either half."""
    from oracle import ref_cpu
    from radialog_amd import synth
    threads = _pick_threads()
    DT = {"bf16": torch.bfloat16, "f16": torch.float16}
    n_tok = 32
    t_all = time.time()
    with torch.no_grad():
        Wv = synth.make_weights({**synth.vision_specs(cfg.vision), **synth.qformer_specs(cfg.qformer)})
        img = synth.synth_images(1, cfg.vision.img)
        ref_cpu.forward_image(img, Wv, cfg)                                           # cold pass: pages the conv kernels in
        t0 = time.time(); q, _ = ref_cpu.forward_image(img, Wv, cfg); t_enc = time.time() - t0
        del Wv
        specs = synth.llama_specs(cfg.llama, lora=True)
        ids = synth.synth_prompt_ids(1, prompt_len, vocab=cfg.llama.vocab)

        def oracle_for(dn, fp8=False):
            W = {name: gen(name, shape, device).to(DT[dn]).cpu() for name, (shape, gen) in specs.items()}
            o = ref_cpu.LlamaOracle(W, cfg.llama, DT[dn], lora=True)
            if fp8:
                # LlamaOracle(fp8=True) with the e4m3 values taken from the fp32 SOURCE tensors like the engine's pack_weight_fp8_k does (not from
                # their model-dtype rounding), one tensor at a time; force_a8: one row of a batch >= 3 run restated at batch 1
                for name, (shape, gen) in specs.items():
                    if name == "lm_head.weight" or (name.startswith("model.layers.") and len(shape) == 2 and
                                                    (name.endswith("_proj.weight") or name.endswith("lora_A.weight"))):
                        o.W8[name] = ref_cpu.fake_quant_e4m3(gen(name, shape, device).float().cpu())
                o.fp8, o.force_a8 = True, True
            return o

        orc = oracle_for(dtype_name)
        toks, rows, t_prefill, t_tok = _oracle_decode(orc, ref_cpu, ids, q, n_tok)
        del orc
        t_sample = time.time() - t_all
    t_cfg0 = t_enc + t_prefill + (n_tok - 1) * t_tok
    t_report = t_enc + t_prefill + new_tokens * t_tok
    res = {
        "value": 1.0 / t_report, "unit": "reports/s", "cores": threads, "host_cpus": os.cpu_count(), "kind": "port",
        "sample": (f"oracle/ref_cpu.py, BASELINE configs[0] run in full on {threads} torch threads (fastest of a calibration sweep; host "
                   f"has {os.cpu_count()} cpus): 1 image 448 px full-size encode {t_enc:.2f} s + prefill T={prompt_len} through all "
                   f"{cfg.llama.layers} layers ({dtype_name}) {t_prefill:.2f} s + {n_tok} greedy tokens at {t_tok*1e3:.0f} ms/token = "
                   f"{t_cfg0:.1f} s of CPU work; value = 1 / (encode + prefill + {new_tokens} x per-token) = 1 / {t_report:.1f} s; "
                   f"wall incl. weight generation {t_sample:.0f} s"),
        "s_per_token": t_tok, "s_encode": t_enc, "s_prefill": t_prefill, "config0_s": t_cfg0, "tokens": toks[:8],
    }
    if hip_tf is not None:
        enc_bar = {"f16": 5e-3, "bf16": 3e-2}
        ht, hl, erel = hip_tf(dtype_name, toks, q)
        res["parity"] = oracle_check(ht, hl, toks, rows, dtype_name, teacher_forced=True)
        res["parity"].update(encoder_rel_l2=erel, encoder_bar=enc_bar[dtype_name])
        res["parity"]["ok"] = res["parity"]["ok"] and erel < enc_bar[dtype_name]
        other = "f16" if dtype_name != "f16" else None
        if other:
            with torch.no_grad():
                orc = oracle_for(other)
                toks2, rows2, _, _ = _oracle_decode(orc, ref_cpu, ids, q, n_tok)
                del orc
            ht, hl, erel = hip_tf(other, toks2, q)
            res["parity_" + other] = oracle_check(ht, hl, toks2, rows2, other, teacher_forced=True)
            res["parity_" + other].update(encoder_rel_l2=erel, encoder_bar=enc_bar[other])
            res["parity_" + other]["ok"] = res["parity_" + other]["ok"] and erel < enc_bar[other]
            if e2e_tf is not None:
                # ONE end-to-end leg: the engine's OWN Q-Former output into its decoder (nothing handed over by the oracle), in the
                # dtype whose noise floor leaves room for a bar -- fp16: the encoder's rounding noise moves full-depth logits by ~0.1,
                # a splice / plumbing error between the halves moves them by O(1). Bar 0.25 on every step + 90 % argmax identity.
                ht, hl = e2e_tf(other, toks2)
                e = oracle_check(ht, hl, toks2, rows2, other, teacher_forced=True, bar=0.25)
                e["checked"] = "END TO END: engine encoder -> engine decoder (its own Q-Former output), teacher-forced, vs the oracle's image -> tokens"
                e["ok"] = e["ok"] and e["tokens_identical"] >= 0.9 * e["tokens_compared"]
                res["parity_e2e_" + other] = e
        if b32_tf is not None:
            # BASELINE configs[2]/[3] per-GPU load: row 0 of a batch-32 prefill + decode (xstat32_k / xsplit32_k / throughput attention / flash
            # prefill) against the same oracle rows
            ht, hl = b32_tf(toks)
            res["parity_b32"] = oracle_check(ht, hl, toks, rows, dtype_name, teacher_forced=True)
            res["parity_b32"]["checked"] = "row 0 of a batch-32 run (31 other prompts, ragged padding), full depth, teacher-forced with the oracle's tokens"
        if fp8_tf is not None:
            # BASELINE configs[4], row 0 of the fp8 engine's batch-32 run (fp8 x fp8 prefill and decode kernels):
            # (a) against the UN-QUANTISED oracle of the model dtype -- what a user of configs[4] gives up (reported, no bar: no reference fp8 exists);
            ht, hl = fp8_tf(toks)
            errs = [float((hl[s_].float() - rows[s_]).abs().max()) for s_ in range(len(toks))]
            same = sum(int(a) == int(b) for a, b in zip(ht, toks))
            top2 = [rows[s_].topk(2).values for s_ in range(len(toks))]
            res["fp8_vs_unquantised"] = {
                "checked": f"fp8 engine (e4m3 weights + activations, LoRA-A rows e4m3 too), row 0 of batch 32, teacher-forced with the {dtype_name} "
                           f"oracle's tokens, against the UN-quantised {dtype_name} oracle's logits, full depth",
                "tokens_identical": same, "tokens_compared": len(toks), "worst_logit_err": max(errs), "median_logit_err": sorted(errs)[len(errs) // 2],
                "median_oracle_margin": sorted(float(t[0] - t[1]) for t in top2)[len(top2) // 2]}
            # (b) against its own definition, the fake-quantised oracle (the fp8 line had no independent check): 16 steps, bar
            # FP8_ABS_BAR = tests/test_gpu_parity.py's one-layer FP8_TOL x sqrt(32 layers) (e4m3 code flips bound the logits, and add up layer by layer)
            with torch.no_grad():
                orc8 = oracle_for(dtype_name, fp8=True)
                toks8, rows8, _, _ = _oracle_decode(orc8, ref_cpu, ids, q, 16)
                del orc8
            ht8, hl8 = fp8_tf(toks8)
            res["parity_fp8"] = oracle_check(ht8, hl8, toks8, rows8, dtype_name, teacher_forced=True, bar=FP8_ABS_BAR)
            res["parity_fp8"]["checked"] = ("fp8 engine, row 0 of batch 32, full depth, teacher-forced, against LlamaOracle(fp8=True) -- the reference math on "
                                            "the same fake-quantised operands (the leg's own definition: no reference fp8 exists)")
    return res


# Absolute logit bars of the full-depth parity legs (tests/test_gpu_fullsize.py): the one-layer tolerance x sqrt(32 layers) -- 1e-2 -> 6e-2
# in fp16 (north_star's dtype and tolerance), 8e-2 -> 0.45 in bf16 (8 x the ulp). 99 % of the steps must be inside, all inside 1.5 x.
PARITY_ABS_BAR = {"f16": 6e-2, "bf16": 0.45}
# fp8 engine against the fake-quantised oracle: an activation one model-dtype ulp apart on the two sides can land on the next e4m3 code (2^-3 of
# its magnitude away), so the one-layer bar is 0.5 whatever the dtype (tests/test_gpu_parity.py FP8_TOL; measured 0.17-0.45) and the same sqrt(32)
# over the full depth: 2.83 (first driver-style run of round 5: worst 1.59 over 16 steps; a wrong scale, group boundary or layout gives O(10))
FP8_ABS_BAR = 0.5 * 32 ** 0.5


def oracle_check(hip_tokens, hip_logits, ref_tokens, ref_logits, dtype="bf16", teacher_forced=False, bar=None):
    """The engine's tokens / logits of the benchmarked configuration against the oracle's, step by step (tests/_parity.py's rules).
    `ok` needs BOTH (round 4): every compared step's worst logit difference under 1.5 x the absolute bar of the dtype (the number of
    steps over the bar itself is reported: the tests demand 99 % under it over 64 steps), and every differing argmax at an oracle top-2 margin <= 2 x the measured error of that step. Free-running
    (teacher_forced=False) the comparison ends at the first differing token -- later inputs differ; teacher-forced (the engine was fed
    the oracle's tokens through rdx_decode_step_ids) every step is compared."""
    n = min(len(ref_tokens), len(hip_tokens))
    bar = PARITY_ABS_BAR[dtype] if bar is None else bar
    same, worst, note, ok, over, compared = 0, 0.0, None, True, 0, 0
    for s in range(n):
        err = float((hip_logits[s].float().cpu() - ref_logits[s]).abs().max())
        worst = max(worst, err)
        compared += 1
        over += int(err >= bar)
        if err >= 1.5 * bar:
            ok = False
            note = note or f"step {s}: logit error {err:.4g} exceeds 1.5 x the absolute bar {bar} of {dtype}"
        if int(hip_tokens[s]) != int(ref_tokens[s]):
            top2 = ref_logits[s].topk(2).values
            margin = float(top2[0] - top2[1])
            flip_ok = margin <= 2.0 * err + 1e-7
            ok = ok and flip_ok
            msg = (f"step {s}: engine token {int(hip_tokens[s])} vs oracle {int(ref_tokens[s])}, oracle top-2 margin {margin:.4g}, logit error "
                   f"{err:.4g} -> " + ("a near-tie the rounding-order noise can flip" + ("" if teacher_forced else "; later steps have different inputs and are not compared")
                                        if flip_ok else "NOT explained by the logit error: MISMATCH"))
            note = msg if note is None or not flip_ok else note
            if not teacher_forced:
                break
            continue
        same += 1
    # the tests' rule (tests/_parity.py): 99 % of the compared steps under the bar itself -- over 32 steps that is "at most one over"
    # (short comparisons -- unit tests, a free-running leg cut at its first flip -- carry only the 1.5 x rule)
    allowed_over = max(1, compared // 100) if compared >= 16 else compared
    if over > allowed_over:
        ok = False
        note = note or f"{over} of {compared} steps over the absolute bar {bar} of {dtype} (at most {allowed_over} allowed)"
    return {"checked": "image -> tokens, full depth, rank 0 row 0 (outside the timed region)" + (", teacher-forced with the oracle's tokens" if teacher_forced else ""),
            "dtype": dtype, "abs_bar": bar, "tokens_identical": same, "tokens_compared": compared, "steps_over_bar": over,
            "steps_over_bar_allowed": allowed_over, "worst_logit_err": worst, "divergence": note, "ok": ok}


# ----------------------------------------------------------------------------------------------------------------------
STUB = os.environ.get("RDX_BENCH_STUB") == "1"


def _sync():
    if not STUB:
        torch.cuda.synchronize()


class _StubEngine:
    """RDX_BENCH_STUB=1 (tests/test_bench_multirank.py only): main()'s multi-rank control flow on a box without GPUs -- sleeps instead of kernels,
    token ids that name (rank, row), and the 'communicator is up' branch of shard.allgather_tokens carried by the launcher's gloo group where
    the real engine calls ncclAllGather. Never measured, never shipped: the line it produces says `"data": "STUB ..."`."""
    def __init__(self, cfg, dtype="bf16", device=0, max_batch=1, max_len=512, lora=True, weights_fp8=False, **_):
        self.cfg, self.device, self.max_batch, self._world, self._rank = cfg, torch.device("cpu"), max_batch, 0, 0

    def load_weights(self, get, **_):
        pass

    def encode_image(self, image, want_image_embeds=True, **_):
        time.sleep(0.001)
        return torch.zeros(image.shape[0], self.cfg.qformer.n_query, self.cfg.qformer.hidden), None

    def generate(self, ids, q, max_new, **_):
        time.sleep(0.002 * (1 + self._rank))                   # rank r is the slower one: the clock must be the MAX over ranks
        B = ids.shape[0]
        toks = (torch.arange(B, dtype=torch.int32)[:, None] + 1000 * self._rank).expand(B, max_new).contiguous()
        return toks, None, max_new

    def comm_unique_id(self):
        return bytes(128)

    def comm_init(self, uid, rank, world):
        self._rank, self._world = rank, world

    @property
    def comm_world(self):
        return 0 if getattr(self, "comm_off", False) else self._world

    def allgather_tokens(self, tokens):
        import torch.distributed as dist
        out = torch.empty(self._world * tokens.shape[0], tokens.shape[1], dtype=tokens.dtype)
        if self._world > 1:
            dist.all_gather_into_tensor(out, tokens.contiguous())
        else:
            out.copy_(tokens)
        return out

    def time_unit(self, what, iters):
        return {0: 3.9, 1: 0.031, 6: 0.032, 7: 0.0376}.get(what, 0.01)

    def close(self):
        pass


def measure_detail(eng, cfg, args, B, T, N, img, ids, out_q, elapsed_per_step_ms, use_graph):
    """Per-phase numbers behind the headline (rank 0 only): encoder ms/img, prefill ms, mean decode step, the dominant kernel's
    live HIP-event duration and the roofline fractions."""
    lc = cfg.llama
    _sync()
    t1 = time.perf_counter()
    for _ in range(5):
        eng.encode_image(img, want_image_embeds=False)
    enc_ms = (time.perf_counter() - t1) / 5 / B * 1e3

    def wbytes(n_rows, k):        # bytes per streamed weight element of a decode projection: the fp8 engine holds (and streams) e4m3 only
        return 1 if args.fp8 else 2

    _sync()
    t2 = time.perf_counter()
    for _ in range(3):
        eng.generate(ids, out_q, max_new=1, eos_id=-1, pad_id=0, use_graph=use_graph)
    _sync()
    prefill_ms = (time.perf_counter() - t2) / 3 * 1e3
    avg_step_ms = (elapsed_per_step_ms - enc_ms * B - prefill_ms) / max(N - 1, 1)
    H_, I_ = lc.hidden, lc.inter
    step_bytes = llama_param_bytes(lc, wbytes)
    kv_bytes = B * (T + N / 2.0) * 524288 + B * 524288          # 2 x 32 layers x 4096 x 2 B per cached token
    # dominant kernel of the decode loop, HIP events on the library's stream
    eng.generate(ids, out_q, max_new=8, eos_id=-1, pad_id=0, use_graph=use_graph)        # state: a prefill + a few steps
    dom, other = None, [None]
    if B <= 2:
        try:
            ms = eng.time_unit(7, 8)               # in situ: 8 eager decode steps, an event pair around each of the 32 chained launches
            nb = H_ * I_ * wbytes(H_, I_) + (3 * H_ + 2 * lc.lora_r) * H_ * wbytes(3 * H_ + 16, H_) + B * (I_ + 2 * H_ + 3 * H_ + 16) * 2 + H_ * 2
            dom = (f"decode_chain_k<{args.dtype}{',W8' if wbytes(H_, I_) == 1 else ''}> (chained down_proj(l) -> RMSNorm+QKV(l+1) launch, fence-free hand-off)",
                   ms, nb, f"decode_chain_k B={B} {args.dtype}{' fp8' if args.fp8 else ''}")
        except Exception:
            dom = None
    if dom is None and B > 32:
        # 33-64 rows (the row-block family): the decode attention is the dominant launch; timed at the mean context of the timed decode
        eng.generate(ids, out_q, max_new=max(N // 2, 8), eos_id=-1, pad_id=0, use_graph=use_graph)
        L_ctx = T + max(N // 2, 8)
        ms_a = eng.time_unit(6, 10)
        nb_a = B * (2 * L_ctx * H_ * 2 + 2 * H_ * 2 + 3 * H_ * 2 + H_ * 2)
        dom = (f"decode_attention_k<{args.dtype}> (throughput variant at {B} rows; LoRA-B + RoPE + KV append + softmax.V)", ms_a, nb_a,
               f"decode_attention_k B={B} {args.dtype}")
    if dom is None:
        ms = eng.time_unit(1, 10)
        wb = wbytes(2 * I_, H_)
        nb = 2 * I_ * H_ * wb + B * H_ * wb + H_ * 2 + B * I_ * 2
        nm = (f"xstat16_k<{args.dtype},EPI_SILU_MUL,NORM> (gate/up SwiGLU with the RMSNorm prologue, one-row-tile family of batch 3-16)" if (3 <= B <= 16 and wb == 2) else
              f"xstat32_k<{args.dtype},EPI_SILU_MUL{',W8,A8 (fp8 x fp8 MFMA)' if wb == 1 else ''}> (gate/up SwiGLU, activation-stationary batch 3-32 GEMM)" if B > 2 else
              f"skinny_gemm_k<{args.dtype},MT,EPI_SILU_MUL,NORM{',W8' if wb == 1 else ''}> (gate/up SwiGLU GEMV)")
        dom = (nm, ms, nb, f"gate_up B={B} {args.dtype}{' fp8' if args.fp8 else ''}")
        if B > 2:
            # rocprofv3 ranks the decode attention first at batch 32 (profiles/r03_bench_default_kernel_stats.md): time it at the state the
            # 8-token generate above left (context T + 8) and name whichever of the two takes longer per launch
            try:
                eng.generate(ids, out_q, max_new=max(N // 2, 8), eos_id=-1, pad_id=0, use_graph=use_graph)   # state: the MEAN context of the timed decode
                L_ctx = T + max(N // 2, 8)
                ms_a = eng.time_unit(6, 10)
                nb_a = B * (2 * L_ctx * H_ * 2 + 2 * H_ * 2 + 3 * H_ * 2 + H_ * 2)       # K and V rows of the context + the appended row, qkv in, out
                other[0] = {"kernel": f"decode_attention_k<{args.dtype}> (batch-32 throughput variant; LoRA-B + RoPE + KV append + softmax.V)",
                            "us_per_launch": ms_a * 1e3, "bytes_per_launch": nb_a, "context": L_ctx,
                            "achieved": nb_a / (ms_a * 1e-3) / 1e9, "frac": nb_a / (ms_a * 1e-3) / 1e9 / HBM_PEAK_GBS}
                if ms_a > ms:
                    other[0], dom = ({"kernel": nm, "us_per_launch": ms * 1e3, "bytes_per_launch": nb, "achieved": nb / (ms * 1e-3) / 1e9,
                                      "frac": nb / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS},
                                     (other[0]["kernel"], ms_a, nb_a, f"decode_attention_k B={B} {args.dtype}{' fp8' if args.fp8 else ''}"))
            except Exception:
                pass
    name, k_ms, k_bytes, key = dom
    eng.generate(ids, out_q, max_new=8, eos_id=-1, pad_id=0, use_graph=use_graph)
    step_ms = eng.time_unit(0, 20)
    enc_tf = encode_flops(cfg) / (enc_ms * 1e-3) / 1e12
    pre_tf = prefill_flops(lc, T, B) / (prefill_ms * 1e-3) / 1e12
    roof = {
        "bound": "hbm", "kernel": name,
        "achieved": k_bytes / (k_ms * 1e-3) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
        "frac": k_bytes / (k_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, "traffic": pmc_traffic(key), "traffic_source": pmc_source(key),
        "bytes_per_launch": k_bytes, "us_per_launch": k_ms * 1e3, "second_kernel": other[0],
        "decode_step_ms": step_ms, "decode_step_weight_GBs": step_bytes / (step_ms * 1e-3) / 1e9,
        "decode_step_frac": step_bytes / (step_ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
        # average over the timed reports: (weights + KV read/write per SURVEY 8(d)) / mean step time / 8 TB/s
        "prefill_ms": prefill_ms, "decode_avg_step_ms": avg_step_ms,
        "decode_avg_frac": (step_bytes + kv_bytes) / (avg_step_ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
        # the encoder always computes in the model dtype (bf16 peak); the prefill GEMMs of the fp8 configuration run on the fp8 MFMA and are
        # priced against the fp8 dense peak (round 3 reported them against the bf16 peak: VERDICT r3 "weak" 9)
        "mfma": {"peak_tflops": MFMA_PEAK_TFLOPS, "encode_gflop_per_img": encode_flops(cfg) / 1e9, "encode_tflops": enc_tf,
                 "encode_frac": enc_tf / MFMA_PEAK_TFLOPS, "prefill_tflop": prefill_flops(lc, T, B) / 1e12, "prefill_tflops": pre_tf,
                 "prefill_peak_tflops": MFMA_FP8_PEAK_TFLOPS if args.fp8 else MFMA_PEAK_TFLOPS,
                 "prefill_frac": pre_tf / (MFMA_FP8_PEAK_TFLOPS if args.fp8 else MFMA_PEAK_TFLOPS),
                 "prefill_weight_GBs": step_bytes / (prefill_ms * 1e-3) / 1e9},
    }
    return enc_ms, roof


def run_steps(eng, cfg, args, B, T, N, rank, world, dist, steps, warmup, use_graph):
    from radialog_amd import synth
    from radialog_amd.shard import allgather_tokens
    img = synth.synth_images(B, cfg.vision.img, seed=16 + rank).to(eng.device)
    ids = synth.synth_prompt_ids(B, T, vocab=cfg.llama.vocab, pad_rows=(B > 1), seed=7 + rank).to(eng.device)
    box = {}

    def step():
        q, _ = eng.encode_image(img, want_image_embeds=False)
        box["q"] = q
        toks, _, n = eng.generate(ids, q, max_new=N, eos_id=-1, pad_id=0, use_graph=use_graph)
        return allgather_tokens(toks, world, engine=eng)          # librdx's ncclAllGather when a communicator is up, else identity

    def fence():
        _sync()
        if dist is not None:
            dist.barrier()
        _sync()

    out = None
    for _ in range(warmup):
        out = step()
    fence()
    t0 = time.perf_counter()
    for _ in range(steps):
        out = step()
    fence()
    elapsed = time.perf_counter() - t0
    return elapsed, out, img, ids, box.get("q")


def fixture_check(dtype, B, fp8, tokens_row0):
    """The first 8 greedy tokens of row 0 of what was just timed against tests/golden/bench_tokens.json (committed; written by
    tools/make_bench_fixture.py on an MI355X from this engine, whose batch-1 bf16 line is itself checked against the full-depth CPU
    oracle in every default run -- cpu_baseline.parity). The kernels are deterministic (fixed reduction orders, no atomics), so any
    difference means a kernel now computes something else."""
    key = f"{dtype}{'+fp8w' if fp8 else ''}_b{B}_row0"
    try:
        with open(os.path.join(REPO, "tests", "golden", "bench_tokens.json")) as f:
            want = json.load(f).get(key)
    except Exception:
        want = None
    if want is None:
        return {"key": key, "tokens": tokens_row0, "expected": None, "ok": True, "note": "no committed fixture for this configuration"}
    return {"key": key, "tokens": tokens_row0, "expected": want, "ok": list(want) == list(tokens_row0)}


def write_outputs(path, **arrays):
    """--dump-outputs: each array as float32 path/<name>.npy. What the timed path returns is small (token ids int32[B x ranks, N],
    exact in float32 below 2^24; Q-Former output f32[B, 32, 768]): 13 MB at the 128 rows one context holds, so nothing is sampled."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(path, name + ".npy"), a.detach().float().cpu().numpy())


def cpu_baseline_pointer():
    """N > 1 lines: the CPU oracle is timed on rank 0 at N = 1 only (contract); multi-rank lines carry the committed N = 1 figure of this
    build so that SCALE records are self-contained."""
    for name in ("r06_bench.json", "r05_bench.json", "r04_bench.json", "r03_bench.json"):
        try:
            with open(os.path.join(REPO, "profiles", name)) as f:
                cb = json.loads(f.read().strip().splitlines()[-1])["cpu_baseline"]
            return {"value": cb["value"], "unit": cb["unit"], "cores": cb["cores"], "kind": cb["kind"],
                    "sample": f"not re-timed at N > 1: the N = 1 figure committed in profiles/{name} ({cb['sample'][:160]}...)", "source": f"profiles/{name}"}
        except Exception:
            continue
    return {"value": None, "unit": "reports/s", "cores": None, "kind": "port", "sample": "timed at N = 1 only (run `python bench.py` without --gpus)"}


def spawn_command(n, port, argv):
    """The launcher line `python bench.py --gpus N` turns itself into (the driver's own form): one process per GPU, 127.0.0.1 rendezvous."""
    return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
            "--master-port", str(port), os.path.abspath(__file__)] + list(argv)


def spawn_ranks(args):
    """`python bench.py --gpus N` with no launcher in the environment: run `torch.distributed.run` with N local ranks (one process per
    GPU) as a child and exit with its status. A child, not an exec: device_count() may already have initialised the HIP runtime here.
    The reference has no inference launcher to mirror (its only one is the training DDP of model/lavis/common/dist_utils.py:57-91)."""
    import socket
    import subprocess
    n = args.gpus
    vis = n if STUB else torch.cuda.device_count()
    if vis < n:
        print(f"bench.py: --gpus {n} but only {vis} GPU(s) are visible to this process (torch.cuda.device_count()); refusing to "
              f"benchmark fewer GPUs than asked for", file=sys.stderr)
        sys.exit(2)
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")       # dmabuf IPC: what RCCL needs between the ranks' processes on this driver
    env.setdefault("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or 8) // n)))
    cmd = spawn_command(n, port, sys.argv[1:])
    print("bench.py: no launcher in the environment, starting %d ranks: %s" % (n, " ".join(cmd)), file=sys.stderr)
    sys.stdout.flush(); sys.stderr.flush()
    rc = subprocess.run(cmd, env=env).returncode
    sys.exit(rc if rc >= 0 else 128 - rc)          # killed by signal S: the shell's 128 + S


def resolve_gpus(args, env):
    """--gpus: an explicit value must agree with the launcher's WORLD_SIZE (exit 2 otherwise: the line would carry the wrong n_gpus);
    without the flag the launcher's WORLD_SIZE is taken (`torchrun --nproc-per-node N bench.py` must not fail), or 1."""
    world = int(env.get("WORLD_SIZE", "1")) if ("WORLD_SIZE" in env or "RANK" in env) else None
    if args.gpus is None:
        args.gpus = world or 1
    if args.gpus < 1:
        print("bench.py: --gpus must be >= 1", file=sys.stderr)
        sys.exit(2)
    if world is not None and world != args.gpus:
        print(f"bench.py: --gpus {args.gpus} but the launcher's WORLD_SIZE is {world}; start it with --nproc-per-node {args.gpus} "
              f"(or run `python bench.py --gpus {args.gpus}` alone: it starts the ranks itself)", file=sys.stderr)
        sys.exit(2)


def gather_clock(dist, elapsed, world, device):
    """MAX over ranks of the per-rank clock + every rank's own value (per_rank_ms_per_step has exactly `world` entries)."""
    te = torch.tensor([elapsed], dtype=torch.float64, device=device)
    allt = [torch.zeros_like(te) for _ in range(world)]
    dist.all_gather(allt, te)
    dist.all_reduce(te, op=dist.ReduceOp.MAX)
    return float(te.item()), [float(t.item()) for t in allt]


def _sig(x, n=5):
    """Floats of the compact line at n significant digits (the line has to stay under 4 KB; the full figures are in the detail file)."""
    if isinstance(x, float):
        return float(f"{x:.{n}g}")
    if isinstance(x, list):
        return [_sig(v, n) for v in x]
    return x


def _parity_brief(p):
    return {"ok": bool(p.get("ok")), "same": p.get("tokens_identical"), "n": p.get("tokens_compared"), "worst": _sig(p.get("worst_logit_err"), 3),
            "bar": _sig(p.get("abs_bar"), 3)}


def compact_line(res, detail_name):
    """The ONE JSON line of stdout, under 4 KB (round 6, VERDICT r5 "weak" 10: the round-5 line was 15 KB, the driver keeps 8 KB of stdout, so the
    configs[2] / configs[4] sub-runs never reached its record): the contract's fields in full, `roofline` and `cpu_baseline` with scalars only, every
    sub-run as `<key>_value` / `_ms_per_step` / `_decode_ms` / `_frac` scalars, every parity leg as {ok, same, n, worst, bar}. Everything else -- kernel
    names, prose, per-phase tables, token fixtures, divergence notes -- is in the detail file written beside it (`detail`).
    A plain run's record (no --full) holds the timed run alone: its line is the contract's fields and that run's own figures."""
    out = {k: res[k] for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                               "dtype", "data")}
    cfg = res["config"]
    out["config"] = {"workload": cfg["workload"][:150], "per_gpu_batch": cfg["per_gpu_batch"], "global_batch": cfg["global_batch"],
                     "prompt_len": cfg["prompt_len"], "new_tokens": cfg["new_tokens"], "parallelism": cfg["parallelism"]}
    if "roofline" not in res:
        out.update(tokens_per_s=_sig(res["tokens_per_s"]), rccl_ranks=res["rccl_ranks"], per_rank_ms_per_step=_sig(res["per_rank_ms_per_step"], 12),
                   collective=(res.get("collective") or "")[:70], build_hash=res.get("build_hash"))
        return out
    roof = res["roofline"]
    r = {"bound": roof["bound"], "kernel": roof["kernel"].split(" (")[0], "achieved": _sig(roof["achieved"]), "peak": roof["peak"], "unit": roof["unit"],
         "frac": _sig(roof["frac"]), "traffic": roof["traffic"], "bytes_per_launch": roof["bytes_per_launch"], "us_per_launch": _sig(roof["us_per_launch"]),
         "decode_avg_step_ms": _sig(roof["decode_avg_step_ms"]), "decode_avg_frac": _sig(roof["decode_avg_frac"]), "prefill_ms": _sig(roof["prefill_ms"]),
         "mfma_encode_frac": _sig(roof["mfma"]["encode_frac"]), "mfma_prefill_frac": _sig(roof["mfma"]["prefill_frac"])}
    ts = roof.get("traffic_source") or {}
    r["traffic_stale"] = ts.get("stale")
    out["encoder_ms_per_img"] = _sig(res["encoder_ms_per_img"])
    out["tokens_per_s"] = _sig(res["tokens_per_s"])
    out["rccl_ranks"] = res["rccl_ranks"]
    out["per_rank_ms_per_step"] = _sig(res["per_rank_ms_per_step"], 12)
    out["collective"] = (res.get("collective") or "")[:70]
    sub_tokens_ok = True
    for key in ("b32", "fp8_b32", "b64", "b128", "fp8_b128", "f16_b1"):
        sub = res.get(key)
        if not sub:
            continue
        out[f"{key}_value"] = _sig(sub["value"])
        out[f"{key}_decode_ms"] = _sig(sub["decode_avg_step_ms"])
        out[f"{key}_frac"] = _sig(sub["decode_avg_frac"])
        sub_tokens_ok = sub_tokens_ok and bool(sub["token_check"]["ok"])
        r[f"{key}_decode_avg_frac"] = _sig(sub["decode_avg_frac"])              # (also inside `roofline`: the driver's record keeps that object's scalars)
        if key in ("b32", "fp8_b32"):                                           # BASELINE configs[2] / [3] and [4]: the whole sub-line
            out[f"{key}_ms_per_step"] = _sig(sub["ms_per_step"])
            out[f"{key}_prefill_ms"] = _sig(sub["prefill_ms"])
            out[f"{key}_global_batch"] = sub["global_batch"]
            out[f"{key}_prefill_mfma_frac"] = r[f"{key}_prefill_mfma_frac"] = _sig(sub["mfma"]["prefill_frac"])
            out[f"{key}_enc_ms"] = _sig(sub["encoder_ms_per_img"])
    if "value_f16" in res:
        out["value_f16"] = _sig(res["value_f16"])
    e = res.get("enc_b256")
    if e and "encoder_ms_per_img" in e:
        out["enc_b256_ms"] = _sig(e["encoder_ms_per_img"])
        out["enc_b256_frac"] = r["enc_b256_mfma_frac"] = _sig(e["encode_frac"])
    out["roofline"] = r
    cb = res.get("cpu_baseline") or {}
    out["cpu_baseline"] = {k: (_sig(cb[k]) if k != "sample" else cb[k][:230]) for k in
                           ("value", "unit", "cores", "host_cpus", "kind", "sample", "s_per_token", "source") if k in cb}
    par = {k[len("parity"):].lstrip("_") or res["dtype"]: _parity_brief(v) for k, v in cb.items() if k.startswith("parity")}
    if par:
        out["parity"] = par
    for k, v in cb.items():
        if k.startswith("fp8_vs_unquantised"):
            out[k] = {"same": v["tokens_identical"], "n": v["tokens_compared"], "median_err": _sig(v["median_logit_err"], 3), "worst": _sig(v["worst_logit_err"], 3),
                      "median_margin": _sig(v["median_oracle_margin"], 3)}
    if "fp8_b32" in res:
        out["fp8_statement"] = "no e4m3 variant keeps the un-quantised tokens on random-init weights: engine rule 30/96, W8A8 31/96 .. W8A16 39/96 (profiles/r06_fp8_variants.md)"
    out["tokens_ok"] = bool(res["token_check"]["ok"]) and sub_tokens_ok          # first 8 tokens of every timed configuration == tests/golden/bench_tokens.json
    for k in ("oracle_checked", "fixtures_match", "results_verified", "max_batch_per_gpu", "build_hash"):
        if k in res:
            out[k] = res[k]
    out["detail"] = detail_name
    return out


def main():
    args = parse()
    resolve_gpus(args, os.environ)
    if args.gpus > 1 and "RANK" not in os.environ and "WORLD_SIZE" not in os.environ:
        spawn_ranks(args)                          # exits with the launcher's status
    # ONE JSON line on stdout, whatever native libraries print: RCCL writes its version banner to fd 1 at communicator bring-up. fd 1 is
    # pointed at stderr for the whole run and the result line goes to the saved descriptor.
    sys.stdout.flush()
    out_fd = os.dup(1)
    os.dup2(2, 1)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    launched = world > 1 or "RANK" in os.environ      # by torch.distributed.run (also at --nproc-per-node 1)
    if not STUB and local_rank >= torch.cuda.device_count():
        print(f"bench.py: rank {rank} needs GPU {local_rank} but only {torch.cuda.device_count()} GPU(s) are visible", file=sys.stderr)
        sys.exit(2)
    if launched:
        import torch.distributed as dist
        if not STUB:
            torch.cuda.set_device(local_rank)
        # launcher-side plumbing only (RCCL id broadcast, barrier, max-over-ranks clock): a gloo group on the host. The data-path
        # collective is librdx's own RCCL communicator; `RDX_BENCH_PG=nccl` puts the plumbing on torch's RCCL group instead.
        backend = "gloo" if STUB else os.environ.get("RDX_BENCH_PG", "gloo")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group("gloo")
    else:
        dist = None

    from radialog_amd.config import full_cfg
    from radialog_amd.engine import RdxEngine, synth_getter
    from radialog_amd.shard import init_comm
    Engine = _StubEngine if STUB else RdxEngine

    cfg = full_cfg()
    T, N = args.prompt_len, args.new_tokens
    max_len = (T + N + 64 + 31) // 32 * 32
    use_graph = not args.no_graph
    host_dev = lambda e: e.device if (dist is not None and dist.get_backend() == "nccl") else "cpu"      # noqa: E731
    want_oracle = args.full and world == 1 and not args.no_cpu_baseline and not STUB

    def timed_run(B, fp8, steps, warmup, keep_engine=False, dtype=None, dump=False):
        """One engine per rank (full weight replica), RCCL communicator inside librdx, `steps` timed steps between barriers, the MAX of
        the per-rank clocks. Every rank calls this (collectives inside); rank 0 also writes the last step's outputs (dump and
        --dump-outputs) and, with --full, gets the per-phase detail."""
        dtype = dtype or args.dtype
        eng = Engine(cfg, dtype=dtype, device=local_rank, max_batch=B, max_len=max_len, lora=True, weights_fp8=fp8)
        eng.load_weights(synth_getter(cfg, eng.device, lora=True))
        comm_note = None
        if launched:
            try:
                init_comm(eng, rank, world)               # RCCL communicator inside librdx (rdx_comm_init)
            except Exception as e:                        # keep the run (and say so in the JSON line): the token gather then goes over the host group
                comm_note = f"rdx_comm_init failed ({type(e).__name__}: {e}); token ids gathered over the torch.distributed host group instead"
                print("warning: " + comm_note, file=sys.stderr)
            if world > 1:                                 # all ranks take the same path: any failure switches every rank to the host group
                ok = torch.tensor([0 if comm_note else 1], dtype=torch.int32, device=host_dev(eng))
                dist.all_reduce(ok, op=dist.ReduceOp.MIN)
                if int(ok.item()) == 0:
                    eng.comm_off = True
                    comm_note = comm_note or "rdx_comm_init failed on another rank; token ids gathered over the torch.distributed host group instead"
        elapsed, out, img, ids, out_q = run_steps(eng, cfg, args, B, T, N, rank, world, dist, steps, warmup, use_graph)
        per_rank_ms = [elapsed / steps * 1e3]
        if dist is not None:
            elapsed, per_rank = gather_clock(dist, elapsed, world, host_dev(eng))
            per_rank_ms = [t / steps * 1e3 for t in per_rank]
        assert out.shape[0] == B * world and out.shape[1] == N, f"gathered token matrix {tuple(out.shape)}, expected {(B * world, N)}"
        r = {"B": B, "fp8": fp8, "dtype": dtype, "steps": steps, "warmup": warmup, "elapsed": elapsed, "per_rank_ms": per_rank_ms, "comm_world": eng.comm_world,
             "comm_note": comm_note, "tokens_row0": [int(t) for t in out[rank * B, :8].tolist()]}
        if rank == 0 and dump and args.dump_outputs:
            write_outputs(args.dump_outputs, tokens=out, qformer_out=out_q)      # before anything else runs on the engine's kept buffers
        if rank == 0 and args.full:
            fp8_was, dt_was = args.fp8, args.dtype
            args.fp8, args.dtype = fp8, dtype
            r["enc_ms"], r["roof"] = measure_detail(eng, cfg, args, B, T, N, img, ids, out_q, elapsed / steps * 1e3, use_graph)
            args.fp8, args.dtype = fp8_was, dt_was
            r["token_check"] = fixture_check(dtype, B, fp8, r["tokens_row0"])
            if keep_engine:       # rank 0: the timed engine stays up for the oracle's teacher-forced check (untimed, after the sub-runs)
                r["engine"], r["img"], r["ids"] = eng, img, ids
                return r
        eng.close()
        return r

    def engine_tf(eng, img, ids, ref_tokens, ref_q):
        """The engine on row 0 of the benchmark's image and prompt: its encoder output against the oracle's (relative L2), and its decoder on
        the oracle's Q-Former output (ref_q None: on its OWN encoder output -- the end-to-end leg), fed the oracle's tokens: (argmax per step,
        fp32 logits [n, V], encoder rel-L2)."""
        q, _ = eng.encode_image(img[:1], want_image_embeds=False)
        erel = None if ref_q is None else float((q.float().cpu() - ref_q).norm() / ref_q.norm())
        n = len(ref_tokens)
        _, lg = eng.prefill(ids[:1], q if ref_q is None else ref_q, max_new=n, eos_id=-1)
        rows = [lg[0].float().cpu().clone()]
        for s_ in range(1, n):
            _, lg = eng.decode_step(input_ids=torch.tensor([ref_tokens[s_ - 1]]))
            rows.append(lg[0].float().cpu().clone())
        hl = torch.stack(rows)
        return hl.argmax(-1).tolist(), hl, erel

    def engine_tf_rows(eng, img, ids, ids_row0, ref_tokens, ref_q):
        """Row 0 of a BATCHED run (the batch 3-32 kernel family) teacher-forced with the oracle's tokens: the batch is the benchmark's own images
        and prompts (ragged left padding) with row 0 replaced by the oracle's prompt and Q-Former output; the other rows run free (their own
        argmax is fed back). -> (argmax of row 0 per step, fp32 logits of row 0 [n, V])."""
        q, _ = eng.encode_image(img, want_image_embeds=False)
        q = q.clone()
        q[0] = ref_q[0].to(q.device)
        ids = ids.clone()
        ids[0] = ids_row0[0].to(ids.device)
        n = len(ref_tokens)
        _, lg = eng.prefill(ids, q, max_new=n, eos_id=-1)
        rows = [lg[0].float().cpu().clone()]
        for s_ in range(1, n):
            nxt = lg.float().argmax(-1).to(torch.int32)
            nxt[0] = int(ref_tokens[s_ - 1])
            _, lg = eng.decode_step(input_ids=nxt)
            rows.append(lg[0].float().cpu().clone())
        hl = torch.stack(rows)
        return hl.argmax(-1).tolist(), hl

    def sub_line(r, workload):
        roof = r["roof"]
        return {"workload": workload, "value": r["steps"] * r["B"] * world / r["elapsed"], "unit": "reports/s", "n_gpus": world, "dtype": r["dtype"] + ("+fp8w" if r["fp8"] else ""),
                "per_gpu_batch": r["B"], "global_batch": r["B"] * world, "steps": r["steps"], "warmup": r["warmup"],
                "ms_per_step": r["elapsed"] / r["steps"] * 1e3, "tokens_per_s": r["steps"] * r["B"] * world * N / r["elapsed"],
                "per_rank_ms_per_step": r["per_rank_ms"], "rccl_ranks": r["comm_world"],
                "encoder_ms_per_img": r["enc_ms"], "prefill_ms": roof["prefill_ms"], "decode_avg_step_ms": roof["decode_avg_step_ms"],
                "decode_avg_frac": roof["decode_avg_frac"], "kernel": roof["kernel"], "kernel_frac": roof["frac"],
                "kernel_us": roof["us_per_launch"], "traffic": roof["traffic"], "traffic_source": roof.get("traffic_source"), "mfma": roof["mfma"],
                "token_check": r["token_check"]}

    def enc_b256():
        """encoder ms/img at the reference's embedding-dump batch (pretraining/train.py:139: batch 256), bf16 MFMA fraction: a vision-only context."""
        from radialog_amd import synth
        eb = 256
        eng = RdxEngine(cfg, dtype=args.dtype, device=local_rank, max_batch=1, max_len=64, lora=True, llama=False)
        eng.load_weights(synth_getter(cfg, eng.device, lora=True), llama=False)
        img = synth.synth_images(eb, cfg.vision.img, device=eng.device, seed=16)
        eng.encode_image(img, want_image_embeds=False)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(3):
            eng.encode_image(img, want_image_embeds=False)
        ms = (time.perf_counter() - t0) / 3 / eb * 1e3
        eng.close()
        tf = encode_flops(cfg) / (ms * 1e-3) / 1e12
        return {"workload": "image encode alone at the reference's embedding-dump batch (pretraining/train.py:139), 256 x 448 px", "batch": eb,
                "encoder_ms_per_img": ms, "images_per_s": 1e3 / ms, "encode_tflops": tf, "encode_frac": tf / MFMA_PEAK_TFLOPS, "peak_tflops": MFMA_PEAK_TFLOPS}

    B = args.batch
    main_r = timed_run(B, args.fp8, args.steps, args.warmup, keep_engine=(B == 1 and want_oracle), dump=True)
    subs = {}
    k2 = max(2, min(args.steps, 3))
    if args.full and B == 1 and not args.fp8 and not args.no_b32:
        # BASELINE configs[2] (one GPU) / configs[3] (8 GPUs: global batch 256, one all-gather of int32[32,256] per rank) in the same job
        # and JSON line: batch 32 per GPU, KV cache in HBM, hipGraph-captured decode step
        subs["b32"] = (timed_run(32, False, k2, 1, keep_engine=want_oracle),
                       f"configs[{2 if world == 1 else 3}]: per-GPU batch 32 (global {32 * world}), same pipeline, "
                       "hipGraph-captured decode step" + (", RCCL all-gather of the token ids" if world > 1 else ""))
    if args.full and B == 1 and not args.fp8 and not args.no_fp8:
        # BASELINE configs[4] per-GPU load: fp8 e4m3 decoder weights + per-row scale, LoRA epilogue, batch 32 per GPU
        subs["fp8_b32"] = (timed_run(32, True, k2, 1, keep_engine=want_oracle),
                           f"configs[4]: fp8 e4m3 decoder GEMM weights + per-row scale + un-merged LoRA epilogue, per-GPU "
                           f"batch 32 (global {32 * world}); no reference fp8 path exists -- its oracle is the reference math on the "
                           "same fake-quantised operands (cpu_baseline.parity_fp8 / tests/test_gpu_parity.py), i.e. unpinnable against the reference itself; "
                           "cpu_baseline.fp8_vs_unquantised says what it costs against the un-quantised oracle")
    if args.full and B == 1 and not args.fp8 and not args.no_b64 and not STUB and world == 1:        # one rank only: the N > 1 run stays lean (its per-GPU loads are b32 / fp8_b32)
        # round 5: 64 reports per GPU (33-64 decoder rows: the row-block family) -- not a BASELINE configuration (those stop at 32 per GPU): what the
        # 288 GB of HBM buy when the 13.2 GB weight stream of a decode step is amortised over twice the reports
        subs["b64"] = (timed_run(64, False, 2, 1), f"per-GPU batch 64 (global {64 * world}): beyond BASELINE configs[2]/[3]'s 32 per GPU, same pipeline, hipGraph step")
        subs["b128"] = (timed_run(128, False, 2, 1), f"per-GPU batch 128 (global {128 * world}), the most one context holds (RDX_MAX_ROWS): four 32-row blocks per tile walker")
        if not args.no_fp8:
            subs["fp8_b128"] = (timed_run(128, True, 2, 1), f"per-GPU batch 128 (global {128 * world}) with the configs[4] weight path: fp8 x fp8 kernels per 32-row block "
                                                            "(row by row the arithmetic of fp8_b32: tests/test_gpu_parity.py::test_fp8_row_blocks_equal_the_32_row_kernels_row_by_row)")
    f16_r = None
    if args.full and B == 1 and not args.fp8 and args.dtype != "f16" and world == 1 and not args.no_f16 and not STUB:
        # the reference's dtype, in which token identity with the CPU path actually holds (parity_f16): the same configs[1] workload timed in fp16
        f16_r = timed_run(1, False, k2, 1, keep_engine=want_oracle, dtype="f16")

    def line_head(r):
        """The headline of the timed run: the contract's fields and what that run alone gives."""
        return {
            "metric": "reports_per_sec (448px CXR encode + 160-tok prefill + 256-tok greedy decode)",
            "value": args.steps * B * world / r["elapsed"], "unit": "reports/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": r["elapsed"] / args.steps * 1e3, "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": args.dtype + ("+fp8w" if args.fp8 else ""),
            "data": "synthetic" if not STUB else "STUB (RDX_BENCH_STUB=1: no GPU, fake timings -- control-flow test only)",
            "config": {"workload": f"configs[{1 if B == 1 else 2}]: per-GPU batch {B} BioViL-T(ResNet-50)+Q-Former encode 448px, "
                                   f"Vicuna-7B prefill T={T}, {N}-token greedy decode (LoRA r=8 un-merged, hipGraph step={use_graph}"
                                   + (", fp8 e4m3 decoder weights + per-row scale [configs[4] weight path]" if args.fp8 else "") + ")",
                       "per_gpu_batch": B, "global_batch": B * world, "prompt_len": T, "new_tokens": N,
                       "parallelism": f"dp{world}", "weights": "random-init (deterministic generator)"},
            "tokens_per_s": args.steps * B * world * N / r["elapsed"],
            "rccl_ranks": r["comm_world"], "per_rank_ms_per_step": r["per_rank_ms"],
            "collective": ("rdx_allgather_tokens (ncclAllGather inside librdx), int32[%d,%d] per rank per step" % (B, N)) if r["comm_world"] else r["comm_note"],
        }

    if rank == 0 and not args.full:
        from radialog_amd import _lib
        res = line_head(main_r)
        res["build_hash"] = "stub" if STUB else _lib.build_hash()
        sys.stdout.flush()
        os.write(out_fd, (json.dumps(compact_line(res, None), separators=(",", ":")) + "\n").encode())
        rc = 0
    elif rank == 0:
        r, roof = main_r, main_r["roof"]
        res = line_head(r)
        res.update(encoder_ms_per_img=r["enc_ms"], roofline=roof, token_check=r["token_check"])
        if args.dtype == "bf16" and not args.fp8:
            res["dtype_note"] = ("bf16 is the THROUGHPUT dtype: against the CPU oracle its greedy tokens flip at near-ties (cpu_baseline.parity: teacher-forced "
                                 "argmax identity, first flip, margin); token identity with the reference's CPU path holds in the reference's own dtype, fp16 -- "
                                 "value_f16 is the same workload timed in fp16, cpu_baseline.parity_f16 its check")
        for key, (sr, wl) in subs.items():
            res[key] = sub_line(sr, wl)
        if f16_r is not None:
            res["value_f16"] = f16_r["steps"] / f16_r["elapsed"]
            res["f16_b1"] = sub_line(f16_r, "configs[1] in fp16 (the reference's dtype; token-identical to the CPU oracle over the checked horizon): per-GPU batch 1")
        if world == 1 and B == 1 and not args.fp8 and not args.no_enc256 and not STUB:
            try:
                res["enc_b256"] = enc_b256()
            except Exception as e:                       # a too-small GPU must not lose the line
                res["enc_b256"] = {"error": f"{type(e).__name__}: {e}"}
        if want_oracle:
            ids1 = r["ids"] if r.get("ids") is not None else None

            def hip_tf(dn, ref_tokens, ref_q):
                if dn == args.dtype and not args.fp8 and r.get("engine") is not None:
                    return engine_tf(r["engine"], r["img"], r["ids"], ref_tokens, ref_q)
                if f16_r is not None and dn == "f16" and f16_r.get("engine") is not None:
                    return engine_tf(f16_r["engine"], f16_r["img"], f16_r["ids"], ref_tokens, ref_q)
                e2 = RdxEngine(cfg, dtype=dn, device=local_rank, max_batch=1, max_len=max_len, lora=True)       # the other dtype: a second engine
                e2.load_weights(synth_getter(cfg, e2.device, lora=True))
                try:
                    return engine_tf(e2, r["img"], r["ids"], ref_tokens, ref_q)
                finally:
                    e2.close()

            def e2e_tf(dn, ref_tokens):
                ht, hl, _ = engine_tf(f16_r["engine"], f16_r["img"], f16_r["ids"], ref_tokens, None)
                return ht, hl

            box = {}          # the batched legs need the oracle's Q-Former output: cpu_baseline hands it to hip_tf first

            def hip_tf_capture(dn, ref_tokens, ref_q):
                box["q"] = ref_q
                return hip_tf(dn, ref_tokens, ref_q)

            def sub_tf(key):
                sr = subs[key][0]
                return lambda ref_tokens: engine_tf_rows(sr["engine"], sr["img"], sr["ids"], ids1, ref_tokens, box["q"])

            have = lambda k: k in subs and subs[k][0].get("engine") is not None and ids1 is not None      # noqa: E731
            res["cpu_baseline"] = cpu_baseline(cfg, args.dtype, T, N, torch.device("cuda", local_rank), hip_tf=None if args.fp8 else hip_tf_capture,
                                               b32_tf=sub_tf("b32") if have("b32") else None, fp8_tf=sub_tf("fp8_b32") if have("fp8_b32") else None,
                                               e2e_tf=e2e_tf if (f16_r is not None and f16_r.get("engine") is not None) else None)
        elif world > 1:
            res["cpu_baseline"] = cpu_baseline_pointer()
        for rr in [r, f16_r] + [sr for sr, _ in subs.values()]:
            if rr is not None and rr.get("engine") is not None:
                rr["engine"].close()
        res["max_batch_per_gpu"] = 128                                      # librdx's decoder holds at most 128 rows per context (rdx_ctx.h RDX_MAX_ROWS)
        cb = res.get("cpu_baseline", {})
        fixtures = [res["token_check"]] + [res[k]["token_check"] for k in subs] + ([res["f16_b1"]["token_check"]] if f16_r is not None else [])
        parity_keys = [k for k in cb if k.startswith("parity")]
        oracle_checked = len(parity_keys) > 0
        oracle_ok = all(cb[k].get("ok", True) for k in parity_keys)
        # the exit code gates on verification again. The CPU oracle -- the independent checker -- failing is fatal (exit 3). A fixture
        # miss is only a WARNING when the oracle checked this very run (the batch-32 / fp8 fixtures were written by this engine, and a toolchain
        # change that moves one ulp may move them); when NO oracle parity ran (N > 1, --no-cpu-baseline, --fp8) the fixtures are the only check
        # there is, and a miss is fatal too.
        res["oracle_checked"] = oracle_checked
        res["oracle_legs"] = {k: bool(cb[k].get("ok")) for k in parity_keys}
        res["fixtures_match"] = all(c.get("ok", True) for c in fixtures)
        res["results_verified"] = (oracle_checked and oracle_ok) or (not oracle_checked and res["fixtures_match"] and not STUB)
        try:
            from radialog_amd import _lib as _l
            res["build_hash"] = "stub" if STUB else _l.build_hash()
        except Exception:
            res["build_hash"] = None
        # the full record (kernel names, prose, per-phase tables, divergence notes) beside the script; the ONE stdout line is its < 4 KB extract
        detail_path = os.environ.get("RDX_BENCH_DETAIL") or os.path.join(REPO, "bench_detail.json")
        try:
            with open(detail_path, "w") as f:
                json.dump(res, f, indent=1)
        except OSError as e:
            print(f"bench.py: could not write {detail_path}: {e}", file=sys.stderr)
        line = json.dumps(compact_line(res, os.path.basename(detail_path)), separators=(",", ":"))
        if len(line) > 4096:
            print(f"bench.py: WARNING: the result line is {len(line)} bytes (> 4096)", file=sys.stderr)
        sys.stdout.flush()
        os.write(out_fd, (line + "\n").encode())
        rc = 0 if (STUB or (oracle_ok and (oracle_checked or res["fixtures_match"]))) else 3
        if not res["fixtures_match"]:
            print("bench.py: WARNING: a timed configuration's first tokens differ from tests/golden/bench_tokens.json (token_check)", file=sys.stderr)
    else:
        rc = 0
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    if rc:
        print("bench.py: the timed configuration's tokens do not match the committed fixture / the oracle (see token_check, cpu_baseline.parity*)",
              file=sys.stderr)
        sys.exit(rc)


if __name__ == "__main__":
    main()
