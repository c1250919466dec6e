#!/usr/bin/env python
"""test.py -- the reference's batched report-generation loop (test.py:277-373) on the MI355X-native path.

Same flags (`--prompt`, `--lora_model`, `--num_workers`, `--use_embs`, `--num_beams`); batches of 12 left-padded
prompts, `lang_model.generate(input_ids=..., dicom=dicom_id if use_embs else None, max_new_tokens=300,
return_dict_in_generate=True, output_scores=True)`, predictions = text after "ASSISTANT:". MIMIC-CXR is credentialed
data and the NLG/CheXbert metrics need Java and a second conda env, so the dataset is replaced by synthetic studies
(`--num_samples`) whose image embeddings are produced by the encoder half first (the reference's
pretraining/train.py evaluate branch) and handed over through the same {dicom: float32[32,768]} mapping.
With WORLD_SIZE > 1 (torch.distributed.run) the studies are sharded across ranks and predictions all-gathered."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from radialog_amd import synth                                              # noqa: E402
from radialog_amd.config import PROMPT_LOOKUP_DEFAULT                      # noqa: E402
from radialog_amd.embed_dump import dump_embeddings                         # noqa: E402
from radialog_amd.modeling_llama_imgemb import LlamaForCausalLM, PeftModelForCausalLM   # noqa: E402
from radialog_amd.prompter import new_conversation, report_prompt          # noqa: E402
from radialog_amd.shard import allgather_ragged, shard_range               # noqa: E402
from radialog_amd.tokenizer import load_tokenizer                          # noqa: E402


ENGINE_ROWS = 128     # librdx holds up to 128 decoder rows per context in the model dtype (rdx_ctx.h RDX_MAX_ROWS; round 5: the row-block decode family) ...
ENGINE_ROWS_FP8 = 128  # ... and with fp8 weights (round 5: the 32-row fp8 x fp8 decode kernels per row block)


def engine_rows(batch_size, num_beams, bin_qa=False, all_qa=False, fp8=False):
    """Rows the engine must hold at once -> (max_batch, report-loop batch size, findings-QA batch size): the report loop runs batch_size
    prompts x num_beams beam rows -- the reference's 12 x 3 = 36 (test.py:267,:279) in ONE pass since round 5 (chunked only when that exceeds the
    engine's rows: 128); the binary QA pass is greedy (14 questions per study, test.py:548-590); the findings QA runs
    batches of 5 with beams (test.py:610-650)."""
    rows = ENGINE_ROWS_FP8 if fp8 else ENGINE_ROWS
    beams = max(num_beams, 1)
    if beams > 8:
        raise ValueError(f"--num_beams {beams}: rdx_beam_search supports at most 8 beams")
    if batch_size * beams > rows:
        chunk = max(1, rows // beams)
        print(f"note: --batch_size {batch_size} x --num_beams {beams} exceeds the engine's {rows} rows; the report loop runs in chunks of {chunk}")
        batch_size = chunk
    qa_batch = max(1, min(5, rows // beams))
    max_batch = max(batch_size * beams, 14 if bin_qa else 0, qa_batch * beams if all_qa else 0, beams, 1)
    return max_batch, batch_size, qa_batch


def main(argv=None):
    """Returns {"ids", "preds", ...} (the reference's script only prints; the return value is what tests/test_gpu_entrypoints.py asserts on)."""
    p = argparse.ArgumentParser()
    p.add_argument("--prompt", type=str, default="img_matching_examples_ig2_noexamples_IMG_findings")
    p.add_argument("--lora_model", type=str, default=None)
    p.add_argument("--num_workers", type=int, default=8)
    p.add_argument("--use_embs", action="store_true", default=False)
    p.add_argument("--num_beams", type=int, default=1)
    p.add_argument("--vicuna", default=None)
    p.add_argument("--num_samples", type=int, default=24)
    p.add_argument("--batch_size", type=int, default=12)
    p.add_argument("--max_new_tokens", type=int, default=300)
    p.add_argument("--repetition_penalty", type=float, default=1.0, help="greedy decode: divide / multiply the logits of tokens already in the sequence (1.0 = off)")
    p.add_argument("--no_repeat_ngram_size", type=int, default=0, help="greedy decode: no n-gram of this size occurs twice (0 = off)")
    p.add_argument("--min_new_tokens", type=int, default=0, help="greedy decode: no EOS before this many generated tokens (0 = off)")
    p.add_argument("--do_sample", action="store_true", help="sample the report instead of decoding greedily (top_k 50, top_p 1.0, as transformers' defaults)")
    p.add_argument("--temperature", type=float, default=1.0, help="with --do_sample: divide the logits by this (1.0 = off)")
    p.add_argument("--seed", type=int, default=None, help="with --do_sample: the sampler's seed (default: drawn from torch's CPU generator)")
    p.add_argument("--logprobs", type=int, default=None, metavar="N", help="report the mean token log-prob of every report (and keep the N = 0 .. 8 likeliest "
                   "tokens of every step); greedy / sampled search only")
    p.add_argument("--prompt_lookup", type=int, nargs="?", const=PROMPT_LOOKUP_DEFAULT, default=0, metavar="N",
                   help="with --do_corr (greedy, num_beams 1): verify up to N tokens per forward, drafted from the prompt and the answer so far "
                        f"(prompt-lookup decoding; without a number: {PROMPT_LOOKUP_DEFAULT})")
    p.add_argument("--dtype", default="bf16", choices=["bf16", "f16"])
    p.add_argument("--synthetic", action="store_true", help="deterministic random-init weights (no checkpoints reachable offline)")
    p.add_argument("--fp8", action="store_true", help="BASELINE configs[4]: decoder GEMMs in OCP e4m3 on the fp8 MFMA (weights_fp8=True)")
    p.add_argument("--kv_fp8", action="store_true", help="the decoder's KV cache as e4m3 codes + one exponent byte per row (kv_fp8=True): half the cache bytes; "
                   "greedy / sampled search only (no --num_beams > 1, no --queue_rows)")
    p.add_argument("--queue_rows", type=int, default=0, help="report loop through a queue (generate_many): this many rows decode at a time and a finished "
                   "row takes the next waiting prompt (0 = off: the batched loop; greedy search only)")
    p.add_argument("--do_corr", action="store_true", help="automatic prompt correction on top of the reports (test.py:437-500)")
    p.add_argument("--do_cp_bin_qa", action="store_true", help="14 yes/no CheXpert questions per study (test.py:545-590)")
    p.add_argument("--do_cp_all_qa", action="store_true", help="'List all the findings' follow-up (test.py:608-650)")
    args = p.parse_args(argv)
    res = {}

    world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world > 1:
        import torch.distributed as dist
        torch.cuda.set_device(local)
        dist.init_process_group("nccl", device_id=torch.device("cuda", local))

    lo, hi = shard_range(args.num_samples, world, rank)
    dicoms = [f"synthetic-{i:05d}" for i in range(lo, hi)]
    tok = load_tokenizer(args.vicuna)
    dt = torch.float16 if args.dtype == "f16" else torch.bfloat16
    try:
        max_batch, args.batch_size, qa_batch = engine_rows(args.batch_size, args.num_beams, args.do_cp_bin_qa, args.do_cp_all_qa, fp8=args.fp8)
    except ValueError as e:
        p.error(str(e))
    beams = max(args.num_beams, 1)
    if args.kv_fp8 and (beams > 1 or args.queue_rows > 0):
        p.error("--kv_fp8 runs greedy / sampled search only: beam search and the row queue are not built on the fp8 KV cache")
    if args.logprobs is not None and (beams > 1 or args.queue_rows > 0 or not 0 <= args.logprobs <= 8):
        p.error("--logprobs N (0 .. 8) runs greedy / sampled search only: per-step logprobs of beams and of the row queue are not built")
    queue_stage = 0
    if args.queue_rows > 0:
        if beams > 1 or args.do_sample or args.repetition_penalty != 1.0 or args.no_repeat_ngram_size or args.min_new_tokens:
            p.error("--queue_rows runs greedy search only (no --num_beams > 1, --do_sample or logits rules)")
        from radialog_amd.engine import QUEUE_STAGE
        queue_stage = QUEUE_STAGE
        if args.queue_rows + queue_stage > (ENGINE_ROWS_FP8 if args.fp8 else ENGINE_ROWS):
            p.error(f"--queue_rows {args.queue_rows} + {queue_stage} staging rows exceed the engine's rows")
        max_batch = max(max_batch, args.queue_rows + queue_stage)
    lang_model = LlamaForCausalLM.from_pretrained(args.vicuna, torch_dtype=dt, device_map="auto", max_batch=max_batch,
                                                  max_len=1024, device=local, synthetic=args.synthetic, weights_fp8=args.fp8, kv_fp8=args.kv_fp8)
    if args.lora_model:
        lang_model = PeftModelForCausalLM.from_pretrained(lang_model, args.lora_model, torch_dtype=dt, use_ram_optimized_load=False).half()
    lang_model.eval()
    if args.use_embs:
        images = synth.synth_images(len(dicoms), 448, seed=1000 + lo)
        lang_model.model.blip_embeddings.update(dump_embeddings(images, dicoms, dtype=args.dtype, device=local, synthetic=args.synthetic))

    all_preds, all_ids, preds_history, mean_lp = [], [], [], []
    if args.queue_rows > 0:
        # opt-in: every study's prompt waits in one queue; rows that finish early are refilled instead of decoding pads to the batch's longest report
        texts = []
        for d in dicoms:
            conv = new_conversation()
            conv.append_message(conv.roles[0], report_prompt("no finding"))
            conv.append_message(conv.roles[1], None)
            texts.append(conv.get_prompt())
        prompts = [tok.batch_encode_plus([t], return_tensors="pt", padding=True)["input_ids"][0].clone() for t in texts]
        seqs = lang_model.generate_many(prompts, dicom=dicoms if args.use_embs else None, max_new_tokens=args.max_new_tokens,
                                        rows=args.queue_rows, stage=queue_stage)
        preds = [tok.batch_decode(q.unsqueeze(0), skip_special_tokens=True)[0] for q in seqs]
        preds_history.extend(preds)
        all_preds.extend([q.split("ASSISTANT:")[1] if "ASSISTANT:" in q else q for q in preds])
        pad = torch.zeros(len(seqs), args.max_new_tokens, dtype=torch.int32, device=seqs[0].device)
        for i, (q, pr) in enumerate(zip(seqs, prompts)):
            gen = q[pr.numel():]
            pad[i, : gen.numel()] = gen.to(torch.int32)
        all_ids.append(pad)
    for s in range(0, len(dicoms) if args.queue_rows <= 0 else 0, args.batch_size):
        batch = dicoms[s: s + args.batch_size]
        texts = []
        for d in batch:
            conv = new_conversation()
            conv.append_message(conv.roles[0], report_prompt("no finding"))
            conv.append_message(conv.roles[1], None)
            texts.append(conv.get_prompt())
        input_ids = tok.batch_encode_plus(texts, return_tensors="pt", padding=True)["input_ids"]
        lang_model.enable_sampling = args.do_sample
        out = lang_model.generate(input_ids=input_ids, dicom=batch if args.use_embs else None, return_dict_in_generate=True,
                                  output_scores=True, max_new_tokens=args.max_new_tokens, num_beams=args.num_beams,
                                  repetition_penalty=args.repetition_penalty, no_repeat_ngram_size=args.no_repeat_ngram_size,
                                  min_new_tokens=args.min_new_tokens, do_sample=args.do_sample, temperature=args.temperature, seed=args.seed,
                                  output_logprobs=args.logprobs is not None, top_logprobs=args.logprobs or 0)
        if args.logprobs is not None:
            from radialog_amd.engine import mean_token_logprob
            mean_lp.extend(mean_token_logprob(out.sequences[:, input_ids.shape[1]:], lang_model.config.eos_token_id, out.token_logprobs).tolist())
        preds = tok.batch_decode(out.sequences, skip_special_tokens=True)
        preds_history.extend(preds)
        all_preds.extend([q.split("ASSISTANT:")[1] if "ASSISTANT:" in q else q for q in preds])
        gen = out.sequences[:, input_ids.shape[1]:]
        pad = torch.zeros(gen.shape[0], args.max_new_tokens, dtype=torch.int32, device=gen.device)
        pad[:, : gen.shape[1]] = gen.to(torch.int32)
        all_ids.append(pad)
    ids = torch.cat(all_ids, 0)
    if world > 1:
        counts = [shard_range(args.num_samples, world, r)[1] - shard_range(args.num_samples, world, r)[0] for r in range(world)]
        ids = allgather_ragged(ids, counts, world)
    if args.do_corr or args.do_cp_bin_qa or args.do_cp_all_qa:
        # downstream re-prompting (test.py:437-674): the whole conversation + one new USER turn; CheXbert labels are not available here,
        # so the correction prompts are driven by synthetic label disagreements of the same shape
        from radialog_amd import downstream as D
        from radialog_amd.chexpert_model import CHEXPERT_COLS
        import numpy as np
        rng = np.random.default_rng(0)
        dc = dicoms if args.use_embs else None
        if args.do_corr:
            P, L = rng.integers(0, 2, (len(dicoms), 14)), rng.integers(0, 2, (len(dicoms), 14))
            lk_stats = {}
            corr = D.run_correction(lang_model, tok, D.get_correction_prompts(list(preds_history), CHEXPERT_COLS, P, L), dc, args.num_beams,
                                    prompt_lookup=args.prompt_lookup, lookup_stats=lk_stats)
            res["corrected"] = corr
            if args.prompt_lookup:
                print(f"rank {rank}: prompt lookup accepted {lk_stats.get('accepted', 0)} / {lk_stats.get('drafted', 0)} drafted tokens in "
                      f"{lk_stats.get('passes', 0)} passes of {lk_stats.get('forwards', 0)} forwards")
            print(f"rank {rank}: {len(corr)} corrected reports; first: {corr[0][:80]!r}")
        if args.do_cp_bin_qa:
            yn = D.run_binary_qa(lang_model, tok, D.get_chexpert_prompts_bin(list(preds_history), CHEXPERT_COLS), CHEXPERT_COLS, dc)
            res["bin_qa"] = yn
            print(f"rank {rank}: binary QA label matrix {yn.shape}, positives {int(yn.sum())}")
        if args.do_cp_all_qa:
            oh = D.run_findings_qa(lang_model, tok, D.get_chexpert_prompts_all(list(preds_history), CHEXPERT_COLS), CHEXPERT_COLS, dc,
                                   batch_size=qa_batch, num_beams=args.num_beams)
            res["all_qa"] = oh
            print(f"rank {rank}: findings QA label matrix {oh.shape}, positives {int(oh.sum())}")
    if rank == 0:
        print(f"generated {ids.shape[0]} reports x {ids.shape[1]} token slots on {world} GPU(s); first: {all_preds[0][:120]!r}")
    if args.logprobs is not None:
        res["mean_logprob"] = mean_lp
        print(f"rank {rank}: mean token log-prob per report: " + " ".join(f"{v:.3f}" for v in mean_lp))
    res.update({"ids": ids.cpu(), "preds": all_preds, "dicoms": dicoms, "batch_size": args.batch_size})
    lang_model.close()
    return res


if __name__ == "__main__":
    main()
