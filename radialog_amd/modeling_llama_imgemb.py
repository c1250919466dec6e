"""`LlamaForCausalLM` with the RaDialog image splice, backed by librdx (mirror of the reference's call surface).

What demo.py:221-236,:287-301 and test.py:287-365 do with the reference class keeps working:
    lang_model = LlamaForCausalLM.from_pretrained(path_or_None, torch_dtype=torch.float16, device_map='auto')
    lang_model.base_model.img_proj_layer = nn.Linear(768, hidden)        # weights arrive with the adapter file
    lang_model = PeftModelForCausalLM.from_pretrained(lang_model, lora_dir, torch_dtype=torch.float16)    # same class name here
    out = lang_model.generate(input_ids=ids, dicom=[...] or None, use_img=bool, return_dict_in_generate=True,
                              output_scores=True, max_new_tokens=300)
    out.sequences  int64[B, T+n]   (prompt included; rows that finished early are padded with pad id 0)
    out.scores     tuple of n tensors [B, V]
The image embeddings reach `generate` the way the reference passes them (modeling_llama_imgemb.py:454-462,:571-579):
`use_img=True` -> torch.load("current_chat_img.pt"); `dicom=[...]` -> lookup in `self.model.blip_embeddings`
(pretraining/embs/*_embeddings_{train_all,test}.pkl when present). `qformer_embs=` can also be passed directly.
"""
from __future__ import annotations

import json
import numbers
import os
import pickle
from types import SimpleNamespace
from typing import List, Optional

import numpy as np
import torch

from .config import LlamaCfg, RaDialogCfg

EMB_TEST_PKL = "pretraining/embs/stage1_pt_instruct_blip_origlr_img448_embeddings_test.pkl"
EMB_TRAIN_PKL = "pretraining/embs/stage1_pt_instruct_blip_origlr_img448_embeddings_train_all.pkl"


class GenerateOutput(SimpleNamespace):
    """`.sequences`, `.scores` like transformers' GreedySearchDecoderOnlyOutput; with generate(output_logprobs=True) also `.token_logprobs` and `.top_logprobs`,
    with generate(prompt_lookup_num_tokens=N) `.lookup_stats` = {"passes", "drafted", "accepted", "forwards"}."""


class _BaseModel:
    """`lang_model.base_model` / `lang_model.model`: holds the side-channel dict and the attribute the callers inject."""

    def __init__(self, config):
        self.config = config
        self.img_proj_layer = None
        self.blip_embeddings = {}
        try:                                                       # modeling_llama_imgemb.py:454-459
            with open(EMB_TRAIN_PKL, "rb") as f:
                self.blip_embeddings = pickle.load(f)
        except Exception:
            self.blip_embeddings = {}
        if os.path.exists(EMB_TEST_PKL):                           # (:461 opens it unguarded; absent file = demo-only use)
            with open(EMB_TEST_PKL, "rb") as f:
                self.blip_embeddings.update(pickle.load(f))

    @property
    def device(self):
        return self._owner.device


class LlamaForCausalLM:
    def __init__(self, cfg: Optional[LlamaCfg] = None, dtype: str = "bf16", max_batch: int = 12, max_len: int = 1024,
                 lora: bool = True, device: int = 0, weights_fp8: bool = False, weights_w4: bool = False,
                 kv_fp8: bool = False):
        self.lcfg = cfg or LlamaCfg()
        self.config = SimpleNamespace(hidden_size=self.lcfg.hidden, vocab_size=self.lcfg.vocab,
                                      num_hidden_layers=self.lcfg.layers, pad_token_id=0, eos_token_id=2)
        self.model = _BaseModel(self.config)
        self.model._owner = self
        self.base_model = self.model
        self.dtype, self.lora = dtype, lora
        self.max_batch, self.max_len = max_batch, max_len
        # BASELINE configs[4]: the decoder's GEMM weights (and, in the prefill / from batch 3, the activations) in OCP e4m3 on the fp8 MFMA. LoRA stays
        # un-merged: the LoRA-B product is a model-dtype epilogue, the 16 LoRA-A rows are part of the QKV weight and quantised with it (their own
        # row scales; weights.py -- the oracle mirrors it, so what this costs on a trained adapter, whose A rows are small against a row's absmax, is
        # NOT measured here: no adapter file is reachable offline). No reference counterpart: `from_pretrained(..., weights_fp8=True)` is this build's extra kwarg
        self.weights_fp8 = bool(weights_fp8)
        # int4 group-quantised projections (RdxEngine(weights_w4=True), radialog_amd/w4.py): `from_pretrained(..., weights_w4=True)`, next to weights_fp8
        self.weights_w4 = bool(weights_w4)
        # the KV cache as e4m3 codes + one power-of-two exponent per row (RdxEngine(kv_fp8=True), radialog_amd/kv8.py): `from_pretrained(..., kv_fp8=True)`.
        # Greedy / sampled generate and scoring only: beams, reuse_prefix_kv and generate_many are not built on it
        self.kv_fp8 = bool(kv_fp8)
        self.device = torch.device("cuda", device)
        self._engine = None
        self._state = None            # reference-named tensors (dict, stored dtype); with _synthetic they overlay the random-init generator
        self._synthetic = False       # only from_pretrained(synthetic=True) turns the deterministic random-init weights on
        self.training = False

    # -- construction -------------------------------------------------------------------------------------------------------
    @classmethod
    def from_pretrained(cls, name_or_path=None, torch_dtype=torch.float16, device_map="auto", synthetic: bool = False, **kw):
        """`name_or_path` must be a local HF checkpoint directory (safetensors or pytorch_model*.bin shards). Anything else
        -- a hub id such as the reference's 'lmsys/vicuna-7b-v1.3' (there is no network here), a typo, None -- raises OSError
        like transformers does for an unreachable model, UNLESS the caller opts in to the deterministic random-init weights
        with `synthetic=True` (benchmarks and parity tests). Nothing falls back to random weights silently."""
        dt = "f16" if torch_dtype == torch.float16 else "bf16"
        kw.pop("use_ram_optimized_load", None)
        self = cls(cfg=kw.pop("cfg", None), dtype=dt, **kw)
        self._synthetic = bool(synthetic)
        if synthetic:
            self._state = None
        elif name_or_path and os.path.isdir(str(name_or_path)):
            self._state = _load_hf_dir(str(name_or_path))
            self.lora = False                      # a bare base model; PeftModelForCausalLM.from_pretrained / load_adapter adds LoRA
        else:
            raise OSError(f"{name_or_path!r} is not a local checkpoint directory (no network access; pass synthetic=True for the "
                          "deterministic random-init weights of the benchmarks)")
        return self

    def load_adapter(self, lora_dir: str):
        """peft adapter dir as finetune.py:121-150 writes it: `adapter_model.bin` = LoRA A/B of q_proj and v_proj under peft's key
        names (`base_model.model.model.layers.N.self_attn.q_proj.lora_A[.default].weight`) + `base_model.model.model.img_proj_layer.
        {weight,bias}`; `adapter_config.json` carries r, lora_alpha and target_modules (finetune.py:167-173: r=8, alpha=16,
        ["q_proj", "v_proj"]). The engine's fused LoRA epilogue supports exactly that family: anything else raises."""
        cfg_path = os.path.join(lora_dir, "adapter_config.json")
        if not os.path.isfile(cfg_path):
            raise OSError(f"{cfg_path} not found: not a peft adapter directory")
        with open(cfg_path) as f:
            acfg = json.load(f)
        r, alpha = int(acfg.get("r", 8)), float(acfg.get("lora_alpha", 16))
        targets = set(acfg.get("target_modules") or [])
        if targets != {"q_proj", "v_proj"}:
            raise ValueError(f"adapter targets {sorted(targets)}: the fused LoRA path covers q_proj and v_proj (finetune.py:171)")
        if r != 8:
            raise ValueError(f"adapter rank r={r}: the fused LoRA epilogue is built for r=8 (finetune.py:168)")
        if float(acfg.get("lora_dropout", 0.0)) and not acfg.get("inference_mode", True):
            raise ValueError("adapter_config.json is not in inference mode")
        bin_path = os.path.join(lora_dir, "adapter_model.bin")
        if not os.path.isfile(bin_path):
            raise OSError(f"{bin_path} not found")
        sd = torch.load(bin_path, map_location="cpu")
        self.lcfg = LlamaCfg(**{**self.lcfg.__dict__, "lora_r": r, "lora_alpha": alpha})
        if self._state is None and not self._synthetic:
            raise RuntimeError("load_adapter: no base weights loaded (LlamaForCausalLM.from_pretrained first)")
        self._state = {} if self._state is None else self._state
        self._adapter_keys = set()
        for k, v in sd.items():
            k = k.replace("base_model.model.", "", 1).replace(".lora_A.default.", ".lora_A.").replace(".lora_B.default.", ".lora_B.")
            self._state[k] = v.float()
            self._adapter_keys.add(k)
        self.lora = True
        if self._engine is not None:               # an engine built before the adapter arrived: release its weight replica and KV cache
            self._engine.close()
        self._engine = None
        return self


    def resize_token_embeddings(self, n):                          # test.py:297 (adds the <IMG> row)
        self.lcfg = LlamaCfg(**{**self.lcfg.__dict__, "vocab": n})
        self.config.vocab_size = n
        return self

    def half(self):
        return self

    def eval(self):
        self.training = False
        return self

    def cuda(self):
        return self

    def close(self):
        """Release the engine's weight replica and KV cache (no reference counterpart: torch frees on garbage collection; the
        entry-point tests run several models in one process)."""
        if self._engine is not None:
            self._engine.close()
        self._engine = None

    def _ensure_engine(self):
        if self._engine is not None:
            return
        from .engine import RdxEngine, synth_getter
        cfg = RaDialogCfg(llama=self.lcfg)
        eng = RdxEngine(cfg, dtype=self.dtype, device=self.device.index or 0, max_batch=self.max_batch, max_len=self.max_len,
                        lora=self.lora, vision=False, llama=True, weights_fp8=self.weights_fp8, weights_w4=self.weights_w4, kv_fp8=self.kv_fp8)
        if self._state is None and not self._synthetic:
            eng.close()
            raise RuntimeError("LlamaForCausalLM has no weights: build it with from_pretrained(local_dir) or from_pretrained(synthetic=True)")
        if self._synthetic:
            base, st = synth_getter(cfg, eng.device, lora=self.lora), (self._state or {})
            get = lambda name: st[name].to(eng.device) if name in st else base(name)          # noqa: E731
        else:
            st, V = self._state, self.lcfg.vocab
            need = ["model.embed_tokens.weight", "lm_head.weight", "model.norm.weight", "model.img_proj_layer.weight",
                    "model.img_proj_layer.bias"]
            if self.lora:
                need += [f"model.layers.{l}.self_attn.{m}.lora_{ab}.weight" for l in (0, self.lcfg.layers - 1)
                         for m in ("q_proj", "v_proj") for ab in "AB"]
            missing = [k for k in need if k not in st]
            if missing:
                eng.close()
                raise KeyError(f"checkpoint lacks {missing}: `img_proj_layer` and the LoRA matrices arrive with the adapter "
                               "(PeftModelForCausalLM.from_pretrained(lang_model, adapter_dir), demo.py:229-234)")

            def get(name):
                t = st[name].to(eng.device)
                if name in ("model.embed_tokens.weight", "lm_head.weight") and t.shape[0] < V:   # resize_token_embeddings
                    # transformers 4.28.1 `_get_resized_embeddings` / `_get_resized_lm_head` -> `_init_weights`: the new rows are drawn
                    # from normal(0, initializer_range = 0.02) (modeling_llama_imgemb.py:349-358). Drawn from a fixed-seed generator
                    # here so that two loads agree; the <IMG> embedding row is never read (the splice replaces it), its lm_head row
                    # gets a near-zero random logit like in the reference.
                    g = torch.Generator().manual_seed(32000 + (0 if name.startswith("model.") else 1))
                    new = torch.randn(V - t.shape[0], t.shape[1], generator=g) * 0.02
                    t = torch.cat([t, new.to(t)], 0)
                return t
        eng.load_weights(get, vision=False, llama=True)
        self._engine = eng

    # -- generation -------------------------------------------------------------------------------------------------------------
    def _image_embs(self, B, dicom, use_img, qformer_embs):
        if qformer_embs is not None:
            return qformer_embs
        if use_img:                                                # modeling_llama_imgemb.py:576
            e = torch.load("current_chat_img.pt")
            return e.expand(B, -1, -1) if e.shape[0] == 1 and B > 1 else e
        if dicom is not None:                                      # :579 (KeyError for an unknown id, like the reference)
            return torch.tensor(np.array([self.model.blip_embeddings[d] for d in dicom]))
        return None

    @torch.no_grad()
    def generate(self, input_ids: torch.Tensor = None, dicom: Optional[List[str]] = None, use_img: bool = False,
                 return_dict_in_generate: bool = False, output_scores: bool = False, max_new_tokens: int = 20,
                 attention_mask: Optional[torch.Tensor] = None, num_beams: int = 1, do_sample: bool = False,
                 qformer_embs: Optional[torch.Tensor] = None, eos_token_id: Optional[int] = None,
                 pad_token_id: Optional[int] = None, length_penalty: float = 1.0, early_stopping: bool = False,
                 repetition_penalty: float = 1.0, no_repeat_ngram_size: int = 0, min_new_tokens: int = 0,
                 temperature: float = 1.0, top_k: int = 50, top_p: float = 1.0, seed: Optional[int] = None,
                 output_logprobs: bool = False, top_logprobs: int = 0, prompt_lookup_num_tokens: Optional[int] = None,
                 max_matching_ngram_size: Optional[int] = None, lookup_corpus=None, **_unused):
        """prompt_lookup_num_tokens=N (transformers' name; None or 0 = off) with max_matching_ngram_size=M (default 3) and lookup_corpus= (token ids of a
        document the answer is expected to quote): batch-1 greedy search whose forwards verify up to N tokens copied from the sequence itself
        (engine.generate_lookup; include/rdx.h rdx_generate_lookup). The tokens are greedy under the returned scores, which are the model's within the parity
        bar; they are NOT guaranteed to equal a plain call's (a verify pass and a plain step round differently). The output gains `.lookup_stats`.
        ValueError for what the library refuses: batch > 1, num_beams > 1, do_sample, active logits rules, output_logprobs, kv_fp8, fp8 weights.
        output_logprobs=True (with return_dict_in_generate; no reference counterpart): the output gains `.token_logprobs` float32 [B, n], the log-prob of
        every generated token under the scores row it was chosen from (what compute_transition_scores(sequences, scores, normalize_logits=True) gives, without
        the [n][B][V] scores), and `.top_logprobs` = (ids int32 [B, n, k], logprobs float32 [B, n, k]), the k = top_logprobs (0 .. 8) likeliest tokens of
        each step; entries behind a row's EOS read (0.0, -1, 0.0). Greedy search and sampling only: num_beams > 1 raises ValueError.
        do_sample=True on a model with `enable_sampling = True` set on it (the way `reuse_prefix_kv` is set): transformers' `sample` with its
        temperature / top_k / top_p warpers (top_k=50 is GenerationConfig's default), drawn from a counter RNG: `seed`, or, when None, 63 bits
        from torch's default CPU generator, so that torch.manual_seed(s) in front of two calls makes them equal. A model without the switch
        refuses do_sample=True with NotImplementedError, as it always has: every reference call site decodes deterministically, and a caller
        that relied on that is not given a stochastic result unasked. With do_sample=False the three warper arguments are ignored, as
        transformers ignores them in greedy search."""
        if do_sample and not getattr(self, "enable_sampling", False):
            raise NotImplementedError("sampling is off on this model (every reference call site decodes deterministically): set "
                                      "`model.enable_sampling = True` to let generate(do_sample=True) sample")
        if num_beams < 1:
            raise ValueError("`num_beams` has to be an integer strictly greater than 0")
        from .engine import LogitsRules, check_top_logprobs
        if not output_logprobs and top_logprobs:
            raise ValueError("top_logprobs needs output_logprobs=True")
        logprobs = check_top_logprobs(top_logprobs, "top_logprobs (generation logprobs)") if output_logprobs else None
        if logprobs is not None and num_beams > 1:
            raise ValueError("output_logprobs / top_logprobs apply to num_beams=1 only: per-step logprobs of beams are not built (beam search returns "
                             "sequences_scores)")
        sampling = _sampling_of(do_sample, num_beams, temperature, top_k, top_p, seed, _unused)        # ValueError before an engine exists
        # transformers builds RepetitionPenaltyLogitsProcessor, which takes a float only, when the value differs from 1.0: 1 (int) is "off" there too
        if not isinstance(repetition_penalty, float) and not (isinstance(repetition_penalty, numbers.Real) and repetition_penalty == 1):
            raise ValueError(f"`repetition_penalty` has to be a strictly positive float, but is {repetition_penalty}")
        rules = LogitsRules(repetition_penalty, no_repeat_ngram_size, min_new_tokens)       # ValueError on what transformers refuses
        if rules.active and num_beams > 1:
            raise ValueError("repetition_penalty / no_repeat_ngram_size / min_new_tokens apply to greedy search only (num_beams=1): beam search "
                             "under logits rules is not built")
        if self.kv_fp8 and num_beams > 1:
            raise ValueError("kv_fp8: beam search is not built on the fp8 KV cache (the beam reorder moves model-dtype rows); num_beams=1 only")
        if self.kv_fp8 and getattr(self, "reuse_prefix_kv", False):
            raise ValueError("kv_fp8: reuse_prefix_kv is not built on the fp8 KV cache (the kept prefix is not held in the model dtype)")
        if input_ids.dim() != 2:
            raise ValueError("You have to specify decoder_input_ids of shape [batch, seq]")
        B, T = input_ids.shape
        lookup = self._lookup_of(prompt_lookup_num_tokens, max_matching_ngram_size, lookup_corpus, B, num_beams, do_sample, rules.active, logprobs is not None)
        eos = self.config.eos_token_id if eos_token_id is None else eos_token_id
        pad = self.config.pad_token_id if pad_token_id is None else pad_token_id
        embs = self._image_embs(B, dicom, use_img, qformer_embs)
        if embs is not None and tuple(embs.shape) != (B, 32, self.lcfg.qformer_dim):
            raise ValueError(f"image embeddings should be of size {(B, 32, self.lcfg.qformer_dim)}, but are {tuple(embs.shape)}")
        self._ensure_engine()
        if num_beams > 1:
            return self._beam_generate(input_ids, embs, num_beams, max_new_tokens, eos, pad, attention_mask, length_penalty,
                                       early_stopping, return_dict_in_generate, output_scores)
        # multi-turn chats (demo.py:277-305 re-sends the whole conversation every turn): with `reuse_prefix_kv` set on the model
        # the KV rows of the token prefix shared with the previous call are kept and only the new turn is prefilled (not under an
        # active logits rule: the token history is not carried across calls, the full prompt is prefilled)
        if lookup is not None:
            toks, scores, n, stats, _trace = self._engine.generate_lookup(input_ids, embs, max_new=max_new_tokens, eos_id=eos, pad_id=pad, mask=attention_mask,
                                                                          lookup=lookup, corpus=lookup_corpus, output_scores=output_scores)
            seq = torch.cat([input_ids.to(toks.device), toks[:, :n].to(torch.int64)], dim=1)
            if not return_dict_in_generate:
                return seq
            return GenerateOutput(sequences=seq, scores=tuple(scores[i].clone() for i in range(n)) if output_scores else None, lookup_stats=stats)
        lp_kw = {} if logprobs is None else {"logprobs": logprobs}
        toks, scores, n, *lp = self._engine.generate(input_ids, embs, max_new=max_new_tokens, eos_id=eos, pad_id=pad,
                                                     mask=attention_mask, output_scores=output_scores,
                                                     reuse_prefix=bool(getattr(self, "reuse_prefix_kv", False)) and attention_mask is None,
                                                     logits_rules=rules, sampling=sampling, **lp_kw)
        toks = toks[:, :n].to(torch.int64)
        # HF stops as soon as every row has emitted EOS; the engine polls every 4th step (api_llama.hip decode_loop), so trim the all-pad tail
        if eos >= 0 and n > 0:
            done = (toks == eos).cumsum(1).clamp(max=1)
            if bool(done[:, -1].all()):
                n = int(done.argmax(1).max()) + 1
                toks = toks[:, :n]
        seq = torch.cat([input_ids.to(toks.device), toks], dim=1)
        if not return_dict_in_generate:
            return seq
        # fresh tensors like HF's: the engine reuses its score buffer on the next call
        sc = tuple(scores[i].clone() for i in range(n)) if output_scores else None
        if logprobs is None:
            return GenerateOutput(sequences=seq, scores=sc)
        chosen, top_ids, top_lp = lp[0]
        return GenerateOutput(sequences=seq, scores=sc, token_logprobs=chosen[:, :n], top_logprobs=(top_ids[:, :n], top_lp[:, :n]))

    def _lookup_of(self, num_tokens, ngram, corpus, B, num_beams, do_sample, rules_active, logprobs):
        """generate()'s prompt-lookup arguments as an engine.Lookup, or None when they are neutral (the existing path). ValueError, before an engine
        exists, for what rdx_generate_lookup refuses."""
        from .engine import Lookup
        if num_tokens is None or (not isinstance(num_tokens, bool) and num_tokens == 0):
            if ngram is not None or corpus is not None:
                raise ValueError("max_matching_ngram_size / lookup_corpus need prompt_lookup_num_tokens")
            return None
        lookup = Lookup(draft_len=num_tokens, ngram_max=3 if ngram is None else ngram, ngram_min=1)        # ValueError on values out of range
        why = ("batch > 1 (prompt-lookup decoding is built for batch 1)" if B != 1 else "num_beams > 1 (beams are not built)" if num_beams > 1 else
               "do_sample (speculative sampling is not built)" if do_sample else
               "repetition_penalty / no_repeat_ngram_size / min_new_tokens (logits rules are not built)" if rules_active else
               "output_logprobs (generation logprobs are not built)" if logprobs else
               "kv_fp8 (the kept prefix is not held in the model dtype)" if self.kv_fp8 else
               "weights_fp8 (the all-row lm_head of a verify pass has no fp8 convention)" if self.weights_fp8 else None)
        if why:
            raise ValueError(f"prompt_lookup_num_tokens does not go with {why}")
        return lookup

    @torch.no_grad()
    def generate_many(self, input_ids: List[torch.Tensor], dicom: Optional[List[str]] = None, qformer_embs: Optional[torch.Tensor] = None,
                      max_new_tokens=20, rows: Optional[int] = None, stage: Optional[int] = None, num_beams: int = 1, do_sample: bool = False,
                      repetition_penalty: float = 1.0, no_repeat_ngram_size: int = 0, min_new_tokens: int = 0,
                      eos_token_id: Optional[int] = None, pad_token_id: Optional[int] = None, output_logprobs: bool = False,
                      top_logprobs: int = 0) -> List[torch.Tensor]:
        """Greedy generation of many prompts of different lengths through a queue (no reference counterpart; RdxEngine.generate_queue): `rows` rows decode
        at a time (default: max_batch less the staging rows) and a row whose report has ended takes the next waiting prompt. input_ids: a list of 1-D
        prompts, unpadded; dicom / qformer_embs ([N, 32, qformer_dim]) as in generate; max_new_tokens: one int or one per prompt. Returns one 1-D int64
        sequence per prompt, in order: the prompt, then what was generated up to and including EOS or up to the prompt's max_new_tokens.
        Greedy search only: num_beams > 1, do_sample, active logits rules and output_logprobs / top_logprobs raise ValueError."""
        from .engine import LogitsRules, QUEUE_STAGE
        if self.kv_fp8:
            raise ValueError("kv_fp8: generate_many is not built on the fp8 KV cache (a row session moves model-dtype cache rows)")
        if num_beams != 1:
            raise ValueError("generate_many runs greedy search only (num_beams=1): beams in a row session are not built")
        if do_sample:
            raise ValueError("generate_many runs greedy search only: sampling in a row session is not built")
        if output_logprobs or top_logprobs:
            raise ValueError("generate_many: generation logprobs in a row session are not built (a moved row's entries would have to move with it)")
        if LogitsRules(repetition_penalty, no_repeat_ngram_size, min_new_tokens).active:
            raise ValueError("generate_many: repetition_penalty / no_repeat_ngram_size / min_new_tokens in a row session are not built")
        prompts = [torch.as_tensor(p).reshape(-1) for p in input_ids]
        N = len(prompts)
        caps = [int(max_new_tokens)] * N if isinstance(max_new_tokens, numbers.Integral) else [int(m) for m in max_new_tokens]
        if len(caps) != N:
            raise ValueError(f"max_new_tokens lists {len(caps)} values for {N} prompts")
        eos = self.config.eos_token_id if eos_token_id is None else eos_token_id
        pad = self.config.pad_token_id if pad_token_id is None else pad_token_id
        embs = self._image_embs(N, dicom, False, qformer_embs) if N else None
        if embs is not None and tuple(embs.shape) != (N, 32, self.lcfg.qformer_dim):
            raise ValueError(f"image embeddings should be of size {(N, 32, self.lcfg.qformer_dim)}, but are {tuple(embs.shape)}")
        if stage is None:
            stage = max(1, min(QUEUE_STAGE, self.max_batch // 2))
        if rows is None:
            rows = self.max_batch - stage
        if rows < 1 or rows + stage > self.max_batch:
            raise ValueError(f"rows ({rows}) + stage ({stage}) must fit max_batch {self.max_batch} of this model")
        self._ensure_engine()
        reqs = [(prompts[i], None if embs is None else embs[i], caps[i]) for i in range(N)]
        outs = self._engine.generate_queue(reqs, rows=rows, stage=stage, eos_id=eos, pad_id=pad)
        return [torch.cat([prompts[i].to(torch.int64).cpu(), outs[i]]).to(self.device) for i in range(N)]


    # -- scoring given tokens ------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def forward(self, input_ids: torch.Tensor = None, attention_mask: Optional[torch.Tensor] = None, labels: Optional[torch.Tensor] = None,
                dicom: Optional[List[str]] = None, use_img: bool = False, qformer_embs: Optional[torch.Tensor] = None,
                return_dict: bool = True, return_logits: bool = True, past_key_values=None, inputs_embeds=None, **_unused):
        """The reference's forward(input_ids, attention_mask, labels=, dicom=, use_img=) (modeling_llama_imgemb.py:705-793) from one scoring pass
        (RdxEngine.score): `.logits` [B, T, V] of every position and `.loss`, the shifted cross-entropy -- logits[:, :-1] against labels[:, 1:], the
        mean of -log p over the labels != -100 (summed on the host in float64, returned as an fp32 scalar; NaN when nothing is counted, as
        CrossEntropyLoss gives). `.token_logprobs` [B, T] float32 (no reference counterpart): log p(labels[b, t] | input_ids[b, :t]) where
        labels[b, t] != -100 and t >= 1, 0 elsewhere. attention_mask=None attends every position, as the reference does. labels=None scores
        nothing and returns the logits. return_logits=False (no reference counterpart) is the cheap path for the loss alone: only the scored
        rows pass the lm_head and `.logits` is None. return_dict=False: the reference's tuple, (loss, logits) or (logits,).
        Not built: past_key_values and inputs_embeds (ValueError)."""
        if past_key_values is not None or inputs_embeds is not None:
            raise ValueError("forward(past_key_values=) / forward(inputs_embeds=) are not built: pass the whole sequence as input_ids")
        if input_ids is None or input_ids.dim() != 2:
            raise ValueError("You have to specify input_ids of shape [batch, seq]")
        B, T = input_ids.shape
        lab = None
        if labels is not None:
            lab = torch.as_tensor(labels).detach().to("cpu", torch.int64)
            if tuple(lab.shape) != (B, T):
                raise ValueError(f"labels of shape {tuple(lab.shape)} do not match input_ids of shape {(B, T)}")
            bad = (lab != -100) & ((lab < 0) | (lab >= self.lcfg.vocab))
            if bool(bad.any()):
                raise ValueError(f"label {int(lab[bad][0])} is outside the vocabulary [0, {self.lcfg.vocab}) and is not -100")
        if attention_mask is not None and tuple(attention_mask.shape) != (B, T):
            raise ValueError(f"attention_mask of shape {tuple(attention_mask.shape)} does not match input_ids of shape {(B, T)}")
        if lab is None and not return_logits:
            raise ValueError("forward(labels=None, return_logits=False) asks for nothing")
        embs = self._image_embs(B, dicom, use_img, qformer_embs)
        if embs is not None and tuple(embs.shape) != (B, 32, self.lcfg.qformer_dim):
            raise ValueError(f"image embeddings should be of size {(B, 32, self.lcfg.qformer_dim)}, but are {tuple(embs.shape)}")
        self._ensure_engine()
        mask = torch.ones(B, T, dtype=torch.int32) if attention_mask is None else attention_mask
        # the shift: position t is scored against labels[t] from the logits of t - 1; position 0 has no predecessor (the engine ignores labels[:, 0])
        eng_labels = torch.full((B, T), -100, dtype=torch.int32) if lab is None else lab.to(torch.int32)
        logprob, _, logits = self._engine.score(input_ids, embs, eng_labels, mask=mask, want_top1=False, want_logits=bool(return_logits))
        loss = None
        if lab is not None:
            counted = lab[:, 1:] != -100
            n = int(counted.sum())
            total = float(logprob[:, 1:].double().cpu()[counted].sum())
            loss = torch.tensor(-total / n if n else float("nan"), dtype=torch.float32, device=logprob.device)
        if not return_dict:
            return (logits,) if loss is None else (loss, logits)
        return CausalLMOutput(loss=loss, logits=logits, token_logprobs=logprob if lab is not None else None)

    __call__ = forward


class CausalLMOutput(SimpleNamespace):
    """`.loss`, `.logits` like transformers' CausalLMOutputWithPast; `.token_logprobs` on top."""


def _sampling_of(do_sample, num_beams, temperature, top_k, top_p, seed, other):
    """generate()'s sampling arguments as an engine.Sampling, or None for do_sample=False. The checks are those of transformers 4.28.1's
    _get_logits_warper and its warper classes: a value that switches a warper off there (temperature 1, top_k 0, top_p 1) does so here."""
    if not do_sample:
        return None
    from .engine import Sampling
    if num_beams > 1:
        raise ValueError("do_sample=True applies to num_beams=1 only: beam-sample is not built")
    for name, neutral in (("typical_p", 1.0), ("epsilon_cutoff", 0.0), ("eta_cutoff", 0.0)):
        v = other.get(name)
        if v is not None and v != neutral:
            raise ValueError(f"`{name}`={v}: this warper is not built (only temperature, top_k and top_p are)")
    if not isinstance(temperature, float) and not (isinstance(temperature, numbers.Real) and not isinstance(temperature, bool) and temperature == 1):
        raise ValueError(f"`temperature` has to be a strictly positive float, but is {temperature}")
    if not temperature > 0:
        raise ValueError(f"`temperature` has to be a strictly positive float, but is {temperature}")
    if top_k is None:
        top_k = 0
    if isinstance(top_k, bool) or not isinstance(top_k, numbers.Integral) or top_k < 0:
        raise ValueError(f"`top_k` has to be a strictly positive integer, but is {top_k}")
    top_p = 1.0 if top_p is None else float(top_p)
    if top_p < 0 or top_p > 1.0 or top_p != top_p:
        raise ValueError(f"`top_p` has to be a float > 0 and < 1, but is {top_p}")
    if top_p == 0.0:
        top_p = 2.0 ** -126             # transformers keeps the one top token; here: the maximum's value group (the library wants p > 0)
    if seed is None:
        seed = int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64))      # the default CPU generator: torch.manual_seed governs it
    return Sampling(float(temperature), int(top_k), top_p, seed)         # ValueError for a seed outside [0, 2^64)


def _beam_generate(self, input_ids, embs, num_beams, max_new_tokens, eos, pad, attention_mask, length_penalty, early_stopping,
                   return_dict_in_generate, output_scores):
    """Tail of BeamSearchScorer.finalize (transformers 4.28.1): one hypothesis per prompt, EOS appended where a hypothesis ended
    before the longest one, rows padded to a common length min(longest + 1, T + max_new_tokens)."""
    if input_ids.shape[0] * num_beams > self.max_batch:
        raise ValueError(f"batch {input_ids.shape[0]} x num_beams {num_beams} exceeds max_batch {self.max_batch} of this model")
    toks, lens, seq_scores, step_scores, n = self._engine.beam_search(input_ids, embs, num_beams, max_new_tokens, eos_id=eos, pad_id=pad,
                                                                      mask=attention_mask, length_penalty=length_penalty,
                                                                      early_stopping=early_stopping, output_scores=output_scores)
    B, T = input_ids.shape
    sent_max = min(int(lens.max()) + 1, max_new_tokens)
    gen = torch.full((B, sent_max), pad, dtype=torch.int64)
    for b in range(B):
        L = int(lens[b])
        gen[b, :L] = toks[b, :L].to(torch.int64)
        if L < sent_max and eos >= 0:
            gen[b, L] = eos
    seq = torch.cat([input_ids.to(torch.int64).cpu(), gen], dim=1).to(self.device)
    if not return_dict_in_generate:
        return seq
    sc = tuple(step_scores[i].clone() for i in range(step_scores.shape[0])) if output_scores else None
    return GenerateOutput(sequences=seq, scores=sc, sequences_scores=seq_scores.to(self.device))


LlamaForCausalLM._beam_generate = _beam_generate


class PeftModelForCausalLM:
    """`PeftModelForCausalLM.from_pretrained(lang_model, adapter_dir, torch_dtype=torch.float16[, use_ram_optimized_load=False])`
    exactly as demo.py:232-234 / test.py:301 call it (peft@e536616): loads the adapter into `lang_model` and returns an object
    with the wrapped model's surface (`generate`, `eval`, `half`, `base_model.model` = the LlamaForCausalLM)."""

    def __init__(self, model: "LlamaForCausalLM"):
        self.base_model = SimpleNamespace(model=model)

    @classmethod
    def from_pretrained(cls, model: "LlamaForCausalLM", model_id: str, torch_dtype=None, **_kw):
        model.load_adapter(str(model_id))
        return cls(model)

    def __getattr__(self, name):
        return getattr(self.base_model.model, name)

    def __setattr__(self, name, value):
        # peft's wrapper is an nn.Module whose attributes callers set on the wrapper (demo.py sets `reuse_prefix_kv`); everything but the
        # wrapper's own `base_model` belongs to the wrapped LlamaForCausalLM, where generate() reads it
        if name == "base_model":
            object.__setattr__(self, name, value)
        else:
            setattr(self.base_model.model, name, value)

    def half(self):
        return self

    def eval(self):
        self.base_model.model.eval()
        return self

    def generate(self, **kw):
        return self.base_model.model.generate(**kw)

    def forward(self, *a, **kw):
        return self.base_model.model.forward(*a, **kw)

    def __call__(self, *a, **kw):
        return self.base_model.model.forward(*a, **kw)


def _load_hf_dir(path: str):
    """Read a local HF checkpoint directory (safetensors or .bin shards) into reference-named tensors IN THE STORED DTYPE (Vicuna-7B:
    fp16, 13.5 GB): nothing is inflated to fp32 on the host -- the engine widens tensor by tensor on the device (rdx_set_weight_typed)."""
    import glob
    out = {}
    files = sorted(glob.glob(os.path.join(path, "*.safetensors")))
    if files:
        from safetensors.torch import load_file
        for f in files:
            out.update(load_file(f))
    else:
        for f in sorted(glob.glob(os.path.join(path, "pytorch_model*.bin"))):
            out.update(torch.load(f, map_location="cpu"))
    if not out:
        raise OSError(f"no weights found under {path}")
    return out
