"""RdxEngine: the thin Python owner of one librdx context (one per process and GPU).

PyTorch-ROCm is used only as the tensor container (device memory, dtype views) and for `torch.distributed`;
all arithmetic of the hot path runs in librdx's HIP kernels. There is no eager/CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import math
import numbers
from dataclasses import dataclass
from typing import Callable, Dict, Optional

import torch

from . import _lib
from ._lib import RdxConfig, check
from .config import RaDialogCfg
from . import weights as W

_TORCH_DT = {"f16": torch.float16, "bf16": torch.bfloat16}
_RDX_DT = {"f16": _lib.RDX_DTYPE_F16, "bf16": _lib.RDX_DTYPE_BF16}


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


@dataclass(frozen=True)
class LogitsRules:
    """The greedy search's logits rules (rdx_logits_rules, include/rdx.h): transformers' `repetition_penalty`, `no_repeat_ngram_size` and
    `min_new_tokens`, applied in that order before the argmax. The defaults are neutral (= off). Raises ValueError on values HF refuses."""
    repetition_penalty: float = 1.0
    no_repeat_ngram_size: int = 0
    min_new_tokens: int = 0

    def __post_init__(self):
        p, n, m = self.repetition_penalty, self.no_repeat_ngram_size, self.min_new_tokens
        if isinstance(p, bool) or not isinstance(p, numbers.Real) or not math.isfinite(p) or not p > 0:
            raise ValueError(f"`repetition_penalty` has to be a strictly positive float, but is {p}")
        if isinstance(n, bool) or not isinstance(n, numbers.Integral) or n < 0:
            raise ValueError(f"`no_repeat_ngram_size` has to be a non-negative integer, but is {n}")
        if isinstance(m, bool) or not isinstance(m, numbers.Integral) or m < 0:
            raise ValueError(f"`min_new_tokens` has to be a non-negative integer, but is {m}")

    @property
    def active(self) -> bool:
        return float(self.repetition_penalty) != 1.0 or self.no_repeat_ngram_size != 0 or self.min_new_tokens != 0

    @classmethod
    def of(cls, rules) -> "LogitsRules":
        """None, a LogitsRules or a (repetition_penalty, no_repeat_ngram_size, min_new_tokens) tuple."""
        if rules is None:
            return cls()
        return rules if isinstance(rules, cls) else cls(*rules)


@dataclass(frozen=True)
class Sampling:
    """Sampled decoding (rdx_sampling, include/rdx.h): transformers' `temperature`, `top_k` and `top_p` warpers in that order, then one draw per row and
    step from a counter RNG keyed by `seed`. Neutral values: temperature 1.0, top_k 0, top_p 1.0. Raises ValueError on what the library refuses."""
    temperature: float = 1.0
    top_k: int = 0
    top_p: float = 1.0
    seed: int = 0

    def __post_init__(self):
        t, k, p, s = self.temperature, self.top_k, self.top_p, self.seed
        if isinstance(t, bool) or not isinstance(t, numbers.Real) or not math.isfinite(t) or not t > 0:
            raise ValueError(f"`temperature` has to be a strictly positive float, but is {t}")
        if isinstance(k, bool) or not isinstance(k, numbers.Integral) or k < 0:
            raise ValueError(f"`top_k` has to be a non-negative integer (0 = off), but is {k}")
        if isinstance(p, bool) or not isinstance(p, numbers.Real) or not (0 < p <= 1.0):
            raise ValueError(f"`top_p` has to be a float > 0 and <= 1 (1.0 = off), but is {p}")
        if isinstance(s, bool) or not isinstance(s, numbers.Integral) or not (0 <= s < 1 << 64):
            raise ValueError(f"`seed` has to be an integer in [0, 2^64), but is {s}")

    @classmethod
    def of(cls, sampling) -> Optional["Sampling"]:
        """None (greedy), a Sampling or a (temperature, top_k, top_p, seed) tuple."""
        if sampling is None or isinstance(sampling, cls):
            return sampling
        return cls(*sampling)


@dataclass(frozen=True)
class Lookup:
    """Prompt-lookup decoding (rdx_lookup, include/rdx.h): drafts of up to `draft_len` tokens (1 .. 15) that followed the most recent earlier occurrence of the
    sequence's last n tokens, n from `ngram_max` (<= 8) down to `ngram_min` (>= 1). Raises ValueError on what the library refuses."""
    draft_len: int = 8
    ngram_max: int = 3
    ngram_min: int = 1

    def __post_init__(self):
        for name in ("draft_len", "ngram_max", "ngram_min"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, numbers.Integral):
                raise ValueError(f"`{name}` has to be an integer, but is {v!r}")
        if not 1 <= self.draft_len <= 15:
            raise ValueError(f"`draft_len` has to be in 1 .. 15, but is {self.draft_len}")
        if not 1 <= self.ngram_max <= 8:
            raise ValueError(f"`ngram_max` has to be in 1 .. 8, but is {self.ngram_max}")
        if not 1 <= self.ngram_min <= self.ngram_max:
            raise ValueError(f"`ngram_min` has to be in 1 .. ngram_max ({self.ngram_max}), but is {self.ngram_min}")

    @classmethod
    def of(cls, lookup) -> "Lookup":
        """A Lookup, an int (the draft length) or a (draft_len, ngram_max, ngram_min) tuple."""
        if isinstance(lookup, cls):
            return lookup
        if isinstance(lookup, numbers.Integral) and not isinstance(lookup, bool):
            return cls(draft_len=int(lookup))
        return cls(*lookup)


def mask_logprobs_after_eos(tokens, eos_id, chosen, top_ids, top_lp):
    """What the Python layer returns for generation log-probs: everything BEHIND a row's first EOS (the pad tokens the step's tail writes for a finished
    row) reads (0.0, -1, 0.0); the EOS entry itself stays. tokens int [B, n], chosen [B, n], top_ids / top_lp [B, n, k]. New tensors; eos_id < 0: copies."""
    tokens = torch.as_tensor(tokens)
    B, n = chosen.shape
    done = torch.zeros(B, n, dtype=torch.bool)
    if eos_id is not None and eos_id >= 0 and n > 1:
        hit = (tokens[:, :n].cpu() == eos_id).to(torch.int64)
        done[:, 1:] = hit.cumsum(dim=1)[:, :-1] > 0
    chosen, top_ids, top_lp = chosen.clone(), top_ids.clone(), top_lp.clone()
    chosen[done] = 0.0
    top_ids[done] = -1
    top_lp[done] = 0.0
    return chosen, top_ids, top_lp


def mean_token_logprob(tokens, eos_id, chosen):
    """float64 [B]: the mean log-prob of each row's generated tokens up to and including its first EOS (all n without one): a report's confidence."""
    tokens = torch.as_tensor(tokens)
    B, n = chosen.shape
    live = torch.ones(B, n, dtype=torch.bool)
    if eos_id is not None and eos_id >= 0 and n > 1:
        live[:, 1:] = (tokens[:, :n].cpu() == eos_id).to(torch.int64).cumsum(dim=1)[:, :-1] == 0
    c = torch.where(live, chosen.double(), torch.zeros(B, n, dtype=torch.float64))
    return c.sum(dim=1) / live.sum(dim=1).clamp(min=1)


def check_top_logprobs(n, what="logprobs"):
    """None (off) or an int in 0 .. RDX_MAX_TOP_LOGPROBS; anything else is a ValueError naming `what`."""
    if n is None:
        return None
    if isinstance(n, bool) or not isinstance(n, int) or not 0 <= n <= _lib.RDX_MAX_TOP_LOGPROBS:
        raise ValueError(f"{what} must be None or an int in 0 .. {_lib.RDX_MAX_TOP_LOGPROBS} (the number of top alternatives per step), got {n!r}")
    return n


class RdxEngine:
    def __init__(self, cfg: RaDialogCfg, dtype: str = "bf16", device: int = 0, max_batch: int = 1, max_len: int = 512,
                 lora: bool = True, vision: bool = True, llama: bool = True, classifier: bool = False,
                 weights_fp8: bool = False, weights_w4: bool = False, kv_fp8: bool = False):
        if dtype not in _RDX_DT:
            raise ValueError(f"dtype must be 'f16' or 'bf16', got {dtype!r}")
        if weights_w4 and weights_fp8:
            raise ValueError("weights_w4 and weights_fp8 do not mix: one weight format per context")
        if weights_w4 and dtype == "f16":
            raise ValueError("weights_w4 needs dtype='bf16' (int4 weights are not built for f16)")
        if kv_fp8 and (classifier or not llama):
            raise ValueError("kv_fp8 is an option of the decoder's KV cache: it needs llama=True")
        self.lib = _lib.load()                       # raises RdxLibraryError when the HIP library is absent
        if not torch.cuda.is_available():
            raise _lib.RdxError("RdxEngine needs a ROCm GPU (torch.cuda.is_available() is False); there is no CPU path")
        self.cfg, self.dtype, self.tdtype = cfg, dtype, _TORCH_DT[dtype]
        self.device = torch.device("cuda", device)
        self.lora = lora
        self.weights_fp8 = weights_fp8               # decoder GEMM weights also quantised to e4m3 + per-row scale (configs[4])
        self.weights_w4 = weights_w4                 # the decoder's seven projections int4 group-quantised (RDX_W_GEMM_W4, radialog_amd/w4.py): the decode step streams
                                                     # the nibbles of QKV, gate/up and down_proj at 1-16 rows; everything else reads the packed dequantised copy
        l, q, v = cfg.llama, cfg.qformer, cfg.vision
        rc = RdxConfig()
        rc.dtype = _RDX_DT[dtype]
        rc.vocab, rc.hidden, rc.inter, rc.layers, rc.heads, rc.max_pos = l.vocab, l.hidden, l.inter, l.layers, l.heads, l.max_pos
        rc.rms_eps = l.rms_eps
        rc.lora_r, rc.lora_scale = (l.lora_r if lora else 0), l.lora_scale
        rc.qformer_dim = l.qformer_dim
        rc.q_hidden, rc.q_layers, rc.q_heads, rc.q_inter = q.hidden, q.layers, q.heads, q.inter
        rc.q_enc_width, rc.q_nquery, rc.q_cross_freq, rc.q_ln_eps = q.enc_width, q.n_query, q.cross_freq, q.ln_eps
        rc.v_img, rc.v_stem, rc.v_b2v, rc.v_proj, rc.v_ln_eps = v.img, v.stem, v.b2v, v.proj, v.ln_eps
        for i in range(4):
            rc.v_planes[i] = v.planes[i]
            rc.v_blocks[i] = v.blocks[i]
        rc.max_batch, rc.max_len = max_batch, max_len
        if classifier:                                   # a findings-classifier context: trunk + its own projector + head
            vision = llama = False
        rc.enable_vision, rc.enable_llama = int(vision), int(llama)
        rc.enable_cls, rc.cls_hidden, rc.cls_classes, rc.cls_pool = int(classifier), cfg.cls.hidden, cfg.cls.classes, cfg.cls.pool
        self.classifier = classifier
        self.max_batch, self.max_len = max_batch, max_len
        self.ctx = C.c_void_p()
        rcode = self.lib.rdx_create(C.byref(self.ctx), device, C.byref(rc))
        if rcode != 0:
            msg = self.lib.rdx_last_error(None)
            raise _lib.RdxError(f"rdx_create failed ({rcode}): {msg.decode() if msg else '?'}")
        self._finalized = False
        self._keep = {}
        # the decoder's KV cache as e4m3 codes + one power-of-two exponent per row (radialog_amd/kv8.py): half the cache bytes; decides what finalize allocates
        self.kv_fp8 = bool(kv_fp8)
        if self.kv_fp8:
            self.set_option("kv_fp8", 1)
        self._rules = LogitsRules()                  # what the context holds (set_logits_rules is the one place that changes it)
        self._sampling = None                        # likewise (set_sampling); None = greedy
        self._logprobs = None                        # likewise (set_logprobs); None = off, else the number of top alternatives

    # ------------------------------------------------------------------------------------------------------------
    def close(self):
        if getattr(self, "ctx", None) is not None and self.ctx.value:
            self.lib.rdx_destroy(self.ctx)
            self.ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self):
        check(self.ctx, self.lib.rdx_sync(self.ctx), "rdx_sync")

    # ------------------------------------------------------------------------------------------------------------
    def _upload(self, items):
        src = {torch.float32: _lib.RDX_SRC_F32, torch.float16: _lib.RDX_SRC_F16, torch.bfloat16: _lib.RDX_SRC_BF16}
        for name, t, kind in items:
            # fp16 / bf16 tensors (a released checkpoint is stored that way) go to the library as they are: widened on the device,
            # tensor by tensor (rdx_set_weight_typed), instead of through an fp32 copy made here
            t = t.to(device=self.device).contiguous()
            if t.dtype not in src:
                t = t.to(torch.float32)
            if t.dim() == 1:
                t = t.view(1, -1)
            rows, cols = t.shape[0], t.numel() // t.shape[0]
            torch.cuda.synchronize(self.device)
            check(self.ctx, self.lib.rdx_set_weight_typed(self.ctx, name.encode(), _ptr(t), src[t.dtype], rows, cols, kind),
                  f"rdx_set_weight({name})")
            del t

    def load_weights(self, get: Callable[[str], torch.Tensor], vision: bool = True, llama: bool = True):
        """`get(name)` returns the fp32 reference-named tensor (any device). Uploads and finalizes."""
        if self.classifier:
            with torch.no_grad():
                self._upload(W.classifier_items(get, self.cfg.vision, self.cfg.cls))
            check(self.ctx, self.lib.rdx_finalize_weights(self.ctx), "rdx_finalize_weights")
            self._finalized = True
            return
        with torch.no_grad():
            if vision:
                self._upload(W.vision_items(get, self.cfg.vision))
                self._upload(W.qformer_items(get, self.cfg.qformer))
            if llama:
                self._upload(W.llama_items(get, self.cfg.llama, self.lora, fp8=self.weights_fp8, dtype=self.tdtype, w4=self.weights_w4))
        check(self.ctx, self.lib.rdx_finalize_weights(self.ctx), "rdx_finalize_weights")
        self._finalized = True

    # ------------------------------------------------------------------------------------------------------------
    def transform_image(self, image_u8, resize: int = 512, crop: int = 448) -> torch.Tensor:
        """rdx_transform_image: the reference's inference transform on the GPU. image_u8: uint8 [H, W] (torch tensor or numpy array: the "L" image of
        demo.py:205-218) -> float32 [3, crop, crop] on this device, bit for bit what Resize(resize) -> CenterCrop(crop) -> ToTensor -> ExpandChannels give
        on the PIL image (ReportDataset.py:96-106)."""
        t = torch.as_tensor(image_u8)
        if t.dim() != 2 or t.dtype != torch.uint8:
            raise ValueError(f"Expected input of shape [1, H, W], found {tuple(t.shape)} ({t.dtype}): one 8-bit channel")
        t = t.to(self.device).contiguous()
        out = torch.empty(3, crop, crop, dtype=torch.float32, device=self.device)
        torch.cuda.synchronize(self.device)
        check(self.ctx, self.lib.rdx_transform_image(self.ctx, _ptr(t), t.shape[0], t.shape[1], int(resize), int(crop), _ptr(out)), "rdx_transform_image")
        self.sync()
        return out

    def encode_image(self, image: torch.Tensor, want_image_embeds: bool = True, previous_image: Optional[torch.Tensor] = None):
        """image float32[B,3,S,S] on this device -> (qformer_out f32[B,nq,Hq], image_embeds f32[B,P,C] or None).
        `previous_image` (same shape) selects the BioViL-T two-image branch (ViT pooler difference features)."""
        v, q = self.cfg.vision, self.cfg.qformer
        if image.dim() != 4 or image.shape[1] != 3 or image.shape[2] != v.img or image.shape[3] != v.img:
            raise ValueError(f"expected image [B,3,{v.img},{v.img}], got {tuple(image.shape)}")
        image = image.to(device=self.device, dtype=torch.float32).contiguous()
        B = image.shape[0]
        out = torch.empty(B, q.n_query, q.hidden, dtype=torch.float32, device=self.device)
        emb = torch.empty(B, v.n_patches, v.proj, dtype=torch.float32, device=self.device) if want_image_embeds else None
        prev = None
        if previous_image is not None:
            if previous_image.shape != image.shape:
                raise AssertionError("current_image and previous_image shapes do not match")     # biovil_t/encoder.py:118
            prev = previous_image.to(device=self.device, dtype=torch.float32).contiguous()
        torch.cuda.synchronize(self.device)
        if prev is None:
            check(self.ctx, self.lib.rdx_encode_image(self.ctx, _ptr(image), B, _ptr(out), _ptr(emb)), "rdx_encode_image")
        else:
            check(self.ctx, self.lib.rdx_encode_image2(self.ctx, _ptr(image), _ptr(prev), B, _ptr(out), _ptr(emb)), "rdx_encode_image2")
        self.sync()
        return out, emb

    def set_logits_rules(self, rules=None) -> LogitsRules:
        """rdx_set_logits_rules: the rules of the next prefill / generate / decode_step calls; None or neutral = off (the plain greedy path)."""
        r = LogitsRules.of(rules)
        c = _lib.RdxLogitsRules(float(r.repetition_penalty), int(r.no_repeat_ngram_size), int(r.min_new_tokens)) if r.active else None
        check(self.ctx, self.lib.rdx_set_logits_rules(self.ctx, None if c is None else C.byref(c)), "rdx_set_logits_rules")
        self._rules = r
        return r

    def set_sampling(self, sampling=None) -> Optional[Sampling]:
        """rdx_set_sampling: the selection of the next prefill / generate / decode_step calls; None = greedy (the argmax)."""
        sm = Sampling.of(sampling)
        c = None if sm is None else _lib.RdxSampling(1, float(sm.temperature), int(sm.top_k), float(sm.top_p), int(sm.seed))
        check(self.ctx, self.lib.rdx_set_sampling(self.ctx, None if c is None else C.byref(c)), "rdx_set_sampling")
        self._sampling = sm
        return sm

    def set_logprobs(self, top_n=None) -> Optional[int]:
        """rdx_set_logprobs: generation log-probs of the next prefill / generate / decode_step calls; None = off, 0 .. 8 = the chosen token's log-prob and
        that many top alternatives per step (read back with get_logprobs)."""
        n = check_top_logprobs(top_n)
        check(self.ctx, self.lib.rdx_set_logprobs(self.ctx, -1 if n is None else n), "rdx_set_logprobs")
        self._logprobs = n
        return n

    def get_logprobs(self, batch: int, n_steps: int, tokens=None, eos_id: int = -1):
        """rdx_get_logprobs: (chosen float32 [batch, n_steps], top_ids int32 [batch, n_steps, k], top_lp float32 [batch, n_steps, k]) of the current
        conversation, on the host, as the device holds them (a finished row's later entries describe the pad token). With `tokens` int [batch, >= n_steps]
        and eos_id >= 0: masked behind each row's first EOS (mask_logprobs_after_eos)."""
        k = self._logprobs
        if k is None:
            raise ValueError("get_logprobs: the logprobs option is off (set_logprobs, or logprobs= of generate / prefill)")
        chosen = torch.zeros(batch, n_steps, dtype=torch.float32)
        top_ids = torch.full((batch, n_steps, k), -1, dtype=torch.int32)
        top_lp = torch.zeros(batch, n_steps, k, dtype=torch.float32)
        check(self.ctx, self.lib.rdx_get_logprobs(self.ctx, batch, n_steps, C.c_void_p(chosen.data_ptr()), C.c_void_p(top_ids.data_ptr()) if k else None,
                                                  C.c_void_p(top_lp.data_ptr()) if k else None), "rdx_get_logprobs")
        if tokens is not None:
            return mask_logprobs_after_eos(tokens, eos_id, chosen, top_ids, top_lp)
        return chosen, top_ids, top_lp

    def logprob_step_test(self, logits, d_step, tokens, vocab, top_n, row_stride=None, step_stride=0, out_ld=None, offset=0, guard_rows=2):
        """logprob_step_k alone (rdx_logprob_step_test). logits: a model-dtype tensor of any shape, read flat from element `offset` on: row b of step s lies at
        offset + s * step_stride + b * row_stride; d_step int [B] (the ADVANCED step counts: row b describes step d_step[b] - 1), tokens int [B, max_new].
        Returns (chosen float32 [B + guard_rows, out_ld], top_ids int32 [.., out_ld, 8], top_lp float32 [.., out_ld, 8]), pre-filled with canaries
        (NaN, -7, NaN) that only the entries the kernel writes replace; the guard rows lie behind the launch's last row."""
        B, max_new = tokens.shape
        x = logits.to(self.device, self.tdtype).contiguous().view(-1)
        ds = d_step.to(self.device, torch.int32).contiguous()
        tk = tokens.to(self.device, torch.int32).contiguous()
        rs = int(vocab if row_stride is None else row_stride)
        ld = int(max_new if out_ld is None else out_ld)
        # every row the kernel can address lies inside the tensor (a step outside [0, max_new) reads nothing)
        last_step = min(max(int(ds.max()) - 1, 0), max_new - 1)
        reach = int(offset) + last_step * int(step_stride) + (B - 1) * rs + int(vocab)
        if ds.numel() != B or offset < 0 or reach > x.numel():
            raise ValueError(f"logprob_step_test: d_step [B]; the last row ends at element {reach} of {x.numel()}")
        chosen = torch.full((B + guard_rows, ld), float("nan"), dtype=torch.float32, device=self.device)
        top_ids = torch.full((B + guard_rows, ld, 8), -7, dtype=torch.int32, device=self.device)
        top_lp = torch.full((B + guard_rows, ld, 8), float("nan"), dtype=torch.float32, device=self.device)
        torch.cuda.synchronize(self.device)
        check(self.ctx, self.lib.rdx_logprob_step_test(self.ctx, C.c_void_p(x.data_ptr() + 2 * int(offset)), rs, int(step_stride), _ptr(ds), _ptr(tk), B, int(vocab),
                                                       max_new, int(top_n), _ptr(chosen), _ptr(top_ids), _ptr(top_lp), ld), "rdx_logprob_step_test")
        return chosen, top_ids, top_lp

    def sample_test(self, logits, n_generated, sampling, rules=None, hist=None, hist_len=None, eos_id=-1):
        """sample_step_k alone (rdx_sample_test): logits [B, V] model dtype, n_generated int [B] (the draw indices), sampling a Sampling or tuple; rules with
        hist int [B, ld] and hist_len int [B] as in select_test. Returns (processed logits [B, V], tokens int32 [B]); the caller's tensors stay."""
        B, V = logits.shape
        r, sm = LogitsRules.of(rules), Sampling.of(sampling)
        x = logits.to(self.device, self.tdtype).contiguous().clone()
        ng = n_generated.to(self.device, torch.int32).contiguous()
        h = None if hist is None else hist.to(self.device, torch.int32).contiguous()
        hl = None if hist_len is None else hist_len.to(self.device, torch.int32).contiguous()
        if ng.numel() != B or (r.active and (h is None or hl is None)):
            raise ValueError("sample_test: n_generated [B]; active rules need hist [B, ld] and hist_len [B]")
        if h is not None and (h.shape[0] != B or hl.numel() != B or int(hl.max()) > h.shape[1] or int(hl.min()) < 0):
            raise ValueError("sample_test: hist [B, ld], hist_len [B] in 0 .. ld")
        out = torch.full((B,), -1, dtype=torch.int32, device=self.device)
        cr = _lib.RdxLogitsRules(float(r.repetition_penalty), int(r.no_repeat_ngram_size), int(r.min_new_tokens))
        cs = _lib.RdxSampling(1, float(sm.temperature), int(sm.top_k), float(sm.top_p), int(sm.seed))
        torch.cuda.synchronize(self.device)
        check(self.ctx, self.lib.rdx_sample_test(self.ctx, _ptr(x), B, V, _ptr(h), _ptr(hl), _ptr(ng), 0 if h is None else h.shape[1], C.byref(cr),
                                                 int(eos_id), C.byref(cs), _ptr(out)), "rdx_sample_test")
        return x, out

    def select_test(self, logits, hist, hist_len, n_generated, rules, eos_id=-1):
        """select_step_k alone (rdx_select_test): logits [B, V] model dtype, hist int [B, ld], hist_len / n_generated int [B]. Returns (processed
        logits [B, V], tokens int32 [B]); the caller's tensors are left as they are."""
        B, V = logits.shape
        r = LogitsRules.of(rules)
        x = logits.to(self.device, self.tdtype).contiguous().clone()
        h = hist.to(self.device, torch.int32).contiguous()
        hl, ng = hist_len.to(self.device, torch.int32).contiguous(), n_generated.to(self.device, torch.int32).contiguous()
        if h.shape[0] != B or hl.numel() != B or ng.numel() != B or int(hl.max()) > h.shape[1] or int(hl.min()) < 0:
            raise ValueError("select_test: hist [B, ld], hist_len [B] in 0 .. ld, n_generated [B]")
        out = torch.full((B,), -1, dtype=torch.int32, device=self.device)
        c = _lib.RdxLogitsRules(float(r.repetition_penalty), int(r.no_repeat_ngram_size), int(r.min_new_tokens))
        torch.cuda.synchronize(self.device)
        check(self.ctx, self.lib.rdx_select_test(self.ctx, _ptr(x), B, V, _ptr(h), _ptr(hl), _ptr(ng), h.shape[1], C.byref(c), int(eos_id), _ptr(out)),
              "rdx_select_test")
        return x, out

    def _reusable_prefix(self, ids: torch.Tensor, qf, pad_id: int) -> int:
        """Number of leading cache slots of the previous generate(reuse_prefix=True) call that this prompt can keep: the
        longest token prefix all rows share with what was fed then (prompt + consumed answer tokens), provided the image
        embeddings are the same, the whole <IMG> block lies inside it and the rest holds neither padding nor <IMG>."""
        conv = getattr(self, "_conv", None)
        if conv is None or conv["seq"].shape[0] != ids.shape[0]:
            return 0
        if (qf is None) != (conv["qf"] is None) or (qf is not None and not torch.equal(qf, conv["qf"])):
            return 0
        seq, new = conv["seq"], ids.cpu().to(torch.int64)
        m = min(seq.shape[1], new.shape[1] - 1)                  # at least one token must be run to get logits
        if m <= 0:
            return 0
        same = (seq[:, :m] == new[:, :m]).all(dim=0).to(torch.int64)
        p = int(same.cumprod(0).sum())
        tail = new[:, p:]
        if p <= 0 or bool((tail == pad_id).any()) or bool((tail == 32000).any()):
            return 0
        return p

    def generate(self, ids: torch.Tensor, qformer_embs: Optional[torch.Tensor], max_new: int, eos_id: int = 2,
                 pad_id: int = 0, mask: Optional[torch.Tensor] = None, output_scores: bool = False, use_graph: bool = True,
                 reuse_prefix: bool = False, logits_rules=None, sampling=None, logprobs: Optional[int] = None):
        """Greedy (sampling=None) or sampled generation. Returns (tokens int32[B,n_steps], scores [n_steps,B,V] model dtype or None, n_steps).
        logprobs: None, or 0 .. 8: a FOURTH element (chosen float32 [B, n_steps], top_ids int32 [B, n_steps, k], top_lp float32 [B, n_steps, k]) on the host --
        the log-prob of every generated token under the scores row it was chosen from (processed / warped under rules / sampling: HF's
        compute_transition_scores(normalize_logits=True)) and the k largest columns of that row with theirs; (0.0, -1, 0.0) behind a row's first EOS.
        reuse_prefix: multi-turn conversations -- keep the KV rows of the token prefix this prompt shares with the previous
        reuse_prefix call and prefill only the rest (rdx_generate_append); outputs are those of the full prompt.
        logits_rules: LogitsRules or (repetition_penalty, no_repeat_ngram_size, min_new_tokens); the scores are then the processed ones
        (HF's .scores). An active rule prefills the whole prompt: the token history is not carried across calls.
        sampling: Sampling or (temperature, top_k, top_p, seed): rules, then the warpers, then one draw per row and step; the scores are the warped ones."""
        B, T = ids.shape
        if reuse_prefix and self.kv_fp8:
            raise ValueError("reuse_prefix is not built on the fp8 KV cache (kv_fp8): the kept prefix is not held in the model dtype")
        self.set_sampling(sampling)
        if self.set_logits_rules(logits_rules).active:
            reuse_prefix = False
        self.set_logprobs(logprobs)
        ids32 = ids.to(device=self.device, dtype=torch.int32).contiguous()
        m32 = None if mask is None else mask.to(device=self.device, dtype=torch.int32).contiguous()
        qf = None if qformer_embs is None else qformer_embs.to(device=self.device, dtype=torch.float32).contiguous()
        key = ("tok", B, max_new)
        toks = self._keep.get(key)
        if toks is None:
            toks = torch.zeros(B, max_new, dtype=torch.int32, device=self.device)
            self._keep[key] = toks
        toks.fill_(pad_id)
        scores = None
        if output_scores:
            skey = ("scores", B, max_new)
            scores = self._keep.get(skey)
            if scores is None:
                scores = torch.zeros(max_new, B, self.cfg.llama.vocab, dtype=self.tdtype, device=self.device)
                self._keep[skey] = scores
        n = C.c_int(0)
        torch.cuda.synchronize(self.device)
        keep = self._reusable_prefix(ids, qf, pad_id) if (reuse_prefix and mask is None) else 0
        self.last_kept_prefix = keep
        if keep:
            tail = ids32[:, keep:].contiguous()
            check(self.ctx, self.lib.rdx_generate_append(self.ctx, _ptr(tail), B, T - keep, keep, max_new, eos_id, pad_id, _ptr(toks),
                                                         _ptr(scores), C.byref(n), int(use_graph)), "rdx_generate_append")
        else:
            check(self.ctx, self.lib.rdx_generate(self.ctx, _ptr(ids32), _ptr(m32), B, T, _ptr(qf), max_new, eos_id, pad_id,
                                                  _ptr(toks), _ptr(scores), C.byref(n), int(use_graph)), "rdx_generate")
        if reuse_prefix and mask is None:
            # what the cache now holds: the prompt and every answer token that was fed back (all but the last one selected)
            self._conv = {"seq": torch.cat([ids.cpu().to(torch.int64), toks[:, :max(n.value - 1, 0)].cpu().to(torch.int64)], dim=1),
                          "qf": None if qf is None else qf.clone()}
        else:
            self._conv = None
        if logprobs is not None:
            return toks, scores, n.value, self.get_logprobs(B, n.value, tokens=toks[:, : n.value], eos_id=eos_id)
        return toks, scores, n.value

    def set_lookup(self, lookup=None) -> Optional[Lookup]:
        """rdx_set_lookup: the draft rule of the next generate_lookup calls; None = off. No other call looks at the option."""
        lk = None if lookup is None else Lookup.of(lookup)
        c = None if lk is None else _lib.RdxLookup(int(lk.draft_len), int(lk.ngram_max), int(lk.ngram_min))
        check(self.ctx, self.lib.rdx_set_lookup(self.ctx, None if c is None else C.byref(c)), "rdx_set_lookup")
        return lk

    def generate_lookup(self, ids: torch.Tensor, qformer_embs: Optional[torch.Tensor], max_new: int, eos_id: int = 2, pad_id: int = 0,
                        mask: Optional[torch.Tensor] = None, lookup=Lookup(), corpus=None, output_scores: bool = False):
        """Batch-1 greedy generation with prompt-lookup drafts (rdx_generate_lookup). ids int [1, T]; corpus: optional int sequence of further token ids
        to search for drafts, in front of the prompt. Returns (tokens int32 [1, max_new], scores [n, 1, V] model dtype or None, n,
        stats = {"passes", "drafted", "accepted", "forwards"}, trace int32 [forwards, 2] = (drafted, accepted) per forward behind the prompt).
        The tokens are greedy under the returned scores; they need not equal generate()'s (a pass and a plain step round differently). Rules, sampling
        and logprobs a previous call left on the context are switched off first, as beam_search does."""
        B, T = ids.shape
        lk = Lookup.of(lookup)
        self.set_logits_rules(None)
        self.set_sampling(None)
        self.set_logprobs(None)
        self.set_lookup(lk)
        ids32 = ids.to(device=self.device, dtype=torch.int32).contiguous()
        m32 = None if mask is None else mask.to(device=self.device, dtype=torch.int32).contiguous()
        qf = None if qformer_embs is None else qformer_embs.to(device=self.device, dtype=torch.float32).contiguous()
        cp = None if corpus is None else torch.as_tensor(corpus).to(device="cpu", dtype=torch.int32).contiguous().view(-1)
        toks = torch.full((B, max_new), pad_id, dtype=torch.int32, device=self.device)
        scores = torch.zeros(max_new, B, self.cfg.llama.vocab, dtype=self.tdtype, device=self.device) if output_scores else None
        cap = max(int(max_new), 1)
        trace = torch.full((cap, 2), -1, dtype=torch.int32)      # the call writes one row per forward
        stats = (C.c_int * 3)()
        n = C.c_int(0)
        self._keep["prefill"] = (ids32, m32, qf, toks)        # decode_step continues the conversation the call leaves behind
        self._conv = None
        torch.cuda.synchronize(self.device)
        check(self.ctx, self.lib.rdx_generate_lookup(self.ctx, _ptr(ids32), _ptr(m32), B, T, _ptr(qf), None if cp is None or cp.numel() == 0 else C.c_void_p(cp.data_ptr()),
                                                     0 if cp is None else cp.numel(), max_new, eos_id, pad_id, _ptr(toks), _ptr(scores), C.byref(n), stats,
                                                     C.c_void_p(trace.data_ptr()), cap), "rdx_generate_lookup")
        if mask is None:      # what the cache now holds, for a generate(reuse_prefix=True) behind this call
            self._conv = {"seq": torch.cat([ids.cpu().to(torch.int64), toks[:, :max(n.value - 1, 0)].cpu().to(torch.int64)], dim=1),
                          "qf": None if qf is None else qf.clone()}
        trace = trace[: int((trace[:, 0] >= 0).sum())]
        stats = {"passes": stats[0], "drafted": stats[1], "accepted": stats[2], "forwards": trace.shape[0]}
        return toks, (None if scores is None else scores[: n.value]), n.value, stats, trace

    def lookup_accept_test(self, part_val, part_idx, d, tail, hist, hist_len, state, lookup, corpus=None, slot_end=1 << 30, advance=True, eos_id=-1, pad_id=0,
                           max_new=64, logits=None, fwd=0):
        """lookup_accept_k alone (rdx_lookup_accept_test). part_val float [d + 1, n_tiles], part_idx int [d + 1, n_tiles]; tail: [last token, drafts ..];
        hist int [hist_ld] with hist_len entries; state (step, slot, position, unfinished); lookup a Lookup. Returns a dict of host tensors: out_tokens
        [max_new] (-7 where not written), tail [16], hist, state [5], status [4], trace [8, 2], pos_ids [16], scores [max_new, V] or None."""
        lk = Lookup.of(lookup)
        dev = self.device
        pv = part_val.to(dev, torch.float32).contiguous()
        pi = part_idx.to(dev, torch.int32).contiguous()
        if pv.shape != pi.shape or pv.shape[0] != d + 1:
            raise ValueError("lookup_accept_test: part_val / part_idx [d + 1, n_tiles]")
        tl = torch.full((16,), -7, dtype=torch.int32)
        tl[: len(tail)] = torch.as_tensor(tail, dtype=torch.int32)
        tl = tl.to(dev)
        h = torch.as_tensor(hist, dtype=torch.int32).to(dev).contiguous()
        st = torch.tensor(list(state) + [int(hist_len)], dtype=torch.int32, device=dev)
        cp = None if corpus is None or len(corpus) == 0 else torch.as_tensor(corpus, dtype=torch.int32).to(dev).contiguous()
        out = torch.full((max_new,), -7, dtype=torch.int32, device=dev)
        status = torch.tensor([-7, -7, int(fwd), 0], dtype=torch.int32, device=dev)
        trace = torch.full((8, 2), -7, dtype=torch.int32, device=dev)
        pos_ids = torch.full((16,), -7, dtype=torch.int32, device=dev)
        lg = None if logits is None else logits.to(dev, self.tdtype).contiguous()
        sc = None if logits is None else torch.zeros(max_new, self.cfg.llama.vocab, dtype=self.tdtype, device=dev)
        if st.numel() != 5 or len(tail) != d + 1 or (lg is not None and tuple(lg.shape) != (d + 1, self.cfg.llama.vocab)):
            raise ValueError("lookup_accept_test: state of 4 ints, tail of d + 1 ids, logits [d + 1, vocab]")
        torch.cuda.synchronize(dev)
        check(self.ctx, self.lib.rdx_lookup_accept_test(self.ctx, _ptr(pv), _ptr(pi), pv.shape[1], int(d), _ptr(tl), _ptr(cp), 0 if cp is None else cp.numel(),
                                                        lk.draft_len, lk.ngram_max, lk.ngram_min, int(slot_end), _ptr(h), h.numel(), _ptr(st), int(bool(advance)),
                                                        int(eos_id), int(pad_id), int(max_new), _ptr(out), _ptr(lg), _ptr(sc), _ptr(status), _ptr(trace), 8,
                                                        _ptr(pos_ids)), "rdx_lookup_accept_test")
        return {"out_tokens": out.cpu(), "tail": tl.cpu(), "hist": h.cpu(), "state": st.cpu(), "status": status.cpu(), "trace": trace.cpu(),
                "pos_ids": pos_ids.cpu(), "scores": None if sc is None else sc.cpu()}

    def beam_search(self, ids: torch.Tensor, qformer_embs: Optional[torch.Tensor], num_beams: int, max_new: int, eos_id: int = 2,
                    pad_id: int = 0, mask: Optional[torch.Tensor] = None, length_penalty: float = 1.0, early_stopping: bool = False,
                    output_scores: bool = False):
        """transformers 4.28.1 beam search over rdx_beam_search. ids int[B, T] (NOT expanded; expanded here with repeat_interleave
        like _expand_inputs_for_generation). Returns (tokens int32[B, max_new] on the host, lengths int32[B], sequence scores f32[B],
        step scores [n, B * num_beams, V] model dtype or None, n forwards)."""
        B, T = ids.shape
        k = int(num_beams)
        rep = lambda t, dt: None if t is None else t.to(device=self.device, dtype=dt).repeat_interleave(k, dim=0).contiguous()   # noqa: E731
        ids32, m32, qf = rep(ids, torch.int32), rep(mask, torch.int32), rep(qformer_embs, torch.float32)
        self.set_logits_rules(None)                  # rules are a greedy-search feature; a call that left some behind must not make this one fail
        self.set_sampling(None)                      # likewise: beam-sample is not built
        self.set_logprobs(None)                      # likewise: beams return sequence scores
        toks = torch.zeros(B, max_new, dtype=torch.int32)
        lens = torch.zeros(B, dtype=torch.int32)
        seq_scores = torch.zeros(B, dtype=torch.float32)
        sc = torch.zeros(max_new, B * k, self.cfg.llama.vocab, dtype=self.tdtype, device=self.device) if output_scores else None
        n = C.c_int(0)
        self._conv = None
        torch.cuda.synchronize(self.device)
        check(self.ctx, self.lib.rdx_beam_search(self.ctx, _ptr(ids32), _ptr(m32), B, k, T, _ptr(qf), max_new, eos_id, pad_id,
                                                 float(length_penalty), int(bool(early_stopping)), C.c_void_p(toks.data_ptr()),
                                                 C.c_void_p(lens.data_ptr()), C.c_void_p(seq_scores.data_ptr()), _ptr(sc), C.byref(n)),
              "rdx_beam_search")
        return toks, lens, seq_scores, (None if sc is None else sc[: n.value]), n.value

    def prefill(self, ids, qformer_embs, max_new, eos_id=2, pad_id=0, mask=None, want_logits=True, logits_rules=None, sampling=None, logprobs: Optional[int] = None):
        """The prompt and token 0. logits_rules, sampling and logprobs (as in generate) stay in force for the decode_step calls behind this prefill; the
        log-probs of the steps run so far: get_logprobs(B, steps)."""
        B, T = ids.shape
        self.set_sampling(sampling)
        self.set_logits_rules(logits_rules)
        self.set_logprobs(logprobs)
        ids32 = ids.to(device=self.device, dtype=torch.int32).contiguous()
        m32 = None if mask is None else mask.to(device=self.device, dtype=torch.int32).contiguous()
        qf = None if qformer_embs is None else qformer_embs.to(device=self.device, dtype=torch.float32).contiguous()
        toks = torch.full((B, max_new), pad_id, dtype=torch.int32, device=self.device)
        logits = torch.empty(B, self.cfg.llama.vocab, dtype=self.tdtype, device=self.device) if want_logits else None
        self._keep["prefill"] = (ids32, m32, qf, toks)
        self._conv = None                            # the KV cache is overwritten: nothing of an earlier conversation can be reused
        torch.cuda.synchronize(self.device)
        check(self.ctx, self.lib.rdx_prefill(self.ctx, _ptr(ids32), _ptr(m32), B, T, _ptr(qf), max_new, eos_id, pad_id,
                                             _ptr(toks), _ptr(logits)), "rdx_prefill")
        self.sync()
        return toks, logits

    def decode_step(self, want_logits=True, input_ids: Optional[torch.Tensor] = None, logits_rules=None, sampling=None, logprobs: Optional[int] = None):
        """One decode step on the token the previous step selected, or on caller-supplied `input_ids` int[B] (rdx_decode_step_ids).
        logits_rules: None keeps the rules the context holds (those of the prefill, unless a generate / beam_search call came in between); rules
        cannot be switched on behind a prefill that ran without any. sampling: None keeps what the context holds, too, and so does logprobs (an int
        switches the option on from this step on, or changes its top-n; earlier steps keep what they wrote)."""
        ids32, m32, qf, toks = self._keep["prefill"]
        if logprobs is not None and check_top_logprobs(logprobs) != self._logprobs:
            self.set_logprobs(logprobs)
        if sampling is not None and Sampling.of(sampling) != self._sampling:
            self.set_sampling(sampling)
        if logits_rules is not None and LogitsRules.of(logits_rules) != self._rules:
            self.set_logits_rules(logits_rules)
        B = ids32.shape[0]
        logits = torch.empty(B, self.cfg.llama.vocab, dtype=self.tdtype, device=self.device) if want_logits else None
        if input_ids is None:
            check(self.ctx, self.lib.rdx_decode_step(self.ctx, _ptr(logits)), "rdx_decode_step")
        else:
            forced = input_ids.to(device=self.device, dtype=torch.int32).contiguous().view(-1)
            if forced.numel() != B:
                raise ValueError(f"input_ids must hold one id per row ({B}), got {forced.numel()}")
            torch.cuda.synchronize(self.device)
            check(self.ctx, self.lib.rdx_decode_step_ids(self.ctx, _ptr(forced), _ptr(logits)), "rdx_decode_step_ids")
        self.sync()
        return toks, logits

    def row_session(self, rows: int, stage: int, cap: int, eos_id: int = 2, pad_id: int = 0, use_graph: bool = True) -> "RowSession":
        """Open a row session (rdx_rows_begin): `rows` live rows refilled one by one through `stage` staging rows, `cap` tokens per request at most.
        Greedy search only: logits rules, sampling and generation log-probs are switched off first. Close it (or leave the `with` block) before any other decoder call."""
        self.set_sampling(None)
        self.set_logits_rules(None)
        self.set_logprobs(None)
        self._conv = None                            # the KV cache is overwritten
        return RowSession(self, rows, stage, cap, eos_id, pad_id, use_graph)

    def generate_queue(self, requests, rows: int, stage: Optional[int] = None, eos_id: int = 2, pad_id: int = 0, poll: int = 4,
                       min_refill: Optional[int] = None, use_graph: bool = True, return_scheduler: bool = False):
        """Continuous batching: `requests` = (ids 1-D, qformer_embs [32, D] or None, max_new) each, run through `rows` live rows by a RowScheduler
        (radialog_amd/rowqueue.py); a finished row takes the next waiting prompt while its neighbours go on decoding. Returns the generated tokens of every
        request, in request order (1-D int64, cut at EOS or at the request's max_new); with return_scheduler also the scheduler (its step / refill counts).
        stage / min_refill default to QUEUE_STAGE / QUEUE_MIN_REFILL (profiles/r15_queue.md), stage bounded by max_batch - rows."""
        from .rowqueue import RowScheduler
        requests = list(requests)
        if stage is None:
            stage = max(1, min(QUEUE_STAGE, self.max_batch - rows))
        if min_refill is None:
            min_refill = QUEUE_MIN_REFILL
        if not requests:
            return ([], None) if return_scheduler else []
        cap = max(int(r[2]) for r in requests)
        with self.row_session(rows, stage, cap, eos_id=eos_id, pad_id=pad_id, use_graph=use_graph) as ses:
            sched = RowScheduler(ses, rows, stage, poll=poll, min_refill=min_refill)
            out = sched.run(requests)
        return (out, sched) if return_scheduler else out

    def score(self, ids, qformer_embs, labels, mask=None, want_top1=False, want_logits=False):
        """rdx_score: per-token log-probabilities of given text from one pass over the prompt's kernels. ids int [B, T]; labels int [B, T] in HF's
        convention (the token at position t, -100 = not scored); mask as in prefill (None -> ids != 0). Returns (logprob float32 [B, T]: at t >= 1 with
        labels[b, t] != -100, log p(labels[b, t] | ids[b, :t]), 0 elsewhere; top1 int32 [B, T] or None: the model's argmax at the same entries, -1
        elsewhere; logits [B, T, V] model dtype or None). Overwrites the KV cache and leaves no conversation: decode_step needs a new prefill.
        Logits rules and sampling held by the context stay as they are and are ignored."""
        B, T = ids.shape
        lab = torch.as_tensor(labels).to(device="cpu", dtype=torch.int32).contiguous()
        if tuple(lab.shape) != (B, T):
            raise ValueError(f"labels must have the shape of ids {(B, T)}, got {tuple(lab.shape)}")
        ids32 = ids.to(device=self.device, dtype=torch.int32).contiguous()
        m32 = None if mask is None else mask.to(device=self.device, dtype=torch.int32).contiguous()
        qf = None if qformer_embs is None else qformer_embs.to(device=self.device, dtype=torch.float32).contiguous()
        logprob = torch.empty(B, T, dtype=torch.float32, device=self.device)
        top1 = torch.empty(B, T, dtype=torch.int32, device=self.device) if want_top1 else None
        logits = torch.empty(B, T, self.cfg.llama.vocab, dtype=self.tdtype, device=self.device) if want_logits else None
        self._conv = None                            # the KV cache is overwritten: nothing of an earlier conversation can be reused
        torch.cuda.synchronize(self.device)
        check(self.ctx, self.lib.rdx_score(self.ctx, _ptr(ids32), _ptr(m32), B, T, _ptr(qf), C.c_void_p(lab.data_ptr()), _ptr(logprob), _ptr(top1),
                                           _ptr(logits)), "rdx_score")
        return logprob, top1, logits

    def score_rows_test(self, logits, target, vocab=None):
        """score_rows_k alone (rdx_score_rows_test): logits [M, ld] model dtype (ld a multiple of 8; columns vocab .. ld - 1 are pad columns), target int [M]
        (-100 = not scored). Returns (logprob float32 [M], top1 int32 [M])."""
        M, ld = logits.shape
        V = ld if vocab is None else int(vocab)
        x = logits.to(self.device, self.tdtype).contiguous()
        tg = target.to(self.device, torch.int32).contiguous()
        if tg.numel() != M:
            raise ValueError("score_rows_test: target [M]")
        lp = torch.full((M,), float("nan"), dtype=torch.float32, device=self.device)
        t1 = torch.full((M,), -7, dtype=torch.int32, device=self.device)
        torch.cuda.synchronize(self.device)
        check(self.ctx, self.lib.rdx_score_rows_test(self.ctx, _ptr(x), M, V, ld, _ptr(tg), _ptr(lp), _ptr(t1)), "rdx_score_rows_test")
        return lp, t1

    def kv_read(self, layer: int, which: int, batch: int) -> torch.Tensor:
        l = self.cfg.llama
        out = torch.empty(self.max_batch, l.heads, self.max_len, l.head_dim, dtype=self.tdtype, device=self.device)
        check(self.ctx, self.lib.rdx_kv_read(self.ctx, layer, which, _ptr(out)), "rdx_kv_read")
        self.sync()
        return out[:batch]

    def kv_read_codes(self, layer: int, which: int, batch: int):
        """An fp8 KV cache (kv_fp8=True) as stored, in logical order: (codes uint8 [batch, heads, max_len, 128], exponents int8 [batch, heads, max_len]) of
        one layer's K (which 0) or V (1); kv_read() returns the same rows dequantised (radialog_amd/kv8.py dequant)."""
        l = self.cfg.llama
        codes = torch.empty(self.max_batch, l.heads, self.max_len, l.head_dim, dtype=torch.uint8, device=self.device)
        exps = torch.empty(self.max_batch, l.heads, self.max_len, dtype=torch.int8, device=self.device)
        check(self.ctx, self.lib.rdx_kv_read_codes(self.ctx, layer, which, _ptr(codes), _ptr(exps)), "rdx_kv_read_codes")
        self.sync()
        return codes[:batch], exps[:batch]

    def kv_cache_bytes(self) -> int:
        """Bytes of the context's KV allocation (rdx_kv_bytes): K and V caches of every layer and, fp8, their row exponents."""
        n = self.lib.rdx_kv_bytes(self.ctx)
        if n < 0:
            raise _lib.RdxError(f"rdx_kv_bytes failed: {self._last_error()}")
        return int(n)

    def kv_write_test(self, layer: int, which: int, rows: torch.Tensor):
        """rdx_kv_write_test: overwrite one layer's K (0) or V (1) cache of a plain engine with rows [batch <= max_batch, heads, max_len, 128] in logical
        order (rows past `batch` become zeros)."""
        l = self.cfg.llama
        full = torch.zeros(self.max_batch, l.heads, self.max_len, l.head_dim, dtype=self.tdtype, device=self.device)
        full[:rows.shape[0]] = rows.to(self.device, self.tdtype)
        torch.cuda.synchronize(self.device)
        check(self.ctx, self.lib.rdx_kv_write_test(self.ctx, layer, which, _ptr(full)), "rdx_kv_write_test")

    def gemm_test(self, x, w, bias=None, resid=None, epi=0, norm_w=None, eps=1e-6, force=0):
        """out = epilogue(x @ w.T) through the production GEMM kernels. x [M,K] model dtype, w [N,K] fp32."""
        M, K = x.shape
        N = w.shape[0]
        x = x.to(self.device, self.tdtype).contiguous()
        w = w.to(self.device, torch.float32).contiguous()
        b = None if bias is None else bias.to(self.device, torch.float32).contiguous()
        r = None if resid is None else resid.to(self.device, self.tdtype).contiguous()
        nw = None if norm_w is None else norm_w.to(self.device, self.tdtype).contiguous()
        out = torch.empty(M, N // 2 if epi == 4 else N, dtype=self.tdtype, device=self.device)
        torch.cuda.synchronize(self.device)
        check(self.ctx, self.lib.rdx_gemm_test(self.ctx, _ptr(x), _ptr(w), _ptr(b), _ptr(r), _ptr(out), M, N, K, epi, _ptr(nw),
                                               eps, force), "rdx_gemm_test")
        return out

    def quant_test(self, x, groups=1, norm_w=None, eps=1e-6):
        """The fp8 path's activation quantisers on caller data (rdx_quant_test): x [M, K] model dtype -> (e4m3 codes uint8 [M, K], fp32 scales
        [M, groups]); norm_w given: RMSNorm -> e4m3 with one scale per row (the prefill's rmsnorm -> fp8)."""
        M, K = x.shape
        x = x.to(self.device, self.tdtype).contiguous()
        nw = None if norm_w is None else norm_w.to(self.device, self.tdtype).contiguous()
        g = 1 if norm_w is not None else groups
        out8 = torch.empty(M, K, dtype=torch.uint8, device=self.device)
        sc = torch.empty(M, g, dtype=torch.float32, device=self.device)
        torch.cuda.synchronize(self.device)
        check(self.ctx, self.lib.rdx_quant_test(self.ctx, _ptr(x), M, K, g, 0 if norm_w is None else 1, _ptr(nw), eps, _ptr(out8), _ptr(sc)), "rdx_quant_test")
        return out8, sc

    def set_option(self, name: str, value: int):
        """rdx_set_option: one runtime switch of this engine (the table: INTEGRATION.md "Runtime switches"; option_names() lists them). The environment is read
        once, when the engine is created; afterwards only this call changes a switch. Raises RdxError for an unknown name, a value out of range, or a switch that
        load_weights allocates by ("kv_fp8", "kperm") once the weights are loaded."""
        check(self.ctx, self.lib.rdx_set_option(self.ctx, name.encode(), int(value)), "rdx_set_option")

    def get_option(self, name: str) -> int:
        """rdx_get_option: the value of a switch as this engine holds it."""
        v = C.c_int(0)
        check(self.ctx, self.lib.rdx_get_option(self.ctx, name.encode(), C.byref(v)), "rdx_get_option")
        return v.value

    def option_names(self) -> list:
        """rdx_option_name: every switch the library has, in table order."""
        names = []
        while (n := self.lib.rdx_option_name(len(names))) is not None:
            names.append(n.decode())
        return names

    def conv_test(self, x, w, bias=None, resid=None, ksize=1, stride=1, epi=0, path=0, iters=0):
        """One NHWC convolution (rdx_conv_test): x [B,H,H,Cin] model dtype, w [Cout, ksize*ksize*Cin] fp32 in the (kh, kw, c) K order;
        path 0 = row-major production dispatch, 1 = fragment-packed pconv_k, 2 = pconv_k with row-major output. Returns out
        [B,Ho,Ho,Cout] (and ms per launch when iters > 0)."""
        B, H, _, Cin = x.shape
        Cout = w.shape[0]
        Ho = (H + 2 * (ksize // 2) - ksize) // stride + 1
        x = x.to(self.device, self.tdtype).contiguous()
        w = w.to(self.device, torch.float32).contiguous()
        b = None if bias is None else bias.to(self.device, torch.float32).contiguous()
        r = None if resid is None else resid.to(self.device, self.tdtype).contiguous()
        out = torch.empty(B, Ho, Ho, Cout, dtype=self.tdtype, device=self.device)
        ms = C.c_float(0)
        torch.cuda.synchronize(self.device)
        check(self.ctx, self.lib.rdx_conv_test(self.ctx, _ptr(x), _ptr(w), _ptr(b), _ptr(r), _ptr(out), B, H, Cin, Cout, ksize, stride, epi,
                                               path, iters, C.byref(ms) if iters else None), "rdx_conv_test")
        return (out, ms.value) if iters else out

    def stem_test(self, image, w, bias, path=0):
        """The stem on its own (rdx_stem_test): image fp32 [B,3,S,S], w fp32 [stem,3,7,7] (torch layout, laid out here as the weight loader does),
        bias fp32 [stem]; path 0 = fused stem_pool_k row-major, 1 = fused fragment-packed (unpacked), 2 = conv_gemm + maxpool_k. Returns
        [B,S/4,S/4,stem] in the model dtype."""
        B, _, S, _ = image.shape
        stem = w.shape[0]
        image = image.to(self.device, torch.float32).contiguous()
        wk = W.stem_khwc4(w.float()).to(self.device)
        b = bias.to(self.device, torch.float32).contiguous()
        out = torch.empty(B, S // 4, S // 4, stem, dtype=self.tdtype, device=self.device)
        torch.cuda.synchronize(self.device)
        check(self.ctx, self.lib.rdx_stem_test(self.ctx, _ptr(image), _ptr(wk), _ptr(b), _ptr(out), B, S, stem, path), "rdx_stem_test")
        return out

    def norm_test(self, op, x, gamma=None, beta=None, emb=None, out_rows_stride=None, want_f32=False, aux=0, pool=0, eps=1e-12):
        """The encoder's LayerNorm / pooling kernels (rdx_norm_test). op 0 layernorm_k, 1 layernorm_ex_k (x [rows, ldx] with H = gamma's length,
        output rows `out_rows_stride` apart, emb [aux, H] added as emb[row % aux]), 2 layernorm_packed_k, 3 scramble_layernorm_k (x [B, P, C]),
        4 avgpool_flatten_k (x [B, G, G, C] -> [B, C * (G // pool) ** 2]). Returns (out, out_f32 or None); op 1 returns out as [rows, ldo]."""
        x = x.to(self.device, self.tdtype).contiguous()
        g = None if gamma is None else gamma.to(self.device, torch.float32).contiguous()
        bt = None if beta is None else beta.to(self.device, torch.float32).contiguous()
        e = None if emb is None else emb.to(self.device, self.tdtype).contiguous()
        f32 = None
        if op == 3:
            B, P, H = x.shape
            rows, aux, ldx, ldo = B, P, H, H
            out = torch.empty(B, P, H, dtype=self.tdtype, device=self.device)
        elif op == 4:
            B, G, _, H = x.shape
            rows, aux, ldx, ldo = B, G, H, H
            out = torch.empty(B, H * (G // pool) ** 2, dtype=self.tdtype, device=self.device)
        else:
            rows, ldx = x.shape
            H = g.numel()
            ldo = out_rows_stride or H
            out = torch.full((rows, ldo), float("nan"), dtype=self.tdtype, device=self.device)
            if e is not None:
                aux = e.shape[0]
        if want_f32:
            f32 = torch.empty(out.shape[:-1] + (H,) if op != 1 else (rows, H), dtype=torch.float32, device=self.device)
        torch.cuda.synchronize(self.device)
        check(self.ctx, self.lib.rdx_norm_test(self.ctx, int(op), _ptr(x), _ptr(g), _ptr(bt), _ptr(e), _ptr(out), _ptr(f32), rows, H, ldx, ldo,
                                               int(aux), int(pool), float(eps)), "rdx_norm_test")
        return out, f32

    def attn_test(self, q, k, v, causal=False, key_mask=None, o_packed=False, kernel=0):
        """softmax(q k^T / sqrt(D)) v through the production attention kernels (rdx_attn_test). q [B,Tq,H,D], k / v [B,Tk,H,D] model-dtype views
        with any strides whose last dim is contiguous (the kernels read 16-byte pieces); key_mask uint8 [B, >= Tk] (1 = attend), rows padded here
        to a multiple of 4 bytes; kernel 0 = production dispatch, 1 = attention_k, 2 = flash_prefill_k. Returns [B,Tq,H,D]."""
        B, Tq, H, D = q.shape
        Tk = k.shape[1]
        for t in (q, k, v):
            assert t.device == self.device and t.dtype == self.tdtype and t.stride(3) == 1
        out = torch.full((B, Tq, H, D), float("nan"), dtype=self.tdtype, device=self.device)
        st = [q.stride(0), q.stride(1), q.stride(2), k.stride(0), k.stride(1), k.stride(2), v.stride(0), v.stride(1), v.stride(2),
              out.stride(0), out.stride(1), out.stride(2)]
        strides = torch.tensor(st, dtype=torch.int64)
        km, km_bs = None, 0
        if key_mask is not None:
            km_bs = (max(key_mask.shape[1], Tk) + 3) // 4 * 4
            km = torch.zeros(B, km_bs, dtype=torch.uint8)
            km[:, :key_mask.shape[1]] = key_mask.to(torch.uint8).cpu()
            km = km.to(self.device)
        torch.cuda.synchronize(self.device)
        check(self.ctx, self.lib.rdx_attn_test(self.ctx, _ptr(q), _ptr(k), _ptr(v), _ptr(out), C.c_void_p(strides.data_ptr()), B, H, Tq, Tk, D,
                                               int(causal), _ptr(km), km_bs, int(o_packed), int(kernel)), "rdx_attn_test")
        return out

    def logits_test(self, x, w, n_valid=None, fp8=False):
        """(logits [M,N] model dtype, argmax int32[M]) of x @ w.T through the lm_head epilogue of the weight-streaming kernels."""
        import ctypes
        M, K = x.shape
        N = w.shape[0]
        x = x.to(self.device, self.tdtype).contiguous()
        w = w.to(self.device, torch.float32).contiguous()
        out = torch.zeros(M, N, dtype=self.tdtype, device=self.device)
        am = (ctypes.c_int32 * M)()
        torch.cuda.synchronize(self.device)
        check(self.ctx, self.lib.rdx_logits_test(self.ctx, _ptr(x), _ptr(w), M, N, N if n_valid is None else n_valid, K, _ptr(out),
                                                 ctypes.cast(am, ctypes.c_void_p), int(fp8)), "rdx_logits_test")
        return out, torch.tensor(list(am), dtype=torch.int32)

    # -- the decoder's 3-16-row / row-block GEMM kernels alone (include/rdx_dec_hooks.h). Inputs may be device tensors (used as they are, so one
    #    weight serves many calls); every output is pre-filled with NaN so that "not written" can be asserted ---------------------------------
    def _dev(self, t, dtype=None):
        return None if t is None else t.to(self.device, dtype or self.tdtype).contiguous()

    def _nan(self, *shape, dtype=None):
        return torch.full(shape, float("nan"), dtype=dtype or self.tdtype, device=self.device)

    def xstat16_test(self, x, norm_w, w, epi=0, eps=1e-6, n_valid=None, ldo=None, out_packed=0):
        """xstat16_k (rdx_xstat16_test): x [M, 4096], norm_w [4096], w fp32 [N, 4096]. Returns out [M, ldo] (epi 4: N / 2 columns), the raw packed
        block [N / 64, 2, 64, 8] for out_packed 1, or (logits, argmax int32[M]) for epi 5."""
        import ctypes
        M, N = x.shape[0], w.shape[0]
        x, nw, w = self._dev(x), self._dev(norm_w), self._dev(w, torch.float32)
        cols = N // 2 if epi == 4 else N
        ldo = ldo or cols
        out = self._nan(N // 64, 2, 64, 8) if out_packed else self._nan(M + 2, ldo)
        am = (ctypes.c_int32 * M)()
        torch.cuda.synchronize(self.device)
        check(self.ctx, self.lib.rdx_xstat16_test(self.ctx, _ptr(x), _ptr(nw), eps, _ptr(w), M, N, epi, N if n_valid is None else n_valid, _ptr(out),
                                                  ldo, out_packed, ctypes.cast(am, ctypes.c_void_p)), "rdx_xstat16_test")
        return (out, torch.tensor(list(am), dtype=torch.int32)) if epi == 5 else out

    def wcode_test(self, w):
        """The device encoder of the coded bf16 weights alone (rdx_wcode_test; the format: radialog_amd/wcode.py): w fp32 [N, K], K % 128 == 0. Returns
        (packed uint16 [tiles, K / 32, 64, 8], planes uint8 [tiles, K / 128, 3328], hdr uint32 [tiles]) as NumPy arrays."""
        from . import wcode
        N, K = w.shape
        nt = (N + 15) // 16
        w = self._dev(w, torch.float32)
        packed = torch.zeros(nt, K // 32, 64, 8, dtype=torch.int16, device=self.device)
        planes = torch.zeros(nt, K // wcode.CHUNK_K, wcode.CHUNK_BYTES, dtype=torch.uint8, device=self.device)
        hdr = torch.zeros(nt, dtype=torch.int32, device=self.device)
        torch.cuda.synchronize(self.device)
        check(self.ctx, self.lib.rdx_wcode_test(self.ctx, _ptr(w), N, K, _ptr(packed), _ptr(planes), _ptr(hdr)), "rdx_wcode_test")
        return packed.cpu().numpy().view("uint16"), planes.cpu().numpy(), hdr.cpu().numpy().view("uint32")

    def wcode_stats(self):
        """(tiles, fallback tiles, bytes, coded GEMV launches, coded chained launches) of this engine's decoder (rdx_wcode_stats): the coded bf16 weight
        copies it holds (zeros where it holds none) and how many launches of the coded kernels it has issued (a captured graph counts once)."""
        out = (C.c_longlong * 5)()
        check(self.ctx, self.lib.rdx_wcode_stats(self.ctx, out), "rdx_wcode_stats")
        return tuple(int(v) for v in out)

    def wcode_dense_test(self, w):
        """The dense words of the device encoder alone (rdx_wcode_dense_test; the definition: wcode.dense): w fp32 [N, K], K % 128 == 0. Returns uint32
        [tiles] as a NumPy array."""
        import numpy as np
        N, K = w.shape
        nt = (N + 15) // 16
        w = self._dev(w, torch.float32)
        out = (C.c_uint32 * nt)()
        torch.cuda.synchronize(self.device)
        check(self.ctx, self.lib.rdx_wcode_dense_test(self.ctx, _ptr(w), N, K, C.cast(out, C.c_void_p)), "rdx_wcode_dense_test")
        return np.array(out, dtype=np.uint32)

    def wcode_dense_words(self, unit, layer, tiles):
        """(hdr uint32 [tiles], dense uint32 [tiles]) of one coded copy of this engine's decoder (rdx_wcode_dense_words): unit 0 = QKV, 2 = gate/up,
        3 = down_proj of `layer`, 4 = lm_head."""
        import numpy as np
        out = (C.c_uint32 * (2 * tiles))()
        check(self.ctx, self.lib.rdx_wcode_dense_words(self.ctx, unit, layer, C.cast(out, C.c_void_p), tiles, None), "rdx_wcode_dense_words")
        a = np.array(out, dtype=np.uint32)
        return a[:tiles], a[tiles:]

    def wcode_dense_tiles(self):
        """The dense tiles over all coded copies of this engine's decoder: those the coded kernels decode without the zero test."""
        n = C.c_longlong(0)
        check(self.ctx, self.lib.rdx_wcode_dense_words(self.ctx, 0, 0, None, 0, C.byref(n)), "rdx_wcode_dense_words")
        return int(n.value)

    def w4_test(self, w):
        """The device quantiser of the int4 group-quantised weights alone (rdx_w4_test; the format: radialog_amd/w4.py): w fp32 [N, K], K % 128 == 0.
        Returns (wprime uint16 [tiles, K / 32, 64, 8], stream uint8 [tiles, K / 128, 1056], scales uint16 [tiles, K / 128, 16]) as NumPy arrays."""
        from . import w4 as w4fmt
        N, K = w.shape
        nt = (N + 15) // 16
        w = self._dev(w, torch.float32)
        wprime = torch.zeros(nt, K // 32, 64, 8, dtype=torch.int16, device=self.device)
        stream = torch.zeros(nt, max(K // w4fmt.CHUNK_K, 1), w4fmt.CHUNK_BYTES, dtype=torch.uint8, device=self.device)
        scales = torch.zeros(nt, max(K // w4fmt.CHUNK_K, 1), 16, dtype=torch.int16, device=self.device)
        torch.cuda.synchronize(self.device)
        check(self.ctx, self.lib.rdx_w4_test(self.ctx, _ptr(w), N, K, _ptr(wprime), _ptr(stream), _ptr(scales)), "rdx_w4_test")
        return wprime.cpu().numpy().view("uint16"), stream.cpu().numpy(), scales.cpu().numpy().view("uint16")

    def w4_stats(self):
        """(int4 tiles, raw tiles, bytes, int4 GEMV launches, int4 chained launches) of this engine's decoder (rdx_w4_stats): the int4 streams it holds
        (zeros where it holds none) and how many launches of the int4 kernels it has issued (a captured graph counts once)."""
        out = (C.c_longlong * 5)()
        check(self.ctx, self.lib.rdx_w4_stats(self.ctx, out), "rdx_w4_stats")
        return tuple(int(v) for v in out)

    def w4_rows_stats(self):
        """(int4 xstat16 launches, int4 xrow16 launches) the 3-16-row step of this engine has issued (rdx_w4_rows_stats; a captured graph counts once):
        QKV and gate/up on xstat16_w4_k, down_proj on xrow16_w4_k."""
        out = (C.c_longlong * 2)()
        check(self.ctx, self.lib.rdx_w4_rows_stats(self.ctx, out), "rdx_w4_rows_stats")
        return tuple(int(v) for v in out)

    def xstat16_w4_test(self, x, norm_w, w, epi=0, eps=1e-6, ldo=None, out_packed=0, raw_lo=None):
        """xstat16_w4_k (rdx_xstat16_w4_test): xstat16_test's arguments for epi 0 / 4; w fp32 [N, 4096] is quantised on the device (radialog_amd/w4.py),
        the tiles of rows >= raw_lo stay raw bf16 (raw_lo < 0: only the tile of rows [-raw_lo, -raw_lo + 16))."""
        M, N = x.shape[0], w.shape[0]
        x, nw, w = self._dev(x), self._dev(norm_w), self._dev(w, torch.float32)
        ldo = ldo or ((N + 15) // 16 * 8 if epi == 4 else N)          # N need not fill its last tile (epi 4 writes whole tiles of 8 columns)
        out = self._nan(N // 64, 2, 64, 8) if out_packed else self._nan(M + 2, ldo)
        torch.cuda.synchronize(self.device)
        check(self.ctx, self.lib.rdx_xstat16_w4_test(self.ctx, _ptr(x), _ptr(nw), eps, _ptr(w), M, N, epi, _ptr(out), ldo, out_packed,
                                                     N if raw_lo is None else raw_lo), "rdx_xstat16_w4_test")
        return out

    def xrow16_w4_test(self, x, w, resid, M=None, ldo=None):
        """xrow16_w4_k (rdx_xrow16_w4_test): xrow16_test's arguments, K % 128 == 0; w is quantised on the device, every tile int4."""
        packed = x.dim() == 4
        M = M if packed else x.shape[0]
        N, K = w.shape
        x, w, r = self._dev(x), self._dev(w, torch.float32), self._dev(resid)
        ldo = ldo or N
        out = self._nan(M + 2, ldo)
        torch.cuda.synchronize(self.device)
        check(self.ctx, self.lib.rdx_xrow16_w4_test(self.ctx, _ptr(x), int(packed), _ptr(w), _ptr(r), M, N, K, _ptr(out), ldo), "rdx_xrow16_w4_test")
        return out

    def xrow16_test(self, x, w, resid, M=None, ldo=None):
        """xrow16_k (rdx_xrow16_test): out [M + 2, ldo] = resid [M, N] + T(x w^T). x [M, K] row-major, or (4-d) the packed block [K / 32, 2, 64, 8]
        with M given."""
        packed = x.dim() == 4
        M = M if packed else x.shape[0]
        N, K = w.shape
        x, w, r = self._dev(x), self._dev(w, torch.float32), self._dev(resid)
        ldo = ldo or N
        out = self._nan(M + 2, ldo)
        torch.cuda.synchronize(self.device)
        check(self.ctx, self.lib.rdx_xrow16_test(self.ctx, _ptr(x), int(packed), _ptr(w), _ptr(r), M, N, K, _ptr(out), ldo), "rdx_xrow16_test")
        return out

    def xstat_blk_test(self, x, norm_w, w, epi=0, resid=None, eps=1e-6, n_valid=None, ldo=None, out_packed=0, want_xp=False):
        """launch_rmsnorm into row tiles + the row-block xstat32_k (rdx_xstat_blk_test): x [M, 4096], norm_w [4096] or None, w fp32 [N, 4096]. Returns
        (out, xp, argmax): out [M + 2, ldo] or the raw packed block [N / 64, mtiles, 64, 8] (out_packed 3); xp the norm's raw packed output
        [128, mtiles, 64, 8] (want_xp); argmax int32[M] (epi 5)."""
        import ctypes
        M, N = x.shape[0], w.shape[0]
        mtl = (M + 15) // 16
        x, nw, w, r = self._dev(x), self._dev(norm_w), self._dev(w, torch.float32), self._dev(resid)
        ldo = ldo or (N // 2 if epi == 4 else N)
        out = self._nan(N // 64, mtl, 64, 8) if out_packed else self._nan(M + 2, ldo)
        xp = self._nan(128, mtl, 64, 8) if want_xp else None
        am = (ctypes.c_int32 * M)()
        torch.cuda.synchronize(self.device)
        check(self.ctx, self.lib.rdx_xstat_blk_test(self.ctx, _ptr(x), _ptr(nw), eps, _ptr(w), _ptr(r), M, N, epi, N if n_valid is None else n_valid,
                                                    _ptr(out), ldo, out_packed, _ptr(xp), ctypes.cast(am, ctypes.c_void_p)), "rdx_xstat_blk_test")
        return out, xp, (torch.tensor(list(am), dtype=torch.int32) if epi == 5 else None)

    def xsplit_blk_test(self, x, w, resid=None, norm_w=None, eps=1e-6):
        """launch_rmsnorm (re-layout) + the row-block xsplit32_k [+ launch_rmsnorm with the slabs] (rdx_xsplit_blk_test): x [M, 11008], w fp32
        [N, 11008]. Returns (slabs fp32 [4, 16 mtiles, N], updated residual rows [M, 4096] or None, raw packed norm [128, mtiles, 64, 8] or None)."""
        M, N = x.shape[0], w.shape[0]
        mtl = (M + 15) // 16
        x, w, nw = self._dev(x), self._dev(w, torch.float32), self._dev(norm_w)
        slab = self._nan(4, 16 * mtl, N, dtype=torch.float32)
        r = None if resid is None else self._dev(resid).clone()
        xn = None if resid is None else self._nan(128, mtl, 64, 8)
        torch.cuda.synchronize(self.device)
        check(self.ctx, self.lib.rdx_xsplit_blk_test(self.ctx, _ptr(x), _ptr(w), _ptr(r), _ptr(nw), eps, M, N, _ptr(slab), _ptr(xn)), "rdx_xsplit_blk_test")
        return slab, r, xn

    def xstat_blk8_test(self, x, norm_w, w, epi=0, eps=1e-6, n_valid=None, ldo=None, out_packed=0):
        """launch_rmsnorm into e4m3 blocks + the fp8 row-block xstat32_k (rdx_xstat_blk8_test): x [M, 4096], norm_w [4096], w fp32 [N, 4096] (quantised to e4m3
        by the production packer). Returns (out, x8 uint8 [NB, 32 * 4096], xscale fp32 [32 NB], argmax or None); out [M + 2, ldo] or, out_packed 2,
        the raw blocks [NB, 32 * N / 2]."""
        import ctypes
        M, N = x.shape[0], w.shape[0]
        NB = (M + 31) // 32
        x, nw, w = self._dev(x), self._dev(norm_w), self._dev(w, torch.float32)
        ldo = ldo or (N // 2 if epi == 4 else N)
        out = self._nan(NB, 32 * (N // 2)) if out_packed else self._nan(M + 2, ldo)
        x8 = torch.full((NB, 32 * 4096), 0xff, dtype=torch.uint8, device=self.device)
        xs = self._nan(32 * NB, dtype=torch.float32)
        am = (ctypes.c_int32 * M)()
        torch.cuda.synchronize(self.device)
        check(self.ctx, self.lib.rdx_xstat_blk8_test(self.ctx, _ptr(x), _ptr(nw), eps, _ptr(w), M, N, epi, N if n_valid is None else n_valid, _ptr(out), ldo,
                                                     out_packed, _ptr(x8), _ptr(xs), ctypes.cast(am, ctypes.c_void_p)), "rdx_xstat_blk8_test")
        return out, x8, xs, (torch.tensor(list(am), dtype=torch.int32) if epi == 5 else None)

    def xsplit_blk8_test(self, x, w, resid=None, norm_w=None, eps=1e-6):
        """launch_rmsnorm (64-deep re-layout per 32-row block) + the fp8 row-block xsplit32_k [+ launch_rmsnorm into e4m3 blocks with the slabs]
        (rdx_xsplit_blk8_test): x [M, K], w fp32 [N, K], K 4096 / 11008. Returns (slabs fp32 [groups, 32 NB, N], updated residual rows or None)."""
        M, K = x.shape
        N = w.shape[0]
        NB = (M + 31) // 32
        x, w, nw = self._dev(x), self._dev(w, torch.float32), self._dev(norm_w)
        slab = self._nan(4 if K == 11008 else 2, 32 * NB, N, dtype=torch.float32)
        r = None if resid is None else self._dev(resid).clone()
        x8 = None if resid is None else torch.empty(NB, 32 * 4096, dtype=torch.uint8, device=self.device)
        xs = None if resid is None else self._nan(32 * NB, dtype=torch.float32)
        torch.cuda.synchronize(self.device)
        check(self.ctx, self.lib.rdx_xsplit_blk8_test(self.ctx, _ptr(x), _ptr(w), _ptr(r), _ptr(nw), eps, M, N, K, _ptr(slab), _ptr(x8), _ptr(xs)),
              "rdx_xsplit_blk8_test")
        return slab, r

    def rmsnorm_test(self, x, norm_w, layout, mtiles=0, slab=None, eps=1e-6, out_bytes=None, n_scales=0):
        """launch_rmsnorm alone (rdx_rmsnorm_test): x [rows, H], norm_w [H] or None (re-layout only), layout 0-5 (ActLayout, csrc/rdx_kernels.h), slab fp32
        [groups, rows the layout holds, H] or None. Returns (error message or None, raw output uint8 [out_bytes], scales fp32 [n_scales] or None, the
        updated copy of x); output and scales are 0xff bytes wherever the norm wrote nothing -- everywhere after a refusal, which does not raise."""
        rows, H = x.shape
        x, nw = self._dev(x).clone(), self._dev(norm_w)
        slab = self._dev(slab, torch.float32)
        out = torch.zeros(out_bytes or rows * H * 2, dtype=torch.uint8, device=self.device)
        xs = torch.zeros(n_scales, dtype=torch.float32, device=self.device) if n_scales else None
        torch.cuda.synchronize(self.device)
        rc = self.lib.rdx_rmsnorm_test(self.ctx, _ptr(x), _ptr(nw), eps, rows, H, layout, mtiles, _ptr(slab), 0 if slab is None else slab.shape[0], _ptr(out),
                                       out.numel(), _ptr(xs), n_scales)
        err = None
        if rc != 0:
            msg = self.lib.rdx_last_error(self.ctx)
            err = msg.decode() if msg else "?"
        return err, out, xs, x

    def _last_error(self):
        msg = self.lib.rdx_last_error(self.ctx)
        return msg.decode() if msg else "?"

    def decode_attn_test(self, qkv, kcache, vcache, slot, key_mask, k_perm, cur_rope=None, cos=None, sin=None, pos=None, lbq=None, lbv=None, lora_scale=1.0,
                         out_packed=0, out_mt=2, out_bytes=None):
        """launch_decode_attention alone (rdx_decode_attn_test): qkv [B, qkv_ld], kcache / vcache [B, heads, max_len, 128] (K in the order k_perm names), slot int
        [B], key_mask uint8 [B, max_len]; cur_rope [B, 2, 128], or cos / sin [max_pos, 128] with pos int [B]; lbq / lbv [128 heads, 8] switch LoRA on. Returns
        (error message or None, raw output uint8 [out_bytes], updated K cache, updated V cache); the caller's tensors are left as they are, and the output is
        0xff bytes wherever the kernel wrote nothing -- everywhere after a refusal, which does not raise."""
        B, heads, max_len = kcache.shape[:3]
        H = 128 * heads
        x, kc, vc = self._dev(qkv), self._dev(kcache).clone(), self._dev(vcache).clone()
        sl, km = self._dev(slot, torch.int32), self._dev(key_mask, torch.uint8)
        cr, ct, st, ps = self._dev(cur_rope), self._dev(cos), self._dev(sin), self._dev(pos, torch.int32)
        bq, bv = self._dev(lbq), self._dev(lbv)
        lora_r = 0 if lbq is None else 8
        if tuple(x.shape) != (B, (3 * H + 2 * lora_r + 15) // 16 * 16) or vc.shape != kc.shape or kc.shape[3] != 128 or sl.numel() != B or tuple(km.shape) != (B, max_len):
            raise ValueError("decode_attn_test: qkv [B, qkv_ld], caches [B, heads, max_len, 128], slot [B], key_mask [B, max_len]")
        if (cr is not None and tuple(cr.shape) != (B, 2, 128)) or (ps is not None and ps.numel() != B) or (bq is not None and (tuple(bq.shape) != (H, 8) or tuple(bv.shape) != (H, 8))):
            raise ValueError("decode_attn_test: cur_rope [B, 2, 128], pos [B], lbq / lbv [hidden, 8]")
        out = torch.full((B * H * 2 if out_bytes is None else out_bytes,), 0xff, dtype=torch.uint8, device=self.device)
        torch.cuda.synchronize(self.device)
        rc = self.lib.rdx_decode_attn_test(self.ctx, heads, B, max_len, int(k_perm), lora_r, float(lora_scale), _ptr(x), _ptr(bq), _ptr(bv), _ptr(cr), _ptr(ct), _ptr(st),
                                           0 if ct is None else ct.shape[0], _ptr(ps), _ptr(sl), _ptr(km), _ptr(kc), _ptr(vc), _ptr(out), out.numel(), int(out_packed),
                                           int(out_mt))
        return (None if rc == 0 else self._last_error()), out, kc, vc

    def decode_attn_kv8_test(self, qkv, kcodes, kexp, vcodes, vexp, slot, key_mask, cur_rope=None, cos=None, sin=None, pos=None, lbq=None, lbv=None, lora_scale=1.0,
                             out_packed=0, out_mt=2, out_bytes=None, guard=0):
        """launch_decode_attention_kv8 alone (rdx_decode_attn_kv8_test): decode_attn_test's arguments with the caches as kcodes / vcodes uint8 [B, heads, max_len,
        128] (K in the kernels' storage order: kv8.k_store) and kexp / vexp int8 [B, heads, max_len]. Returns (error or None, raw output uint8, kcodes, kexp,
        vcodes, vexp after the launch); each of the four is followed by `guard` bytes that were 0xff before the launch (flat uint8 tensors, the buffer first)."""
        B, heads, max_len = kcodes.shape[:3]
        H = 128 * heads
        x = self._dev(qkv)

        def guarded(t, dt):
            t = self._dev(t, dt).contiguous()
            buf = torch.full((t.numel() + guard,), 0xff, dtype=torch.uint8, device=self.device)
            buf[:t.numel()] = t.view(torch.uint8).reshape(-1)
            return buf
        kc, vc, ke, ve = guarded(kcodes, torch.uint8), guarded(vcodes, torch.uint8), guarded(kexp, torch.int8), guarded(vexp, torch.int8)
        sl, km = self._dev(slot, torch.int32), self._dev(key_mask, torch.uint8)
        cr, ct, st, ps = self._dev(cur_rope), self._dev(cos), self._dev(sin), self._dev(pos, torch.int32)
        bq, bv = self._dev(lbq), self._dev(lbv)
        lora_r = 0 if lbq is None else 8
        if tuple(x.shape) != (B, (3 * H + 2 * lora_r + 15) // 16 * 16) or vcodes.shape != kcodes.shape or kcodes.shape[3] != 128 or tuple(kexp.shape) != (B, heads, max_len) \
                or vexp.shape != kexp.shape or sl.numel() != B or tuple(km.shape) != (B, max_len):
            raise ValueError("decode_attn_kv8_test: qkv [B, qkv_ld], codes [B, heads, max_len, 128], exponents [B, heads, max_len], slot [B], key_mask [B, max_len]")
        out = torch.full((B * H * 2 if out_bytes is None else out_bytes,), 0xff, dtype=torch.uint8, device=self.device)
        torch.cuda.synchronize(self.device)
        rc = self.lib.rdx_decode_attn_kv8_test(self.ctx, heads, B, max_len, lora_r, float(lora_scale), _ptr(x), _ptr(bq), _ptr(bv), _ptr(cr), _ptr(ct), _ptr(st),
                                               0 if ct is None else ct.shape[0], _ptr(ps), _ptr(sl), _ptr(km), _ptr(kc), _ptr(ke), _ptr(vc), _ptr(ve), _ptr(out),
                                               out.numel(), int(out_packed), int(out_mt))
        return (None if rc == 0 else self._last_error()), out, kc, ke, vc, ve

    def kv8_quant_test(self, krows, vrows, T, max_len, slot0, kcodes, kexp, vcodes, vexp, guard=0):
        """launch_kv8_quant_rows alone (rdx_kv8_quant_test): krows / vrows [B, heads, stage_len, 128] model dtype; rows t < T go to positions slot0 + t of the
        codes [B, heads, max_len, 128] uint8 (K in the storage order) and exponents [B, heads, max_len] int8. Returns (error or None, kcodes, kexp, vcodes,
        vexp) as flat uint8 tensors, each followed by `guard` bytes that were 0xff before the launch."""
        B, heads, stage_len = krows.shape[:3]
        kr, vr = self._dev(krows), self._dev(vrows)

        def guarded(t, dt):
            t = self._dev(t, dt).contiguous()
            buf = torch.full((t.numel() + guard,), 0xff, dtype=torch.uint8, device=self.device)
            buf[:t.numel()] = t.view(torch.uint8).reshape(-1)
            return buf
        kc, vc, ke, ve = guarded(kcodes, torch.uint8), guarded(vcodes, torch.uint8), guarded(kexp, torch.int8), guarded(vexp, torch.int8)
        if vr.shape != kr.shape or kr.shape[3] != 128 or tuple(kcodes.shape) != (B, heads, max_len, 128) or vcodes.shape != kcodes.shape \
                or tuple(kexp.shape) != (B, heads, max_len) or vexp.shape != kexp.shape:
            raise ValueError("kv8_quant_test: rows [B, heads, stage_len, 128], codes [B, heads, max_len, 128], exponents [B, heads, max_len]")
        torch.cuda.synchronize(self.device)
        rc = self.lib.rdx_kv8_quant_test(self.ctx, heads, B, int(T), stage_len, int(max_len), int(slot0), _ptr(kr), _ptr(vr), _ptr(kc), _ptr(ke), _ptr(vc), _ptr(ve))
        return (None if rc == 0 else self._last_error()), kc, ke, vc, ve

    def rope_kv_test(self, qkv, pos_ids, cos, sin, slot0, kcache, vcache, k_perm, lbq=None, lbv=None, lora_scale=1.0):
        """launch_rope_kv_prefill alone (rdx_rope_kv_test): qkv [B, T, qkv_ld], pos_ids int [B, T], cos / sin [max_pos, 128], caches [B, heads, max_len, 128].
        Returns (error message or None, qout [B T, hidden] (0xff bytes where nothing was written), updated K cache, updated V cache)."""
        B, heads, max_len = kcache.shape[:3]
        T, H = qkv.shape[1], 128 * heads
        x, kc, vc = self._dev(qkv), self._dev(kcache).clone(), self._dev(vcache).clone()
        pi, ct, st, bq, bv = self._dev(pos_ids, torch.int32), self._dev(cos), self._dev(sin), self._dev(lbq), self._dev(lbv)
        lora_r = 0 if lbq is None else 8
        bad_b = bq is not None and (tuple(bq.shape) != (H, 8) or tuple(bv.shape) != (H, 8))
        if tuple(x.shape) != (B, T, (3 * H + 2 * lora_r + 15) // 16 * 16) or vc.shape != kc.shape or kc.shape[3] != 128 or tuple(pi.shape) != (B, T) or bad_b \
                or ct.shape != st.shape or ct.shape[1] != 128:
            raise ValueError("rope_kv_test: qkv [B, T, qkv_ld], pos_ids [B, T], cos / sin [max_pos, 128], caches [B, heads, max_len, 128], lbq / lbv [hidden, 8]")
        qout = torch.full((B * T * H * 2,), 0xff, dtype=torch.uint8, device=self.device)
        torch.cuda.synchronize(self.device)
        rc = self.lib.rdx_rope_kv_test(self.ctx, heads, B, T, max_len, int(k_perm), lora_r, float(lora_scale), _ptr(x), _ptr(bq), _ptr(bv), _ptr(ct), _ptr(st), ct.shape[0],
                                       _ptr(pi), int(slot0), _ptr(kc), _ptr(vc), _ptr(qout))
        return (None if rc == 0 else self._last_error()), qout.view(self.tdtype).view(B * T, H), kc, vc

    def classify_findings(self, image: torch.Tensor) -> torch.Tensor:
        """ChexpertClassifier.forward: float32[B,3,S,S] on the device -> float32[B,classes] logits."""
        image = image.to(self.device, torch.float32).contiguous()
        B = image.shape[0]
        out = torch.empty(B, self.cfg.cls.classes, dtype=torch.float32, device=self.device)
        torch.cuda.synchronize(self.device)
        check(self.ctx, self.lib.rdx_classify_findings(self.ctx, _ptr(image), B, _ptr(out)), "rdx_classify_findings")
        return out

    # -- data-parallel collective (RCCL inside the C ABI) ---------------------------------------------------------------
    def comm_unique_id(self) -> bytes:
        """128 opaque bytes from ncclGetUniqueId (rank 0); hand them to every rank, then comm_init everywhere."""
        buf = C.create_string_buffer(128)
        rc = self.lib.rdx_comm_unique_id(buf)
        if rc != 0:
            msg = self.lib.rdx_last_error(None)
            raise _lib.RdxError(f"rdx_comm_unique_id failed ({rc}): {msg.decode() if msg else '?'}")
        return buf.raw

    def comm_init(self, unique_id: bytes, rank: int, world: int):
        if len(unique_id) != 128:
            raise ValueError("the RCCL unique id is 128 bytes")
        buf = C.create_string_buffer(unique_id, 128)
        check(self.ctx, self.lib.rdx_comm_init(self.ctx, buf, rank, world), "rdx_comm_init")

    @property
    def comm_world(self) -> int:
        """Ranks of the RCCL communicator inside librdx (0: none, or switched off by the launcher with `comm_off = True` after a
        bring-up that did not succeed on every rank)."""
        return 0 if getattr(self, "comm_off", False) else int(self.lib.rdx_comm_world(self.ctx))

    def allgather_tokens(self, tokens: torch.Tensor) -> torch.Tensor:
        """int32[B_local, N] on this device -> int32[world * B_local, N], rank-major: one ncclAllGather on the engine's stream."""
        if tokens.dtype != torch.int32 or not tokens.is_cuda or tokens.dim() != 2:
            raise ValueError("allgather_tokens takes an int32 [rows, n] tensor on the engine's device")
        world = self.comm_world
        if world <= 0:
            raise _lib.RdxError("allgather_tokens: no communicator (comm_init / shard.init_comm first)")
        tokens = tokens.contiguous()
        out = torch.empty(world * tokens.shape[0], tokens.shape[1], dtype=torch.int32, device=self.device)
        torch.cuda.synchronize(self.device)
        check(self.ctx, self.lib.rdx_allgather_tokens(self.ctx, _ptr(tokens), _ptr(out), tokens.shape[0], tokens.shape[1]), "rdx_allgather_tokens")
        self.sync()
        return out

    def kernel_bench(self, rows, N, K, H=0, ksize=0, stride=1, epi=0, iters=20, trace_wgs=0):
        """ms per launch of one GEMM / NHWC convolution through the encoder's dispatch (rdx_kernel_bench); with trace_wgs also the
        int64 [trace_wgs, 8] per-workgroup timeline of gemm_dma_k (100 MHz ticks)."""
        ms = C.c_float(0)
        tr = torch.zeros(max(trace_wgs, 1), 8, dtype=torch.int64)
        check(self.ctx, self.lib.rdx_kernel_bench(self.ctx, rows, N, K, H, ksize, stride, epi, iters, C.byref(ms),
                                                  C.c_void_p(tr.data_ptr()) if trace_wgs else None, trace_wgs), "rdx_kernel_bench")
        return (ms.value, tr) if trace_wgs else ms.value

    def time_unit(self, what: int, iters: int) -> float:
        ms = C.c_float(0)
        check(self.ctx, self.lib.rdx_time(self.ctx, what, iters, C.byref(ms)), "rdx_time")
        return ms.value


    def attn_trace(self, layer: int):
        """Debug: 8 timestamps (100 MHz ticks) inside the stand-alone decode-attention kernel (workgroup 0,0)."""
        buf = torch.zeros(8, dtype=torch.int64)
        check(self.ctx, self.lib.rdx_attn_trace(self.ctx, layer, buf.data_ptr()), "rdx_attn_trace")
        return buf

    def gemv_trace(self, what: int, layer: int, max_tiles: int = 2048):
        """Debug: per-workgroup timestamps [tiles, 8] of one stand-alone decode GEMV (1 gate/up, 2 qkv, 4 down); what = 7: of the chained
        down(layer) -> QKV(layer + 1) launch inside ONE real eager decode step (advances the state; batch <= 2); what = 8 (_lib.TRACE_ATTN_OPROJ): of the
        fused attention + o_proj launch of `layer`, the same way (attention workgroups first; slots in include/rdx_hooks.h)."""
        buf = torch.zeros(max_tiles, 8, dtype=torch.int64)
        check(self.ctx, self.lib.rdx_gemv_trace(self.ctx, what, layer, buf.data_ptr(), max_tiles), "rdx_gemv_trace")
        return buf


# generate_queue's defaults: staging rows per session and free rows a refill waits for, by the measured table of profiles/r15_queue.md (stage 4;
# min_refill 2: 57.2 / 33.6 ms per request at 12 / 32 rows against 57.1 / 34.0 for 1 and 60.5 / 32.9 for 4)
QUEUE_STAGE = 4
QUEUE_MIN_REFILL = 2


class RowSession:
    """One open row session of an engine (rdx_rows_begin .. rdx_rows_end): the object a RowScheduler drives. Owns out_tokens [rows][cap]."""

    def __init__(self, eng: RdxEngine, rows: int, stage: int, cap: int, eos_id: int, pad_id: int, use_graph: bool = True):
        self.eng, self.rows, self.stage, self.cap = eng, int(rows), int(stage), int(cap)
        self.eos_id, self.pad_id, self.use_graph, self.max_len = int(eos_id), int(pad_id), bool(use_graph), eng.max_len
        self.tokens = torch.full((max(self.rows, 1), max(self.cap, 1)), self.pad_id, dtype=torch.int32, device=eng.device)
        self._logits = None                          # ONE [rows][vocab] buffer: a step with logits replays the same graph every time
        self._keep = None
        self.open = False
        torch.cuda.synchronize(eng.device)
        check(eng.ctx, eng.lib.rdx_rows_begin(eng.ctx, self.rows, self.stage, self.cap, self.eos_id, self.pad_id, _ptr(self.tokens)), "rdx_rows_begin")
        self.open = True

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def close(self):
        if self.open:
            self.open = False
            check(self.eng.ctx, self.eng.lib.rdx_rows_end(self.eng.ctx), "rdx_rows_end")

    def refill(self, ids, mask, qformer_embs, rows, want_logits: bool = False):
        """R prompts ids [R, T] (left-padded; mask [R, T] or None -> ids != pad_id) into the live rows `rows`. Returns their last-position logits
        [R, vocab] (model dtype) with want_logits, else None."""
        e = self.eng
        R, T = ids.shape
        rows_h = torch.as_tensor(list(rows), dtype=torch.int32)
        if rows_h.numel() != R:
            raise ValueError(f"refill: {R} prompts for {rows_h.numel()} rows")
        ids32 = ids.to(device=e.device, dtype=torch.int32).contiguous()
        m32 = None if mask is None else mask.to(device=e.device, dtype=torch.int32).contiguous()
        qf = None if qformer_embs is None else qformer_embs.to(device=e.device, dtype=torch.float32).contiguous()
        logits = torch.empty(R, e.cfg.llama.vocab, dtype=e.tdtype, device=e.device) if want_logits else None
        torch.cuda.synchronize(e.device)             # the inputs were written on torch's stream
        check(e.ctx, e.lib.rdx_rows_refill(e.ctx, _ptr(ids32), _ptr(m32), R, T, _ptr(qf), C.c_void_p(rows_h.data_ptr()), _ptr(logits)), "rdx_rows_refill")
        self._keep = (ids32, m32, qf, logits)        # alive until the stream has consumed them (the next refill syncs first)
        if want_logits:
            e.sync()
        return logits

    def step(self, n: int = 1, want_logits: bool = False):
        """n decode steps of all rows, enqueued without a sync. want_logits (n == 1 only): a copy of the step's logits [rows, vocab]."""
        e = self.eng
        if want_logits and self._logits is None:
            self._logits = torch.empty(self.rows, e.cfg.llama.vocab, dtype=e.tdtype, device=e.device)
            torch.cuda.synchronize(e.device)
        check(e.ctx, e.lib.rdx_rows_step(e.ctx, int(n), int(self.use_graph), _ptr(self._logits) if want_logits else None), "rdx_rows_step")
        if not want_logits:
            return None
        e.sync()
        return self._logits.clone()

    def poll(self):
        """(unfinished, steps) per row as lists, after draining the stream."""
        unf = torch.zeros(self.rows, dtype=torch.int32)
        steps = torch.zeros(self.rows, dtype=torch.int32)
        check(self.eng.ctx, self.eng.lib.rdx_rows_poll(self.eng.ctx, C.c_void_p(unf.data_ptr()), C.c_void_p(steps.data_ptr())), "rdx_rows_poll")
        return unf.tolist(), steps.tolist()

    def park(self, rows):
        rows_h = torch.as_tensor(list(rows), dtype=torch.int32)
        check(self.eng.ctx, self.eng.lib.rdx_rows_park(self.eng.ctx, C.c_void_p(rows_h.data_ptr()), int(rows_h.numel())), "rdx_rows_park")

    def read_tokens(self, row: int) -> torch.Tensor:
        """The row's out_tokens [cap] on the host (drains the stream first)."""
        self.eng.sync()
        return self.tokens[row].cpu()


def synth_getter(cfg: RaDialogCfg, device, lora: bool = True) -> Callable[[str], torch.Tensor]:
    """Lazy deterministic random-init weights (radialog_amd.synth), generated on `device` one tensor at a time."""
    from . import synth
    specs: Dict[str, tuple] = {}
    specs.update(synth.vision_specs(cfg.vision))
    specs.update(synth.qformer_specs(cfg.qformer))
    specs.update(synth.llama_specs(cfg.llama, lora=lora))
    specs.update(synth.classifier_specs(cfg.vision, cfg.cls))       # `biovil_encoder.*`, fc1, fc2 (classifier contexts)

    def get(name: str) -> torch.Tensor:
        shape, gen = specs[name]
        return gen(name, shape, device)

    return get
