"""The greedy search's logits rules restated in plain torch on the CPU, from their definition (include/rdx.h, rdx_logits_rules): what
select_step_k (radialog_amd/csrc/elem.hip) must reproduce bit for bit. Order: repetition penalty, n-gram ban, min-new-tokens, argmax.

    x        [B, V] tensor in the model dtype (fp16 / bf16): one logits row per batch row
    hists    B lists of token ids: the prompt as passed (pads and <IMG> ids included) followed by every token selected so far
    n_gen    B ints: tokens the row has generated (what min_new_tokens compares with)
    rules    (repetition_penalty, no_repeat_ngram_size, min_new_tokens); (1.0, 0, 0) changes nothing

`apply_rules` returns (processed [B, V] in x's dtype, tokens int64 [B]); x itself is left alone."""
import torch

NEUTRAL = (1.0, 0, 0)


def penalise(row: torch.Tensor, hist, p: float) -> torch.Tensor:
    """Every DISTINCT token of the history once: x < 0 ? x * p : x / p in fp32 (p rounded to fp32, IEEE division), then ONE round-to-nearest-even to
    the row's dtype -- what torch.where(score < 0, score * p, score / p) gives on a CPU tensor of that dtype."""
    out = row.clone()
    ids = sorted({int(t) for t in hist if 0 <= int(t) < row.numel()})
    if not ids:
        return out
    idx = torch.tensor(ids, dtype=torch.long)
    x32 = row[idx].to(torch.float32)
    p32 = torch.tensor(p, dtype=torch.float32)
    out[idx] = torch.where(x32 < 0, x32 * p32, x32 / p32).to(row.dtype)
    return out


def banned_ngram_tokens(hist, n: int):
    """Tokens that would complete an n-gram already in the history: with L = len(hist) and L + 1 >= n, every hist[j + n - 1] whose n - 1 predecessors
    hist[j .. j + n - 2] equal the last n - 1 tokens of the history (j + n - 1 < L). n = 1 bans every token of the history."""
    L = len(hist)
    if n <= 0 or L + 1 < n:
        return []
    tail = list(hist[L - n + 1:]) if n > 1 else []
    return sorted({int(hist[j + n - 1]) for j in range(L - n + 1) if list(hist[j:j + n - 1]) == tail})


def apply_rules(x: torch.Tensor, hists, n_gen, rules=NEUTRAL, eos_id: int = -1):
    p, n, m = rules
    B, V = x.shape
    out = x.clone()
    for b in range(B):
        row = out[b]
        if float(p) != 1.0:
            row = penalise(row, hists[b], float(p))
        for t in banned_ngram_tokens(hists[b], int(n)):
            if 0 <= t < V:
                row[t] = float("-inf")
        if m > 0 and eos_id >= 0 and int(n_gen[b]) < m and eos_id < V:
            row[eos_id] = float("-inf")
        out[b] = row
    return out, greedy_argmax(out)


def greedy_argmax(x: torch.Tensor) -> torch.Tensor:
    """argmax of every row with the LOWEST index on ties, spelled out (torch.argmax documents no tie rule for every backend)."""
    x32 = x.to(torch.float32)
    best = x32.max(dim=1, keepdim=True).values
    V = x.shape[1]
    idx = torch.arange(V).expand_as(x32)
    return torch.where(x32 == best, idx, torch.full_like(idx, V)).min(dim=1).values
