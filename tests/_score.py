"""Restatement of the scoring pass (include/rdx.h: rdx_score, score_rows_k) for the tests, in float64 on the model-dtype logits.

  token_logprobs(logits [B, T, V], labels [B, T]) -> float64 [B, T]: at t >= 1 with labels[b, t] != -100, log_softmax(logits[b, t - 1])[labels[b, t]];
                                                    0 at every other entry (the shift by one and HF's ignore_index).
  loss(logits, labels) -> float64 scalar: the mean of -token_logprobs over the counted entries, NaN when nothing is counted (CrossEntropyLoss).
  row_logprob / row_top1: the kernel's definition on single rows [M, V] with targets [M] (-100 -> (0.0, -1)); ties: the lowest index.

The kernel's bar (score_rows_bar) is DERIVED here from the fp32 operations of the definition, not from what the kernel gives. With u = 2^-24 (half an
fp32 ulp, relative), V the vocabulary, x the row, m its maximum, t the target:
  1. d = fl(x_t - m): both operands are exact model-dtype values of magnitude <= 65504 (fp16; bf16 logits are far smaller), so |d| <= 2 x 65504 and the
     one rounding costs at most u |d|.
  2. the arguments a_i = fl(x_i - m) <= 0 carry a relative error u each; exp turns it into a relative error u |a_i| of the term. Summed with the weights
     p_i = e_i / S this is u sum p_i |a_i| = u (H(p) - log S) <= u log V  (H: the entropy of the row's softmax) -- relative to S.
  3. expf: E_EXP ulp per term (the device library's expf is documented at 1 ulp; 2 is taken), relative 2 u E_EXP.
  4. the sum of non-negative terms: thread k adds its 16-byte pieces k, k + 256, ... element by element -- at most n_ser = 8 ceil(ceil(V / 8) / 256)
     serial additions -- and a tree of 8 levels joins the 256 partial sums: relative (n_ser + 8) u.
  5. logf: E_LOG ulp of its result (documented 1 ulp; 2 taken): 2 u E_LOG |log S|; and it turns the relative error r_S of S (2. to 4.) into an absolute r_S.
  6. the final subtraction: u |logprob|.
  bar = u (|d| + |logprob| + 2 E_LOG |log S|) + u (log V + 2 E_EXP + n_ser + 8), evaluated per row from the float64 restatement.
For V = 32001 and ordinary logits that is about 1e-5; a dropped 16-byte piece moves S by 8 / 32001 = 2.5e-4 at equal logits.
"""
import math

import torch

E_EXP, E_LOG = 2, 2
U = 2.0 ** -24


def token_logprobs(logits, labels):
    lg = logits.double()
    B, T, V = lg.shape
    labels = labels.to(torch.int64)
    out = torch.zeros(B, T, dtype=torch.float64)
    lsm = torch.log_softmax(lg[:, :-1], dim=-1)
    tgt = labels[:, 1:]
    counted = tgt != -100
    picked = lsm.gather(-1, tgt.clamp(min=0).unsqueeze(-1)).squeeze(-1)
    out[:, 1:] = torch.where(counted, picked, torch.zeros_like(picked))
    return out


def loss(logits, labels):
    lp = token_logprobs(logits, labels)
    counted = labels[:, 1:] != -100
    n = int(counted.sum())
    if n == 0:
        return torch.tensor(float("nan"), dtype=torch.float64)
    return -(lp[:, 1:][counted].sum()) / n


def row_top1(x, target):
    """x [M, V] (only the real columns), target [M]: argmax with the lowest index on ties, -1 for ignored rows."""
    xd = x.double()
    m = xd.max(dim=-1, keepdim=True).values
    V = x.shape[1]
    idx = torch.where(xd == m, torch.arange(V).expand_as(xd), torch.full_like(xd, V, dtype=torch.int64)).min(dim=-1).values
    return torch.where(target == -100, torch.full_like(idx, -1), idx)


def row_logprob(x, target):
    xd = x.double()
    lsm = torch.log_softmax(xd, dim=-1)
    picked = lsm.gather(-1, target.clamp(min=0).to(torch.int64).unsqueeze(-1)).squeeze(-1)
    return torch.where(target == -100, torch.zeros_like(picked), picked)


def score_rows_bar(x, target):
    """The derived bar of every row (float64 [M]); 0 for ignored rows (their result is exact)."""
    xd = x.double()
    V = x.shape[1]
    m = xd.max(dim=-1).values
    xt = xd.gather(-1, target.clamp(min=0).to(torch.int64).unsqueeze(-1)).squeeze(-1)
    d = (xt - m).abs()
    log_s = torch.logsumexp(xd - m.unsqueeze(-1), dim=-1).abs()
    lp = row_logprob(x, target).abs()
    n_ser = 8 * math.ceil(math.ceil(V / 8) / 256)
    bar = U * (d + lp + 2 * E_LOG * log_s) + U * (math.log(V) + 2 * E_EXP + n_ser + 8)
    bar = torch.where(torch.isfinite(bar), bar, torch.zeros_like(bar))        # a -inf target: the result is -inf exactly
    return torch.where(target == -100, torch.zeros_like(bar), bar)


def within(got, want, bar):
    """Element-wise: |got - want| <= bar, with non-finite values required to be equal (-inf == -inf)."""
    got, want = got.double(), want.double()
    fin = torch.isfinite(want)
    ok_fin = fin & torch.isfinite(got) & ((got - want).abs() <= bar)
    ok_inf = ~fin & ((got == want) | (torch.isnan(got) & torch.isnan(want)))
    return ok_fin | ok_inf


# ---- the kernel test's inputs and the emulation of the kernel's reduction order (shared by the host and the GPU test) --------------------------------
KERNEL_CASES = [(M, V) for M in (1, 3, 130) for V in (32001, 32000, 4099, 8)]


def pad_ld(V):
    return (V + 63) // 64 * 64


def kernel_case(M, V, dtype, seed=0):
    """logits [M, ld] in `dtype` with pad columns alternating NaN / +65504 (bf16: the nearest value), targets [M]. Row kinds cycle: random (target
    V - 1), random (target 0), all equal, -inf entries, +-60000, ignored row full of NaN, random with a random target. M == 1: the first kind only."""
    g = torch.Generator().manual_seed(1000 * M + V + seed)
    ld = pad_ld(V)
    x = torch.empty(M, ld, dtype=torch.float32)
    x[:, :V] = torch.randn(M, V, generator=g) * 3.0
    tgt = torch.randint(0, V, (M,), generator=g, dtype=torch.int64)
    for r in range(M):
        kind = r % 7
        if kind == 0:
            tgt[r] = V - 1
        elif kind == 1:
            tgt[r] = 0
        elif kind == 2:
            x[r, :V] = 1.25
        elif kind == 3:
            x[r, torch.randperm(V, generator=g)[: max(V // 3, 1)]] = float("-inf")
            if not torch.isfinite(x[r, :V]).any():
                x[r, 0] = 0.5
        elif kind == 4:
            x[r, :V] = torch.where(torch.rand(V, generator=g) < 0.5, torch.tensor(60000.0), torch.tensor(-60000.0))
            x[r, int(tgt[r])] = 60000.0 if r % 2 else -60000.0
            x[r, (int(tgt[r]) + 1) % V] = 60000.0
        elif kind == 5:
            x[r, :V] = float("nan")
            tgt[r] = -100
    pad = torch.arange(ld - V)
    x[:, V:] = torch.where(pad % 2 == 0, torch.tensor(float("nan")), torch.tensor(65504.0)).expand(M, ld - V)
    return x.to(dtype), tgt


def emulate_kernel(xp, target, V, fault=None):
    """fp32 emulation of score_rows_k's reduction order on the padded rows xp [M, ld]: thread k of 256 owns the 16-byte pieces k, k + 256, ...; the max /
    argmax and the sum are 256-leaf trees (leaf i joins i + 128, then + 64, ...). fault: None, or one of the planted faults
    "pads" (pad columns summed and searched), "drop" (the 16-byte piece that holds the maximum left out), "label" (the target off by one),
    "maxld" (the maximum taken over ld instead of vocab). Returns (logprob float32 [M], top1 int64 [M])."""
    M, ld = xp.shape
    x = xp.float()
    nch = ld // 8 if fault == "pads" else (V + 7) // 8
    width = nch * 8
    cols = torch.arange(width)
    lp = torch.zeros(M, dtype=torch.float32)
    t1 = torch.full((M,), -1, dtype=torch.int64)
    for r in range(M):
        tg = int(target[r])
        if tg == -100:
            continue
        row = x[r, :width].clone()
        valid = torch.ones(width, dtype=torch.bool) if fault == "pads" else cols < V
        if fault == "drop":
            am = int(torch.where(valid, row, torch.tensor(float("-inf"))).nan_to_num(nan=float("-inf")).argmax())
            valid = valid & ((cols // 8) != am // 8)
        mrow = torch.where(valid, row, torch.tensor(float("-inf")))
        mrow_nonan = torch.where(torch.isnan(mrow), torch.tensor(float("-inf")), mrow)      # x > bv is false for NaN
        m = mrow_nonan.max()
        if fault == "maxld":
            full = x[r]
            m = torch.where(torch.isnan(full), torch.tensor(float("-inf")), full).max()
        hits = (mrow_nonan == m).nonzero()
        t1[r] = int(hits[0]) if len(hits) else -1
        e = torch.where(valid, torch.exp(row - m), torch.zeros(()))                          # fp32 exp of the fp32 difference
        # thread k: pieces k, k + 256, ... in order, elements in order
        pieces = e.view(nch, 8)
        part = torch.zeros(256, dtype=torch.float32)
        for k0 in range(0, nch, 256):
            blk = pieces[k0:k0 + 256]
            for j in range(8):
                part[: blk.shape[0]] = part[: blk.shape[0]] + blk[:, j]
        o = 128
        while o > 0:
            part[:o] = part[:o] + part[o:2 * o]
            o //= 2
        tq = tg + 1 if fault == "label" else tg
        xt = x[r, tq] if tq < ld else torch.tensor(float("nan"))
        lp[r] = (xt - m) - torch.log(part[0])
    return lp, t1
