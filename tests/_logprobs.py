"""Restatement of the generation log-probs (include/rdx.h: rdx_set_logprobs, logprob_step_k) for the tests, in float64 on the model-dtype scores rows.

  chosen(x [M, V], tok [M]) -> float64 [M]: log_softmax(x)[tok].
  top_ids(x, n) -> int64 [M, n]: the n columns with the largest value, descending, lowest index on ties -- by EXACT value (the rows are model-dtype numbers,
      so there is nothing to tolerate), then by index. -inf columns follow the finite ones; NaN columns never enter; a slot without a candidate holds -1.
  top_lp(x, ids) -> float64 [M, n]: log_softmax(x) at those columns, 0.0 at a -1 slot.
  entries(scores [n, B, V], tokens [B, n], k): the three of them for every (row, step) of a generate() call.

The kernel's bar (logprob_bar) is _score.score_rows_bar's formula, DERIVED from the fp32 operations of the definition and not from what the kernel gives. With
u = 2^-24, x the row, m its maximum, c the column the entry describes (the token, or a top column), lp its log-prob:
  1. d = fl(x_c - m): exact model-dtype operands, one rounding: u |d|.
  2. the arguments fl(x_i - m) carry a relative error u each, which exp turns into u |a_i| of the term; summed with the softmax weights: <= u log V of S.
  3. expf: E_EXP ulp per term, relative 2 u E_EXP.
  4. the sum. logprob_step_k keeps element i of the row at LDS element i whatever the row's address, and thread t of 256 adds the terms of the 8-element
     groups t, t + 256, ... of that index space one element after the other: a thread owns at most ceil(ceil(V / 8) / 256) groups, so its chain is
     n_ser = 8 ceil(ceil(V / 8) / 256) serial additions (128 for V = 32001, 8 for V <= 2048); a tree of 8 levels joins the 256 partial sums: (n_ser + 8) u.
     (The head / 16-byte pieces / tail walk only decides which thread LOADS an element; it adds nothing.)
  5. logf: E_LOG ulp of its result, 2 u E_LOG |log S|; and the relative error of S becomes an absolute one.
  6. the final subtraction: u |lp|.
  bar = u (|d| + |lp| + 2 E_LOG |log S|) + u (log V + 2 E_EXP + n_ser + 8) per entry; 0 where the result is exact (-inf, a -1 slot).
The arg-max rounds of the top-n compare exact values: no error, hence no bar on the ids.
"""
import math

import torch

import _score as S

U, E_EXP, E_LOG = S.U, S.E_EXP, S.E_LOG
MAX_TOP = 8


def n_ser(V):
    """The longest serial chain of additions of one thread of logprob_step_k: 8 elements per group, ceil(groups / 256) groups."""
    return 8 * math.ceil(math.ceil(V / 8) / 256)


def chosen(x, tok):
    lsm = torch.log_softmax(x.double(), dim=-1)
    return lsm.gather(-1, tok.to(torch.int64).unsqueeze(-1)).squeeze(-1)


def top_ids(x, n):
    M, V = x.shape
    out = torch.full((M, n), -1, dtype=torch.int64)
    if n == 0:
        return out
    xd = x.double()
    nan = torch.isnan(xd)
    key = torch.where(nan, torch.full_like(xd, float("-inf")), xd)
    order = torch.sort(key, dim=-1, descending=True, stable=True).indices          # stable: equal values keep their index order
    for r in range(M):
        o = order[r]
        if bool(nan[r].any()):
            o = o[~nan[r][o]]
        o = o[:n]
        out[r, : o.numel()] = o
    return out


def top_lp(x, ids):
    lsm = torch.log_softmax(x.double(), dim=-1)
    picked = lsm.gather(-1, ids.clamp(min=0))
    return torch.where(ids < 0, torch.zeros_like(picked), picked)


def logprob_bar(x, col):
    """The derived bar of the entries of columns col [M] or [M, n] (float64, the shape of col); 0 for a -1 slot and wherever the result is not finite."""
    xd = x.double()
    V = x.shape[1]
    c2 = col.to(torch.int64).reshape(x.shape[0], -1)
    m = xd.max(dim=-1, keepdim=True).values
    xc = xd.gather(-1, c2.clamp(min=0))
    d = (xc - m).abs()
    log_s = torch.logsumexp(xd - m, dim=-1, keepdim=True).abs()
    lp = torch.log_softmax(xd, dim=-1).gather(-1, c2.clamp(min=0)).abs()
    bar = U * (d + lp + 2 * E_LOG * log_s) + U * (math.log(V) + 2 * E_EXP + n_ser(V) + 8)
    bar = torch.where(torch.isfinite(bar), bar, torch.zeros_like(bar))
    bar = torch.where(c2 < 0, torch.zeros_like(bar), bar)
    return bar.reshape(col.shape)


def entries(scores, tokens, k):
    """generate()'s scores [n, B, V] and tokens [B, >= n] -> (chosen float64 [B, n], ids int64 [B, n, k], lp float64 [B, n, k], bar_chosen, bar_top)."""
    n, B, V = scores.shape
    x = scores.permute(1, 0, 2).reshape(B * n, V).cpu()
    tok = tokens[:, :n].reshape(-1).cpu().to(torch.int64)
    ids = top_ids(x, k)
    return (chosen(x, tok).view(B, n), ids.view(B, n, k), top_lp(x, ids).view(B, n, k), logprob_bar(x, tok).view(B, n), logprob_bar(x, ids).view(B, n, k))


within = S.within


# ---- the kernel test's inputs (shared by the host and the GPU test) -----------------------------------------------------------------------------------------
KERNEL_CASES = [(B, V) for B in (1, 3, 130) for V in (32001, 32000, 4099, 8)]
MAX_NEW = 3           # of the kernel cases: row b describes step b % 4, and step 3 == max_new must write nothing


def kernel_case(B, V, dtype, seed=0):
    """_score.kernel_case's rows (random with the token at V - 1 / at 0, all equal, -inf entries, +-60000, a row of NaN, random) as padded rows xp [B, ld] with
    NaN / +65504 pad columns, plus exact ties at the top: in every 7th row (kind 6; with B == 1 in row 0) the columns V - 1, 0 and V // 2 (and 1 where V > 3)
    share one value above every other. tokens [B]: the targets, 0 for the NaN row (whose entries are NaN / -1)."""
    xp, tgt = S.kernel_case(B, V, dtype, seed)
    x = xp.float()
    for r in range(B):
        if r % 7 == 6 or B == 1:
            for c in {V - 1, 0, V // 2, 1 if V > 3 else 0}:
                x[r, c] = 24.0
    tok = torch.where(tgt == -100, torch.zeros_like(tgt), tgt)
    return x.to(dtype), tok


def d_steps(B):
    return torch.tensor([1 + b % (MAX_NEW + 1) for b in range(B)], dtype=torch.int32)


def lay_out(xp, V, strided, offset=0):
    """The case's rows as the kernel addresses them. strided False: one [B][ld] block (row stride ld, step stride 0, pad columns between the rows). True: the
    captured-with-scores form [MAX_NEW][B][V] (row stride V: odd starts for odd V; step stride B V), row b at step d_step[b] - 1, everything else NaN.
    Returns (flat buffer behind `offset` leading NaN elements, row_stride, step_stride)."""
    B, ld = xp.shape
    if not strided:
        flat, rs, ss = xp.reshape(-1), ld, 0
    else:
        buf = torch.full((MAX_NEW, B, V), float("nan"), dtype=xp.dtype)
        ds = d_steps(B)
        for b in range(B):
            if ds[b] - 1 < MAX_NEW:
                buf[int(ds[b]) - 1, b] = xp[b, :V]
        flat, rs, ss = buf.reshape(-1), V, B * V
    return torch.cat([torch.full((offset,), float("nan"), dtype=xp.dtype), flat]), rs, ss


# ---- fp32 emulation of logprob_step_k's order --------------------------------------------------------------------------------------------------------------
def emulate_kernel(xp, tok, V, top_n, elem0=0, fault=None):
    """xp [M, ld] padded rows, tok [M]. The kernel in fp32: the maximum (NaN never compares greater), thread k of 256 summing exp(x - m) over the groups k,
    k + 256, ... of 8 elements in index order, the 256-leaf tree (leaf i joins i + 128, then + 64, ...), (x_c - m) - log S for the token and the top-n columns
    picked by exact value, then index. elem0: the row's first element relative to a 16-byte boundary (0 .. 7) -- it matters to the planted faults only:
      "drop"  the 16-byte piece of memory that holds the maximum never reaches LDS (read as -inf),
      "head"  the scalar head in front of the first 16-byte boundary is skipped (read as -inf; needs elem0 != 0),
      "label" the token off by one,
      "pads"  the pad columns V .. ld - 1 take part.
    Returns (chosen float32 [M], ids int64 [M, top_n], lp float32 [M, top_n])."""
    M, ld = xp.shape
    W = ld if fault == "pads" else V
    ninf = torch.tensor(float("-inf"))
    out_c = torch.zeros(M, dtype=torch.float32)
    out_i = torch.full((M, top_n), -1, dtype=torch.int64)
    out_l = torch.zeros(M, top_n, dtype=torch.float32)
    head = (8 - elem0) % 8
    for r in range(M):
        row = xp[r, :W].float().clone()
        if fault == "head":
            row[:head] = ninf
        if fault == "drop":
            am = int(torch.where(torch.isnan(row), ninf, row).argmax())
            if am >= head:
                lo = head + (am - head) // 8 * 8
                row[lo: lo + 8] = ninf
            else:
                row[:head] = ninf
        m = torch.where(torch.isnan(row), ninf, row).max()
        e = torch.exp(row - m)
        ng = (W + 7) // 8
        e = torch.cat([e, torch.zeros(ng * 8 - W)]).view(ng, 8)
        part = torch.zeros(256, dtype=torch.float32)
        for g0 in range(0, ng, 256):
            blk = e[g0: g0 + 256]
            for j in range(8):
                part[: blk.shape[0]] = part[: blk.shape[0]] + blk[:, j]
        o = 128
        while o > 0:
            part[:o] = part[:o] + part[o: 2 * o]
            o //= 2
        log_s = torch.log(part[0])
        t = int(tok[r]) + (1 if fault == "label" else 0)
        out_c[r] = (row[t] - m) - log_s if t < W else float("nan")
        ids = top_ids(row.unsqueeze(0), top_n)[0]
        out_i[r] = ids
        vals = row[ids.clamp(min=0)]
        out_l[r] = torch.where(ids < 0, torch.zeros(()), (vals - m) - log_s)
    return out_c, out_i, out_l
