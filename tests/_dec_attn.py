"""Decode attention (csrc/attn_body.h) and the prompt's RoPE / KV write (csrc/attn.hip rope_kv_prefill_k) restated in plain torch on the CPU, with the inputs
and the bar of tests/test_decode_attn_ref.py (CPU: the restatement is exact where it claims to be, and the bar sees a dropped or misplaced position) and
tests/test_gpu_decode_attn.py (the kernels themselves).

THE RESTATEMENT follows the rounding points listed at the top of attn_body.h, T = the model dtype:
  new token   q += T(T(B_q a_q) scale), v alike (peft LoRA un-merged); q' = T(T(q cos) + T(rotate_half(q) sin)), k' alike
  scores      s_j = T(T(q' . k_j) / sqrt(128)), the divisor being the fp32 value of the square root; -inf where the mask byte is zero
  softmax     over the cached positions j < slot and the new one, P rounded to T
  output      sum_j P_j v_j, rounded to T by the kernel
Every function takes `prec` (torch.float32 or torch.float64) and runs the same operations in it.

THE INPUTS lie on dyadic grids, so that every value the kernel forms in fp32 before a rounding to T is exact, whatever the summation order and whether or not
multiply-adds are contracted: q, k, v and the cached K rows are multiples of 1/8 in [-1, 1] (hot rows: up to +-2), LoRA A values and B rows multiples of 1/4,
lora_scale a power of two, "cos" and "sin" drawn from {0, +-1, +-1/2} (the kernels only multiply by them); the cached V rows are arbitrary T values in (-1, 1).
test_decode_attn_ref.py holds fp32 against fp64 bit for bit on these families. q', the appended cache rows and the scores are therefore EXACT.

THE BAR for the attention output is derived, not tuned (the form of test_flash_prefill_and_attention_k_agree): the kernel's fp32 softmax may round a
probability to the other neighbour in T, so |out - ref| <= sum_j ulp_T(P_j) [P_j > 0] |v_j| + ulp_T(ref), ref = the fp64 sum of T(P_j) v_j.

HOT POSITIONS. With flat probabilities that bar hides a dropped position in bf16 (ulp_T(P) is P / 128 or more, and a thousand of them add up to more than one
P). Every (row, head) pair therefore has one hot position that carries a fifth to a half of the mass: its K row is +-a (a grid value up to 2) with the sign
of q' on as many dims as it takes, grid noise on the others. The hot position may be the new token itself; its raw k is then solved through the RoPE, whose cos / sin
row is drawn for that row from the invertible half of the set (exactly one of cos, sin is +-1 per dim pair)."""
import math

import torch

from _dec_gemm import DT, ulp  # noqa: F401  (DT re-exported)

D = 128
SQRT_D = float(torch.tensor(float(D), dtype=torch.float32).sqrt())          # the fp32 value the kernel divides by
LORA_SCALE = 0.25
SHARE_LO, SHARE_HI = 0.2, 0.5


def qkv_ld(heads, lora):
    return (3 * D * heads + (16 if lora else 0) + 15) // 16 * 16


# ---- the K cache order, restated from the comment in rdx_common.h: every group of 16 positions is stored [dim / 32][g = (dim % 32) / 8][r = pos % 16][8] ----
def kperm_offset(pos, dim):
    """Element offset of (pos, dim) inside one (row, head) slab in the fragment order."""
    return (pos // 16) * 2048 + (((dim // 32) * 64 + ((dim % 32) // 8) * 16 + pos % 16) * 8) + dim % 8


def k_permute(rows, perm=1):
    """[..., L, 128] row-major -> the slab in storage order (same shape, L % 16 == 0)."""
    if not perm:
        return rows
    lead, L, n = rows.shape[:-2], rows.shape[-2], rows.dim() - 2
    r = rows.reshape(*lead, L // 16, 16, 4, 4, 8)                           # [group][r][dim / 32][g][8]
    return r.permute(*range(n), n, n + 2, n + 3, n + 1, n + 4).reshape(*lead, L, D)


def k_unpermute(slab, perm=1):
    if not perm:
        return slab
    lead, L, n = slab.shape[:-2], slab.shape[-2], slab.dim() - 2
    r = slab.reshape(*lead, L // 16, 4, 4, 16, 8)                           # [group][dim / 32][g][r][8]
    return r.permute(*range(n), n, n + 3, n + 1, n + 2, n + 4).reshape(*lead, L, D)


# ---- the restatement ------------------------------------------------------------------------------------------------------------------------------------
def rot_half(x):
    return torch.cat((-x[..., D // 2:], x[..., :D // 2]), dim=-1)


def new_token(x, heads, dt, prec, cos, sin, lbq=None, lbv=None, scale=LORA_SCALE):
    """x [N, qkv_ld] (q | k | v | A_q | A_v), cos / sin [N, 128], lbq / lbv [hidden, 8] or None -> q', k', v' [N, heads, 128] in prec (T values)."""
    H = D * heads

    def R(t):
        return t.to(dt).to(prec)
    q, k, v = (x[:, i * H:(i + 1) * H].to(prec) for i in range(3))
    if lbq is not None:
        aq, av = x[:, 3 * H:3 * H + 8].to(prec), x[:, 3 * H + 8:3 * H + 16].to(prec)
        q = R(q + R(R(aq @ lbq.to(prec).t()) * scale))
        v = R(v + R(R(av @ lbv.to(prec).t()) * scale))
    q, k, v = (t.reshape(-1, heads, D) for t in (q, k, v))
    c, s = cos.to(prec)[:, None], sin.to(prec)[:, None]
    q = R(R(q * c) + R(rot_half(q) * s))
    k = R(R(k * c) + R(rot_half(k) * s))
    return q, k, v


def raw_dots(q, kall, order=0):
    """q [N, h, 128], kall [N, h, L, 128] -> q . k_j [N, h, L], summed pairwise (torch's own order) or, order 1, sequentially from the last dim down."""
    prod = q[:, :, None, :] * kall
    return prod.sum(-1) if order == 0 else prod.flip(-1).cumsum(-1)[..., -1]


def scores(dots, mask, dt):
    """T(T(dots) / sqrt(128)) in the precision of dots; -inf where mask [N, L] is zero."""
    prec = dots.dtype
    s = (dots.to(dt).to(prec) / torch.tensor(SQRT_D, dtype=prec)).to(dt).to(prec)
    return s.masked_fill(~mask.bool()[:, None, :], -math.inf)


def attend(s, vall, dt):
    """s [N, h, L], vall [N, h, L, 128] -> (P rounded to T, the output before its rounding [N, h, 128], the bound), softmax and P V in the precision of s."""
    prec = s.dtype
    e = torch.exp(s - s.amax(-1, keepdim=True))
    p = (e / e.sum(-1, keepdim=True)).to(dt).to(prec)
    out = (p[..., None] * vall.to(prec)).sum(-2)
    bound = ((ulp(p, dt) * (p > 0))[..., None] * vall.double().abs()).sum(-2) + ulp(out, dt)
    return p, out, bound


class Case:
    """One launch: inputs (model dtype, logical row-major caches) and, after ref(), the restatement's results."""

    def ref(self, prec=torch.float64, order=0):
        dt, B, L = self.dt, self.B, self.max_len
        q, k, v = new_token(self.x, self.heads, dt, prec, self.cos, self.sin, self.lbq, self.lbv)
        kall, vall = self.kc.to(prec).clone(), self.vc.to(prec).clone()
        idx = self.slot.long()
        rows = torch.arange(B)
        kall[rows, :, idx], vall[rows, :, idx] = k, v                          # the in-place append
        live = (torch.arange(L)[None] <= idx[:, None]) & self.mask.bool()      # cached positions below the slot, and the slot itself
        dots = raw_dots(q, kall, order)
        s = scores(dots, live, dt)
        p, out, bound = attend(s, vall, dt)
        return {"q": q, "k": k, "v": v, "dots": dots, "s": s, "p": p, "out": out.reshape(B, -1), "bound": bound.reshape(B, -1), "kall": kall, "vall": vall,
                "live": live}


def grid(g, shape, step=8, lim=1.0):
    n = int(lim * step)
    return torch.randint(-n, n + 1, shape, generator=g).float() / step


def rope_rows(g, n, invertible):
    """cos, sin [n, 128] from {0, +-1, +-1/2}, every dim drawn on its own; invertible [n] bool: rows where each dim pair (d, d + 64) has either both cos = +-1 and
    both sin = 0, or both cos = 0 and both sin = +-1."""
    vals = torch.tensor([0.0, 1.0, -1.0, 0.5, -0.5])
    cos, sin = vals[torch.randint(0, 5, (n, D), generator=g)], vals[torch.randint(0, 5, (n, D), generator=g)]
    sign = lambda: (torch.randint(0, 2, (n, D), generator=g) * 2 - 1).float()
    kind = torch.randint(0, 2, (n, D // 2), generator=g).repeat(1, 2).bool()  # the same kind for d and d + 64
    ci, si = torch.where(kind, sign(), torch.zeros(n, D)), torch.where(kind, torch.zeros(n, D), sign())
    inv = torch.as_tensor(invertible).bool()[:, None]
    return torch.where(inv, ci, cos), torch.where(inv, si, sin)


def solve_rope(target, cos, sin):
    """raw [..., 128] with T(T(raw cos) + T(rotate_half(raw) sin)) = target, for an invertible cos / sin row (rope_rows)."""
    h = D // 2
    raw = torch.zeros_like(target)
    # cos kind: target[d] = cos[d] raw[d].  sin kind: target[d] = -sin[d] raw[d + 64] (d < 64), target[d + 64] = sin[d + 64] raw[d]
    raw += cos * target
    raw[..., h:] += (-sin * target)[..., :h]
    raw[..., :h] += (sin * target)[..., h:]
    return raw


def hot_row(g, qp, flat_scores, live, pos, dt):
    """A K row for position `pos` of one pair that takes a third of the mass: +-a with the sign of q' on a growing random set of dims, grid noise elsewhere. qp [128] fp64,
    flat_scores [L] fp64 (the pair's scores with -inf where dead; the entry at pos is ignored)."""
    others = flat_scores.clone()
    others[pos] = -math.inf
    z = torch.exp(others[live]).sum() if bool(live.any()) else torch.tensor(0.0, dtype=torch.float64)
    target = math.log(max(float(z), 1e-3) * 0.5)                            # odds 1 : 2
    noise = grid(g, (D,)).double()
    order = torch.randperm(D, generator=g)
    best = None
    for a in (0.125, 0.25, 0.5, 1.0, 2.0):
        al = torch.sign(qp[order]) * math.copysign(a, target)                # +-a, aligned with q' (against it for a negative target)
        gain = qp[order] * (al - noise[order])
        c = ((qp * noise).sum() + torch.cat((torch.zeros(1, dtype=torch.float64), gain.cumsum(0)))) / SQRT_D
        n = int((c - target).abs().argmin())
        err = float((c[n] - target).abs())
        if best is None or err < best[0]:
            row = noise.clone()
            row[order[:n]] = al[:n]
            best = (err, row)
        if err < 0.25:
            break
    return best[1]


def make_case(dt, heads, max_len, slots, hot, seed, lora=False, pad=None, mask_hot=(), flat=False, kc=None, vc=None):
    """slots [B]: the cache slot of each row's new token (= its number of cached positions); hot [B][heads]: the hot position of each pair (== the slot: the new
    token); pad [B]: leading positions masked out (left padding); mask_hot: rows whose hot positions get a zero mask byte AFTER the row is built (the output must
    ignore them); kc / vc: caches to start from (model dtype, row-major; the hot rows are written into a copy of kc); flat: no hot rows and all-zero K, i.e. uniform probabilities (the recorded reason for the hot rows)."""
    g = torch.Generator().manual_seed(seed)
    c = Case()
    B = len(slots)
    c.dt, c.heads, c.B, c.max_len, c.lora = dt, heads, B, max_len, lora
    H = D * heads
    c.slot = torch.tensor(slots, dtype=torch.int32)
    c.hot = hot
    pad = pad or [0] * B
    x = torch.zeros(B, qkv_ld(heads, lora))
    x[:, :3 * H] = grid(g, (B, 3 * H))
    c.lbq = c.lbv = None
    if lora:
        x[:, 3 * H:3 * H + 16] = grid(g, (B, 16), step=4)
        c.lbq, c.lbv = grid(g, (H, 8), step=4).to(dt), grid(g, (H, 8), step=4).to(dt)
    new_hot = [(not flat) and any(hot[b][h] == slots[b] for h in range(heads)) for b in range(B)]
    cos, sin = rope_rows(g, B, new_hot)
    c.cos, c.sin = cos.to(dt), sin.to(dt)
    # rows from the slot up: stale values the kernel must not use
    c.kc = grid(g, (B, heads, max_len, D)).to(dt) if kc is None else kc.clone()
    c.vc = (torch.rand(B, heads, max_len, D, generator=g) * 1.98 - 0.99).to(dt) if vc is None else vc.clone()
    c.mask = torch.ones(B, max_len, dtype=torch.uint8)
    for b in range(B):
        c.mask[b, :pad[b]] = 0
    if flat:                                                                 # every score is zero: uniform probabilities
        c.kc.zero_()
        x[:, H:2 * H] = 0
    c.x = x.to(dt)
    if not flat:
        q, k, _ = new_token(c.x, heads, dt, torch.float64, c.cos, c.sin, c.lbq, c.lbv)
        kall = c.kc.double().clone()
        kall[torch.arange(B), :, c.slot.long()] = k
        live = (torch.arange(max_len)[None] <= c.slot.long()[:, None]) & c.mask.bool()
        s = scores(raw_dots(q, kall), live, dt)
        for b in range(B):
            for h in range(heads):
                p = hot[b][h]
                assert pad[b] <= p <= slots[b], "the hot position must be live"
                lv = live[b].clone()
                lv[p] = False
                row = hot_row(g, q[b, h], s[b, h], lv, p, dt)
                if p == slots[b]:
                    x[b, H + h * D:H + (h + 1) * D] = solve_rope(row, cos[b].double(), sin[b].double()).float()
                else:
                    c.kc[b, h, p] = row.to(dt)
        c.x = x.to(dt)
        assert torch.equal(c.x.float(), x) and bool((c.x[:, H:2 * H].float().abs() <= 2).all()), "the raw k of a hot new token left the grid"
    for b in mask_hot:
        for h in range(heads):
            assert hot[b][h] < slots[b], "a row's own slot cannot be masked"
            c.mask[b, hot[b][h]] = 0
    c.masked_rows = tuple(mask_hot)
    return c


def hot_shares(case, r):
    """P of every pair's hot position [B, heads] (0 where it is masked)."""
    idx = torch.tensor(case.hot).long()
    return r["p"].gather(-1, idx[..., None])[..., 0]


def assert_hot(case, r):
    sh = hot_shares(case, r)
    for b in range(case.B):
        if b not in case.masked_rows:
            assert bool(((sh[b] >= SHARE_LO) & (sh[b] <= SHARE_HI)).all()), f"row {b}: hot shares {sh[b].tolist()} outside [{SHARE_LO}, {SHARE_HI}]"
        else:
            assert bool((sh[b] == 0).all())


def ratio(out, r):
    """Worst |out - ref| / bound over a launch ([B, hidden], any float dtype), inf where out is not finite."""
    o = out.double()
    q = (o - r["out"]).abs() / r["bound"]
    return float(torch.where(torch.isfinite(o), q, torch.full_like(q, math.inf)).max())


# ---- the prompt's write -----------------------------------------------------------------------------------------------------------------------------------
def prefill_ref(x, heads, dt, prec, cos_t, sin_t, pos_ids, lbq=None, lbv=None):
    """x [B, T, qkv_ld], pos_ids [B, T] -> qout [B T, hidden], k', v' [B, heads, T, 128] (prec, T values)."""
    B, T = x.shape[:2]
    pi = pos_ids.reshape(-1).long()
    q, k, v = new_token(x.reshape(B * T, -1), heads, dt, prec, cos_t[pi], sin_t[pi], lbq, lbv)
    per = lambda t: t.reshape(B, T, heads, D).permute(0, 2, 1, 3)
    return q.reshape(B * T, -1), per(k), per(v)


# ---- the launches of tests/test_gpu_decode_attn.py (test_decode_attn_ref.py runs their inputs through the fp32 / fp64 comparison) ---------------------------
# RDX_ATT_TP value -> contexts on either side of every boundary of that variant (attn_body.h: V row sweep SPAN, half and whole register window, tail trips)
VARIANTS = {0: "16 waves", 2: "8 waves", 1: "4 waves"}
EDGES_ALL = [(1, 2, 15), (15, 16, 17)]
EDGES = {0: [(59, 60, 61), (239, 240, 241), (479, 480, 481), (719, 720, 721), (959, 960, 961)],
         2: [(27, 28, 29), (223, 224, 225), (335, 336, 337), (559, 560, 561)],
         1: [(63, 64, 65), (127, 128, 129), (191, 192, 193), (255, 256, 257)]}
EDGE_TOP = (1535,)                                                          # at max_len 1536
SWEEP_CTX = {0: 1000, 2: 700, 1: 300}                                       # beyond the register window, into the second tail trip


def edge_groups(variant):
    return EDGES_ALL + EDGES[variant] + [EDGE_TOP]


def edge_case(dt, group, seed, lora):
    """One launch for the contexts of `group` (the middle one is the boundary): per context a row with hot positions (last cached, first live) and a row with
    (just inside the boundary, the new token); the first row of the largest context is left-padded; one extra row has its hot position masked."""
    bnd = group[len(group) // 2]
    slots, hot, pad = [], [], []
    for ctx in group:
        p = min(3, ctx - 1) if ctx == max(group) else 0
        slots += [ctx, ctx]
        pad += [p, 0]
        hot += [[ctx - 1, p], [min(bnd - 1, ctx - 1), ctx]]
    top = max(group)
    slots.append(top)
    pad.append(0)
    hot.append([min(bnd - 1, top - 1)] * 2)
    return make_case(dt, 2, (top + 1 + 31) // 32 * 32, slots, hot, seed, lora=lora, pad=pad, mask_hot=(len(slots) - 1,))


def sweep_launches(ctx):
    return (ctx + 15) // 16


_SWEEP_BASE = {}


def sweep_case(dt, ctx, i, seed):
    """Launch i of the sweep over context ctx: 8 rows x 2 heads, the hot positions 16 i .. 16 i + 15 (clamped to the last cached one). The launches of one sweep
    start from the same caches (drawn once); new token, LoRA and RoPE rows are drawn per launch."""
    max_len = (ctx + 1 + 31) // 32 * 32
    key = (dt, ctx, seed)
    if key not in _SWEEP_BASE:
        _SWEEP_BASE.clear()
        g = torch.Generator().manual_seed(seed)
        _SWEEP_BASE[key] = (grid(g, (8, 2, max_len, D)).to(dt), (torch.rand(8, 2, max_len, D, generator=g) * 1.98 - 0.99).to(dt))
    kc, vc = _SWEEP_BASE[key]
    hot = [[min(16 * i + 2 * b + h, ctx - 1) for h in range(2)] for b in range(8)]
    return make_case(dt, 2, max_len, [ctx] * 8, hot, seed + 1 + i, lora=bool(i & 1), kc=kc, vc=vc)
