"""Inputs of the fp8 KV cache's kernel tests (tests/test_gpu_kv8_attn.py; their conditions are asserted on the CPU by tests/test_kv8_host.py): the cases of
tests/_dec_attn.py on caches whose rows carry DIFFERENT exponents.

The stock cases give every K row the exponent -8 (grid rows with amax 1) and every V row -8 (amax just under 1): an exponent applied to the wrong position,
head or row would go unseen. Here cache row (b, h, j) is scaled by a power of two that changes with each of the three indices:
  K    the grid row times 2^-((j + h + b) mod 3): still multiples of a power of two, every product and sum of the scores stays exact in fp32;
  V    dequant(quant(rand 2^-((j + 2 h + b) mod 4))): arbitrary stored values.
The hot rows are written on top by make_case, as in the stock cases. Every K row (hot rows included: +-a <= 2 and grid noise) round-trips the format
exactly, so the K cache IS a stored cache; both statements are asserted by stored()."""
import torch

import _dec_attn as A
from radialog_amd import kv8

D = A.D


def base_caches(g, dt, B, heads, max_len):
    """(K, V) [B, heads, max_len, 128] in dt, scaled as the module docstring says."""
    j, h, b = torch.arange(max_len)[None, None, :], torch.arange(heads)[None, :, None], torch.arange(B)[:, None, None]
    kc = A.grid(g, (B, heads, max_len, D)) * torch.exp2(-((j + h + b) % 3).float())[..., None]
    vc = (torch.rand(B, heads, max_len, D, generator=g) * 1.98 - 0.99) * torch.exp2(-((j + 2 * h + b) % 4).float())[..., None]
    kd = kc.to(dt)
    assert torch.equal(kd.float(), kc)
    return kd, kv8.roundtrip(vc.to(dt))


def stored(case):
    """The case's caches as codes and exponents: (kcodes, kexp, vcodes, vexp), logical order. Asserts that the caches hold stored values."""
    kq, vq = kv8.quant(case.kc), kv8.quant(case.vc)
    assert torch.equal(kv8.dequant(*kq, dtype=case.dt).view(torch.int16), case.kc.view(torch.int16)), "a K row of the case does not round-trip the format"
    assert torch.equal(kv8.dequant(*vq, dtype=case.dt).view(torch.int16), case.vc.view(torch.int16)), "a V row of the case is not a stored value"
    return kq[0], kq[1], vq[0], vq[1]


def exponents_vary(case, kexp, vexp):
    """The condition on the inputs: over the positions a launch reads (below each row's slot), the exponents of neighbouring positions differ -- but for the
    pairs a hot row breaks: a pair's hot row is drawn on top with an exponent of its own and has two neighbours, so up to two equal pairs per head; beyond
    that, nine in ten must differ -- and so do those of the two heads and of neighbouring rows at the same position (more than half of the positions; a
    context of one or two positions may consist of hot rows alone)."""
    for name, e in (("K", kexp), ("V", vexp)):
        for b in range(case.B):
            n = int(case.slot[b])
            x = e[b, :, :n]
            if n > 1:
                same = x[:, 1:] == x[:, :-1]
                assert int(same.sum()) <= 2 * x.shape[0] or float(same.float().mean()) <= 0.1, (name, b, int(same.sum()), n)
            hd = (x[0] != x[1]).float().mean()
            assert hd > 0.5 or (n <= 2), (name, b, float(hd))
            if b + 1 < case.B:
                m = min(n, int(case.slot[b + 1]))
                rw = (e[b, :, :m] != e[b + 1, :, :m]).float().mean()
                assert rw > 0.5 or m <= 2, (name, b, float(rw))


def edge_case(dt, group, seed, lora):
    """_dec_attn.edge_case (the three contexts around one boundary; hot positions last cached, first live, just inside the boundary, the new token; one row
    left-padded, one with its hot position masked) on the scaled caches."""
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
    max_len = (top + 1 + 31) // 32 * 32
    g = torch.Generator().manual_seed(seed + 77)
    kc, vc = base_caches(g, dt, len(slots), 2, max_len)
    return A.make_case(dt, 2, max_len, slots, hot, seed, lora=lora, pad=pad, mask_hot=(len(slots) - 1,), kc=kc, vc=vc)


_SWEEP_BASE = {}


def sweep_case(dt, ctx, i, seed):
    """_dec_attn.sweep_case on the scaled caches: launch i has the hot positions 16 i .. 16 i + 15."""
    max_len = (ctx + 1 + 31) // 32 * 32
    key = (dt, ctx, seed)
    if key not in _SWEEP_BASE:
        _SWEEP_BASE.clear()
        _SWEEP_BASE[key] = base_caches(torch.Generator().manual_seed(seed), dt, 8, 2, max_len)
    kc, vc = _SWEEP_BASE[key]
    hot = [[min(16 * i + 2 * b + h, ctx - 1) for h in range(2)] for b in range(8)]
    return A.make_case(dt, 2, max_len, [ctx] * 8, hot, seed + 1 + i, lora=bool(i & 1), kc=kc, vc=vc)


def packed_case(dt, B, seed):
    """The rows of test_packed_outputs_equal_the_row_major_one on the scaled caches."""
    slots = [1 + (7 * b) % 50 for b in range(B)]
    hot = [[(3 * b) % (slots[b] + 1), (5 * b + 1) % (slots[b] + 1)] for b in range(B)]
    kc, vc = base_caches(torch.Generator().manual_seed(seed + 5), dt, B, 2, 64)
    return A.make_case(dt, 2, 64, slots, hot, seed, lora=True, kc=kc, vc=vc)
