"""CPU leg of the decode-attention tests: the restatement of tests/_dec_attn.py is exact where the GPU tests hold the kernels bit for bit (fp32 and fp64 agree
on q', k', v', the raw dots in two summation orders and the scores, on every input family of tests/test_gpu_decode_attn.py), it equals oracle.ref_cpu.LlamaOracle's
attention, its K-cache order is the one the comment in csrc/rdx_common.h states, and its bar sees what it is meant to see: a dropped hot position, a hot position
with its neighbour's V row -- and, the recorded reason for hot positions, NOT a dropped position among flat probabilities in bf16."""
import math

import pytest
import torch

import _dec_attn as A

DTS = ["f16", "bf16"]


def _bits(t, dt):
    return t.to(dt).contiguous().view(torch.int16)


def _exact(case):
    """fp32 (two summation orders) against fp64, bit for bit."""
    r64 = case.ref(torch.float64)
    for order in (0, 1):
        r32 = case.ref(torch.float32, order)
        for key in ("q", "k", "v", "dots", "s"):
            assert torch.equal(r32[key].double(), r64[key]), f"{key} (order {order}): the fp32 evaluation differs from fp64"
    return r64


@pytest.mark.parametrize("dtn", DTS)
@pytest.mark.parametrize("variant", list(A.VARIANTS))
def test_fp32_and_fp64_agree_bit_for_bit_on_the_edge_launches(dtn, variant):
    dt = A.DT[dtn]
    for gi, group in enumerate(A.edge_groups(variant)):
        case = A.edge_case(dt, group, 100 * variant + gi, lora=bool(gi & 1))
        r = _exact(case)
        A.assert_hot(case, r)


@pytest.mark.parametrize("dtn", DTS)
@pytest.mark.parametrize("variant", list(A.VARIANTS))
def test_fp32_and_fp64_agree_bit_for_bit_on_the_sweep_launches(dtn, variant):
    dt, ctx = A.DT[dtn], A.SWEEP_CTX[variant]
    n = A.sweep_launches(ctx)
    for i in (0, 1, n // 2, n - 1):
        case = A.sweep_case(dt, ctx, i, 7000 + variant)
        r = _exact(case)
        A.assert_hot(case, r)


@pytest.mark.parametrize("dtn", DTS)
def test_prompt_write_inputs_are_exact(dtn):
    dt = A.DT[dtn]
    g = torch.Generator().manual_seed(5)
    B, T, heads = 2, 37, 2
    x = torch.zeros(B, T, A.qkv_ld(heads, True))
    x[..., :3 * 128 * heads] = A.grid(g, (B, T, 3 * 128 * heads))
    x[..., 3 * 128 * heads:3 * 128 * heads + 16] = A.grid(g, (B, T, 16), step=4)
    lbq, lbv = A.grid(g, (256, 8), step=4).to(dt), A.grid(g, (256, 8), step=4).to(dt)
    cos, sin = A.rope_rows(g, 64, [False] * 64)
    pos = torch.randint(0, 64, (B, T), generator=g)
    a = A.prefill_ref(x.to(dt), heads, dt, torch.float32, cos.to(dt), sin.to(dt), pos, lbq, lbv)
    b = A.prefill_ref(x.to(dt), heads, dt, torch.float64, cos.to(dt), sin.to(dt), pos, lbq, lbv)
    for u, v in zip(a, b):
        assert torch.equal(u.double(), v)


def test_kperm_elements_sit_where_the_comment_says():
    L = 64
    rows = torch.arange(L * 128, dtype=torch.int32).reshape(L, 128)        # value = pos * 128 + dim
    slab = A.k_permute(rows).reshape(-1)
    for pos, dim in [(0, 0), (0, 7), (0, 8), (1, 0), (15, 0), (0, 32), (0, 31), (5, 77), (16, 0), (17, 9), (31, 127), (47, 64), (63, 127), (33, 40)]:
        assert int(slab[A.kperm_offset(pos, dim)]) == pos * 128 + dim, (pos, dim)
    # the comment's picture: one group = [dim / 32][lane = 16 g + r][8] -- lane 16 g + r of chunk c holds position r, dims 32 c + 8 g .. + 8
    grp = slab[:2048].reshape(4, 64, 8)
    for c, g, r in [(0, 0, 0), (1, 2, 3), (3, 3, 15), (2, 0, 9)]:
        assert grp[c, 16 * g + r].tolist() == [r * 128 + 32 * c + 8 * g + e for e in range(8)]
    assert torch.equal(A.k_unpermute(A.k_permute(rows)), rows) and torch.equal(A.k_permute(rows, 0), rows)
    offs = sorted(A.kperm_offset(p, d) for p in range(L) for d in range(128))
    assert offs == list(range(L * 128))


@pytest.mark.parametrize("dtn", DTS)
def test_restatement_equals_the_oracle_attention(dtn):
    """One decoder layer of oracle.ref_cpu.LlamaOracle (exact mode: fp64 contractions, the reference's rounding points) on the same numbers: the projections are
    signed permutations, so that its q, k, v ARE grid values; its RMSNorm is switched off; q', k', v' and P are taken from its two matmuls, the attention output
    from the input of o_proj. q', k', v' are equal bit for bit. The oracle's softmax is fp32 (the reference's), the restatement's fp64: a probability may round
    to the other neighbour, so P is held to one ulp and the output to the bar."""
    from oracle.ref_cpu import LlamaOracle
    from radialog_amd.config import LlamaCfg
    dt = A.DT[dtn]
    heads, H, B, L = 2, 256, 3, 40
    cfg = LlamaCfg(vocab=8, hidden=H, inter=16, layers=1, heads=heads, max_pos=B, lora_r=8, lora_alpha=2)
    assert cfg.lora_scale == A.LORA_SCALE
    g = torch.Generator().manual_seed(11)

    def sperm(n_out):
        w = torch.zeros(n_out, H)
        w[torch.arange(n_out), torch.randperm(H, generator=g)[:n_out]] = (torch.randint(0, 2, (n_out,), generator=g) * 2 - 1).float()
        return w
    pre = "model.layers.0."
    W = {pre + "input_layernorm.weight": torch.ones(H), pre + "post_attention_layernorm.weight": torch.ones(H)}
    for nm in ("q_proj", "k_proj", "v_proj", "o_proj"):
        W[pre + f"self_attn.{nm}.weight"] = sperm(H)
    for nm in ("q_proj", "v_proj"):
        W[pre + f"self_attn.{nm}.lora_A.weight"] = sperm(8) * 2
        W[pre + f"self_attn.{nm}.lora_B.weight"] = A.grid(g, (H, 8), step=4)
    orc = LlamaOracle(W, cfg, dtype=dt, lora=True, exact=True)
    orc._rms = lambda x, w: x
    cos, sin = A.rope_rows(g, B, [False] * B)
    orc.cos, orc.sin = cos.to(dt), sin.to(dt)
    seen = []
    mm = orc._mm

    class Done(Exception):
        pass

    def spy_mm(a, b):
        seen.append((a.clone(), b.clone()))
        return mm(a, b)

    lin = orc._lin

    def spy_lin(x, key, groups=1, a8=None):
        if key.endswith("o_proj.weight"):
            seen.append(x.clone())
            raise Done
        return lin(x, key, groups, a8)
    orc._mm, orc._lin = spy_mm, spy_lin
    xh = A.grid(g, (B, 1, H)).to(dt)
    kp, vp = A.grid(g, (B, heads, L, 128)).to(dt), (torch.rand(B, heads, L, 128, generator=g) * 1.98 - 0.99).to(dt)
    key_mask = torch.ones(B, L + 1)
    key_mask[1, :5] = 0
    with pytest.raises(Done):
        orc.layer(0, xh, orc._mask(key_mask, 1, L), torch.arange(B).view(B, 1), (kp, vp))
    (q_o, kT_o), (p_o, v_o), o_o = seen
    # the same numbers as a hook call would get them: the QKV row of the fused projection, caches with room for the new token
    x2 = xh[:, 0].double()
    row = torch.cat([x2 @ W[pre + f"self_attn.{nm}.weight"].double().t() for nm in ("q_proj", "k_proj", "v_proj")]
                    + [x2 @ W[pre + f"self_attn.{nm}.lora_A.weight"].double().t() for nm in ("q_proj", "v_proj")], dim=1)
    case = A.Case()
    case.dt, case.heads, case.B, case.max_len = dt, heads, B, 64
    case.x = row.to(dt)
    assert torch.equal(case.x.double(), row)
    case.lbq, case.lbv = W[pre + "self_attn.q_proj.lora_B.weight"].to(dt), W[pre + "self_attn.v_proj.lora_B.weight"].to(dt)
    case.cos, case.sin = orc.cos, orc.sin
    case.slot = torch.full((B,), L, dtype=torch.int32)
    case.kc, case.vc = torch.zeros(B, heads, 64, 128, dtype=dt), torch.zeros(B, heads, 64, 128, dtype=dt)
    case.kc[:, :, :L], case.vc[:, :, :L] = kp, vp
    case.mask = torch.ones(B, 64, dtype=torch.uint8)
    case.mask[:, :L + 1] = key_mask.to(torch.uint8)
    r = case.ref()
    assert torch.equal(_bits(r["q"], dt), _bits(q_o[:, :, 0], dt)), "q'"
    assert torch.equal(_bits(r["k"], dt), _bits(kT_o[:, :, :, L], dt)), "k'"
    assert torch.equal(_bits(r["v"], dt), _bits(v_o[:, :, L], dt)), "v'"
    p_r, p_or = r["p"][:, :, :L + 1], p_o[:, :, 0].double()
    off = (p_r - p_or).abs()
    assert bool((off <= A.ulp(p_r, dt)).all()), "P differs from the oracle's by more than one ulp"
    m = A.ratio(o_o[:, 0], r)
    print(f"oracle {dtn}: {int((off > 0).sum())} of {off.numel()} probabilities round the other way; output {m:.3f} x the bar")
    assert m <= 1.0


def _pair_ratio(out, r, heads):
    """Worst |out - ref| / bound per (row, head) pair."""
    q = (out - r["out"]).abs() / r["bound"]
    return q.reshape(q.shape[0], heads, 128).amax(-1)


def _with_p(r, p, vall=None):
    vall = r["vall"] if vall is None else vall
    return (p[..., None] * vall).sum(-2).reshape(p.shape[0], -1)


@pytest.mark.parametrize("dtn", DTS)
@pytest.mark.parametrize("ctx", [600, 1535])
def test_the_bar_sees_a_dropped_or_misplaced_hot_position(dtn, ctx):
    """For the hot placements the GPU tests use (last cached, first live, next to a window edge, mid-window, the new token): the output without the hot position
    (its P V term left out; its score left out of the softmax as well) and the output with its neighbour's V row lie outside the bar of every pair."""
    dt = A.DT[dtn]
    hot = [[ctx - 1, 3], [479, ctx], [480, 240], [ctx // 2, 0], [59, 60], [ctx, ctx - 2], [239, 1], [ctx - 16, 17]]
    case = A.make_case(dt, 2, (ctx + 32) // 32 * 32, [ctx] * 8, hot, 31 + ctx, lora=True, pad=[3] + [0] * 7)
    r = case.ref()
    A.assert_hot(case, r)
    assert A.ratio(r["out"].to(dt), r) <= 1.0                                # the reference itself, rounded, passes
    idx = torch.tensor(hot).long()[..., None]
    p0 = r["p"].scatter(-1, idx, 0.0)
    drop_pv = _pair_ratio(_with_p(r, p0), r, 2)
    s1 = r["s"].scatter(-1, idx, -math.inf)
    drop_all = _pair_ratio(A.attend(s1, r["vall"], dt)[1].reshape(case.B, -1), r, 2)
    nb = torch.where(idx > 0, idx - 1, idx + 1)                              # the neighbour's V row in the hot position's place
    v2 = r["vall"].scatter(-2, idx[..., None].expand(-1, -1, 1, 128), r["vall"].gather(-2, nb[..., None].expand(-1, -1, 1, 128)))
    wrong_v = _pair_ratio(_with_p(r, r["p"], v2), r, 2)
    print(f"sensitivity {dtn} ctx {ctx}: dropped P V term {float(drop_pv.min()):.0f}-{float(drop_pv.max()):.0f} x the bar, dropped score "
          f"{float(drop_all.min()):.0f}-{float(drop_all.max()):.0f} x, neighbour's V row {float(wrong_v.min()):.0f}-{float(wrong_v.max()):.0f} x")
    assert bool((drop_pv > 1).all()) and bool((drop_all > 1).all()) and bool((wrong_v > 1).all())


def test_flat_probabilities_hide_a_dropped_position_in_bf16():
    """The recorded reason for the hot positions: at context 600 without them, the P V term of ANY single position can go missing inside the bf16 bar."""
    dt, ctx = torch.bfloat16, 600
    case = A.make_case(dt, 2, 608, [ctx] * 4, None, 77, flat=True)
    r = case.ref()
    term = (r["p"][..., None] * r["vall"]).abs() / r["bound"].reshape(case.B, 2, 1, 128)
    worst = float(term.amax())
    print(f"flat bf16 ctx {ctx}: the worst single dropped position moves the output by {worst:.2f} x the bar")
    assert worst < 1.0
