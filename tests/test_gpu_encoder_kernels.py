"""The image encoder's non-GEMM kernels one launch at a time, through the test hooks rdx_stem_test / rdx_norm_test / rdx_attn_test
(include/rdx_enc_hooks.h), against a plain fp64 evaluation of the same operation on the model-dtype-rounded operands, with the kernels' documented
rounding points emulated:

  * stem (stem.hip, elem.hip img_prep_k / maxpool_k): T(relu(conv + bias)), the 3 x 3 / 2 max pool exact on those values. Inputs are white noise
    with three DIFFERENT channels (the encoder tests' synthetic radiographs repeat one channel, under which an R/B swap or a channel / kw mix-up in
    the weight layout passes) and one image whose border pixels hold the extremes 0 / 1;
  * LayerNorms (layernorm_k, layernorm_ex_k, layernorm_packed_k, scramble_layernorm_k) and avgpool_flatten_k: fp32 outputs within
    1e-5 x max(1, |ref|), model-dtype outputs within one ulp of T(ref) beyond the fp32 statistics' own error (_ln_allow);
  * attention (attn.hip attention_k, flash.hip flash_prefill_k): T(Q K^T), T(. / sqrt(D)), softmax in fp64, P rounded to T, output within two
    model-dtype ulps of max |V|.

Every bar is also shown to REJECT a plausible bug: the reference is perturbed (weight channels permuted, pool window shifted by a pixel, last key
dropped, eps x 10, the scramble replaced by a plain permute) and the same comparison against the kernel output must fail (_sensitive)."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DT = {"f16": torch.float16, "bf16": torch.bfloat16}
MANT = {torch.float16: 10, torch.bfloat16: 7}
MIN_NORMAL = {torch.float16: 2.0 ** -14, torch.bfloat16: 2.0 ** -126}


@pytest.fixture(scope="module", params=["f16", "bf16"])
def eng(request):
    from radialog_amd.config import small_cfg
    from radialog_amd.engine import RdxEngine
    e = RdxEngine(small_cfg(), dtype=request.param, device=0, max_batch=1, max_len=32, llama=False, vision=False)
    e.dt = DT[request.param]
    yield e
    e.close()


def ulp(x, dt):
    """Spacing of the model dtype at |x| (fp64; subnormal spacing below the smallest normal)."""
    a = x.double().abs().clamp_min(MIN_NORMAL[dt])
    return torch.exp2(torch.floor(torch.log2(a)) - MANT[dt])


def ulps_off(out, ref, dt, allow=0.0):
    """|out - T(ref)| in model-dtype ulps at the larger of the two magnitudes, after `allow` (an absolute fp32-accumulation allowance)."""
    o, r = out.double().cpu(), ref.to(dt).double()
    d = ((o - r).abs() - allow).clamp_min(0.0)
    return d / ulp(torch.maximum(o.abs(), r.abs()), dt)


def _sensitive(check, name):
    """A perturbed reference must fail the bar: `check` returns (passes, worst measure)."""
    ok, worst = check()
    assert not ok, f"the bar does not see {name}: worst {worst:.3g}"
    return worst


# ----------------------------------------------------------------------------------------------------------------------------------------
# stem: img_prep_k + stem_pool_k (row-major / fragment-packed) and conv_gemm + maxpool_k
# ----------------------------------------------------------------------------------------------------------------------------------------
def _stem_inputs(B, S, stem, seed):
    g = torch.Generator().manual_seed(seed)
    img = torch.rand(B, 3, S, S, generator=g)                        # three independent channels
    b = B - 1                                                        # the last image: extremes on its 3-pixel border ring
    ring = torch.ones(S, S, dtype=torch.bool)
    ring[3:S - 3, 3:S - 3] = False
    yy, xx = torch.meshgrid(torch.arange(S), torch.arange(S), indexing="ij")
    ext = ((yy + xx) % 2).float()
    for c in range(3):
        img[b, c][ring] = (ext if c != 1 else 1 - ext)[ring]
    w = torch.randn(stem, 3, 7, 7, generator=g) / math.sqrt(147.0)
    bias = torch.randn(stem, generator=g) * 0.2 - 0.1               # many conv outputs clipped by the ReLU
    return img, w, bias


def _stem_ref(img, w, bias, dt, shift=0):
    """fp64 on the rounded operands: T(relu(conv7x7/2 + bias)), then the exact 3 x 3 / 2 pad-1 max pool. Returns (pooled NHWC, pooled fp32
    accumulation allowance). shift = 1 moves every pool window one conv pixel right (a perturbation for the sensitivity check)."""
    x, wt = img.to(dt).double(), w.to(dt).double()
    y = F.conv2d(x, wt, stride=2, padding=3) + bias.double().view(1, -1, 1, 1)
    a = F.conv2d(x.abs(), wt.abs(), stride=2, padding=3) + bias.double().abs().view(1, -1, 1, 1)
    y = y.relu().to(dt).double()
    if shift:
        y = F.pad(y[..., shift:], (0, shift), value=0.0)
    pool = F.max_pool2d(y, 3, 2, 1).permute(0, 2, 3, 1)
    allow = F.max_pool2d(a, 3, 2, 1).permute(0, 2, 3, 1) * 2.0 ** -18   # K = 147 fp32 products summed: far below one ulp unless they cancel
    return pool, allow


def _stem_bar(out, ref, allow, dt):
    u = ulps_off(out, ref, dt, allow)
    frac1 = float((u <= 1).double().mean())
    return bool(u.max() <= 2 and frac1 >= 0.999), float(u.max()), frac1


STEM_CASES = [(S, stem) for S in (64, 128, 200, 448, 488) for stem in (32, 64)]


@pytest.mark.parametrize("S,stem", STEM_CASES)
def test_stem_matches_fp64_reference(eng, S, stem):
    """Three images (B = 3) and the first alone (B = 1), every path. 200 / 488 px give ragged 4 x 16 pooled tiles (50 = 12.5 row tiles, 122 = 7.6
    column tiles) and -- at B = 1 / 3 -- pad rows in the last packed tile (whose zeroing the hook checks)."""
    dt = eng.dt
    img, w, bias = _stem_inputs(3, S, stem, seed=S * 10 + stem)
    ref, allow = _stem_ref(img, w, bias, dt)
    outs = {}
    for path in (0, 1, 2):
        out = eng.stem_test(img, w, bias, path=path).cpu()
        assert out.shape == (3, S // 4, S // 4, stem) and torch.isfinite(out).all()
        ok, worst, frac1 = _stem_bar(out, ref, allow, dt)
        print(f"stem {dt} S={S} stem={stem} path {path}: worst {worst:.2f} ulp, {100 * frac1:.3f} % within 1 ulp")
        assert ok, f"path {path}: worst {worst} ulp, {frac1:.5f} within 1 ulp"
        outs[path] = out
        one = eng.stem_test(img[:1], w, bias, path=path).cpu()
        assert torch.equal(one, out[:1]), f"path {path}: image 0 alone differs from image 0 of the batch of three"
    assert torch.equal(outs[0], outs[1]), "stem_pool_k: packed and row-major outputs differ"
    assert float(ulps_off(outs[2], outs[0].double(), dt).max()) <= 1, "fused and two-kernel stems differ by more than one ulp"
    if S == 64:
        # the bar rejects: the weight's channel axis permuted (R <-> B), the pool window one conv pixel off
        ref_p, allow_p = _stem_ref(img, w[:, [2, 1, 0]], bias, dt)
        _sensitive(lambda: _stem_bar(outs[0], ref_p, allow_p, dt)[:2], "R and B swapped in the stem weight")
        ref_s, allow_s = _stem_ref(img, w, bias, dt, shift=1)
        _sensitive(lambda: _stem_bar(outs[0], ref_s, allow_s, dt)[:2], "a pool window shifted by one pixel")


# ----------------------------------------------------------------------------------------------------------------------------------------
# LayerNorms and the classifier's average pool
# ----------------------------------------------------------------------------------------------------------------------------------------
def _ln_ref(x, gamma, beta, eps):
    x = x.double()
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    return (x - mean) / torch.sqrt(var + eps) * gamma.double() + beta.double()


def _ln_inputs(rows, H, dt, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, H, generator=g) + 3.0                      # an offset: the two-pass variance matters
    x[1] = torch.randn(H, generator=g) * 1e-3                        # variance ~ eps: eps x 10 must show
    gamma = 1.0 + 0.1 * torch.randn(H, generator=g)
    beta = 0.1 * torch.randn(H, generator=g)
    return x.to(dt), gamma, beta


EPS = 1e-6


def _ln_allow(ref):
    """The fp32 statistics' own error, absolute: the row mean of values offset by 3 is off by ~1e-7, which near y = 0 is several model-dtype
    ulps of a tiny value (measured: up to 5 in fp16 without this allowance). 2^-20 x max(1, |ref|) is 1 / 1000 of an fp16 ulp at |y| = 1."""
    return 2.0 ** -20 * ref.abs().clamp_min(1.0)


def _ln_bar(out, out_f32, ref, dt):
    """(passes, worst of: model-dtype ulps beyond _ln_allow, fp32 error / max(1, |ref|) in units of 1e-5)."""
    u = float(ulps_off(out, ref, dt, _ln_allow(ref)).max())
    e = 0.0
    if out_f32 is not None:
        e = float(((out_f32.double().cpu() - ref).abs() / ref.abs().clamp_min(1.0)).max())
    return u <= 1 and e <= 1e-5, max(u, e * 1e5)


@pytest.mark.parametrize("rows,H", [(64, 768), (33, 1408), (5, 256)])
def test_layernorm_and_layernorm_ex_match_fp64(eng, rows, H):
    dt = eng.dt
    x, gamma, beta = _ln_inputs(rows, H, dt, seed=rows + H)
    ref = _ln_ref(x, gamma, beta, EPS)
    out, f32 = eng.norm_test(0, x, gamma, beta, want_f32=True, eps=EPS)
    ok, worst = _ln_bar(out, f32, ref, dt)
    print(f"layernorm_k {dt} {rows}x{H}: worst {worst:.3g} (ulp / 1e-5 rel units)")
    assert ok, worst
    _sensitive(lambda: _ln_bar(out, f32, _ln_ref(x, gamma, beta, 10 * EPS), dt), "eps x 10")
    # layernorm_ex_k: strided rows in and out, a 7-row embedding broadcast as emb[row % 7]
    g = torch.Generator().manual_seed(H)
    xs = torch.zeros(rows, H + 24, dtype=dt)
    xs[:, :H] = x
    emb = (torch.randn(7, H, generator=g) * 0.5).to(dt)
    out, _ = eng.norm_test(1, xs, gamma, beta, emb=emb, out_rows_stride=H + 40, eps=EPS)
    out = out.cpu()
    assert torch.isnan(out[:, H:].float()).all(), "layernorm_ex_k wrote past H in a strided output row"
    ref_ex = ref + emb.double()[torch.arange(rows) % 7]
    u = float(ulps_off(out[:, :H], ref_ex, dt, _ln_allow(ref_ex)).max())
    print(f"layernorm_ex_k {dt} {rows}x{H}: worst {u:.2f} ulp")
    assert u <= 1, f"layernorm_ex_k: {u} ulp"
    assert float(ulps_off(out[:, :H], ref + emb.double()[torch.arange(rows) % 3], dt).max()) > 1, "emb row index not seen"


@pytest.mark.parametrize("M,H", [(48, 192), (40, 256), (32, 288), (64, 768), (40, 768), (16, 1024)])
def test_layernorm_packed_matches_fp64(eng, M, H):
    """layernorm_packed_k<T, 2 / 6 / 8> (H <= 256, <= 768, <= 1024) at both sides of every boundary; M = 40: a ragged last 16-row tile."""
    dt = eng.dt
    x, gamma, beta = _ln_inputs(M, H, dt, seed=M * 7 + H)
    ref = _ln_ref(x, gamma, beta, EPS)
    out, f32 = eng.norm_test(2, x, gamma, beta, want_f32=True, eps=EPS)
    ok, worst = _ln_bar(out, f32, ref, dt)
    print(f"layernorm_packed_k {dt} {M}x{H}: worst {worst:.3g}")
    assert ok, worst
    _sensitive(lambda: _ln_bar(out, f32, _ln_ref(x, gamma, beta, 10 * EPS), dt), "eps x 10")


def _scramble_ref(x, gamma, beta, eps, plain=False):
    """blip2_qformer.py:469: the projector's NCHW output [B][C][P] reshaped to [B][P][C] WITHOUT a permute; `plain` = the (wrong) permute."""
    B, P, C = x.shape
    t = x.double() if plain else x.double().permute(0, 2, 1).contiguous().view(B, P, C)
    return _ln_ref(t, gamma, beta, eps)


@pytest.mark.parametrize("P,C", [(196, 1408), (16, 352), (256, 128), (16, 100), (25, 100)])
def test_scramble_layernorm_matches_fp64(eng, P, C):
    """C % 8 == 0: the 16-byte gather path; C = 100: the scalar path, with P dividing (25) and not dividing (16) C."""
    dt = eng.dt
    B = 2
    g = torch.Generator().manual_seed(P + C)
    x = (torch.randn(B, P, C, generator=g) + torch.linspace(-2, 2, C)).to(dt)     # channel-dependent offsets: a wrong gather shows in the mean
    gamma = 1.0 + 0.1 * torch.randn(C, generator=g)
    beta = 0.1 * torch.randn(C, generator=g)
    ref = _scramble_ref(x, gamma, beta, 1e-5)
    out, f32 = eng.norm_test(3, x, gamma, beta, want_f32=True, eps=1e-5)
    ok, worst = _ln_bar(out, f32, ref, dt)
    print(f"scramble_layernorm_k {dt} P={P} C={C}: worst {worst:.3g}")
    assert ok, worst
    _sensitive(lambda: _ln_bar(out, f32, _scramble_ref(x, gamma, beta, 1e-5, plain=True), dt), "a plain permute instead of the scramble")


@pytest.mark.parametrize("G", [16, 15])
def test_avgpool_flatten_matches_fp64(eng, G):
    """avg_pool2d(4) (floor: 15 -> 3) + x.view(B, -1) of [B][C][Gp][Gp], from the NHWC projector output."""
    dt = eng.dt
    B, C, pool = 2, 128, 4
    x = torch.randn(B, G, G, C, generator=torch.Generator().manual_seed(G)).to(dt)
    ref = F.avg_pool2d(x.double().permute(0, 3, 1, 2), pool).reshape(B, -1)
    out, _ = eng.norm_test(4, x, aux=G, pool=pool)
    u = float(ulps_off(out, ref, dt).max())
    print(f"avgpool_flatten_k {dt} G={G}: worst {u:.2f} ulp")
    assert out.shape == ref.shape and u <= 1, u
    wrong = F.avg_pool2d(x.double().permute(0, 3, 1, 2), pool).permute(0, 2, 3, 1).reshape(B, -1)      # NHWC flatten order
    assert float(ulps_off(out, wrong, dt).max()) > 1


# ----------------------------------------------------------------------------------------------------------------------------------------
# attention
# ----------------------------------------------------------------------------------------------------------------------------------------
def _attn_ref(q, k, v, dt, causal=False, mask=None, drop_last=False):
    """q [B,Tq,H,D], k / v [B,Tk,H,D] (model dtype): T(QK^T), T(./sqrt(D)), fp64 softmax, T(P), P V in fp64. Rows without a visible key give 0."""
    B, Tq, H, D = q.shape
    Tk = k.shape[1]
    qd, kd, vd = (t.double().cpu().permute(0, 2, 1, 3) for t in (q, k, v))
    s = (qd @ kd.transpose(-1, -2)).to(dt).double()
    s = (s / math.sqrt(D)).to(dt).double()
    ok = torch.ones(B, 1, Tq, Tk, dtype=torch.bool)
    if causal:
        ok &= (torch.arange(Tk).view(1, Tk) <= torch.arange(Tq).view(Tq, 1) + (Tk - Tq)).view(1, 1, Tq, Tk)
    if mask is not None:
        ok &= mask.bool().view(B, 1, 1, Tk)
    if drop_last:
        ok[..., Tk - 1] = False
    s = s.masked_fill(~ok, -math.inf)
    p = torch.softmax(s, -1).nan_to_num(0.0)
    p = p.to(dt).double()
    return (p @ vd).permute(0, 2, 1, 3), p


def _attn_bar(out, ref, v, dt):
    tol = 2 * float(ulp(v.double().abs().max(), dt))
    err = float((out.double().cpu() - ref).abs().max())
    return err <= tol, err / tol


def _qkv(B, Tq, Tk, H, D, dt, dev, seed):
    """Q, K, V as strided views the way the callers lay them out: Q inside a fused [token][3][head][D + 8] row, K head-major [B][H][Tk][D],
    V with its own padded token stride."""
    g = torch.Generator().manual_seed(seed)
    qb = torch.randn(B, Tq, 3, H, D + 8, generator=g).to(dt).to(dev)
    kb = torch.randn(B, H, Tk, D, generator=g).to(dt).to(dev)
    vb = torch.randn(B, Tk + 3, H * D + 16, generator=g).to(dt).to(dev)
    q = qb[:, :, 1, :, :D]
    k = kb.permute(0, 2, 1, 3)
    v = vb[:, 2:Tk + 2, 8:8 + H * D].unflatten(2, (H, D))
    k[:, Tk - 1] = q[:, 0]                  # query 0 puts most of its weight on the LAST key (the one next to the clamped / masked padding)
    return q, k, v


ATTN_SHAPES = [(32, 32), (32, 16), (32, 196), (392, 392), (1, 1), (17, 300), (5, 1000)]


@pytest.mark.parametrize("D", [32, 64, 128])
def test_attention_matches_fp64(eng, D):
    dt, dev = eng.dt, eng.device
    B, H = 2, 2
    worst = 0.0
    for i, (Tq, Tk) in enumerate(ATTN_SHAPES):
        q, k, v = _qkv(B, Tq, Tk, H, D, dt, dev, seed=D * 100 + i)
        ref, _ = _attn_ref(q, k, v, dt)
        for o_packed in (False, True):
            out = eng.attn_test(q, k, v, o_packed=o_packed)
            assert torch.isfinite(out).all()
            ok, m = _attn_bar(out, ref, v, dt)
            worst = max(worst, m)
            assert ok, f"D={D} Tq={Tq} Tk={Tk} packed={o_packed}: {m:.3g} x the bar"
        if Tk > 1 and (Tq, Tk) != (1, 1):
            _sensitive(lambda: _attn_bar(out, _attn_ref(q, k, v, dt, drop_last=True)[0], v, dt), f"the last key dropped (Tk = {Tk})")
    # causal with an append offset (Tk > Tq), and a left-padded key mask with fully masked query rows
    Tq, Tk = 24, 56
    q, k, v = _qkv(B, Tq, Tk, H, D, dt, dev, seed=D + 7)
    mask = torch.ones(B, Tk, dtype=torch.uint8)
    mask[0, :40] = 0                                                 # row 0: queries 0 .. 7 see keys <= q + 32, all padded
    mask[1, :3] = 0
    ref, _ = _attn_ref(q, k, v, dt, causal=True, mask=mask)
    out = eng.attn_test(q, k, v, causal=True, key_mask=mask)
    ok, m = _attn_bar(out, ref, v, dt)
    worst = max(worst, m)
    assert ok, f"causal + key mask: {m:.3g} x the bar"
    dead = out[0, :8].float()
    assert torch.isfinite(dead).all() and bool((dead == 0).all()), "a query row without any visible key must give exactly 0"
    # non-causal, a whole batch row masked
    mask2 = torch.ones(B, Tk, dtype=torch.uint8)
    mask2[1] = 0
    out = eng.attn_test(q, k, v, key_mask=mask2, o_packed=True)
    ref, _ = _attn_ref(q, k, v, dt, mask=mask2)
    ok, m = _attn_bar(out, ref, v, dt)
    assert ok and bool((out[1].float() == 0).all()), f"fully masked batch row: {m:.3g} x the bar"
    print(f"attention {dt} D={D}: worst {worst:.3f} x the 2-ulp-of-max|V| bar")


def test_flash_prefill_and_attention_k_agree(eng):
    """D = 128, causal, left-padded mask (fully masked rows included): flash_prefill_k and attention_k each against fp64, and against each other
    within one model-dtype ulp per probability (flash.hip: fexp and the reciprocal multiply round a probability the other way only near a
    rounding boundary), plus one ulp of the output for its final rounding."""
    dt, dev = eng.dt, eng.device
    B, H, T, D = 2, 2, 160, 128
    q, k, v = _qkv(B, T, T, H, D, dt, dev, seed=1234)
    mask = torch.ones(B, T, dtype=torch.uint8)
    mask[0, :37] = 0
    ref, p = _attn_ref(q, k, v, dt, causal=True, mask=mask)
    outs = {}
    for kernel in (1, 2):
        for o_packed in (False, True):
            out = eng.attn_test(q, k, v, causal=True, key_mask=mask, kernel=kernel, o_packed=o_packed)
            ok, m = _attn_bar(out, ref, v, dt)
            print(f"attention {dt} D=128 causal masked, kernel {kernel} packed={o_packed}: {m:.3f} x the bar")
            assert ok, f"kernel {kernel}: {m:.3g} x the bar"
            assert bool((out[0, :37].float() == 0).all())
            outs[(kernel, o_packed)] = out.double().cpu()
    bound = (ulp(p, dt) * (p > 0)) @ v.double().cpu().abs().permute(0, 2, 1, 3)          # [B,H,Tq,D]: one ulp per probability
    bound = bound.permute(0, 2, 1, 3) + ulp(ref, dt)
    diff = (outs[(1, False)] - outs[(2, False)]).abs()
    print(f"flash vs attention_k {dt}: worst {float((diff / bound).max()):.3f} x the one-ulp-per-probability bound")
    assert bool((diff <= bound).all())
    with pytest.raises(Exception, match="flash_prefill_k does not take"):
        eng.attn_test(q, k, v, causal=False, key_mask=mask, kernel=2)
