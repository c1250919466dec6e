"""References, bars, layouts and fp32 emulations of the decoder's 3-16-row (xs16.hip) and row-block (xstat32.hip, BLK) GEMM kernels, shared by
tests/test_decoder_gemm_refs.py (CPU: the bars accept a correct fp32 evaluation and reject plausible bugs) and tests/test_gpu_decoder_gemms.py
(the kernels themselves).

THE BAR. Every reference is fp64 on the model-dtype-rounded operands with the kernels' rounding points (skinny_body.h, xs16.hip header): the norm
T(w T(x rstd)), T(acc), T(resid + T(acc)), swiglu()'s chain, T(logit). A kernel's fp32 accumulator is not the exact sum y; it lies within an
absolute allowance `al` of it, made of two derived parts and nothing else:

  accumulation   c 2^-24 sum_k |x_k| |w_k|, c = the longest chain of fp32 additions a product goes through. An MFMA 16x16x32 adds 32 products to
                 its accumulator in an undocumented order: counted as 32 (sequential, the worst case). Then one addition per further chunk of the
                 wave, one per wave of the fixed-order LDS reduction, one per K-group slab:
                   xstat16_k           32 + 16 chunks + 8 waves              = 56
                   xrow16_k            32 + ceil(K / 32 / 16) chunks + 16    = 49 .. 70   (70 at K = 11008: 22 chunks; more than the issue's 64,
                                                                                          because the MFMA is counted sequentially)
                   xstat32_k<BLK>      32 + 16 + 8                           = 56
                   xsplit32_k<BLK>     32 + 11 chunks + 8 waves (+ 4 slabs)  = 51 (55)
                 (sum |x||w| itself is evaluated in fp32: 1e-6 of an allowance)
  rstd           the RMSNorm statistics are fp32. xstat16_k: 7 roundings per lane (8 squares, exact products of 11-bit values), 6 in wave_sum, 7
                 across the waves, 1 for + eps (the division by 4096 is exact): the mean square is within 21 x 2^-24, rsqrt halves that (10.5) and
                 v_rsq_f32 adds one fp32 ulp (<= 2 x 2^-24), the product x rstd is rounded to fp32 once more (1): 13.5 x 2^-24. rmsnorm4096_k
                 (15 + 6 + 3 + 1 = 25 roundings) comes to 15.5. Both are below RSTD_REL = 2^-20. An element whose exact x rstd has a rounding
                 boundary of T within that relative distance may round either way; w T(.) follows. rms_ref returns, per element, how far the other
                 candidate lies from the reference (0 for all but ~2^-9 of the fp16 elements), and gemm_ref adds |w_nk| times that to output n.

Rounding is monotone, so an accumulator in [y - al, y + al] gives an output in [T(y - al), T(y + al)], and a monotone chain of roundings maps
interval ends to interval ends. The bars below are those intervals, evaluated with the kernel's own fp32 operations where they are exact:

  plain / logits   out in [T(y - al), T(y + al)]                      (implies |out - T(y)| <= al + 1 ulp, the one-ulp bar)
  residual         out in [T(r + T(y - al)), T(r + T(y + al))]        (the inner ulp is carried through the outer rounding)
  SwiGLU           g in [T(yg - al), T(yg + al)], u alike; s = T(silu(g)) over both ends of g, each widened by the fp32 evaluation's own error
                   (x / (1 + expf(-x)): expf one ulp, the sum and the correctly rounded quotient half an ulp each: SILU_REL = 4 x 2^-24); out in the
                   hull of T(s u) over the four corners (s u is exact in fp32: two 11-bit factors). silu is not monotone around -1.28, but g takes
                   only the T values of its interval, which are its two ends unless the allowance spans more than an ulp.

`check` reports the worst excess over the interval and the worst distance from the centre T(...) in ulps (what the test prints)."""
import math

import torch

DT = {"f16": torch.float16, "bf16": torch.bfloat16}
MANT = {torch.float16: 10, torch.bfloat16: 7}
MIN_NORMAL = {torch.float16: 2.0 ** -14, torch.bfloat16: 2.0 ** -126}
U32 = 2.0 ** -24
RSTD_REL = 2.0 ** -20
SILU_REL = 2.0 ** -22
EPS = 1e-6
EPS32 = float(torch.tensor(EPS, dtype=torch.float32))          # what the kernels receive


def T(x, dt):
    return x.to(dt).double()


def ulp(x, dt):
    """Spacing of the model dtype at |x| (fp64; subnormal spacing below the smallest normal)."""
    a = x.double().abs().clamp_min(MIN_NORMAL[dt])
    return torch.exp2(torch.floor(torch.log2(a)) - MANT[dt])


def c_xstat16():
    return 32 + 16 + 8


def c_xrow16(K):
    return 32 + math.ceil(K / 32 / 16) + 16


def c_xstat_blk():
    return 32 + 16 + 8


def c_xsplit_blk(combine=True):
    return 32 + 11 + 8 + (4 if combine else 0)


# ---- layouts, restated from the comments of xs16.hip / xstat32.hip: [k / 32][row tiles][lane = 16 g + r][8], g = (k % 32) / 8, r = row % 16 ----
def unpack_frag(buf):
    """[K / 32, MT, 64, 8] -> rows [16 MT, K]."""
    KB, MT = buf.shape[:2]
    return buf.reshape(KB, MT, 4, 16, 8).permute(1, 3, 0, 2, 4).reshape(16 * MT, 32 * KB)


def pack_frag(rows, MT):
    """rows [M <= 16 MT, K] -> [K / 32, MT, 64, 8], pad rows zero."""
    M, K = rows.shape
    full = torch.zeros(16 * MT, K, dtype=rows.dtype)
    full[:M] = rows
    return full.reshape(MT, 16, K // 32, 4, 8).permute(2, 0, 3, 1, 4).reshape(K // 32, MT, 64, 8).contiguous()


def unpack_frag64(buf):
    """One 32-row block in the fp8 kernels' 64-deep order [f][2 row tiles][lane = 16 g + r][8], f = 2 (k / 64) + (k % 16) / 8, g = (k % 64) / 16
    (ActLayout value 2, csrc/rdx_kernels.h) -> rows [32, K]. buf: flat, 32 K elements."""
    K = buf.numel() // 32
    b = buf.reshape(K // 64, 2, 2, 4, 16, 8)                    # [k / 64][h = (k % 16) / 8][mt][g][r][j]
    return b.permute(2, 4, 0, 3, 1, 5).reshape(32, K)           # row = 16 mt + r, k = 64 (k / 64) + 16 g + 8 h + j


def unpack_frag64_e4m3(buf):
    """The byte-order twin for the e4m3 block (ActLayout value 4): one 32-row block [k / 64][2 row tiles][lane = 16 g + r][16 bytes = k % 16],
    g = (k % 64) / 16 -> codes [32, K]. buf: flat, 32 K bytes."""
    K = buf.numel() // 32
    return buf.reshape(K // 64, 2, 4, 16, 16).permute(1, 3, 0, 2, 4).reshape(32, K)


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------
def make_rows(M, K, dt, seed, scales=True):
    """Rows that differ from each other: independent noise, (scales) a power-of-two scale per row that survives where no norm follows, and row 1
    with a mean square near eps = 1e-6 so that eps x 10 shows behind a norm."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g)
    if scales:
        x = x * torch.exp2(((torch.arange(M) * 5) % 7 - 3).float()).view(M, 1) * 0.5
    if M > 1:
        x[1] = torch.randn(K, generator=g) * 1e-3
    return x.to(dt)


def make_norm_w(K, dt, seed):
    g = torch.Generator().manual_seed(seed)
    return (1.0 + 0.2 * torch.randn(K, generator=g)).to(dt)


def make_w(N, K, dt, seed, std=0.02):
    """fp32 weights that are exactly representable in the model dtype (the production packer's rounding is then the identity)."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(N, K, generator=g) * std).to(dt).float()


# ---- references -----------------------------------------------------------------------------------------------------------------------------
def rms_ref(x, nw, dt, eps=EPS32, delta=RSTD_REL):
    """(xn, dxn, lo, hi): xn = T(w T(x rstd)) in fp64; lo / hi = the same through T(x rstd (1 -+ delta)) ordered, dxn = how far they lie from xn."""
    xd = x.double()
    rstd = 1.0 / torch.sqrt((xd * xd).mean(-1, keepdim=True) + eps)
    y = xd * rstd
    w = nw.to(dt).double()
    xn = T(w * T(y, dt), dt)
    a, b = T(w * T(y * (1 - delta), dt), dt), T(w * T(y * (1 + delta), dt), dt)
    return xn, torch.maximum((a - xn).abs(), (b - xn).abs()), torch.minimum(a, b), torch.maximum(a, b)


def gemm_ref(xn, w, c, dxn=None):
    """(y, al): y = xn w^T in fp64 (xn fp64 values of the model dtype, w fp32 [N, K]); al = c 2^-24 sum |x||w| (+ sum_k |w_nk| dxn_k)."""
    y = xn @ w.double().t()
    al = c * U32 * (xn.abs().float() @ w.abs().t()).double()
    if dxn is not None:
        cols = (dxn > 0).any(0).nonzero().flatten()
        if cols.numel():
            al = al + dxn[:, cols] @ w[:, cols].double().abs().t()
    return y, al


def silu64(g):
    return g / (1.0 + torch.exp(-g))


def bar_plain(y, al, dt):
    return T(y - al, dt), T(y + al, dt), T(y, dt), al


def _add32(r, a, dt):
    return (r.float() + a.float()).to(dt).double()             # the kernel's fp32 sum of two model-dtype values, then its store


def bar_resid(y, al, resid, dt):
    r = resid.to(dt)
    return _add32(r, T(y - al, dt), dt), _add32(r, T(y + al, dt), dt), _add32(r, T(y, dt), dt), al + ulp(T(y, dt), dt)


def bar_swiglu(y, al, dt):
    """y, al [M, N] with W's 16-row tiles = 8 gate rows, then the 8 matching up rows -> (lo, hi, centre) [M, N / 2]."""
    M, N = y.shape
    y4, a4 = y.reshape(M, N // 16, 2, 8), al.reshape(M, N // 16, 2, 8)
    g, u, ag, au = y4[:, :, 0], y4[:, :, 1], a4[:, :, 0], a4[:, :, 1]
    ss = []
    for gv in (T(g - ag, dt), T(g + ag, dt)):
        s = silu64(gv)
        e = SILU_REL * s.abs()
        ss += [T(s - e, dt), T(s + e, dt)]
    s_lo, s_hi = torch.stack(ss).amin(0), torch.stack(ss).amax(0)
    corners = torch.stack([(s.float() * uv.float()).to(dt).double() for s in (s_lo, s_hi) for uv in (T(u - au, dt), T(u + au, dt))])
    centre = (T(silu64(T(g, dt)), dt).float() * T(u, dt).float()).to(dt).double()
    return corners.amin(0).reshape(M, N // 2), corners.amax(0).reshape(M, N // 2), centre.reshape(M, N // 2), None


def check(out, bar, dt):
    """(inside the interval everywhere and finite; worst excess over the interval in ulps; worst distance from the centre T(ref) in ulps at the
    larger of the two magnitudes, after the bar's absolute allowance -- plain: al, the one-ulp bar; residual: al + the inner rounding's ulp,
    which the outer rounding carries through; SwiGLU: none, the raw distance)."""
    lo, hi, centre, al = bar
    o = out.double().cpu()
    u = ulp(torch.maximum(o.abs(), centre.abs()), dt)
    ex = torch.maximum(torch.maximum(lo - o, o - hi), torch.zeros_like(o)) / u
    ex = torch.where(torch.isfinite(o), ex, torch.full_like(ex, float("inf")))
    d = (o - centre).abs() - (0.0 if al is None else al)
    return bool(ex.max() == 0), float(ex.max()), float((d.clamp_min(0.0) / u).max())


def sensitive(out, bar, dt, name):
    """A perturbed reference must fail the same bar."""
    ok, ex, _ = check(out, bar, dt)
    assert not ok, f"the bar does not see {name}"
    return ex


def first_argmax(logits):
    """argmax over the last dim, lowest index on ties (torch.argmax of a model-dtype row, greedy_search)."""
    f = logits.float()
    n = f.shape[-1]
    idx = torch.arange(n).expand_as(f)
    return torch.where(f == f.amax(-1, keepdim=True), idx, torch.full_like(idx, n)).amin(-1)


# ---- perturbations: what a plausible bug computes (applied to the reference's operands) -------------------------------------------------------
def drop_piece(xn, k0):
    """One 8-element K piece (one lane group of one chunk of one wave's range) missing."""
    x = xn.clone()
    x[:, k0:k0 + 8] = 0
    return x


def swap_chunks(w, c):
    """Two adjacent 32-deep chunks exchanged in the weight only."""
    w2 = w.clone()
    w2[:, 32 * c:32 * c + 32], w2[:, 32 * c + 32:32 * c + 64] = w[:, 32 * c + 32:32 * c + 64], w[:, 32 * c:32 * c + 32]
    return w2


def swap_gate_up(w, tile):
    """Gate and up halves of one 16-row weight tile exchanged."""
    w2 = w.clone()
    w2[16 * tile:16 * tile + 8], w2[16 * tile + 8:16 * tile + 16] = w[16 * tile + 8:16 * tile + 16], w[16 * tile:16 * tile + 8]
    return w2


def neighbour_row(x):
    """The last row replaced by its neighbour (a ragged tile whose last lane reads one row up)."""
    x2 = x.clone()
    x2[-1] = x[-2]
    return x2


# ---- fp32 emulations of the kernels (torch fp32, the kernels' order of partial sums) ----------------------------------------------------------
def emu_norm(x, nw, dt, eps=EPS32):
    xf = x.float()
    rs = torch.rsqrt((xf * xf).sum(-1, keepdim=True) / x.shape[1] + torch.tensor(eps, dtype=torch.float32))
    return (nw.to(dt).float() * (xf * rs).to(dt).float()).to(dt)


def wave_slices(KC, waves):
    """Chunk ranges [KC s / waves, KC (s + 1) / waves) of xrow16_k / xsplit32_k; xstat16_k / xstat32_k: KC = 128, 8 waves."""
    return [range(KC * s // waves, KC * (s + 1) // waves) for s in range(waves)]


def emu_gemm(xn, w, slices):
    """fp32 [M, N]: one fp32 partial per 32-deep chunk, added chunk by chunk within a wave, then wave by wave."""
    xf, wf = xn.float(), w.float()
    total = None
    for sl in slices:
        acc = torch.zeros(xf.shape[0], wf.shape[0])
        for c in sl:
            acc = acc + xf[:, 32 * c:32 * c + 32] @ wf[:, 32 * c:32 * c + 32].t()
        total = acc if total is None else total + acc
    return total


def emu_resid(acc, resid, dt):
    return (resid.to(dt).float() + acc.to(dt).float()).to(dt)


def emu_swiglu(acc, dt):
    M, N = acc.shape
    a4 = acc.reshape(M, N // 16, 2, 8)
    g, u = a4[:, :, 0].to(dt).float(), a4[:, :, 1].to(dt).float()
    s = (g / (1.0 + torch.exp(-g))).to(dt).float()
    return (s * u).to(dt).reshape(M, N // 2)


def combine_slabs(slabs, resid, dt):
    """x += T(sum of the slabs in group order): the fp32 arithmetic of rmsnorm4096_k's slab prologue, exactly."""
    acc = torch.zeros_like(slabs[0])
    for s in slabs:
        acc = acc + s
    return (resid.to(dt).float() + acc.to(dt).float()).to(dt)
