"""The 3-16-row GEMM kernels on int4 group-quantised weights (xs16.hip: xstat16_w4_k, xrow16_w4_k; radialog_amd/w4.py is the format) against the bf16
kernels of the same family on W' = dequantize(quantize(W)): same operands, same K split over the waves, same MFMA order -- the tolerance is zero,
outputs are compared as bit patterns (the unwritten, NaN-filled parts of the buffers included). rdx_xstat16_w4_test / rdx_xrow16_w4_test quantise W with
the production quantiser and must equal rdx_xstat16_test / rdx_xrow16_test on W'; raw rows keep bf16(W). Every case also differs from the bf16 kernel on
the unquantised W: a hook that forgot to quantise would equal that one.

xstat16 (K = 4096). N = 8192: 512 tiles, the kernel's minimum, one trip per workgroup (no prefetch). N = 8240: 515 tiles = 258 groups on 129 workgroups
with two trips each -- the prefetching trip runs -- and the last group holds one tile. N = 8232: the same 515 tiles with the last one padded (8 real
rows: for SwiGLU its gate rows without their up rows); the bf16 hook takes N % 16 == 0 only, so its reference is N = 8240 on W' with 8 zero rows
behind it, compared over the columns < 8232, and the int4 kernel must leave the columns from 8232 on unwritten. N = 12304, raw_lo = 12288: the production QKV with its raw LoRA-A tile at the
end, 385 groups on 256 workgroups, one or two trips. N = 8240 with tile 257 raw: a raw tile between int4 tiles, in the second trip of its workgroup.
xrow16 (N = 16 / 48). K = 512: one fragment per wave, four waves share each int4 chunk; 640: 20 fragments, uneven slices; 4096: aligned slices of two
chunks; 11008: the production down_proj, every slice edge inside a chunk (first trip + tail); 19840: 155 chunks, nine or ten per wave -- the only
size here at which the unguarded middle trips run."""
import numpy as np
import pytest
import torch

from radialog_amd import w4
from radialog_amd.config import small_cfg

pytestmark = pytest.mark.gpu

K16 = 4096
N_MAX = 12304


@pytest.fixture(scope="module")
def eng():
    from radialog_amd.engine import RdxEngine
    e = RdxEngine(small_cfg(), dtype="bf16", device=0, max_batch=1, max_len=32, llama=False, vision=False)
    yield e
    e.close()


def _bits(t):
    return t.contiguous().view(torch.int16)


def _wprime(w, raw=None):
    """dequantize(quantize(w)) as an fp32 tensor on w's device; the rows of the slice `raw` keep bf16(w)."""
    wp = torch.from_numpy(w4.dequantize(w4.quantize(w.cpu().numpy())))
    if raw is not None:
        wp[raw] = w.cpu()[raw].to(torch.bfloat16).float()
    return wp.to(w.device)


@pytest.fixture(scope="module")
def stat_ops():
    """x [16, 4096], the norm weight, W fp32 [12304, 4096] and its W' (every row quantised): made once, the cases take leading rows of them."""
    g = torch.Generator(device="cuda").manual_seed(1604)
    x = torch.randn(16, K16, generator=g, device="cuda").to(torch.bfloat16)
    nw = (1.0 + 0.1 * torch.randn(K16, generator=g, device="cuda")).to(torch.bfloat16)
    w = torch.randn(N_MAX, K16, generator=g, device="cuda") * 0.02
    return x, nw, w, _wprime(w)


def _stat_case(eng, x, nw, w, wp, raw_lo, packed_too):
    N = w.shape[0]
    variants = [dict(epi=0, ldo=N + 24), dict(epi=4, ldo=N // 2 + 8)] + ([dict(epi=4, out_packed=1)] if packed_too else [])
    for M in (3, 8, 12, 16):
        for kw in variants:
            ref = eng.xstat16_test(x[:M], nw, wp, **kw)
            got = eng.xstat16_w4_test(x[:M], nw, w, raw_lo=raw_lo, **kw)
            plain = eng.xstat16_test(x[:M], nw, w, **kw)
            live = ref[:M] if not kw.get("out_packed") else ref[:, 0, :, :]
            assert torch.isfinite(live.float()).any() and live.float().nan_to_num().abs().max() > 0
            assert torch.equal(_bits(ref), _bits(got)), f"M = {M}, {kw}: int4 kernel != bf16 kernel on W'"
            assert not torch.equal(_bits(plain), _bits(got)), f"M = {M}, {kw}: the hook did not quantise"


@pytest.mark.parametrize("N", [8192, 8240])
def test_xstat16_w4_equals_xstat16_on_the_dequantised_weight(eng, stat_ops, N):
    x, nw, w, wp = stat_ops
    _stat_case(eng, x, nw, w[:N].contiguous(), wp[:N].contiguous(), None, N % 64 == 0)


def test_xstat16_w4_padded_last_tile(eng, stat_ops):
    """N = 8232: tile 514 holds rows 8224 .. 8231 and 8 rows of padding. epi 0: columns < 8232 are the reference's, the rest of every row stays NaN
    (the `n < N` guard). epi 4, row-major: the tile's 8 gate rows meet absent (zero) up rows -- the whole buffer equals the reference's, which
    multiplies explicit zero rows, and the columns behind the tile's 8 stay NaN."""
    x, nw, w, wp = stat_ops
    N, NP = 8232, 8240
    w8 = w[:N].contiguous()
    zeros = torch.zeros(NP - N, K16, device=w.device)
    wp_pad, w_pad = torch.cat([wp[:N], zeros]), torch.cat([w8, zeros])
    for M in (3, 8, 12, 16):
        ref = eng.xstat16_test(x[:M], nw, wp_pad, epi=0, ldo=NP + 24)
        got = eng.xstat16_w4_test(x[:M], nw, w8, epi=0, ldo=NP + 24)
        plain = eng.xstat16_test(x[:M], nw, w_pad, epi=0, ldo=NP + 24)
        assert torch.isfinite(ref[:M, :NP].float()).all() and (ref[:M, N:NP].float() == 0).all()
        assert torch.equal(_bits(ref)[:, :N], _bits(got)[:, :N]), f"M = {M}, epi 0: int4 kernel != bf16 kernel on W'"
        assert torch.isnan(got[:, N:].float()).all() and torch.isnan(got[M:].float()).all(), f"M = {M}, epi 0: a column >= N or a row >= M was written"
        assert not torch.equal(_bits(plain)[:, :N], _bits(got)[:, :N])
        ref = eng.xstat16_test(x[:M], nw, wp_pad, epi=4, ldo=NP // 2 + 8)
        got = eng.xstat16_w4_test(x[:M], nw, w8, epi=4, ldo=NP // 2 + 8)
        plain = eng.xstat16_test(x[:M], nw, w_pad, epi=4, ldo=NP // 2 + 8)
        assert torch.isfinite(ref[:M, :NP // 2].float()).all()
        assert torch.equal(_bits(ref), _bits(got)), f"M = {M}, epi 4: int4 kernel != bf16 kernel on W'"
        assert torch.isnan(got[:, NP // 2:].float()).all() and torch.isnan(got[M:].float()).all()
        assert not torch.equal(_bits(plain), _bits(got))


def test_xstat16_w4_production_qkv_with_its_raw_tile(eng, stat_ops):
    x, nw, w, wp = stat_ops
    wp = wp.clone()
    wp[12288:] = w[12288:].to(torch.bfloat16).float()
    _stat_case(eng, x, nw, w, wp, 12288, False)


def test_xstat16_w4_raw_tile_between_int4_tiles(eng, stat_ops):
    x, nw, w, wp = stat_ops
    N, lo = 8240, 257 * 16
    w, wp = w[:N].contiguous(), wp[:N].clone()
    wp[lo:lo + 16] = w[lo:lo + 16].to(torch.bfloat16).float()
    _stat_case(eng, x, nw, w, wp, -lo, False)
    # the tiles around the raw one are what they are without it
    allq = eng.xstat16_w4_test(x[:12], nw, w)
    got = eng.xstat16_w4_test(x[:12], nw, w, raw_lo=-lo)
    assert torch.equal(_bits(allq)[:, :lo], _bits(got)[:, :lo]) and torch.equal(_bits(allq)[:, lo + 16:], _bits(got)[:, lo + 16:])
    assert not torch.equal(_bits(allq)[:12, lo:lo + 16], _bits(got)[:12, lo:lo + 16])


def test_xstat16_w4_zero_groups_and_tiny_scales(eng, stat_ops):
    x, nw, w, _ = stat_ops
    w = w[:8192].clone()
    w[3, 128:256] = 0.0             # s = 0
    w[20, :] = 0.0
    w[41, 0:128] = 1e-40            # the scale underflows to 0
    w[42, 256:384] *= 2.0 ** 20     # a large group next to small ones
    wp = _wprime(w)
    for M in (3, 16):
        ref = eng.xstat16_test(x[:M], nw, wp)
        got = eng.xstat16_w4_test(x[:M], nw, w)
        assert torch.isfinite(ref[:M].float()).all()
        assert torch.equal(_bits(ref), _bits(got))
        assert (ref[:M, 20].float() == 0).all()
        assert not torch.equal(_bits(eng.xstat16_test(x[:M], nw, w)), _bits(got))


@pytest.fixture(scope="module")
def row_ops():
    """Per K: x [16, K], W fp32 [48, K], its W' and a residual [16, 48], made once; the cases take leading rows / columns of them."""
    out = {}
    for K in (512, 640, 4096, 11008, 19840):
        g = torch.Generator(device="cuda").manual_seed(7000 + K)
        x = torch.randn(16, K, generator=g, device="cuda").to(torch.bfloat16)
        w = torch.randn(48, K, generator=g, device="cuda") * 0.02
        r = torch.randn(16, 48, generator=g, device="cuda").to(torch.bfloat16)
        out[K] = (x, w, _wprime(w), r)
    return out


def _pack_blk32(x, M):
    """Rows 0 .. M of x as the fragment-packed 32-row block (rdx_kernels.h ACT_BLK32): [k / 32][2 row tiles][lane = 16 ((k % 32) / 8) + row][8], other rows zero."""
    K = x.shape[1]
    blk = torch.zeros(K // 32, 2, 64, 8, dtype=x.dtype, device=x.device)
    # row m, k = 32 c + 8 g + e  ->  blk[c, 0, 16 g + m, e]
    v = x[:M].reshape(M, K // 32, 4, 8).permute(1, 2, 0, 3)          # [c, g, m, e]
    for gi in range(4):
        blk[:, 0, 16 * gi:16 * gi + M, :] = v[:, gi]
    return blk


@pytest.mark.parametrize("N", [16, 48])
@pytest.mark.parametrize("K", [512, 640, 4096, 11008, 19840])
def test_xrow16_w4_equals_xrow16_on_the_dequantised_weight(eng, row_ops, K, N):
    x, w, wp, r = row_ops[K]
    w, wp, r = w[:N].contiguous(), wp[:N].contiguous(), r[:, :N].contiguous()
    for M in (3, 5, 9, 13, 16):
        for packed in (False, True):
            xin = _pack_blk32(x, M) if packed else x[:M]
            kw = dict(M=M) if packed else {}
            ref = eng.xrow16_test(xin, wp, r[:M], ldo=N + 8, **kw)
            got = eng.xrow16_w4_test(xin, w, r[:M], ldo=N + 8, **kw)
            plain = eng.xrow16_test(xin, w, r[:M], ldo=N + 8, **kw)
            assert torch.isfinite(ref[:M, :N].float()).all() and ref[:M, :N].float().abs().max() > 0
            assert torch.equal(_bits(ref), _bits(got)), f"M = {M}, packed = {packed}: int4 kernel != bf16 kernel on W'"
            assert not torch.equal(_bits(plain), _bits(got)), f"M = {M}, packed = {packed}: the hook did not quantise"
        if M == 16:
            # the packed block built here is the one the re-layout launch builds
            assert torch.equal(_bits(eng.xrow16_test(_pack_blk32(x, 16), wp, r, M=16)), _bits(eng.xrow16_test(x, wp, r)))


def test_shapes_without_an_int4_form_are_refused(eng, stat_ops, row_ops):
    from radialog_amd._lib import RdxError
    x, nw, w, _ = stat_ops
    with pytest.raises(RdxError, match="xstat16_w4_k"):
        eng.xstat16_w4_test(x[:2], nw, w[:8192])                       # 2 rows
    with pytest.raises(RdxError, match="xstat16_w4_k"):
        eng.xstat16_w4_test(x[:8], nw, w[:4096])                       # 256 tiles
    xr, wr, _, r = row_ops[512]
    with pytest.raises(RdxError, match="K % 128"):
        eng.xrow16_w4_test(xr[:8, :480], wr[:16, :480].contiguous(), r[:8, :16].contiguous())
