"""The batch <= 2 GEMV on coded bf16 weights (skinny_gemm_wc_k: 13 bits per weight, decoded in registers; radialog_amd/wcode.py is the format) against
the same GEMV on the raw packed weights: same operands, same K split over the waves, same MFMA order -- the tolerance is zero, outputs are compared
as bit patterns. rdx_gemm_test force 12 encodes W itself and must equal force 1; the logits epilogue goes through rdx_logits_test (mode 2 against
mode 0), because rdx_gemm_test has no argmax partials to hand it. The device encoder is compared with the Python one byte for byte.

Shapes: K = 128 (one coded chunk) and 384 (three: most waves of a tile get an empty slice, the others a part of a chunk), 4096, and 11008 = 344 packed
chunks over 16 waves (21.5 each: every wave's slice starts or ends inside a coded chunk); N = 16, 40 (a padded last tile), 784 (49 tiles: the 16-wave
form at K >= 4096, the 8-wave form below) and 8208 (513 tiles: the 4-wave form, which exists up to M K = 8192). Two rows of K = 11008 do not fit the
GEMV's LDS stage: no coded form, the hook says so."""
import numpy as np
import pytest
import torch

from radialog_amd import _lib, wcode
from radialog_amd.config import small_cfg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from radialog_amd.engine import RdxEngine
    e = RdxEngine(small_cfg(), dtype="bf16", device=0, max_batch=1, max_len=64, vision=False, llama=False)
    yield e
    e.close()


def _operands(M, N, K, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(M, K, generator=g, device="cuda").to(torch.bfloat16)
    w = torch.randn(N, K, generator=g, device="cuda") * 0.02
    nw = (1.0 + 0.1 * torch.randn(K, generator=g, device="cuda")).to(torch.bfloat16)
    r = torch.randn(M, N, generator=g, device="cuda").to(torch.bfloat16)
    return x, w, nw, r


def _bits(t):
    return t.contiguous().view(torch.int16)


def _both(eng, x, w, nw, r, epi, norm):
    kw = dict(epi=epi, norm_w=nw if norm else None, resid=r if epi == 3 else None)
    raw = eng.gemm_test(x, w, force=1, **kw)
    cod = eng.gemm_test(x, w, force=12, **kw)
    assert torch.isfinite(raw.float()).all() and raw.float().abs().max() > 0
    return raw, cod


# M, N, K, epilogue (0 none, 3 + residual, 4 SwiGLU), fused RMSNorm
CASES = [(1, 16, 128, 0, True), (2, 16, 128, 3, False), (1, 40, 384, 0, True), (2, 40, 384, 3, False), (2, 784, 384, 4, True),
         (1, 784, 4096, 4, True), (2, 784, 4096, 0, True), (2, 16, 4096, 3, False),
         (1, 16, 11008, 3, False), (1, 40, 11008, 0, True), (1, 784, 11008, 4, True),
         (1, 8208, 4096, 0, True), (2, 8208, 4096, 4, True), (1, 8208, 4096, 3, False)]


@pytest.mark.parametrize("M,N,K,epi,norm", CASES)
def test_coded_gemv_equals_the_raw_gemv_bit_for_bit(eng, M, N, K, epi, norm):
    x, w, nw, r = _operands(M, N, K, seed=K + N + M)
    raw, cod = _both(eng, x, w, nw, r, epi, norm)
    assert torch.equal(_bits(raw), _bits(cod))


@pytest.mark.parametrize("M,N,K,n_valid", [(1, 8208, 4096, 8200), (2, 48, 384, 41), (1, 784, 11008, 784)])
def test_coded_logits_epilogue_equals_the_raw_one(eng, M, N, K, n_valid):
    x, w, _, _ = _operands(M, N, K, seed=7 * K + N)
    lr, ar = eng.logits_test(x, w, n_valid=n_valid, fp8=0)
    lc, ac = eng.logits_test(x, w, n_valid=n_valid, fp8=2)
    assert torch.equal(_bits(lr), _bits(lc)) and torch.equal(ar, ac)


@pytest.mark.parametrize("K", [384, 4096])
def test_a_fallback_tile_between_coded_ones(eng, K):
    """One weight of 1e-30 in tile 1 of 3: 70 binades under its neighbours, outside the window -- the tile is flagged and streams its raw bytes."""
    x, w, nw, r = _operands(2, 48, K, seed=11)
    w[16 + 5, K // 2 + 3] = 1e-30
    _, _, hdr = eng.wcode_test(w)
    assert list(hdr >> 8) == [0, 1, 0]
    for epi, norm in ((0, True), (3, False)):
        raw, cod = _both(eng, x, w, nw, r, epi, norm)
        assert torch.equal(_bits(raw), _bits(cod))


def test_zeros_are_coded_not_exceptions(eng):
    x, w, nw, r = _operands(1, 48, 4096, seed=12)
    w[3, 100] = 0.0
    w[20, :64] = 0.0
    w[40, 4000] = -0.0
    w[41, 7] = 1e-40          # rounds to a bf16 subnormal
    _, _, hdr = eng.wcode_test(w)
    assert not (hdr >> 8).any()
    raw, cod = _both(eng, x, w, nw, r, 0, True)
    assert torch.equal(_bits(raw), _bits(cod))


def test_two_rows_of_11008_have_no_coded_form(eng):
    x, w, nw, r = _operands(2, 16, 11008, seed=13)
    with pytest.raises(_lib.RdxError, match="force 12"):
        eng.gemm_test(x, w, force=12)


def test_device_encoder_equals_the_python_encoder_byte_for_byte(eng):
    g = torch.Generator().manual_seed(5)
    w = torch.randn(40, 384, generator=g) * 0.02
    w[0, 0] = 0.0
    w[1, 1] = -0.0
    w[2, 130] = 1e-40
    w[17, 200] = 1e-30        # tile 1 falls back; its planes are written all the same
    w[33, 383] = float("inf")  # tile 2 as well
    packed, planes, hdr = eng.wcode_test(w)
    want_packed = wcode.pack_bf16(w.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16))
    assert (packed == want_packed).all()
    want_planes, want_hdr = wcode.encode(want_packed)
    assert list(hdr >> 8) == [0, 1, 1] and (hdr == want_hdr).all()
    assert (planes == want_planes).all()
    assert (wcode.decode(planes, hdr)[0] == packed[0]).all()
