"""The batch <= 2 GEMV on int4 group-quantised weights (skinny_gemm_w4_k: 4.125 bits per weight, decoded in registers to the dequantised bf16 value;
radialog_amd/w4.py is the format) against the same GEMV on the packed bf16 weights W' = dequantize(quantize(W)): same operands, same K split over the
waves, same MFMA order -- the tolerance is zero, outputs are compared as bit patterns. rdx_gemm_test force 13 quantises W itself and must equal force 1
on W'. The cases are those of tests/test_gpu_wcode_gemv.py (K = 128 / 384 / 4096 / 11008, N = 16 / 40 / 784 / 8208, M = 1 / 2, epilogues 0 / 3 / 4, with
and without the fused RMSNorm: every wave count, partial first and last chunks of a wave's K slice, a padded last tile), plus a raw tile between two
int4 tiles (force 14), the situation of the LoRA-A rows inside the fused QKV weight."""
import pytest
import torch

from radialog_amd import _lib, w4
from radialog_amd.config import small_cfg
from test_gpu_wcode_gemv import CASES, _bits, _operands

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from radialog_amd.engine import RdxEngine
    e = RdxEngine(small_cfg(), dtype="bf16", device=0, max_batch=1, max_len=64, vision=False, llama=False)
    yield e
    e.close()


def _wprime(w, raw_rows=None):
    """dequantize(quantize(w)) as an fp32 tensor on w's device; rows in raw_rows keep bf16(w)."""
    wn = w.cpu().numpy()
    wp = torch.from_numpy(w4.dequantize(w4.quantize(wn)))
    if raw_rows is not None:
        wp[raw_rows] = w.cpu()[raw_rows].to(torch.bfloat16).float()
    return wp.to(w.device)


def _both(eng, x, w, nw, r, epi, norm, force=13, raw_rows=None):
    kw = dict(epi=epi, norm_w=nw if norm else None, resid=r if epi == 3 else None)
    ref = eng.gemm_test(x, _wprime(w, raw_rows), force=1, **kw)
    got = eng.gemm_test(x, w, force=force, **kw)
    assert torch.isfinite(ref.float()).all() and ref.float().abs().max() > 0
    return ref, got


@pytest.mark.parametrize("M,N,K,epi,norm", CASES)
def test_w4_gemv_equals_the_bf16_gemv_on_the_dequantised_weight(eng, M, N, K, epi, norm):
    x, w, nw, r = _operands(M, N, K, seed=K + N + M)
    ref, got = _both(eng, x, w, nw, r, epi, norm)
    assert torch.equal(_bits(ref), _bits(got))
    # the weight is not what it was: int4 moved the result (a hook that multiplied the unquantised W would equal force 1 on W instead)
    plain = eng.gemm_test(x, w, force=1, epi=epi, norm_w=nw if norm else None, resid=r if epi == 3 else None)
    assert not torch.equal(_bits(plain), _bits(got))


@pytest.mark.parametrize("K", [384, 4096])
def test_a_raw_tile_between_int4_tiles(eng, K):
    """Tile 1 of 3 is left un-quantised and flagged raw (force 14): it streams its packed bf16 bytes, next to int4 tiles."""
    x, w, nw, r = _operands(2, 48, K, seed=11)
    raw = slice(16, 32)
    for epi, norm in ((0, True), (3, False)):
        ref, got = _both(eng, x, w, nw, r, epi, norm, force=14, raw_rows=raw)
        assert torch.equal(_bits(ref), _bits(got))
        allq, _ = _both(eng, x, w, nw, r, epi, norm)
        assert torch.equal(_bits(allq)[:, :16], _bits(got)[:, :16]) and torch.equal(_bits(allq)[:, 32:], _bits(got)[:, 32:])
        assert not torch.equal(_bits(allq)[:, 16:32], _bits(got)[:, 16:32])


def test_zero_groups_and_tiny_scales(eng):
    x, w, nw, r = _operands(1, 48, 4096, seed=12)
    w[3, 128:256] = 0.0             # s = 0
    w[20, :] = 0.0
    w[41, 0:128] = 1e-40           # the scale underflows to 0
    w[42, 256:384] *= 2.0 ** 20    # a large group next to small ones
    ref, got = _both(eng, x, w, nw, r, 0, True)
    assert torch.equal(_bits(ref), _bits(got))


def test_two_rows_of_11008_have_no_w4_form(eng):
    x, w, nw, r = _operands(2, 16, 11008, seed=13)
    with pytest.raises(_lib.RdxError, match="force 13"):
        eng.gemm_test(x, w, force=13)
