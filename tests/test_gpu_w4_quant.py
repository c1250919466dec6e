"""The device quantiser of the int4 group-quantised weights (csrc/gemm.hip quant_w4_k, through rdx_w4_test) against its definition
radialog_amd/w4.py: the packed bf16 copy of the dequantised weight bit for bit, the stream and the scales byte for byte. And the refusals of
rdx_set_weight(RDX_W_GEMM_W4): -8 with a message in an f16 context, for K % 128 != 0 and next to fp8 weights; -1 for a NaN."""
import ctypes as C

import numpy as np
import pytest
import torch

from radialog_amd import _lib, w4, wcode
from radialog_amd.config import small_cfg

pytestmark = pytest.mark.gpu


def _engine(dtype="bf16"):
    from radialog_amd.engine import RdxEngine
    return RdxEngine(small_cfg(), dtype=dtype, device=0, max_batch=1, max_len=64, vision=False, llama=False)


@pytest.fixture(scope="module")
def eng():
    e = _engine()
    yield e
    e.close()


def _check(eng, w):
    wn = w.numpy()
    n, k = wn.shape
    wprime, stream, scales = eng.w4_test(w)
    q, s = w4.quantize(wn)
    want_stream = w4.pack(q, s)
    assert (stream == want_stream).all(), "stream bytes"
    nt = (n + 15) // 16
    sfull = np.zeros((nt * 16, k // 128), dtype=np.uint16)
    sfull[:n] = s
    assert (scales == sfull.reshape(nt, 16, k // 128).transpose(0, 2, 1)).all(), "scales"
    assert (wprime == wcode.pack_bf16(w4.bf16_bits(w4.dequantize(q, s)))).all(), "W' bits"
    assert (wprime == w4.packed_wprime(wn)).all()
    return q, s


@pytest.mark.parametrize("N,K", [(16, 128), (40, 384), (48, 4096), (16, 11008)])
def test_device_quantiser_equals_the_definition(eng, N, K):
    g = torch.Generator().manual_seed(N * 131 + K)
    w = torch.randn(N, K, generator=g) * 0.02
    q, _ = _check(eng, w)
    assert np.abs(q).max() == 7


def test_planted_groups(eng):
    g = torch.Generator().manual_seed(9)
    w = torch.randn(40, 384, generator=g) * 0.02
    w[3, 128:256] = 0.0                       # an all-zero group: s = 0
    w[17, 300] = 0.02 * 2.0 ** 20             # one outlier 2^20 times its neighbours: everything else of the group quantises to 0
    w[33, 0:128] = 1e-40                      # a / 7 rounds to a zero scale
    w[5, 7] = -0.0
    w[6, 0:128] = torch.tensor([0.5, 1.5, 2.5, 3.5, -0.5, -1.5, -2.5, 7.0]).repeat(16)      # s = 1: half-way quotients, to even
    q, s = _check(eng, w)
    assert s[3, 1] == 0 and not q[3, 128:256].any()
    assert q[17, 300] == 7 and np.count_nonzero(q[17, 256:384]) == 1
    assert s[33, 0] == 0 and not q[33, 0:128].any()
    assert list(q[6, :8]) == [0, 2, 2, 4, 0, -2, -2, 7]


def test_nan_and_inf_are_refused(eng):
    for bad in (float("nan"), float("inf")):
        w = torch.randn(16, 128) * 0.02
        w[9, 77] = bad
        with pytest.raises(_lib.RdxError, match=r"\(-1\).*Inf or a NaN"):
            eng.w4_test(w)


def _set_weight(e, name, w, kind):
    w = w.to(e.device, torch.float32).contiguous()
    torch.cuda.synchronize(e.device)
    rc = e.lib.rdx_set_weight(e.ctx, name.encode(), C.c_void_p(w.data_ptr()), w.shape[0], w.shape[1], kind)
    msg = e.lib.rdx_last_error(e.ctx)
    return rc, (msg.decode() if msg else "")


def test_refusals_of_set_weight():
    w = torch.randn(32, 256) * 0.02
    e = _engine("f16")
    try:
        rc, msg = _set_weight(e, "a", w, _lib.RDX_W_GEMM_W4)
        assert rc == -8 and "f16" in msg
    finally:
        e.close()
    e = _engine("bf16")
    try:
        rc, msg = _set_weight(e, "a", torch.randn(32, 192) * 0.02, _lib.RDX_W_GEMM_W4)
        assert rc == -8 and "128" in msg
        wn = w.clone()
        wn[1, 1] = float("nan")
        rc, msg = _set_weight(e, "a", wn, _lib.RDX_W_GEMM_W4)
        assert rc == -1 and msg
        assert _set_weight(e, "a", w, _lib.RDX_W_GEMM_W4)[0] == 0          # (the refused calls left nothing behind under the name)
        rc, msg = _set_weight(e, "b", w, _lib.RDX_W_GEMM_FP8)
        assert rc == -8 and "W4" in msg
    finally:
        e.close()
    e = _engine("bf16")
    try:
        assert _set_weight(e, "f", w, _lib.RDX_W_GEMM_FP8)[0] == 0
        rc, msg = _set_weight(e, "a", w, _lib.RDX_W_GEMM_W4)
        assert rc == -8 and "FP8" in msg
    finally:
        e.close()
