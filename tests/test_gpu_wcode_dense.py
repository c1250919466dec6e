"""The dense decode of the batch <= 2 GEMV on coded bf16 weights (skinny_gemm_wc_k, csrc/skinny_body.h): a tile whose dense word is set -- no weight
of index 0, csrc/gemm.hip encode_wc_k, radialog_amd/wcode.py dense() -- runs a twin of the coded K loop whose decode has no zero test. The reference is
the same GEMV on the raw packed weights (rdx_gemm_test force 1 against force 12, rdx_logits_test mode 0 against mode 2): same operands, same K split,
same MFMA order, so the tolerance is zero and outputs are compared as bit patterns.

Gaussian weights of 0.02 reach h = 0 (|w| < 2^-125) only as an exact zero of the generator, one weight in millions, so nearly every full tile of them
is dense: the cases of tests/test_gpu_wcode_gemv.py's shapes run the dense loop here and are asserted to (the device's dense words are read back). One launch holds a dense, a general and a raw tile side by side; the
window edges (index 1 and 15, base 0 and base 111) are planted."""
import numpy as np
import pytest
import torch

from radialog_amd import wcode
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


def _mostly_dense(d, full):
    """The first `full` tiles: all dense where they are few, at least 95 % of them otherwise (an exact 0.0 among millions of weights is not an error)."""
    return d[:full].all() if full < 20 else d[:full].sum() >= 0.95 * full


def _host_dense(w):
    return wcode.dense(wcode.pack_bf16(w.cpu().to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)))


# M, N, K, epilogue (0 none, 3 + residual, 4 SwiGLU), fused RMSNorm. K = 128: one chunk; 384: most waves get an empty or partial slice; 11008: slices
# off the chunk grid. N = 48 / 40 (a padded last tile: general): 8-wave form at K = 384, 16-wave at K >= 4096; N = 784: 8- and 16-wave; 8208: 4-wave.
CASES = [(1, 48, 128, 0, True), (2, 48, 128, 3, False), (1, 48, 384, 0, True), (2, 40, 384, 3, False), (2, 784, 384, 4, True),
         (1, 48, 4096, 3, False), (2, 48, 4096, 0, True), (1, 784, 4096, 4, True), (2, 784, 4096, 0, True),
         (1, 48, 11008, 3, False), (1, 40, 11008, 0, True), (1, 784, 11008, 4, True),
         (1, 8208, 4096, 0, True), (2, 8208, 4096, 4, True), (1, 8208, 4096, 3, False)]


@pytest.mark.parametrize("M,N,K,epi,norm", CASES)
def test_dense_tiles_equal_the_raw_gemv_bit_for_bit(eng, M, N, K, epi, norm):
    x, w, nw, r = _operands(M, N, K, seed=3 * K + N + M)
    d = eng.wcode_dense_test(w)
    assert (d == _host_dense(w)).all()
    assert _mostly_dense(d, N // 16) and (N % 16 == 0 or d[-1] == 0)          # the full tiles are dense, the padded one is not
    raw, cod = _both(eng, x, w, nw, r, epi, norm)
    assert torch.equal(_bits(raw), _bits(cod))


@pytest.mark.parametrize("M,N,K,n_valid", [(1, 8208, 4096, 8200), (2, 48, 384, 41), (1, 784, 11008, 784)])
def test_dense_logits_epilogue_equals_the_raw_one(eng, M, N, K, n_valid):
    x, w, _, _ = _operands(M, N, K, seed=5 * K + N)
    assert _mostly_dense(eng.wcode_dense_test(w), N // 16)
    lr, ar = eng.logits_test(x, w, n_valid=n_valid, fp8=0)
    lc, ac = eng.logits_test(x, w, n_valid=n_valid, fp8=2)
    assert torch.equal(_bits(lr), _bits(lc)) and torch.equal(ar, ac)


@pytest.mark.parametrize("K", [384, 4096])
def test_dense_general_and_raw_tiles_in_one_launch(eng, K):
    x, w, nw, r = _operands(2, 48, K, seed=21)
    w[16 + 3, 100] = 0.0                 # tile 1: index 0 three ways, still coded
    w[16 + 9, K - 1] = -0.0
    w[16 + 12, 7] = 1e-40                # rounds to a bf16 subnormal
    w[32 + 5, K // 2 + 3] = 1e-30        # tile 2: outside the window
    _, _, hdr = eng.wcode_test(w)
    d = eng.wcode_dense_test(w)
    assert list(d) == [1, 0, 0] and list(hdr >> 8) == [0, 0, 1]
    assert (d == _host_dense(w)).all()
    for epi, norm in ((0, True), (3, False), (4, True)):
        raw, cod = _both(eng, x, w, nw, r, epi, norm)
        assert torch.equal(_bits(raw), _bits(cod))
    lr, ar = eng.logits_test(x, w, n_valid=45, fp8=0)
    lc, ac = eng.logits_test(x, w, n_valid=45, fp8=2)
    assert torch.equal(_bits(lr), _bits(lc)) and torch.equal(ar, ac)


def _pow2_weights(N, K, exps, seed):
    """+-2^(e - 127) (1 + m / 128), e drawn from `exps` (biased bf16 exponents), m any 7-bit mantissa: exact in bf16."""
    g = torch.Generator().manual_seed(seed)
    e = torch.tensor(exps)[torch.randint(0, len(exps), (N, K), generator=g)]
    m = torch.randint(0, 128, (N, K), generator=g)
    s = torch.randint(0, 2, (N, K), generator=g)
    bits = ((s << 15) | (e << 7) | m).to(torch.int16)
    return bits.view(torch.bfloat16).float().cuda()


@pytest.mark.parametrize("name,exps,xscale", [
    ("index 1 and 15 only", [2 * 46, 2 * 46 + 1, 2 * 60, 2 * 60 + 1], 2.0 ** 10),
    ("top h = 126, base 111", list(range(2 * 112, 2 * 126 + 2)), 2.0 ** -120),
    ("top h <= 15, base 0", list(range(2, 2 * 15 + 2)), 2.0 ** 100),
])
def test_window_edges(eng, name, exps, xscale):
    M, N, K = 2, 32, 384
    x, _, nw, r = _operands(M, N, K, seed=31)
    x = (x.float() * xscale).to(torch.bfloat16)
    w = _pow2_weights(N, K, exps, seed=len(exps))
    _, _, hdr = eng.wcode_test(w)
    hs = sorted({e >> 1 for e in exps})
    assert list(hdr) == [max(hs[-1] - 15, 0)] * 2, name            # not raw, the expected base
    assert list(eng.wcode_dense_test(w)) == [1, 1], name
    for epi, norm in ((0, False), (3, False)):
        raw, cod = _both(eng, x, w, nw, r, epi, norm)
        assert torch.equal(_bits(raw), _bits(cod)), name
