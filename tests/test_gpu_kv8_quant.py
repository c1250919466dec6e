"""kv8_quant_rows_k (csrc/attn.hip: the prompt's staged K / V rows into the fp8 KV cache) alone, through rdx_kv8_quant_test, against radialog_amd/kv8.py
byte for byte: codes (K through the storage order, kv8.k_logical) and exponents of positions [slot0, slot0 + T), every other byte of the four buffers as
it was, 0xff guards behind each. B 3, heads 2, T 1 / 17 / 160, max_len 192. The rows hold magnitudes from 2^-20 to 2^8, a zero row, the format's boundary
rows (amax 448 2^k and just above, 0.875, values that quantise to subnormal codes under the clamped exponent) and -0 elements."""
import pytest
import torch

import _dec_attn as A
from radialog_amd import kv8

pytestmark = pytest.mark.gpu

B, HEADS, MAX_LEN, GUARD = 3, 2, 192, 4096


@pytest.fixture(scope="module", params=["f16", "bf16"])
def eng(request):
    from radialog_amd.config import small_cfg
    from radialog_amd.engine import RdxEngine
    e = RdxEngine(small_cfg(), dtype=request.param, device=0, max_batch=1, max_len=32, llama=False, vision=False)
    e.dt = A.DT[request.param]
    yield e
    e.close()


def _rows(dt, n, seed):
    """n rows of 128 in dt: random magnitudes 2^-20 .. 2^8 with the special rows first."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, 128, generator=g) * torch.exp2(torch.randint(-20, 9, (n, 1), generator=g).float())
    x[torch.rand(n, 128, generator=g) < 0.05] = -0.0
    special = []
    for amax in (448.0, 449.0, 0.875, 0.876, 448.0 * 2 ** -15, 456.0 * 2 ** -15, 2.0 ** -20, 3 * 2.0 ** -24, 1.0, 240.0, 225.0, 256.0):
        r = torch.zeros(128)
        r[5], r[77], r[6], r[7] = amax, -amax / 3, amax * 2.0 ** -9, -0.0
        special.append(r)
    special.append(torch.zeros(128))
    k = min(n, len(special))
    order = torch.randperm(len(special), generator=g)[:k]
    x[:k] = torch.stack(special)[order]
    return x.to(dt)


@pytest.mark.parametrize("T", [1, 17, 160])
def test_staged_rows_become_kv8_quant_bytes(eng, T):
    dt = eng.dt
    stage = (T + 15) // 16 * 16
    g = torch.Generator().manual_seed(T)
    krows = torch.full((B, HEADS, stage, 128), 7.0, dtype=dt)                  # rows t >= T of the staging buffer: values the kernel must not read into the cache
    vrows = torch.full((B, HEADS, stage, 128), -9.0, dtype=dt)
    krows[:, :, :T] = _rows(dt, B * HEADS * T, 10 + T).reshape(B, HEADS, T, 128)
    vrows[:, :, :T] = _rows(dt, B * HEADS * T, 20 + T).reshape(B, HEADS, T, 128)
    kc0, vc0 = (torch.randint(0, 0x7f, (B, HEADS, MAX_LEN, 128), generator=g, dtype=torch.uint8) for _ in range(2))
    ke0, ve0 = (torch.randint(-15, 16, (B, HEADS, MAX_LEN), generator=g, dtype=torch.int8) for _ in range(2))
    err, kc, ke, vc, ve = eng.kv8_quant_test(krows, vrows, T, MAX_LEN, 0, kv8.k_store(kc0), ke0, vc0, ve0, guard=GUARD)
    assert err is None, err
    nc, ne = kc0.numel(), ke0.numel()
    for name, buf, size in (("K codes", kc, nc), ("K exponents", ke, ne), ("V codes", vc, nc), ("V exponents", ve, ne)):
        assert bool((buf.cpu()[size:] == 0xff).all()), f"guard bytes behind the {name} were written"
    kc = kv8.k_logical(kc.cpu()[:nc].reshape(kc0.shape))
    vc = vc.cpu()[:nc].reshape(vc0.shape)
    ke, ve = ke.cpu()[:ne].view(torch.int8).reshape(ke0.shape), ve.cpu()[:ne].view(torch.int8).reshape(ve0.shape)
    for name, rows, codes, exps, c0, e0 in (("K", krows, kc, ke, kc0, ke0), ("V", vrows, vc, ve, vc0, ve0)):
        wc, we = kv8.quant(rows[:, :, :T])
        assert torch.equal(exps[:, :, :T], we), f"{name}: {int((exps[:, :, :T] != we).sum())} exponents differ from kv8.quant"
        assert torch.equal(codes[:, :, :T], wc), f"{name}: {int((codes[:, :, :T] != wc).sum())} codes differ from kv8.quant"
        assert torch.equal(codes[:, :, T:], c0[:, :, T:]) and torch.equal(exps[:, :, T:], e0[:, :, T:]), f"{name}: positions >= T were written"
    assert len(set(kv8.quant(krows[:, :, :T])[1].reshape(-1).tolist())) >= min(3, T)


def test_refusals(eng):
    dt = eng.dt
    rows = torch.zeros(1, HEADS, 16, 128, dtype=dt)
    codes, exps = torch.zeros(1, HEADS, 32, 128, dtype=torch.uint8), torch.zeros(1, HEADS, 32, dtype=torch.int8)
    assert eng.kv8_quant_test(rows, rows, 16, 32, 16, codes, exps, codes, exps)[0] is None
    for what, T, slot0 in (("more rows than staged", 17, 0), ("slots past max_len", 16, 17), ("negative slot", 4, -1)):
        err, kc, ke, vc, ve = eng.kv8_quant_test(rows, rows, T, 32, slot0, codes, exps, codes, exps)
        assert err is not None and "rdx_kv8_quant_test" in err, f"{what}: not refused"
        assert not bool(kc.cpu().any()) and not bool(ke.cpu().any()) and not bool(vc.cpu().any()) and not bool(ve.cpu().any()), f"{what}: a refused launch wrote"
