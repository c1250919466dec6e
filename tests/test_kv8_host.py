"""The fp8 KV cache format (radialog_amd/kv8.py) on the CPU: hand-computed rows, what the format promises (every stored value is a bf16 and an f16 value, the
quantiser is idempotent, the relative error bound), the inputs of the kernel tests (tests/_kv8.py: the K rows round-trip exactly and the exponents change
with position, head and row), and the argument checks that need no GPU."""
import pytest
import torch

import _dec_attn as A
import _kv8 as K8
from radialog_amd import kv8
from radialog_amd.config import small_cfg


def _row(**at):
    x = torch.zeros(128)
    for k, v in at.items():
        x[int(k[1:])] = v
    return x


def test_hand_computed_rows():
    """448 -> e 0, code 448 (0x7e); 449 -> e 1, code 224 (0x76); 0.875 -> e -9, code 448; a zero row -> e -15; 1e-30 -> e -15 and zero codes; -0 keeps its sign."""
    x = torch.stack([_row(i3=448.0, i4=-3.0), _row(i3=-449.0), _row(i3=0.875), _row(), _row(i5=1e-30), _row(i0=-0.0, i1=1.0)])
    c, e = kv8.quant(x)
    assert e.tolist() == [0, 1, -9, -15, -15, -8] and e.dtype == torch.int8 and c.dtype == torch.uint8
    assert c[0, 3] == 0x7e and c[0, 4] == 0xc4 and c[1, 3] == 0xf6 and c[2, 3] == 0x7e          # 448; -3 = -1.5 x 2; -224; 448
    assert not bool(c[3].any()) and not bool(c[4].any())
    assert c[5, 0] == 0x80 and c[5, 1] == 0x78                                                  # -0; 1 x 2^8 = 256
    d = kv8.dequant(c, e)
    assert d[0, 3] == 448 and d[0, 4] == -3 and d[1, 3] == -448 and d[2, 3] == 0.875 and d[5, 1] == 1 and not bool(d[3].any()) and not bool(d[4].any())
    assert torch.signbit(d[5, 0])


def test_exponent_rule_at_both_ends_of_every_binade():
    """e is the SMALLEST integer with amax 2^-e <= 448, clamped at -15: just above 448 2^k the exponent steps up."""
    for k in range(-14, 20):
        for amax, want in ((448.0 * 2.0 ** k, k), (448.0 * 2.0 ** k * (1 + 2.0 ** -7), k + 1), (256.0 * 2.0 ** k, k), (225.0 * 2.0 ** k, k)):
            assert int(kv8.exponent(_row(i9=amax))) == max(want, kv8.EMIN), (k, amax)
    assert int(kv8.exponent(_row(i9=2.0 ** -24))) == kv8.EMIN


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_stored_values_are_model_dtype_values_and_the_quantiser_is_idempotent(dt):
    """Magnitudes over the whole useful range of both dtypes (down to rows that quantise to subnormal codes under the clamped exponent): dequant asserts that x'
    is exactly a value of the dtype. quant(x') gives x' again, bit for bit, and the same BYTES unless the row's largest code is 224 and e is not the clamp:
    then e - 1 and doubled codes (kv8.py's docstring) -- both directions are held, so the exception is exactly that one."""
    g = torch.Generator().manual_seed(3)
    x = (torch.randn(4000, 128, generator=g) * torch.logspace(-7, 4, 4000)[:, None]).to(dt)
    c, e = kv8.quant(x)
    xp = kv8.dequant(c, e, dtype=dt)
    assert torch.equal(kv8.dequant(c, e, dtype=torch.bfloat16).float(), kv8.dequant(c, e, dtype=torch.float16).float())
    c2, e2 = kv8.quant(xp)
    assert torch.equal(kv8.dequant(c2, e2, dtype=dt).view(torch.int16), xp.view(torch.int16))
    same = (c == c2).all(-1) & (e == e2)
    corner = ((c & 0x7f).amax(-1) == 0x76) & (e > kv8.EMIN)
    assert torch.equal(same, ~corner) and bool(corner.any()) and bool(same.any())
    assert torch.equal(e2[corner], e[corner] - 1)
    # half an ulp of a 3-bit mantissa: |x - x'| <= 2^-4 |x'| wherever the code is normal, and <= 2^-4 |x| wherever x 2^-e itself lies in the normal range
    # (an x just under the smallest normal code that rounds up to it misses the second form by a factor 1 / (1 - 2^-4): the first covers it)
    normal = (c & 0x78) != 0
    err, ref = (x.double() - xp.double()).abs(), x.double().abs()
    assert bool((err[normal] <= xp.double().abs()[normal] * 2.0 ** -4).all())
    in_range = torch.ldexp(ref, -e.to(torch.int32)[:, None]) >= 2.0 ** -6
    assert bool((err[in_range] <= ref[in_range] * 2.0 ** -4).all()) and bool(in_range.any()) and bool((~in_range).any())
    assert bool(((c & 0x7f) != 0x7f).all())                                                      # nothing saturates, no NaN code


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_stock_k_rows_round_trip_with_exponent_minus_8(dt):
    case = A.edge_case(dt, A.EDGES[1][1], 11, lora=True)
    c, e = kv8.quant(case.kc)
    assert torch.equal(kv8.dequant(c, e, dtype=dt).view(torch.int16), case.kc.view(torch.int16))
    amax1 = case.kc.float().abs().amax(-1) == 1
    assert bool(amax1.any()) and bool((e[amax1] == -8).all())
    s = A.sweep_case(dt, 300, 2, 5)
    assert torch.equal(kv8.roundtrip(s.kc).view(torch.int16), s.kc.view(torch.int16))


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_inputs_of_the_kernel_tests_hold_their_conditions(dt):
    """tests/_kv8.py: both caches hold stored values (stored() asserts the round trip), the exponents change with position, head and row, and the hot
    positions still carry their share."""
    for case in (K8.edge_case(dt, A.EDGES[0][1], 3, lora=False), K8.edge_case(dt, A.EDGES_ALL[0], 4, lora=True), K8.sweep_case(dt, 300, 7, 7101),
                 K8.packed_case(dt, 20, 920), K8.packed_case(dt, 40, 940), K8.packed_case(dt, 2, 5), K8.edge_case(dt, A.EDGES[2][1], 302, lora=True),
                 K8.edge_case(dt, A.EDGE_TOP, 107, lora=True)):
        kc, ke, vc, ve = K8.stored(case)
        K8.exponents_vary(case, ke, ve)
        assert len(set(ke.reshape(-1).tolist())) >= 3 and len(set(ve.reshape(-1).tolist())) >= 4
        A.assert_hot(case, case.ref())
    # the stock caches would not do: one exponent everywhere
    stock = A.edge_case(dt, A.EDGES[0][1], 3, lora=False)
    with pytest.raises(AssertionError):
        K8.exponents_vary(stock, *[kv8.quant(t)[1] for t in (stock.kc, stock.vc)])


def test_k_storage_order_is_a_permutation_with_contiguous_fragment_lanes():
    """kv8.k_store: inside a group of 16 positions, lane (g, r) of an MFMA A fragment owns 32 contiguous bytes -- the pieces dims 32 c + 8 g .. + 8 of position r."""
    L = 48
    idx = torch.arange(L * 128, dtype=torch.int32).reshape(1, L, 128)
    st = kv8.k_store(idx)
    assert torch.equal(kv8.k_logical(st), idx) and sorted(st.reshape(-1).tolist()) == list(range(L * 128))
    flat = st.reshape(-1)
    for pos, g in ((0, 0), (5, 2), (17, 3), (47, 1)):
        lane = flat[(pos // 16) * 2048 + (g * 16 + pos % 16) * 32:][:32]
        want = torch.cat([idx[0, pos, 32 * c + 8 * g:32 * c + 8 * g + 8] for c in range(4)])
        assert torch.equal(lane, want)


def test_cache_bytes():
    assert kv8.cache_bytes(32, 1, 32, 1536) == 2 * 32 * 32 * 1536 * 129             # 406 MB per row at max_len 1536, against 805 MB in two bytes
    assert kv8.cache_bytes(32, 1, 32, 1536) * 2 == 2 * 32 * 32 * 1536 * 128 * 2 + 2 * 2 * 32 * 32 * 1536


def test_argument_validation_without_a_gpu():
    from radialog_amd.engine import RdxEngine
    from radialog_amd.modeling_llama_imgemb import LlamaForCausalLM
    with pytest.raises(ValueError, match="kv_fp8"):
        RdxEngine(small_cfg(), dtype="bf16", llama=False, vision=False, kv_fp8=True)
    with pytest.raises(ValueError, match="kv_fp8"):
        RdxEngine(small_cfg(), dtype="bf16", classifier=True, kv_fp8=True)
    m = LlamaForCausalLM(cfg=small_cfg().llama, kv_fp8=True)
    ids = torch.zeros(1, 40, dtype=torch.int64)
    with pytest.raises(ValueError, match="kv_fp8"):
        m.generate(ids, num_beams=2, use_img=False)
    m.reuse_prefix_kv = True
    with pytest.raises(ValueError, match="kv_fp8"):
        m.generate(ids, use_img=False)
    with pytest.raises(ValueError, match="kv_fp8"):
        m.generate_many([ids[0]])
    with pytest.raises(AssertionError):
        kv8.quant(_row(i1=float("inf")))
