"""The int4 group-quantised weight format (radialog_amd/w4.py) on the host: hand-computed groups that pin every rounding of the definition, the
stream layout's round trip, the quantisation error bound, and where the Python layers put the new weight kind. No GPU."""
import numpy as np
import pytest
import torch

from radialog_amd import _lib, w4, weights
from radialog_amd.config import LlamaCfg, RaDialogCfg, small_cfg


def _group(**at):
    """One row of one group: zeros, with w[k] = v for k=v pairs given as k<index>=value."""
    w = np.zeros((1, 128), dtype=np.float32)
    for k, v in at.items():
        w[0, int(k[1:])] = v
    return w


def _bits(x):
    return w4.bf16_bits(np.asarray(x, dtype=np.float32))


def test_all_zero_group():
    q, s = w4.quantize(_group())
    assert s[0, 0] == 0 and not q.any()
    assert (_bits(w4.dequantize(q, s)) == 0).all()          # +0, every one


def test_single_value_and_a_scale_that_rounds_down():
    # a = 3: fp32(3 / 7) = 0x3EDB6DB7 -> bf16 0x3EDB = 0.427734375 (the low half 0x6DB7 is under 0x8000: down)
    # q = rint(3 / 0.427734375 = 7.0137) = 7; 7 * 0.427734375 = 2.994140625 = 1.4970703125 * 2, 0.4970703125 * 128 = 63.625 -> 64: W' = 3.0
    q, s = w4.quantize(_group(k5=3.0))
    assert s[0, 0] == 0x3EDB
    assert q[0, 5] == 7 and np.count_nonzero(q) == 1
    wp = w4.dequantize(q, s)
    assert _bits(wp)[0, 5] == 0x4040 and np.count_nonzero(wp) == 1


def test_scale_rounds_up_to_nearest():
    # a = 5: fp32(5 / 7) = 0x3F36DB6E -> the low half 0xDB6E is over 0x8000: bf16 0x3F37 = 0.71484375 (truncation would give 0x3F36)
    # q = rint(5 / 0.71484375 = 6.9945) = 7; 7 * 0.71484375 = 5.00390625 = 1.2509765625 * 4, 0.2509765625 * 128 = 32.125 -> 32: W' = 5.0
    q, s = w4.quantize(_group(k0=5.0))
    assert s[0, 0] == 0x3F37 and q[0, 0] == 7
    assert _bits(w4.dequantize(q, s))[0, 0] == 0x40A0


def test_negative_absmax_is_minus_seven():
    q, s = w4.quantize(_group(k9=-7.0, k10=3.0))
    assert s[0, 0] == 0x3F80                                 # 7 / 7 = 1.0
    assert q[0, 9] == -7 and q[0, 10] == 3
    wp = w4.dequantize(q, s)
    assert wp[0, 9] == -7.0 and wp[0, 10] == 3.0
    assert q.min() == -7                                     # -8 is representable in the nibble, a symmetric scale never produces it


def test_half_way_cases_round_to_even():
    # s = 1.0: w / s is w itself
    q, s = w4.quantize(_group(k0=7.0, k1=2.5, k2=3.5, k3=-0.5, k4=0.5, k5=1.5, k6=-2.5, k7=-6.5))
    assert s[0, 0] == 0x3F80
    assert list(q[0, :8]) == [7, 2, 4, 0, 0, 2, -2, -6]
    assert _bits(w4.dequantize(q, s))[0, 3] == 0x0000       # rint(-0.5) = -0 is q = 0, which dequantises to +0


def test_scale_underflows_to_zero():
    # a = 1e-40 (an fp32 subnormal): a / 7 = 1.4e-41 is under half of the smallest bf16 subnormal (2^-133 = 9.2e-41): s = 0, every q = 0
    w = np.full((1, 128), 1e-40, dtype=np.float32)
    q, s = w4.quantize(w)
    assert s[0, 0] == 0 and not q.any() and not w4.dequantize(q, s).any()


def test_non_finite_weight_is_refused():
    for bad in (np.inf, -np.inf, np.nan):
        with pytest.raises(ValueError):
            w4.quantize(_group(k3=bad))


@pytest.mark.parametrize("n", [16, 40])
@pytest.mark.parametrize("k", [128, 384, 11008])
def test_pack_unpack_round_trip(n, k):
    rng = np.random.default_rng(n * 100003 + k)
    q = rng.integers(-8, 8, size=(n, k), dtype=np.int8)
    s = rng.integers(0, 0x7F80, size=(n, k // 128), dtype=np.uint16)
    stream = w4.pack(q, s)
    assert stream.shape == ((n + 15) // 16, k // 128, w4.CHUNK_BYTES) and stream.dtype == np.uint8
    q2, s2 = w4.unpack(stream, n)
    assert (q2 == q).all() and (s2 == s).all()
    if n % 16:          # the padded rows: nibbles 8 (q = 0), scales 0
        qa, sa = w4.unpack(stream, (n + 15) // 16 * 16)
        assert not qa[n:].any() and not sa[n:].any()


def test_stream_positions_of_one_weight():
    """Row 16 + 3, k = 128 + 32 * 2 + 8 * 1 + 5: tile 1, chunk 1, fragment j = 2, g = 1, e = 5 -> lane 19, dword 2, nibble 2 * (5 - 4) + 1 = 3."""
    q = np.zeros((32, 256), dtype=np.int8)
    s = np.zeros((32, 2), dtype=np.uint16)
    q[19, 128 + 64 + 8 + 5] = -3
    s[19, 1] = 0x3C12
    stream = w4.pack(q, s)
    dw = stream[1, 1, :1024].view("<u4").reshape(64, 4)
    assert dw[19, 2] == (0x88888888 & ~(0xF << 12)) | ((-3 + 8) << 12)
    dw[19, 2] = 0x88888888
    assert (dw == 0x88888888).all()
    sc = stream[1, 1, 1024:].view("<u2")
    assert sc[3] == 0x3C12 and np.count_nonzero(sc) == 1


def test_error_bound_on_random_weights():
    """|W' - W| <= s / 2 + 0.03 s + 2^-8 |q s|: with t = w / s exact, |q - t| <= 1 / 2 inside the clamp; the scale is a / 7 rounded to bf16 (relative
    error <= 2^-8, the fp32 division's 2^-24 beside it), so |t| <= 7 (1 + 2^-8) / (1 - 2^-24...) < 7 + 0.03 and the clamp at 7 adds at most 0.03 s; the
    fp32 division w / s is off by <= 2^-24 |t|, which can move a rint only across a half-way point it is that close to (absorbed in the 0.03 s, of which
    the overshoot uses 7 * 2^-8 = 0.0274); the product q s is exact in fp32 and rounds to bf16 with relative error <= 2^-8."""
    rng = np.random.default_rng(12)
    for w in (rng.standard_normal((40, 1024)).astype(np.float32) * 0.02, rng.uniform(-0.05, 0.05, (24, 512)).astype(np.float32),
              (rng.standard_normal((16, 256)) * np.exp(rng.uniform(-20, 20, (16, 256)))).astype(np.float32)):
        q, s = w4.quantize(w)
        wp = w4.dequantize(q, s)
        sf = np.repeat(w4.bf16_float(s).astype(np.float64), 128, axis=1)
        bound = sf / 2 + 0.03 * sf + 2.0 ** -8 * np.abs(q.astype(np.float64) * sf)
        assert (np.abs(wp.astype(np.float64) - w.astype(np.float64)) <= bound).all()
        assert np.abs(q).max() == 7 and q.min() >= -7


def test_packed_wprime_keeps_rows_past_n_quant_raw():
    rng = np.random.default_rng(3)
    w = rng.standard_normal((48, 128)).astype(np.float32)
    from radialog_amd import wcode
    p = w4.packed_wprime(w, n_quant=32)
    assert (p[2] == wcode.pack_bf16(w4.bf16_bits(w))[2]).all()
    assert (p[:2] == wcode.pack_bf16(w4.bf16_bits(w4.dequantize(w4.quantize(w[:32]))))).all()


def _items(w4_on, fp8=False):
    c = LlamaCfg(vocab=64, hidden=128, inter=256, layers=2, heads=1, qformer_dim=32, max_pos=16)

    def get(name):
        shapes = {"embed_tokens": (c.vocab, c.hidden), "lm_head": (c.vocab, c.hidden), "norm": (c.hidden,), "layernorm": (c.hidden,),
                  "img_proj_layer.weight": (c.hidden, c.qformer_dim), "img_proj_layer.bias": (c.hidden,),
                  "lora_A": (c.lora_r, c.hidden), "lora_B": (c.hidden, c.lora_r), "gate_proj": (c.inter, c.hidden), "up_proj": (c.inter, c.hidden),
                  "down_proj": (c.hidden, c.inter), "_proj.weight": (c.hidden, c.hidden)}
        for key, shp in shapes.items():
            if key in name:
                return torch.zeros(shp)
        raise KeyError(name)
    return {name: kind for name, _, kind in weights.llama_items(get, c, lora=True, fp8=fp8, w4=w4_on)}, c


def test_llama_items_puts_the_kind_on_the_seven_projections():
    kinds, c = _items(True)
    plain, _ = _items(False)
    want = {f"l{l}.{n}" for l in range(c.layers) for n in ("wqkv", "wo", "wgu", "wdown")}       # q / k / v fused, gate / up fused: seven projections
    assert {n for n, k in kinds.items() if k == _lib.RDX_W_GEMM_W4} == want
    assert _lib.RDX_W_GEMM_W4 == 4 and _lib.RDX_W_GEMM_W4 not in plain.values()
    for n, k in kinds.items():
        if n not in want:
            assert k == plain[n], n                                # lm_head, embeddings, norms, LoRA-B, img_proj: as without it
    assert kinds["lm_head"] == _lib.RDX_W_GEMM
    with pytest.raises(ValueError):
        _items(True, fp8=True)


def test_engine_refuses_w4_with_fp8_and_with_f16():
    from radialog_amd.engine import RdxEngine
    with pytest.raises(ValueError, match="weights_fp8"):
        RdxEngine(small_cfg(), dtype="bf16", weights_w4=True, weights_fp8=True)
    with pytest.raises(ValueError, match="f16"):
        RdxEngine(small_cfg(), dtype="f16", weights_w4=True)
    assert isinstance(small_cfg(), RaDialogCfg)
