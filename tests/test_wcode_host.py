"""The coded bf16 weight format (radialog_amd/wcode.py: 13 bits per weight, the definition the device encoder and the kernels' decode are held to)
round-trips bit for bit on tiles built to break it, flags exactly the tiles it cannot express, and expresses every tile of the engine's synthetic
weights. No GPU."""
import numpy as np
import pytest
import torch

from radialog_amd import synth, wcode

K = 256          # two coded chunks


def bf16(sign, exp, man):
    return np.uint16((sign << 15) | (exp << 7) | man)


def tile(fill):
    """One 16-row tile [16][K] of uint16 bit patterns."""
    return np.full((16, K), fill, dtype=np.uint16)


def roundtrip(w_bits):
    packed = wcode.pack_bf16(w_bits)
    planes, hdr = wcode.encode(packed)
    assert planes.dtype == np.uint8 and planes.shape == (packed.shape[0], packed.shape[1] // 4, wcode.CHUNK_BYTES)
    assert planes.shape[2] * 8 == 13 * 64 * 32              # 13 bits for each of a chunk's 64 x 32 weights
    return packed, planes, hdr, wcode.decode(planes, hdr)


def test_pack_is_the_fragment_order():
    w = np.arange(32 * 64, dtype=np.uint16).reshape(32, 64)
    p = wcode.pack_bf16(w)
    for (t, c, g, r) in ((0, 0, 0, 0), (1, 1, 3, 15), (0, 1, 2, 7)):
        assert (p[t, c, 16 * g + r] == w[16 * t + r, 32 * c + 8 * g: 32 * c + 8 * g + 8]).all()


def test_all_equal_exponents():
    rng = np.random.default_rng(1)
    w = (bf16(0, 120, 0) | rng.integers(0, 128, (16, K)).astype(np.uint16) | (rng.integers(0, 2, (16, K)).astype(np.uint16) << 15)).astype(np.uint16)
    packed, _, hdr, back = roundtrip(w)
    assert hdr[0] >> 8 == 0 and (back == packed).all()


def test_span_of_exactly_the_window_and_one_more():
    """h = e >> 1: the window holds top - 14 .. top. A weight 14 h-steps under the top fits, one 15 under does not."""
    w = tile(bf16(0, 2 * 60, 5))
    w[3, 7] = bf16(1, 2 * 46 + 1, 99)          # h = 46 = 60 - 14
    packed, _, hdr, back = roundtrip(w)
    assert hdr[0] == (60 - wcode.WINDOW) and (back == packed).all()
    w[9, 200] = bf16(0, 2 * 45 + 1, 3)         # h = 45 = 60 - 15: outside
    packed, _, hdr, back = roundtrip(w)
    assert hdr[0] >> 8 == 1
    # a second, clean tile next to it stays coded
    w2 = np.concatenate([w, tile(bf16(0, 2 * 60, 5))])
    packed, _, hdr, back = roundtrip(w2)
    assert list(hdr >> 8) == [1, 0] and (back[1] == packed[1]).all()


def test_zeros_of_both_signs_and_subnormals_are_not_exceptions():
    w = tile(bf16(0, 125, 17))
    w[0, 0] = 0x0000
    w[1, 1] = 0x8000                  # -0
    w[2, 2] = bf16(0, 0, 1)           # smallest subnormal
    w[3, 3] = bf16(1, 0, 127)         # largest subnormal, negative
    w[4, 4] = bf16(0, 1, 64)          # first normal binade: h = 0 as well
    packed, _, hdr, back = roundtrip(w)
    assert hdr[0] >> 8 == 0 and (back == packed).all()
    assert back.view(np.uint16).reshape(-1).tolist().count(0x8000) == 1


def test_inf_and_nan_fall_back():
    for bits in (0x7F80, 0xFF80, 0x7FC1):
        w = tile(bf16(0, 125, 17))
        w[5, 130] = bits
        _, _, hdr, _ = roundtrip(w)
        assert hdr[0] >> 8 == 1, hex(bits)
    w = tile(0x7F80)                  # nothing but Inf: still flagged
    assert roundtrip(w)[2][0] >> 8 == 1


def test_a_tile_of_zeros():
    """The padding rows of the last tile, and a whole tile of them."""
    packed, planes, hdr, back = roundtrip(tile(0))
    assert hdr[0] == 0 and not planes.any() and (back == packed).all()
    w = np.full((20, K), bf16(1, 118, 1), dtype=np.uint16)      # 20 rows: rows 4..15 of tile 1 are padding
    packed, _, hdr, back = roundtrip(w)
    assert list(hdr >> 8) == [0, 0] and (back == packed).all()


def test_small_top_exponent_keeps_base_at_zero():
    w = tile(bf16(0, 2 * 9, 1))
    w[0, 0] = bf16(0, 2 * 1, 1)
    packed, _, hdr, back = roundtrip(w)
    assert hdr[0] == 0 and (back == packed).all()


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_random_bit_patterns(seed):
    """Random 16-bit patterns span every exponent: almost every tile falls back, and what does not, decodes exactly; narrowed to a window they all do."""
    rng = np.random.default_rng(seed)
    w = rng.integers(0, 65536, (64, K), dtype=np.uint16)
    packed, _, hdr, back = roundtrip(w)
    ok = (hdr >> 8) == 0
    assert (back[ok] == packed[ok]).all()
    e = rng.integers(2 * 50, 2 * 65, (64, K)).astype(np.uint16)           # h in 50..64: 15 values
    zero = rng.random((64, K)) < 0.01
    w = ((w & 0x807F) | (e << 7)).astype(np.uint16)
    w[zero] &= 0x80FF                                                       # h = 0 with any sign, any low byte
    packed, _, hdr, back = roundtrip(w)
    assert not (hdr >> 8).any() and (back == packed).all()


@pytest.mark.parametrize("shape", [(64, 4096), (64, 11008)])
def test_no_tile_of_the_synthetic_weights_falls_back(shape):
    w = synth._sym(f"wcode.host.{shape[1]}", shape, 0.02, "cpu")          # the generator and the width of the Llama projections (synth.llama_specs)
    bits = w.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    packed, _, hdr, back = roundtrip(bits)
    assert wcode.fallback_tiles(hdr) == 0
    assert (back == packed).all()
