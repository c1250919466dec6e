"""The dense word of the coded bf16 weight format (radialog_amd/wcode.py dense()): 1 iff a tile is not flagged raw and none of its weights has index 0
(h = 0). On such a tile the kernels decode the high byte as (index + base) | sign << 7, with no zero test (csrc/rdx_common.h wc_hi4 DENSE): the NumPy
restatement of that formula is held to wcode.decode here, and the share of dense tiles on the synthetic weights to the 95 % the cheap path rests on.
No GPU."""
import numpy as np
import pytest
import torch

from radialog_amd import synth, wcode

K = 256          # two coded chunks


def bf16(sign, exp, man):
    return np.uint16((sign << 15) | (exp << 7) | man)


def tile(fill):
    return np.full((16, K), fill, dtype=np.uint16)


def dense_of(w_bits):
    packed = wcode.pack_bf16(w_bits)
    d = wcode.dense(packed)
    assert d.dtype == np.uint32 and d.shape == (packed.shape[0],)
    _, hdr = wcode.encode(packed)
    assert not (d & (hdr >> 8)).any()          # never dense and raw
    return d


def normal_tile(seed=0):
    """Normal weights inside one window: h in 50..64, both signs, any low byte."""
    rng = np.random.default_rng(seed)
    w = rng.integers(0, 65536, (16, K), dtype=np.uint16)
    e = rng.integers(2 * 50, 2 * 65, (16, K)).astype(np.uint16)
    return ((w & 0x807F) | (e << 7)).astype(np.uint16)


def test_a_tile_of_normal_weights_inside_the_window_is_dense():
    assert list(dense_of(normal_tile())) == [1]
    assert list(dense_of(tile(bf16(1, 125, 17)))) == [1]


@pytest.mark.parametrize("name,bits", [("+0", 0x0000), ("-0", 0x8000), ("smallest subnormal", int(bf16(0, 0, 1))), ("largest subnormal", int(bf16(1, 0, 127))),
                                       ("first normal binade", int(bf16(0, 1, 64)))])
def test_one_weight_of_index_zero_makes_the_tile_general(name, bits):
    w = normal_tile(1)
    w[7, 131] = bits
    packed = wcode.pack_bf16(w)
    _, hdr = wcode.encode(packed)
    assert hdr[0] >> 8 == 0, name                  # still coded
    assert list(wcode.dense(packed)) == [0], name


@pytest.mark.parametrize("name,bits", [("out of window", int(bf16(0, 2 * 30, 3))), ("inf", 0x7F80), ("-inf", 0xFF80), ("nan", 0x7FC1)])
def test_a_raw_flagged_tile_is_not_dense(name, bits):
    w = normal_tile(2)
    w[3, 200] = bits
    packed = wcode.pack_bf16(w)
    _, hdr = wcode.encode(packed)
    assert hdr[0] >> 8 == 1, name
    assert list(wcode.dense(packed)) == [0], name


def test_the_all_zero_tile_and_the_padded_last_tile_are_not_dense():
    assert list(dense_of(tile(0))) == [0]
    w = np.full((20, K), bf16(1, 118, 1), dtype=np.uint16)      # 20 rows: rows 4..15 of tile 1 are padding zeros
    assert list(dense_of(w)) == [1, 0]


def dense_formula(planes, hdr):
    """wcode.decode with the high byte restated as the dense kernels compute it: ((idx + base) | sign << 7), no zero case."""
    nt, kq, _ = planes.shape
    base = (hdr & 0xFF).astype(np.uint32)[:, None, None, None, None]
    lo0 = planes[:, :, 0:1024].reshape(nt, kq, 64, 2, 8)
    lo1 = planes[:, :, 1024:2048].reshape(nt, kq, 64, 2, 8)
    lo = np.concatenate([lo0, lo1], axis=3).astype(np.uint32)
    ixw = np.ascontiguousarray(planes[:, :, 2048:3072]).view("<u4").reshape(nt, kq, 64, 4, 1).astype(np.uint32)
    sgw = np.ascontiguousarray(planes[:, :, 3072:3328]).view("<u4").reshape(nt, kq, 64, 1, 1).astype(np.uint32)
    e = np.arange(8)
    nib = np.where(e < 4, 2 * e, 2 * (e - 4) + 1).astype(np.uint32)
    idx = (ixw >> (4 * nib)) & 0xF
    j = np.arange(4)[:, None]
    bit = ((2 * j + e // 4) + 8 * (e % 4)).astype(np.uint32)
    sign = (sgw >> bit) & 1
    hi = (idx + base) | (sign << 7)
    assert (hi < 256).all()
    w = (hi << 8) | lo
    return np.ascontiguousarray(w.transpose(0, 1, 3, 2, 4)).reshape(nt, kq * 4, 64, 8).astype(np.uint16)


@pytest.mark.parametrize("top", [15, 64, 126])          # base = 0, 49, 111
def test_the_dense_formula_equals_decode_on_every_dense_tile(top):
    """Random windowed inputs: h in top - 14 .. top (index 1 .. 15), both signs, any low byte; 0x00 and 0xff low bytes and both window edges planted in
    every tile. A few tiles get a zero: they are not dense and are left to the general decode."""
    rng = np.random.default_rng(top)
    nt = 12
    w = rng.integers(0, 65536, (16 * nt, K), dtype=np.uint16)
    h = rng.integers(top - 14, top + 1, (16 * nt, K)).astype(np.uint16)
    w = ((w & 0x80FF) | (h << 8)).astype(np.uint16)
    for t in range(nt):
        r = 16 * t
        w[r, 0] = (0 << 15) | ((top - 14) << 8) | 0x00          # index 1
        w[r + 1, 1] = (1 << 15) | ((top - 14) << 8) | 0xFF
        w[r + 2, 2] = (0 << 15) | (top << 8) | 0xFF             # index 15
        w[r + 3, 3] = (1 << 15) | (top << 8) | 0x00
    w[16 * 4 + 9, 77] = 0x8000
    w[16 * 9 + 1, 140] = 0x0000
    packed = wcode.pack_bf16(w)
    planes, hdr = wcode.encode(packed)
    d = wcode.dense(packed)
    assert not (hdr >> 8).any() and (hdr & 0xFF == max(top - wcode.WINDOW, 0)).all()
    assert list(d) == [0 if t in (4, 9) else 1 for t in range(nt)]
    want = wcode.decode(planes, hdr)
    got = dense_formula(planes, hdr)
    sel = d == 1
    assert (got[sel] == want[sel]).all() and (want[sel] == packed[sel]).all()
    if top > wcode.WINDOW:                                      # base > 0: the general tiles need the zero test (with base 0 index 0 decodes to 0 anyway)
        assert not (got[~sel] == want[~sel]).all()


@pytest.mark.parametrize("name,shape", [("model.layers.3.self_attn.q_proj.weight", (4096, 4096)), ("model.layers.3.mlp.down_proj.weight", (4096, 11008)),
                                        ("model.layers.3.mlp.gate_proj.weight", (11008, 4096))])
def test_the_synthetic_weights_are_dense_on_at_least_95_percent_of_their_tiles(name, shape):
    """A condition, not a measurement: a build that marks nothing dense must not pass (counted: 255 / 256, 249 / 256, 686 / 688)."""
    w = synth._sym(name, shape, 0.02, "cpu")
    bits = w.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    d = wcode.dense(wcode.pack_bf16(bits))
    print(f"{name}: {int(d.sum())} of {d.size} tiles dense")
    assert d.sum() >= 0.95 * d.size
