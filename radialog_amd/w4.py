"""int4 group-quantised weights ("W4", W4A16): the definition of the 4.125-bit format the decode step streams at 1-16 rows instead of the packed bf16 bytes (batch <= 2:
the GEMV and the chained launch; 3-16 rows: xstat16_w4_k / xrow16_w4_k for QKV, gate/up and down_proj), as a
NumPy quantiser, dequantiser, packer and unpacker. The device quantiser (csrc/gemm.hip quant_w4_k) and the in-register decode (csrc/rdx_common.h
w4_frag) are compared with this file byte for byte and bit for bit.

int4 is a STORAGE format of one weight stream, not an arithmetic: a quantised weight is defined by its dequantised bf16 value W'. Everything but the
1-16-row decode steps (o_proj and the lm_head there too, every kernel from 17 rows, the prefill, score()) multiplies a packed bf16 copy of W'; those
steps decode the nibbles to exactly W' in registers.

For W [N][K] fp32, K % 128 == 0, groups of GROUP = 128 consecutive k of one row (every op below is a NumPy float32 op: IEEE, round to nearest even):
    a  = max |w| over the group
    s  = bf16(a / 7)                      one fp32 division, one rounding to bf16; a == 0 or s == 0  ->  s = 0 and every q = 0
    q  = clamp(rint(w / float(s)), -8, 7) an fp32 DIVISION (not a reciprocal multiply), rint = half to even
    W' = bf16(float(q) * float(s))        the product is exact in fp32: one rounding
Stored per group: 128 nibbles q + 8 and the 16 bits of s.

Stream layout. The packed bf16 weight is [tiles][K / 32][64 lanes][8] (lane = 16 g + r holds W[16 tile + r][32 c + 8 g .. + 8], wcode.pack_bf16). One
W4 chunk is one 16-row tile x 128 k = four packed chunks c = 4 qc + j, CHUNK_BYTES bytes:

    [0, 1024)     nibbles: lane * 16 + 4 j .. + 4    one little-endian dword per MFMA A fragment j = 0..3 of the lane; weight e = 0..7 of the
                                                     fragment (k = 128 qc + 32 j + 8 g + e) is nibble 2 e (e < 4) or 2 (e - 4) + 1 (e >= 4)
    [1024, 1056)  scales:  2 r .. + 2                the bf16 bits of s for row 16 tile + r, little-endian

so a wave reads the nibbles of a chunk with one contiguous 1 KiB load (16 bytes per lane: exactly the four fragments the lane would have loaded from
the packed buffer) and lane (g, r) its row's scale with a 2-byte load behind them. Chunks are laid [tiles][K / 128]. Rows past N (a padded tile) are
zero: s = 0, nibbles 8. One header word per tile: bit 8 = the tile is RAW (not quantised: W' = bf16(W); the kernels stream its packed bf16 bytes; its
chunk bytes are nibbles 8 / scales 0). The fused QKV weight's LoRA-A tiles are the raw ones.
"""
import numpy as np

GROUP = 128
CHUNK_K = 128
CHUNK_BYTES = 64 * 16 + 16 * 2
QMAX = 7.0


def bf16_bits(x: np.ndarray) -> np.ndarray:
    """float32 -> bf16 bit patterns (uint16), round to nearest even; finite inputs."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return ((b + np.uint32(0x7FFF) + ((b >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)


def bf16_float(bits: np.ndarray) -> np.ndarray:
    """bf16 bit patterns -> float32 (exact)."""
    return (np.ascontiguousarray(bits, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def quantize(w: np.ndarray):
    """w [N][K] float32 -> (q int8 [N][K] in -8..7, s uint16 [N][K / 128] bf16 bit patterns)."""
    w = np.ascontiguousarray(w, dtype=np.float32)
    n, k = w.shape
    assert k % GROUP == 0
    if not np.isfinite(w).all():
        raise ValueError("w4.quantize: non-finite weight")
    wg = w.reshape(n, k // GROUP, GROUP)
    a = np.abs(wg).max(axis=2)
    s = bf16_bits(a / np.float32(QMAX))
    sf = bf16_float(s)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        t = wg / sf[:, :, None]
    q = np.clip(np.rint(t), -8, 7)
    q = np.where(sf[:, :, None] == 0, 0, q).astype(np.int8)
    return q.reshape(n, k), s


def dequantize(q, s=None) -> np.ndarray:
    """(q, s) -> W' as float32 [N][K] (every value is a bf16 value). Takes the pair quantize() returns, or its two members."""
    if s is None:
        q, s = q
    n, k = q.shape
    sf = bf16_float(s)
    p = q.reshape(n, k // GROUP, GROUP).astype(np.float32) * sf[:, :, None]
    return bf16_float(bf16_bits(p)).reshape(n, k)


def _nibble_of(e):
    return np.where(e < 4, 2 * e, 2 * (e - 4) + 1)


def pack(q: np.ndarray, s: np.ndarray) -> np.ndarray:
    """(q int8 [N][K], s uint16 [N][K / 128]) -> stream uint8 [ceil(N / 16)][K / 128][CHUNK_BYTES]."""
    n, k = q.shape
    assert k % CHUNK_K == 0 and s.shape == (n, k // GROUP)
    nt, kq = (n + 15) // 16, k // CHUNK_K
    qf = np.zeros((nt * 16, k), dtype=np.uint32)
    qf[:n] = (q.astype(np.int32) + 8).astype(np.uint32)
    qf[n:] = 8
    sfull = np.zeros((nt * 16, kq), dtype=np.uint16)
    sfull[:n] = s
    # [tile][r][qc][j][g][e] -> [tile][qc][g][r][j][e]
    x = qf.reshape(nt, 16, kq, 4, 4, 8).transpose(0, 2, 4, 1, 3, 5)
    sh = (4 * _nibble_of(np.arange(8))).astype(np.uint32)
    dw = (x << sh).sum(axis=-1, dtype=np.uint64).astype("<u4")                  # [tile][qc][g][r][j]
    out = np.zeros((nt, kq, CHUNK_BYTES), dtype=np.uint8)
    out[:, :, :1024] = np.ascontiguousarray(dw).view(np.uint8).reshape(nt, kq, 1024)
    sc = np.ascontiguousarray(sfull.reshape(nt, 16, kq).transpose(0, 2, 1)).astype("<u2")     # [tile][qc][r]
    out[:, :, 1024:] = sc.view(np.uint8).reshape(nt, kq, 32)
    return out


def unpack(stream: np.ndarray, n: int):
    """stream [tiles][K / 128][CHUNK_BYTES] -> (q int8 [n][K], s uint16 [n][K / 128]): the first n rows."""
    nt, kq, nb = stream.shape
    assert nb == CHUNK_BYTES and n <= nt * 16
    dw = np.ascontiguousarray(stream[:, :, :1024]).view("<u4").reshape(nt, kq, 4, 16, 4, 1).astype(np.uint32)     # [tile][qc][g][r][j][1]
    sh = (4 * _nibble_of(np.arange(8))).astype(np.uint32)
    x = ((dw >> sh) & np.uint32(0xF)).astype(np.int32) - 8                                      # [tile][qc][g][r][j][e]
    q = np.ascontiguousarray(x.transpose(0, 3, 1, 4, 2, 5)).reshape(nt * 16, kq * CHUNK_K).astype(np.int8)
    sc = np.ascontiguousarray(stream[:, :, 1024:]).view("<u2").reshape(nt, kq, 16)
    s = np.ascontiguousarray(sc.transpose(0, 2, 1)).reshape(nt * 16, kq).astype(np.uint16)
    return q[:n], s[:n]


def packed_wprime(w: np.ndarray, n_quant=None) -> np.ndarray:
    """The packed bf16 buffer [tiles][K / 32][64][8] (uint16) the library keeps for w: W' for rows < n_quant (default: all), bf16(w) for the rest."""
    from .wcode import pack_bf16
    w = np.ascontiguousarray(w, dtype=np.float32)
    n_quant = w.shape[0] if n_quant is None else n_quant
    bits = bf16_bits(w)
    if n_quant:
        bits[:n_quant] = bf16_bits(dequantize(quantize(w[:n_quant])))
    return pack_bf16(bits)
