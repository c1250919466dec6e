"""Coded bf16 weights ("WC"): the definition of the 13-bit format the batch <= 2 GEMV streams instead of the packed bf16 bytes, as a NumPy
encoder and decoder. The device encoder (csrc/gemm.hip encode_wc_k) and the in-register decode (csrc/rdx_common.h wc_frag) are compared with this
file byte for byte and bit for bit.

A bf16 weight is s e7..e0 m6..m0. The low byte (e0 m6..m0) is stored verbatim; of the high byte the sign is kept and h = (e7..e1) is replaced by
a 4-bit index into a window of one 16-row tile:  index 0 <-> h = 0 (zero, subnormals and the first normal binade: the low byte tells them apart),
index i = 1..15 <-> h = base + i, with base = max(top - 15, 0) and top the tile's largest h below 127. That is 30 binades under the tile's largest
weight plus everything tiny, at 8 + 4 + 1 = 13 bits. A tile that holds a weight outside the window (0 < h <= base) or an Inf / NaN (h = 127) is
flagged raw: the kernels read its packed bf16 bytes instead. Its planes exist all the same, with index 0 for what does not fit.

Input of the encoder is the PACKED weight [tiles][K / 32][64 lanes][8] (uint16 bit patterns; lane = 16 g + r holds W[16 tile + r][32 c + 8 g .. + 8]):
what the GEMV streams, so that lane (g, r) decodes exactly the fragments it would have loaded. Per tile and per 128 k-values (four packed chunks
c = 4 q + j) the output is CHUNK_BYTES bytes in three planes of whole-wave contiguous loads:

    [0, 1024)     lo0:  lane * 16 + 8 j + e          low byte of weight e = 0..7 of fragment j = 0, 1
    [1024, 2048)  lo1:  the same for j = 2, 3
    [2048, 3072)  idx:  lane * 16 + 4 j .. + 4       one little-endian dword per fragment, nibble 2 e (e < 4) or 2 (e - 4) + 1 (e >= 4)
    [3072, 3328)  sign: lane * 4 .. + 4              one little-endian dword, bit (2 j + e // 4) + 8 (e % 4)

and one header word per tile: base | raw << 8, and one dense word per tile (dense() below): 1 iff the tile is not raw and holds no index 0.
"""
import numpy as np

CHUNK_K = 128
CHUNK_BYTES = 64 * 52
WINDOW = 15          # h values a non-zero index can name


def pack_bf16(w_bits: np.ndarray) -> np.ndarray:
    """[N][K] uint16 bit patterns -> the packed order [ceil(N / 16)][K / 32][64][8] of pack_weight_k (rows past N are zero)."""
    n, k = w_bits.shape
    assert k % 32 == 0
    nt = (n + 15) // 16
    full = np.zeros((nt * 16, k), dtype=np.uint16)
    full[:n] = w_bits
    # [tile][r][chunk][g][8] -> [tile][chunk][g][r][8]
    return np.ascontiguousarray(full.reshape(nt, 16, k // 32, 4, 8).transpose(0, 2, 3, 1, 4)).reshape(nt, k // 32, 64, 8)


def encode(packed: np.ndarray):
    """packed [tiles][K / 32][64][8] uint16 -> (planes uint8 [tiles][K / 128][CHUNK_BYTES], hdr uint32 [tiles])."""
    nt, kc, lanes, eight = packed.shape
    assert lanes == 64 and eight == 8 and kc % 4 == 0 and packed.dtype == np.uint16
    kq = kc // 4
    w = packed.astype(np.uint32)
    h = (w >> 8) & 0x7F
    lo = (w & 0xFF).astype(np.uint8)
    sign = w >> 15
    finite = h != 127
    top = np.where(finite, h, 0).reshape(nt, -1).max(axis=1)
    base = np.maximum(top.astype(np.int64) - WINDOW, 0)
    idx = h.astype(np.int64) - base[:, None, None, None]
    inside = (h == 0) | ((idx >= 1) & (idx <= WINDOW) & finite)
    raw = ~inside.reshape(nt, -1).all(axis=1)
    idx = np.where(inside & (h != 0), idx, 0).astype(np.uint32)

    # [tile][q][j][lane][e]
    lo = lo.reshape(nt, kq, 4, 64, 8)
    idx = idx.reshape(nt, kq, 4, 64, 8)
    sign = sign.reshape(nt, kq, 4, 64, 8)
    planes = np.zeros((nt, kq, CHUNK_BYTES), dtype=np.uint8)
    # low bytes: plane j // 2, byte lane * 16 + 8 (j % 2) + e
    lo_l = lo.transpose(0, 1, 3, 2, 4)                                   # [tile][q][lane][j][e]
    planes[:, :, 0:1024] = lo_l[:, :, :, 0:2, :].reshape(nt, kq, 1024)
    planes[:, :, 1024:2048] = lo_l[:, :, :, 2:4, :].reshape(nt, kq, 1024)
    # indices: one dword per (lane, j)
    e = np.arange(8)
    nib = np.where(e < 4, 2 * e, 2 * (e - 4) + 1).astype(np.uint32)
    ixw = (idx << (4 * nib)).sum(axis=-1, dtype=np.uint64).astype(np.uint32)      # [tile][q][j][lane]
    ixw = np.ascontiguousarray(ixw.transpose(0, 1, 3, 2)).astype("<u4")          # [tile][q][lane][j]
    planes[:, :, 2048:3072] = ixw.view(np.uint8).reshape(nt, kq, 1024)
    # signs: one dword per lane
    j = np.arange(4)[:, None, None]
    bit = ((2 * j + e // 4) + 8 * (e % 4)).astype(np.uint32)                     # [j][1][e]
    sgw = (sign << bit).sum(axis=(2, 4), dtype=np.uint64).astype("<u4")          # [tile][q][lane]
    planes[:, :, 3072:3328] = np.ascontiguousarray(sgw).view(np.uint8).reshape(nt, kq, 256)
    hdr = (base.astype(np.uint32) | (raw.astype(np.uint32) << 8)).astype(np.uint32)
    return planes, hdr


def decode(planes: np.ndarray, hdr: np.ndarray) -> np.ndarray:
    """The packed uint16 weights [tiles][K / 32][64][8] the planes stand for. Exact for every tile whose header is not flagged raw; a flagged tile
    decodes to something else (its out-of-window weights come back as tiny values): the kernels do not decode it."""
    nt, kq, nb = planes.shape
    assert nb == CHUNK_BYTES
    base = (hdr & 0xFF).astype(np.uint32)[:, None, None, None, None]
    lo0 = planes[:, :, 0:1024].reshape(nt, kq, 64, 2, 8)
    lo1 = planes[:, :, 1024:2048].reshape(nt, kq, 64, 2, 8)
    lo = np.concatenate([lo0, lo1], axis=3).astype(np.uint32)                     # [tile][q][lane][j][e]
    ixw = np.ascontiguousarray(planes[:, :, 2048:3072]).view("<u4").reshape(nt, kq, 64, 4, 1).astype(np.uint32)
    sgw = np.ascontiguousarray(planes[:, :, 3072:3328]).view("<u4").reshape(nt, kq, 64, 1, 1).astype(np.uint32)
    e = np.arange(8)
    nib = np.where(e < 4, 2 * e, 2 * (e - 4) + 1).astype(np.uint32)
    idx = (ixw >> (4 * nib)) & 0xF
    j = np.arange(4)[:, None]
    bit = ((2 * j + e // 4) + 8 * (e % 4)).astype(np.uint32)                      # [j][e]
    sign = (sgw >> bit) & 1
    h = np.where(idx != 0, base + idx, 0)
    w = (sign << 15) | (h << 8) | lo
    # [tile][q][lane][j][e] -> [tile][4 q + j][lane][e]
    return np.ascontiguousarray(w.transpose(0, 1, 3, 2, 4)).reshape(nt, kq * 4, 64, 8).astype(np.uint16)


def dense(packed: np.ndarray) -> np.ndarray:
    """The dense words of the packed weight [tiles][K / 32][64][8] uint16 (the input of encode): uint32 [tiles], 1 for a tile that is not flagged raw and
    none of whose weights has h = 0 (index 0: zeros, subnormals, the first normal binade; padding rows are zeros), 0 otherwise. Every index of a dense tile
    is 1..15, so its high bytes are sign << 7 | (base + index) with no zero case: the kernels decode it without the zero test. The device encoder
    stores the words behind the header words, hdr[tiles + tile]."""
    nt = packed.shape[0]
    assert packed.dtype == np.uint16
    h = ((packed >> 8) & 0x7F).astype(np.int32).reshape(nt, -1)
    lo, hi = h.min(axis=1), h.max(axis=1)
    # no h = 0, no Inf / NaN (then top = hi), and the smallest h inside the window: index >= 1 for every weight
    return ((lo >= 1) & (hi <= 126) & (lo - np.maximum(hi - WINDOW, 0) >= 1)).astype(np.uint32)


def fallback_tiles(hdr: np.ndarray) -> int:
    return int(((hdr >> 8) & 1).sum())
