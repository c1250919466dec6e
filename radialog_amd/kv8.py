"""fp8 KV cache ("kv8"): the definition of the opt-in cache format of the decoder, in plain torch on the CPU. The device quantiser (csrc/attn.hip
kv8_quant_rows_k, and wave 0 of decode attention for the new token's row), the in-register expansion (csrc/rdx_common.h kv8_expand) and the read-back
kernel (kv8_read_k) are compared with this file byte for byte and bit for bit.

kv8 is a STORAGE format of the cache, not an arithmetic: a stored row is defined by its dequantised value x', and decode attention over a kv8 cache gives
the bits it gives over a cache of the model dtype T that holds x'.

For one cache row (one position of one head: 128 values x of the model dtype T, finite):
    amax = max |x|
    e    = the smallest integer with amax 2^-e <= 448: with frexp(amax) = (m, ex), e = ex - 9 if m <= 0.875 else ex - 8; clamped below at EMIN = -15
           (a zero row gets -15); one signed byte
    code = RNE_e4m3(x 2^-e)               OCP e4m3fn; the scaling by a power of two is exact, so there is ONE rounding, and nothing saturates
    x'   = code 2^e
Every x' is exactly a bf16 and an f16 value: a code has 4 significant bits, and e >= -15 keeps the smallest subnormal code (2^-9) at 2^-24, the smallest
f16 subnormal. The quantiser is idempotent in VALUE: dequant(quant(x')) is x', bit for bit. It gives the same BYTES too, with one exception: a row whose
largest code came out as 224 (amax 2^-e in (224, 240) rounds down to 224 = 0.875 2^8, the closed end of the exponent rule) re-quantises with e - 1 and
every code doubled -- the same values in other bytes (test_kv8_host.py holds both statements). Nothing in the engine re-quantises a stored row.
The side information is one byte per 128.

K and V each hold codes [rows][heads][max_len][128] bytes and exponents [rows][heads][max_len] int8. This file and the library's read-back calls speak
the LOGICAL order only; how the K codes of a (row, head) slab are stored is the kernels' business (k_store / k_logical below restate it for the
kernel tests: every group of 16 positions is [g = (dim % 32) / 8][r = pos % 16][dim / 32][8], so that the 32 bytes of an MFMA A-fragment lane are
contiguous). V codes are stored row-major.
"""
import torch

D = 128
EMIN = -15
CODE_MAX = 448.0


def exponent(x: torch.Tensor) -> torch.Tensor:
    """x [..., 128] (any float dtype, finite) -> the row exponents [...] int8."""
    amax = x.double().abs().amax(-1)
    m, ex = torch.frexp(amax)
    e = torch.where(m <= 0.875, ex - 9, ex - 8)
    return torch.where(amax == 0, torch.full_like(e, EMIN), e).clamp_min(EMIN).to(torch.int8)


def quant(x: torch.Tensor):
    """x [..., 128] -> (codes uint8 [..., 128], e int8 [...])."""
    assert x.shape[-1] == D
    e = exponent(x)
    scaled = torch.ldexp(x.double(), -e.to(torch.int32)[..., None]).float()          # exact, or below half the smallest code (which rounds to a zero)
    assert bool((scaled.abs() <= CODE_MAX).all()), "kv8.quant: non-finite input"
    return scaled.to(torch.float8_e4m3fn).view(torch.uint8), e


def dequant(codes: torch.Tensor, e: torch.Tensor, dtype=torch.float32) -> torch.Tensor:
    """(codes uint8 [..., 128], e int8 [...]) -> x' [..., 128] in `dtype` (exact in float32, bfloat16 and float16)."""
    v = torch.ldexp(codes.view(torch.float8_e4m3fn).double(), e.to(torch.int32)[..., None])
    out = v.to(dtype)
    assert torch.equal(out.double(), v), "kv8.dequant: a stored value is not representable"
    return out


def roundtrip(x: torch.Tensor) -> torch.Tensor:
    """x' in the dtype of x."""
    return dequant(*quant(x), dtype=x.dtype)


def cache_bytes(layers: int, rows: int, heads: int, max_len: int) -> int:
    """Bytes of the K and V codes and exponents of a decoder."""
    return 2 * layers * rows * heads * max_len * (D + 1)


# ---- the storage order of the K codes (kernel tests only) ------------------------------------------------------------------------------------------------
def k_store(codes: torch.Tensor) -> torch.Tensor:
    """[..., L, 128] logical -> the slab as stored (same shape, L % 16 == 0)."""
    lead, L, n = codes.shape[:-2], codes.shape[-2], codes.dim() - 2
    r = codes.reshape(*lead, L // 16, 16, 4, 4, 8)                                     # [group][r][dim / 32][g][8]
    return r.permute(*range(n), n, n + 3, n + 1, n + 2, n + 4).reshape(*lead, L, D)  # [group][g][r][dim / 32][8]


def k_logical(slab: torch.Tensor) -> torch.Tensor:
    lead, L, n = slab.shape[:-2], slab.shape[-2], slab.dim() - 2
    r = slab.reshape(*lead, L // 16, 4, 16, 4, 8)                                      # [group][g][r][dim / 32][8]
    return r.permute(*range(n), n, n + 2, n + 3, n + 1, n + 4).reshape(*lead, L, D)
