"""Sampled decoding restated in plain torch / numpy on the CPU in fp64, from its definition (include/rdx.h, rdx_sampling): what sample_step_k
(radialog_amd/csrc/elem.hip) must reproduce -- the scores row bit for bit, the token within the acceptance rule below. Order: the logits rules
(tests/_logits_rules.py), temperature, top-k, top-p on values, the integer draw.

    x          [B, V] tensor in the model dtype (fp16 / bf16): one logits row per batch row, the rules already applied
    sampling   (temperature, top_k, top_p, seed); (1.0, 0, 1.0, .) warps nothing
    n_gen      B ints: the draw index of each row = the tokens it has generated

The acceptance rule for a device token. With F the fp64 normalised CDF over the kept elements in index order and u = u24 * 2^-24, token i must be kept
and satisfy F[i-1] - DELTA <= u < F[i] + DELTA, DELTA = 2^-16: the device takes exp in fp32 through exp2 (argument rounding over the fp32 exp range,
<= 88 * 2^-23 relative) and quantises every mass to 2^-32 (<= 32001 * 2^-33 in sum); together about 1.4e-5 <= 2^-16. The kept set has no such slack:
a row is usable for a bit-for-bit comparison when no M(v) lies within MARGIN = 2^-14 of 1 - p (`margin`), and the tests redraw the others."""
import math

import numpy as np
import torch

DELTA = 2.0 ** -16
MARGIN = 2.0 ** -14
_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_MASK = 0xFFFFFFFF


def philox4x32_10(ctr, key):
    """Philox4x32 with 10 rounds (Salmon et al., SC'11) on python ints: ctr 4 words, key 2 words -> 4 words."""
    c0, c1, c2, c3 = (int(c) & _MASK for c in ctr)
    k0, k1 = (int(k) & _MASK for k in key)
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & _MASK, p1 & _MASK, ((p0 >> 32) ^ c3 ^ k1) & _MASK, p0 & _MASK
        k0, k1 = (k0 + _W0) & _MASK, (k1 + _W1) & _MASK
    return c0, c1, c2, c3


def u24(seed: int, row: int, draw: int) -> int:
    return philox4x32_10((row, draw, 0, 0), (seed & _MASK, (seed >> 32) & _MASK))[0] >> 8


def scale(x: torch.Tensor, t: float) -> torch.Tensor:
    """scores / temperature on a model-dtype tensor: fp32 IEEE division (t rounded to fp32), one round-to-nearest-even."""
    if float(t) == 1.0:
        return x.clone()
    return (x.to(torch.float32) / torch.tensor(t, dtype=torch.float32)).to(x.dtype)


def _weights(s64: np.ndarray) -> np.ndarray:
    m = s64.max()
    with np.errstate(invalid="ignore"):
        w = np.exp(s64 - m)
    return np.where(np.isfinite(s64), w, 0.0) if np.isfinite(m) else np.zeros_like(s64)


def warp_row(row: torch.Tensor, t: float, k: int, p: float):
    """One row through temperature, top-k and the value-based top-p. Returns (scores row in the row's dtype: kept = scaled value, dropped = -inf;
    kept mask bool [V]; the smallest |M(v) - (1 - p)| over the values whose fate M decides, inf when top-p is off)."""
    s = scale(row, t)
    s64 = s.to(torch.float64).numpy()
    V = s64.shape[0]
    kept = np.ones(V, dtype=bool)
    if k > 0:
        v = np.sort(s64)[V - min(int(k), V)]                       # the min(k, V)-th largest
        kept &= ~(s64 < v)                                          # ties with it stay
    gap = math.inf
    p32 = float(np.float32(p))
    if p32 < 1.0:
        w = np.where(kept, _weights(np.where(kept, s64, -np.inf)), 0.0)
        order = np.argsort(s64, kind="stable")
        cs = np.cumsum(w[order])
        last_le = np.searchsorted(s64[order], s64, side="right") - 1   # the last element of the sorted row with a value <= s_i
        M = cs[last_le] / cs[-1]
        top = s64 == s64[kept].max()
        drop = (M <= 1.0 - p32) & ~top
        decided = kept & ~top
        if decided.any():
            gap = float(np.abs(M[decided] - (1.0 - p32)).min())
        kept &= ~drop
    out = s.clone()
    out[torch.from_numpy(~kept)] = float("-inf")
    return out, kept, gap


def cdf(scores_row: torch.Tensor) -> np.ndarray:
    """fp64 normalised inclusive CDF in index order over the kept (finite) elements of a processed row; flat across dropped ones."""
    w = _weights(scores_row.to(torch.float64).numpy())
    c = np.cumsum(w)
    return c / c[-1]


def accepts(scores_row: torch.Tensor, token: int, u24_: int):
    """The acceptance rule. Returns (ok, text for the assertion message)."""
    F = cdf(scores_row)
    u = u24_ * 2.0 ** -24
    lo = F[token - 1] if token > 0 else 0.0
    ok = bool(torch.isfinite(scores_row[token].float())) and lo - DELTA <= u < F[token] + DELTA
    return ok, f"token {token}: F[i-1] = {lo:.9f}, u = {u:.9f}, F[i] = {F[token]:.9f}, score {float(scores_row[token])}"


def draw(scores_row: torch.Tensor, u24_: int) -> int:
    """The integer draw of the definition, with fp64 masses: q = rint(w * 2^32), C = prefix sums in index order, target = (u24 * C_last) >> 24, the
    first i with C_i > target."""
    q = np.rint(_weights(scores_row.to(torch.float64).numpy()) * 2.0 ** 32).astype(np.uint64)
    C = np.cumsum(q, dtype=np.uint64)
    target = (int(u24_) * int(C[-1])) >> 24
    return int(np.searchsorted(C, np.uint64(target), side="right"))


def sample_rows(x: torch.Tensor, n_gen, sampling):
    """Every row of x: (scores [B, V], tokens int64 [B] by `draw`, u24 per row, the smallest top-p gap per row)."""
    t, k, p, seed = sampling
    out, toks, us, gaps = x.clone(), [], [], []
    for b in range(x.shape[0]):
        out[b], _, gap = warp_row(x[b], t, k, p)
        us.append(u24(int(seed), b, int(n_gen[b])))
        toks.append(draw(out[b], us[-1]))
        gaps.append(gap)
    return out, torch.tensor(toks, dtype=torch.int64), us, gaps
