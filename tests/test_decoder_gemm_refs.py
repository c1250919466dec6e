"""CPU leg of tests/test_gpu_decoder_gemms.py: the fragment layouts as the test restates them, and the evidence that the bars of tests/_dec_gemm.py
are neither too tight for a correct fp32 evaluation (torch fp32 partial sums per 32-deep chunk, combined per wave and then across waves / slabs in
the kernels' order, fp32 statistics, the kernels' rounding points) nor too loose to see a plausible bug (the perturbations the GPU tests use)."""
import pytest
import torch

import _dec_gemm as D

DTS = ["f16", "bf16"]


@pytest.mark.parametrize("mtiles", [2, 3, 8, 12])
def test_fragment_layout_round_trips_and_matches_its_statement(mtiles):
    """[k / 32][row tiles][lane = 16 g + r][8] with g = (k % 32) / 8, r = row % 16: pack and unpack are inverse, pad rows pack to zero, and single
    elements sit where the statement says (so the two functions are not merely each other's inverse)."""
    M, K = 16 * mtiles - 5, 160
    rows = torch.arange(M * K, dtype=torch.float32).reshape(M, K) + 1
    buf = D.pack_frag(rows, mtiles)
    assert buf.shape == (K // 32, mtiles, 64, 8)
    back = D.unpack_frag(buf)
    assert torch.equal(back[:M], rows) and float(back[M:].abs().max()) == 0.0
    for m, k in [(0, 0), (M - 1, K - 1), (17, 41), (16 * mtiles - 16, 96), (5, 159)]:
        assert buf[k // 32, m // 16, 16 * ((k % 32) // 8) + m % 16, k % 8] == rows[m, k]
    if mtiles == 2:          # the fp8 kernels' 64-deep order of one 32-row block
        K = 128
        rows = torch.arange(32 * K, dtype=torch.float32).reshape(32, K)
        buf = torch.zeros(K // 32, 2, 64, 8)
        for m in range(32):
            for k in range(K):
                buf[2 * (k // 64) + (k % 16) // 8, m // 16, 16 * ((k % 64) // 16) + m % 16, k % 8] = rows[m, k]
        assert torch.equal(D.unpack_frag64(buf.flatten()), rows)


def _xstat(dt, N, M=13, seed=3):
    K = 4096
    x, nw, w = D.make_rows(M, K, dt, seed), D.make_norm_w(K, dt, seed + 1), D.make_w(N, K, dt, seed + 2)
    xn, dxn, _, _ = D.rms_ref(x, nw, dt)
    acc = D.emu_gemm(D.emu_norm(x, nw, dt), w, D.wave_slices(128, 8))
    return x, nw, w, xn, dxn, acc


@pytest.mark.parametrize("dtn", DTS)
def test_xstat_bars_accept_fp32_and_reject_bugs(dtn):
    """xstat16_k / the row-block xstat32_k behind a norm (same chain count, 56): plain, SwiGLU; dropped K piece, swapped chunks, gate / up
    exchanged, eps x 10 on the low-variance row, the last row replaced by its neighbour."""
    dt = D.DT[dtn]
    x, nw, w, xn, dxn, acc = _xstat(dt, 64)
    c = D.c_xstat16()
    y, al = D.gemm_ref(xn, w, c, dxn)
    out = acc.to(dt)
    ok, ex, off = D.check(out, D.bar_plain(y, al, dt), dt)
    assert ok and off <= 1, (ex, off)
    D.sensitive(out, D.bar_plain(*D.gemm_ref(D.drop_piece(xn, 512 * 3 + 32 * 5 + 8), w, c, dxn), dt), dt, "a dropped 8-element K piece")
    D.sensitive(out, D.bar_plain(*D.gemm_ref(xn, D.swap_chunks(w, 16 * 2 + 7), c, dxn), dt), dt, "two chunks swapped in the weight")
    xn10, dxn10, _, _ = D.rms_ref(x, nw, dt, eps=10 * D.EPS32)
    ok10, _, _ = D.check(out[1:2], D.bar_plain(*D.gemm_ref(xn10[1:2], w, c, dxn10[1:2]), dt), dt)
    assert not ok10, "eps x 10 on the low-variance row not seen"
    xb = D.neighbour_row(x)
    xnb, dxnb, _, _ = D.rms_ref(xb, nw, dt)
    D.sensitive(out, D.bar_plain(*D.gemm_ref(xnb, w, c, dxnb), dt), dt, "the last row replaced by its neighbour")
    sw = D.emu_swiglu(acc, dt)
    ok, ex, off = D.check(sw, D.bar_swiglu(y, al, dt), dt)
    assert ok, (ex, off)
    D.sensitive(sw, D.bar_swiglu(*D.gemm_ref(xn, D.swap_gate_up(w, 2), c, dxn), dt), dt, "gate and up halves of a tile exchanged")
    # the norm alone (the packing norms' output): inside its own interval
    _, _, lo, hi = D.rms_ref(x, nw, dt)
    e = D.emu_norm(x, nw, dt).double()
    assert bool(((e >= lo) & (e <= hi)).all())


@pytest.mark.parametrize("dtn", DTS)
@pytest.mark.parametrize("K", [512, 544, 4128, 11008])
def test_xrow16_bar_accepts_fp32_and_rejects_bugs(dtn, K):
    """xrow16_k: 16 waves over K / 32 chunks (uneven at 544 and 4128, 21 / 22 at 11008), residual epilogue, no norm: rows of different scales."""
    dt = D.DT[dtn]
    M, N = 13, 64
    x, w = D.make_rows(M, K, dt, K), D.make_w(N, K, dt, K + 1)
    resid = D.make_rows(M, N, dt, K + 2, scales=False)
    xd = x.double()
    c = D.c_xrow16(K)
    out = D.emu_resid(D.emu_gemm(x, w, D.wave_slices(K // 32, 16)), resid, dt)
    ok, ex, off = D.check(out, D.bar_resid(*D.gemm_ref(xd, w, c), resid, dt), dt)
    assert ok, (ex, off)
    D.sensitive(out, D.bar_resid(*D.gemm_ref(D.drop_piece(xd, K - 40), w, c), resid, dt), dt, "a dropped 8-element K piece")
    D.sensitive(out, D.bar_resid(*D.gemm_ref(xd, D.swap_chunks(w, K // 64), c), resid, dt), dt, "two chunks swapped in the weight")
    D.sensitive(out, D.bar_resid(*D.gemm_ref(D.neighbour_row(x).double(), w, c), resid, dt), dt, "the last row replaced by its neighbour")


@pytest.mark.parametrize("dtn", DTS)
def test_xsplit_bar_accepts_fp32_and_rejects_a_missing_slab(dtn):
    """The row-block xsplit32_k at K = 11008: 4 K groups of 8 waves over 344 chunks (10 / 11 per wave), one fp32 slab per group; the slabs are held
    to the accumulation allowance alone (nothing is rounded to the model dtype), the combined rows to the residual bar."""
    dt = D.DT[dtn]
    M, N, K = 37, 64, 11008
    x, w = D.make_rows(M, K, dt, 5), D.make_w(N, K, dt, 6)
    resid = D.make_rows(M, N, dt, 7, scales=False)
    sl = D.wave_slices(344, 32)
    slabs = [D.emu_gemm(x, w, sl[8 * g:8 * g + 8]) for g in range(4)]
    xd = x.double()
    for g in range(4):
        k0, k1 = 32 * sl[8 * g][0], 32 * sl[8 * g + 7][-1] + 32
        assert (k0, k1) == (2752 * g, 2752 * g + 2752)
        y, al = D.gemm_ref(xd[:, k0:k1], w[:, k0:k1], D.c_xsplit_blk(False))
        assert bool(((slabs[g].double() - y).abs() <= al).all()), g
    out = D.combine_slabs(slabs, resid, dt)
    y, al = D.gemm_ref(xd, w, D.c_xsplit_blk())
    ok, ex, off = D.check(out, D.bar_resid(y, al, resid, dt), dt)
    assert ok, (ex, off)
    D.sensitive(D.combine_slabs(slabs[:2] + slabs[3:], resid, dt), D.bar_resid(y, al, resid, dt), dt, "one slab group left out of the combine")


def test_first_argmax_takes_the_lowest_index_on_ties():
    lg = torch.tensor([[1.0, 3.0, 3.0, 2.0], [5.0, 1.0, 5.0, 5.0]], dtype=torch.float16)
    assert D.first_argmax(lg).tolist() == [1, 0]
