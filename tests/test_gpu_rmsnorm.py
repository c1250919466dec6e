"""launch_rmsnorm (elem.hip: rmsnorm4096_k at H = 4096 with a weight and <= 4 slab groups, rmsnorm_k otherwise) alone, through rdx_rmsnorm_test, into
every activation layout of ActLayout (csrc/rdx_kernels.h). The hook fills output and scales with 0xff bytes first, so "not written" can be asserted.
Layout 0 (row-major) is held against the fp64 reference of tests/_dec_gemm.py (rms_ref's RSTD_REL interval, the bar of the decoder GEMM tests);
everything else is exact: a packed layout, un-permuted, IS the row-major output; layout 4's e4m3 codes and scales ARE layout 5's; a slab fold IS
_dec_gemm.combine_slabs followed by a slab-free norm; a combination without a kernel is refused before anything is launched.

Shapes: H = 4096 with a weight (rmsnorm4096_k), H = 512 and H = 4096 without a weight (rmsnorm_k; no weight = re-layout only); 1, 17 and 32 rows for the
32-row layouts, 33 and 40 rows (3 row tiles: one whole pad tile short of two blocks) for the row tiles and the e4m3 blocks; 2 and 4 slab groups, and 5
(rmsnorm_k's loop, beyond rmsnorm4096_k's four registers) where rmsnorm_k holds the layout."""
import pytest
import torch

import _dec_gemm as D

pytestmark = pytest.mark.gpu

ROWS, BLK32, BLK64, TILES32, BLK64_E4M3, ROWS_E4M3 = range(6)        # ActLayout
SLACK = 4096                                                          # bytes (and 8 scales) past every layout's extent that must stay 0xff
LEGS = [(4096, True), (512, True), (4096, False)]                     # (H, with a norm weight)
_CACHE = {}


@pytest.fixture(scope="module", params=["f16", "bf16"])
def eng(request):
    from radialog_amd.config import small_cfg
    from radialog_amd.engine import RdxEngine
    e = RdxEngine(small_cfg(), dtype=request.param, device=0, max_batch=1, max_len=32, llama=False, vision=False)
    e.dt = D.DT[request.param]
    yield e
    e.close()
    _CACHE.clear()


def _held(layout, rows, mtiles):
    """Rows the layout's buffer holds."""
    if layout in (ROWS, ROWS_E4M3):
        return rows
    if layout == TILES32:
        return 16 * mtiles
    return 32 * ((mtiles + 1) // 2) if layout == BLK64_E4M3 and mtiles > 2 else 32


def _run(eng, x, nw, layout, mtiles=0, slab=None):
    """(error or None, un-permuted rows [held, H] (model dtype, or e4m3 codes as uint8), scales [held] or None, updated x), all on the CPU. Asserts that
    nothing past the layout's extent was written, and after a refusal nothing at all."""
    rows, H = x.shape
    held = _held(layout, rows, mtiles)
    e4m3 = layout in (BLK64_E4M3, ROWS_E4M3)
    nbytes = held * H * (1 if e4m3 else 2)
    err, out, xs, xnew = eng.rmsnorm_test(x, nw, layout, mtiles=mtiles, slab=slab, eps=D.EPS, out_bytes=nbytes + SLACK, n_scales=held + 8 if e4m3 else 0)
    out, xs, xnew = out.cpu(), None if xs is None else xs.cpu(), xnew.cpu()
    if err is not None:
        assert bool((out == 0xff).all()) and (xs is None or bool((xs.view(torch.uint8) == 0xff).all())), "a refused norm wrote its output"
        assert torch.equal(xnew, x.to(eng.dt)), "a refused norm changed x"
        return err, None, None, xnew
    assert bool((out[nbytes:] == 0xff).all()), f"layout {layout}: bytes past the layout's extent were written"
    if e4m3:
        assert bool((xs[held:].view(torch.uint8) == 0xff).all()), f"layout {layout}: scales past the layout's rows were written"
        xs = xs[:held]
    body = out[:nbytes] if e4m3 else out[:nbytes].view(eng.dt)
    if layout in (BLK32, TILES32):
        r = D.unpack_frag(body.reshape(H // 32, held // 16, 64, 8))
    elif layout == BLK64:
        r = D.unpack_frag64(body)
    elif layout == BLK64_E4M3:
        r = torch.cat([D.unpack_frag64_e4m3(b) for b in body.reshape(held // 32, 32 * H)])
    else:
        r = body.reshape(held, H)
    return None, r, xs, xnew


def _inputs(eng, H, with_w):
    """40 rows, the norm weight (or None) and the layout-0 output of all 40 rows: one launch per (dtype, H, weight), shared by the tests."""
    key = (eng.dt, H, with_w)
    if key not in _CACHE:
        x = D.make_rows(40, H, eng.dt, 7 + H)
        nw = D.make_norm_w(H, eng.dt, 8 + H) if with_w else None
        err, ref, _, xnew = _run(eng, x, nw, ROWS)
        assert err is None and torch.equal(xnew, x), "layout 0 without slabs"
        _CACHE[key] = (x, nw, ref)
    return _CACHE[key]


def _bits(t):
    return t if t.dtype == torch.uint8 else t.contiguous().view(torch.int16)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _cases(H, with_w, slabs=False):
    """(layout, rows, mtiles) the launcher supports on this leg."""
    big = H == 4096 and with_w                                       # rmsnorm4096_k: the only holder of slabs into row tiles and of more than one e4m3 block
    c = [(lay, rows, 0) for lay in (ROWS_E4M3, BLK32, BLK64, BLK64_E4M3) + ((ROWS,) if slabs else ()) for rows in (1, 17, 32)]
    c += [(TILES32, rows, (rows + 15) // 16) for rows in (1, 17, 32) if not slabs or big]
    c += [(TILES32, rows, 3) for rows in (33, 40) if not slabs or big]
    c += [(BLK64_E4M3, rows, 3) for rows in (33, 40) if big]
    return c


@pytest.mark.parametrize("H,with_w", LEGS)
def test_layout0_lies_in_the_reference_interval(eng, H, with_w):
    """Row-major output against fp64: inside rms_ref's interval (RSTD_REL), every element. Without a weight the launch is a copy."""
    x, nw, ref = _inputs(eng, H, with_w)
    if not with_w:
        assert _same(ref, x), "w = null is a re-layout only"
        return
    _, _, lo, hi = D.rms_ref(x, nw, eng.dt)
    o = ref.double()
    worst = float((torch.maximum(lo - o, o - hi).clamp_min(0) / D.ulp(o, eng.dt)).max())
    print(f"rmsnorm layout 0 {eng.dt} H={H}: worst excess over the interval {worst} ulp")
    assert bool(torch.isfinite(o).all()) and bool(((o >= lo) & (o <= hi)).all()), f"{worst} ulp outside the RSTD_REL interval"
    for rows in (1, 17):                                             # a call's rows do not depend on how many rows it has
        assert _same(_run(eng, x[:rows], nw, ROWS)[1], ref[:rows]), f"{rows}-row call differs from the 40-row call"


@pytest.mark.parametrize("H,with_w", LEGS)
def test_packed_layouts_equal_row_major(eng, H, with_w):
    """Layouts 1, 2, 3 un-permuted = layout 0 bit for bit on the real rows, pad rows zero; layout 4's codes and scales = layout 5's, pad rows zero bytes
    with scale 1. (Bytes past every extent: _run.)"""
    x, nw, ref = _inputs(eng, H, with_w)
    codes = {}
    for layout, rows, mtiles in _cases(H, with_w):
        err, r, xs, xnew = _run(eng, x[:rows], nw, layout, mtiles)
        what = f"layout {layout}, {rows} rows, mtiles {mtiles}"
        assert err is None, f"{what}: {err}"
        assert torch.equal(xnew, x[:rows]), f"{what}: x changed without slabs"
        if layout == ROWS_E4M3:
            codes[rows] = (r, xs)
            continue
        assert not bool(_bits(r[rows:]).any()), f"{what}: pad rows are not zero"
        if layout != BLK64_E4M3:
            assert _same(r[:rows], ref[:rows]), f"{what}: differs from the row-major output"
            continue
        if rows not in codes:
            codes[rows] = _run(eng, x[:rows], nw, ROWS_E4M3)[1:3]
        assert torch.equal(r[:rows], codes[rows][0]), f"{what}: e4m3 codes differ from the row-major codes"
        assert torch.equal(xs[:rows], codes[rows][1]) and bool((xs[rows:] == 1.0).all()), f"{what}: scales differ from the row-major ones / pad scales are not 1"


@pytest.mark.parametrize("H,with_w", LEGS)
def test_slabs_are_folded_in_first(eng, H, with_w):
    """x += T(sum of the slabs, group order) exactly (combine_slabs), written back, and the output = a slab-free call on the updated rows. 2 and 4 groups
    on both kernels; 5 groups (rmsnorm_k even at H = 4096 with a weight) into the one-block layouts."""
    x, nw, _ = _inputs(eng, H, with_w)
    g = torch.Generator().manual_seed(99 + H)
    for layout, rows, mtiles in _cases(H, with_w, slabs=True):
        for groups in (2, 4, 5):
            if groups == 5 and (rows != 17 or mtiles):
                continue
            held = 32 if layout in (ROWS, ROWS_E4M3) else _held(layout, rows, mtiles)
            slab = torch.randn(groups, held, H, generator=g) * 0.25
            what = f"layout {layout}, {rows} rows, mtiles {mtiles}, {groups} groups"
            err, r, xs, xnew = _run(eng, x[:rows], nw, layout, mtiles, slab=slab)
            assert err is None, f"{what}: {err}"
            assert _same(xnew, D.combine_slabs(list(slab[:, :rows]), x[:rows], eng.dt)), f"{what}: updated x is not x + T(sum of slabs)"
            err, r0, xs0, _ = _run(eng, xnew, nw, layout, mtiles)
            assert err is None and _same(r, r0) and (xs is None or torch.equal(xs, xs0)), f"{what}: output differs from the slab-free norm of the updated rows"


def test_combinations_without_a_kernel_are_refused(eng):
    """rmsnorm_k holds no slabs into row tiles and one e4m3 block; rmsnorm4096_k four slab groups. Refused before anything is launched: an error, output,
    scales and x untouched (_run)."""
    for H, with_w in LEGS:
        x, nw, _ = _inputs(eng, H, with_w)
        big = H == 4096 and with_w
        for groups in ((5,) if big else (2, 5)):
            slab = torch.zeros(groups, 64, H)
            assert _run(eng, x[:33], nw, TILES32, 3, slab=slab[:, :48])[0] is not None, f"H {H}, weight {with_w}: {groups} slab groups into row tiles"
            assert _run(eng, x[:33], nw, BLK64_E4M3, 3, slab=slab)[0] is not None, f"H {H}, weight {with_w}: {groups} slab groups into e4m3 blocks"
        if not big:
            assert _run(eng, x[:33], nw, BLK64_E4M3, 3)[0] is not None, f"H {H}, weight {with_w}: two e4m3 blocks"
    x, nw, _ = _inputs(eng, 4096, True)
    assert _run(eng, x[:33], nw, BLK32)[0] is not None, "33 rows into a 32-row block"
    assert _run(eng, x[:40], nw, TILES32, 2)[0] is not None, "40 rows into two row tiles"
    assert _run(eng, x[:33], nw, ROWS, slab=torch.zeros(2, 64, 4096))[0] is not None, "row-major slabs hold 32 rows"
