"""The decoder's 3-16-row GEMMs (xs16.hip: xstat16_k, xrow16_k) and row-block GEMMs (xstat32.hip: xstat32_k<.., BLK>, xsplit32_k<.., BLK>, their fp8
forms, and the packing norms in front of them) one launch at a time through the hooks of include/rdx_dec_hooks.h, against fp64 on the
model-dtype-rounded operands with the kernels' rounding points. The references, the derivation of every bar (chain counts, the fp32 rstd, the
propagation through the residual and SwiGLU epilogues) and the perturbations are in tests/_dec_gemm.py; tests/test_decoder_gemm_refs.py shows on
the CPU that those bars accept a correct fp32 evaluation and reject each perturbation. Beyond the bars, exact invariants: row independence, packed
= row-major, NaN where nothing may be written, the greedy choice = first argmax of the kernel's own logits with planted ties, and -- fp8 -- bit
equality with the 32-row kernels row block by row block. One weight per test, reused over all row counts."""
import pytest
import torch

import _dec_gemm as D
from _dec_gemm import EPS

pytestmark = pytest.mark.gpu

M16 = [16, 13, 12, 9, 8, 5, 4, 3]                                  # 16 first: the call every smaller one must agree with row by row
MBLK = [192, 177, 160, 128, 100, 88, 80, 49, 48, 33, 20]           # mtiles 12, 12, 10, 8, 7, 6, 5, 4, 3, 3, 2
K = 4096
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


def _normed_rows(dt, M, seed):
    """(x, norm weight, xn, dxn, lo, hi) of M rows of 4096, computed once per dtype."""
    key = ("rows", dt, M)
    if key not in _CACHE:
        x, nw = D.make_rows(M, K, dt, seed), D.make_norm_w(K, dt, seed + 1)
        _CACHE[key] = (x, nw) + D.rms_ref(x, nw, dt)
    return _CACHE[key]


def _isnan(t):
    return bool(torch.isnan(t.float()).all())


def _plant(w, xn, m, n1, n2, logit=16.0):
    """Weight rows n1 and n2 := the same multiple of normalised row m, so that both columns tie at ~`logit`, far above every other column of row m
    (sigma = |xn| x 0.02 ~ 1.3, the maximum of 12 304 such ~ 5.5)."""
    row = (xn[m] * (logit / float((xn[m] * xn[m]).sum()))).float()
    w[n1] = row
    w[n2] = row


def _norm_sensitivity(out, x, nw, w, c, dt, bar_fn, name):
    """`out`: kernel rows for x behind the norm; the same bar on perturbed references must fail. w: a column slice of the weight."""
    xn, dxn, _, _ = D.rms_ref(x, nw, dt)
    D.sensitive(out, bar_fn(*D.gemm_ref(D.drop_piece(xn, 512 * 3 + 32 * 5 + 8), w, c, dxn)), dt, f"{name}: a dropped 8-element K piece of wave 3")
    D.sensitive(out, bar_fn(*D.gemm_ref(xn, D.swap_chunks(w, 16 * 6 + 15), c, dxn)), dt, f"{name}: two chunks swapped in the weight (a wave boundary)")
    xn10, dxn10, _, _ = D.rms_ref(x, nw, dt, eps=10 * D.EPS32)
    y10, al10 = D.gemm_ref(xn10[1:2], w, c, dxn10[1:2])
    D.sensitive(out[1:2], bar_fn(y10, al10), dt, f"{name}: eps x 10 on the low-variance row")
    xb = D.neighbour_row(x)
    xnb, dxnb, _, _ = D.rms_ref(xb, nw, dt)
    D.sensitive(out, bar_fn(*D.gemm_ref(xnb, w, c, dxnb)), dt, f"{name}: the last row replaced by its neighbour")


# ------------------------------------------------------------------------------------------------------------------------------------------
# xstat16_k
# ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [8192, 8208])
def test_xstat16_plain_matches_fp64(eng, N):
    """launch_xstat16, EPI_NONE, every row count, ldo = N + 24. N = 8192: 512 tiles = 256 groups of two, the grid is 256 workgroups with ONE trip
    each, so only the peeled last trip runs (no prefetch). N = 8208: 513 tiles = 257 groups; 257 % 256 = 1 < 128, so the launcher takes
    ceil(257 / 2) = 129 workgroups x 2 trips (the reduced grid), workgroup 128 has one trip, and the last group's second tile (513) is past
    `ntiles`: its weight pointer is clamped to tile 512 and nothing of it is stored. Chain count 56 (tests/_dec_gemm.py)."""
    dt = eng.dt
    x, nw, xn, dxn, _, _ = _normed_rows(dt, 16, 11)
    w = D.make_w(N, K, dt, N)
    wd = w.to(eng.device)
    c = D.c_xstat16()
    y, al = D.gemm_ref(xn, w, c, dxn)
    full, worst = None, 0.0
    for M in M16:
        out = eng.xstat16_test(x[:M], nw, wd, epi=0, ldo=N + 24).cpu()
        assert _isnan(out[M:]) and _isnan(out[:, N:]), f"M = {M}: rows >= M or columns >= N of a padded ldo were written"
        o = out[:M, :N]
        ok, ex, off = D.check(o, D.bar_plain(y[:M], al[:M], dt), dt)
        worst = max(worst, off)
        assert ok and off <= 1, f"M = {M}: {ex} ulp outside the interval, {off} ulp from T(ref) beyond the allowance"
        if full is None:
            full = o
        assert torch.equal(o, full[:M]), f"row independence: rows of the {M}-row call differ from the 16-row call's"
    print(f"xstat16_k NONE {dt} N={N}: worst {worst:.3f} ulp beyond the allowance")
    cols = slice(N - 512, N)                                     # the last tiles (the ragged group at 8208)
    _norm_sensitivity(full[:13, cols], x[:13], nw, w[cols], c, dt, lambda y_, al_: D.bar_plain(y_, al_, dt), "xstat16_k")


@pytest.mark.parametrize("N,n_valid", [(8208, 8201), (12304, 12290)])
def test_xstat16_logits_and_greedy_choice(eng, N, n_valid):
    """EPI_LOGITS. 8208: the reduced grid (129 workgroups x 2 trips); 12304: 769 tiles = 385 groups, 385 % 256 = 129 >= 128: the full 256-workgroup
    grid, 1-2 trips. Logits T(acc) for n < n_valid (NaN beyond: not written), choice = first argmax of the kernel's own logits. Planted exact
    ties (duplicated weight rows aligned with one activation row, far above every other logit): row 0 in the two tiles of one trip (workgroup 5:
    tiles 10, 11), row 2 in two trips of one workgroup (tile 14 and tile 14 + 2 G), row 1 as a pair whose larger index is >= n_valid (never a
    candidate: the smaller one must win although the larger has the same weights)."""
    dt = eng.dt
    x, nw, xn, dxn, _, _ = _normed_rows(dt, 16, 11)
    groups = (N // 16 + 1) // 2
    G = 256 if groups % 256 >= 128 else (groups + 1) // 2
    pairs = {0: (10 * 16 + 3, 11 * 16 + 9), 2: (14 * 16 + 5, (14 + 2 * G) * 16 + 5), 1: (n_valid - 3, n_valid + 2)}
    assert pairs[2][1] < n_valid and pairs[1][1] < N
    w = D.make_w(N, K, dt, N + 1)
    for m, (n1, n2) in pairs.items():
        _plant(w, xn, m, n1, n2)
    w = w.to(dt).float()
    wd = w.to(eng.device)
    y, al = D.gemm_ref(xn, w, D.c_xstat16(), dxn)
    full, worst = None, 0.0
    for M in M16:
        out, am = eng.xstat16_test(x[:M], nw, wd, epi=5, n_valid=n_valid)
        out = out.cpu()
        assert _isnan(out[M:]) and _isnan(out[:, n_valid:]), f"M = {M}: rows >= M or logit columns >= n_valid were written"
        o = out[:M, :n_valid]
        ok, ex, off = D.check(o, D.bar_plain(y[:M, :n_valid], al[:M, :n_valid], dt), dt)
        worst = max(worst, off)
        assert ok and off <= 1, f"M = {M}: {ex} ulp outside the interval, {off} beyond the allowance"
        assert torch.equal(am.long(), D.first_argmax(o)), f"M = {M}: the choice is not the first argmax of the kernel's own logits"
        for m, (n1, n2) in pairs.items():
            if n2 < n_valid:
                assert o[m, n1] == o[m, n2] == o[m].max(), f"row {m}: the planted tie is not an exact tie at the top"
            assert int(am[m]) == n1, f"row {m}: planted tie ({n1}, {n2}) -> {int(am[m])}"
        if full is None:
            full = o
        assert torch.equal(o, full[:M]), f"row independence at {M} rows"
    print(f"xstat16_k LOGITS {dt} N={N}: worst {worst:.3f} ulp beyond the allowance")


def test_xstat16_swiglu_packed_and_the_seam_into_xrow16(eng):
    """EPI_SILU_MUL at N = 22016: 1376 tiles = 688 groups on 256 workgroups -> 3 trips on workgroups 0-175, so the counted-wait middle loop
    (trip 1 of 3) runs. out_packed 0 and 1 must hold the same values (unpacked here from the stated layout), the packed block's pad rows M..15 are
    exactly zero and its second row tile is never written; xrow16_k (down_proj, K = 11008) fed the packed block directly -- the production seam of
    api_llama.hip -- equals xrow16_k fed the same rows re-laid from row-major, and meets the residual bar on those rows."""
    dt = eng.dt
    N, I, ND = 22016, 11008, 64
    x, nw, xn, dxn, _, _ = _normed_rows(dt, 16, 11)
    w = D.make_w(N, K, dt, N)
    wd = w.to(eng.device)
    wdn = D.make_w(ND, I, dt, 5)
    wdn_d = wdn.to(eng.device)
    resid = D.make_rows(16, ND, dt, 6, scales=False)
    c = D.c_xstat16()
    y, al = D.gemm_ref(xn, w, c, dxn)
    bar = D.bar_swiglu(y, al, dt)
    full, exact, worst_seam = None, 1.0, 0.0
    for M in M16:
        out = eng.xstat16_test(x[:M], nw, wd, epi=4, ldo=I + 8).cpu()
        assert _isnan(out[M:]) and _isnan(out[:, I:]), f"M = {M}: rows >= M or columns >= N / 2 were written"
        o = out[:M, :I].contiguous()
        ok, ex, _ = D.check(o, tuple(None if b is None else b[:M] for b in bar), dt)
        assert ok, f"M = {M}: {ex} ulp outside the SwiGLU interval"
        exact = min(exact, float((o.double() == bar[2][:M]).double().mean()))
        pk = eng.xstat16_test(x[:M], nw, wd, epi=4, out_packed=1)
        rows = D.unpack_frag(pk.cpu())
        assert torch.equal(rows[:M], o), f"M = {M}: out_packed 1 differs from the row-major output"
        assert float(rows[M:16].float().abs().max() if M < 16 else 0.0) == 0.0, f"M = {M}: pad rows of the packed block are not zero"
        assert _isnan(rows[16:]), "the second row tile of the packed block was written"
        seam = eng.xrow16_test(pk, wdn_d, resid[:M], M=M).cpu()
        relaid = eng.xrow16_test(o, wdn_d, resid[:M]).cpu()
        assert _isnan(seam[M:]) and torch.equal(seam[:M], relaid[:M]), f"M = {M}: xrow16_k on the packed block differs from xrow16_k on the re-laid rows"
        ok, ex, off = D.check(seam[:M], D.bar_resid(*D.gemm_ref(o.double(), wdn, D.c_xrow16(I)), resid[:M], dt), dt)
        worst_seam = max(worst_seam, off)
        assert ok, f"M = {M}: the seam's xrow16_k output is {ex} ulp outside the residual interval"
        if full is None:
            full = o
        assert torch.equal(o, full[:M]), f"row independence at {M} rows"
    print(f"xstat16_k SILU_MUL {dt}: all inside the interval, >= {100 * exact:.2f} % bit-equal to T(ref); seam xrow16_k worst {worst_seam:.3f} ulp")
    t0 = N // 16 - 32                                             # the last 32 tiles
    ys, als = D.gemm_ref(xn[:13], D.swap_gate_up(w[16 * t0:], 7), c, dxn[:13])
    D.sensitive(full[:13, 8 * t0:], D.bar_swiglu(ys, als, dt), dt, "xstat16_k: gate and up halves of a tile exchanged")


# ------------------------------------------------------------------------------------------------------------------------------------------
# xrow16_k
# ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [64, 4096])
@pytest.mark.parametrize("Kx", [512, 544, 4096, 4128, 11008])
def test_xrow16_matches_fp64(eng, Kx, N):
    """launch_xrow16 behind the production re-layout (launch_rmsnorm into ACT_BLK32 without a weight), residual epilogue, ldo = N + 8. 16 waves split
    K / 32 chunks as [KC w / 16, KC (w + 1) / 16): 512 -> one chunk per wave (tail only, one MFMA); 544 -> 17 chunks, wave 15 gets two; 4096 ->
    exactly XR_U = 8 per wave (the main loop's condition cb + 8 < c1 fails at once: tail only, whole ring); 4128 -> 129 chunks, one wave gets 9
    (one trip of the main loop with clamped refills, then a tail of one); 11008 -> 344 chunks, 21 / 22 per wave. At <= 4, <= 8, <= 12 rows
    the padding lanes re-read real rows (`xlane`): every row count must reproduce the 16-row call's rows bit for bit. Chain count 32 + ceil(KC / 16)
    + 16. No norm in front: the rows keep their different scales (2^-4 .. 2^2) and row 1 is ~1e-3."""
    dt = eng.dt
    x = D.make_rows(16, Kx, dt, Kx)
    w = D.make_w(N, Kx, dt, Kx + N)
    wd = w.to(eng.device)
    resid = D.make_rows(16, N, dt, 9, scales=False)
    c = D.c_xrow16(Kx)
    y, al = D.gemm_ref(x.double(), w, c)
    full, worst = None, 0.0
    for M in M16:
        out = eng.xrow16_test(x[:M], wd, resid[:M], ldo=N + 8).cpu()
        assert _isnan(out[M:]) and _isnan(out[:, N:]), f"M = {M}: rows >= M or columns >= N were written"
        o = out[:M, :N]
        ok, ex, off = D.check(o, D.bar_resid(y[:M], al[:M], resid[:M], dt), dt)
        worst = max(worst, off)
        assert ok, f"M = {M}: {ex} ulp outside the residual interval ({off} beyond the allowance)"
        if full is None:
            full = o
        assert torch.equal(o, full[:M]), f"row independence (xlane) at {M} rows"
    print(f"xrow16_k {dt} K={Kx} N={N}: worst {worst:.3f} ulp beyond the allowance")
    if N == 64:
        xd, r13, o13 = x[:13].double(), resid[:13], full[:13]
        KC = Kx // 32
        k0 = 32 * (KC * 5 // 16) + 8                              # lane group 1 of the first chunk of wave 5
        D.sensitive(o13, D.bar_resid(*D.gemm_ref(D.drop_piece(xd, k0), w, c), r13, dt), dt, "xrow16_k: a dropped 8-element K piece")
        D.sensitive(o13, D.bar_resid(*D.gemm_ref(xd, D.swap_chunks(w, KC - 2), c), r13, dt), dt, "xrow16_k: the last two chunks swapped in the weight")
        D.sensitive(o13, D.bar_resid(*D.gemm_ref(D.neighbour_row(x[:13]).double(), w, c), r13, dt), dt, "xrow16_k: row 12 replaced by row 11")


# ------------------------------------------------------------------------------------------------------------------------------------------
# row blocks, model dtype
# ------------------------------------------------------------------------------------------------------------------------------------------
def _blk_ref(dt, N, normed):
    key = ("blk", dt, N, normed)
    if key not in _CACHE:
        x, nw, xn, dxn, _, _ = _normed_rows(dt, 192, 21)
        w = D.make_w(N, K, dt, N + 7)
        if N == 8208:                                             # planted ties for the logits variant (harmless for the others)
            _plant(w, xn, 0, 10 * 16 + 3, 11 * 16 + 9)
            _plant(w, xn, 2, 14 * 16 + 5, 300 * 16 + 5)
            _plant(w, xn, 40, 8201 - 3, 8201 + 2)
            w = w.to(dt).float()
        y, al = D.gemm_ref(xn if normed else x.double(), w, D.c_xstat_blk(), dxn if normed else None)
        _CACHE[key] = (w, y, al)
    return _CACHE[key]


@pytest.mark.parametrize("variant", ["none", "resid", "swiglu", "logits"])
@pytest.mark.parametrize("N", [2048, 8208])
def test_xstat_blk_matches_fp64(eng, N, variant):
    """launch_rmsnorm into row tiles (ACT_TILES32) + launch_xstat_blk (xstat32_k<T, EPI, false, false, true>) at M = 20 .. 192. Grid 256 = 8 XCDs x 32 slots; NB =
    ceil(mtiles / 2) row blocks per walker, 32 / NB walkers per XCD (NB = 3, 5, 6 leave 2, 2, 2 slots idle: M = 80 / 88 / 160, 177, 192), G =
    8 (32 / NB) walkers over the N / 16 tiles (N = 2048: 128 tiles, the minimum, fewer tiles than walkers at NB = 1; 8208: 513, a ragged last
    round). An odd mtiles (M = 33, 48, 80, 100) makes the last block's second row tile a clamped re-read of the first (never stored); a ragged last
    tile re-reads real rows (xs_src_lane). Variants: none / logits / swiglu behind the norm WITH a weight (rmsnorm4096_k into ACT_TILES32), resid behind the
    re-layout only (rmsnorm_k into ACT_TILES32, no weight: rows keep their scales). swiglu: out_packed 0, and 3 where N % 64 == 0. Chain count 56. Row
    independence holds across ALL row counts, not only equal mtiles: a row's fragments, its MFMA column and the reduction order do not depend on
    mtiles or on the row's block (columns of an MFMA are independent), so every call must reproduce the 192-row call's rows bit for bit."""
    dt = eng.dt
    x, nw, xn, dxn, lo, hi = _normed_rows(dt, 192, 21)
    normed = variant != "resid"
    w, y, al = _blk_ref(dt, N, normed)
    wd = w.to(eng.device)
    resid = D.make_rows(192, N, dt, 23, scales=False) if variant == "resid" else None
    epi = {"none": 0, "resid": 3, "swiglu": 4, "logits": 5}[variant]
    n_valid = {2048: 2040, 8208: 8201}[N] if variant == "logits" else N
    cols = N // 2 if variant == "swiglu" else N
    ldo = cols + 8
    if variant == "swiglu":
        bar = D.bar_swiglu(y, al, dt)
    elif variant == "resid":
        bar = D.bar_resid(y, al, resid, dt)
    else:
        bar = D.bar_plain(y, al, dt)
    full, worst, exact = None, 0.0, 1.0
    for M in MBLK:
        mtl = (M + 15) // 16
        out, xp, am = eng.xstat_blk_test(x[:M], nw if normed else None, wd, epi=epi, resid=None if resid is None else resid[:M], n_valid=n_valid,
                                         ldo=ldo, want_xp=variant == "none")
        out = out.cpu()
        assert _isnan(out[M:]) and _isnan(out[:, min(cols, n_valid):]), f"M = {M}: rows >= M or columns >= N (n_valid) were written"
        o = out[:M, :min(cols, n_valid)]
        ok, ex, off = D.check(o, tuple(None if b is None else b[:M, :o.shape[1]] for b in bar), dt)
        worst = max(worst, off)
        exact = min(exact, float((o.double() == bar[2][:M, :o.shape[1]]).double().mean()))
        assert ok and (variant == "swiglu" or off <= 1), f"M = {M}: {ex} ulp outside the interval, {off} beyond the allowance"
        if full is None:
            full = o
        assert torch.equal(o, full[:M]), f"row independence: the {M}-row call differs from the 192-row call"
        if variant == "none":                                     # the packing norm's own output: inside the rstd interval, pad rows zero
            rows = D.unpack_frag(xp.cpu()).double()
            assert rows.shape == (16 * mtl, K) and bool(((rows[:M] >= lo[:M]) & (rows[:M] <= hi[:M])).all()), f"M = {M}: launch_rmsnorm into row tiles"
            assert float(rows[M:].abs().max() if M < 16 * mtl else 0.0) == 0.0, f"M = {M}: pad rows of the packed norm output are not zero"
        if variant == "swiglu" and N % 64 == 0:
            pk, _, _ = eng.xstat_blk_test(x[:M], nw, wd, epi=4, out_packed=3)
            rows = D.unpack_frag(pk.cpu())
            assert torch.equal(rows[:M], o), f"M = {M}: out_packed 3 differs from the row-major output"
            assert float(rows[M:].float().abs().max() if M < 16 * mtl else 0.0) == 0.0, f"M = {M}: pad rows of the packed block are not zero"
        if variant == "logits":
            assert torch.equal(am.long(), D.first_argmax(o)), f"M = {M}: the choice is not the first argmax of the kernel's own logits"
            if N == 8208:
                for m, n1, n2 in [(0, 163, 185), (2, 229, 4805), (40, 8198, 8203)]:
                    if m < M:
                        assert int(am[m]) == n1 and (n2 >= n_valid or o[m, n1] == o[m, n2] == o[m].max()), f"row {m}: planted tie -> {int(am[m])}"
    print(f"xstat32_k<BLK> {variant} {dt} N={N}: " + (f"all inside the interval, >= {100 * exact:.2f} % bit-equal to T(ref)" if variant == "swiglu" else
                                                      f"worst {worst:.3f} ulp beyond the allowance"))
    # sensitivity at 49 rows (row 48 alone in the last tile), on the last 256 columns
    cs = slice(N - 256, N)
    o49 = full[:49]
    c = D.c_xstat_blk()
    if variant == "none":
        _norm_sensitivity(o49[:, cs], x[:49], nw, w[cs], c, dt, lambda y_, al_: D.bar_plain(y_, al_, dt), "xstat32_k<BLK>")
    elif variant == "resid":
        xd, r = x[:49].double(), resid[:49, cs]
        D.sensitive(o49[:, cs], D.bar_resid(*D.gemm_ref(D.drop_piece(xd, 512 * 6 + 24), w[cs], c), r, dt), dt, "xstat32_k<BLK> resid: a dropped K piece")
        D.sensitive(o49[:, cs], D.bar_resid(*D.gemm_ref(D.neighbour_row(x[:49]).double(), w[cs], c), r, dt), dt, "xstat32_k<BLK> resid: row 48 := row 47")
    elif variant == "swiglu":
        ys, als = D.gemm_ref(xn[:49], D.swap_gate_up(w[cs], 3), c, dxn[:49])
        D.sensitive(o49[:, (N - 256) // 2:], D.bar_swiglu(ys, als, dt), dt, "xstat32_k<BLK>: gate and up halves of a tile exchanged")


@pytest.mark.parametrize("N", [2048, 4096])
def test_xsplit_blk_slabs_and_the_slab_norm(eng, N):
    """launch_rmsnorm (re-layout of [M][11008] into ACT_TILES32) + launch_xsplit_blk (xsplit32_k<T, 344, 4, false, 1, false, true>) at M = 33 .. 128: PS =
    32 / NB slots per XCD hold PS / 4 tile walkers x 4 K groups (NB = 3: 10 slots -> 2 walkers, 2 + 2 idle), K group kg = chunks [86 kg, 86 kg + 86)
    = k in [2752 kg, 2752 kg + 2752) over 8 waves (10 / 11 chunks each), slabs [4][16 mtiles][N] with the PADDED row count as the plane stride.
    Each slab is held to the accumulation allowance alone against the fp64 partial product of its K range (c = 51; nothing is rounded), rows >= M
    of every plane keep their NaN. The combine x += T(s0 + s1 + s2 + s3) is exact fp32 arithmetic, redone here: it must meet the residual bar
    (c = 55) and -- N = 4096, where the slab fold into row tiles exists (rmsnorm4096_k, H = 4096 only) -- equal the kernel's updated rows
    bit for bit; the packed norm of those rows lies in the rstd interval of the kernel's own rows, pad rows zero."""
    dt = eng.dt
    KD = 11008
    x = D.make_rows(128, KD, dt, 31)
    w = D.make_w(N, KD, dt, N + 3)
    wd = w.to(eng.device)
    resid = D.make_rows(128, N, dt, 33, scales=False)
    nw = D.make_norm_w(N, dt, 34)
    xd = x.double()
    parts = [D.gemm_ref(xd[:, 2752 * g:2752 * g + 2752], w[:, 2752 * g:2752 * g + 2752], D.c_xsplit_blk(False)) for g in range(4)]
    y, al = D.gemm_ref(xd, w, D.c_xsplit_blk())
    full, worst, worst_slab = None, 0.0, 0.0
    for M in [128, 88, 64, 48, 33]:
        mtl = (M + 15) // 16
        slab, r2, xnp = eng.xsplit_blk_test(x[:M], wd, resid=resid[:M] if N == 4096 else None, norm_w=nw if N == 4096 else None)
        slab = slab.cpu()
        assert slab.shape == (4, 16 * mtl, N) and _isnan(slab[:, M:]), f"M = {M}: slab rows >= M were written"
        for g in range(4):
            d = (slab[g, :M].double() - parts[g][0][:M]).abs() / parts[g][1][:M]
            assert bool(torch.isfinite(slab[g, :M]).all()) and float(d.max()) <= 1, f"M = {M}: slab {g} is {float(d.max())} allowances from its fp64 partial"
            worst_slab = max(worst_slab, float(d.max()))
        host = D.combine_slabs([slab[g, :M] for g in range(4)], resid[:M], dt)
        ok, ex, off = D.check(host, D.bar_resid(y[:M], al[:M], resid[:M], dt), dt)
        worst = max(worst, off)
        assert ok, f"M = {M}: the combined rows are {ex} ulp outside the residual interval"
        if N == 4096:
            assert torch.equal(r2.cpu(), host), f"M = {M}: the slab-folding norm's updated rows differ from x + T(s0 + s1 + s2 + s3)"
            rows = D.unpack_frag(xnp.cpu()).double()
            _, _, lo, hi = D.rms_ref(host, nw, dt)
            assert bool(((rows[:M] >= lo) & (rows[:M] <= hi)).all()), f"M = {M}: the slab norm's packed output leaves the rstd interval"
            assert float(rows[M:].abs().max() if M < 16 * mtl else 0.0) == 0.0, f"M = {M}: pad rows of the slab norm's packed output are not zero"
        if full is None:
            full = slab
        assert torch.equal(slab[:, :M], full[:, :M]), f"row independence: slabs of the {M}-row call differ from the 128-row call's"
        if M == 33:
            D.sensitive(D.combine_slabs([slab[g, :M] for g in (0, 1, 3)], resid[:M], dt), D.bar_resid(y[:M], al[:M], resid[:M], dt), dt,
                        "slab group 2 left out of the combine")
            D.sensitive(host, D.bar_resid(*D.gemm_ref(D.neighbour_row(x[:33]).double(), w, D.c_xsplit_blk()), resid[:M], dt), dt, "row 32 := row 31")
            D.sensitive(host, D.bar_resid(*D.gemm_ref(D.drop_piece(xd[:33], 2752 * 2 + 32 * 43 + 16), w, D.c_xsplit_blk()), resid[:M], dt), dt, "a dropped K piece")
    print(f"xsplit32_k<BLK> {dt} N={N}: slabs within {worst_slab:.3f} of their allowance, combined rows worst {worst:.3f} ulp beyond theirs")


# ------------------------------------------------------------------------------------------------------------------------------------------
# row blocks, fp8
# ------------------------------------------------------------------------------------------------------------------------------------------
def _windows(M):
    return [0, 8] if M == 40 else list(range(0, M, 32))


@pytest.mark.parametrize("epi", [0, 4])
def test_xstat_blk8_is_the_32_row_arithmetic_bit_for_bit(eng, epi):
    """README round 5: the fp8 row-block kernels are the 32-row arithmetic row by row. launch_rmsnorm into e4m3 blocks (ACT_BLK64_E4M3) + launch_xstat_blk8 at M = 40 (rows
    0-31 and 8-39), 96 and 128 (block by block) against rdx_gemm_test force 4 (rmsnorm4096_k into ACT_BLK64_E4M3 + xstat32_k<T, EPI, true, true>) on those 32
    rows. N = 8192, not the row-block minimum of 2048: the 32-row kernel it is compared with takes >= 512 tiles only (xstat32_supported)."""
    dt = eng.dt
    N = 8192
    x, nw = D.make_rows(128, K, dt, 41), D.make_norm_w(K, dt, 42)
    wd = D.make_w(N, K, dt, 43, std=0.03).to(eng.device)
    cols = N // 2 if epi == 4 else N
    for M in (40, 96, 128):
        out, _, xs, _ = eng.xstat_blk8_test(x[:M], nw, wd, epi=epi)
        assert _isnan(out[M:]) and bool(torch.isfinite(out[:M].float()).all())
        assert bool((xs[M:] == 1).all()), "xscale of pad rows"
        for a in _windows(M):
            ref32 = eng.gemm_test(x[a:a + 32], wd, None, None, epi, nw, EPS, 4)
            assert ref32.shape == (32, cols) and torch.equal(out[a:a + 32], ref32), f"M = {M}: rows {a}..{a + 31} differ from the 32-row kernel's"


@pytest.mark.parametrize("Kx,N", [(4096, 2048), (4096, 4096), (11008, 2048), (11008, 4096)])
def test_xsplit_blk8_is_the_32_row_arithmetic_bit_for_bit(eng, Kx, N):
    """launch_xsplit_blk8 (W8A16 K-split, 2 / 4 groups) [+ launch_rmsnorm into e4m3 blocks with the slabs] against rdx_gemm_test force 6 on every 32-row
    window: the slabs combined here in the kernels' fp32 order, and -- N = 4096 -- the rows the slab norm updated. Plus the fake-quantised fp64
    reference at the tolerance of test_fp8_x_fp8_gemm_matches_fake_quantised_fp32 (groups 0: the activations are not quantised)."""
    from test_gpu_gemm import _fake_quant_e4m3, _ref
    dt = eng.dt
    x = D.make_rows(128, Kx, dt, 51, scales=False)
    w = D.make_w(N, Kx, dt, 52, std=0.03)
    wd = w.to(eng.device)
    resid = D.make_rows(128, N, dt, 53, scales=False)
    nw = D.make_norm_w(N, dt, 54)
    G = 4 if Kx == 11008 else 2
    for M in (40, 96, 128):
        NB = (M + 31) // 32
        slab, r2 = eng.xsplit_blk8_test(x[:M], wd, resid=resid[:M] if N == 4096 else None, norm_w=nw if N == 4096 else None)
        slab = slab.cpu()
        assert slab.shape == (G, 32 * NB, N) and _isnan(slab[:, M:]), f"M = {M}: slab rows >= M were written"
        host = D.combine_slabs([slab[g, :M] for g in range(G)], resid[:M], dt)
        if N == 4096:
            assert torch.equal(r2.cpu(), host), f"M = {M}: the slab-folding norm's updated rows differ from x + T(sum of slabs)"
        for a in _windows(M):
            ref32 = eng.gemm_test(x[a:a + 32], wd, None, resid[a:a + 32], 3, None, EPS, 6).cpu()
            assert torch.equal(host[a:a + 32], ref32), f"M = {M}: rows {a}..{a + 31} differ from the 32-row K-split kernel's"
    ref = _ref(x, _fake_quant_e4m3(w), None, resid, 3, None, EPS, dt, wdt=torch.float32).float()
    tol = 2 * {torch.float16: 2e-3, torch.bfloat16: 1.6e-2}[dt] * max(1.0, float(ref.abs().max()))
    err = float((host.float() - ref).abs().max())
    assert err < tol, f"max abs err {err} (tol {tol})"


@pytest.mark.parametrize("N", [2048])
def test_xstat_blk8_matches_fake_quantised_fp64(eng, N):
    """The fp8 x fp8 row-block kernel against the fake-quantised reference (oracle.ref_cpu.fake_quant_e4m3 activations behind the norm, one scale
    per row; _fake_quant_e4m3 weights), tolerance of test_fp8_x_fp8_gemm_matches_fake_quantised_fp32 behind a norm, at the row-block minimum of
    128 tiles."""
    from test_gpu_gemm import _fake_quant_e4m3, _ref
    dt = eng.dt
    x, nw = D.make_rows(128, K, dt, 41), D.make_norm_w(K, dt, 42)
    w = D.make_w(N, K, dt, 44, std=0.03)
    wd = w.to(eng.device)
    ref = _ref(x, _fake_quant_e4m3(w), None, None, 0, nw, EPS, dt, wdt=torch.float32, act_groups=1).float()
    tol = max(2 * {torch.float16: 2e-3, torch.bfloat16: 1.6e-2}[dt], 1.25e-2) * max(1.0, float(ref.abs().max()))
    for M in (40, 96, 128):
        out, _, _, _ = eng.xstat_blk8_test(x[:M], nw, wd, epi=0)
        out = out.cpu()
        err = float((out[:M].float() - ref[:M]).abs().max())
        assert _isnan(out[M:]) and err < tol, f"M = {M}: max abs err {err} (tol {tol})"


def test_unsupported_shapes_are_errors(eng):
    """Every hook asks the production *_supported predicate first: a shape outside a family is an RdxError and nothing is launched (the NaN fill of
    the outputs is the wrapper's; the hooks return before any launch)."""
    from radialog_amd._lib import RdxError
    dt = eng.dt
    x, nw = D.make_rows(17, K, dt, 1), D.make_norm_w(K, dt, 2)
    w = D.make_w(8192, K, dt, 3)
    with pytest.raises(RdxError, match="xstat16_k"):
        eng.xstat16_test(x, nw, w)                                # 17 rows
    with pytest.raises(RdxError, match="xstat16_k"):
        eng.xstat16_test(x[:8], nw, w[:4096])                     # 256 tiles
    with pytest.raises(RdxError, match="xrow16_k"):
        eng.xrow16_test(x[:8, :480], w[:64, :480], x[:8, :64])    # K < 512
    with pytest.raises(RdxError, match="row-block"):
        eng.xstat_blk_test(x, nw, w[:1024])                       # 64 tiles
    with pytest.raises(RdxError, match="row-block"):
        eng.xsplit_blk_test(D.make_rows(20, 11008, dt, 4), D.make_w(2048, 11008, dt, 5))       # mtiles 2
    with pytest.raises(RdxError, match="fp8 row-block"):
        eng.xstat_blk8_test(x, nw, w[:2048])                      # 17 rows: mtiles 2
