"""launch_decode_attention (csrc/attn_body.h in its 16-, 8- and 4-wave stand-alone builds) and launch_rope_kv_prefill (csrc/attn.hip) alone, through
rdx_decode_attn_test / rdx_rope_kv_test, against the restatement of tests/_dec_attn.py (its docstring has the input grids, the hot positions and the derived
bar; tests/test_decode_attn_ref.py shows on the CPU that the restatement is exact on these inputs and that the bar sees a dropped or misplaced hot position).

Held bit for bit: the row appended to K (un-permuted) and V, every other byte of both caches, q and the cache rows of the prompt's write, a packed output
against the row-major one, and 0xff wherever nothing may be written. Held to the bar: the attention output, every element of every launch.
One exception to "bit for bit", found with these tests: where the restatement's RoPE gives -0 (both products are negative zeros: a zero "cos" or element times a
negative factor), the kernels may store +0. The compiler forms T(x cos) as v_fma_mixlo_f16 x, cos, 0, and (-0) + (+0) is +0; which elements of a lane's eight take
that instruction is the compiler's choice. The two zeros are the same number to everything that reads the cache (a product with either is a zero, and a sum's
value does not depend on the sign of a zero term), so the RoPE outputs (K rows, qout) are compared as numbers: every non-zero bit pattern identical, a zero
where the restatement has a zero. Everything else, the untouched cache rows included, is compared as bits.
heads = 2 throughout; the variant is the launcher's choice, by the option "att_tp" (RDX_ATT_TP in the whole-model tests)."""
import pytest
import torch

import _dec_attn as A
import _dec_gemm as G

pytestmark = pytest.mark.gpu

ROWS, BLK32, BLK64, TILES32 = range(4)                                # ActLayout
SLACK = 4096                                                          # bytes past a layout's extent that must stay 0xff
HEADS, H = 2, 256


@pytest.fixture(scope="module", params=["f16", "bf16"])
def eng(request):
    from radialog_amd.config import small_cfg
    from radialog_amd.engine import RdxEngine
    e = RdxEngine(small_cfg(), dtype=request.param, device=0, max_batch=1, max_len=32, llama=False, vision=False)
    e.dt = A.DT[request.param]
    yield e
    e.close()


def _variant(eng, variant):
    eng.set_option("att_tp", variant)                                    # the engine is shared: 0, the launcher's own choice, is set too


def _bits(t):
    return t.contiguous().view(torch.int16)


def _same(got, want, what, zero_sign=True):
    """Bit for bit, naming the first elements that differ. zero_sign False (only where a kernel's RoPE output is held against the restatement): a zero may
    have either sign -- see the module docstring."""
    a, b = _bits(got), _bits(want)
    if not zero_sign:
        z = (got == 0) & (want == 0)
        a, b = a.masked_fill(z, 0), b.masked_fill(z, 0)
    if not torch.equal(a, b):
        idx = (a != b).nonzero()
        first = [(tuple(i.tolist()), float(got[tuple(i)]), float(want[tuple(i)])) for i in idx[:6]]
        raise AssertionError(f"{what}: {idx.shape[0]} elements differ; (index, got, want): {first}")


def _launch(eng, case, k_perm, tables=False, kc_store=None, **kw):
    """One hook call on a case; the rope row comes from cur_rope or, tables, from cos / sin tables through pos (rows the launch does not use hold other values)."""
    B = case.B
    rope = {"cur_rope": torch.stack([case.cos, case.sin], 1)}
    if tables:
        pos = (torch.arange(B) * 3 + 2) % (B + 5)                         # distinct, unordered
        if len(set(pos.tolist())) != B:
            pos = torch.arange(B - 1, -1, -1) + 2
        cos_t, sin_t = (torch.full((int(pos.max()) + 4, 128), 0.75, dtype=case.dt) for _ in range(2))
        cos_t[pos.long()], sin_t[pos.long()] = case.cos, case.sin
        rope = {"cos": cos_t, "sin": sin_t, "pos": pos}
    return eng.decode_attn_test(case.x, A.k_permute(case.kc, k_perm) if kc_store is None else kc_store, case.vc, case.slot, case.mask, k_perm,
                                lbq=case.lbq, lbv=case.lbv, lora_scale=A.LORA_SCALE, **rope, **kw)


def _check(eng, case, r, res, k_perm, what):
    """The row-major output inside the bar everywhere; both caches = the inputs with the restatement's k' / v' at each row's slot, bit for bit. Returns the
    worst |out - ref| / bound."""
    err, out, kc2, vc2 = res
    assert err is None, f"{what}: {err}"
    out = out.cpu()
    assert bool((out[case.B * H * 2:] == 0xff).all()), f"{what}: bytes past the row-major output were written"
    o = out[:case.B * H * 2].view(eng.dt).reshape(case.B, H)
    m = A.ratio(o, r)
    assert m <= 1.0, f"{what}: output {m:.3g} x the bar (row, element {divmod(int(((o.double() - r['out']).abs() / r['bound']).argmax()), H)})"
    kc2, vc2, rows, idx = A.k_unpermute(kc2.cpu(), k_perm), vc2.cpu(), torch.arange(case.B), case.slot.long()
    _same(kc2[rows, :, idx], r["k"].to(eng.dt), f"{what}: the K row appended at the slot", zero_sign=False)
    _same(vc2[rows, :, idx], r["v"].to(eng.dt), f"{what}: the V row appended at the slot")
    kc2[rows, :, idx], vc2[rows, :, idx] = case.kc[rows, :, idx], case.vc[rows, :, idx]
    _same(kc2, case.kc, f"{what}: K cache away from the slot")
    _same(vc2, case.vc, f"{what}: V cache away from the slot")
    return m, o


@pytest.mark.parametrize("k_perm", [0, 1])
@pytest.mark.parametrize("variant", list(A.VARIANTS))
def test_contexts_on_either_side_of_every_boundary(eng, variant, k_perm):
    """_dec_attn.edge_groups: per launch the three contexts around one boundary (1 / 2 / 15 and 1535 at max_len 1536 included), per context the hot position
    last cached, first live, just inside the boundary and the new token; rows of different slots in one launch, one left-padded, one with its hot position
    masked out."""
    _variant(eng, variant)
    worst = 0.0
    for gi, group in enumerate(A.edge_groups(variant)):
        case = A.edge_case(eng.dt, group, 100 * variant + gi, lora=bool(gi & 1))
        r = case.ref()
        A.assert_hot(case, r)
        m, _ = _check(eng, case, r, _launch(eng, case, k_perm), k_perm, f"{A.VARIANTS[variant]}, k_perm {k_perm}, contexts {group}")
        worst = max(worst, m)
    print(f"decode attention edges {eng.dt} {A.VARIANTS[variant]} k_perm {k_perm}: worst {worst:.3f} x the bar")


@pytest.mark.parametrize("variant", list(A.VARIANTS))
def test_every_cached_position_is_the_hot_one_once(eng, variant):
    """One context per variant beyond the register window and into the second tail trip (1000, 700, 300): 16 pairs a launch, the hot positions 16 i .. 16 i + 15
    in launch i, no position left out. K in the order production pairs with the variant (fragment order with the 16-wave build)."""
    _variant(eng, variant)
    ctx, k_perm = A.SWEEP_CTX[variant], int(variant == 0)
    worst, seen = 0.0, set()
    for i in range(A.sweep_launches(ctx)):
        case = A.sweep_case(eng.dt, ctx, i, 7000 + variant)
        r = case.ref()
        A.assert_hot(case, r)
        m, _ = _check(eng, case, r, _launch(eng, case, k_perm), k_perm, f"{A.VARIANTS[variant]}, context {ctx}, hot positions {case.hot}")
        worst = max(worst, m)
        seen |= {p for row in case.hot for p in row}
    assert seen == set(range(ctx))
    print(f"decode attention sweep {eng.dt} {A.VARIANTS[variant]} context {ctx}: worst {worst:.3f} x the bar")


@pytest.mark.parametrize("variant", list(A.VARIANTS))
def test_in_place_append_with_and_without_lora_from_either_rope_source(eng, variant):
    """lora_r 0 and 8; the cos / sin row from cur_rope and from the tables through pos: the same bits either way, and the restatement's (_check: the slot row
    of K and V exact, every other byte of both caches unchanged)."""
    _variant(eng, variant)
    group = A.EDGES[variant][1]
    for lora in (False, True):
        for k_perm in (0, 1):
            case = A.edge_case(eng.dt, group, 300 + variant, lora=lora)
            r = case.ref()
            outs = []
            for tables in (False, True):
                res = _launch(eng, case, k_perm, tables=tables)
                outs.append(_check(eng, case, r, res, k_perm, f"{A.VARIANTS[variant]}, lora {lora}, k_perm {k_perm}, tables {tables}")[1])
            assert torch.equal(_bits(outs[0]), _bits(outs[1])), "cur_rope and tables + pos give different outputs"


def _unpack(layout, body, held, dt):
    body = body.view(dt)
    if layout in (BLK32, TILES32):
        return G.unpack_frag(body.reshape(H // 32, held // 16, 64, 8))
    return torch.cat([G.unpack_frag64(b) for b in body.reshape(held // 32, 32 * H)])


@pytest.mark.parametrize("variant", list(A.VARIANTS))
def test_packed_outputs_equal_the_row_major_one(eng, variant):
    """ACT_TILES32 (out_mt 3) and ACT_BLK64 (its second 32-row block) at 40 rows, ACT_BLK32 at 20: un-permuted with the helpers of _dec_gemm.py they are the
    row-major output bit for bit; rows the launch does not have and everything past the layout's extent stay 0xff."""
    _variant(eng, variant)
    for B, legs in ((40, ((TILES32, 3, 48), (BLK64, 0, 64))), (20, ((BLK32, 0, 32),))):
        slots = [1 + (7 * b) % 50 for b in range(B)]
        hot = [[(3 * b) % (slots[b] + 1), (5 * b + 1) % (slots[b] + 1)] for b in range(B)]
        case = A.make_case(eng.dt, HEADS, 64, slots, hot, 900 + B, lora=True)
        r = case.ref()
        k_perm = B & 1 ^ 1
        _, rows = _check(eng, case, r, _launch(eng, case, k_perm, out_bytes=B * H * 2 + SLACK), k_perm, f"{B} rows, row-major")
        for layout, mt, held in legs:
            what = f"{A.VARIANTS[variant]}, {B} rows, layout {layout}"
            err, out, kc2, vc2 = _launch(eng, case, k_perm, out_packed=layout, out_mt=mt, out_bytes=held * H * 2 + SLACK)
            assert err is None, f"{what}: {err}"
            out = out.cpu()
            assert bool((out[held * H * 2:] == 0xff).all()), f"{what}: bytes past the layout's extent were written"
            u = _unpack(layout, out[:held * H * 2], held, eng.dt)
            _same(u[:B], rows, f"{what}: against the row-major output")
            assert bool((u[B:].contiguous().view(torch.uint8) == 0xff).all()), f"{what}: rows the launch does not have were written"


def _prompt(eng, B, T, slot0, k_perm, lora, seed):
    """The prompt's write, then one decode step over the cache it wrote. Position ids are left-padded (row b repeats its first id pad_b times) and start at
    slot0; table rows of odd ids are invertible, and every pair's hot position is a prompt token with an odd id whose raw k is solved through the RoPE."""
    dt = eng.dt
    g = torch.Generator().manual_seed(seed)
    max_len = (slot0 + T + 1 + 31) // 32 * 32
    max_pos = slot0 + T + 3
    x = torch.zeros(B, T, A.qkv_ld(HEADS, lora))
    x[..., :3 * H] = A.grid(g, (B, T, 3 * H))
    lbq = lbv = None
    if lora:
        x[..., 3 * H:3 * H + 16] = A.grid(g, (B, T, 16), step=4)
        lbq, lbv = A.grid(g, (H, 8), step=4).to(dt), A.grid(g, (H, 8), step=4).to(dt)
    cos_t, sin_t = A.rope_rows(g, max_pos, (torch.arange(max_pos) & 1).bool())
    pads = [(5 * b) % 7 for b in range(B)]
    pos_ids = torch.stack([slot0 + (torch.arange(T) - pads[b]).clamp_min(0) for b in range(B)]).int()
    kc0 = A.grid(g, (B, HEADS, max_len, 128)).to(dt)
    vc0 = (torch.rand(B, HEADS, max_len, 128, generator=g) * 1.98 - 0.99).to(dt)
    # the decode step's case over the cache the prompt will leave; its hot rows are then put into the prompt
    _, k, v = A.prefill_ref(x.to(dt), HEADS, dt, torch.float64, cos_t.to(dt), sin_t.to(dt), pos_ids, lbq, lbv)
    kc, vc = kc0.clone(), vc0.clone()
    kc[:, :, slot0:slot0 + T], vc[:, :, slot0:slot0 + T] = k.to(dt), v.to(dt)
    hot = []
    for b in range(B):
        cand = [slot0 + T - 1, slot0 + pads[b] + 1 + b]
        hot.append([p if int(pos_ids[b, p - slot0]) & 1 else p - 1 for p in cand])
    case = A.make_case(dt, HEADS, max_len, [slot0 + T] * B, hot, seed + 1, lora=lora, kc=kc, vc=vc)
    for b in range(B):
        for h in range(HEADS):
            t = hot[b][h] - slot0
            pid = int(pos_ids[b, t])
            assert pid & 1
            x[b, t, H + 128 * h:H + 128 * (h + 1)] = A.solve_rope(case.kc[b, h, hot[b][h]].double(), cos_t[pid].double(), sin_t[pid].double()).float()
    xT = x.to(dt)
    assert torch.equal(xT.float(), x)
    q, k, v = A.prefill_ref(xT, HEADS, dt, torch.float64, cos_t.to(dt), sin_t.to(dt), pos_ids, lbq, lbv)
    assert torch.equal(k.to(dt), case.kc[:, :, slot0:slot0 + T]), "the hot rows did not come back through the RoPE"
    case.kc[:, :, slot0:slot0 + T] = k.to(dt)                                # the same values; a zero may have changed its sign on the way
    what = f"prompt {B} x {T} at slot {slot0}, k_perm {k_perm}, lora {lora}"
    err, qout, kc2, vc2 = eng.rope_kv_test(xT, pos_ids, cos_t.to(dt), sin_t.to(dt), slot0, A.k_permute(kc0, k_perm), vc0, k_perm, lbq, lbv, A.LORA_SCALE)
    assert err is None, f"{what}: {err}"
    _same(qout.cpu(), q.to(dt), f"{what}: qout", zero_sign=False)
    ku, new = A.k_unpermute(kc2.cpu(), k_perm), slice(slot0, slot0 + T)
    _same(ku[:, :, new], case.kc[:, :, new], f"{what}: K rows [slot0, slot0 + T)", zero_sign=False)
    ku[:, :, new] = case.kc[:, :, new]
    _same(ku, case.kc, f"{what}: K rows outside [slot0, slot0 + T)")
    _same(vc2.cpu(), case.vc, f"{what}: V cache (rows [slot0, slot0 + T) = v', every other row unchanged)")
    case.kc = A.k_unpermute(kc2.cpu(), k_perm).clone()                       # the cache as the kernel left it (the same numbers; a zero may differ in sign)
    r = case.ref()
    A.assert_hot(case, r)
    return _check(eng, case, r, _launch(eng, case, k_perm, kc_store=kc2), k_perm, what + ", decode step")[0]


@pytest.mark.parametrize("k_perm", [0, 1])
def test_prompt_write_then_a_decode_step(eng, k_perm):
    """rdx_rope_kv_test below 2048 tokens (one token per workgroup) and above (tpb = 5 at 3 x 701: T is no multiple of it), from slot 0 and appended behind 19
    cached rows: qout and the written rows exact, every other cache byte untouched; then decode attention over the cache the kernel wrote."""
    _variant(eng, 0)
    worst = 0.0
    for B, T, slot0, lora in ((2, 37, 0, True), (2, 37, 19, False), (3, 701, 0, False), (3, 701, 19, True)):
        worst = max(worst, _prompt(eng, B, T, slot0, k_perm, lora, 40 + T + slot0))
    print(f"prompt write + decode step {eng.dt} k_perm {k_perm}: worst {worst:.3f} x the bar")


def test_refusals_leave_everything_untouched(eng):
    """Every item of the two refusal lists: an error, output all 0xff, caches bit for bit the input."""
    _variant(eng, 0)
    dt = eng.dt

    def refused(case, what, **kw):
        err, out, kc2, vc2 = _launch(eng, case, 1, **kw)
        assert err is not None, f"{what}: not refused"
        assert bool((out.cpu() == 0xff).all()), f"{what}: a refused launch wrote its output"
        assert torch.equal(_bits(kc2.cpu()), _bits(A.k_permute(case.kc))) and torch.equal(_bits(vc2.cpu()), _bits(case.vc)), f"{what}: a refused launch changed a cache"

    def base(B=2, max_len=64):
        return A.make_case(dt, HEADS, max_len, [9 + b % 7 for b in range(B)], [[3, 5]] * B, 1, lora=True)
    assert _launch(eng, base(), 1)[0] is None
    for ml in (48, 1568):
        c = base()
        c.max_len, c.kc, c.vc, c.mask = ml, torch.zeros(2, HEADS, ml, 128, dtype=dt), torch.zeros(2, HEADS, ml, 128, dtype=dt), torch.ones(2, ml, dtype=torch.uint8)
        refused(c, f"max_len {ml}")
    for s in (0, 64, -1):
        c = base()
        c.slot[1] = s
        refused(c, f"slot {s}")
    c = base()
    c.mask[1, int(c.slot[1])] = 0
    refused(c, "zero mask byte at the row's own slot")
    refused(base(33), "33 rows into a 32-row block", out_packed=BLK32, out_bytes=64 * H * 2)
    refused(base(40), "40 rows into two row tiles", out_packed=TILES32, out_mt=2, out_bytes=64 * H * 2)
    refused(base(), "layout 4", out_packed=4, out_bytes=64 * H * 2)
    # a position outside the tables
    c = base()
    err, out, kc2, vc2 = eng.decode_attn_test(c.x, A.k_permute(c.kc), c.vc, c.slot, c.mask, 1, cos=torch.zeros(4, 128, dtype=dt), sin=torch.zeros(4, 128, dtype=dt),
                                              pos=torch.tensor([1, 4]), lbq=c.lbq, lbv=c.lbv, lora_scale=A.LORA_SCALE)
    assert err is not None and bool((out.cpu() == 0xff).all()) and torch.equal(_bits(kc2.cpu()), _bits(A.k_permute(c.kc))) and torch.equal(_bits(vc2.cpu()), _bits(c.vc))

    # the prompt's write
    g = torch.Generator().manual_seed(3)
    x = A.grid(g, (2, 5, A.qkv_ld(HEADS, False))).to(dt)
    kc0, vc0 = A.grid(g, (2, HEADS, 32, 128)).to(dt), A.grid(g, (2, HEADS, 32, 128)).to(dt)
    cos, sin = (t.to(dt) for t in A.rope_rows(g, 8, [False] * 8))
    ok_pos = torch.arange(5).repeat(2, 1)
    assert eng.rope_kv_test(x, ok_pos, cos, sin, 27, kc0, vc0, 0)[0] is None
    bad = ok_pos.clone()
    bad[1, 3] = 8
    neg = ok_pos.clone()
    neg[0, 0] = -1
    for what, pos, slot0 in (("slot0 + T > max_len", ok_pos, 28), ("slot0 < 0", ok_pos, -1), ("position id = max_pos", bad, 0), ("negative position id", neg, 0)):
        err, qout, kc2, vc2 = eng.rope_kv_test(x, pos, cos, sin, slot0, kc0, vc0, 0)
        assert err is not None, f"{what}: not refused"
        assert bool((qout.cpu().contiguous().view(torch.uint8) == 0xff).all()), f"{what}: a refused launch wrote qout"
        assert torch.equal(_bits(kc2.cpu()), _bits(kc0)) and torch.equal(_bits(vc2.cpu()), _bits(vc0)), f"{what}: a refused launch changed a cache"
