"""launch_decode_attention_kv8 (csrc/attn_body.h KV8 in its 16-, 8- and 4-wave stand-alone builds: decode attention on the fp8 KV cache, radialog_amd/kv8.py)
alone, through rdx_decode_attn_kv8_test, on the inputs of tests/_kv8.py (the cases of tests/_dec_attn.py on caches whose exponents change with the
position, the head and the row; tests/test_kv8_host.py asserts that on the CPU).

Per launch:
  (a) the output equals, BIT FOR BIT, what the existing build of the same variant (rdx_decode_attn_test) gives on model-dtype caches holding the stored values;
  (b) the output is inside _dec_attn's derived bar against the fp64 restatement;
  (c) the code row and the exponent appended at each row's slot are kv8.quant of the restatement's k' / v', byte for byte -- for K a zero code may have
      either sign, as tests/test_gpu_decode_attn.py allows for the zeros of the kernels' RoPE;
  (d) every other code and exponent byte is unchanged;
  (e) 0xff guard bytes behind the output, both code buffers and both exponent buffers hold.
heads = 2; the variant is the launcher's choice, by the option "att_tp" (RDX_ATT_TP in the whole-model tests). The kv8 builds keep their twins' row sweeps and register windows,
so the boundaries are _dec_attn.EDGES."""
import pytest
import torch

import _dec_attn as A
import _dec_gemm as G
import _kv8 as K8
from radialog_amd import kv8

pytestmark = pytest.mark.gpu

ROWS, BLK32, BLK64, TILES32 = range(4)
GUARD = 4096
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


def _rope(case, tables):
    if not tables:
        return {"cur_rope": torch.stack([case.cos, case.sin], 1)}
    B = case.B
    pos = (torch.arange(B) * 3 + 2) % (B + 5)
    if len(set(pos.tolist())) != B:
        pos = torch.arange(B - 1, -1, -1) + 2
    cos_t, sin_t = (torch.full((int(pos.max()) + 4, 128), 0.75, dtype=case.dt) for _ in range(2))
    cos_t[pos.long()], sin_t[pos.long()] = case.cos, case.sin
    return {"cos": cos_t, "sin": sin_t, "pos": pos}


def _pair(eng, case, k_perm, tables=False, **kw):
    """The kv8 launch and its model-dtype twin on the same case. Returns (kv8 result, twin result, the stored caches)."""
    st = K8.stored(case)
    K8.exponents_vary(case, st[1], st[3])
    args = dict(lbq=case.lbq, lbv=case.lbv, lora_scale=A.LORA_SCALE, **_rope(case, tables), **kw)
    r8 = eng.decode_attn_kv8_test(case.x, kv8.k_store(st[0]), st[1], st[2], st[3], case.slot, case.mask, guard=GUARD, **args)
    rt = eng.decode_attn_test(case.x, A.k_permute(case.kc, k_perm), case.vc, case.slot, case.mask, k_perm, **args)
    return r8, rt, st


def _zero_code(c):
    return (c & 0x7f) == 0


def _check(eng, case, r, res, what, out_bytes=None):
    """(a) .. (e) of the module docstring on one pair of launches with a row-major output. Returns the worst |out - ref| / bound."""
    (err, out, kc2, ke2, vc2, ve2), (errt, outt, _, _), (kc0, ke0, vc0, ve0) = res
    assert err is None and errt is None, f"{what}: {err} / {errt}"
    B, n = case.B, case.B * H * 2
    out, outt = out.cpu(), outt.cpu()
    assert torch.equal(out[:n], outt[:n]), f"{what}: (a) {int((out[:n] != outt[:n]).sum())} output bytes differ from the model-dtype build's on the stored values"
    assert bool((out[n:] == 0xff).all()), f"{what}: (e) bytes past the output were written"
    o = out[:n].view(eng.dt).reshape(B, H)
    m = A.ratio(o, r)
    assert m <= 1.0, f"{what}: (b) output {m:.3g} x the bar"
    nc, ne = kc0.numel(), ke0.numel()
    for name, buf, size in (("K codes", kc2, nc), ("K exponents", ke2, ne), ("V codes", vc2, nc), ("V exponents", ve2, ne)):
        assert bool((buf.cpu()[size:] == 0xff).all()), f"{what}: (e) guard bytes behind the {name} were written"
    kc2 = kv8.k_logical(kc2.cpu()[:nc].reshape(kc0.shape))
    vc2 = vc2.cpu()[:nc].reshape(vc0.shape)
    ke2, ve2 = ke2.cpu()[:ne].view(torch.int8).reshape(ke0.shape), ve2.cpu()[:ne].view(torch.int8).reshape(ve0.shape)
    rows, idx = torch.arange(B), case.slot.long()
    kq, vq = kv8.quant(r["k"].to(eng.dt)), kv8.quant(r["v"].to(eng.dt))
    got_k, got_v = kc2[rows, :, idx], vc2[rows, :, idx]
    kdiff = (got_k != kq[0]) & ~(_zero_code(got_k) & _zero_code(kq[0]))
    assert not bool(kdiff.any()), f"{what}: (c) {int(kdiff.sum())} codes of the appended K rows differ from kv8.quant(k')"
    assert torch.equal(got_v, vq[0]), f"{what}: (c) {int((got_v != vq[0]).sum())} codes of the appended V rows differ from kv8.quant(v')"
    assert torch.equal(ke2[rows, :, idx], kq[1]) and torch.equal(ve2[rows, :, idx], vq[1]), f"{what}: (c) the appended exponents differ from kv8.quant's"
    kc2[rows, :, idx], vc2[rows, :, idx], ke2[rows, :, idx], ve2[rows, :, idx] = kc0[rows, :, idx], vc0[rows, :, idx], ke0[rows, :, idx], ve0[rows, :, idx]
    assert torch.equal(kc2, kc0) and torch.equal(vc2, vc0), f"{what}: (d) code bytes away from the slot changed"
    assert torch.equal(ke2, ke0) and torch.equal(ve2, ve0), f"{what}: (d) exponents away from the slot changed"
    return m, o


@pytest.mark.parametrize("variant", list(A.VARIANTS))
def test_contexts_on_either_side_of_every_boundary(eng, variant):
    """_dec_attn.edge_groups (1 / 2 / 15, 15 / 16 / 17, the variant's row sweep, half window, window and tail trips, 1535 at max_len 1536): rows of different
    slots in one launch, one left-padded, one with its hot position masked out; LoRA on in every other launch."""
    _variant(eng, variant)
    worst = 0.0
    for gi, group in enumerate(A.edge_groups(variant)):
        case = K8.edge_case(eng.dt, group, 100 * variant + gi, lora=bool(gi & 1))
        r = case.ref()
        A.assert_hot(case, r)
        m, _ = _check(eng, case, r, _pair(eng, case, int(variant == 0)), f"{A.VARIANTS[variant]}, contexts {group}")
        worst = max(worst, m)
    print(f"kv8 decode attention edges {eng.dt} {A.VARIANTS[variant]}: worst {worst:.3f} x the bar")


@pytest.mark.parametrize("variant", list(A.VARIANTS))
def test_every_cached_position_is_the_hot_one_once(eng, variant):
    """One context per variant beyond the register window and into the second tail trip (1000, 700, 300): the hot positions 16 i .. 16 i + 15 in launch i."""
    _variant(eng, variant)
    ctx = A.SWEEP_CTX[variant]
    worst, seen = 0.0, set()
    for i in range(A.sweep_launches(ctx)):
        case = K8.sweep_case(eng.dt, ctx, i, 7100 + variant)
        r = case.ref()
        A.assert_hot(case, r)
        m, _ = _check(eng, case, r, _pair(eng, case, int(variant == 0)), f"{A.VARIANTS[variant]}, context {ctx}, hot positions {case.hot}")
        worst = max(worst, m)
        seen |= {p for row in case.hot for p in row}
    assert seen == set(range(ctx))
    print(f"kv8 decode attention sweep {eng.dt} {A.VARIANTS[variant]} context {ctx}: worst {worst:.3f} x the bar")


@pytest.mark.parametrize("variant", list(A.VARIANTS))
def test_append_with_and_without_lora_from_either_rope_source(eng, variant):
    """lora_r 0 and 8; the cos / sin row from cur_rope and from the tables through pos: the same bits either way."""
    _variant(eng, variant)
    group = A.EDGES[variant][1]
    for lora in (False, True):
        case = K8.edge_case(eng.dt, group, 300 + variant, lora=lora)
        r = case.ref()
        outs = [_check(eng, case, r, _pair(eng, case, 0, tables=tables), f"{A.VARIANTS[variant]}, lora {lora}, tables {tables}")[1] for tables in (False, True)]
        assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16)), "cur_rope and tables + pos give different outputs"


@pytest.mark.parametrize("variant", list(A.VARIANTS))
def test_packed_outputs_equal_the_row_major_one(eng, variant):
    """ACT_TILES32 (out_mt 3) and ACT_BLK64 (its second 32-row block) at 40 rows, ACT_BLK32 at 20 rows: the shared output stage. Un-permuted they are the
    row-major output bit for bit; rows the launch does not have and everything past the layout's extent stay 0xff."""
    _variant(eng, variant)
    for B, legs in ((40, ((TILES32, 3, 48), (BLK64, 0, 64))), (20, ((BLK32, 0, 32),))):
        case = K8.packed_case(eng.dt, B, 900 + B)
        r = case.ref()
        _, rows = _check(eng, case, r, _pair(eng, case, B & 1 ^ 1, out_bytes=B * H * 2 + GUARD), f"{B} rows, row-major")
        st = K8.stored(case)
        for layout, mt, held in legs:
            what = f"{A.VARIANTS[variant]}, {B} rows, layout {layout}"
            err, out = eng.decode_attn_kv8_test(case.x, kv8.k_store(st[0]), st[1], st[2], st[3], case.slot, case.mask, lbq=case.lbq, lbv=case.lbv,
                                                lora_scale=A.LORA_SCALE, cur_rope=torch.stack([case.cos, case.sin], 1), out_packed=layout, out_mt=mt,
                                                out_bytes=held * H * 2 + GUARD)[:2]
            assert err is None, f"{what}: {err}"
            out = out.cpu()
            assert bool((out[held * H * 2:] == 0xff).all()), f"{what}: bytes past the layout's extent were written"
            body = out[:held * H * 2].view(eng.dt)
            u = G.unpack_frag(body.reshape(H // 32, held // 16, 64, 8)) if layout in (BLK32, TILES32) else torch.cat([G.unpack_frag64(b) for b in body.reshape(held // 32, 32 * H)])
            assert torch.equal(u[:B].contiguous().view(torch.int16), rows.contiguous().view(torch.int16)), f"{what}: differs from the row-major output"
            assert bool((u[B:].contiguous().view(torch.uint8) == 0xff).all()), f"{what}: rows the launch does not have were written"


def test_refusals_leave_everything_untouched(eng):
    """The refusal list of rdx_decode_attn_test holds for the kv8 hook: an error, output all 0xff, codes and exponents the input bytes."""
    _variant(eng, 0)
    case = K8.packed_case(eng.dt, 2, 5)
    st = K8.stored(case)

    def call(slot=None, mask=None, **kw):
        return eng.decode_attn_kv8_test(case.x, kv8.k_store(st[0]), st[1], st[2], st[3], case.slot if slot is None else slot, case.mask if mask is None else mask,
                                        lbq=case.lbq, lbv=case.lbv, lora_scale=A.LORA_SCALE, cur_rope=torch.stack([case.cos, case.sin], 1), **kw)
    assert call()[0] is None
    bad_slot, bad_mask = case.slot.clone(), case.mask.clone()
    bad_slot[1] = 64
    bad_mask[1, int(case.slot[1])] = 0
    for what, kw in (("slot = max_len", dict(slot=bad_slot)), ("zero mask byte at the row's own slot", dict(mask=bad_mask)),
                     ("layout 4", dict(out_packed=4, out_bytes=64 * H * 2)), ("2 row tiles for 40 rows", dict(out_packed=TILES32, out_mt=0, out_bytes=64 * H * 2))):
        err, out, kc2, ke2, vc2, ve2 = call(**kw)
        assert err is not None and "rdx_decode_attn_kv8_test" in err, f"{what}: not refused"
        assert bool((out.cpu() == 0xff).all()), f"{what}: a refused launch wrote its output"
        assert torch.equal(kc2.cpu(), kv8.k_store(st[0]).reshape(-1)) and torch.equal(vc2.cpu(), st[2].reshape(-1)), f"{what}: a refused launch changed the codes"
        assert torch.equal(ke2.cpu().view(torch.int8), st[1].reshape(-1)) and torch.equal(ve2.cpu().view(torch.int8), st[3].reshape(-1)), f"{what}: a refused launch changed the exponents"
