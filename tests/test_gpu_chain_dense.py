"""The dense decode inside the coded chained launch (decode_chain_wc_k, csrc/chain.hip): per tile, one scalar choice between the raw loop, the general
coded decode and the dense one (no zero test; the tile's dense word, csrc/gemm.hip encode_wc_k) -- in the pre-decode ahead of the seam, the
unconditional first trip, the K loop and the tail of both roles. With the harness of tests/test_gpu_chain_predecode.py: one engine, option "wcode"
on / off / on, tokens and every step's logits torch.equal, eager and as a replayed graph, batch 1 and 2, 3 layers. The reference is the raw chained
kernel (decode_chain_k), which none of this touches.

    (512, 4, 1408):   a QKV wave's slice is exactly the pre-decoded chunk, the down_proj slices lie off the coded-chunk grid;
    (2560, 20, 4224): one chunk past the ring.

Once as generated (dense tiles exist: read back through rdx_wcode_dense_words), once with plants in layer 1's q_proj and down_proj: a 0.0 in row 5 makes
tile 0 -- the polling wave's tile -- general, a 1e-30 in row 21 makes tile 1 raw, the rest stay what they were: all three paths run in one QKV workgroup
and in the down_proj role."""
import pytest
import torch

from test_gpu_chain_predecode import _cfg, _on_equals_off

pytestmark = pytest.mark.gpu

UNIT_QKV, UNIT_DOWN = 0, 3
PLANTED = ("layers.1.mlp.down_proj.weight", "layers.1.self_attn.q_proj.weight")


def _engine(which, B, plant=False):
    from radialog_amd.engine import RdxEngine, synth_getter
    cfg = _cfg(which)
    eng = RdxEngine(cfg, dtype="bf16", device=0, max_batch=B, max_len=128, lora=True, vision=False)
    get = synth_getter(cfg, eng.device, lora=True)
    if plant:
        inner = get

        def get(name):
            t = inner(name)
            if any(name.endswith(s) for s in PLANTED):
                t = t.clone()
                t[5, 77] = 0.0             # tile 0: an index 0, still coded -> general
                t[21, 77] = 1e-30          # tile 1: 70 binades under its tile's largest weight -> raw
            return t
    eng.load_weights(get, vision=False)
    return cfg, eng


def _tiles(cfg, unit):
    L = cfg.llama
    return (3 * L.hidden + 2 * L.lora_r + 15) // 16 if unit == UNIT_QKV else L.hidden // 16


def _words(cfg, eng):
    """{unit: (hdr, dense)} of layer 1's fused QKV weight and down_proj."""
    return {u: eng.wcode_dense_words(u, 1, _tiles(cfg, u)) for u in (UNIT_QKV, UNIT_DOWN)}


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("which", ["exactly_pre", "one_past_ring"])
def test_dense_step_equals_raw_step_bitwise(which, B):
    cfg, eng = _engine(which, B)
    try:
        tiles, raw = eng.wcode_stats()[:2]
        dense = eng.wcode_dense_tiles()
        print(f"{which} B={B}: {dense} of {tiles} coded tiles dense, {raw} raw")
        assert raw == 0 and dense >= 0.9 * tiles               # the dense loops are what runs
        for u, (hdr, d) in _words(cfg, eng).items():
            assert not (hdr >> 8).any() and d.sum() >= 0.9 * d.size, u
        _on_equals_off(cfg, eng, B)
    finally:
        eng.close()


@pytest.fixture(scope="module")
def clean():
    """{width: ({unit: (hdr, dense)}, dense tiles)} of the engines as generated: what the plants are compared with."""
    out = {}
    for which in ("exactly_pre", "one_past_ring"):
        cfg, eng = _engine(which, 1)
        try:
            out[which] = (_words(cfg, eng), eng.wcode_dense_tiles())
        finally:
            eng.close()
    return out


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("which", ["exactly_pre", "one_past_ring"])
def test_dense_general_and_raw_tiles_in_one_workgroup(which, B, clean):
    clean_words, clean_total = clean[which]
    cfg, eng = _engine(which, B, plant=True)
    try:
        assert eng.wcode_stats()[1] == 2                       # tile 1 of either weight
        lost = 0
        for u, (hdr, d) in _words(cfg, eng).items():
            chdr, cd = clean_words[u]
            assert list(hdr[:3] >> 8) == [0, 1, 0] and list(d[:3]) == [0, 0, 1], u          # general, raw, dense: QKV workgroup 0 holds tiles 0..3
            assert (d[2:] == cd[2:]).all() and (hdr[2:] == chdr[2:]).all(), u
            lost += int(cd[0]) + int(cd[1])
        assert lost == 4 and eng.wcode_dense_tiles() == clean_total - lost
        _on_equals_off(cfg, eng, B)
    finally:
        eng.close()
