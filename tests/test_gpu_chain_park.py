"""The QKV role of the coded chained launch (decode_chain_wc_k, csrc/chain.hip) decodes the first chunks of a wave's ring into a wave-private LDS region
ahead of the hand-off (chain_tile PARK), refills those ring slots behind the activation row loads and takes the parked fragments from LDS in its first
trip; the role's `red` lies over the park region. With the harness of tests/test_gpu_chain_predecode.py -- one engine, option "wcode" on / off / on,
tokens and every step's logits torch.equal, eager and as a replayed graph, batch 1 and 2, 3 layers, the launch counts of rdx_wcode_stats -- on the
widths at which the parked path takes its other branches (a QKV wave's slice is hidden / 512 coded chunks; 512, 1536 and 2560 run in that file):

    (1024,  8, 1408): 2 chunks: at most what is decoded ahead; every refill is a clamped duplicate, whose fragments multiply the zero line;
    (2048, 16, 2816): 4 chunks = the ring: decoded chunks plus the rest of the ring, no K-loop trip;
    (3072, 24, 1408): 6 chunks: a slot refilled behind the row loads is consumed by the tail;
    (4096, 32, 1408): 8 chunks: the production slice and the production LDS size; batch 2 is the largest LDS request the launch makes.

Two more at (2048, 16, 2816), with plants in rows 5 and 21 of layer 1's q_proj (tiles 0 and 1 of QKV workgroup 0; tile 0 is the polling wave's): exact
zeros make the two tiles general next to dense tiles of the same workgroup; out-of-window weights make them raw -- they park nothing and stream their
packed bytes through the ring's registers. The reference is the raw chained kernel (decode_chain_k), which none of this touches."""
import pytest
import torch

from radialog_amd.config import LlamaCfg, RaDialogCfg
from test_gpu_chain_predecode import _on_equals_off

pytestmark = pytest.mark.gpu

UNIT_QKV = 0
WIDTHS = {"two_chunks": (1024, 8, 1408), "ring": (2048, 16, 2816), "six_chunks": (3072, 24, 1408), "production_slice": (4096, 32, 1408)}
Q_PROJ = "layers.1.self_attn.q_proj.weight"


def _cfg(which):
    hidden, heads, inter = WIDTHS[which]
    return RaDialogCfg(llama=LlamaCfg(vocab=8001, hidden=hidden, inter=inter, layers=3, heads=heads, qformer_dim=192))


def _engine(which, B, plant=None):
    from radialog_amd.engine import RdxEngine, synth_getter
    cfg = _cfg(which)
    assert cfg.llama.head_dim == 128
    eng = RdxEngine(cfg, dtype="bf16", device=0, max_batch=B, max_len=128, lora=True, vision=False)
    get = synth_getter(cfg, eng.device, lora=True)
    if plant is not None:
        inner = get

        def get(name):
            t = inner(name)
            if name.endswith(Q_PROJ):
                t = t.clone()
                t[5, 77] = plant           # tile 0
                t[21, 77] = plant          # tile 1
            return t
    eng.load_weights(get, vision=False)
    return cfg, eng


def _qkv_words(cfg, eng):
    L = cfg.llama
    return eng.wcode_dense_words(UNIT_QKV, 1, (3 * L.hidden + 2 * L.lora_r + 15) // 16)


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("which", sorted(WIDTHS))
def test_parked_step_equals_raw_step_bitwise(which, B):
    cfg, eng = _engine(which, B)
    try:
        assert eng.wcode_stats()[0] > 0 and eng.wcode_stats()[1] == 0           # coded copies exist, no tile falls back on the synthetic weights
        _on_equals_off(cfg, eng, B)
        assert eng.time_unit(7, 1) > 0.0         # the chained family is the one that ran
    finally:
        eng.close()


@pytest.mark.parametrize("B", [1, 2])
def test_general_tiles_park_next_to_dense_ones(B):
    cfg, eng = _engine("ring", B, plant=0.0)
    try:
        assert eng.wcode_stats()[1] == 0
        hdr, d = _qkv_words(cfg, eng)
        print(f"B={B}: header words {list(hdr[:4])}, dense words {list(d[:4])}")
        assert not (hdr[:4] >> 8).any() and list(d[:2]) == [0, 0] and d[2:4].any()      # QKV workgroup 0: general, general, and a dense tile
        _on_equals_off(cfg, eng, B)
    finally:
        eng.close()


@pytest.mark.parametrize("B", [1, 2])
def test_raw_tiles_park_nothing(B):
    cfg, eng = _engine("ring", B, plant=1e-30)      # 70 binades under its tile's largest weight: outside the window
    try:
        assert eng.wcode_stats()[1] == 2
        hdr, _ = _qkv_words(cfg, eng)
        assert list(hdr[:4] >> 8) == [1, 1, 0, 0]                               # the polling wave's tile and its neighbour stream raw
        _on_equals_off(cfg, eng, B)
    finally:
        eng.close()
