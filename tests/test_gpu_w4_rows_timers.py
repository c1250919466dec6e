"""The unit timers (rdx_time 1-5, RdxEngine.time_unit) launch what the step launches: the same builder per unit and the same choose-and-count helper
(api_dispatch.hip), so the launch counters see a timer's launches exactly as they see the step's. On the engine pair of tests/test_gpu_w4_rows_step.py
(int4 engine A, plain bf16 engine B on the dequantised weights; two layers), n timed iterations move

    3 rows, A, "w4" on:   gate/up and QKV  int4 xstat16 launches by n * layers     down_proj  int4 xrow16 launches by n * layers
                          o_proj and the lm_head: nothing (they stream the packed copy)          "w4" off: nothing at all
    1 row, A:             gate/up  int4 GEMV launches by n * layers
    1 row, B:             gate/up  coded GEMV launches by n * layers               QKV: nothing (layer 0's stand-alone QKV is raw)

Before the timers were rebuilt on the step's helpers, the 3-row int4 timers launched the bf16 kernels on the packed copy and the 1-row timers
launched without counting: every counter-moving line above failed."""
import pytest

from radialog_amd import synth
from test_gpu_w4_rows_step import N_NEW, T_PROMPT, pair  # noqa: F401  (the module-scoped engine pair)

pytestmark = pytest.mark.gpu

N_IT = 2
GATE_UP, QKV, O_PROJ, DOWN, LM_HEAD = 1, 2, 3, 4, 5


def _prefill_and_step(cfg, eng, B):
    ids = synth.synth_prompt_ids(B, T_PROMPT, vocab=cfg.llama.vocab, img_offset=6, pad_rows=False, seed=43)
    qf = synth.synth("t.w4rows.qf", (B, 32, cfg.llama.qformer_dim), -1.0, 1.0)
    _, _, n = eng.generate(ids, qf, max_new=N_NEW, eos_id=-1, use_graph=False)
    assert n == N_NEW


def _counters(eng):
    """(int4 xstat16, int4 xrow16, int4 GEMV, int4 chained, coded GEMV, coded chained) launches so far"""
    return eng.w4_rows_stats() + eng.w4_stats()[3:] + eng.wcode_stats()[3:]


def _moved(eng, unit):
    n0 = _counters(eng)
    assert eng.time_unit(unit, N_IT) > 0.0
    return tuple(b - a for a, b in zip(n0, _counters(eng)))


def test_timers_at_3_rows_launch_the_int4_kernels_of_the_step(pair):
    cfg, a, _ = pair
    nl = N_IT * cfg.llama.layers
    _prefill_and_step(cfg, a, 3)
    assert _moved(a, GATE_UP) == (nl, 0, 0, 0, 0, 0)
    assert _moved(a, QKV) == (nl, 0, 0, 0, 0, 0)
    assert _moved(a, DOWN) == (0, nl, 0, 0, 0, 0)
    assert _moved(a, O_PROJ) == (0,) * 6
    assert _moved(a, LM_HEAD) == (0,) * 6
    a.set_option("w4", 0)
    try:
        for unit in (GATE_UP, QKV, O_PROJ, DOWN, LM_HEAD):
            assert _moved(a, unit) == (0,) * 6, f"unit {unit} with the option off"
    finally:
        a.set_option("w4", 1)


def test_timers_at_1_row_count_the_streams_of_the_chained_family(pair):
    cfg, a, b = pair
    nl = N_IT * cfg.llama.layers
    _prefill_and_step(cfg, a, 1)
    assert _moved(a, GATE_UP) == (0, 0, nl, 0, 0, 0)
    _prefill_and_step(cfg, b, 1)
    assert _moved(b, GATE_UP) == (0, 0, 0, 0, nl, 0)
    assert _moved(b, QKV) == (0,) * 6
