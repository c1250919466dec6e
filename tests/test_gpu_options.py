"""The runtime switches (csrc/api_options.hip: one table): every switch's environment variable is read once, at rdx_create, into the context; after that only
rdx_set_option changes it, per context; rdx_get_option / rdx_option_name say what is in force. Held here: the defaults, the environment at create (a second
engine of the same process sees a changed variable, a live engine does not), the round trip, the refusals (which change nothing), the before-finalize rows,
the letters of RDX_WS_CFG, and that the table of INTEGRATION.md lists exactly what the library enumerates. No kernel is launched: that a switch still selects
what it selected is held by the tests that use each one (the golden-bit cases, the A/B parity legs, the attention variants, the wsgemm tile shapes)."""
import os

import pytest

from radialog_amd.config import small_cfg

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# option -> (environment variable or None, default): today's values, kept
TABLE = {
    "fuse_ao": ("RDX_FUSE_AO", 1), "chain": ("RDX_CHAIN", 1), "flash_min": ("RDX_FLASH_MIN", 512), "xs16": ("RDX_XS16", 1), "prompt_blk": ("RDX_PBLK", 1),
    "blk_down": ("RDX_BLK_DOWN", 1), "pconv": ("RDX_PCONV", 1), "pconv_ksplit": ("RDX_PCONV_KSPLIT", 1), "kperm": ("RDX_KPERM", -1), "wcode": (None, 1),
    "w4": (None, 1), "kv_fp8": (None, 0), "score_chunk": (None, 2048), "att_tp": ("RDX_ATT_TP", 0), "att_mid": ("RDX_ATT_MID", 1), "xdup": ("RDX_XDUP", 1),
    "ws_cfg": ("RDX_WS_CFG", 0), "beam_fullcopy": ("RDX_BEAM_FULLCOPY", 0), "eos_poll": ("RDX_EOS_POLL", 4),
}
BOOLS = {"fuse_ao", "chain", "xs16", "prompt_blk", "blk_down", "pconv", "pconv_ksplit", "wcode", "w4", "kv_fp8", "att_mid", "xdup", "beam_fullcopy"}
# two settings of every variable, neither the default where the switch has more than two values: (text, the value it means)
ENV_A = {n: (str(1 - d), 1 - d) for n, (e, d) in TABLE.items() if e and n in BOOLS}
ENV_A.update(flash_min=("7", 7), kperm=("0", 0), att_tp=("1", 1), ws_cfg=("C", 3), eos_poll=("16", 16))
ENV_B = {n: (str(d), d) for n, (e, d) in TABLE.items() if e and n in BOOLS}
ENV_B.update(flash_min=("9", 9), kperm=("1", 1), att_tp=("2", 2), ws_cfg=("5", 5), eos_poll=("1", 1))
# (option, a value outside its range): the bools store value != 0 and have none
OUT_OF_RANGE = [("kperm", -2), ("kperm", 2), ("score_chunk", -1), ("att_tp", -1), ("att_tp", 3), ("ws_cfg", -1), ("ws_cfg", 6)]
BEFORE_FINALIZE = {"kperm": 0, "kv_fp8": 1}


def _bare():
    """The kernel-free engine of the decode-attention tests."""
    from radialog_amd.engine import RdxEngine
    return RdxEngine(small_cfg(), dtype="bf16", device=0, max_batch=1, max_len=32, llama=False, vision=False)


def _setenv(monkeypatch, which):
    for name, (text, _) in which.items():
        monkeypatch.setenv(TABLE[name][0], text)


@pytest.fixture
def clean_env(monkeypatch):
    for env, _ in TABLE.values():
        if env:
            monkeypatch.delenv(env, raising=False)
    return monkeypatch


@pytest.fixture
def eng(clean_env):
    e = _bare()
    yield e
    e.close()


def _values(e):
    return {n: e.get_option(n) for n in e.option_names()}


def test_defaults(eng):
    assert eng.option_names() == list(TABLE)
    assert _values(eng) == {n: d for n, (_, d) in TABLE.items()}


def test_the_environment_is_read_at_create_and_only_there(clean_env):
    assert set(ENV_A) == set(ENV_B) == {n for n, (e, _) in TABLE.items() if e}
    want0 = {n: d for n, (_, d) in TABLE.items()}
    want_a, want_b = dict(want0, **{n: v for n, (_, v) in ENV_A.items()}), dict(want0, **{n: v for n, (_, v) in ENV_B.items()})
    assert all(want_a[n] != want_b[n] for n in ENV_A) and all(want_a[n] != want0[n] for n in ENV_A)
    _setenv(clean_env, ENV_A)
    first = _bare()
    try:
        assert _values(first) == want_a
        _setenv(clean_env, ENV_B)
        assert _values(first) == want_a, "a live engine followed the environment"
        second = _bare()
        try:
            assert _values(second) == want_b, "a second engine of the process did not see the changed environment"
            assert _values(first) == want_a
        finally:
            second.close()
    finally:
        first.close()


def test_ws_cfg_letters(clean_env):
    for text, want in (("A", 1), ("C", 3), ("E", 5), ("3", 3)):
        clean_env.setenv("RDX_WS_CFG", text)
        e = _bare()
        try:
            assert e.get_option("ws_cfg") == want
        finally:
            e.close()


def test_an_environment_value_out_of_range_fails_the_create(clean_env):
    from radialog_amd._lib import RdxError
    clean_env.setenv("RDX_ATT_TP", "3")
    with pytest.raises(RdxError, match="RDX_ATT_TP"):
        _bare()


def test_round_trip_and_refusals(eng):
    from radialog_amd._lib import RdxError
    for name, (_, d) in TABLE.items():
        for v in ((1 - d, d) if name in BOOLS else {"flash_min": (0, 1, d), "kperm": (0, 1, d), "score_chunk": (0, 64, d), "att_tp": (1, 2, d),
                                                   "ws_cfg": (1, 5, d), "eos_poll": (1, 16, d)}[name]):
            eng.set_option(name, v)
            assert eng.get_option(name) == v, name
    eng.set_option("xs16", 7)
    assert eng.get_option("xs16") == 1                                    # a bool stores value != 0
    before = _values(eng)
    for name, v in OUT_OF_RANGE:
        with pytest.raises(RdxError, match=name):
            eng.set_option(name, v)
    with pytest.raises(RdxError, match="score_chunk -1 is negative"):
        eng.set_option("score_chunk", -1)
    with pytest.raises(RdxError, match="unknown option 'no_such_switch'"):
        eng.set_option("no_such_switch", 1)
    with pytest.raises(RdxError, match="unknown option 'no_such_switch'"):
        eng.get_option("no_such_switch")
    assert _values(eng) == before, "a refused call changed a value"


def test_before_finalize_rows_are_refused_after_load_weights(clean_env):
    from radialog_amd._lib import RdxError
    from radialog_amd.engine import RdxEngine, synth_getter
    cfg = small_cfg()
    e = RdxEngine(cfg, dtype="bf16", device=0, max_batch=2, max_len=64, lora=True, vision=False)
    try:
        for name, v in BEFORE_FINALIZE.items():                          # before: settable, and back
            e.set_option(name, v)
            assert e.get_option(name) == v
            e.set_option(name, TABLE[name][1])
        e.load_weights(synth_getter(cfg, e.device, lora=True), vision=False)
        before = _values(e)
        for name, v in BEFORE_FINALIZE.items():
            with pytest.raises(RdxError, match=f"{name} decides what rdx_finalize_weights allocates; set it before that call"):
                e.set_option(name, v)
        assert _values(e) == before
        e.set_option("att_tp", 2)                                        # the any-time rows stay settable
        assert e.get_option("att_tp") == 2
    finally:
        e.close()


def test_the_documented_table_is_the_library_table(eng):
    text = open(os.path.join(REPO, "INTEGRATION.md")).read()
    lines = text[text.index("### Runtime switches"):].splitlines()
    start = next(i for i, l in enumerate(lines) if l.startswith("|"))
    end = next(i for i in range(start, len(lines)) if not lines[i].startswith("|"))             # the section's first table
    rows = [[c.strip() for c in l.strip().strip("|").split("|")] for l in lines[start:end]]
    assert rows[0] == ["option", "environment variable", "default", "when settable", "what it selects"] and set(rows[1]) == {"---"}
    body = rows[2:]
    tick = lambda c: c.strip("`")
    assert [tick(r[0]) for r in body] == eng.option_names()
    assert {tick(r[0]): (None if r[1] == "--" else tick(r[1]), int(r[2])) for r in body} == TABLE
    assert {tick(r[0]) for r in body if r[3].startswith("before finalize")} == set(BEFORE_FINALIZE)
