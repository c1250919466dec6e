"""The in-situ trace units of rdx_gemv_trace: the hooks header and the binding module name the same `what` values, and the fused attention +
o_proj unit (8) is declared and documented in include/rdx_hooks.h."""
import os
import re

from radialog_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(REPO, "include", "rdx_hooks.h")).read()


def test_header_and_bindings_agree_on_the_in_situ_trace_units():
    defines = {k: int(v) for k, v in re.findall(r"#define\s+(RDX_TRACE_[A-Z_]+)\s+(\d+)", _header())}
    assert defines == {"RDX_TRACE_CHAIN": _lib.TRACE_CHAIN, "RDX_TRACE_ATTN_OPROJ": _lib.TRACE_ATTN_OPROJ}
    assert _lib.TRACE_ATTN_OPROJ == 8 and _lib.TRACE_CHAIN == 7


def test_fused_launch_trace_is_declared_with_the_hook():
    text = _header()
    decl = text.index("int rdx_gemv_trace(rdx_ctx* ctx, int what, int layer, long long* host, int max_tiles);")
    doc = text[:decl]
    assert "what = 8 (RDX_TRACE_ATTN_OPROJ)" in doc[doc.rindex("/*"):]
    assert "rdx_gemv_trace" in _lib.HOOK_SYMBOLS and len(_lib.HOOK_SYMBOLS["rdx_gemv_trace"][1]) == 5
