"""CPU: the switch of the decoder backward's d-memory launch (slnlp_tf_set_dmem_batched) is declared, exported and bound, and
the plan's workspace has room for the per-layer pointer table the merged launch reads."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    import __graft_entry__ as ge
    ge.build()
    from slnlp import _lib
    return _lib.load()


def test_switch_is_declared_exported_and_bound():
    lib = _lib()
    from slnlp import _lib as binding
    src = open(os.path.join(ROOT, "include", "slnlp.h")).read()
    assert re.search(r"\bint\s+slnlp_tf_set_dmem_batched\s*\(\s*slnlp_tf_plan\s*\*\s*plan\s*,\s*int\s+on\s*\)\s*;", src)
    assert hasattr(lib, "slnlp_tf_set_dmem_batched")
    assert "slnlp_tf_set_dmem_batched" in binding.SIGNATURES
    assert lib.slnlp_tf_set_dmem_batched(None, 1) == 1            # null plan -> SLNLP_ERR_INVALID_ARG, not an abort
    assert b"tf_set_dmem_batched" in lib.slnlp_last_error()


def test_workspace_holds_the_layer_table():
    """The table sits behind the LayerNorm tables: one 56-byte entry per decoder layer, 256-byte aligned."""
    from slnlp import tf_engine as te
    lib = _lib()
    sizes = [int(lib.slnlp_tf_workspace_bytes(C.byref(te.make_config(64, 4, n, 128, 64, 16, 6, 13)))) for n in (1, 2, 6)]
    assert all(s > 0 and s % 256 == 0 for s in sizes) and sizes[0] < sizes[1] < sizes[2]
