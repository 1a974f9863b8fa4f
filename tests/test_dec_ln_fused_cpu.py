"""CPU: the decoder's LayerNorm-as-prologue launch (slnlp_gemm_rows_ln) and its plan switch (slnlp_tf_set_dec_ln_fused) are
declared in the header, exported by the library and bound in slnlp._lib.SIGNATURES; both refuse a null handle with the
invalid-argument code and their own name in slnlp_last_error()."""
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
    assert re.search(r"\bint\s+slnlp_tf_set_dec_ln_fused\s*\(\s*slnlp_tf_plan\s*\*\s*plan\s*,\s*int\s+on\s*\)\s*;", src)
    assert hasattr(lib, "slnlp_tf_set_dec_ln_fused")
    assert "slnlp_tf_set_dec_ln_fused" in binding.SIGNATURES
    assert lib.slnlp_tf_set_dec_ln_fused(None, 1) == 1            # null plan -> SLNLP_ERR_INVALID_ARG, not an abort
    assert b"tf_set_dec_ln_fused" in lib.slnlp_last_error()


def test_operator_is_declared_exported_and_bound():
    lib = _lib()
    from slnlp import _lib as binding
    src = open(os.path.join(ROOT, "include", "slnlp.h")).read()
    assert re.search(r"\bint\s+slnlp_gemm_rows_ln\s*\(\s*const\s+slnlp_gemm_args\s*\*\s*args\s*,", src)
    assert hasattr(lib, "slnlp_gemm_rows_ln")
    restype, argtypes = binding.SIGNATURES["slnlp_gemm_rows_ln"]
    assert len(argtypes) == 12                                    # args, x, ldx, gamma, beta, eps, y, stats, y_hi, y_lo, ldp, stream
    assert lib.slnlp_gemm_rows_ln(None, None, 0, None, None, 1e-5, None, None, None, None, 0, None) == 1
    assert b"gemm_rows_ln" in lib.slnlp_last_error()


def test_engine_class_has_no_method_for_the_switch():
    """Tests and tools reach it through slnlp._lib.load().slnlp_tf_set_dec_ln_fused(engine.handle, on)."""
    from slnlp import tf_engine as te
    assert not any("ln_fused" in n for n in dir(te.TransformerEngine))
