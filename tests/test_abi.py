"""CPU: the C-ABI library builds, loads without a GPU, exports every symbol
include/slnlp.h declares, and its arena layout is the reference state_dict."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from slnlp import _lib
    return _lib.load()


def header_symbols():
    src = open(os.path.join(ROOT, "include", "slnlp.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(slnlp_[a-z0-9_]+)\s*\(", src)))


def test_every_declared_symbol_is_exported_and_bound(lib):
    from slnlp import _lib
    syms = header_symbols()
    assert len(syms) >= 25
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in slnlp.h but not exported by libslnlp.so"
        assert s in _lib.SIGNATURES, f"{s} has no ctypes signature in slnlp/_lib.py"
    assert sorted(_lib.SIGNATURES) == syms
    assert lib.slnlp_abi_version() == 1


def test_layout_is_reference_state_dict(lib):
    from oracle import transformer_ref as tr
    from slnlp import tf_engine as te
    for (E, H, N, F, Vs, Vt) in [(32, 4, 2, 64, 64, 16), (128, 4, 2, 256, 3000, 202), (512, 8, 6, 512, 3000, 202)]:
        cfg = te.make_config(E, H, N, F, Vs, Vt, 50, 48)
        ents, total = te.layout(cfg)
        want = tr.param_shapes(E, H, N, F, Vs, Vt)
        assert [(n, s) for n, s, _ in ents] == [(n, tuple(s)) for n, s in want]
        end = 0
        for n, s, off in ents:
            assert off % 4 == 0 and off >= end                 # 16-byte aligned, non-overlapping
            numel = 1
            for d in s:
                numel *= d
            end = off + numel
        assert total >= end and total % 4 == 0
    assert sum(1 for _ in ents) == 2 + 12 * 6 + 2 + 18 * 6 + 2 + 2
    # parameter counts quoted in SURVEY.md section 8 (a1)
    cfg = te.make_config(128, 4, 2, 256, 3000, 200, 50, 48)
    ents, _ = te.layout(cfg)
    count = 0
    for _, s, _ in ents:
        k = 1
        for d in s:
            k *= d
        count += k
    assert count == 1098440


def test_argument_validation_returns_codes_not_aborts(lib):
    from slnlp import _lib, tf_engine as te
    bad = te.make_config(130, 4, 2, 256, 3000, 202, 50, 48)       # head_dim 32.5
    assert lib.slnlp_tf_num_params(C.byref(bad)) == -1
    assert b"divisible" in lib.slnlp_last_error()
    bad = te.make_config(128, 4, 2, 256, 3000, 202, 5, 5001)      # beyond the reference's 5000-row positional table
    assert lib.slnlp_tf_workspace_bytes(C.byref(bad)) == -1
    assert b"seq_len" in lib.slnlp_last_error()
    assert lib.slnlp_tf_workspace_bytes(C.byref(te.make_config(128, 4, 2, 256, 3000, 202, 50, 65))) > 0      # S > 64 is fine
    bad = te.make_config(128, 4, 2, 256, 3000, 202, 1024, 65)     # more tokens per step than the embedding backward indexes
    assert lib.slnlp_tf_workspace_bytes(C.byref(bad)) == -1 and b"tokens" in lib.slnlp_last_error()
    a = _lib.GemmArgs()
    assert lib.slnlp_gemm(C.byref(a), None) == 1                  # null operands -> SLNLP_ERR_INVALID_ARG
    assert lib.slnlp_gemm(None, None) == 1
    # the attention launchers that take output planes: every refusal comes before a launch, so none needs a device
    buf = (C.c_float * 16)()
    p = C.cast(buf, C.c_void_p).value                             # any non-null address: nothing below gets as far as reading it
    INVALID = 1

    def fwd(S=20, dh=8, ctx=p, hi=None, lo=None, q8=None, drop=0.0, ld_ids=None, B=2):
        return lib.slnlp_attn_self_fwd_ex(p, p, S if ld_ids is None else ld_ids, 1, 1, B, S, 2, dh, ctx, p, drop, 0, None, hi, lo, q8, None)

    def bwd(S=20, dh=8, dqkv=p, hi=None, lo=None, scratch=None, drop=0.0, B=2):
        return lib.slnlp_attn_self_bwd_ex(p, p, p, B, S, 2, dh, dqkv, drop, 0, None, scratch, hi, lo, None)

    def xbwd(S=20, dh=8, hi=None, lo=None, ld=32, drop=0.0, dkv=p):
        return lib.slnlp_attn_cross_bwd_ex(p, p, ld, p, p, 2, S, 2, dh, p, dkv, ld, drop, 0, None, hi, lo, None)

    for call in (fwd, bwd, xbwd):
        for kw in (dict(hi=p), dict(lo=p)):                       # one plane of a pair without the other
            assert call(**kw) == INVALID and b"go together" in lib.slnlp_last_error(), (call.__name__, kw)
        assert call(dh=6, hi=p, lo=p) == INVALID and b"head_dim" in lib.slnlp_last_error()       # the existing shape checks
        assert call(S=0, hi=p, lo=p) == INVALID
        assert call(drop=0.25, hi=p, lo=p) == INVALID and b"dropout" in lib.slnlp_last_error()   # dropout without its rng
        assert call(drop=1.0, hi=p, lo=p) == INVALID and b"dropout" in lib.slnlp_last_error()
    assert fwd(q8=p) == INVALID and b"q8" in lib.slnlp_last_error()                              # q8 without hi / lo
    assert fwd(ctx=None) == INVALID and b"null" in lib.slnlp_last_error()                        # no fp32 output and no planes
    assert bwd(dqkv=None) == INVALID and b"null" in lib.slnlp_last_error()
    assert fwd(S=65, ctx=None, hi=p, lo=p) == INVALID and b"S <= 64" in lib.slnlp_last_error()   # planes only: one-tile kernels
    assert bwd(S=65, dqkv=None, hi=p, lo=p, scratch=p) == INVALID and b"S <= 64" in lib.slnlp_last_error()
    assert bwd(S=65, hi=p, lo=p) == INVALID and b"scratch" in lib.slnlp_last_error()             # S > 64 without long_scratch
    assert fwd(ld_ids=19) == INVALID and b"ld_ids" in lib.slnlp_last_error()
    assert fwd(B=0, hi=p, lo=p) == INVALID and bwd(B=0, hi=p, lo=p) == INVALID
    assert xbwd(ld=31, hi=p, lo=p) == INVALID and b"ld" in lib.slnlp_last_error()                # ld_kv / ld_dkv: multiples of 4, >= 2E
    assert xbwd(ld=28, hi=p, lo=p) == INVALID
    assert xbwd(dkv=None, hi=p, lo=p) == INVALID and b"null" in lib.slnlp_last_error()           # the cross backward always writes fp32


def test_attn_mem_entry_points_validate_before_they_touch_a_device(lib):
    """slnlp_attn_mem_fwd / _bwd / _dmem_all check shapes and pointers first: codes and messages, no launch, no GPU needed."""
    from slnlp import _lib
    buf = (C.c_float * 16)()
    p = C.cast(buf, C.c_void_p).value                           # any non-null address: nothing below gets as far as reading it
    INVALID = 1                                                  # SLNLP_ERR_INVALID_ARG

    def fwd(B, S, H, dh, qk=p):
        return lib.slnlp_attn_mem_fwd(qk, p, p, B, S, H, dh, p, p, p, p, 0.0, 0, None, None)

    def bwd(B, S, H, dh, dsc=p):
        return lib.slnlp_attn_mem_bwd(p, p, p, p, p, p, p, B, S, H, dh, dsc, p, p, p, None, 0, 0.0, 0, None, None)

    def dmem_all(B, S, H, dh, tab=p, N=1):
        return lib.slnlp_attn_mem_dmem_all(tab, N, B, S, H, dh, p, 0.0, None, None)

    for call in (fwd, bwd, dmem_all):
        assert call(2, 3, 65, 4) == INVALID and b"heads" in lib.slnlp_last_error()          # H = 65 > the 64 the LDS tables hold
        assert call(2, 3, 2, 6) == INVALID and b"head_dim" in lib.slnlp_last_error()        # dh not a multiple of 4
        assert call(2, 3, 8, 256) == INVALID and b"2048" in lib.slnlp_last_error()          # H * dh = 2048 > 1024
        assert call(2, 0, 2, 4) == INVALID and call(0, 3, 2, 4) == INVALID and call(2, 5001, 2, 4) == INVALID
    assert fwd(2, 3, 2, 4, qk=None) == INVALID and b"null" in lib.slnlp_last_error()
    assert bwd(2, 3, 2, 4, dsc=None) == INVALID and b"null" in lib.slnlp_last_error()
    assert dmem_all(2, 3, 2, 4, tab=None) == INVALID and b"null" in lib.slnlp_last_error()
    assert dmem_all(2, 3, 2, 4, N=0) == INVALID
    assert lib.slnlp_attn_mem_fwd(p, p, p, 2, 3, 2, 4, p, p, p, p, 0.25, 0, None, None) == INVALID      # dropout without its rng
    assert b"dropout" in lib.slnlp_last_error()
    assert C.sizeof(_lib.XmemDmemLayer) == 56                    # slnlp_xmem_dmem_layer: six pointers, drop_site, pad


def test_set_xmem_heads_takes_0_1_2_4_only(lib):
    try:
        for hp in (3, -1, 8, 5):
            assert lib.slnlp_set_xmem_heads(hp) == 1 and b"set_xmem_heads" in lib.slnlp_last_error()
        for hp in (1, 2, 4, 0):
            assert lib.slnlp_set_xmem_heads(hp) == 0
    finally:
        assert lib.slnlp_set_xmem_heads(0) == 0


def test_product_path_fails_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from slnlp import ops, tf_engine as te
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.gemm(torch.zeros(4, 4), torch.zeros(4, 4), M=4, N=4, K=4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        te.TransformerEngine(te.make_config(32, 4, 2, 64, 64, 16, 4, 12))


def test_bench_flop_contract():
    """bench.py prices a step with SURVEY.md section 8d's algorithmic-FLOP formula (forward per sequence; x3 for training)."""
    import bench
    f = {k: bench.fwd_flops_per_seq(bench.WORKLOADS[k]) for k in ("cfg1", "cfg2", "e1024", "cfg5")}
    assert abs(f["cfg1"] / 3.46e7 - 1) < 0.01 and abs(f["cfg2"] / 1.26e9 - 1) < 0.01
    assert abs(f["e1024"] / 4.37e9 - 1) < 0.01 and abs(f["cfg5"] / 5.83e9 - 1) < 0.01
