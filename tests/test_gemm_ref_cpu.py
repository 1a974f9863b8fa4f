"""CPU: tests/gemm_ref.py judged before it judges a kernel (tests/test_gemm_edges_gpu.py).  Every integer case meets the
conditions exactness rests on and tells the precisions apart; every float case leaves float32 its margin and puts a lost pass
outside the precision-3 bound; and subtly wrong kernels, built from the reference's own passes, break the integer equality at
every shape and -- where the float bound can see them at all -- that bound too."""
import itertools

import pytest
import torch

import gemm_ref as gr
import kernel_refs as kr

CASES = [pytest.param(f, s, id=f"{f}-{gr.case_id(s)}") for f, shapes in gr.FAMILIES.items() for s in shapes]


def _split(family, precision=3):
    return gr.split_of("fp32" if family == "fp32" else "planes", precision)


def _precisions(family):
    return (1, 2, 3) if family == "planes" else (1, 3)


def test_tables_hold_every_edge_the_kernels_branch_on():
    """Each listed value at least once per table, every shape one its launcher accepts (the argument checks of gemm_planes.hip,
    gemm_rows.hip and gemm.hip restated), and the split factors cover 2, 3, 8 and one past the K tiles."""
    cols = lambda shapes, i: {s[i] for s in shapes}
    assert cols(gr.PLANE_SHAPES, 0) == {1, 63, 64, 65, 96, 97, 130} and cols(gr.PLANE_SHAPES, 1) == {4, 60, 64, 68, 192}
    assert cols(gr.PLANE_SHAPES, 2) == {4, 60, 64, 68, 132, 576, 1536}
    assert all(n % 4 == 0 for _, n, _ in gr.PLANE_SHAPES)                  # operand columns padded to a multiple of 4
    assert set(gr.PLANE_KNOBS) == set(gr.PLANE_GEO) == {64, 96, 128, 12832, 256}
    assert {s[2] for s in gr.PLANE_SPLITS} == {68, 576, 1536}
    for (M, N, K), splits in gr.PLANE_SPLITS.items():
        assert (M, N, K) in gr.PLANE_SHAPES and set(splits) >= {2, 3, 8} and max(splits) > gr.ktiles(K)
    assert len(gr.PLANE_GROUP) == 4 and {j[0] for j in gr.PLANE_GROUP} == set(gr.LAYOUTS) and len({j[2] for j in gr.PLANE_GROUP}) == 4
    assert all(p != 2 or layout != "forward" for layout, p, _, _ in gr.PLANE_GROUP)      # precision 2 is built for B m-major
    assert cols(gr.ROWS_SHAPES, 2) == {64, 448, 512, 576, 960, 1024} and {gr.ktiles(k) for k in cols(gr.ROWS_SHAPES, 2)} == {1, 7, 8, 9, 15, 16}
    assert cols(gr.ROWS_SHAPES, 0) == {1, 15, 16, 17, 50, 64, 65, 130} and cols(gr.ROWS_SHAPES, 1) == {1, 15, 16, 17, 202}
    assert len(set(gr.ROWS_SHAPES)) == len(gr.ROWS_SHAPES)
    assert cols(gr.ROWS_BWD_SHAPES, 0) == {1, 15, 17, 50, 64, 130} and cols(gr.ROWS_BWD_SHAPES, 1) == {64, 576, 1024}
    assert cols(gr.ROWS_BWD_SHAPES, 2) == {4, 12, 20, 64, 132, 200}
    assert all(nout % 64 == 0 and nout <= 1024 and kin % 4 == 0 for _, nout, kin in gr.ROWS_BWD_SHAPES)
    assert cols(gr.F32_SHAPES, 0) == {1, 7, 65} and cols(gr.F32_SHAPES, 1) == {1, 5, 65, 130} and cols(gr.F32_SHAPES, 2) == {1, 3, 63, 64, 65, 192, 257}
    for shapes, table in ((gr.PLANE_EPI_SHAPES, gr.PLANE_SHAPES), (gr.ROWS_EPI_SHAPES, gr.ROWS_SHAPES), (gr.F32_EPI_SHAPES, gr.F32_SHAPES)):
        assert all(s in table for s in shapes)


@pytest.mark.parametrize("family,shape", CASES)
def test_integer_cases_meet_the_conditions_exactness_rests_on(family, shape):
    """For the data actually drawn: the splits are exact (hi + lo is the value, both bf16), max sum_k |a||b| < 2^22, at least
    40 % of a tailed operand has a non-zero lo (an eighth where both are tailed: a quarter of the elements are drawn so), and a float32
    accumulation one k at a time reproduces the fp64 product exactly."""
    for pairing, (_, A, B) in [(pg, pr) for pg in gr.case_pairings(family, shape) for pr in gr.products(family, shape, pg)]:
        (M, K), N = A.shape, B.shape[0]
        for split in (kr.bf16_split, gr.trunc_split):
            for x, kind in ((A, pairing[0]), (B, pairing[1])):
                hi, lo = split(x)
                assert torch.equal(hi + lo, x) and torch.equal(hi.bfloat16().float(), hi) and torch.equal(lo.bfloat16().float(), lo)
                share = float((lo != 0).float().mean())
                if kind == "S":
                    assert share == 0.0
                elif x.numel() >= 64:
                    assert share >= gr.TAIL_FLOOR[gr.TT_SHARE if pairing == "TT" else gr.TAIL_SHARE], (pairing, share)
        s = float((A.double().abs() @ B.double().abs().T).max())
        assert s < gr.SUM_LIMIT, (pairing, s)
        acc = torch.zeros(M, N, dtype=torch.float32)
        for k in range(K):
            acc = acc + A[:, k:k + 1] * B[:, k]
        assert torch.equal(acc.double(), A.double() @ B.double().T)
        if pairing == "TT":
            for split in (kr.bf16_split, gr.trunc_split):
                assert bool((gr.passes(A, B, split)[3] != 0).any()), "no lo x lo product: the case does not tell three passes from four"
            if min(M, N) > 1 and K > 4:
                assert not torch.equal(gr.expected(A, B, 3, kr.bf16_split), gr.expected(A, B, 3, gr.trunc_split))


@pytest.mark.parametrize("family,shape", CASES)
def test_integer_cases_tell_the_precisions_apart(family, shape):
    """(A tailed, B short) separates precision 3 from 2 and 1 (the A_lo B_hi pass); (A short, B tailed) separates 1 from 2 and 3 (the
    A_hi B_lo pass): with both pairings every two precisions differ on every shape, in the product and -- 3 against the others --
    in the row sums."""
    for (_, At, Bs), (_, As, Bt) in zip(gr.products(family, shape, "TS"), gr.products(family, shape, "ST")):
        ts, st = [{p: gr.expected(A, B, p, _split(family)) for p in (1, 2, 3)} for A, B in ((At, Bs), (As, Bt))]
        assert not torch.equal(ts[3], ts[2]) and not torch.equal(ts[3], ts[1])
        assert not torch.equal(st[1], st[2]) and not torch.equal(st[1], st[3])
        assert not torch.equal(gr.expected_rowsum(At, 3), gr.expected_rowsum(At, 1)) and torch.equal(gr.expected_rowsum(At, 3), At.double().sum(1))


@pytest.mark.parametrize("family,shape", [c for c in CASES if c.values[1] in gr.PLANE_EPI_SHAPES + gr.ROWS_EPI_SHAPES + gr.F32_EPI_SHAPES])
def test_integer_epilogues_stay_exact(family, shape):
    """Integer bias and residual, ReLU, gate_scale = 2 and dropout at p = 0.5 (scale 2): every value the chain passes through is
    an integer below 2^24 for the data drawn."""
    for pairing in gr.case_pairings(family, shape):
        for _, A, B in gr.products(family, shape, pairing):
            top = float((A.double().abs() @ B.double().abs().T).max()) + 64
            assert (top * gr.GATE_SCALE) * (1.0 / (1.0 - gr.DROP_P)) + 64 < gr.EXACT_LIMIT
    assert 1.0 / (1.0 - gr.DROP_P) == 2.0


@pytest.mark.parametrize("family,shape", CASES)
def test_float_cases_leave_float32_its_margin_and_a_lost_pass_outside_the_bound(family, shape):
    fam = "fp32" if family == "fp32" else "planes"
    for name, A, B in gr.products(family, shape, "float"):
        y = {p: gr.yardsticks(A, B, p, fam) for p in (1, 2, 3)}
        print(family, shape, name, {p: f"e_fmt {v['e_fmt']:.2e} bound {v['bound']:.2e}" for p, v in y.items()}, f"e_fp32 {y[3]['e_fp32']:.2e}")
        assert not torch.isnan(y[3]["ref"]).any() and bool((y[3]["mag"] > 0).all())
        assert y[3]["e_fp32"] <= gr.COND and y[3]["rs_e_fp32"] <= gr.COND
        assert y[3]["bound"] <= y[2]["e_fmt"] / 4, (y[3]["bound"], y[2]["e_fmt"])      # the tolerance alone sees a lost pass
        assert y[3]["e_fmt"] < y[2]["e_fmt"] and y[3]["e_fmt"] < y[1]["e_fmt"]


# what the float bound of a precision can see: at precision 2 a lost A_hi B_lo pass is the size of the format's own error (the
# A_lo B_hi pass it never runs), and no tolerance sees a pass too many -- those are what the integer cases are for
FLOAT_SEES = {3: ("the A_hi B_lo pass lost on the last 64-k tile", "the A_lo B_hi pass lost on the last 64-k tile",
                  "both tails of the last k-octet lost", "the last row run with one pass", "K short by one tile in one split-K slice"),
              2: ("K short by one tile in one split-K slice",),
              1: ("the last k element dropped", "K short by one tile in one split-K slice")}


@pytest.mark.parametrize("family,shape", CASES)
def test_mutants_break_the_integer_equality_and_the_float_bound(family, shape):
    """A pass lost on the last 64-k tile, both tails of the last k-octet lost, the last k dropped at precision 1, the last row
    run with one pass, K short by one tile in one split-K slice, one pass too many at precision 1.  Integer cases: every mutant
    differs from the expected value under at least one pairing (the pairing whose tailed operand the mutant touches), at every
    shape.  Float cases: every mutant FLOAT_SEES lists for the precision is outside the bound."""
    fam = "fp32" if family == "fp32" else "planes"
    for (i, (out, Af, Bf)), p in itertools.product(enumerate(gr.products(family, shape, "float")), _precisions(family)):
        split = gr.split_of(fam, p)
        caught = {}
        for pairing in gr.case_pairings(family, shape):
            _, A, B = gr.products(family, shape, pairing)[i]
            exp = gr.expected(A, B, p, split)
            for name, m in gr.mutants(A, B, p, split).items():
                caught[name] = caught.get(name, False) or not torch.equal(m, exp)
        assert caught and all(caught.values()), (out, p, [n for n, c in caught.items() if not c])
        y = gr.yardsticks(Af, Bf, p, fam)
        muts = gr.mutants(Af, Bf, p, split)
        assert set(muts) == set(caught)
        for name, m in muts.items():
            e = gr.comp_err(m, y["ref"], y["mag"])
            print(family, shape, out, p, name, f"{e:.2e} against {y['bound']:.2e}")
            if name in FLOAT_SEES[p]:
                assert e > y["bound"], (p, name, e, y["bound"])
        assert ("one extra pass" in muts) == (p == 1)


def test_comp_err_sees_one_wrong_element_in_a_small_row():
    """The reason for the componentwise measure: an element of a row 2^-20 the size of the others, wrong by 1e-3 of its own products, is far
    inside max |err| / max |ref| and far outside the bound here; a NaN and a non-zero against a zero magnitude are infinite."""
    M, N, K = 8, 8, 64
    A, B = gr.float_pair(M, N, K)
    A[3] = A[3] * 2.0 ** -20 / A[3].abs().max()
    y = gr.yardsticks(A, B, 3)
    got = y["ref"].clone()
    got[3, 5] += 1e-3 * y["mag"][3, 5]                                   # (a lost tail: 2^-9 of a few products)
    assert kr.rel(got, y["ref"]) < 1e-8 and gr.comp_err(got, y["ref"], y["mag"]) > 10 * y["bound"]
    assert gr.comp_err(y["ref"], y["ref"], y["mag"]) == 0.0
    got = y["ref"].clone()
    got[0, 0] = float("nan")
    assert gr.comp_err(got, y["ref"], y["mag"]) == float("inf")
    assert gr.comp_err(torch.ones(1, 1), torch.zeros(1, 1), torch.zeros(1, 1)) == float("inf")
    assert gr.comp_err(torch.zeros(1, 1), torch.zeros(1, 1), torch.zeros(1, 1)) == 0.0


def test_formats_are_what_the_kernels_make():
    """trunc_split is the upper half of the word and the rounded rest; fmt_matmul at precision 2 is the head of a with both planes
    of b, at 1 and 3 kernel_refs.fmt_matmul; fp32_tiled adds whole tiles in tile order; the epilogue chain in its order."""
    x = torch.tensor([257.0, 259.0, -259.0, 1.0, 0.0, 511.0, 3.14159])
    hi, lo = gr.trunc_split(x)
    assert hi.tolist()[:6] == [256.0, 258.0, -258.0, 1.0, 0.0, 510.0] and lo.tolist()[:6] == [1.0, 1.0, -1.0, 0.0, 0.0, 1.0]
    assert kr.bf16_split(x)[0].tolist()[:3] == [256.0, 260.0, -260.0]
    assert abs(float(hi[6] + lo[6]) - 3.14159) < 3.14159 * 2.0 ** -15 and float(hi[6]) <= 3.14159
    a, b = gr.float_operand(5, 70, 1).double(), gr.float_operand(6, 70, 2).double()
    (ah, al), (bh, bl) = kr.bf16_split(a), kr.bf16_split(b)
    assert torch.equal(gr.fmt_matmul(a, b.T, 2), ah @ bh.T + ah @ bl.T)
    for p in (1, 3):
        assert torch.equal(gr.fmt_matmul(a, b.T, p), kr.fmt_matmul(a, b.T, p))
        assert torch.equal(gr.expected(a.float(), b.float(), p), gr.passes(a, b)[0] + (gr.passes(a, b)[1] + gr.passes(a, b)[2] if p == 3 else 0))
    t = gr.fp32_tiled(a, b)
    want = (a.float()[:, :64] @ b.float()[:, :64].T) + (a.float()[:, 64:] @ b.float()[:, 64:].T)
    assert torch.equal(t, want.double())
    prod = torch.tensor([[-3.0, 5.0], [7.0, -9.0]], dtype=torch.float64)
    out = gr.epilogue(prod, bias=torch.tensor([4.0, 1.0]), relu=True, gate=torch.tensor([[1.0, -1.0], [1.0, 1.0]]), gate_scale=2.0,
                      mask=torch.tensor([[1.0, 1.0], [0.0, 1.0]]), drop_scale=2.0, resid=torch.tensor([[1.0, 1.0], [1.0, 1.0]]))
    assert out.tolist() == [[5.0, 1.0], [1.0, 1.0]]
