"""GPU: the three GEMM families -- csrc/gemm.hip (fp32 operands), csrc/gemm_planes.hip (pre-split planes: five tile geometries,
split-K, grouped launches) and csrc/gemm_rows.hip (the decoder's B-row products, forward and the backward pair) -- held to exact
integer products and to fp64 per element.  Cases, references and yardsticks live in tests/gemm_ref.py;
tests/test_gemm_ref_cpu.py judges them (conditions, and mutants that these tests would fail on).

  a. integer cases: every output -- C, its planes, rowsum_a, dX, dW, db -- EQUALS the one value its precision has, for every
     layout, precision, tile knob and split factor.  Condition: max sum_k |a||b| < 2^22 (gemm_ref.SUM_LIMIT).  The single
     64 x 64 x 64 plane product comes first and alone: it is the premise (the bf16 matrix pipe is exact on integers this far
     under 2^24) everything else in (a) rests on;
  b. float cases: err = max |got - fp64| / (|A||B|^T + |bias| + |resid|) < 4 x (e_fmt + e_fp32) floored at 2e-5, computed at run
     time per case and output, printed and recorded;
  c. written and nothing else: every output sits in a sentinel-filled allocation with room before, behind and beside it; no
     sentinel is left inside [M, N] and every word outside still holds it -- the plane words of the 64-aligned box past (M, N)
     included: the kernels store elements (m < M, n < N) only (include/slnlp.h, at C_hi).  From zero-filled planes the padding
     is zero afterwards.  After every split-K launch the first 16 KiB of scratch are zero and a second launch on the same
     scratch returns the same bits;
  d. poison: one NaN at A[M-1, K-1] / at B[N-1, 0] makes exactly that row / column of C NaN, every other element keeps its bits;
  e. refusals: calls the header does not allow return SLNLP_ERR_INVALID_ARG and leave the outputs untouched.

SLNLP_GEMM_EDGES_PROFILE=<path>: also write the measured errors, their bounds and the sum condition there
(profiles/gemm_edges_parity.json)."""
import contextlib
import ctypes as C
import json
import os

import pytest
import torch

import gemm_ref as gr
import kernel_refs as kr
from kernel_refs import planes_are_the_split_of

pytestmark = pytest.mark.gpu

F32_SENTINEL = -1.2345678e30       # finite, and no result of these inputs
W16_SENTINEL = 0x7FA5              # a bf16 NaN with a payload: no split of a number is a NaN, and the NaN the hardware makes is quiet
HEAD, PHEAD = 16, 8                # elements in front of an fp32 output / a plane: 64 and 16 bytes, so the vector stores stay
SITE = 5
MEASURED = {}
INVALID_ARG = 1


@pytest.fixture(scope="module")
def ops():
    from slnlp import ops as o
    yield o
    path = os.environ.get("SLNLP_GEMM_EDGES_PROFILE")
    if path and MEASURED:
        doc = {"what": "tests/test_gemm_edges_gpu.py on an MI355X: err = max |kernel - fp64 reference| / (|A||B|^T + |bias| + |resid|) per "
                       "output of the float cases (rowsum_a / db: over sum_k |a|) and the bound 4 x (e_fmt + e_fp32) floored at 2e-5 it was "
                       "held to, the worst over the knobs of a case; the integer cases are exact (torch.equal) under the sum condition",
               "sum_condition": gr.SUM_LIMIT, "integer_cases": "exact at every case",
               "cases": dict(sorted(MEASURED.items()))}
        with open(path, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


def _lib():
    from slnlp._lib import load
    return load()


@contextlib.contextmanager
def knob(setter, value, reset):
    from slnlp._lib import check
    try:
        check(getattr(_lib(), setter)(value), setter)
        yield
    finally:
        getattr(_lib(), setter)(reset)


def pad64(n):
    return (n + 63) // 64 * 64


# ------------------------------------------------------------------------------------------------ outputs with sentinels
class F32Out:
    """[M, N] fp32 with ldc = N + 8 inside a sentinel-filled allocation: HEAD words in front, 64 rows behind."""

    def __init__(self, M, N, extra=8, head=HEAD):
        self.M, self.N, self.ld, self.rows, self.head = M, N, N + extra, M + 64, head
        self.flat = torch.full((head + self.rows * self.ld,), F32_SENTINEL, dtype=torch.float32, device="cuda")
        self.ptr = self.flat[head:].data_ptr()

    def reset(self):
        self.flat.fill_(F32_SENTINEL)

    def untouched(self):
        return bool((self.flat == F32_SENTINEL).all())

    def take(self, what="C"):
        """(c) for this output -> its [M, N] on the CPU."""
        f = self.flat.cpu()
        v = f[self.head:].view(self.rows, self.ld).clone()
        inner = v[:self.M, :self.N].clone()
        assert bool((inner != F32_SENTINEL).all()), f"{what}: an element was not written"
        v[:self.M, :self.N] = F32_SENTINEL
        assert bool((v == F32_SENTINEL).all()), f"{what}: written outside [M, N]"
        assert bool((f[:self.head] == F32_SENTINEL).all()), f"{what}: written before its first element"
        return inner


class VecOut(F32Out):
    """rowsum_a [M] with a sentinel head and tail."""

    def __init__(self, M):
        super().__init__(1, M, extra=16, head=4)

    def take(self, what="rowsum_a"):
        return super().take(what)[0]


class PlanesOut:
    """hi / lo planes of [M, N]: 64 rows and 64 columns beyond the 64-aligned box, PHEAD words into their allocations."""

    def __init__(self, M, N, fill=W16_SENTINEL, head=PHEAD):
        self.M, self.N, self.R, self.ld, self.head, self.fill = M, N, pad64(M) + 64, pad64(N) + 64, head, fill
        self.flat = [torch.full((head + self.R * self.ld,), fill, dtype=torch.int16, device="cuda") for _ in range(2)]
        self.hi, self.lo = [f[head:].data_ptr() for f in self.flat]

    def reset(self):
        for f in self.flat:
            f.fill_(self.fill)

    def untouched(self):
        return all(bool((f == self.fill).all()) for f in self.flat)

    def take(self, what="C planes"):
        """(c): nothing but (m < M, n < N) is stored -- the box past (M, N) keeps its words like everything else."""
        out = []
        for name, flat in zip(("hi", "lo"), self.flat):
            f = flat.cpu()
            v = f[self.head:].view(self.R, self.ld).clone()
            inner = v[:self.M, :self.N].clone()
            if self.fill == W16_SENTINEL:
                assert bool((inner != W16_SENTINEL).all()), f"{what} {name}: an element was not written"
            v[:self.M, :self.N] = self.fill
            box = v[:pad64(self.M), :pad64(self.N)]
            assert bool((box == self.fill).all()), f"{what} {name}: the padding inside the 64-aligned box was stored to"
            assert bool((v == self.fill).all()), f"{what} {name}: written outside the 64-aligned box"
            assert bool((f[:self.head] == self.fill).all()), f"{what} {name}: written before its first element"
            out.append(inner)
        return tuple(out)


# ------------------------------------------------------------------------------------------------ operands
def planes_of(x):
    """float32 [R, C] on the CPU -> (hi, lo) int16 planes on the device, zero-padded to multiples of 64 (split_bf16's bits)."""
    R, Cc = x.shape
    out = []
    for t in kr.bf16_split(x.float()):
        p = torch.zeros(pad64(R), pad64(Cc), dtype=torch.int16)
        p[:R, :Cc] = t.to(torch.bfloat16).view(torch.int16)
        out.append(p.cuda())
    return tuple(out)


_DATA = {}


def pair(shape, kind):
    """(A [M, K], B [N, K]) on the CPU: kind "float" or an integer pairing."""
    key = (shape, kind)
    if key not in _DATA:
        _DATA[key] = gr.float_pair(*shape) if kind == "float" else gr.int_pair(*shape, kind)
    return _DATA[key]


def epi_tensors(ops, M, N, integer):
    """bias, gate, resid (integers, or Gaussians for the float cases), the rng and its p = 0.5 mask."""
    key = ("epi", M, N, integer)
    if key not in _DATA:
        if integer:
            bias, gate, resid = gr.int_vector(N, 3), gr.int_matrix(M, N, 4, -3, 4), gr.int_matrix(M, N, 5)
        else:
            bias, gate, resid = gr.float_operand(1, N, 3)[0], gr.int_matrix(M, N, 4, -3, 4), gr.float_operand(M, N, 5)
        rng = ops.make_rng(seed=7, step=3)
        mask = ops.dropout_mask(M, N, gr.DROP_P, SITE, rng).cpu()
        _DATA[key] = dict(bias=bias, gate=gate, resid=resid, rng=rng, mask=mask, dev=dict(bias=bias.cuda(), gate=gate.cuda(), resid=resid.cuda()))
    return _DATA[key]


EPILOGUES = ("late", "early")          # without dropout (bias, ReLU, gate, residual in the row-major phase) / with it (accumulator layout)


def set_epilogue(j, e, route):
    j.bias, j.relu = e["dev"]["bias"].data_ptr(), 1
    j.gate, j.ldg, j.gate_scale, j.gate_mode = e["dev"]["gate"].data_ptr(), e["dev"]["gate"].stride(0), gr.GATE_SCALE, 0
    j.resid, j.ldr = e["dev"]["resid"].data_ptr(), e["dev"]["resid"].stride(0)
    if route == "early":
        j.drop_p, j.drop_site, j.rng = gr.DROP_P, SITE, e["rng"].data_ptr()


def epilogue_args(e, route):
    kw = dict(bias=e["bias"], relu=True, gate=e["gate"], gate_scale=gr.GATE_SCALE, resid=e["resid"])
    if route == "early":
        kw.update(mask=e["mask"], drop_scale=1.0 / (1.0 - gr.DROP_P))
    return kw


def same(got, want, what):
    got, want = got.double(), want.double()
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        first = [(tuple(i.tolist()), float(got[tuple(i)]), float(want[tuple(i)])) for i in bad[:8]]
        raise AssertionError(f"{what}: {len(bad)} of {got.numel()} elements differ; (index, got, expected) {first}")


def held(tag, name, got, ref, mag, bound, e_fmt, e_fp32):
    """(b): measure, print, record the worst per (tag, name), then assert."""
    e = gr.comp_err(got, ref, mag)
    print(f"{tag} {name}: err {e:.2e} e_fmt {e_fmt:.2e} e_fp32 {e_fp32:.2e} bound {bound:.2e}")
    rec = MEASURED.setdefault(tag, {})
    if name not in rec or e > rec[name]["err"]:
        rec[name] = {"err": float(f"{e:.3e}"), "bound": float(f"{bound:.3e}")}
    assert e < bound, (tag, name, e, bound)


# ================================================================================================ the plane GEMM
_PLANE_OPS = {}


def plane_operands(shape, kind, layout, A=None, B=None):
    key = (shape, kind, layout)
    if A is not None or key not in _PLANE_OPS:
        if A is None:
            A, B = pair(shape, kind)
        v = (planes_of(A if layout != "wgrad" else A.T.contiguous()), planes_of(B if layout == "forward" else B.T.contiguous()))
        if kind is None:
            return v
        _PLANE_OPS[key] = v
    return _PLANE_OPS[key]


def plane_job(opnds, layout, precision, shape, out=None, planes=None, rs=None):
    from slnlp._lib import GemmArgs
    (Ah, Al), (Bh, Bl) = opnds
    M, N, K = shape
    j = GemmArgs()
    j.A_hi, j.A_lo, j.lda_p = Ah.data_ptr(), Al.data_ptr(), Ah.stride(0)
    j.B_hi, j.B_lo, j.ldb_p = Bh.data_ptr(), Bl.data_ptr(), Bh.stride(0)
    j.a_kmajor, j.b_kmajor, j.precision = int(layout != "wgrad"), int(layout == "forward"), precision
    j.M, j.N, j.K = M, N, K
    if out is not None:
        j.C, j.ldc = out.ptr, out.ld
    if planes is not None:
        j.C_hi, j.C_lo, j.ldc_p = planes.hi, planes.lo, planes.ld
    if rs is not None:
        j.rowsum_a = rs.ptr
    return j


def launch(j):
    from slnlp._lib import check, stream_ptr
    check(_lib().slnlp_gemm(C.byref(j), stream_ptr()), "gemm")
    torch.cuda.synchronize()


def expected_geo(knob_value, layout, split=1):
    return gr.PLANE_GEO[knob_value] if knob_value != 96 or (layout != "wgrad" and split == 1) else 0


def plane_run(ops, opnds, layout, precision, shape, *, epi=None, route=None, split=1, scratch=None, fill=W16_SENTINEL, want_c=True, scalar=False):
    """One launch with every output framed -> (C or None, (hi, lo), rowsum_a) on the CPU, (c) asserted on the way.  ``scalar``:
    C one float past a 16-byte boundary with an odd ldc, the planes 4 bytes past an 8-byte one -- a valid call that takes the
    per-element stores."""
    M, N, K = shape
    out = (F32Out(M, N, extra=9 - N % 2, head=1) if scalar else F32Out(M, N)) if want_c else None
    planes, rs = PlanesOut(M, N, fill, head=2 if scalar else PHEAD), VecOut(M)
    assert not scalar or (out.ptr % 16 == 4 and out.ld % 2 == 1 and planes.hi % 8 == 4)
    j = plane_job(opnds, layout, precision, shape, out, planes, rs)
    if epi is not None:
        set_epilogue(j, epi, route)
    if split == 1:
        launch(j)
    else:
        ops.gemm_group([j], [split], scratch)
        torch.cuda.synchronize()
    return (out.take() if want_c else None), planes.take(), rs.take()


def test_one_64_tile_is_exact_on_integers(ops):
    """The premise of (a), first and alone: one 64 x 64 x 64 product on the 64 x 64 tile, three passes, A tailed and B short
    (sum_k |a||b| < 2^22, in fact < 2^17 here).  Every element equals the integer product: the bf16 matrix pipe aligns its
    products finely enough for integers this far under 2^24.  A failure here lists the differing elements; it is a finding
    about the premise, not a tolerance to widen."""
    shape = (64, 64, 64)
    A, B = pair(shape, "TS")
    with knob("slnlp_set_plane_tile", 64, 0):
        c, (hi, lo), rs = plane_run(ops, plane_operands(shape, "TS", "forward"), "forward", 3, shape)
    same(c, A.double() @ B.double().T, "64 x 64 x 64, precision 3")
    same(rs, A.double().sum(1), "rowsum_a")
    assert planes_are_the_split_of((hi, lo), c)


def plane_precisions(layout):
    return (1, 3) if layout == "forward" else (1, 2, 3)


PLANE_PARAMS = [pytest.param(layout, p, id=f"{layout}-p{p}") for layout in gr.LAYOUTS for p in plane_precisions(layout)]


@pytest.mark.parametrize("layout,precision", PLANE_PARAMS)
def test_plane_integer_cases_are_exact_at_every_tile(ops, layout, precision):
    """(a) and (c): every shape and pairing at every tile knob -- C, its planes and rowsum_a -- and at the epilogue shapes the
    exact epilogue (integer bias and residual, ReLU, gate x 2, dropout at p = 0.5) on both routes; once per shape from
    zero-filled planes (the padding is zero afterwards: the next GEMM relies on it) and with the fp32 output NULL, and once with
    outputs whose alignment sends the stores down the per-element path."""
    for shape in gr.PLANE_SHAPES:
        M, N, K = shape
        for pairing in gr.pairings(*shape):
            A, B = pair(shape, pairing)
            exp, exp_rs = gr.expected(A, B, precision), gr.expected_rowsum(A, precision)
            opnds = plane_operands(shape, pairing, layout)
            for kv in gr.PLANE_KNOBS:
                tag = f"{layout} p{precision} {shape} {pairing} tile {kv}"
                with knob("slnlp_set_plane_tile", kv, 0):
                    assert ops.plane_geo([plane_job(opnds, layout, precision, shape, F32Out(1, 1))]) == expected_geo(kv, layout), tag
                    c, (hi, lo), rs = plane_run(ops, opnds, layout, precision, shape)
                    same(c, exp, tag)
                    same(rs, exp_rs, tag + " rowsum_a")
                    assert planes_are_the_split_of((hi, lo), c), tag
                    if shape in gr.PLANE_EPI_SHAPES:
                        e = epi_tensors(ops, M, N, True)
                        for route in EPILOGUES:
                            c, (hi, lo), rs = plane_run(ops, opnds, layout, precision, shape, epi=e, route=route)
                            same(c, gr.epilogue(exp, **epilogue_args(e, route)), f"{tag} epilogue {route}")
                            same(rs, exp_rs, f"{tag} epilogue {route} rowsum_a")
                            assert planes_are_the_split_of((hi, lo), c), f"{tag} epilogue {route}"
            if pairing == "TS":
                for kv in (64, 128):
                    with knob("slnlp_set_plane_tile", kv, 0):
                        c, (hi, lo), rs = plane_run(ops, opnds, layout, precision, shape, scalar=True)
                    same(c, exp, f"{layout} p{precision} {shape} tile {kv}, per-element stores")
                    assert planes_are_the_split_of((hi, lo), c)
                want = kr.bf16_split(exp.float())
                for kv in (64, 96):
                    with knob("slnlp_set_plane_tile", kv, 0):
                        _, (hi, lo), _ = plane_run(ops, opnds, layout, precision, shape, fill=0, want_c=False)
                    assert torch.equal(hi, want[0].to(torch.bfloat16).view(torch.int16)) and torch.equal(lo, want[1].to(torch.bfloat16).view(torch.int16))


@pytest.mark.parametrize("layout", gr.LAYOUTS)
def test_plane_split_k_is_exact_leaves_scratch_zero_and_repeats(ops, layout):
    """(a) and (c) under split-K: factors 2, 3, 8 and one past the K tiles at K = 68, 576, 1536 (two of them do not divide the
    tiles), every tile knob (the 96 x 64 tile never splits: 64 x 64 is taken), every precision of the layout; the epilogue
    behind the in-kernel meeting at K = 576.  After each launch the first 16 KiB of scratch are zero; a second launch on the
    same scratch returns the same bits."""
    from slnlp._lib import GemmArgs
    for shape, splits in gr.PLANE_SPLITS.items():
        M, N, K = shape
        for precision in plane_precisions(layout):
            for pairing in gr.PAIRINGS:
                A, B = pair(shape, pairing)
                exp, exp_rs = gr.expected(A, B, precision), gr.expected_rowsum(A, precision)
                opnds = plane_operands(shape, pairing, layout)
                routes = (None,) + (("early",) if shape in gr.PLANE_EPI_SHAPES and pairing == "TS" else ())
                for split in splits:
                    probe = plane_job(opnds, layout, precision, shape, F32Out(1, 1))
                    nbytes = int(_lib().slnlp_gemm_group_scratch_bytes((GemmArgs * 1)(probe), (C.c_int32 * 1)(split), 1))
                    for kv in gr.PLANE_KNOBS:
                        tag = f"{layout} p{precision} {shape} {pairing} tile {kv} split {split}"
                        scratch = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
                        with knob("slnlp_set_plane_tile", kv, 0):
                            assert ops.plane_geo([probe], [split]) == expected_geo(kv, layout, split), tag
                            for route in routes:
                                e = epi_tensors(ops, M, N, True) if route else None
                                want = gr.epilogue(exp, **epilogue_args(e, route)) if route else exp
                                first = plane_run(ops, opnds, layout, precision, shape, epi=e, route=route, split=split, scratch=scratch)
                                assert int(scratch[:16384].view(torch.int32).abs().max()) == 0, tag + ": arrival counters not back to zero"
                                again = plane_run(ops, opnds, layout, precision, shape, epi=e, route=route, split=split, scratch=scratch)
                                assert int(scratch[:16384].view(torch.int32).abs().max()) == 0, tag
                                same(first[0], want, tag)
                                same(first[2], exp_rs, tag + " rowsum_a")
                                assert planes_are_the_split_of(first[1], first[0]), tag
                                assert torch.equal(first[0], again[0]) and torch.equal(first[2], again[2]), tag + ": a second launch on the same scratch differs"
                                assert all(torch.equal(a, b) for a, b in zip(first[1], again[1])), tag


def test_plane_grouped_launch_of_four_shapes_and_layouts(ops):
    """(a) and (c): four jobs of four shapes in ONE launch -- forward, data gradient at two passes, two weight gradients with
    split-K 3 and 8 (two and three passes sharing the launch) -- at the automatic geometry and at each forced one."""
    from slnlp._lib import GemmArgs
    for pairing in gr.PAIRINGS:
        jobs, outs, wants, keep = [], [], [], []
        for layout, precision, shape, split in gr.PLANE_GROUP:
            A, B = pair(shape, pairing)
            opnds = plane_operands(shape, pairing, layout)
            o = (F32Out(shape[0], shape[1]), PlanesOut(shape[0], shape[1]), VecOut(shape[0]))
            jobs.append(plane_job(opnds, layout, precision, shape, *o))
            outs.append(o)
            wants.append((gr.expected(A, B, precision), gr.expected_rowsum(A, precision)))
        splits = [s for _, _, _, s in gr.PLANE_GROUP]
        nbytes = int(_lib().slnlp_gemm_group_scratch_bytes((GemmArgs * 4)(*jobs), (C.c_int32 * 4)(*splits), 4))
        for kv in (0,) + gr.PLANE_KNOBS:
            scratch = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
            for o in outs:
                for t in o:
                    t.reset()
            with knob("slnlp_set_plane_tile", kv, 0):
                ops.gemm_group(jobs, splits, scratch)
                torch.cuda.synchronize()
            assert int(scratch[:16384].view(torch.int32).abs().max()) == 0
            for (o, pl, rs), (want, want_rs), job in zip(outs, wants, gr.PLANE_GROUP):
                tag = f"group {pairing} tile {kv} job {job}"
                c = o.take()
                same(c, want, tag)
                same(rs.take(), want_rs, tag + " rowsum_a")
                assert planes_are_the_split_of(pl.take(), c), tag


@pytest.mark.parametrize("layout,precision", PLANE_PARAMS)
def test_plane_float_cases_against_fp64_per_element(ops, layout, precision):
    """(b) and (c): every shape at every tile knob; at the epilogue shapes also bias -> ReLU -> gate -> dropout -> residual on
    Gaussian bias and residual; at the split shapes also split-K 3."""
    for shape in gr.PLANE_SHAPES:
        M, N, K = shape
        A, B = pair(shape, "float")
        y = gr.yardsticks(A, B, precision)
        assert y["e_fp32"] <= gr.COND and y["rs_e_fp32"] <= gr.COND            # the premise of the bound (test_gemm_ref_cpu.py)
        opnds = plane_operands(shape, "float", layout)
        tag = f"planes {layout} p{precision} {gr.case_id(shape)}"
        runs = [(kv, 1) for kv in gr.PLANE_KNOBS] + ([(64, 3), (128, 3)] if shape in gr.PLANE_SPLITS else [])
        for kv, split in runs:
            scratch = torch.zeros(int(4 * 256 * 256 * 3 * 4 + 65536), dtype=torch.uint8, device="cuda") if split > 1 else None
            with knob("slnlp_set_plane_tile", kv, 0):
                c, (hi, lo), rs = plane_run(ops, opnds, layout, precision, shape, split=split, scratch=scratch)
            held(tag, "C", c, y["ref"], y["mag"], y["bound"], y["e_fmt"], y["e_fp32"])
            held(tag, "rowsum_a", rs, y["rs_ref"], y["rs_mag"], y["rs_bound"], y["rs_e_fmt"], y["rs_e_fp32"])
            assert planes_are_the_split_of((hi, lo), c), tag
        if shape in gr.PLANE_EPI_SHAPES:
            e = epi_tensors(ops, M, N, False)
            for route in EPILOGUES:
                ye = gr.yardsticks(A, B, precision, **epilogue_args(e, route))
                for kv in gr.PLANE_KNOBS:
                    with knob("slnlp_set_plane_tile", kv, 0):
                        c, (hi, lo), _ = plane_run(ops, opnds, layout, precision, shape, epi=e, route=route)
                    held(tag + " epilogue " + route, "C", c, ye["ref"], ye["mag"], ye["bound"], ye["e_fmt"], ye["e_fp32"])
                    assert planes_are_the_split_of((hi, lo), c), tag


# ================================================================================================ gemm_rows, forward
def rows_job(Ap, W, precision, shape, out=None, planes=None):
    from slnlp._lib import GemmArgs
    M, N, K = shape
    j = GemmArgs()
    j.A_hi, j.A_lo, j.lda_p = Ap[0].data_ptr(), Ap[1].data_ptr(), Ap[0].stride(0)
    j.B, j.ldb = W.data_ptr(), W.stride(0)
    j.a_kmajor, j.b_kmajor, j.precision = 1, 1, precision
    j.M, j.N, j.K = M, N, K
    if out is not None:
        j.C, j.ldc = out.ptr, out.ld
    if planes is not None:
        j.C_hi, j.C_lo, j.ldc_p = planes.hi, planes.lo, planes.ld
    return j


def rows_run(Ap, W, precision, shape, epi=None, route=None):
    from slnlp._lib import check, stream_ptr
    out, planes = F32Out(shape[0], shape[1]), PlanesOut(shape[0], shape[1])
    j = rows_job(Ap, W, precision, shape, out, planes)
    if epi is not None:
        set_epilogue(j, epi, route)
    check(_lib().slnlp_gemm_rows(C.byref(j), stream_ptr()), "gemm_rows")
    torch.cuda.synchronize()
    return out.take(), planes.take()


@pytest.mark.parametrize("precision", [1, 3])
def test_rows_integer_cases_are_exact_at_every_tile(ops, precision):
    """(a) and (c): 1, 7, 8, 9, 15 and 16 K tiles (wave w takes tiles w, w + 8: 9 is the first wrap, 15 leaves the last wave
    short), rows and columns around the 16-wide MFMA tile and the 64-row block, the three workgroup tiles; the exact epilogue
    at the epilogue shapes."""
    for shape in gr.ROWS_SHAPES:
        M, N, K = shape
        for pairing in gr.pairings(*shape):
            A, B = pair(shape, pairing)
            exp = gr.expected(A, B, precision)
            Ap, W = planes_of(A), B.cuda()
            for tile in gr.ROWS_TILES:
                tag = f"rows p{precision} {shape} {pairing} tile {tile}"
                with knob("slnlp_set_rows_tile", tile, -1):
                    c, pl = rows_run(Ap, W, precision, shape)
                    same(c, exp, tag)
                    assert planes_are_the_split_of(pl, c), tag
                    if shape in gr.ROWS_EPI_SHAPES:
                        e = epi_tensors(ops, M, N, True)
                        for route in EPILOGUES:
                            c, pl = rows_run(Ap, W, precision, shape, e, route)
                            same(c, gr.epilogue(exp, **epilogue_args(e, route)), f"{tag} epilogue {route}")
                            assert planes_are_the_split_of(pl, c), f"{tag} epilogue {route}"


@pytest.mark.parametrize("precision", [1, 3])
def test_rows_float_cases_against_fp64_per_element(ops, precision):
    for shape in gr.ROWS_SHAPES:
        A, B = pair(shape, "float")
        y = gr.yardsticks(A, B, precision)
        assert y["e_fp32"] <= gr.COND
        Ap, W = planes_of(A), B.cuda()
        for tile in gr.ROWS_TILES:
            with knob("slnlp_set_rows_tile", tile, -1):
                c, pl = rows_run(Ap, W, precision, shape)
            held(f"rows p{precision} {gr.case_id(shape)}", "C", c, y["ref"], y["mag"], y["bound"], y["e_fmt"], y["e_fp32"])
            assert planes_are_the_split_of(pl, c)


# ================================================================================================ gemm_rows, the backward pair
def bwd_data(shape, kind):
    key = ("bwd", shape, kind)
    if key not in _DATA:
        _DATA[key] = gr.bwd_operands(shape, kind)
    return _DATA[key]


def bwd_run(dYp, W, Xp, precision, shape):
    """slnlp_gemm_rows_bwd with dX, its planes, dW and db framed -> (dX, planes, dW, db) on the CPU."""
    from slnlp._lib import GemmArgs, check, stream_ptr
    Bt, Nout, Kin = shape
    dX, pl, dW, db = F32Out(Bt, Kin), PlanesOut(Bt, Kin), F32Out(Nout, Kin), VecOut(Nout)
    d, w = GemmArgs(), GemmArgs()
    d.C, d.ldc, d.M, d.N, d.K = dX.ptr, dX.ld, Bt, Kin, Nout
    d.a_kmajor, d.b_kmajor, d.precision = 1, 0, precision
    d.A_hi, d.A_lo, d.lda_p = dYp[0].data_ptr(), dYp[1].data_ptr(), dYp[0].stride(0)
    d.B, d.ldb = W.data_ptr(), W.stride(0)
    d.C_hi, d.C_lo, d.ldc_p = pl.hi, pl.lo, pl.ld
    w.C, w.ldc, w.M, w.N, w.K = dW.ptr, dW.ld, Nout, Kin, Bt
    w.a_kmajor, w.b_kmajor, w.precision = 0, 0, precision
    w.A_hi, w.A_lo, w.lda_p = dYp[0].data_ptr(), dYp[1].data_ptr(), dYp[0].stride(0)
    w.B_hi, w.B_lo, w.ldb_p = Xp[0].data_ptr(), Xp[1].data_ptr(), Xp[0].stride(0)
    w.rowsum_a = db.ptr
    check(_lib().slnlp_gemm_rows_bwd(C.byref(d), C.byref(w), stream_ptr()), "gemm_rows_bwd")
    torch.cuda.synchronize()
    return dX.take("dX"), pl.take("dX planes"), dW.take("dW"), db.take("db")


@pytest.mark.parametrize("precision", [1, 3])
def test_rows_bwd_integer_cases_are_exact_at_every_tile(ops, precision):
    """(a) and (c): dX = dY W, dW = dY^T X, db = column sums of dY in one launch.  Kin 4 and 12 sit inside the data gradient's
    `min(c0 + 4 * (lane & 3), N - 4)` column clamp, Kin 132 gives the weight gradient two column units, 130 rows three K tiles."""
    for shape in gr.ROWS_BWD_SHAPES:
        for pairing in gr.case_pairings("rows_bwd", shape):
            dY, W, X = bwd_data(shape, pairing)
            want = (gr.expected(dY, W.T, precision), gr.expected(dY.T, X.T, precision), gr.expected_rowsum(dY.T, precision))
            dYp, Wd, Xp = planes_of(dY), W.cuda(), planes_of(X)
            for tile in gr.ROWS_TILES:
                tag = f"rows_bwd p{precision} {shape} {pairing} tile {tile}"
                with knob("slnlp_set_rows_tile", tile, -1):
                    dX, pl, dW, db = bwd_run(dYp, Wd, Xp, precision, shape)
                same(dX, want[0], tag + " dX")
                same(dW, want[1], tag + " dW")
                same(db, want[2], tag + " db")
                assert planes_are_the_split_of(pl, dX), tag


@pytest.mark.parametrize("precision", [1, 3])
def test_rows_bwd_float_cases_against_fp64_per_element(ops, precision):
    for shape in gr.ROWS_BWD_SHAPES:
        dY, W, X = bwd_data(shape, "float")
        yd, yw = gr.yardsticks(dY, W.T.contiguous(), precision), gr.yardsticks(dY.T.contiguous(), X.T.contiguous(), precision)
        assert yd["e_fp32"] <= gr.COND and yw["e_fp32"] <= gr.COND and yw["rs_e_fp32"] <= gr.COND
        dYp, Wd, Xp = planes_of(dY), W.cuda(), planes_of(X)
        tag = f"rows_bwd p{precision} {gr.case_id(shape)}"
        for tile in gr.ROWS_TILES:
            with knob("slnlp_set_rows_tile", tile, -1):
                dX, pl, dW, db = bwd_run(dYp, Wd, Xp, precision, shape)
            held(tag, "dX", dX, yd["ref"], yd["mag"], yd["bound"], yd["e_fmt"], yd["e_fp32"])
            held(tag, "dW", dW, yw["ref"], yw["mag"], yw["bound"], yw["e_fmt"], yw["e_fp32"])
            held(tag, "db", db, yw["rs_ref"], yw["rs_mag"], yw["rs_bound"], yw["rs_e_fmt"], yw["rs_e_fp32"])
            assert planes_are_the_split_of(pl, dX), tag


# ================================================================================================ the fp32-operand GEMM
F32_STORAGE = ("plain", "padded", "unaligned")


def store(x, how):
    """A [rows, cols] view on the device of x's values: contiguous; row stride a multiple of 4 with NaN in the padding (the
    vector loads); or one float past a 16-byte boundary with an odd row stride and NaN between the rows (the scalar loads)."""
    rows, cols = x.shape
    if how == "plain":
        return x.contiguous().cuda()
    ld = (cols + 3) // 4 * 4 + 4 if how == "padded" else cols + 1 + cols % 2
    off = 0 if how == "padded" else 1
    flat = torch.full((off + rows * ld + 8,), float("nan"), dtype=torch.float32)
    flat[off:off + rows * ld].view(rows, ld)[:, :cols] = x
    dev = flat.cuda()
    v = dev[off:off + rows * ld].view(rows, ld)[:, :cols]
    assert (v.data_ptr() % 16 == 0 and ld % 4 == 0) if how == "padded" else (v.data_ptr() % 16 == 4 and ld % 2 == 1)
    return v


def f32_run(ops, A, B, layout, precision, shape, how, epi=None, route=None, want_planes=False):
    from slnlp._lib import GemmArgs
    M, N, K = shape
    Ad = store(A if layout != "wgrad" else A.T, how)
    Bd = store(B if layout == "forward" else B.T, how)
    out, rs = F32Out(M, N), (VecOut(M) if layout == "wgrad" else None)
    planes = PlanesOut(M, N) if want_planes else None
    j = GemmArgs()
    j.A, j.lda, j.a_kmajor = Ad.data_ptr(), Ad.stride(0), int(layout != "wgrad")
    j.B, j.ldb, j.b_kmajor = Bd.data_ptr(), Bd.stride(0), int(layout == "forward")
    j.C, j.ldc, j.M, j.N, j.K, j.precision = out.ptr, out.ld, M, N, K, precision
    if rs is not None:
        j.rowsum_a = rs.ptr
    if planes is not None:
        j.C_hi, j.C_lo, j.ldc_p = planes.hi, planes.lo, planes.ld
    if epi is not None:
        set_epilogue(j, epi, route)
    launch(j)
    return out.take(), (rs.take() if rs is not None else None), (planes.take() if planes is not None else None)


F32_PARAMS = [pytest.param(layout, p, id=f"{layout}-p{p}") for layout in gr.LAYOUTS for p in (1, 3)]


@pytest.mark.parametrize("layout,precision", F32_PARAMS)
def test_f32_integer_cases_are_exact_on_every_load_path(ops, layout, precision):
    """(a) and (c): K = 1 .. 257 (192 = three K tiles: halves of 2 + 1), one and two thread groups, contiguous operands, padded
    strides with NaN in the padding, and views one float past a 16-byte boundary with an odd stride (the scalar-load build).
    At precision 3 the expected value is made with this family's truncating split."""
    split = gr.split_of("fp32", precision)
    for shape in gr.F32_SHAPES:
        M, N, K = shape
        for pairing in gr.pairings(*shape):
            A, B = pair(shape, pairing)
            exp, exp_rs = gr.expected(A, B, precision, split), gr.expected_rowsum(A, precision, split)
            for ks in gr.F32_KS:
                for how in F32_STORAGE:
                    tag = f"fp32 {layout} p{precision} {shape} {pairing} ks {ks} {how}"
                    with knob("slnlp_set_gemm_ks", ks, 0):
                        c, rs, pl = f32_run(ops, A, B, layout, precision, shape, how, want_planes=how == "plain")
                        same(c, exp, tag)
                        if rs is not None:
                            same(rs, exp_rs, tag + " rowsum_a")
                        if pl is not None:
                            assert planes_are_the_split_of(pl, c), tag
                        if shape in gr.F32_EPI_SHAPES and how != "padded":
                            e = epi_tensors(ops, M, N, True)
                            for route in EPILOGUES:
                                c, _, _ = f32_run(ops, A, B, layout, precision, shape, how, e, route)
                                same(c, gr.epilogue(exp, **epilogue_args(e, route)), f"{tag} epilogue {route}")


@pytest.mark.parametrize("layout,precision", F32_PARAMS)
def test_f32_float_cases_against_fp64_per_element(ops, layout, precision):
    for shape in gr.F32_SHAPES:
        A, B = pair(shape, "float")
        y = gr.yardsticks(A, B, precision, "fp32")
        assert y["e_fp32"] <= gr.COND and y["rs_e_fp32"] <= gr.COND
        tag = f"fp32 {layout} p{precision} {gr.case_id(shape)}"
        for ks in gr.F32_KS:
            for how in F32_STORAGE:
                with knob("slnlp_set_gemm_ks", ks, 0):
                    c, rs, _ = f32_run(ops, A, B, layout, precision, shape, how)
                held(tag, "C", c, y["ref"], y["mag"], y["bound"], y["e_fmt"], y["e_fp32"])
                if rs is not None:
                    held(tag, "rowsum_a", rs, y["rs_ref"], y["rs_mag"], y["rs_bound"], y["rs_e_fmt"], y["rs_e_fp32"])


def test_f32_batched_head_jobs_are_exact(ops):
    """(a) and (c): one batch = H job per stride pattern of csrc/linear_jobs.hpp (head_expand, head_reduce, head_wgrad) through
    slnlp_gemm_group at (B, H, dh) = (3, 2, 8), the three in one launch: A tailed, B short, so A B^T exactly."""
    from test_attn_mem_gpu import head_expand_job, head_reduce_job, head_wgrad_job
    Bt, H, dh = gr.F32_BATCH
    E = H * dh
    x, dy, W = gr.int_operand(Bt, E, "T", 71), gr.int_operand(Bt, E, "T", 72), gr.int_operand(E, E, "S", 73)
    xh_t, xh_s = gr.int_operand(Bt, H * E, "T", 74).view(Bt, H, E), gr.int_operand(Bt, H * E, "S", 75).view(Bt, H, E)
    outs = dict(expand=F32Out(Bt, H * E, extra=0), reduce=F32Out(Bt, E, extra=0), dW=F32Out(E, E, extra=0))
    view = lambda o, *s: o.flat[o.head:o.head + o.M * o.N].view(*s)
    xc, dyc, Wc, xtc, xsc = x.cuda(), dy.cuda(), W.cuda(), xh_t.cuda(), xh_s.cuda()
    jobs = [head_expand_job(xc, Wc, view(outs["expand"], Bt, H, E), Bt, H, dh), head_reduce_job(xtc, Wc, view(outs["reduce"], Bt, E), Bt, H, dh),
            head_wgrad_job(dyc, xsc, view(outs["dW"], E, E), Bt, H, dh)]
    ops.gemm_group(jobs, scratch=torch.zeros(16, dtype=torch.uint8, device="cuda"))
    torch.cuda.synchronize()
    Wd = W.double().view(H, dh, E)
    same(outs["expand"].take("expand").view(Bt, H, E), torch.einsum("bhd,hde->bhe", x.double().view(Bt, H, dh), Wd), "head_expand")
    same(outs["reduce"].take("reduce"), torch.einsum("bhe,hde->bhd", xh_t.double(), Wd).reshape(Bt, E), "head_reduce")
    same(outs["dW"].take("dW"), torch.einsum("bhd,bhe->hde", dy.double().view(Bt, H, dh), xh_s.double()).reshape(E, E), "head_wgrad")


# ================================================================================================ d. poison
def _poisoned(A, B):
    """[(which, A', B', rows that must be NaN or None, columns that must be NaN or None)]"""
    Ap, Bp = A.clone(), B.clone()
    Ap[-1, -1] = float("nan")
    Bp[-1, 0] = float("nan")
    return [("A[M-1, K-1]", Ap, B, A.shape[0] - 1, None), ("B[N-1, 0]", A, Bp, None, B.shape[0] - 1)]


def _only_that_line_is_nan(clean, got, row, col, what):
    nan = torch.isnan(got)
    want = torch.zeros_like(nan)
    if row is not None:
        want[row] = True
    else:
        want[:, col] = True
    assert torch.equal(nan, want), f"{what}: NaN elsewhere than the poisoned line, or not all of it"
    assert not torch.isnan(clean).any()
    assert torch.equal(clean.view(torch.int32)[~want], got.view(torch.int32)[~want]), f"{what}: another element changed its bits"


@pytest.mark.parametrize("layout", gr.LAYOUTS)
def test_poison_reaches_one_line_of_the_plane_and_fp32_products(ops, layout):
    for family, shape in (("planes", (65, 68, 68)), ("fp32", (65, 65, 63))):
        A, B = pair(shape, "float")
        run = (lambda a, b: plane_run(ops, plane_operands(shape, None, layout, a, b), layout, 3, shape)[0]) if family == "planes" else \
              (lambda a, b: f32_run(ops, a, b, layout, 3, shape, "plain")[0])
        clean = run(A, B)
        for which, a, b, row, col in _poisoned(A, B):
            _only_that_line_is_nan(clean, run(a, b), row, col, f"{family} {layout} {which}")


def test_poison_reaches_one_line_of_the_row_products(ops):
    shape = (17, 17, 576)
    A, B = pair(shape, "float")
    clean = rows_run(planes_of(A), B.cuda(), 3, shape)[0]
    for which, a, b, row, col in _poisoned(A, B):
        _only_that_line_is_nan(clean, rows_run(planes_of(a), b.cuda(), 3, shape)[0], row, col, f"rows {which}")
    bshape = (17, 576, 20)
    dY, W, X = bwd_data(bshape, "float")
    cdX, _, cdW, cdb = bwd_run(planes_of(dY), W.cuda(), planes_of(X), 3, bshape)
    p = dY.clone()
    p[-1, -1] = float("nan")                                 # dY[B-1, Nout-1]: A[M-1, K-1] of the data gradient, A(m = Nout-1, k = B-1) of the weight gradient
    dX, _, dW, db = bwd_run(planes_of(p), W.cuda(), planes_of(X), 3, bshape)
    _only_that_line_is_nan(cdX, dX, bshape[0] - 1, None, "rows_bwd dX")
    _only_that_line_is_nan(cdW, dW, bshape[1] - 1, None, "rows_bwd dW")
    _only_that_line_is_nan(cdb[None], db[None], None, bshape[1] - 1, "rows_bwd db")
    p = W.clone()
    p[0, -1] = float("nan")                                  # W[0, Kin-1]: B[N-1, 0] of the data gradient; the weight gradient does not read W
    dX, _, dW, db = bwd_run(planes_of(dY), p.cuda(), planes_of(X), 3, bshape)
    _only_that_line_is_nan(cdX, dX, None, bshape[2] - 1, "rows_bwd dX (W poisoned)")
    assert torch.equal(cdW.view(torch.int32), dW.view(torch.int32)) and torch.equal(cdb.view(torch.int32), db.view(torch.int32))


# ================================================================================================ e. refusals
def test_refused_calls_return_the_argument_error_and_touch_nothing(ops):
    """Calls include/slnlp.h does not allow: each returns SLNLP_ERR_INVALID_ARG before anything is launched."""
    from slnlp._lib import GemmArgs, stream_ptr
    lib = _lib()
    shape = (65, 68, 68)
    M, N, K = shape
    out, planes, rs = F32Out(M, N), PlanesOut(M, N), VecOut(M)
    fresh = lambda layout, precision: plane_job(plane_operands(shape, "TS", layout), layout, precision, shape, out, planes, rs)

    def refused(call, what):
        rc = call()
        torch.cuda.synchronize()
        assert rc == INVALID_ARG, (what, rc, lib.slnlp_last_error())
        assert out.untouched() and planes.untouched() and rs.untouched(), what + ": an output was touched"

    # gemm_rows past 16 K tiles
    rshape = (17, 17, 1088)
    Ar, Br = gr.int_pair(*rshape, "TS")
    Apr, Wr = planes_of(Ar), Br.cuda()
    ro, rp = F32Out(17, 17), PlanesOut(17, 17)
    j = rows_job(Apr, Wr, 3, rshape, ro, rp)
    assert lib.slnlp_gemm_rows(C.byref(j), stream_ptr()) == INVALID_ARG
    torch.cuda.synchronize()
    assert ro.untouched() and rp.untouched()
    # plane strides that are not multiples of 64
    for field in ("lda_p", "ldb_p"):
        j = fresh("forward", 3)
        setattr(j, field, getattr(j, field) + 32)
        refused(lambda: lib.slnlp_gemm(C.byref(j), stream_ptr()), field + " + 32")
    # precision 2 with k-major B
    j = fresh("forward", 2)
    refused(lambda: lib.slnlp_gemm(C.byref(j), stream_ptr()), "precision 2, B k-major")
    # A m-major with B k-major
    j = fresh("wgrad", 3)
    j.b_kmajor = 1
    refused(lambda: lib.slnlp_gemm(C.byref(j), stream_ptr()), "A m-major, B k-major")
    # planes 8 bytes off a 16-byte boundary
    for field in ("A_hi", "A_lo", "B_hi", "B_lo"):
        j = fresh("forward", 3)
        setattr(j, field, getattr(j, field) + 8)
        refused(lambda: lib.slnlp_gemm(C.byref(j), stream_ptr()), field + " + 8 bytes")
    # ldc < N, in every family
    j = fresh("forward", 3)
    j.ldc = N - 4
    refused(lambda: lib.slnlp_gemm(C.byref(j), stream_ptr()), "planes: ldc < N")
    j = fresh("dgrad", 3)
    j.ldc = N - 4
    refused(lambda: lib.slnlp_gemm_group((GemmArgs * 1)(j), (C.c_int32 * 1)(1), 1, None, 0, stream_ptr()), "planes, grouped: ldc < N")
    j = rows_job(Apr, Wr, 3, (17, 17, 576), ro, rp)
    j.ldc = 16
    assert lib.slnlp_gemm_rows(C.byref(j), stream_ptr()) == INVALID_ARG
    A, B = pair(shape, "TS")
    Ad, Bd = A.cuda(), B.cuda()
    j = GemmArgs()
    j.A, j.lda, j.a_kmajor, j.B, j.ldb, j.b_kmajor = Ad.data_ptr(), K, 1, Bd.data_ptr(), K, 1
    j.C, j.ldc, j.M, j.N, j.K, j.precision = out.ptr, N - 1, M, N, K, 3
    refused(lambda: lib.slnlp_gemm(C.byref(j), stream_ptr()), "fp32: ldc < N")
    torch.cuda.synchronize()
    assert ro.untouched() and rp.untouched()
