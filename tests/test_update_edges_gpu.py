"""GPU: the fused update kernels (csrc/update.hip) against the fp64 reference of tests/update_ref.py, element by element, at
ragged sizes and on the trip seams.  Reference, allowance, cases and inputs live in update_ref.py; test_update_ref_cpu.py pins
them to torch and shows that the comparison rejects wrong variants.

  a. every entry point of slnlp.ops at 1, 255 and 257 float4, in the second sum-of-squares trip and in the second update trip,
     4 steps each (clipped, coefficient exactly 1, max_norm 0, an all-zero gradient): the norm, the step dP and every state
     tensor within the allowance at every element after every step, the reference fed the kernel's own state; the device step
     count; the rng counter; the skip range bit-identical where the path honours it; sentinels around every arena intact;
  b. Adam / AdamW from a step count of 999 and 99 999;
  c. segment tables: the 5-segment table scaled to each size, boundaries on the seams, 1024 one-float4 segments;
  d. two runs from the same inputs give the same bits (clip_coef sums in a fixed order);
  e. one NaN / one infinite gradient element, in either sum-of-squares trip: what torch does (update_ref's reference);
  f. plan level: the bf16 hi / lo weight planes the update writes are the split of the arena over the range the plan passes,
     and the split of the initial weights outside it; a fresh engine on a copy of the arena gives the same log-probs.

SLNLP_UPDATE_EDGES_PROFILE=<path>: also write each case's worst err / allowance and the c it was held with there
(profiles/update_edges_parity.json)."""
import json
import os

import numpy as np
import pytest
import torch

import kernel_refs as kr
import update_ref as ur
from test_param_groups_gpu import weight_planes

pytestmark = pytest.mark.gpu

SENTINEL = -1.2345678e30          # finite, and no result of these inputs
SLACK = 1024                      # floats on either side of every arena
MEASURED = {}


@pytest.fixture(scope="module")
def ops():
    from slnlp import ops as o
    yield o
    path = os.environ.get("SLNLP_UPDATE_EDGES_PROFILE")
    if path and MEASURED:
        doc = {"what": "tests/test_update_edges_gpu.py on an MI355X: per case the worst err / allowance over its steps and elements (which "
                       "value: the norm, the step dP, or a state tensor S1 / S2), the largest c of its steps -- 4 x what the float32 "
                       "twin of the fp64 reference needs, floored at 4 -- and beyond_half_ulp: the largest share of the allowance's "
                       "other parts an element needs once the half ulp of its store is taken off (tests/update_ref.py)",
               "cases": dict(sorted(MEASURED.items()))}
        with open(path, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


# ------------------------------------------------------------------------------------------------ arenas with sentinels
class Arena:
    """n floats in the middle of an allocation pre-filled with a sentinel."""

    def __init__(self, data):
        n = data.shape[0]
        self.flat = torch.full((n + 2 * SLACK,), SENTINEL, dtype=torch.float32, device="cuda")
        self.t = self.flat[SLACK:SLACK + n]
        self.t.copy_(torch.from_numpy(np.ascontiguousarray(data)))

    def host(self):
        return self.t.cpu().numpy()

    def intact(self):
        n = self.t.shape[0]
        return bool((self.flat[:SLACK] == SENTINEL).all()) and bool((self.flat[SLACK + n:] == SENTINEL).all())


class Run:
    """The device side of one case: arenas, rates, counters, and the launch of its entry point."""

    def __init__(self, ops, case, p0, s1, s2):
        self.ops, self.case = ops, case
        self.P, self.S1, self.S2 = Arena(p0), Arena(s1), Arena(s2)
        self.cnt = torch.full((1,), float(case.t0), device="cuda")
        self.rng = ops.make_rng(1, 41) if case.entry == "sgd" else None
        t = case.table
        self.lr = torch.tensor(t.lr if t else [case.lr], dtype=torch.float32, device="cuda")
        self.table = ops.ParamGroupTable(case.n, t.seg_begin, t.group, t.wd) if t else None

    def launch(self, g, max_norm):
        c, ops = self.case, self.ops
        G = Arena(g)
        P, S1, S2 = self.P.t, self.S1.t, self.S2.t
        if c.entry == "sgd":
            norm = ops.clip_sgd_step(P, G.t, S1, self.lr, momentum=c.momentum, max_norm=max_norm, rng=self.rng)
        elif c.entry == "sgd_ex":
            norm = ops.clip_sgd_step_ex(P, G.t, S1, self.lr, self.cnt, momentum=c.momentum, dampening=c.dampening, weight_decay=c.wd,
                                        nesterov=c.nesterov, max_norm=max_norm, skip=c.skip)
        elif c.entry == "adam":
            norm = ops.clip_adam_step(P, G.t, S1, S2, self.lr, self.cnt, betas=c.betas, eps=c.eps, weight_decay=c.wd, max_norm=max_norm)
        elif c.entry == "adamw":
            norm = ops.clip_adamw_step(P, G.t, S1, S2, self.lr, self.cnt, betas=c.betas, eps=c.eps, weight_decay=c.wd, max_norm=max_norm,
                                       skip=c.skip)
        elif c.entry == "sgd_groups":
            norm = ops.clip_sgd_step_groups(P, G.t, S1, self.table, self.lr, self.cnt, momentum=c.momentum, dampening=c.dampening,
                                            nesterov=c.nesterov, max_norm=max_norm, skip=c.skip)
        else:
            norm = ops.clip_adam_step_groups(P, G.t, S1, S2, self.table, self.lr, self.cnt, betas=c.betas, eps=c.eps, decoupled=c.decoupled,
                                             max_norm=max_norm, skip=c.skip)
        norm = norm.cpu().numpy()[0]
        assert G.intact() and np.array_equal(G.host(), g, equal_nan=True), "the gradient arena was written"
        return norm

    def state(self):
        return self.P.host(), self.S1.host(), self.S2.host()

    def intact(self):
        return self.P.intact() and self.S1.intact() and self.S2.intact()


def judged_steps(ops, case, grads, max_norms, p0, s1, s2):
    """Run the case's steps; after each, judge norm, dP and the states against the reference fed the kernel's own state.
    -> (the Run, worst (ratio, value, index, step), largest c, largest share of the allowance beyond its half ulp)."""
    run = Run(ops, case, p0, s1, s2)
    worst, c_max, share = (0.0, "", 0, 0), 0.0, 0.0
    before = run.state()
    for k, (g, mx) in enumerate(zip(grads, max_norms)):
        norm = run.launch(g, mx)
        after = run.state()
        ref = ur.reference(case, before[0], g, before[1], before[2], case.t0 + k, mx)
        c = ur.measure_c(case, ref, before[0], g, before[1], before[2], case.t0 + k, mx)
        (ratio, which, i), per = ur.compare(ref, before[0], after[0], after[1], after[2], norm, c)
        print(f"{case.id} step {k}: c {c:.1f}  " + "  ".join(f"{v} {per[v][0]:.3f}@{per[v][1]}" for v in per))
        if ratio >= worst[0]:
            worst = (ratio, which, i, k)
        c_max = max(c_max, c)
        if os.environ.get("SLNLP_UPDATE_EDGES_PROFILE"):
            share = max(share, ur.arithmetic_share(ref, before[0], after[0], after[1], after[2], c))
        assert ratio <= 1, (f"{case.id} step {k}: {which}[{i}] is {ratio:.3g} allowances from the reference "
                            f"(float4 {i // 4} of {case.n // 4}, norm {norm}, reference norm {float(ref.norm)})")
        if not g.any():                                      # the all-zero gradient: exact where a single rounding decides
            assert norm == 0.0
            if case.family == "sgd" and not case.general:
                decayed = (np.float64(ur.f32(case.momentum)) * before[1].astype(np.float64)).astype(np.float32)
                assert np.array_equal(after[1], decayed), "momentum buffers: not m x b, rounded once"
        before = after
    return run, worst, c_max, share


def run_case(ops, case):
    p0, s1, s2, grads, max_norms = case.inputs()
    run, worst, c_max, share = judged_steps(ops, case, grads, max_norms, p0, s1, s2)
    MEASURED[case.id] = {"worst": round(worst[0], 6), "value": worst[1], "step": worst[3], "c": round(c_max, 2), "beyond_half_ulp": round(share, 4)}
    if case.entry != "sgd":
        assert float(run.cnt) == float(case.t0 + case.steps)            # the device step count
    else:
        assert int(run.rng[1]) == 41 + case.steps                        # the dropout step counter: one per step
    if case.honours_skip:
        s = slice(*case.skip)
        P, S1, S2 = run.state()
        assert np.array_equal(P[s], p0[s]) and np.array_equal(S1[s], s1[s]) and np.array_equal(S2[s], s2[s]), "the skip range was stepped"
    assert run.intact(), "written outside an arena"
    return run


# ------------------------------------------------------------------------------------------------ a, b, c
@pytest.mark.parametrize("case", ur.entry_cases(), ids=lambda c: c.id)
def test_every_entry_point_at_every_size(ops, case):
    run_case(ops, case)


@pytest.mark.parametrize("case", ur.count_cases(), ids=lambda c: c.id)
def test_adam_from_a_non_zero_step_count(ops, case):
    run_case(ops, case)


@pytest.mark.parametrize("case", ur.table_cases("a", ur.SIZES) + ur.table_cases("b", [ur.SIZES[4]]) + ur.table_cases("c", None),
                         ids=lambda c: c.id)
def test_segment_tables(ops, case):
    run_case(ops, case)


@pytest.mark.parametrize("n", ur.SIZES, ids=ur.SIZE_IDS)
def test_zero_gradient_from_a_zero_state_moves_nothing(ops, n):
    """norm 0, coefficient 1; Adam's m / (sqrt(v) + eps) is 0 / eps: no weight, no state element changes a bit."""
    for case in (ur.Case("sgd_ex", n), ur.Case("adam", n), ur.Case("adam", n, betas=(0.9, 0.99))):
        p0, z = case.inputs()[0], np.zeros(n, np.float32)
        run = Run(ops, case, p0, z, z)
        assert run.launch(z, 0.5) == 0.0
        P, S1, S2 = run.state()
        assert np.array_equal(P, p0) and not S1.any() and not S2.any() and run.intact() and float(run.cnt) == 1.0


# ------------------------------------------------------------------------------------------------ d
RERUN = [("sgd", {}), ("sgd_ex", ur.SGD_OPTIONS["nesterov_wd"]), ("adam", {}), ("adamw", dict(wd=1e-2))]


@pytest.mark.parametrize("entry,kw", RERUN, ids=[e for e, _ in RERUN])
@pytest.mark.parametrize("n", ur.SIZES[3:], ids=ur.SIZE_IDS[3:])
def test_two_runs_give_the_same_bits(ops, n, entry, kw):
    case = ur.Case(entry, n, random_state=True, **kw)
    p0, s1, s2, grads, max_norms = case.inputs()
    got = []
    for _ in range(2):
        run = Run(ops, case, p0, s1, s2)
        norms = [run.launch(g, mx) for g, mx in zip(grads[:2], max_norms[:2])]
        got.append((np.array(norms), *run.state()))
    for a, b in zip(*got):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))
    assert not np.array_equal(got[0][1], p0)


# ------------------------------------------------------------------------------------------------ e
NONFINITE = [("sgd_ex", "plain"), ("sgd_ex", "wd"), ("adam", "b2_0.999-wd0"), ("adamw", "b2_0.999-wd0.01")]
PLACES = [(ur.SIZES[2], "trip1", 4 * 1 + 1), (ur.SIZES[3], "trip1", 4 * 1000 + 1), (ur.SIZES[3], "trip2", 4 * (ur.SUMSQ_SEAM4 + 1) + 2)]


@pytest.mark.parametrize("value", [np.nan, np.inf], ids=["nan", "inf"])
@pytest.mark.parametrize("n,trip,at", PLACES, ids=[f"{ur.SIZE_ID[n]}-{trip}" for n, trip, _ in PLACES])
@pytest.mark.parametrize("entry,tag", NONFINITE, ids=[f"{e}-{t}" for e, t in NONFINITE])
def test_a_non_finite_gradient_element_does_what_torch_does(ops, entry, tag, n, trip, at, value):
    """One NaN element: the norm and the coefficient are NaN, and with them every stepped weight and every state element
    (torch's clamp propagates NaN: the fit dies visibly instead of taking an unclipped step).  One infinite element: the norm is
    infinite, the coefficient 0, every finite gradient becomes 0 and the element itself NaN (inf x 0).  These are ordinary
    floating-point inputs; the arenas stay inside their sentinels."""
    kw = ur.SGD_OPTIONS[tag] if entry == "sgd_ex" else ur.ADAM_OPTIONS[tag]
    case = ur.Case(entry, n, tag=tag, skip=ur.default_skip(n) if (entry == "adamw" or tag == "wd") else (0, 0), **kw)
    assert not (case.skip[0] <= at < case.skip[1])
    p0, s1, s2, grads, _ = case.inputs()
    g = grads[0].copy()
    g[at] = value
    run = judged_steps(ops, case, [g], [0.5], p0, s1, s2)[0]
    P, S1, S2 = run.state()
    stepped = case.live() if case.honours_skip else np.ones(n, bool)
    if np.isnan(value):
        assert np.isnan(P[stepped]).all() and np.isnan(S1[stepped]).all() and (case.family == "sgd" or np.isnan(S2[stepped]).all())
        assert np.array_equal(P[~stepped], p0[~stepped])
    else:
        assert np.isnan(P[at]) and np.isfinite(np.delete(P, at)).all()
    assert run.intact()


# ------------------------------------------------------------------------------------------------ f
PLANE_SHAPES = {"B4": dict(Vs=64, Vt=16, E=64, H=4, N=2, F=64, B=4, S=12),          # B <= ROWS_MAX_B: the encoder's range only
                "B65": dict(Vs=64, Vt=16, E=64, H=4, N=2, F=64, B=65, S=4)}         # above it: to the end of the arena


def _bits(x):
    return x.to(torch.bfloat16).view(torch.int16)


@pytest.mark.parametrize("kind", ["sgd", "adam", "adamw"])
@pytest.mark.parametrize("shape", list(PLANE_SHAPES))
def test_update_writes_the_split_of_the_arena_over_the_plans_range(shape, kind):
    """Planes == split of the fp32 twin, bit for bit, for the one producer that is an optimizer: after 1 and after 3 fused steps
    the hi / lo weight planes over [wplane_begin, wplane_end) are the split of the arena as it stands, outside it still the split
    of the initial weights (which pins the range); and a fresh engine on a copy of the arena, which splits everything itself,
    gives the same log-probs as the stepped engine reading the planes the update left."""
    from slnlp import synth, tf_engine as te
    c = PLANE_SHAPES[shape]
    X, _, y = [torch.from_numpy(a).cuda() for a in synth.make_batch(c["B"], c["S"], c["Vs"], c["Vt"], seed=1, min_len=3)]
    cfg = te.make_config(c["E"], c["H"], c["N"], c["F"], c["Vs"], c["Vt"], c["B"], c["S"])
    eng = te.TransformerEngine(cfg, device="cuda:0")
    n = eng.arena_floats
    p_init = torch.from_numpy(np.random.default_rng(2).standard_normal(n).astype(np.float32) * np.float32(0.1))
    eng.params.copy_(p_init.cuda())
    eng.set_lr(0.03)
    eng.set_update(kind=kind, weight_decay=1e-2)
    off = {name: o for name, _, o in eng.entries}
    lo = off["transformer.encoder.layers.0.self_attn.in_proj_weight"]
    hi = off["transformer.encoder.norm.weight"] if c["B"] <= 64 else n
    assert 0 < lo < hi <= n
    init = [_bits(h) for h in kr.bf16_split(p_init)]
    v2 = torch.zeros_like(eng.params)
    for step in range(3):
        if kind == "sgd":
            eng.train_step(X, y)
        else:
            eng.train_step_adam(X, y, v2, weight_decay=1e-2)
        if step in (0, 2):
            torch.cuda.synchronize()
            planes, arena = [p.cpu() for p in weight_planes(eng, 0, n)], eng.params.cpu()
            assert not torch.equal(arena[lo:hi], p_init[lo:hi])
            assert kr.planes_are_the_split_of([p[lo:hi] for p in planes], arena[lo:hi]), f"step {step}: planes != split of the arena"
            for p, p0 in zip(planes, init):
                assert torch.equal(p[:lo], p0[:lo]) and torch.equal(p[hi:], p0[hi:]), f"step {step}: planes written outside [{lo}, {hi})"
    logp = eng.forward(X, y, train=False).clone()
    fresh = te.TransformerEngine(cfg, device="cuda:0")
    fresh.params.copy_(eng.params)
    again = fresh.forward(X, y, train=False)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(logp).all()) and torch.equal(logp, again)
