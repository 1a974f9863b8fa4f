"""CPU: tests/update_ref.py judged before the GPU test relies on it -- the numpy reference against clip_grad_norm_ +
torch.optim.SGD / Adam / AdamW in fp64 (1e-12: the round-off of two orderings, loose only against a difference of formula),
the comparison against deliberately wrong variants of the reference (each must be rejected at every size where it applies),
and the conditions on the inputs (every edge element steps by at least 64 allowances, 99 % of the arena does)."""
import numpy as np
import pytest
import torch

import update_ref as ur

SMALL = [ur.SIZES[0], ur.SIZES[2]]
RTOL = 1e-12


# ------------------------------------------------------------------------------------------------ the reference against torch
def torch_pieces(case, p0):
    """fp64 parameters cut at the table's boundaries and the skip range's ends, one torch param group per table group."""
    n, t = case.n, case.table
    begin = t.seg_begin if t else [0]
    cuts = sorted(set(begin + [n] + ([case.skip[0], case.skip[1]] if case.skip[1] > case.skip[0] else [])))
    pieces = [(b, e, torch.nn.Parameter(torch.from_numpy(p0[b:e].astype(np.float64)))) for b, e in zip(cuts, cuts[1:])]
    if t:
        ends = begin[1:] + [n]
        groups = []
        for gi in range(len(t.lr)):
            spans = [(b, e) for b, e, g in zip(begin, ends, t.group) if g == gi]
            mine = [p for b, e, p in pieces if any(sb <= b and e <= se for sb, se in spans)]
            groups.append({"params": mine, "lr": ur.f32(t.lr[gi]), "weight_decay": ur.f32(t.wd[gi])})
    else:
        groups = [{"params": [p for _, _, p in pieces], "lr": ur.f32(case.lr), "weight_decay": ur.f32(case.wd)}]
    if case.family == "sgd":
        opt = torch.optim.SGD(groups, lr=1.0, momentum=ur.f32(case.momentum), dampening=ur.f32(case.dampening) if case.momentum else 0.0,
                              nesterov=case.nesterov, foreach=False)
    else:
        cls = torch.optim.AdamW if case.decoupled else torch.optim.Adam
        opt = cls(groups, lr=1.0, betas=(ur.f32(case.betas[0]), ur.f32(case.betas[1])), eps=ur.f32(case.eps), foreach=False)
    return pieces, opt


def torch_step(case, pieces, opt, g, max_norm):
    for b, e, p in pieces:
        skipped = case.honours_skip and case.skip[0] <= b and e <= case.skip[1]
        p.grad = None if skipped else torch.from_numpy(g[b:e].astype(np.float64))
    total = torch.nn.utils.clip_grad_norm_([p for _, _, p in pieces], max_norm, foreach=False) if max_norm > 0 else None
    opt.step()
    return total


def gather(case, pieces, opt=None, key=None):
    out = np.zeros(case.n)
    for b, e, p in pieces:
        if key is None:
            out[b:e] = p.detach().numpy()
        elif p in opt.state and key in opt.state[p] and opt.state[p][key] is not None:
            out[b:e] = opt.state[p][key].numpy()
    return out


def close(a, b):
    scale = float(np.nanmax(np.abs(np.where(np.isfinite(b), b, 0.0)))) if b.size else 0.0
    return np.allclose(a, b, rtol=RTOL, atol=RTOL * scale, equal_nan=True)


def against_torch(case, grads, max_norms, p0):
    pieces, opt = torch_pieces(case, p0)
    P, S1, S2 = p0.astype(np.float64), np.zeros(case.n), np.zeros(case.n)
    for k, (g, mx) in enumerate(zip(grads, max_norms)):
        r = ur.step(case, P, g, S1, S2, k, mx)                    # the fp64 chain: nothing is rounded between the steps
        total = torch_step(case, pieces, opt, g, mx)
        P, S1, S2 = r.P, r.S1, r.S2
        if total is not None:
            assert close(np.array([r.norm]), np.array([float(total)])), (case.id, k)
        assert close(P, gather(case, pieces)), (case.id, k, "P")
        if case.family == "sgd":
            if case.momentum != 0:
                assert close(S1, gather(case, pieces, opt, "momentum_buffer")), (case.id, k, "momentum_buffer")
        else:
            assert close(S1, gather(case, pieces, opt, "exp_avg")), (case.id, k, "exp_avg")
            assert close(S2, gather(case, pieces, opt, "exp_avg_sq")), (case.id, k, "exp_avg_sq")
    return P


TORCH_CASES = ([c for c in ur.entry_cases(SMALL) if c.entry != "sgd"]          # (sgd: sgd_ex's plain loop from a non-zero buffer)
               + ur.table_cases("a", SMALL) + ur.table_cases("b", SMALL))


@pytest.mark.parametrize("case", TORCH_CASES, ids=lambda c: c.id)
def test_reference_equals_torch_in_fp64(case):
    p0, _, _, grads, max_norms = case.inputs()
    P = against_torch(case, grads, max_norms, p0)
    assert not np.array_equal(P, p0.astype(np.float64))


NONFINITE_ENTRIES = [("sgd_ex", "plain"), ("sgd_ex", "wd"), ("adam", "b2_0.999-wd0"), ("adamw", "b2_0.999-wd0.01")]


def nonfinite_case(entry, tag, n):
    kw = ur.SGD_OPTIONS[tag] if entry == "sgd_ex" else ur.ADAM_OPTIONS[tag]
    return ur.Case(entry, n, tag=tag, skip=ur.default_skip(n) if (entry == "adamw" or tag == "wd") else (0, 0), **kw)


@pytest.mark.parametrize("value", [np.nan, np.inf], ids=["nan", "inf"])
@pytest.mark.parametrize("entry,tag", NONFINITE_ENTRIES)
def test_reference_follows_torch_on_a_non_finite_gradient(entry, tag, value):
    """A NaN element makes the norm, the coefficient and with it every stepped weight and state element NaN; an infinite one
    makes the coefficient 0, the finite gradients 0 and the element itself NaN (inf x 0)."""
    case = nonfinite_case(entry, tag, ur.SIZES[2])
    p0, _, _, grads, _ = case.inputs()
    g = grads[0].copy()
    g[5] = value
    P = against_torch(case, [g], [0.5], p0)
    stepped = case.live() if case.honours_skip else np.ones(case.n, bool)
    if np.isnan(value):
        assert np.isnan(P[stepped]).all() and np.array_equal(P[~stepped], p0[~stepped].astype(np.float64))
    else:
        assert np.isnan(P[5]) and np.isfinite(np.delete(P, 5)).all()


# ------------------------------------------------------------------------------------------------ the comparison bites
_SIM, _C = {}, {}


def simulated(case):
    """The case's chain, kept for the case asked last (the largest hold hundreds of MB)."""
    if case.id not in _SIM:
        _SIM.clear()
        _C.clear()
        _SIM[case.id] = ur.simulate(case)
    return _SIM[case.id]


def judged_all(case, k, mutate):
    """err / allowance per judged value of the mutant's step k (its results stored as float32, as a kernel would store them)
    against the reference; c is the reference's and its twin's, whatever the mutant does."""
    P, G, S1, S2, t0, mx, ref = simulated(case)[k]
    got = ur.step(case, P, G, S1, S2, t0, mx, mutate=mutate)
    if k not in _C:
        _C[k] = ur.measure_c(case, ref, P, G, S1, S2, t0, mx)
    with np.errstate(all="ignore"):
        return ur.compare(ref, P, got.P.astype(np.float32), got.S1.astype(np.float32), got.S2.astype(np.float32), np.float32(got.norm), _C[k])


def judged(case, k, mutate):
    return judged_all(case, k, mutate)[0]


def base_cases(n):
    """Four code paths of the reference at the small sizes; at the two large ones (2 s a step here) one SGD and one Adam path."""
    cases = [ur.Case("sgd", n, random_state=True),
             ur.Case("sgd_ex", n, tag="wd", skip=ur.default_skip(n), **ur.SGD_OPTIONS["wd"]),
             ur.Case("adamw", n, tag="b2_0.99-wd0.01", skip=ur.default_skip(n), **ur.ADAM_OPTIONS["b2_0.99-wd0.01"]),
             ur.Case("adam", n, tag="b2_0.999-wd0", **ur.ADAM_OPTIONS["b2_0.999-wd0"])]
    return cases if n < ur.SIZES[3] else [cases[1], cases[3]]


def steps_of(n, steps=(0, 1, 2)):
    """The steps with a gradient; the clipped one alone at the two large sizes."""
    return steps if n < ur.SIZES[3] else steps[:1]


@pytest.mark.parametrize("n", ur.SIZES, ids=ur.SIZE_IDS)
def test_the_reference_itself_and_its_float32_twin_pass(n):
    for case in base_cases(n):
        for k in steps_of(n, range(ur.STEPS)):
            ratio, which, i = judged(case, k, None)
            assert ratio <= 1, (case.id, k, which, i, ratio)              # stored as float32: half an ulp, the allowance's first part


@pytest.mark.parametrize("n", ur.SIZES, ids=ur.SIZE_IDS)
def test_mutant_last_float4_not_updated(n):
    for case in base_cases(n):
        for k in steps_of(n, range(ur.STEPS)):
            ratio, which, i = judged(case, k, {"untouched_float4": n // 4 - 1})
            assert ratio > 1 and i // 4 == n // 4 - 1, (case.id, k, ratio, which, i)


@pytest.mark.parametrize("n,seam", [(ur.SIZES[3], ur.SUMSQ_SEAM4), (ur.SIZES[4], ur.SUMSQ_SEAM4), (ur.SIZES[4], ur.UPDATE_SEAM4)],
                         ids=["sumsq_trip2-at_sumsq_seam", "update_trip2-at_sumsq_seam", "update_trip2-at_update_seam"])
def test_mutant_first_float4_of_a_second_trip_not_updated(n, seam):
    for case in base_cases(n):
        for k in steps_of(n):
            ratio, which, i = judged(case, k, {"untouched_float4": seam})
            assert ratio > 1 and i // 4 == seam, (case.id, k, ratio, which, i)


@pytest.mark.parametrize("n", ur.SIZES[3:], ids=ur.SIZE_IDS[3:])
def test_mutant_first_float4_of_the_second_sumsq_trip_not_summed(n):
    for case in base_cases(n):
        per = judged_all(case, 0, {"norm_drops_float4": ur.SUMSQ_SEAM4})[1]
        assert per["norm"][0] > 1 and max(per[k][0] for k in ("dP", "S1", "S2")) > 1, (case.id, per)   # the norm AND what it clips


@pytest.mark.parametrize("n", ur.SIZES[3:], ids=ur.SIZE_IDS[3:])
def test_mutant_second_sumsq_trip_dropped_from_the_norm(n):
    for case in base_cases(n):
        per = judged_all(case, 0, {"norm_drops_trip2": True})[1]
        assert per["norm"][0] > 1 and max(per[k][0] for k in ("dP", "S1", "S2")) > 1, (case.id, per)


@pytest.mark.parametrize("which", ["a", "b", "c"])
def test_mutant_neighbour_segment_lr_at_a_boundary(which):
    sizes = ur.SIZES[1:] if which == "a" else [ur.SIZES[2], ur.SIZES[4]]
    applied = 0
    for case in ur.table_cases(which, sizes):
        if case.tag.split("-")[-1] not in ("wd", "table_" + which):               # one SGD and the two Adam variants
            continue
        if case.n >= ur.SIZES[3] and case.decoupled:
            continue
        t = case.table
        bounds = [b for s, b in enumerate(t.begin4) if s and t.lr[t.group[s]] != t.lr[t.group[s - 1]] and case.live()[4 * b]]
        for b in (bounds if which != "c" else bounds[::97]):
            for k in steps_of(case.n):
                ratio, _, i = judged(case, k, {"neighbour_lr": b})
                assert ratio > 1 and i // 4 == b, (case.id, b, k, ratio, i)
                applied += 1
    assert applied >= 30


@pytest.mark.parametrize("n", ur.SIZES, ids=ur.SIZE_IDS)
def test_mutant_first_step_treated_as_not_first_under_dampening(n):
    case = ur.Case("sgd_ex", n, tag="dampening", skip=ur.default_skip(n), **ur.SGD_OPTIONS["dampening"])
    ratio, which, _ = judged(case, 0, {"never_first": True})
    assert ratio > 1, (ratio, which)


@pytest.mark.parametrize("n", ur.SIZES[1:], ids=ur.SIZE_IDS[1:])
def test_mutant_skip_range_shifted_by_one_float4(n):
    for case in base_cases(n) + ur.table_cases("b", [n])[1::4]:               # (table b: the SGD wd variant and AdamW)
        if not case.honours_skip:
            continue
        for k in steps_of(n):
            ratio, _, i = judged(case, k, {"skip_shift": True})
            assert ratio > 1 and i // 4 in (case.skip[0] // 4, case.skip[1] // 4), (case.id, k, ratio, i)


@pytest.mark.parametrize("n", ur.SIZES, ids=ur.SIZE_IDS)
def test_mutant_clipping_omitted_on_the_clipped_step(n):
    for case in base_cases(n):
        assert simulated(case)[0][6].clipped and not simulated(case)[1][6].clipped and float(simulated(case)[1][6].coef) == 1.0
        ratio, which, _ = judged(case, 0, {"no_clip": True})
        assert ratio > 1, (case.id, ratio, which)


@pytest.mark.parametrize("n", ur.SIZES, ids=ur.SIZE_IDS)
def test_mutant_beta2_bias_correction_one_step_late(n):
    for case in base_cases(n)[-2 if n < ur.SIZES[3] else -1:] + ur.count_cases():
        if case.n != n:
            continue
        for k in steps_of(n, range(case.steps)):
            ratio, which, _ = judged(case, k, {"bc2_at_t": True})
            if case.t0 >= 99999:
                continue                                    # 0.999^1e5 is below float32: both corrections are 1, nothing to tell apart
            assert ratio > 1 and which == "dP", (case.id, k, ratio, which)


# ------------------------------------------------------------------------------------------------ the inputs
ALL_CASES = (ur.entry_cases() + ur.table_cases("a", ur.SIZES) + ur.table_cases("b", [ur.SIZES[4]]) + ur.table_cases("c", None)
             + ur.count_cases())


@pytest.mark.parametrize("case", ALL_CASES, ids=lambda c: c.id)
def test_inputs_meet_the_conditions(case):
    sim = ur.simulate(case)
    assert ur.conditions(case, sim) == []
    norms = [float(s[6].norm) for s in sim]
    if case.steps == ur.STEPS:
        r0, r1, r2, r3 = (s[6] for s in sim)
        assert r0.clipped and 0.4 < float(r0.coef) < 0.6                             # above max_norm
        assert not r1.clipped and float(r1.coef) == 1.0 and sim[1][5] > 0             # below it: exactly 1
        assert sim[2][5] == 0.0 and float(r2.coef) == 1.0                             # max_norm = 0: no clipping
        assert norms[3] == 0.0 and float(r3.coef) == 1.0                              # the all-zero gradient
    for s in sim:                                                                     # nothing is left out of the comparison
        ref = s[6]
        for k in ("dP", "S1", "S2"):
            a = ur.allowance({"dP": ref.P, "S1": ref.S1, "S2": ref.S2}[k], ref.mag[k], ref.sens[k], ur.C_FLOOR)
            assert a.shape == (case.n,) and np.isfinite(a).all() and (a > 0).all(), (case.id, k)


def test_case_ids_are_unique_and_the_sizes_are_the_seams():
    ids = [c.id for c in ALL_CASES]
    assert len(set(ids)) == len(ids)
    assert [n // 4 for n in ur.SIZES] == [1, 255, 257, 1024 * 256 + 3, 2048 * 256 + 517]
    t, skip = ur.table_b(ur.SIZES[4], "sgd")
    assert ur.UPDATE_SEAM4 in t.begin4 and t.begin4[-1] == ur.SIZES[4] // 4 - 1
    assert any(b - a == 1 and d - b == 1 and t.group[i] != t.group[i + 1] for i, (a, b, d) in enumerate(zip(t.begin4, t.begin4[1:], t.begin4[2:])))
    assert skip == (4 * (ur.UPDATE_SEAM4 - 1), 4 * (ur.UPDATE_SEAM4 + 1))
    tc, _ = ur.table_c("adam")
    assert len(tc.begin4) == len(tc.lr) == 1024 and len(set(tc.lr)) == 1024
