"""The fused update kernels (csrc/update.hip) restated in plain numpy, the per-element allowance they are held to, and the cases
the CPU and GPU tests share (test_update_ref_cpu.py, test_update_edges_gpu.py).  Nothing here calls torch.optim; the CPU test
pins this module to clip_grad_norm_ + torch.optim.SGD / Adam / AdamW in fp64.

The reference.  ``step`` is one update of one arena, generic in the dtype: float64 is the reference, float32 its twin.
  clip        norm = sqrt(sum g^2); coef = min(max_norm / (norm + 1e-6), 1) when max_norm > 0, else 1; a NaN norm gives a NaN
              coefficient (torch's clamp propagates NaN), an infinite one gives 0
  sgd, plain  b = m b + coef g; p -= lr b                                   (no dampening, no weight decay, no Nesterov)
  sgd         d = coef g + wd p; b = d on the first step, else m b + (1 - dampening) d; p -= lr (d + m b if Nesterov else b);
              momentum 0 zeroes dampening (torch keeps no buffer then)               (torch/optim/sgd.py _single_tensor_sgd)
  adam        g' = coef g + wd p; m += (1 - b1)(g' - m); v = b2 v + (1 - b2) g'^2; t = count + 1;
              p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
  adamw       p *= 1 - lr wd first, then adam with no L2 term
The skip range (a parameter torch never steps) is honoured by the general SGD loop and by AdamW, not by the plain SGD loop or
plain Adam, as the kernels do.  lr and weight decay are one pair or come from a segment table.  Every scalar enters as the
float32 the C ABI passes, widened (``f32``): what is left between kernel and reference is the kernel's arithmetic.

The comparison (``compare``) judges the returned norm, the step dP = P_after - P_before (formed in fp64 from the fp32 arrays)
and each state tensor apart, element by element, against
    allowance = 1/2 ulp32(stored result) + c 2^-24 (sum of the magnitudes of the terms that form the value)
                + where clipping is active: |value(coef (1 + 1e-5)) - value(coef)|, the project's bound on the norm carried
                  through the clipped-gradient term
and returns the worst err / allowance with its index; no maximum over a tensor enters.  The norm is held to 1e-5 of the fp64 norm.
The magnitudes (``Result.mag``), per value:
  sgd    b: |m b| + (1 - dampening)(|coef g| + |wd p|);  dP: lr times the magnitudes of the direction's terms
  adam   m: |m| + (1 - b1)(|g'|_mag + |m|);  v: b2 v + (1 - b2) |g'|_mag^2;
         dP: |p|(1 + lr wd) for AdamW's decay factor, formed as 1 - lr wd before it meets p
             + step_size mag(m) / den                                         (the numerator's error)
             + |upd| (1 + (1 + b1^t) / (1 - b1^t)                            (1 - b1^t is formed from 1 and b1^t)
                      + 1/2 (sqrt(v^) / den)(mag(v) / v + (1 + b2^t) / (1 - b2^t)))       (likewise, under the square root)
  The bias corrections are the one place where the sum of magnitudes is far above the value: 1 - 0.999^1 is 1e-3 formed from
  two numbers near 1, so half an ulp of powf's result is 3e-5 of it.
``c`` is measured (``measure_c``), never fixed: the float32 twin of the same formulas, from the same inputs, against the fp64
reference; the smallest c under which the twin passes, times 4 (the project's margin for FMA contraction and operation order),
floored at 4.  It is measured against the twin, never against the kernel.

Inputs (``Case.inputs``): p0 ~ N(0, 1), gradients ~ N(0, 1); max_norm is half the gradient norm on step 0 (clipped), twice it on
step 1 (coef exactly 1), 0 on step 2 (no clipping), and step 3 has an all-zero gradient.  So that an element the kernel never
touched stands out, the gradients of the float4s at the edges (first, last, both sides of every trip seam, segment boundary and
skip-range end) keep one sign over the steps and |g| >= 0.5; ``conditions`` checks on the CPU, from the reference alone, that on
the steps with a gradient every such element's |dP| is at least 64 allowances and that 99 % of the arena's stepped elements
meet the same (the elements of a skip range on a path that honours it do not step: they are compared for identity; with a
gradient of zero there, a path that ignores the range leaves them at, or next to, where they were, so they are not counted
either).  Where the arena reaches into the second sum-of-squares trip, the first float4 of that trip carries about a fifth
of the squared norm, so that a float4 lost from the norm is not hidden under the norm's own 1e-5."""
import functools

import numpy as np

OPT_BLOCKS, BLOCK, GRID_CAP = 1024, 256, 2048
SUMSQ_SEAM4 = OPT_BLOCKS * BLOCK             # float4 index where sumsq_body's second trip begins
UPDATE_SEAM4 = GRID_CAP * BLOCK              # ... and the update loop's
SIZES = [4, 4 * 255, 4 * 257, 4 * (SUMSQ_SEAM4 + 3), 4 * (UPDATE_SEAM4 + 517)]
SIZE_IDS = ["one_float4", "255_float4", "257_float4", "sumsq_trip2", "update_trip2"]
SIZE_ID = dict(zip(SIZES, SIZE_IDS))
TABLE_C_N = 4 * (1024 + 5)
NORM_BOUND = 1e-5
MARGIN, C_FLOOR = 4.0, 4.0
EDGE_FACTOR, BULK_SHARE = 64.0, 0.99
STEPS = 4


def f32(x):
    """The float32 the ABI passes, widened."""
    return float(np.float32(x))


# ================================================================================================================ tables
class Table:
    """seg_begin (floats, multiples of 4), seg_group, per-group lr and weight decay."""

    def __init__(self, n, begin4, group, lr, wd):
        self.n, self.begin4, self.group = n, [int(b) for b in begin4], [int(g) for g in group]
        used = sorted(set(self.group))                      # (a table scaled to a tiny arena keeps fewer segments: renumber)
        self.group = [used.index(g) for g in self.group]
        self.lr, self.wd = [lr[g] for g in used], [wd[g] for g in used]
        assert self.begin4[0] == 0 and all(a < b for a, b in zip(self.begin4, self.begin4[1:])) and self.begin4[-1] < n // 4

    seg_begin = property(lambda self: [4 * b for b in self.begin4])

    def per_element(self, values, dtype):
        ends = self.begin4[1:] + [self.n // 4]
        out = np.empty(self.n, dtype=dtype)
        for b, e, g in zip(self.begin4, ends, self.group):
            out[4 * b:4 * e] = f32(values[g])
        return out

    def with_lr(self, lr):
        t = Table.__new__(Table)
        t.__dict__.update(self.__dict__)
        t.lr = list(lr)
        return t


A_FRAC = [0, 4100 / 262144, 70000 / 262144, 0.5, 200004 / 262144]
A_GROUP, A_WD = [0, 1, 2, 0, 1], [1e-2, 0.0, 1e-3]
A_LR = {"sgd": [0.05, 0.01, 0.002], "adam": [1e-2, 3e-3, 1e-3]}


def _dedup(begin4, group, n4):
    b_out, g_out = [], []
    for b, g in zip(begin4, group):
        if b < n4 and (not b_out or b > b_out[-1]):
            b_out.append(b)
            g_out.append(g)
    return b_out, g_out


def table_a(n, family, wd=None):
    """The 5-segment, 3-group table of test_param_groups_gpu.py scaled to n floats, and its skip range (floats)."""
    n4 = n // 4
    begin4, group = _dedup([min(int(round(f * n4)), n4 - 1) for f in A_FRAC], A_GROUP, n4)
    skip4 = (n4 // 32, 3 * n4 // 64)
    return Table(n, begin4, group, A_LR[family], A_WD if wd is None else wd), _skip(skip4)


def table_b(n, family):
    """Boundaries on the seams: a segment that begins on the update's trip seam (the arena's middle where it has no second trip),
    the last float4 a segment of its own, two adjacent one-float4 segments in different groups, and a skip range from one float4
    before the seam to one behind it."""
    n4 = n // 4
    seam = UPDATE_SEAM4 if n4 > UPDATE_SEAM4 + 1 else n4 // 2
    a = min(1000, n4 // 4)
    begin4, group = _dedup([0, a, a + 1, a + 2, seam, n4 - 1], [0, 1, 2, 0, 1, 2], n4)
    skip4 = (seam - 1, seam + 1) if seam - 1 >= 1 and seam + 1 <= n4 - 1 else (0, 0)
    return Table(n, begin4, group, A_LR[family], A_WD), _skip(skip4)


def table_c(family):
    """GROUPS_MAX_SEGMENTS = 1024 segments in 1024 groups, every one a float4 long (the last one runs to the arena's end), each
    with its own lr and weight decay: an off-by-one of the binary search shows at every index."""
    k = 1024
    scale = 1.0 if family == "sgd" else 0.2
    lr = [scale * (0.02 + 0.03 * ((i * 37) % k) / k) for i in range(k)]
    wd = [1e-2 * (1 + (i * 101) % k) / k for i in range(k)]
    return Table(TABLE_C_N, list(range(k)), list(range(k)), lr, wd), (0, 0)


def _skip(skip4):
    return (4 * skip4[0], 4 * skip4[1]) if skip4[1] > skip4[0] else (0, 0)


# ================================================================================================================ cases
class Case:
    """One entry point, one arena size, one set of options.  entry: sgd (slnlp_clip_sgd_step), sgd_ex, adam, adamw, sgd_groups,
    adam_groups (``decoupled`` chooses AdamW)."""

    def __init__(self, entry, n, *, lr=None, wd=0.0, momentum=0.9, dampening=0.0, nesterov=False, betas=(0.9, 0.999), eps=1e-8,
                 decoupled=False, table=None, skip=(0, 0), t0=0, steps=STEPS, random_state=False, tag=""):
        self.entry, self.n, self.table, self.skip, self.t0, self.steps = entry, n, table, tuple(skip), t0, steps
        self.family = "sgd" if entry.startswith("sgd") else "adam"
        self.decoupled = entry == "adamw" or (entry == "adam_groups" and decoupled)
        self.lr = (0.05 if self.family == "sgd" else 1e-2) if lr is None else lr
        self.wd, self.momentum, self.dampening, self.nesterov, self.betas, self.eps = wd, momentum, dampening, nesterov, betas, eps
        self.random_state = random_state or t0 > 0
        self.tag = tag
        assert entry in ("sgd", "sgd_ex", "adam", "adamw", "sgd_groups", "adam_groups") and (table is not None) == entry.endswith("groups")

    @property
    def id(self):
        return "-".join(x for x in (self.entry + ("w" if self.entry == "adam_groups" and self.decoupled else ""), self.tag,
                                    SIZE_ID.get(self.n, str(self.n))) if x)

    # ---- what the kernels decide -------------------------------------------------------------------------------------
    @property
    def general(self):
        """The general SGD loop: dampening (with momentum), Nesterov, or any weight decay (of any group)."""
        damp = self.dampening if self.momentum != 0 else 0.0
        any_wd = any(w != 0 for w in self.table.wd) if self.table else self.wd != 0
        return self.family == "sgd" and (damp != 0 or any_wd or self.nesterov)

    @property
    def honours_skip(self):
        return self.skip[1] > self.skip[0] and (self.general or self.decoupled)

    def rates(self, dtype=np.float64):
        if self.table:
            return self.table.per_element(self.table.lr, dtype), self.table.per_element(self.table.wd, dtype)
        return dtype(f32(self.lr)), dtype(f32(self.wd))

    def live(self):
        """Elements outside the skip range (all of them without one)."""
        m = np.ones(self.n, dtype=bool)
        m[self.skip[0]:self.skip[1]] = False
        return m

    def edge_float4s(self):
        n4 = self.n // 4
        cand = {0, n4 - 1, SUMSQ_SEAM4 - 1, SUMSQ_SEAM4, UPDATE_SEAM4 - 1, UPDATE_SEAM4}
        for b in (self.table.begin4 if self.table else []):
            cand |= {b - 1, b}
        if self.skip[1] > self.skip[0]:
            cand |= {self.skip[0] // 4 - 1, self.skip[0] // 4, self.skip[1] // 4 - 1, self.skip[1] // 4}
        return sorted(i for i in cand if 0 <= i < n4)

    # ---- inputs ------------------------------------------------------------------------------------------------------
    def inputs(self):
        """-> p0, s1, s2 (float32), [gradient per step], [max_norm per step]."""
        n = self.n
        p0 = _normal(n, 1).copy()
        if self.random_state:
            s1, s2 = (_normal(n, 3) * np.float32(1e-3)), np.abs(_normal(n, 4) * np.float32(1e-3))
        else:
            s1, s2 = np.zeros(n, np.float32), np.zeros(n, np.float32)
        edges = np.concatenate([np.arange(4 * i, 4 * i + 4) for i in self.edge_float4s()])
        sign = np.where(_normal(n, 20)[edges] < 0, np.float32(-1), np.float32(1))
        grads, max_norms = [], []
        for k in range(self.steps):
            if k == 3:
                grads.append(np.zeros(n, np.float32))
                max_norms.append(0.5)
                continue
            g = _normal(n, 20 + k).copy()
            g[edges] = sign * np.maximum(np.abs(g[edges]), np.float32(0.5))
            if n // 4 > SUMSQ_SEAM4:
                g[4 * SUMSQ_SEAM4:4 * SUMSQ_SEAM4 + 4] *= np.float32(np.sqrt(n / 16.0))
            g[self.skip[0]:self.skip[1]] = 0                                  # a parameter that gets no gradient
            norm = float(np.sqrt(np.sum(g.astype(np.float64) ** 2)))
            grads.append(g)
            max_norms.append([f32(0.5 * norm), f32(2.0 * norm), 0.0][k % 3])
        return p0, s1, s2, grads, max_norms


@functools.lru_cache(maxsize=16)
def _normal(n, seed):
    a = np.random.default_rng(1000 * seed + 7).standard_normal(n).astype(np.float32)
    a.setflags(write=False)
    return a


SGD_OPTIONS = {"plain": {}, "nesterov": dict(nesterov=True), "dampening": dict(dampening=0.3), "wd": dict(wd=1e-2),
               "nesterov_wd": dict(nesterov=True, wd=1e-2), "momentum0_wd": dict(momentum=0.0, wd=1e-2)}
ADAM_OPTIONS = {f"b2_{b2}-wd{wd:g}": dict(betas=(0.9, b2), wd=wd) for b2 in (0.999, 0.99) for wd in (0.0, 1e-2)}


def default_skip(n):
    n4 = n // 4
    return _skip((n4 // 3, n4 // 3 + n4 // 16 + 1)) if n4 >= 8 else (0, 0)


def entry_cases(sizes=SIZES):
    """Every ungrouped entry point at every size, with every option the GPU test runs."""
    out = []
    for n in sizes:
        out.append(Case("sgd", n, random_state=True))
        for tag, kw in SGD_OPTIONS.items():
            out.append(Case("sgd_ex", n, tag=tag, skip=default_skip(n) if tag != "plain" else (0, 0), **kw))
        for tag, kw in ADAM_OPTIONS.items():
            out.append(Case("adam", n, tag=tag, **kw))
            out.append(Case("adamw", n, tag=tag, skip=default_skip(n), **kw))
    return out


GROUP_VARIANTS = [("sgd_groups", "plain", dict(wd=[0.0, 0.0, 0.0])), ("sgd_groups", "wd", {}), ("sgd_groups", "nesterov", dict(nesterov=True)),
                  ("sgd_groups", "dampening", dict(dampening=0.3)), ("adam_groups", "", {}), ("adam_groups", "", dict(decoupled=True))]


def table_cases(which, sizes):
    """Tables (a) / (b) at ``sizes`` through both grouped entry points; (c) at its own size."""
    out = []
    for n in ([TABLE_C_N] if which == "c" else sizes):
        for entry, tag, kw in GROUP_VARIANTS:
            kw = dict(kw)
            family = "sgd" if entry.startswith("sgd") else "adam"
            wd = kw.pop("wd", None)
            if which == "a":
                table, skip = table_a(n, family, wd)
            elif which == "b":
                table, skip = table_b(n, family)
                if wd is not None:
                    table.wd = wd[:len(table.wd)]
            else:
                table, skip = table_c(family)
                if wd is not None:
                    table.wd = [0.0] * len(table.wd)
            out.append(Case(entry, n, table=table, skip=skip, tag="-".join(x for x in ("table_" + which, tag) if x), **kw))
    return out


def count_cases():
    """Adam and AdamW from a device step count of 999 and of 99 999, two steps each."""
    return [Case(entry, n, t0=t0, steps=2, tag=f"from{t0}", skip=default_skip(n) if entry == "adamw" else (0, 0), wd=1e-2)
            for entry in ("adam", "adamw") for t0 in (999, 99999) for n in (SIZES[2], SIZES[4])]


# ================================================================================================================ reference
class Result:
    """P, S1, S2 after the step, dP, norm, coef, whether clipping was active, and mag / sens per judged value."""


def clip(G, max_norm, dtype, mutate):
    with np.errstate(all="ignore"):
        sq = G * G
        if "norm_drops_float4" in mutate:
            i = mutate["norm_drops_float4"]
            sq = sq.copy()
            sq[4 * i:4 * i + 4] = 0
        if "norm_drops_trip2" in mutate:
            sq = sq.copy()
            sq[4 * SUMSQ_SEAM4:8 * SUMSQ_SEAM4] = 0
        norm = np.sqrt(np.sum(sq, dtype=dtype))
        if max_norm > 0 and "no_clip" not in mutate:
            q = dtype(f32(max_norm)) / (norm + dtype(f32(1e-6)))
            coef = q if np.isnan(q) else min(q, dtype(1))
        else:
            coef = dtype(1)
    return dtype(norm), dtype(coef)


def step(case, P, G, S1, S2, t0, max_norm, *, dtype=np.float64, mutate=None, _coef_scale=None):
    """One update in ``dtype`` from (float32) inputs -> Result.  ``mutate``: a deliberately wrong variant (the CPU test's proof
    that the comparison bites)."""
    mutate = mutate or {}
    P, G, S1, S2 = (np.asarray(a).astype(dtype) for a in (P, G, S1, S2))
    one = dtype(1)
    r = Result()
    r.norm, coef = clip(G, max_norm, dtype, mutate)
    r.coef, r.clipped = coef, bool(max_norm > 0 and coef < 1)
    if _coef_scale is not None:
        coef = coef * dtype(_coef_scale)
    lr, wd = case.rates(dtype)
    if "neighbour_lr" in mutate:                                  # the float4 at a boundary takes the rate of the segment before it
        b = mutate["neighbour_lr"]
        lr = lr.copy()
        lr[4 * b:4 * b + 4] = lr[4 * b - 1]
    skip = case.skip
    if "skip_shift" in mutate and skip[1] > skip[0]:
        skip = (skip[0] + 4, skip[1] + 4)
    with np.errstate(all="ignore"):
        gc = coef * G
        a_gc = np.abs(gc)
        if case.family == "sgd":
            m = dtype(f32(case.momentum))
            if not case.general:
                nS1 = m * S1 + gc
                mag_S1 = np.abs(m * S1) + a_gc
                nP = P - lr * nS1
                mag_dP = lr * mag_S1
                honour = False
            else:
                damp = dtype(f32(case.dampening)) if case.momentum != 0 else dtype(0)
                first = t0 == 0 and "never_first" not in mutate
                d = gc + wd * P
                mag_d = a_gc + np.abs(wd * P)
                if first:
                    nS1, mag_S1 = d, mag_d
                else:
                    nS1 = m * S1 + (one - damp) * d
                    mag_S1 = np.abs(m * S1) + (one - damp) * mag_d
                if case.nesterov:
                    dirn, mag_dir = d + m * nS1, mag_d + m * mag_S1
                else:
                    dirn, mag_dir = nS1, mag_S1
                nP = P - lr * dirn
                mag_dP = lr * mag_dir
                honour = True
            nS2, mag_S2 = S2, np.zeros_like(S2)
        else:
            b1, b2, eps = dtype(f32(case.betas[0])), dtype(f32(case.betas[1])), dtype(f32(case.eps))
            t = dtype(t0 + 1)
            p1, p2 = np.power(b1, t), np.power(b2, dtype(t0) if "bc2_at_t" in mutate else t)
            bc1, bc2 = one - p1, one - p2
            if case.decoupled:
                w1 = P * (one - lr * wd)
                g1, mag_g = gc, a_gc
                mag_w = np.abs(P) * (one + lr * wd)
            else:
                w1 = P
                g1 = gc + wd * P
                mag_g = a_gc + np.abs(wd * P)
                mag_w = 0
            nS1 = S1 + (one - b1) * (g1 - S1)
            mag_S1 = np.abs(S1) + (one - b1) * (mag_g + np.abs(S1))
            nS2 = b2 * S2 + (one - b2) * g1 * g1
            mag_S2 = b2 * np.abs(S2) + (one - b2) * mag_g * mag_g
            sq = np.sqrt(nS2) / np.sqrt(bc2)
            den = sq + eps
            ss = lr / bc1
            upd = ss * (nS1 / den)
            nP = w1 - upd
            cond_v = np.where(nS2 > 0, mag_S2 / np.where(nS2 > 0, nS2, one), 0)
            mag_dP = mag_w + ss * mag_S1 / den + np.abs(upd) * (one + (one + p1) / bc1 + dtype(0.5) * (sq / den) * (cond_v + (one + p2) / bc2))
            honour = case.decoupled
        if honour and skip[1] > skip[0]:
            s = slice(skip[0], skip[1])
            nP, nS1 = nP.copy(), nS1.copy()
            nP[s], nS1[s] = P[s], S1[s]
            mag_dP = mag_dP.copy() if isinstance(mag_dP, np.ndarray) else mag_dP
            for mg in (mag_dP, mag_S1):
                mg[s] = 0
            if case.family == "adam":
                nS2 = nS2.copy()
                nS2[s], mag_S2[s] = S2[s], 0
        if "untouched_float4" in mutate:
            i = mutate["untouched_float4"]
            for new, old in ((nP, P), (nS1, S1), (nS2, S2)):
                if new is not old:
                    new[4 * i:4 * i + 4] = old[4 * i:4 * i + 4]
        r.P, r.S1, r.S2, r.dP = nP, nS1, nS2, nP - P
        r.mag = {"dP": mag_dP, "S1": mag_S1, "S2": mag_S2}
    return r


def reference(case, P, G, S1, S2, t0, max_norm):
    """The fp64 step with, where clipping is active, what a norm off by its bound moves each value by."""
    r = step(case, P, G, S1, S2, t0, max_norm)
    zero = {"dP": 0.0, "S1": 0.0, "S2": 0.0}
    if r.clipped and r.coef > 0:
        q = step(case, P, G, S1, S2, t0, max_norm, _coef_scale=1.0 + NORM_BOUND)
        with np.errstate(all="ignore"):
            r.sens = {"dP": np.abs(q.dP - r.dP), "S1": np.abs(q.S1 - r.S1), "S2": np.abs(q.S2 - r.S2)}
    else:
        r.sens = zero
    return r


# ================================================================================================================ comparison
def ulp32(x):
    with np.errstate(all="ignore"):
        return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


def allowance(stored, mag, sens, c):
    with np.errstate(all="ignore"):
        rest = c * 2.0 ** -24 * mag + sens
        return 0.5 * ulp32(np.abs(stored) + rest) + rest


def _ratio(got, ref, allow):
    with np.errstate(all="ignore"):
        got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
        same = (got == ref) | (np.isnan(got) & np.isnan(ref))
        finite = np.isfinite(got) & np.isfinite(ref)
        return np.where(same, 0.0, np.where(finite, np.abs(got - ref) / allow, np.inf))


def values(P_before, P, S1, S2):
    """What is judged, from the float32 arrays a kernel (or a mutant) left."""
    return {"dP": np.asarray(P, np.float32).astype(np.float64) - np.asarray(P_before, np.float32).astype(np.float64),
            "S1": np.asarray(S1, np.float32).astype(np.float64), "S2": np.asarray(S2, np.float32).astype(np.float64)}


def compare(ref, P_before, P, S1, S2, norm, c):
    """-> (worst err / allowance, which value, its index), {value: (ratio, index)}.  ``ref``: ``reference``'s Result."""
    got = values(P_before, P, S1, S2)
    stored = {"dP": ref.P, "S1": ref.S1, "S2": ref.S2}
    want = {"dP": ref.dP, "S1": ref.S1, "S2": ref.S2}
    per = {}
    for k in got:
        ratio = _ratio(got[k], want[k], allowance(stored[k], ref.mag[k], ref.sens[k], c))
        i = int(np.argmax(ratio))
        per[k] = (float(ratio[i]), i)
    rn, gn = float(ref.norm), float(norm)
    if np.isfinite(rn) and np.isfinite(gn):
        per["norm"] = (abs(gn - rn) / (NORM_BOUND * rn) if rn > 0 else (0.0 if gn == 0 else np.inf), 0)
    else:
        per["norm"] = (0.0 if (gn == rn or (np.isnan(gn) and np.isnan(rn))) else np.inf, 0)
    worst = max(per, key=lambda k: per[k][0])
    return (per[worst][0], worst, per[worst][1]), per


def arithmetic_share(ref, P_before, P, S1, S2, c):
    """Over the 2 M elements of the large arenas a correctly rounded store comes arbitrarily close to the half ulp that is the
    allowance's first part, so the worst err / allowance sits just under 1 and says little.  This is the other figure: the
    largest share of the allowance's remaining parts that an element needs once its half ulp is taken off (0: the stores'
    rounding accounts for every difference)."""
    got = values(P_before, P, S1, S2)
    stored = {"dP": ref.P, "S1": ref.S1, "S2": ref.S2}
    want = {"dP": ref.dP, "S1": ref.S1, "S2": ref.S2}
    share = 0.0
    with np.errstate(all="ignore"):
        for k in got:
            rest = c * 2.0 ** -24 * ref.mag[k] + ref.sens[k]
            over = np.abs(got[k] - want[k]) - 0.5 * ulp32(np.abs(stored[k]) + rest)
            s = np.where((over > 0) & np.isfinite(want[k]), over / rest, 0.0)
            share = max(share, float(np.nanmax(s)))
    return share


def measure_c(case, ref, P, G, S1, S2, t0, max_norm):
    """4 x the smallest c under which the float32 twin of ``step``, from the same inputs, passes against ``ref``; at least 4."""
    twin = step(case, P, G, S1, S2, t0, max_norm, dtype=np.float32)
    got = values(P, twin.P, twin.S1, twin.S2)
    stored = {"dP": ref.P, "S1": ref.S1, "S2": ref.S2}
    want = {"dP": ref.dP, "S1": ref.S1, "S2": ref.S2}
    need = 0.0
    with np.errstate(all="ignore"):
        for k in got:
            over = np.abs(got[k] - want[k]) - 0.5 * ulp32(stored[k]) - ref.sens[k]
            mag = np.broadcast_to(ref.mag[k], over.shape)
            c = np.where(over > 0, over / np.where(mag > 0, 2.0 ** -24 * mag, np.nan), 0.0)
            c = c[np.isfinite(want[k])]
            if c.size:
                assert not np.isnan(c).any(), f"{case.id}: the float32 twin differs at an element of {k} whose terms are all zero"
                need = max(need, float(c.max()))
    return max(C_FLOOR, MARGIN * need)


# ================================================================================================================ the chain, on the CPU
def simulate(case):
    """The case's steps from the reference alone, its state rounded to float32 after every step as the kernels store it ->
    [(P, G, S1, S2, t0, max_norm, ref)] per step."""
    P, S1, S2, grads, max_norms = case.inputs()
    out = []
    for k, (G, mx) in enumerate(zip(grads, max_norms)):
        ref = reference(case, P, G, S1, S2, case.t0 + k, mx)
        out.append((P, G, S1, S2, case.t0 + k, mx, ref))
        P, S1, S2 = ref.P.astype(np.float32), ref.S1.astype(np.float32), ref.S2.astype(np.float32)
    return out


def conditions(case, sim=None):
    """On every step with a gradient: [(step, problem)] -- empty when the inputs meet the conditions of the module docstring."""
    problems = []
    live = case.live()
    edges = np.concatenate([np.arange(4 * i, 4 * i + 4) for i in case.edge_float4s()])
    edges = edges[live[edges]]
    assert edges.size, case.id
    for k, (P, G, S1, S2, t0, mx, ref) in enumerate(sim or simulate(case)):
        if not G.any():
            continue
        c = measure_c(case, ref, P, G, S1, S2, t0, mx)
        ok = np.abs(ref.dP) >= EDGE_FACTOR * allowance(ref.P, ref.mag["dP"], ref.sens["dP"], c)
        if not ok[edges].all():
            problems.append((k, f"edge elements {edges[~ok[edges]].tolist()} step by less than {EDGE_FACTOR:g} allowances"))
        share = float(ok[live].mean())
        if share < BULK_SHARE:
            problems.append((k, f"only {share:.4f} of the stepped elements step by {EDGE_FACTOR:g} allowances"))
    return problems
