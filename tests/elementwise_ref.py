"""Plain references for the kernels of csrc/elementwise.hip (embedding gather / scatter-add, LayerNorm, the log-softmax / NLL
criterion) and the case table that tests/test_elementwise_edges_gpu.py runs and tests/test_elementwise_ref_cpu.py judges.

The fp64 references are torch on the CPU; `embed_bwd_tree` and `ln_reduce_tree` restate the kernels' documented summation
orders in float32 numpy (plain IEEE adds, nothing contracted), for the bit-for-bit checks.  No device anywhere in this file."""
import math

import numpy as np
import torch

F32 = np.float32

# the project's bounds (tests/test_kernels_gpu.py), all relative to the reference tensor's maximum
TOL_EMBED_FWD, TOL_EMBED_BWD, TOL_LOSS_GRAD, TOL_LN_FWD, TOL_LN_BWD = 1e-6, 1e-5, 1e-5, 2e-5, 5e-5
TOL_STATS = 2e-5             # LayerNorm (mean, rstd), of their own maxima
TOL_LOGP = 1e-6


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).float()


def err(got, ref):
    """max |got - ref| / max |ref| in float64; a reference that is exactly zero admits exactly zero only."""
    got, ref = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(ref).detach().double().cpu()
    top = float(ref.abs().max())
    if top == 0.0:
        return 0.0 if float(got.abs().max()) == 0.0 else math.inf
    e = float((got - ref).abs().max()) / top
    return e if e == e else math.inf                     # a NaN where the reference has a number is an infinite error


def row_err(got, ref):
    """The embedding gradient's metric: each table row against ITS OWN maximum, the worst row.  (Against the tensor maximum a
    wrong rare row hides under the hot id's row, which is a sum of hundreds of tokens.)"""
    return max(err(g, r) for g, r in zip(torch.as_tensor(got), torch.as_tensor(ref)))


# ======================================================================================================== embedding
def token_ids(ids):
    """ids [B, S] -> the id of every position m = s * B + b, [S * B]."""
    return ids.T.reshape(-1)


def embed_fwd_ref(ids, table, pe=None, *, scale=None, mask=None, p=0.0, nan_idx=-1):
    """out[s * B + b] = table[ids[b, s]] * scale + pe[s], a zero row for an id outside [0, V); then mask / (1 - p); then NaN rows
    where the id is nan_idx (>= 0; negative: none).  fp64 [S * B, E]."""
    B, S = ids.shape
    V, E = table.shape
    tok = token_ids(ids)
    ok = (tok >= 0) & (tok < V)
    out = table.double()[tok.clamp(0, V - 1)] * ok[:, None] * (math.sqrt(E) if scale is None else scale)
    if pe is not None:
        out = out + pe[:S].double().repeat_interleave(B, 0)
    if mask is not None:
        out = out * mask.double() / (1.0 - p)
    if nan_idx >= 0:                                     # -1 means "none", and is no match for an id of -1 (outside the table: a zero row)
        out[tok == nan_idx] = math.nan
    return out


def embed_bwd_ref(ids, dx, V, *, scale=None, zero_row=-1, mask=None, p=0.0):
    """dtable[v] = scale * sum over the positions with id v of dx (* mask / (1 - p)); ids outside [0, V) give nothing; zero_row
    cleared.  fp64 [V, E]."""
    E = dx.shape[1]
    tok = token_ids(ids)
    ok = (tok >= 0) & (tok < V)
    g = dx.double() if mask is None else dx.double() * mask.double() / (1.0 - p)
    dt = torch.zeros(V, E, dtype=torch.float64).index_add_(0, tok[ok], g[ok]) * (math.sqrt(E) if scale is None else scale)
    if 0 <= zero_row < V:
        dt[zero_row] = 0.0
    return dt


def _ordered_sum(rows, E):
    acc = np.zeros(E, F32)
    for r in rows:
        acc = acc + r
    return acc


def embed_bwd_tree(ids, dx, V, *, scale=None, zero_row=-1, n_tokens=None, col_limit=None):
    """The kernels' summation order in float32 (no dropout): chunks of 64 positions m = s * B + b; inside a chunk wave w adds the
    positions [16 w, 16 w + 16) of an id in increasing order from +0, and the four wave sums are added in wave order; the chunk
    partials of an id, in chunk order, are cut into four runs of ceil(n / 4), each added in order from +0, the runs added in order;
    the result times scale.  float32 [V, E].

    n_tokens / col_limit restate two faults for the CPU tests: only the first n_tokens positions are summed (a dropped last
    chunk), only the columns below col_limit are written (a skipped column trip)."""
    E = dx.shape[1]
    g = dx.numpy().astype(F32)
    tok = token_ids(ids).numpy()
    tok = np.where((tok >= 0) & (tok < V), tok, -1)
    M = len(tok) if n_tokens is None else n_tokens
    parts = [[] for _ in range(V)]
    for m0 in range(0, M, 64):
        n = min(64, M - m0)
        acc = np.zeros((4, V, E), F32)
        for k in range(n):
            if tok[m0 + k] >= 0:
                acc[k // 16, tok[m0 + k]] += g[m0 + k]
        r = ((acc[0] + acc[1]) + acc[2]) + acc[3]
        for t in np.unique(tok[m0:m0 + n]):
            if t >= 0:
                parts[t].append(r[t])
    sc = F32(math.sqrt(E) if scale is None else scale)
    out = np.zeros((V, E), F32)
    for t in range(V):
        n = len(parts[t])
        if n == 0:
            continue
        per = (n + 3) // 4
        a = [_ordered_sum(parts[t][w * per:min((w + 1) * per, n)], E) for w in range(4)]
        out[t] = (((a[0] + a[1]) + a[2]) + a[3]) * sc
    if 0 <= zero_row < V:
        out[zero_row] = 0.0
    if col_limit is not None:
        out[:, col_limit:] = 0.0
    return torch.from_numpy(out)


# ======================================================================================================== LayerNorm
def layernorm_ref(x, gamma, beta, eps=1e-5, dy=None):
    """fp64: y, mean, rstd (eps added to the biased variance) and, given dy, dx, dgamma, dbeta."""
    x, gamma, beta = x.double(), gamma.double(), beta.double()
    mean = x.mean(1)
    rstd = 1.0 / torch.sqrt(((x - mean[:, None]) ** 2).mean(1) + eps)
    xhat = (x - mean[:, None]) * rstd[:, None]
    out = dict(y=xhat * gamma + beta, mean=mean, rstd=rstd, xhat=xhat)
    if dy is not None:
        dy = dy.double()
        gd = dy * gamma
        out["dx"] = rstd[:, None] * (gd - gd.mean(1, keepdim=True) - xhat * (gd * xhat).mean(1, keepdim=True))
        out["dgamma"], out["dbeta"] = (dy * xhat).sum(0), dy.sum(0)
    return out


def ln_partial_chunk(rows):
    """Rows per chunk of the (dgamma, dbeta) partial sums: 16, doubled while that would be more than 1024 chunks."""
    c = 16
    while -(-rows // c) > 1024:
        c *= 2
    return c


def ln_partial_ref(dy, xhat, rows, full_rows, *, drop_tail_of=None, chunk=None):
    """fp64 chunk sums [nblk, 2, E] of the first `rows` rows in the chunk geometry of `full_rows`: [j][0] = sum dy xhat,
    [j][1] = sum dy over chunk j's rows; chunks past the last row are zero.  drop_tail_of = 8 restates a fault for the CPU tests:
    the rows a loop unrolled by 8 leaves to its tail are not added."""
    chunk = ln_partial_chunk(max(full_rows, 1)) if chunk is None else chunk
    nblk = -(-full_rows // chunk)
    out = torch.zeros(nblk, 2, dy.shape[1], dtype=torch.float64)
    for j in range(nblk):
        r0, r1 = j * chunk, min((j + 1) * chunk, rows)
        if drop_tail_of and r1 > r0:
            r1 = r0 + (r1 - r0) // drop_tail_of * drop_tail_of
        if r1 > r0:
            out[j, 0] = (dy[r0:r1].double() * xhat[r0:r1].double()).sum(0)
            out[j, 1] = dy[r0:r1].double().sum(0)
    return out


def ln_reduce_tree(partial):
    """ln_param_reduce's order in float32: group g adds the partials g, g + 4, ... in increasing order from +0, then
    (r0 + r1) + (r2 + r3).  partial [nblk, 2, E] -> (dgamma, dbeta) float32 [E]."""
    p = partial.numpy().astype(F32)
    r = [_ordered_sum(p[g::4], p.shape[1:]) for g in range(4)]
    out = (r[0] + r[1]) + (r[2] + r[3])
    return torch.from_numpy(out[0].copy()), torch.from_numpy(out[1].copy())


def layernorm_fwd_f32(x, gamma, beta, eps=1e-5, one_pass=False):
    """The forward in float32 numpy: two-pass statistics as the kernel computes them, or (one_pass) var = E[x^2] - mean^2 -- the
    restatement whose error on an offset input the forward bound must not admit."""
    x, gamma, beta = x.numpy().astype(F32), gamma.numpy().astype(F32), beta.numpy().astype(F32)
    E = F32(x.shape[1])
    mean = x.sum(1, dtype=F32) / E
    if one_pass:
        var = (x * x).sum(1, dtype=F32) / E - mean * mean
    else:
        var = ((x - mean[:, None]) ** 2).sum(1, dtype=F32) / E
    rstd = F32(1) / np.sqrt(var + F32(eps))
    return torch.from_numpy((x - mean[:, None]) * rstd[:, None] * gamma + beta)


# ============================================================================================================== loss
def lsm_nll_ref(logits, y, ignore_index, *, weight=None, label_smoothing=0.0, reduction="mean", count_ignored=False):
    """logp = log_softmax(logits); CrossEntropyLoss(weight, ignore_index, label_smoothing, reduction) applied to logp (so through
    a second log_softmax l), targets outside [0, V) counted as ignored:
        loss = sum_kept [(1 - eps) w[y_i] (-l[i, y_i]) + (eps / V) sum_c w[c] (-l[i, c])] / D,  D = sum_kept w[y_i] or 1 ("sum")
    -> fp64 (logp [B, V], loss scalar (NaN when D = 0), d loss / d logits [B, V], exactly zero in ignored rows).
    count_ignored restates a fault for the CPU tests: D counts every row of the batch."""
    x = logits.double()
    B, V = x.shape
    w = torch.ones(V, dtype=torch.float64) if weight is None else weight.double()
    eps = float(label_smoothing)
    logp = torch.log_softmax(x, -1)
    l = torch.log_softmax(logp, -1)
    kept = (y != ignore_index) & (y >= 0) & (y < V)
    yc = y.clamp(0, V - 1)
    wy = w[yc] * kept
    a = (eps / V) * w[None, :].repeat(B, 1)
    a[torch.arange(B), yc] += (1.0 - eps) * w[yc]
    a = a * kept[:, None]
    if reduction == "sum":
        D = torch.tensor(1.0, dtype=torch.float64)
    else:
        D = (w[yc] if count_ignored else wy).sum()
    loss = -(a * l).sum() / D
    dlogp = (torch.exp(l) * a.sum(1, keepdim=True) - a) / D
    dlogits = dlogp - torch.exp(logp) * dlogp.sum(1, keepdim=True)
    dlogits[~kept] = 0.0
    return logp, loss, dlogits


def lsm_nll_f32(logits, y, ignore_index, subtract_max=True):
    """The plain criterion in float32 torch on the CPU, the kernel's formulas; subtract_max False restates the fault the saturated
    case guards against (a softmax that forgot its max) -> (logp, loss, dlogits)."""
    x = logits.float()
    B, V = x.shape
    m = x.max(1, keepdim=True).values if subtract_max else torch.zeros(B, 1)
    lp = x - (m + torch.log(torch.exp(x - m).sum(1, keepdim=True)))
    m2 = lp.max(1, keepdim=True).values if subtract_max else torch.zeros(B, 1)
    lse2 = m2 + torch.log(torch.exp(lp - m2).sum(1, keepdim=True))
    kept = (y != ignore_index) & (y >= 0) & (y < V)
    onehot = torch.zeros(B, V)
    onehot[torch.arange(B), y.clamp(0, V - 1)] = 1.0
    wgt = kept.float()[:, None] / kept.float().sum()
    dlp = wgt * (torch.exp(lp - lse2) - onehot)
    loss = (-(lp - lse2)[torch.arange(B), y.clamp(0, V - 1)] * kept).sum() / kept.float().sum()
    return lp, loss, dlp - torch.exp(lp) * dlp.sum(1, keepdim=True)


# ======================================================================================================== the cases
# ---- embedding forward: (B, S, V, E)
EMBED_FWD_STRIDE = (33, 64, 40, 1024)       # 540672 float4 > 2048 workgroups x 256: the grid-stride trip runs
EMBED_FWD_SMALL = (7, 5, 30, 4)             # ids outside [0, V), no positional table, padded ids, nan_idx under dropout
ID_PAD = 3                                  # extra columns of the padded id matrix: ld_ids = S + 3

# ---- embedding backward, chunk + combine path: (B, S, V, E, how the ids are drawn)
EMBED_BWD_CASES = [
    (5, 13, 40, 512, "hot"),        # M = 65: the first size past one chunk; two column trips
    (50, 48, 300, 260, "hot"),      # the last column trip has one live lane
    (50, 48, 300, 1024, "hot"),     # four column trips
    (7, 19, 30, 4, "hot"),          # smallest E
    (7, 19, 200, 64, "perm"),       # every id once
    (7, 19, 30, 64, "equal"),       # every id equal
    (256, 256, 8, 4, "every"),      # 65536 tokens; id 0 ~40 % of them and in every chunk: a combine list of exactly 1024 entries
]
EMBED_BWD_ONE_CHUNK = [(50, 1, 202, 512), (64, 1, 40, 128)]      # M <= 64: chunk path (mask given) == single launch (no mask)


def embed_case_id(case):
    return "x".join(str(v) for v in case)


def embed_ids(B, S, V, kind="hot", *, seed=0, oor=False):
    """[B, S] ids.  hot: id 0 for ~40 % of the positions (the <pad> row), the rest uniform, so rare ids occur once or never;
    perm: every id at most once; equal: one id; every: hot, and id 0 at the first position of every 64-position chunk.
    oor: a tenth of the positions, and positions 1 to 3 for certain, become -1, V or V + 5."""
    g = torch.Generator().manual_seed(1000 + seed + B * S + V)
    M = B * S
    if kind == "perm":
        tok = torch.randperm(V, generator=g)[:M]
    elif kind == "equal":
        tok = torch.full((M,), V // 2, dtype=torch.int64)
    else:
        tok = torch.randint(0, V, (M,), generator=g)
        tok[torch.rand(M, generator=g) < 0.4] = 0
        if kind == "every":
            tok[::64] = 0
    if oor:
        bad = torch.tensor([-1, V, V + 5])[torch.randint(0, 3, (M,), generator=g)]
        where = torch.rand(M, generator=g) < 0.1
        if kind == "every":
            where[::64] = False
        tok = torch.where(where, bad, tok)
        tok[1:4] = torch.tensor([-1, V, V + 5])           # each of the three at least once, however few the positions
    return tok.reshape(S, B).T.contiguous()            # position m = s * B + b holds tok[m]


def padded(ids):
    """The same ids inside a wider matrix (the caller takes the [:, :S] view: row stride S + ID_PAD); the padding holds an id
    outside every table, so a kernel that walked the rows with stride S would gather zero rows and miss its reference."""
    B, S = ids.shape
    wide = torch.full((B, S + ID_PAD), 2 ** 40, dtype=torch.int64)
    wide[:, :S] = ids
    return wide


def embed_bwd_inputs(case, oor=False):
    B, S, V, E, kind = case
    return embed_ids(B, S, V, kind, oor=oor), rnd(S * B, E, seed=3 + E)


def occurring_id(ids, V):
    tok = token_ids(ids)
    return int(tok[(tok >= 0) & (tok < V)][-1])


# ---- LayerNorm
LN_FWD_SHAPES = [(1, 4), (3, 252), (5, 256), (6, 260), (4, 508), (9, 512), (7, 516), (5, 1020), (2, 1024)]
LN_OFFSET_SHAPES = [(64, 512), (64, 1024)]
LN_OFFSET = 100.0            # at 1000 the two-pass float32 arithmetic itself is past the 2e-5 bound
LN_EPS = [1e-5, 1e-3]
LN_BWD_CASES = [            # (kernel instance, rows, E)
    ("u4g1", 50, 1024), ("u4g1", 3, 516), ("u1g1", 1, 4), ("u1g1", 1023, 256),
    ("u1g4f", 1024, 4), ("u2g4f", 1025, 260), ("u4g4f", 1040, 1020), ("u1g4f-chunk32", 16400, 32),
    ("u1g4", 1025, 128), ("u2g4", 1026, 512), ("u4g4", 1030, 1024),
]
LN_SHORT_CASES = [(1000, 1040, 512), (20, 50, 128)]          # (rows, full_rows, E): the short last batch of an epoch
LN_ZERO_VAR = (50, 128)
LN_TABLE_E, LN_TABLE_N, LN_TABLE_ENC, LN_TABLE_DEC = 128, 6, 96, 6
LN_TABLE_SHORT_ENC = [23, 24, 25, 31]                        # last chunk: a tail of 7, exactly 8, 8 + 1, 8 + 7 rows
LN_TABLE_FUSED_FULL = 1040
REDUCE_NBLK = [1, 2, 3, 4, 5, 28, 29, 31, 32, 33, 60, 61, 64, 65, 1024]
REDUCE_E = [4, 60, 64, 68, 200, 1024]


def ln_inputs(rows, E, *, offset=0.0, seed=0, const_rows=()):
    """x (scale 3, plus offset; const_rows set to the constant 2), gamma, beta, dy, add_to_dx."""
    x = rnd(rows, E, seed=seed + 1, scale=3.0 if offset == 0.0 else 1.0) + offset
    for r in const_rows:
        x[r] = 2.0
    return x, 1 + 0.1 * rnd(E, seed=seed + 2), 0.1 * rnd(E, seed=seed + 3), rnd(rows, E, seed=seed + 4), rnd(rows, E, seed=seed + 5)


# ---- loss: (B, V)
LOSS_CASES = [(1, 1), (3, 2), (5, 63), (4, 64), (6, 65), (1024, 202), (2, 4100)]
LOSS_PAD = 5                 # ld = V + 5
LOSS_SATURATED = (6, 65)     # logits x 30: past exp's float32 range without the max
LOSS_ALL_IGNORED = (4, 64)
LOSS_OOR = (6, 65)           # targets -3 and V + 1
LSM_BWD_CASES = [(1, 1), (3, 65), (5, 64), (1024, 202)]


def loss_ignore(V):
    return 1 if V >= 2 else -100


def loss_inputs(B, V, *, scale=1.0, kind="mixed"):
    """logits (scale 2, times `scale`) and targets.  mixed: valid targets with rows 1 and B // 2 ignored where the batch has
    them to spare (B >= 3 / B >= 5); all_ignored; oor: mixed, with targets -3 and V + 1 in rows 0 and B - 1."""
    ign = loss_ignore(V)
    logits = rnd(B, V, seed=B + V, scale=2.0) * scale
    y = torch.randint(2 if V > 2 else 0, V, (B,), generator=torch.Generator().manual_seed(B * 7 + V))
    if V == 2:
        y[:] = 0
    if B >= 3:
        y[1] = ign
    if B >= 5:
        y[B // 2] = ign
    if kind == "all_ignored":
        y[:] = ign
    if kind == "oor":
        y[0], y[B - 1] = -3, V + 1
    return logits, y, ign


def loss_weight(V):
    return torch.rand(V, generator=torch.Generator().manual_seed(4 + V)) + 0.25


# ---- optimizer step: arena sizes
OPT_N = [4, 1028, 2 ** 21 + 1024]        # one float4; a ragged tail; n / 4 > 2048 x 256: the update's grid-stride trip
