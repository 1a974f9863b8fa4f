"""fp64 restatement of the running average the library keeps on the device (csrc/average.hip), after
``torch.optim.swa_utils``: ``AveragedModel``'s default ``avg_fn`` ("swa") and ``get_ema_multi_avg_fn(decay)`` ("ema").

The first model fed is copied; model number ``c + 1`` (``c`` models in the average so far) then moves it by
``(p - avg) / (c + 1)`` (swa) or ``(p - avg) * (1 - decay)`` (ema).  Floats ``skip`` [begin, end) are copied every time.

``bound(updates, M)``: what an fp32 implementation may be off by after ``updates`` updates on values of magnitude <= ``M``.
Each update is at most three roundings (the difference, its scaling, the sum) of quantities bounded by 2 M -- 3 * 2 M * 2^-24
< 8 * 2^-24 * M -- and the recurrence does not amplify what is already there (|1 - weight| <= 1): the errors add."""
import numpy as np


def average_ref(snapshots, kind, decay=0.0, skip=None):
    """``snapshots``: the models fed, in order, each a flat array.  Returns the average in float64."""
    assert kind in ("swa", "ema") and len(snapshots) > 0
    avg = None
    for c, p in enumerate(snapshots):
        p = np.asarray(p, dtype=np.float64).reshape(-1)
        if c == 0:
            avg = p.copy()
        elif kind == "swa":
            avg = avg + (p - avg) / (c + 1)
        else:
            avg = avg + (p - avg) * (1.0 - decay)
        if skip is not None and skip[1] > skip[0]:
            avg[skip[0]:skip[1]] = p[skip[0]:skip[1]]
    return avg


def average_ref_dicts(dicts, kind, decay=0.0):
    """The same per key of a list of state dicts (name -> array-like); returns {name: float64 array of that shape}."""
    out = {}
    for k in dicts[0]:
        shape = np.asarray(dicts[0][k]).shape
        out[k] = average_ref([np.asarray(d[k]) for d in dicts], kind, decay).reshape(shape)
    return out


def bound(updates, M):
    return updates * 8 * 2.0 ** -24 * float(M)
