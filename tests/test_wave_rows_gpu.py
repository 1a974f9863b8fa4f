"""GPU: the wave-per-row loop of the judging kernels (csrc/common.hpp: ``wave_rows``) past its wrap.  A launch has at most 2048
blocks of four waves, so with more than 8192 rows a wave takes a second row: N = 8197 makes waves 0 .. 4 do so.  The rows on both
sides of the wrap (0, 8191, 8192, 8196) must come out of the big call with the bits they have when each is passed alone in a 1-row
call -- a row's result is a function of the row -- and ``fit_temperature``, whose row terms pass through the same loop into sums
over all N rows, must agree with the numpy restatement under the bounds tests/test_calibration_gpu.py states."""
import numpy as np
import pytest
import torch

from calibration_ref import fit_temperature_ref, newton_step
from test_calibration_cpu import make_logp

pytestmark = pytest.mark.gpu

N, V, LD = 8197, 3, 6
ROWS = (0, 8191, 8192, 8196)


@pytest.fixture(scope="module")
def data():
    logp, y = make_logp(N, V, 2.0, 0.6, 7)
    buf = torch.full((N, LD), float("nan"), dtype=torch.float32, device="cuda")      # (the padding is NaN: never to be read)
    buf[:, :V] = torch.from_numpy(logp).cuda()
    return logp, y, buf[:, :V], torch.from_numpy(y).cuda()


def _bits(t):
    return t.contiguous().cpu().numpy().tobytes()


def test_rows_past_the_wrap_have_their_single_row_bits(data):
    from slnlp import ops
    _, _, z, y = data
    state = ops.temperature_state(1.0 / 1.7, z.device)
    log_w = torch.log_softmax(torch.tensor([0.3, -0.2, 0.1], dtype=torch.float64, device=z.device), dim=0)

    def outputs(zz, yy):
        pred, picked, rank, _ = ops.score_rows(zz, yy)
        idx, prob = ops.topk_rows(zz, 2, state=state)
        return {"scale_logp": ops.scale_logp(zz, state), "shift_logp": ops.shift_logp(zz, log_w, state), "score_rows.pred": pred,
                "score_rows.picked": picked, "score_rows.rank": rank, "reliability_rows.rows": ops.reliability_rows(zz, yy, state=state)[0],
                "topk_rows.idx": idx, "topk_rows.prob": prob}
    big = outputs(z, y)
    for r in ROWS:
        alone = outputs(z[r:r + 1], y[r:r + 1].contiguous())
        for name, t in big.items():
            assert tuple(alone[name].shape) == (1, *t.shape[1:]), name
            assert _bits(t[r:r + 1]) == _bits(alone[name]), (name, r, t[r:r + 1].tolist(), alone[name].tolist())


def test_fit_temperature_past_the_wrap_against_the_restatement(data):
    from slnlp import ops
    logp, y, z, yd = data
    want = fit_temperature_ref(logp, y)
    got = ops.temperature_download(ops.fit_temperature(z, yd))
    print(f"device {got}\nref    {want}")
    assert (got["reason"], got["rows"], got["bad_labels"]) == (want["reason"], want["rows"], want["bad_labels"])
    assert got["temperature"] == 1.0 / got["beta"]
    assert got["reason"] in ("gradient", "step")             # a converged search: the data has a temperature off the bounds
    residual, deviation = newton_step(logp, y, got["beta"]), abs(got["temperature"] / want["temperature"] - 1.0)
    print(f"newton_step_residual {residual:.3e} temperature_relative_deviation {deviation:.3e}")
    assert residual <= 1e-9 and deviation <= 1e-9
    assert abs(got["iterations"] - want["iterations"]) <= 1 and 1 <= got["iterations"] <= 16
    for k in ("nll_before", "nll_after"):
        assert abs(got[k] - want[k]) <= 1e-12 * abs(want[k]), (k, got[k], want[k])
    assert got["nll_after"] <= got["nll_before"]
