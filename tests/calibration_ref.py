"""The definitions of include/mmu.h's temperature scaling restated in numpy, for the calibration tests
(test_calibration_host.py, test_temperature_nll_gpu.py, test_decompose_scaled_gpu.py,
test_calibration_gpu.py):
  p_kt(beta) = softmax(beta_k z_kt)   p_k = mean_t p_kt   p(beta) = mean_k p_k
  nll_s(beta) = -ln max(p(beta)_y, 1e-12), and p_y = 0 for a label outside [0, C).
The softmax is written exp(beta (z - max z)) / sum: for beta >= 0 that is softmax(beta z) exactly
(max(beta z) = beta max z), and it is the form whose float32 evaluation is a fair yardstick -- forming
beta z first would round a product of magnitude beta |z| before the subtraction cancels it.
"""
import numpy as np


def temperature_nll_ref(z, y, beta, dt):
    """z f32 [S, K, T, C], y int [S], beta [J, K] -> nll [S, J] at precision dt"""
    S, K, T, C = z.shape
    beta = np.asarray(beta)
    inside = (y >= 0) & (y < C)
    yc = np.where(inside, y, 0)
    J = beta.shape[0]
    out = np.empty((S, J), dtype=dt)
    d = z.astype(dt)
    d = d - d.max(-1, keepdims=True)
    step = max(1, 2_000_000 // z.size)            # candidates per slab: about 2M elements at a time
    for j in range(0, J, step):
        e = np.exp(beta[j:j + step].astype(dt)[:, None, :, None, None] * d[None])       # [j, S, K, T, C]
        p = e[:, np.arange(S), :, :, yc] / e.sum(-1, dtype=dt).transpose(1, 0, 2, 3)     # [S, j, K, T]
        py = p.mean(3, dtype=dt).mean(2, dtype=dt)                                         # mean_t, then mean_k
        py = np.where(inside[:, None], py, dt(0))
        out[:, j:j + step] = -np.log(np.maximum(py, dt(1e-12)))
    return out


def mean_nll_evaluator(z, y):
    """the fp64 evaluator fit_temperature takes: beta f64 [J, K] -> mean NLL f64 [J] (each candidate's
    samples summed on their own, so a candidate's figure does not depend on its neighbours)"""
    def evaluate(beta):
        nll = np.ascontiguousarray(temperature_nll_ref(z, y, beta, np.float64).T)
        return nll.sum(1) / z.shape[0]
    return evaluate
