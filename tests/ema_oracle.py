"""fp64 restatement of the Polyak average the HIP optimisers keep (include/glowhip.h, glowhip_optim_step_ema): the recurrence
e' = e + (p' - e) * w, the host-side warm-up rule that chooses w, and the error bound the device's fp32 result is held to.  Nothing
here reads the package: the tests hold training._HipOptimizer to these lines, not the other way round."""
import numpy as np


def decay_at(t, ema_decay, warmup):
    """decay of the EMA update that follows `t` applied ones: min(ema_decay, (1 + t) / (10 + t)) with warm-up, else ema_decay."""
    return min(float(ema_decay), (1.0 + t) / (10.0 + t)) if warmup else float(ema_decay)


def weight_at(t, ema_decay, warmup):
    """w = float32(1 - decay_t), the subtraction in doubles; returned as a python float holding the float32's value."""
    return float(np.float32(1.0 - decay_at(t, ema_decay, warmup)))


def advance(e, p_new, w):
    """One update in fp64 from the (device's own) new parameter values and the float w the device was given."""
    e = np.asarray(e, dtype=np.float64)
    return e + (np.asarray(p_new, dtype=np.float64) - e) * float(w)


def bound(T, M):
    """Largest |device - oracle| after T updates: each update rounds three times in fp32 (p' - e: magnitude <= 2M; the product:
    <= 2M w; the sum: <= M), half an ulp each, i.e. at most (2M + 2M w + M) * 2^-24 <= 5 M 2^-24 per update; the error carried
    in from earlier updates is multiplied by (1 - w) <= 1.  M = largest |p| or |e| seen for the tensor."""
    return 5.0 * T * 2.0 ** -24 * float(M)
