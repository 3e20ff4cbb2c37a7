"""numpy float32 reference of the weight average (las_ema_update / las_ema_swap, ops.ema_decay_at): the C contract of
include/las_hip.h restated.  The update is two fp32 products and one fp32 sum in a fixed order, with (1 - decay) formed once in
fp32; numpy evaluates float32 arrays elementwise without contraction, so the device result is reproduced bit for bit."""
import numpy as np


def decay_at(k, decay):
    """The decay of the k-th update after the initialising copy, k >= 1: min(decay, (1 + k)/(10 + k)), in Python floats."""
    assert k >= 1
    return min(float(decay), (1.0 + k) / (10.0 + k))


def update(ema, p, decay):
    """decay*ema + (1 - decay)*p in float32, in that order.  Returns a new array; ema and p are left alone."""
    ema, p = np.asarray(ema, dtype=np.float32), np.asarray(p, dtype=np.float32)
    d = np.float32(decay)
    rest = np.float32(1.0) - d
    with np.errstate(all='ignore'):
        a = d * ema
        b = rest * p
        return (a + b).astype(np.float32)


def swap(p, ema):
    """(new p, new ema): the two exchanged, as copies."""
    return np.array(ema, dtype=np.float32, copy=True), np.array(p, dtype=np.float32, copy=True)
