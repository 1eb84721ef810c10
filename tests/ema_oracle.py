"""Float64 statement of the generator weight average that sgg_adam_ema keeps -- test infrastructure.

    t    = number of applied updates, this one included (Adam's ``iterations`` after its increment)
    d_t  = min(decay, (1 + t) / (10 + t))                       tf.train.ExponentialMovingAverage(decay, num_updates)
    ema  = d_t * ema + (1 - d_t) * theta_new

The kernel holds d_t and 1 - d_t as f32 (``decay_f32``); ``ema_run`` takes the sequence of parameter vectors an optimizer
produced and applies the rule in float64 with those two f32 factors, so what is left between it and the kernel is the
rounding of the kernel's own three f32 operations per element and step."""
import numpy as np


def decay_at(decay, t):
    """d_t in float64 from a float64 decay."""
    t = float(int(t))
    return min(float(decay), (1.0 + t) / (10.0 + t))


def decay_f32(decay, t):
    """(d_t, 1 - d_t) as the kernel holds them: the decay enters as f32, the ramp is evaluated in double and rounded to f32
    once, and the complement is formed in f32."""
    d = np.float32(decay_at(float(np.float32(decay)), t))
    return d, np.float32(1.0) - d


def ramp_end(decay):
    """The first t at which d_t equals the decay itself."""
    t = 0
    while (1.0 + t) / (10.0 + t) < decay:
        t += 1
    return t


def ema_step(ema, theta_new, decay, t):
    d, omd = decay_f32(decay, t)
    return float(d) * np.asarray(ema, dtype=np.float64) + float(omd) * np.asarray(theta_new, dtype=np.float64)


def ema_run(ema0, thetas, decay, t0=0):
    """The average after the updates t0 + 1, t0 + 2, ... whose results are ``thetas`` (skipped updates are simply not in the
    list).  Returns (ema, max_abs) with max_abs the largest magnitude any average or parameter took on the way -- the scale
    of the kernel's roundings."""
    ema = np.asarray(ema0, dtype=np.float64)
    max_abs = float(np.abs(ema).max()) if ema.size else 0.0
    for k, th in enumerate(thetas):
        th = np.asarray(th, dtype=np.float64)
        ema = ema_step(ema, th, decay, t0 + k + 1)
        max_abs = max(max_abs, float(np.abs(th).max()), float(np.abs(ema).max()))
    return ema, max_abs
