"""Learning-rate schedules as a pure function of the step count.

``lr_at(t, ...)`` is the learning rate of the optimiser step taken after ``t`` earlier ones (the host's count, skipped
`-mp` steps included).  Nothing else is kept: a resumed run that restores its count continues the curve.

    warm-up     t < warmup_steps:   base_lr * (t + 1) / warmup_steps
    afterwards  u = (t - warmup_steps) / (total_steps - warmup_steps)
      'poly'    max(min_lr, base_lr * (1 - u) ** poly_power)
      'cosine'  min_lr + (base_lr - min_lr) * (1 + cos(pi * u)) / 2
    t >= total_steps:               min_lr
    schedule None:                  base_lr
"""
import math

SCHEDULES = ('poly', 'cosine')


def lr_at(t, base_lr, schedule=None, total_steps=None, warmup_steps=0, poly_power=0.9, min_lr=0.0):
    if schedule is None:
        return float(base_lr)
    if schedule not in SCHEDULES:
        raise ValueError("schedule must be None, 'poly' or 'cosine'; got %r" % (schedule,))
    if total_steps is None or total_steps <= 0:
        raise ValueError('schedule=%r needs total_steps > 0; got %r' % (schedule, total_steps))
    if warmup_steps < 0 or warmup_steps >= total_steps:
        raise ValueError('warmup_steps must be in [0, total_steps); got %r of %r' % (warmup_steps, total_steps))
    if t < 0:
        raise ValueError('t counts optimiser steps already taken; got %r' % (t,))
    if t >= total_steps:
        return float(min_lr)
    if t < warmup_steps:
        return float(base_lr) * (t + 1) / warmup_steps
    u = (t - warmup_steps) / float(total_steps - warmup_steps)
    if schedule == 'poly':
        return max(float(min_lr), float(base_lr) * (1.0 - u) ** poly_power)
    return float(min_lr) + (float(base_lr) - float(min_lr)) * (1.0 + math.cos(math.pi * u)) / 2.0
