"""What the tools/time_*.py share: a window of calls between two stream events, and alternating windows of several contestants."""
import numpy as np
import torch


def window(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3   # us per call


def report(fns, n, warm, rounds, name='', width=72):
    """`warm` calls of every contestant of {label: callable}, then `rounds` windows of n calls each in turn; one row per contestant
    with the median, every window and the spread of the windows in percent of the median -> {label: median in us}."""
    for fn in fns.values():
        for _ in range(warm):
            fn()
    vals = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():          # alternating
            vals[k].append(window(fn, n))
    for k, v in vals.items():
        print('%-*s median %10.1f us  (%s)  spread %.1f %%' % (width, name + k, float(np.median(v)), ' '.join('%.1f' % x for x in v),
              100.0 * (max(v) - min(v)) / float(np.median(v))), flush=True)
    return {k: float(np.median(v)) for k, v in vals.items()}
