"""What tools/neighbor_prior_bench.py and tools/kde_prior_bench.py share: the synthetic points and the two clocks."""
import time

import numpy as np
import torch


def blobs(n, seed, num_classes, centres=None):
    """Points around 40 'land' centres, denser where a centre is heavier; classes correlate with the centre."""
    rng = np.random.default_rng(seed)
    if centres is None:
        centres = np.stack([rng.uniform(-160, 160, 40), rng.uniform(-50, 65, 40), rng.uniform(2, 12, 40), rng.random(40) ** 2 + 0.05], 1)
    w = centres[:, 3] / centres[:, 3].sum()
    which = rng.choice(len(centres), n, p=w)
    pts = centres[which, :2] + rng.normal(0, 1, (n, 2)) * centres[which, 2:3]
    pts[:, 0] = np.clip(pts[:, 0], -179.99, 179.99)
    pts[:, 1] = np.clip(pts[:, 1], -89.99, 89.99)
    cls = (which * (num_classes // len(centres)) + rng.integers(0, max(1, num_classes // 8), n)) % num_classes
    return pts, cls, centres


def timed(fn, repeats):
    """After a warm-up call, the median of HIP-event times of single calls, in seconds."""
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e-3)
    return float(np.median(times))


def wall(fn):
    """(result, wall seconds) of one call between two synchronisations."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0
