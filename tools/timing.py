"""The timer of the tools that time single passes (time_depth.py, time_labels.py, time_instances.py, time_bev.py): device events around
back-to-back calls on the handle's stream, the candidates alternating within ONE process, and the median and spread of the rounds."""
import torch


def alternating_rounds(stream, calls, reps, rounds):
    """calls: name -> callable that launches on `stream`.  Every callable is warmed up (3 calls); then, `rounds` times, each in turn is called
    `reps` times back to back between two device events.  Returns name -> [ms per call, one figure per round]."""
    ms = {k: [] for k in calls}
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        for f in calls.values():
            for _ in range(3):
                f()
        for _ in range(rounds):
            for k, f in calls.items():
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record(stream)
                for _ in range(reps):
                    f()
                t1.record(stream)
                t1.synchronize()
                ms[k].append(t0.elapsed_time(t1) / reps)
    return ms


def median_spread(figures):
    """(median, min, max) of one name's rounds."""
    s = sorted(figures)
    return s[len(s) // 2], s[0], s[-1]
