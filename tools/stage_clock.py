"""StageClock: the wrap / time / restore helper of the bench tools (longform_bench, localise_bench, clip_bench).  It
replaces attributes of modules, classes or instances by timed versions for one call of the real entry point and puts them
back afterwards, so the stage split is measured on the code as it ships."""
import time

import torch


class StageClock:
    """Wraps the stage functions a call goes through; every wrapped call is bracketed by device synchronisations and its wall
    time is added to ``ms[stage]``."""

    def __init__(self):
        self.ms = {}
        self._undo = []

    def wrap(self, owner, attr, stage):
        """stage: a name, or a list of names for the first, second, ... call (the last one for every later call)."""
        fn = getattr(owner, attr)
        names = [stage] if isinstance(stage, str) else list(stage)
        calls = [0]

        def timed(*a, **kw):
            name = names[min(calls[0], len(names) - 1)]
            calls[0] += 1
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = fn(*a, **kw)
            torch.cuda.synchronize()
            self.ms[name] = self.ms.get(name, 0.0) + (time.perf_counter() - t0) * 1e3
            return r
        had = attr in vars(owner)
        self._undo.append((owner, attr, fn, had))
        setattr(owner, attr, timed)

    def restore(self):
        for owner, attr, fn, had in reversed(self._undo):
            if had:
                setattr(owner, attr, fn)
            else:
                delattr(owner, attr)
        self._undo = []
