"""Per-run random streams of ``RRT_Planner.plan_runs``: run i draws what ``random.seed(s); np.random.seed(s);
torch.manual_seed(s); planner.reset(); planner.plan()`` draws, s = seeds[i], while several runs share one forest.

The reference draws its samples from the GLOBAL ``random`` / ``np.random`` generators (planners/base_planner.py:162-207,
planners/RRT.py:134-140,153-156), and ``planners/_draw.py`` works on them too.  So each run keeps its own two states and swaps
them in around its draws; the caller's states are put back when ``plan_runs`` returns.  The start noise (and the DDPM step
noise) of a run comes from its own device ``torch.Generator``, seeded as ``torch.manual_seed(s)`` seeds the default one, and
is drawn with the same shapes in the same order as ``plan()`` draws it.  Nothing here needs a GPU except that generator.
"""
from __future__ import annotations

import random
from contextlib import contextmanager

import numpy as np


class RunStreams:
    """The generator states one seeded run owns.  ``device``: where its torch generator lives (None: no torch generator)."""

    def __init__(self, seed, device=None):
        self.seed = int(seed)
        self.py = random.Random(self.seed).getstate()                 # what random.seed(s) leaves
        self.np = np.random.RandomState(self.seed).get_state()        # what np.random.seed(s) leaves
        self.gen = None
        if device is not None:
            import torch
            self.gen = torch.Generator(device=device)
            self.gen.manual_seed(self.seed)                            # what torch.manual_seed(s) leaves on that device

    @contextmanager
    def active(self):
        """The global ``random`` / ``np.random`` hold this run's states inside the block; the run keeps where they end."""
        random.setstate(self.py)
        np.random.set_state(self.np)
        try:
            yield self
        finally:
            self.py = random.getstate()
            self.np = np.random.get_state()


@contextmanager
def caller_states_kept():
    """Whatever runs inside, the caller's global ``random`` / ``np.random`` states are restored on the way out."""
    py, npst = random.getstate(), np.random.get_state()
    try:
        yield
    finally:
        random.setstate(py)
        np.random.set_state(npst)


def draw_runs(draw_round, streams, sizes):
    """One round of several runs: ``draw_round(B) -> (samples, cond_goals)`` on the global generators (the facade's
    ``RRT_Planner.draw_round``), called for every run with ``sizes[i] > 0`` under that run's states.  -> list of (s, c) or
    None per run.  The caller keeps its own states around the whole loop (``caller_states_kept``)."""
    out = []
    for st, B in zip(streams, sizes):
        if B <= 0:
            out.append(None)
            continue
        with st.active():
            out.append(draw_round(int(B)))
    return out
