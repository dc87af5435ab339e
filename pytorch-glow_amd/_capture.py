"""The one way this package records a hipGraph, and the one rule for when a recorded graph is stale ("Captured graphs").

Each of the five sites (`network.model.GraphedSampler` / `GraphedForward`, `training.GraphedTrainStep`, `network.restore.LatentFit`,
`network.posterior.LatentMALA`) gives a `Capture` its body and a function that returns its SIGNATURE: a dict of named items --
addresses, version counters, epochs -- for what ITS captured launches reach and an eager call in between could move or rebuild
(`FlowPlan.capture_signature`, `_HipOptimizer.capture_signature`).  What a stale graph costs -- an error, a recapture -- is the site's."""
import gc

import torch

from . import _lib

REASONS = {"parameters": "a parameter was re-allocated", "versions": "the parameters changed",
           "family": "the plan was packed for the other kernel family", "pack_epoch": "the plan was packed for the other kernel family",
           "_ws": "the plan's inference workspace was re-allocated (an eager call with a larger batch)"}


def address(t):
    return t.data_ptr() if isinstance(t, torch.Tensor) else None


def moved(then, now):
    """The names of the items of ``then`` (the signature taken at capture) that differ in ``now``.  An item that was None at capture
    -- a buffer that did not exist yet -- is not compared: no captured launch can reach it, so one allocated later (the inference
    workspace of the first evaluation forward between two training steps) must not cost a recapture."""
    return [name for name, value in then.items() if value is not None and now.get(name) != value]


class Capture:
    """``body`` recorded once on a side stream, by the sequence every site follows: the side stream joins the current one;
    ``warmup`` eager runs of the body on it (the inference graphs: workspace, job tables, lazy inits -- the other sites have an eager
    step behind them instead); a device synchronise; ``plan.pack_sync()``, so nothing of an earlier pack is left for the captured
    calls to join; the recording, under ``torch.no_grad()`` and with Python's cycle collector off.  Nothing runs
    during the recording."""

    def __init__(self, plan, body, signature, warmup=0):
        dev = plan.device
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.no_grad():
            if warmup:
                with torch.cuda.stream(side):
                    for _ in range(warmup):
                        body()
                torch.cuda.current_stream(dev).wait_stream(side)
            # No garbage collection inside the recording.  A finished loop and its `Capture` are a reference cycle (the body and
            # the signature close over the loop), so the graph and the side stream of an earlier fit die only when the cycle
            # collector runs -- and the body's thousands of small host objects make it run inside the recording, where destroying
            # a graph or a stream aborts the process (torch.cuda.graph used to collect on entry and no longer does by default).
            # Keep the collector off until the recording has ended; what is dead dies after it, as it did before.
            torch.cuda.synchronize(dev)
            plan.pack_sync()
            self.graph = torch.cuda.CUDAGraph()
            collecting = gc.isenabled()
            gc.disable()
            try:
                # (thread_local: a DataLoader's pinning thread may touch the device while this thread captures)
                with torch.cuda.graph(self.graph, stream=side, capture_error_mode="thread_local"):
                    body()
            finally:
                if collecting:
                    gc.enable()
        self.replay = self.graph.replay
        self._signature, self._then = signature, signature()

    def moved(self):
        """What moved since the capture; empty: a replay reaches what the recording reached."""
        return moved(self._then, self._signature())

    def check(self, who):
        """Raise instead of replaying over something that moved."""
        names = self.moved()
        if names:
            why = dict.fromkeys(REASONS.get(name, f"{name} moved") for name in names)
            raise _lib.GlowHipError(f"{who}: {', '.join(why)} since the capture -- capture again")
