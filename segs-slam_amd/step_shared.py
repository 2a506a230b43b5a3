"""What TrainerStep (gaussian_trainer.py) and ScaffoldTrainerStep (neural_gaussians.py) share, written once: pointer and stream
marshalling, the fused-Adam launch in its two forms, the redo of an iteration the device dropped, and the staging / capture /
replay of a whole-iteration hipGraph.  Each step supplies its own `_iteration_body`, graph key and captured body."""
from __future__ import annotations

import ctypes as C

import torch

from . import _capi


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def stream_ptr(device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def adam_step(buckets, groups, opt, count, guard, device, grad_scale: float = 1.0, staged_lr=None):
    """The fused Adam over the (offset, count, lr) `groups` of `buckets` = (params, grads, exp_avg, exp_avg_sq), step count
    `count` on the device.  `guard`: pointer to the device word that drops the step when non-zero, or None.  An empty shard
    still launches (the count advances): one empty segment.  Eager form (segs_adam_step_device): the host says which of the
    count's two words is current.  `staged_lr` (segs_adam_step_graph, capturable): pointer to the groups' learning rates as
    device doubles -- the table's are 0 -- and the call index is on the device too."""
    groups = groups or [(0, 0, 0.0)]
    segs = (_capi.AdamSegment * len(groups))()
    for i, (o, n, lr) in enumerate(groups):
        segs[i].offset, segs[i].count, segs[i].lr = o, n, float(lr) if staged_lr is None else 0.0
    lib, o = _capi.lib(), opt
    if staged_lr is None:
        st = lib.segs_adam_step_device(*map(ptr, buckets), segs, len(segs), o.beta1, o.beta2, o.eps, ptr(count.words),
                                       count.eager_call(), float(grad_scale), 1, guard, stream_ptr(device))
    else:
        st = lib.segs_adam_step_graph(*map(ptr, buckets), segs, len(segs), staged_lr, o.beta1, o.beta2, o.eps, ptr(count.words),
                                      float(grad_scale), 1, guard, stream_ptr(device))
    _capi.check(st, "segs_adam_step_graph" if staged_lr is not None else "segs_adam_step_device")


class IterationStage:
    """The per-iteration values of a captured iteration at fixed addresses: packed keyframe, target image, learning rates."""

    def __init__(self, packed_floats: int, gt: torch.Tensor):
        self.packed = torch.zeros(packed_floats, dtype=torch.float32, device=gt.device)
        self.gt = torch.empty_like(gt)
        self.lr = torch.zeros(16, dtype=torch.float64, device=gt.device)
        self.table = None                  # ScaffoldTrainerStep: the frequency regulariser's target tables

    def fill(self, keyframe_parts, gt: torch.Tensor):
        off = 0
        for t in keyframe_parts:
            self.packed[off:off + t.numel()].copy_(t.reshape(-1))
            off += t.numel()
        self.gt.copy_(gt)

    def lr_ptr(self, group: int = 0):
        return C.c_void_p(self.lr.data_ptr() + 8 * group)


class DroppedStepRedo:
    """The bookkeeping around `_iteration_body(keyframe, gt, iteration, ...)` both steps share.  The step has `world`, `rank`,
    `iteration`, `engine` (None: a backend without an overflow word) and `_exchange()`."""

    def _init_step_state(self):
        self.redo_dropped_steps = True
        self.redone_steps = 0
        self._last_iteration = None
        self.use_graph = False
        self._graphs = {}
        self.graph_replays = 0
        self.keyframe_selector = None    # keyframe_window.SlidingWindowKeyframes: the mapper's walk instead of round-robin

    def keyframe_for(self, step: int, n_keyframes: int) -> int:
        """Deterministic shared schedule: rank r takes keyframe (step * world + r) mod n."""
        return (step * self.world + self.rank) % n_keyframes

    def _next_iteration(self, keyframes, gt_images, gt_depths=None):
        """training_once: redo the previous iteration if the device dropped it, then run the next one (and remember it).
        `gt_depths` (ScaffoldTrainerStep): a list indexed like `keyframes` whose entry goes to `_iteration_body` too."""
        self._redo_if_dropped()
        self.iteration += 1
        if self.keyframe_selector is None:
            k = self.keyframe_for(self.iteration - 1, len(keyframes))
        else:
            # useOneRandomSlidingWindowKeyframe (src/gaussian_mapper.cpp:827): one draw per rank, identical on every rank
            k = self.keyframe_selector.use_for_ranks(self.world)[self.rank]
        prev = (keyframes[k], gt_images[k], self.iteration) + (() if gt_depths is None else (gt_depths[k],))
        self._last_iteration = prev
        return self._iteration_body(*prev)

    def _redo_if_dropped(self):
        # An iteration the device dropped is run again -- same keyframe, same iteration number -- as soon as the host resolves that
        # step's overflow word, which is before the next iteration is queued.  One rank: the engine's own status word.  N > 1: the
        # SUMMED word every rank mirrored to its host after the gradient exchange (BucketExchange.mirror_flag), so all ranks
        # redo the same iteration together and replicas stay bit-identical.
        prev, eng = self._last_iteration, self.engine
        if prev is None or not self.redo_dropped_steps or self.use_graph:
            return
        resident = eng is not None and eng.resident
        for _ in range(4):
            if self.world == 1:
                dropped = resident and not eng.check(raise_on_overflow=False)
            else:
                dropped = bool(self._exchange().step_dropped())
                if resident:
                    eng.check(raise_on_overflow=False)      # the rank that overflowed re-calibrates in its next forward
            if not dropped:
                break
            self.redone_steps += 1
            self._iteration_body(*prev)
            if self.world == 1:
                break                                       # (a re-calibrating forward cannot overflow)
        else:
            raise RuntimeError("an iteration kept being dropped by the device")
        self._last_iteration = None

    def finish(self):
        """Resolve the LAST iteration's overflow word and run that iteration again if the device dropped it (training_once only
        learns of a drop at the next call).  Call once after the last training_once of a run, before reporting."""
        self._redo_if_dropped()

    # ---- whole-iteration hipGraph --------------------------------------------------------------------------------------------
    def _graph_ready(self) -> bool:
        """The resident rasterizer is calibrated and no overflow has just come to light (else: eager, which re-sizes)."""
        eng = self.engine
        return bool(eng.resident and eng.capacity > 0 and eng.poll() and eng.capacity > 0)

    def _replay_iteration(self, stage: IterationStage, groups, counts, key, max_cached: int, make_body) -> bool:
        """Refresh the staged learning rates, capture the iteration on a miss of `key` (`make_body()` -> the function to capture;
        the cache is emptied first when it holds more than `max_cached`), replay it and book it.  False: an overflow came to
        light before the capture -- take the eager path."""
        eng = self.engine
        vals = (C.c_double * len(groups))(*[float(g[2]) for g in groups])
        _capi.check(_capi.lib().segs_set_doubles(ptr(stage.lr), vals, len(groups), stream_ptr(stage.lr.device)), "segs_set_doubles")
        for c in counts:
            c.sync_device_calls()
        g = self._graphs.get(key)
        if g is None:
            eng.check(raise_on_overflow=False)           # nothing pending while the capture runs
            if eng.capacity <= 0:
                return False
            if len(self._graphs) > max_cached:
                self._graphs.clear()
            body = make_body()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                body()
            self._graphs[key] = g
        g.replay()
        for c in counts:
            c.calls += 1                                 # (the device-side call count advanced with the replay)
        eng.after_graph_replay()
        self.graph_replays += 1
        return True
