"""Trainer step around the rasterizer: render -> L1 + lambda*(1-SSIM) -> backward -> [RCCL all-reduce] -> Adam.

Mirror of the loop body of GaussianTrainer::trainingOnce (src/gaussian_trainer.cpp:47-117) -- the minimal
"render + L1/SSIM + Adam" step of SURVEY section 3.2 -- over the rasterizer's own inputs as trainable parameters
(means3D, scales, rotations, opacity, colors = 14 floats per Gaussian, one flat fp32 bucket).

Keyframe-parallel training (new functionality: the reference is single-GPU, F3): one process
per GPU, every rank holds a full replica, rank r renders keyframe r of the step; the only exchange is the one of
keyframe_parallel.BucketExchange over the flat gradient bucket (RCCL over xGMI when the backend is "nccl"):
reduce-scatter -> fused Adam on this rank's shard -> all-gather of the parameters (or, dense, one all-reduce and a full
Adam on every rank); replicas stay bit-identical either way.

The raster backend and the optimizer are injectable so that the distributed logic can be exercised on CPU
(gloo, world_size 2) in tests; the product wiring is `TrainerStep.on_gpu(...)` = HIP engine + fused HIP Adam.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Callable, Dict, Optional

import torch
import torch.distributed as dist

from . import _capi, loss_utils
from .raster_engine import FIELDS, FLOATS_PER_GAUSSIAN, split_flat
from .step_shared import DroppedStepRedo, IterationStage, adam_step, ptr, stream_ptr


@dataclass
class OptimizationParams:
    """The subset of GaussianOptimizationParams (include/gaussian_parameters.h) the step uses."""
    lambda_dssim: float = 0.2           # cfg/gaussian_mapper/RGB-D/Replica/office0.yaml:89
    position_lr_init: float = 0.00016
    position_lr_final: float = 0.0000016
    position_lr_max_steps: int = 30000
    scaling_lr: float = 0.005
    rotation_lr: float = 0.001
    opacity_lr: float = 0.05
    feature_lr: float = 0.0025          # colours
    beta1: float = 0.9
    beta2: float = 0.999
    eps: float = 1e-15                  # src/gaussian_model.cpp:632-661


def expon_lr(step: int, lr_init: float, lr_final: float, max_steps: int) -> float:
    """getExponLrFunc (src/gaussian_model.cpp:1393-1409) with lr_delay_steps = 0 (delay_rate == 1)."""
    if step < 0 or (lr_init == 0.0 and lr_final == 0.0):
        return 0.0
    t = min(max(step / max_steps, 0.0), 1.0)
    return math.exp(math.log(lr_init) * (1 - t) + math.log(lr_final) * t)


class DeviceStepCount:
    """Step count of one set of torch::optim::Adam parameter groups, kept on the device (segs_adam_step_device,
    include/segs_train.h): two int64 words used in turn, `calls` says which one the next launch reads.  A guarded step that
    the device drops does not advance it, and the host never has to find out."""

    def __init__(self, device):
        # [0], [1]: the pair; [2]: the call count as the hipGraph-capturable form keeps it on the device (segs_adam_step_graph)
        self.words = torch.zeros(3, dtype=torch.int64, device=device)
        self.calls = 0
        self._device_calls_current = True     # words[2] == calls (the eager form does not touch words[2])

    def clone(self) -> "DeviceStepCount":
        c = DeviceStepCount(self.words.device)
        c.words.copy_(self.words)
        c.calls = self.calls
        c._device_calls_current = self._device_calls_current
        return c

    def eager_call(self) -> int:
        """Call index for segs_adam_step_device (host-side parity); the device-side call count falls behind."""
        call = self.calls
        self.calls += 1
        self._device_calls_current = False
        return call

    def sync_device_calls(self):
        """Before capturing / replaying segs_adam_step_graph after eager calls: bring words[2] up to the host's count."""
        if not self._device_calls_current:
            self.words[2:3].fill_(self.calls)
            self._device_calls_current = True

    def value(self) -> int:
        """Steps taken so far (synchronises; for tests and checkpoints)."""
        return int(self.words[self.calls & 1].item())

    def dropped(self) -> int:
        """Launches the device dropped (guard word set: an iteration whose pass overflowed the resident capacity on some
        rank): launches issued minus steps taken (synchronises).  The reference never drops an iteration; the loss returned
        for a dropped one comes from a truncated image and the iteration counter / LR schedule still advanced."""
        return self.calls - self.value()


def field_segments(lrs: Dict[str, float], P: int):
    """(offset, count, lr) of the five per-Gaussian fields inside the flat bucket (raster_engine.FIELDS order)."""
    out, off = [], 0
    for name, n in FIELDS:
        out.append((off, P * n, float(lrs[name])))
        off += P * n
    return out


class FusedAdam:
    """segs_adam_step_device over the flat bucket (include/segs_train.h): one launch, step count on the device, optionally
    guarded by a device word (the all-reduced overflow word of the resident rasterizer) and restricted to a shard."""

    def __init__(self, n_params: int, device, opt: OptimizationParams):
        _capi.lib()                      # (there is no CPU fallback: a missing library is an error here)
        self.opt = opt
        self.exp_avg = torch.zeros(n_params, dtype=torch.float32, device=device)
        self.exp_avg_sq = torch.zeros(n_params, dtype=torch.float32, device=device)
        self.count = DeviceStepCount(device)

    @property
    def step_count(self) -> int:
        return self.count.value()

    def step(self, params_flat: torch.Tensor, grads_flat: torch.Tensor, lrs: Dict[str, float], P: int, grad_scale: float,
             exchange=None, guard: Optional[torch.Tensor] = None):
        groups = field_segments(lrs, P)
        if exchange is not None:
            groups = exchange.clip_segments(groups)
        adam_step((params_flat, grads_flat, self.exp_avg, self.exp_avg_sq), groups, self.opt, self.count, ptr(guard),
                  params_flat.device, grad_scale)


class FusedL1SSIM:
    """segs_l1_ssim_loss (include/segs_train.h): loss and dL/dimage in two HBM-streaming kernels."""

    def __init__(self, H: int, W: int, device, lambda_dssim: float):
        self._lib = _capi.lib()
        self.H, self.W, self.lam = int(H), int(W), float(lambda_dssim)
        self.temp = torch.empty(self._lib.segs_l1_ssim_temp_bytes(H, W), dtype=torch.uint8, device=device)
        self.out = torch.zeros(3, dtype=torch.float32, device=device)     # loss, l1, ssim
        self.dL = torch.empty((3, H, W), dtype=torch.float32, device=device)

    def __call__(self, image: torch.Tensor, gt: torch.Tensor):
        assert image.is_contiguous() and gt.is_contiguous() and image.shape == (3, self.H, self.W) == gt.shape
        st = self._lib.segs_l1_ssim_loss(ptr(image), ptr(gt), self.H, self.W, self.lam, ptr(self.out), ptr(self.dL), ptr(self.temp),
                                         stream_ptr(image.device))
        _capi.check(st, "segs_l1_ssim_loss")
        return self.out[0], self.dL


class TorchAdam:
    """Same arithmetic with torch ops (LibTorch C++ Adam formula); used for CPU tests of the distributed logic."""

    def __init__(self, n_params: int, device, opt: OptimizationParams):
        self.opt = opt
        self.exp_avg = torch.zeros(n_params, dtype=torch.float32, device=device)
        self.exp_avg_sq = torch.zeros(n_params, dtype=torch.float32, device=device)
        self.step_count = 0

    def step(self, params_flat, grads_flat, lrs, P, grad_scale, exchange=None, guard=None):
        """`exchange`: update only this rank's shard (moments outside it are not kept current, as in FusedAdam)."""
        o = self.opt
        if guard is not None and float(guard.reshape(-1)[0]) != 0:
            grads_flat.zero_()
            return
        self.step_count += 1
        bc1 = 1.0 - o.beta1 ** self.step_count
        bc2 = 1.0 - o.beta2 ** self.step_count
        groups = field_segments(lrs, P)
        if exchange is not None:
            groups = exchange.clip_segments(groups)
        for off, cnt, lr in groups:
            sl = slice(off, off + cnt)
            g = grads_flat[sl] * grad_scale
            self.exp_avg[sl].mul_(o.beta1).add_(g, alpha=1 - o.beta1)
            self.exp_avg_sq[sl].mul_(o.beta2).addcmul_(g, g, value=1 - o.beta2)
            denom = (self.exp_avg_sq[sl].sqrt() / math.sqrt(bc2)).add_(o.eps)
            params_flat[sl].addcdiv_(self.exp_avg[sl], denom, value=-(lr / bc1))
        grads_flat.zero_()


class TrainerStep(DroppedStepRedo):
    """One keyframe-parallel training step.  `render_backward(params: dict, keyframe, dL_fn) -> (image, loss)` must
    render the keyframe, call dL_fn(image) -> (loss, dL_dimage) and leave parameter gradients in `grads_flat`."""

    def __init__(self, params_flat: torch.Tensor, P: int, render_backward: Callable, optimizer, opt: OptimizationParams,
                 grads_flat: torch.Tensor, process_group=None, sharded_optimizer: bool = True,
                 single_rank_collectives: bool = False):
        import inspect
        from .keyframe_parallel import BucketExchange
        assert params_flat.numel() == FLOATS_PER_GAUSSIAN * P and grads_flat.numel() == params_flat.numel()
        self.params_flat, self.grads_flat, self.P = params_flat, grads_flat, P
        self.params = split_flat(params_flat, P)
        self.render_backward, self.optimizer, self.opt = render_backward, optimizer, opt
        self.pg = process_group
        self.exchange = BucketExchange(params_flat.numel(), params_flat.device, process_group, sharded=sharded_optimizer,
                                       single_rank_collectives=single_rank_collectives, grads=grads_flat)
        self.world, self.rank = self.exchange.world, self.exchange.rank
        self.iteration = 0
        self.engine = None               # the HIP raster engine (on_gpu); None: a backend without an overflow word
        self._stage = None
        self._init_step_state()
        # a backend that knows an overflow word (the HIP engine) takes a hook it calls right after its forward
        self._backend_takes_hook = render_backward is not None and "after_forward" in inspect.signature(render_backward).parameters

    def learning_rates(self, iteration: int) -> Dict[str, float]:
        o = self.opt  # updateLearningRate (src/gaussian_model.cpp:874-998): only the position group is scheduled
        return {"means3D": expon_lr(iteration, o.position_lr_init, o.position_lr_final, o.position_lr_max_steps),
                "scales": o.scaling_lr, "rotations": o.rotation_lr, "opacity": o.opacity_lr, "colors": o.feature_lr}

    fused_loss = None  # set by on_gpu(): FusedL1SSIM

    def loss_and_grad(self, image: torch.Tensor, gt: torch.Tensor):
        """Ll1 and (1-lambda) Ll1 + lambda (1 - SSIM)  (src/gaussian_trainer.cpp:89-90) and its gradient wrt image."""
        if self.fused_loss is not None:
            return self.fused_loss(image, gt)
        img = image.detach().requires_grad_(True)
        Ll1 = loss_utils.l1_loss(img, gt)
        loss = (1.0 - self.opt.lambda_dssim) * Ll1 + self.opt.lambda_dssim * (1.0 - loss_utils.ssim(img, gt))
        (dL,) = torch.autograd.grad(loss, img)
        return loss.detach(), dL.contiguous()

    def _exchange_sharded(self) -> bool:
        return self.exchange.sharded

    def _exchange(self):
        return self.exchange

    def training_once(self, keyframes, gt_images) -> torch.Tensor:
        """Nothing here waits for the device: a pass whose instance count outgrew some rank's resident capacity is dropped by
        every rank on the device (the optimizer is guarded by the all-reduced overflow word and its step count lives there);
        the rank concerned re-sizes its scratch at its next forward.  The dropped iteration is then run again by every rank before
        the next one (`redo_dropped_steps`, step_shared.DroppedStepRedo), so no optimizer step of the reference's sequence is lost
        (src/gaussian_mapper.cpp:1027-1030 never skips one).  CONTRACT: the keyframe's and the target's tensors of a call must
        stay unchanged until the next call (or finish()) has returned -- a redo trains on them again."""
        return self._next_iteration(keyframes, gt_images)

    def _iteration_body(self, keyframe, gt, it: int) -> torch.Tensor:
        lrs = self.learning_rates(it)
        ex = self.exchange
        if self.use_graph and not ex.active:
            loss = self._training_once_graph(keyframe, gt, lrs)
            if loss is not None:
                return loss
        dL_fn = lambda im: self.loss_and_grad(im, gt)  # noqa: E731
        if self._backend_takes_hook:
            loss = self.render_backward(self.params, keyframe, dL_fn, after_forward=ex.reduce_flag_async)
        else:
            loss = self.render_backward(self.params, keyframe, dL_fn)
            ex.reduce_flag_async(None)
        flag = ex.wait_flag()
        ex.reduce_gradients(self.grads_flat)  # sum over the keyframes of this step
        if ex.active and self.redo_dropped_steps:
            ex.mirror_flag()
        self.optimizer.step(self.params_flat, self.grads_flat, lrs, self.P, 1.0 / self.world, exchange=ex, guard=flag)
        ex.gather(self.params_flat)
        return loss

    # ---- whole-iteration hipGraph (the on_gpu wiring: HIP raster engine + fused loss + fused Adam) -------------------------
    def enable_graph(self, on: bool = True):
        """Replay the iteration from a captured hipGraph (single rank, calibrated resident rasterizer): the keyframe matrices,
        the target image and the learning rates go through staging buffers refreshed before each replay; same kernels, same
        arguments, same order as the eager path."""
        assert self.engine is not None and isinstance(self.optimizer, FusedAdam), "graph mode needs TrainerStep.on_gpu()"
        self.use_graph, self._graphs, self._stage, self.graph_replays = bool(on), {}, None, 0

    def _training_once_graph(self, keyframe, gt, lrs):
        eng, opt = self.engine, self.optimizer
        if not self._graph_ready():
            return None
        view, proj, campos, tanx, tany = keyframe
        if self._stage is None:
            self._stage = IterationStage(35, gt)
        st = self._stage
        st.fill((view, proj, campos), gt)
        groups = field_segments(lrs, self.P)
        key = (eng.capacity, eng._bin_r.data_ptr(), float(tanx), float(tany), tuple(gt.shape))

        def body():
            pk = st.packed
            skf = (pk[0:16].view(4, 4), pk[16:32].view(4, 4), pk[32:35], tanx, tany)
            self.render_backward(self.params, skf, lambda im: self.loss_and_grad(im, st.gt))
            adam_step((self.params_flat, self.grads_flat, opt.exp_avg, opt.exp_avg_sq), groups, opt.opt, opt.count,
                      ptr(eng.overflow_word()), self.params_flat.device, staged_lr=st.lr_ptr())

        if not self._replay_iteration(st, groups, (opt.count,), key, 0, lambda: body):   # one graph: a new key replaces it
            return None
        return self.fused_loss.out[0]

    # ---- product wiring -------------------------------------------------------------------------------
    @staticmethod
    def on_gpu(scene, device, opt: Optional[OptimizationParams] = None, process_group=None, sharded_optimizer: bool = True,
               single_rank_collectives: bool = False):
        """HIP raster engine + fused HIP Adam over a segs_slam_amd.scenes.Scene's Gaussians."""
        import numpy as np
        from .raster_engine import RasterEngine
        opt = opt or OptimizationParams()
        P = scene.P
        cam = scene.camera
        eng = RasterEngine(P, cam.width, cam.height, device, resident=True)
        params_flat = torch.empty(FLOATS_PER_GAUSSIAN * P, dtype=torch.float32, device=device)
        views = split_flat(params_flat, P)
        for name, arr in (("means3D", scene.means3D), ("scales", scene.scales), ("rotations", scene.rotations),
                          ("opacity", scene.opacity), ("colors", scene.colors)):
            views[name].copy_(torch.from_numpy(np.ascontiguousarray(arr)))
        bg = torch.from_numpy(scene.bg).to(device)

        def render_backward(params, keyframe, dL_fn, after_forward=None):
            view, proj, campos, tanx, tany = keyframe
            # (a forward that finds the previous pass overflowed goes through the synchronising path and re-sizes the scratch)
            image = eng.forward(bg, params["means3D"], params["colors"], params["opacity"], params["scales"],
                                params["rotations"], view, proj, campos, tanx, tany)
            if after_forward is not None:
                after_forward(eng.overflow_word())
            loss, dL = dL_fn(image)
            eng.backward(dL)
            return loss

        step = TrainerStep(params_flat, P, render_backward, FusedAdam(params_flat.numel(), device, opt), opt, eng.grads_flat,
                           process_group, sharded_optimizer=sharded_optimizer, single_rank_collectives=single_rank_collectives)
        step.engine = eng
        step.fused_loss = FusedL1SSIM(cam.height, cam.width, device, opt.lambda_dssim)
        return step


def keyframe_tensors(cam, device):
    """(view, proj, campos, tanfovx, tanfovy) of a scenes.Camera on `device`."""
    t = lambda a: torch.from_numpy(a).to(device)  # noqa: E731
    return (t(cam.world_view_transform), t(cam.full_proj_transform), t(cam.camera_center), cam.tanfovx, cam.tanfovy)
