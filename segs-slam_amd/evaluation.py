"""Keyframe evaluation on the device (include/segs_eval.h, csrc/eval_metrics.hip).

GaussianMapper::renderAndRecordKeyframe / renderAndRecordAllKeyframes (src/gaussian_mapper.cpp:1769-1840, 1909-1981): render a
keyframe, mask render and target by the target's non-zero (channel, row)s, take SSIM, PSNR and the per-channel PSNR, and record
them -- and, on request, the three images -- under result_dir/<iteration><suffix>/.  The reference reads three scalars back per
keyframe; here every keyframe's numbers go into one row of a device table and the whole set costs one readback at the end.
"""
from __future__ import annotations

import os
from dataclasses import dataclass
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _capi
from .step_shared import ptr, stream_ptr

COLUMNS = ("ssim", "psnr", "psnr_gs", "mse", "mse_r", "mse_g", "mse_b", "l1")      # the eight words of a row (segs_eval.h)
IMAGES = ("image", "gt", "loss")


class FusedImageMetrics:
    """segs_eval_frame / segs_eval_images_u8 at one image size.  `table`: the (n_slots, 8) float32 device tensor the rows go to
    (its own, NaN-filled, unless one is handed in to be shared between sizes)."""

    def __init__(self, H: int, W: int, device, n_slots: int, table: Optional[torch.Tensor] = None):
        self._lib = _capi.lib()
        self.H, self.W, self.n_slots = int(H), int(W), int(n_slots)
        nbytes = int(self._lib.segs_eval_temp_bytes(self.H, self.W))
        if nbytes == 0 or self.n_slots <= 0:
            raise ValueError(f"image size {self.H} x {self.W} or slot count {n_slots} is outside the range of include/segs_eval.h")
        self.temp = torch.empty(nbytes, dtype=torch.uint8, device=device)
        if table is None:
            table = torch.full((self.n_slots, len(COLUMNS)), float("nan"), dtype=torch.float32, device=device)
        assert table.is_cuda and table.is_contiguous() and table.dtype == torch.float32 and tuple(table.shape) == (self.n_slots, len(COLUMNS))
        self.table = table
        self._flags_of = None          # (target pointer, version): whose row flags `temp` holds

    def _check(self, image: torch.Tensor, gt: torch.Tensor):
        for t in (image, gt):
            if not (t.is_cuda and t.is_contiguous() and t.dtype == torch.float32 and tuple(t.shape) == (3, self.H, self.W)):
                raise ValueError(f"image and target are contiguous float32 (3, {self.H}, {self.W}) tensors on the GPU")

    def measure(self, image: torch.Tensor, gt: torch.Tensor, slot: int, row_mask: bool = True) -> None:
        """Row `slot` of the table = the eight numbers of (image, gt).  Launches only: nothing is read back."""
        self._check(image, gt)
        st = self._lib.segs_eval_frame(ptr(image), ptr(gt), self.H, self.W, int(bool(row_mask)), ptr(self.table), self.n_slots,
                                       int(slot), ptr(self.temp), stream_ptr(image.device))
        _capi.check(st, "segs_eval_frame")
        self._flags_of = (gt.data_ptr(), gt._version) if row_mask else None

    def images_u8(self, image: torch.Tensor, gt: torch.Tensor, row_mask: bool = True, which: Sequence[str] = IMAGES) -> Dict[str, torch.Tensor]:
        """The recorded images as uint8 (H, W, 3) RGB device tensors: "image" the masked render, "gt" the masked target, "loss"
        their absolute difference (src/gaussian_mapper.cpp:1820-1840)."""
        self._check(image, gt)
        bad = [w for w in which if w not in IMAGES]
        if bad:
            raise ValueError(f"unknown image name {bad}: choose from {IMAGES}")
        out = {w: torch.empty((self.H, self.W, 3), dtype=torch.uint8, device=image.device) for w in which}
        # the row flags a measure() of this very target left in temp are read again instead of being recomputed
        flags = self.temp if (row_mask and self._flags_of == (gt.data_ptr(), gt._version)) else None
        st = self._lib.segs_eval_images_u8(ptr(image), ptr(gt), self.H, self.W, int(bool(row_mask)), *(ptr(out.get(w)) for w in IMAGES),
                                           ptr(flags), stream_ptr(image.device))
        _capi.check(st, "segs_eval_images_u8")
        return out

    def results(self) -> np.ndarray:
        """THE readback: the table as float64 (n_slots, 8); columns as COLUMNS.  Rows never measured are NaN (own table)."""
        return self.table.cpu().numpy().astype(np.float64)


@dataclass
class RecordParams:
    """The Record.* keys of GaussianMapper::readConfigFromFile (src/gaussian_mapper.cpp:334-347).  Defaults: what an absent key
    reads as there (an empty cv::FileNode converts to 0)."""
    record_rendered_image: bool = False
    record_ground_truth_image: bool = False
    record_loss_image: bool = False
    all_keyframes_record_interval: int = 0
    keyframe_record_interval: int = 0
    training_report_interval: int = 0

    @classmethod
    def from_config(cls, raw) -> "RecordParams":
        """From a flat key -> value mapping (mapper_config.read_opencv_yaml, or an entry of data/mapper_cfgs.json)."""
        def num(key):
            v = raw.get("Record." + key, 0)
            if isinstance(v, str):
                raise ValueError(f"Record.{key} is not numeric: {v!r}")
            return int(v)
        return cls(record_rendered_image=num("record_rendered_image") != 0,
                   record_ground_truth_image=num("record_ground_truth_image") != 0,
                   record_loss_image=num("record_loss_image") != 0,
                   all_keyframes_record_interval=num("all_keyframes_record_interval"),
                   keyframe_record_interval=num("keyframe_record_interval"),
                   training_report_interval=num("training_report_interval"))

    def due(self, iteration: int) -> bool:
        """The interval test of trainForOneIteration (src/gaussian_mapper.cpp:1018)."""
        return bool(self.all_keyframes_record_interval) and iteration % self.all_keyframes_record_interval == 0

    def wanted_images(self) -> Tuple[str, ...]:
        on = (self.record_rendered_image, self.record_ground_truth_image, self.record_loss_image)
        return tuple(w for w, o in zip(IMAGES, on) if o)


@dataclass
class EvalReport:
    """ids[i]: keyframe id; table[i]: its eight numbers (float64 copies of the float32 words; columns as COLUMNS);
    render_ms[i]: its render time.  images[i] (when recorded): {"image" | "gt" | "loss": uint8 (H, W, 3) RGB array}."""
    ids: List[int]
    table: np.ndarray
    render_ms: np.ndarray
    images: Optional[List[Dict[str, np.ndarray]]] = None

    def column(self, name: str) -> np.ndarray:
        return self.table[:, COLUMNS.index(name)]

    # Plain means over the keyframes.  (The reference accumulates into uninitialised floats, src/gaussian_mapper.cpp:1956: what it
    # prints as averages is undefined; these are the numbers it means.)
    @property
    def ssim_mean(self) -> float:
        return float(np.mean(self.column("ssim"))) if len(self.ids) else float("nan")

    @property
    def psnr_mean(self) -> float:
        return float(np.mean(self.column("psnr"))) if len(self.ids) else float("nan")

    @property
    def psnr_gs_mean(self) -> float:
        return float(np.mean(self.column("psnr_gs"))) if len(self.ids) else float("nan")

    @property
    def render_ms_mean(self) -> float:
        return float(np.mean(self.render_ms)) if len(self.ids) else float("nan")


# (file, header line, column or None for the render time, digits): src/gaussian_mapper.cpp:1936-1965
_RECORD_FILES = (
    ("render_time.txt", "##[Gaussian Mapper]Render time statistics: keyframe id, time(milliseconds)", None, 8),
    ("dssim.txt", "##[Gaussian Mapper]keyframe id, dssim", "ssim", 10),
    ("psnr.txt", "##[Gaussian Mapper]keyframe id, psnr", "psnr", 10),
    ("psnr_gaussian_splatting.txt", "##[Gaussian Mapper]keyframe id, psnr_gaussian_splatting", "psnr_gs", 10),
)
# (directory, file name suffix): src/gaussian_mapper.cpp:1824, 1831, 1839, 1915-1923
_IMAGE_DIRS = {"image": ("image", ""), "gt": ("image_gt", ""), "loss": ("image_loss", "_loss")}


class KeyframeEvaluator:
    """renderAndRecordAllKeyframes on a ScaffoldTrainerStep.  Inert for training: parameters, Adam moments and step counts, the
    densification statistics and the iteration number are not touched -- an evaluation is forwards only -- and the step is left
    at the pyramid level it was at.  An iteration the device dropped is run again first (step.finish()), as before anything
    else that renders between two iterations (seed_keyframe, pose_gradient): afterwards nothing is pending."""

    def __init__(self, step, record: Optional[RecordParams] = None):
        self.step = step
        self.record = record if record is not None else RecordParams()
        self.table = None
        self._metrics = {}

    def reserve(self, n_slots: int):
        """A table of at least n_slots rows (rows already measured are kept)."""
        if self.table is not None and self.table.shape[0] >= n_slots:
            return
        new = torch.full((int(n_slots), len(COLUMNS)), float("nan"), dtype=torch.float32, device=self.step.model.device)
        if self.table is not None:
            new[:self.table.shape[0]] = self.table
        self.table = new
        self._metrics.clear()

    def metrics(self, H: int, W: int) -> FusedImageMetrics:
        """The FusedImageMetrics of one image size, all writing into the evaluator's table."""
        m = self._metrics.get((H, W))
        if m is None:
            m = self._metrics[(H, W)] = FusedImageMetrics(H, W, self.step.model.device, self.table.shape[0], self.table)
        return m

    def _render(self, kf):
        step = self.step
        dev = step.model.device
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        if step.model.A == 0:     # every anchor was pruned: a zero image, as in the reference's rasterizer (src/rasterize_points.cu:81)
            start.record(torch.cuda.current_stream(dev))
            image = torch.zeros(3, step.H, step.W, device=dev)
            end.record(torch.cuda.current_stream(dev))
            return image, start, end
        for attempt in range(2):
            start.record(torch.cuda.current_stream(dev))
            image = step.render(kf)
            end.record(torch.cuda.current_stream(dev))
            if not step.engine.resident or step.engine.check(raise_on_overflow=False):
                return image, start, end
            # the resident scratch overflowed (first use of a size, or a map that grew): the next forward re-calibrates
        raise RuntimeError("resident rasterizer kept overflowing its re-sized scratch")

    def evaluate(self, kf, gt: torch.Tensor, slot: int, want_images: Sequence[str] = ()):
        """Render `kf` at the size of `gt`, measure against `gt` into row `slot` (with the step's row_mask setting), restore the
        step's level.  Returns (start event, end event, images): the events bracket the render; images = images_u8 of
        `want_images` (device tensors) or None."""
        step = self.step
        step.finish()
        self.reserve(slot + 1)
        level = (step.W, step.H)
        H, W = int(gt.shape[-2]), int(gt.shape[-1])
        try:
            step.use_level(W, H)
            image, start, end = self._render(kf)
            m = self.metrics(H, W)
            m.measure(image, gt, slot, row_mask=step.row_mask)
            images = m.images_u8(image, gt, row_mask=step.row_mask, which=tuple(want_images)) if want_images else None
        finally:
            step.use_level(*level)
        return start, end, images

    def evaluate_all(self, items: Iterable[Tuple[int, object, torch.Tensor]]) -> EvalReport:
        """items: (keyframe id, keyframe, target image) triples.  One host readback of the table after a single synchronise.
        With a record_* switch on, each keyframe's recorded images are also copied to the host as they are made."""
        items = list(items)
        self.reserve(max(len(items), 1))
        want = self.record.wanted_images()
        events, images = [], ([] if want else None)
        for slot, (_kfid, kf, gt) in enumerate(items):
            start, end, im = self.evaluate(kf, gt, slot, want)
            events.append((start, end))
            if want:
                images.append({k: v.cpu().numpy() for k, v in im.items()})
        torch.cuda.synchronize(self.step.model.device)
        table = self.table[:len(items)].cpu().numpy().astype(np.float64)
        render_ms = np.array([s.elapsed_time(e) for s, e in events], dtype=np.float64)
        return EvalReport([int(i[0]) for i in items], table, render_ms, images)

    def write(self, report: EvalReport, result_dir: str, iteration: int, suffix: str = "") -> List[str]:
        """The record files of renderAndRecordAllKeyframes under result_dir/<iteration><suffix>/ (src/gaussian_mapper.cpp:1912,
        1936-1965: header line, then `<keyframe id> <value>` per line, std::fixed with 8 digits for the time and 10 for the
        others), and -- per record_* switch -- the JPEG images image/<iteration>_<id>.jpg, image_gt/<iteration>_<id>.jpg and
        image_loss/<iteration>_<id>_loss.jpg.  Returns the paths written."""
        return write_report(report, self.record, result_dir, iteration, suffix)


def _fixed(value: float, digits: int) -> str:
    return f"{float(value):.{digits}f}"          # std::fixed: "inf" / "nan" for the non-finite, like operator<<


def write_report(report: EvalReport, record: RecordParams, result_dir: str, iteration: int, suffix: str = "") -> List[str]:
    out_dir = os.path.join(result_dir, f"{int(iteration)}{suffix}")
    want = record.wanted_images()
    if want:
        if report.images is None or any(w not in im for im in report.images for w in want):
            raise ValueError("the report holds no recorded images: evaluate with the same RecordParams that write() is given")
        try:
            from PIL import Image
        except ImportError as e:
            raise RuntimeError("recording images (Record.record_*_image) needs Pillow to encode the JPEG files; it is not installed") from e
    os.makedirs(out_dir, exist_ok=True)
    paths = []
    for name, header, column, digits in _RECORD_FILES:
        values = report.render_ms if column is None else report.column(column)
        path = os.path.join(out_dir, name)
        with open(path, "w", newline="\n") as f:
            f.write(header + "\n")
            for kfid, v in zip(report.ids, values):
                f.write(f"{kfid} {_fixed(v, digits)}\n")
        paths.append(path)
    for w in want:
        sub, tail = _IMAGE_DIRS[w]
        os.makedirs(os.path.join(out_dir, sub), exist_ok=True)
        for kfid, im in zip(report.ids, report.images):
            path = os.path.join(out_dir, sub, f"{int(iteration)}_{kfid}{tail}.jpg")
            Image.fromarray(np.ascontiguousarray(im[w])).save(path, quality=95)     # 95: cv::imwrite's default
            paths.append(path)
    return paths
