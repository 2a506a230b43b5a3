"""Host-side mirror of include/gaussian_rasterizer.h:25-151 / src/gaussian_rasterizer.cpp.

GaussianRasterizationSettings, GaussianRasterizerFunction (autograd), rasterizeGaussians and the
GaussianRasterizer module keep the reference's names, argument order and error behaviour.
GaussianRasterizerDepthFunction, rasterizeGaussiansWithDepth and GaussianRasterizer.forward_with_depth have no reference
counterpart: the same render plus a differentiable depth map (sum z alpha T) and alpha map (1 - T_final).
GaussianRasterizerCameraFunction, rasterizeGaussiansWithCameraGrad and GaussianRasterizer.forward_with_camera_grad (no reference
counterpart either) take viewmatrix and projmatrix as tensor inputs of the autograd function, so that a loss on colour, depth or
alpha also differentiates with respect to the camera (pose refinement, bundle adjustment of keyframe poses).
"""
from __future__ import annotations

from dataclasses import dataclass

import torch

from . import rasterize_points as rp


@dataclass
class GaussianRasterizationSettings:
    """include/gaussian_rasterizer.h:25-57 (fields keep the reference's trailing underscore)."""
    image_height_: int
    image_width_: int
    tanfovx_: float
    tanfovy_: float
    bg_: torch.Tensor
    scale_modifier_: float
    viewmatrix_: torch.Tensor
    projmatrix_: torch.Tensor
    sh_degree_: int
    campos_: torch.Tensor
    prefiltered_: bool = False


def _raster_forward(ctx, fn, means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, viewmatrix, projmatrix,
                    sh_degree, rs):
    """The forward of the three Functions: calls rp.`fn`, keeps on ctx what _raster_backward needs
    -> fn's outputs without num_rendered and the three buffers: (color, radii[, depth, alpha])."""
    num_rendered, *outputs, geomBuffer, binningBuffer, imgBuffer = fn(
        rs.bg_, means3D, colors_precomp, opacities, scales, rotations, rs.scale_modifier_, cov3Ds_precomp, viewmatrix, projmatrix,
        rs.tanfovx_, rs.tanfovy_, rs.image_height_, rs.image_width_, sh, sh_degree, rs.campos_, rs.prefiltered_)
    radii = outputs[1]
    ctx.num_rendered = num_rendered
    ctx.scale_modifier = rs.scale_modifier_
    ctx.tanfovx, ctx.tanfovy = rs.tanfovx_, rs.tanfovy_
    ctx.sh_degree = sh_degree
    ctx.save_for_backward(rs.bg_, viewmatrix, projmatrix, rs.campos_, colors_precomp, means3D, scales, rotations, cov3Ds_precomp,
                          radii, sh, geomBuffer, binningBuffer, imgBuffer)
    ctx.mark_non_differentiable(radii)
    return tuple(outputs)


def _raster_backward(ctx, fn, grad_out_color, *grad_maps):
    """Calls rp.`fn` on what _raster_forward kept -> (gradients of means3D, means2D, sh, colors_precomp, opacities, scales, rotations,
    cov3Ds_precomp: the order of src/gaussian_rasterizer.cpp:143-153, "absent" inputs (0-element tensors) get None; fn's tuple),
    or None when no gradient arrived at all (the map forms, which leave an unused output's gradient None)."""
    (bg, viewmatrix, projmatrix, campos, colors_precomp, means3D, scales, rotations, cov3Ds_precomp, radii, sh,
     geomBuffer, binningBuffer, imgBuffer) = ctx.saved_tensors
    if grad_maps:      # a None map gradient goes down as NULL: no work for it
        ref = next((t for t in (grad_out_color, *grad_maps) if t is not None), None)
        if ref is None:
            return None
        if grad_out_color is None:      # only a map gradient arrived: a zero colour gradient stands in
            grad_out_color = torch.zeros((3,) + tuple(ref.shape), dtype=torch.float32, device=means3D.device)
        grad_out_color, *grad_maps = (t.contiguous() if t is not None else None for t in (grad_out_color, *grad_maps))
    out = fn(bg, means3D, radii, colors_precomp, scales, rotations, ctx.scale_modifier, cov3Ds_precomp, viewmatrix, projmatrix,
             ctx.tanfovx, ctx.tanfovy, grad_out_color, *grad_maps, sh, ctx.sh_degree, campos, geomBuffer, ctx.num_rendered,
             binningBuffer, imgBuffer)
    dL_dmeans2D, dL_dcolors, dL_dopacity, dL_dmeans3D, dL_dcov3D, dL_dsh, dL_dscales, dL_drotations = out[:8]
    g = lambda t, ref: t if ref.numel() != 0 else None  # noqa: E731
    return (dL_dmeans3D, dL_dmeans2D, g(dL_dsh, sh), g(dL_dcolors, colors_precomp), dL_dopacity, g(dL_dscales, scales),
            g(dL_drotations, rotations), g(dL_dcov3D, cov3Ds_precomp)), out


class GaussianRasterizerFunction(torch.autograd.Function):
    """src/gaussian_rasterizer.cpp:27-154."""

    @staticmethod
    def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, raster_settings):
        rs = raster_settings
        return _raster_forward(ctx, rp.RasterizeGaussiansCUDA, means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                        rs.viewmatrix_, rs.projmatrix_, rs.sh_degree_, rs)

    @staticmethod
    def backward(ctx, grad_out_color, _grad_radii=None):
        return _raster_backward(ctx, rp.RasterizeGaussiansBackwardCUDA, grad_out_color)[0] + (None,)


class GaussianRasterizerDepthFunction(torch.autograd.Function):
    """GaussianRasterizerFunction plus the depth and alpha maps (rasterize_points.RasterizeGaussiansDepthCUDA)."""

    @staticmethod
    def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, raster_settings):
        rs = raster_settings
        ctx.set_materialize_grads(False)
        return _raster_forward(ctx, rp.RasterizeGaussiansDepthCUDA, means3D, sh, colors_precomp, opacities, scales, rotations,
                        cov3Ds_precomp, rs.viewmatrix_, rs.projmatrix_, rs.sh_degree_, rs)

    @staticmethod
    def backward(ctx, grad_out_color, _grad_radii=None, grad_depth=None, grad_alpha=None):
        g = _raster_backward(ctx, rp.RasterizeGaussiansDepthBackwardCUDA, grad_out_color, grad_depth, grad_alpha)
        return g[0] + (None,) if g else (None,) * 9


class GaussianRasterizerCameraFunction(torch.autograd.Function):
    """GaussianRasterizerDepthFunction with viewmatrix and projmatrix as differentiable inputs: two independent (4, 4) tensors in
    the transposed layout, the ones of raster_settings being ignored (rasterize_points.RasterizeGaussiansCameraBackwardCUDA).
    Precomputed colours only: the SH colours depend on campos, whose gradient is not provided."""

    @staticmethod
    def forward(ctx, means3D, means2D, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, viewmatrix, projmatrix,
                raster_settings):
        ctx.set_materialize_grads(False)
        no_sh = torch.empty(0, dtype=torch.float32, device=means3D.device)
        return _raster_forward(ctx, rp.RasterizeGaussiansDepthCUDA, means3D, no_sh, colors_precomp, opacities, scales, rotations,
                        cov3Ds_precomp, viewmatrix, projmatrix, 0, raster_settings)

    @staticmethod
    def backward(ctx, grad_out_color, _grad_radii=None, grad_depth=None, grad_alpha=None):
        g = _raster_backward(ctx, rp.RasterizeGaussiansCameraBackwardCUDA, grad_out_color, grad_depth, grad_alpha)
        if g is None:
            return (None,) * 10
        (dL_dmeans3D, dL_dmeans2D, _, _, dL_dopacity, dL_dscales, dL_drotations, dL_dcov3D), out = g
        viewmatrix, projmatrix = ctx.saved_tensors[1:3]
        return (dL_dmeans3D, dL_dmeans2D, out[1], dL_dopacity, dL_dscales, dL_drotations, dL_dcov3D, out[8].to(viewmatrix.dtype),
                out[9].to(projmatrix.dtype), None)      # out[1]: dL_dcolors as the wrapper returns it, never "absent" here


def rasterizeGaussians(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, raster_settings):
    """include/gaussian_rasterizer.h:79-101."""
    return GaussianRasterizerFunction.apply(means3D, means2D, sh, colors_precomp, opacities, scales, rotations,
                                            cov3Ds_precomp, raster_settings)


def rasterizeGaussiansWithDepth(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, raster_settings):
    """rasterizeGaussians plus the depth and alpha maps: -> (color (3,H,W), radii (P), depth (H,W), alpha (H,W))."""
    return GaussianRasterizerDepthFunction.apply(means3D, means2D, sh, colors_precomp, opacities, scales, rotations,
                                                 cov3Ds_precomp, raster_settings)


def rasterizeGaussiansWithCameraGrad(means3D, means2D, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, viewmatrix,
                                     projmatrix, raster_settings):
    """rasterizeGaussiansWithDepth with the two camera matrices as differentiable (4, 4) tensor inputs (transposed layout; the
    ones inside raster_settings are not used): -> (color (3,H,W), radii (P), depth (H,W), alpha (H,W)).  After backward(),
    viewmatrix.grad / projmatrix.grad -- or whatever pose parameters produced them -- are filled."""
    return GaussianRasterizerCameraFunction.apply(means3D, means2D, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                                                  viewmatrix, projmatrix, raster_settings)


class GaussianRasterizer(torch.nn.Module):
    """include/gaussian_rasterizer.h:103-151, src/gaussian_rasterizer.cpp:19-25,156-307."""

    def __init__(self, raster_settings: GaussianRasterizationSettings):
        super().__init__()
        self.raster_settings_ = raster_settings

    @staticmethod
    def _or_absent(like: torch.Tensor, has, tensors):
        """-> each of `tensors`, or where its `has` is false the reference's "absent": a 0-element tensor on like's device."""
        e = torch.empty(0, dtype=torch.float32, device=like.device)
        return [t if h else e for h, t in zip(has, tensors)]

    def markVisibleGaussians(self, positions):
        with torch.no_grad():
            rs = self.raster_settings_
            return rp.markVisible(positions, rs.viewmatrix_, rs.projmatrix_)

    def _check(self, has_shs, has_colors_precomp, has_scales, has_rotations, has_cov3D_precomp):
        if (not has_shs and not has_colors_precomp) or (has_shs and has_colors_precomp):
            raise RuntimeError("Please provide excatly one of either SHs or precomputed colors!")
        if ((not has_scales or not has_rotations) and not has_cov3D_precomp) or \
                ((has_scales or has_rotations) and has_cov3D_precomp):
            raise RuntimeError("Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!")

    def forward(self, means3D, means2D, opacities, has_shs, has_colors_precomp, has_scales, has_rotations,
                has_cov3D_precomp, shs=None, colors_precomp=None, scales=None, rotations=None, cov3D_precomp=None):
        self._check(has_shs, has_colors_precomp, has_scales, has_rotations, has_cov3D_precomp)
        shs, colors_precomp, scales, rotations, cov3D_precomp = self._or_absent(
            means3D, (has_shs, has_colors_precomp, has_scales, has_rotations, has_cov3D_precomp),
            (shs, colors_precomp, scales, rotations, cov3D_precomp))
        color, radii = rasterizeGaussians(means3D, means2D, shs, colors_precomp, opacities, scales, rotations,
                                          cov3D_precomp, self.raster_settings_)
        return color, radii

    def forward_with_depth(self, means3D, means2D, opacities, has_shs, has_colors_precomp, has_scales, has_rotations,
                           has_cov3D_precomp, shs=None, colors_precomp=None, scales=None, rotations=None, cov3D_precomp=None):
        """forward() plus the depth map (sum z alpha T) and alpha map (1 - T_final): -> (color, radii, depth, alpha)."""
        self._check(has_shs, has_colors_precomp, has_scales, has_rotations, has_cov3D_precomp)
        shs, colors_precomp, scales, rotations, cov3D_precomp = self._or_absent(
            means3D, (has_shs, has_colors_precomp, has_scales, has_rotations, has_cov3D_precomp),
            (shs, colors_precomp, scales, rotations, cov3D_precomp))
        return rasterizeGaussiansWithDepth(means3D, means2D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp,
                                           self.raster_settings_)

    def forward_with_camera_grad(self, means3D, means2D, opacities, has_scales, has_rotations, has_cov3D_precomp, colors_precomp,
                                 scales=None, rotations=None, cov3D_precomp=None, viewmatrix=None, projmatrix=None):
        """forward_with_depth() differentiable with respect to the camera too: viewmatrix / projmatrix (default: the settings'
        tensors) are inputs of the autograd graph.  Precomputed colours only.  -> (color, radii, depth, alpha)."""
        self._check(False, True, has_scales, has_rotations, has_cov3D_precomp)
        rs = self.raster_settings_
        scales, rotations, cov3D_precomp = self._or_absent(means3D, (has_scales, has_rotations, has_cov3D_precomp),
                                                           (scales, rotations, cov3D_precomp))
        return rasterizeGaussiansWithCameraGrad(means3D, means2D, colors_precomp, opacities, scales, rotations, cov3D_precomp,
                                                rs.viewmatrix_ if viewmatrix is None else viewmatrix,
                                                rs.projmatrix_ if projmatrix is None else projmatrix, rs)

    def visible_filter(self, means3D, has_scales, has_rotations, has_cov3D_precomp, scales=None, rotations=None,
                       cov3D_precomp=None):
        rs = self.raster_settings_
        scales, rotations, cov3D_precomp = self._or_absent(means3D, (has_scales, has_rotations, has_cov3D_precomp),
                                                           (scales, rotations, cov3D_precomp))
        with torch.no_grad():
            return rp.RasterizeGaussiansfilterCUDA(means3D, scales, rotations, rs.scale_modifier_, cov3D_precomp,
                                                   rs.viewmatrix_, rs.projmatrix_, rs.tanfovx_, rs.tanfovy_,
                                                   rs.image_height_, rs.image_width_, rs.prefiltered_, False)

    def project2_image(self, means3D, means2D, opacities, has_shs, has_colors_precomp, has_scales, has_rotations,
                       has_cov3D_precomp, shs=None, colors_precomp=None, scales=None, rotations=None, cov3D_precomp=None):
        self._check(has_shs, has_colors_precomp, has_scales, has_rotations, has_cov3D_precomp)
        rs = self.raster_settings_
        shs, colors_precomp, scales, rotations, cov3D_precomp = self._or_absent(
            means3D, (has_shs, has_colors_precomp, has_scales, has_rotations, has_cov3D_precomp),
            (shs, colors_precomp, scales, rotations, cov3D_precomp))
        points_image_2d, radii, color = rp.RasterizeGaussiansprojectCUDA(
            rs.bg_, means3D, colors_precomp, opacities, scales, rotations, rs.scale_modifier_, cov3D_precomp,
            rs.viewmatrix_, rs.projmatrix_, rs.tanfovx_, rs.tanfovy_, rs.image_height_, rs.image_width_, shs,
            rs.sh_degree_, rs.campos_, rs.prefiltered_)
        return points_image_2d, radii, color
