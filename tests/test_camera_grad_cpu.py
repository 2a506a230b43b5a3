"""CPU-side checks of the camera gradient (segs_*_camera, include/segs_raster.h), and the float64 references its GPU tests share.

The gradient of a render with respect to the two camera matrices (viewmatrix V and projmatrix PV, two independent inputs in the
transposed layout t_i = sum_j V[4 j + i] p_j + V[12 + i]) is a sum over the binned Gaussians of per-Gaussian contributions c_i:

  dL/dV[12 + i]  += dt_i                                          dt = dL/dt of the per-Gaussian backward (+ dL/dz on t_z)
  dL/dV[4 j + i] += dt_i p_j + (J^T dM2)[i][j]                    dM2 = dL/d(J Wv): the Wv inside M2 = J Wv enters on its own
  dL/dPV[4 j + i] += dh_i p_j (p_3 = 1)                           dh = (g.x w, g.y w, 0, -(g.x hom.x + g.y hom.y) w^2)

`contributions_f64` evaluates the c_i in float64 from those equations (the layout of oracle/preprocess_backward_f64.py, extended),
fed the CPU oracle's dL_dmean2D / dL_dconic; `autograd_truth` is float64 autograd of oracle.torch_ref.render with V and PV as
leaves.  The entries are cancelling sums -- |entry| goes down to 0.003 of S_k = sum_i |c_ik| on scene G, one entry is ~0 -- so
every bar here is relative to S_k: 1e-5 S_k for the closed form against autograd (this file: it pins the arithmetic the GPU
tests measure the device against; float32 inputs put it at <= 1e-6 S_k), 1e-4 S_k for the device (tests/test_camera_grad_gpu.py:
the project's per-Gaussian relative gradient bar carried through the sum).
"""
import functools
import os
import re

import numpy as np
import torch

from oracle import gs_oracle
from segs_slam_amd import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- scenes -------------------------------------------------------------------------------------------------------------------
def scene_G():
    """3000 @ 160x96: 12 workgroups, 2379 binned (test_depth_render_gpu._gradient_scene)."""
    from tests.test_depth_render_gpu import _gradient_scene
    return _gradient_scene()


def scene_C():
    """600 @ 96x64 seen through a rotated camera with a wider field of view than the scene was drawn for: binned Gaussians whose
    view-space x / z or y / z is clamped to 1.3 tan(fov / 2) (no stock scene has one)."""
    sc = scenes.make_scene(600, 96, 64, 80.0, 80.0, seed=321, bg=(0.1, 0.3, 0.2))
    sc.scales *= 4.0
    sc.camera = scenes.keyframe_camera(96, 64, 144.0, 144.0, seed=11, keyframe=0)
    sc.dL_dout_color[:] = (scenes.uniform01(sc.dL_dout_color.size, 91, 9).reshape(sc.dL_dout_color.shape) * 2 - 1)
    return sc


def clamped_mask(sc, radii):
    cam = sc.camera
    V = cam.world_view_transform.reshape(4, 4).astype(np.float64)
    t = sc.means3D.astype(np.float64) @ V[:3, :3] + V[3, :3]
    return (radii > 0) & ((np.abs(t[:, 0] / t[:, 2]) > 1.3 * cam.tanfovx) | (np.abs(t[:, 1] / t[:, 2]) > 1.3 * cam.tanfovy))


def map_weights(sc, unstable):
    """dL/dcolour of the scene and the depth / alpha weights of test_depth_and_alpha_gradients_match_float64_colour_trick, zero on
    the unstable pixels."""
    cam = sc.camera
    rng = np.random.default_rng(77)
    dL = sc.dL_dout_color.copy()
    dD = (0.5 * rng.uniform(-1, 1, (cam.height, cam.width))).astype(np.float32)
    dA = rng.uniform(-1, 1, (cam.height, cam.width)).astype(np.float32)
    for x in (dL[0], dL[1], dL[2], dD, dA):
        x[unstable] = 0.0
    return dL, dD, dA


# ---- the closed form ----------------------------------------------------------------------------------------------------------
def contributions_f64(m3, sc, rot, view, proj, W, H, tx, ty, g2, gc, radii, mod=1.0, dz=None, cov3D=None, with_jt=True):
    """(P, 32) float64: per-Gaussian contributions to [dL/dV (16) | dL/dPV (16)], entry 4 j + i of each; zero rows where radii <= 0.
    dz: per-Gaussian dL/dz of the view-space depth (the depth form), or None.  cov3D: (P, 6) covariances instead of sc / rot.
    with_jt=False leaves out the J^T dM2 term (what pushing dL/dmean3D through the chain would give)."""
    f = np.float64
    m3, view, proj, g2, gc = (np.asarray(a).astype(f) for a in (m3, view, proj, g2, gc))
    hx_, hy_ = W / (2 * tx), H / (2 * ty)
    V = view.reshape(4, 4)      # V[j, i] = view[4 j + i]
    Wv = V[:3, :3].T            # Wv[i][j] = view[4 j + i]
    t = m3 @ V[:3, :3] + V[3, :3]
    limx, limy = 1.3 * tx, 1.3 * ty
    rx, ry = t[:, 0] / t[:, 2], t[:, 1] / t[:, 2]
    fx, fy = ~((rx < -limx) | (rx > limx)), ~((ry < -limy) | (ry > limy))
    txc, tyc, tz = np.clip(rx, -limx, limx) * t[:, 2], np.clip(ry, -limy, limy) * t[:, 2], t[:, 2]
    P = m3.shape[0]
    J = np.zeros((P, 2, 3)); J[:, 0, 0] = hx_ / tz; J[:, 0, 2] = -hx_ * txc / tz**2; J[:, 1, 1] = hy_ / tz; J[:, 1, 2] = -hy_ * tyc / tz**2
    M2 = J @ Wv
    if cov3D is not None:
        c6 = np.asarray(cov3D).astype(f)
        Sigma = np.stack([np.stack([c6[:, 0], c6[:, 1], c6[:, 2]], 1), np.stack([c6[:, 1], c6[:, 3], c6[:, 4]], 1),
                          np.stack([c6[:, 2], c6[:, 4], c6[:, 5]], 1)], 1)
    else:
        r, x, y, z = np.asarray(rot).astype(f).T
        R = np.stack([np.stack([1 - 2 * (y*y + z*z), 2 * (x*y - r*z), 2 * (x*z + r*y)], 1),
                      np.stack([2 * (x*y + r*z), 1 - 2 * (x*x + z*z), 2 * (y*z - r*x)], 1),
                      np.stack([2 * (x*z - r*y), 2 * (y*z + r*x), 1 - 2 * (x*x + y*y)], 1)], 1)
        L = R * (mod * np.asarray(sc).astype(f))[:, None, :]
        Sigma = L @ L.transpose(0, 2, 1)
    E = M2 @ Sigma              # = U L^T
    Cm = E @ M2.transpose(0, 2, 1); a = Cm[:, 0, 0] + 0.3; b = Cm[:, 0, 1]; c = Cm[:, 1, 1] + 0.3
    det = a * c - b * b; k = 1 / (det**2 + 1e-7)
    G = np.zeros((P, 2, 2)); G[:, 0, 0] = gc[:, 0, 0]; G[:, 0, 1] = G[:, 1, 0] = gc[:, 0, 1]; G[:, 1, 1] = gc[:, 1, 1]
    adj = np.zeros((P, 2, 2)); adj[:, 0, 0] = c; adj[:, 0, 1] = adj[:, 1, 0] = -b; adj[:, 1, 1] = a
    Dc = -k[:, None, None] * (adj @ G @ adj)
    dM2 = 2 * Dc @ E
    dJ = dM2 @ Wv.T
    dtx = np.where(fx, -hx_ / tz**2 * dJ[:, 0, 2], 0.0); dty = np.where(fy, -hy_ / tz**2 * dJ[:, 1, 2], 0.0)
    dtz = -hx_ / tz**2 * dJ[:, 0, 0] - hy_ / tz**2 * dJ[:, 1, 1] + 2 * hx_ * txc / tz**3 * dJ[:, 0, 2] + 2 * hy_ * tyc / tz**3 * dJ[:, 1, 2]
    if dz is not None:
        dtz = dtz + np.asarray(dz).astype(f)
    dt = np.stack([dtx, dty, dtz], 1)
    dWv = J.transpose(0, 2, 1) @ dM2 if with_jt else np.zeros((P, 3, 3))       # [i][j]
    out = np.zeros((P, 32))
    for i in range(3):
        out[:, 12 + i] = dt[:, i]
        for j in range(3):
            out[:, 4 * j + i] = dt[:, i] * m3[:, j] + dWv[:, i, j]
    PV = proj.reshape(4, 4)
    hom = m3 @ PV[:3, :] + PV[3, :]
    w = 1 / (hom[:, 3] + 1e-7)
    dh = np.stack([g2[:, 0] * w, g2[:, 1] * w, np.zeros(P), -(g2[:, 0] * hom[:, 0] + g2[:, 1] * hom[:, 1]) * w * w], 1)
    p1 = np.concatenate([m3, np.ones((P, 1))], 1)
    for i in range(4):
        for j in range(4):
            out[:, 16 + 4 * j + i] = dh[:, i] * p1[:, j]
    out[~(np.asarray(radii) > 0)] = 0
    return out


def scene_contributions(sc, o, g2, gc, **kw):
    cam = sc.camera
    return contributions_f64(sc.means3D, sc.scales, sc.rotations, cam.world_view_transform, cam.full_proj_transform, cam.width,
                             cam.height, cam.tanfovx, cam.tanfovy, g2, gc, o.get("radii"), sc.scale_modifier, **kw)


STRUCTURAL_ZEROS = [3, 7, 11, 15] + [16 + e for e in (2, 6, 10, 14)]     # dL/dV[4 j + 3], dL/dPV[4 j + 2]


# ---- the truth ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case(name):
    """-> (scene, oracle after its forward, unstable pixel mask, (dL, dD, dA) with the unstable pixels zeroed)."""
    sc = {"G": scene_G, "C": scene_C}[name]()
    o, _ = gs_oracle.run_scene(sc, backward=False)
    unstable = o.unstable_pixels(3e-3)
    assert unstable.mean() < 0.05, float(unstable.mean())
    return sc, o, unstable, map_weights(sc, unstable)


def _oracle_trick(sc, colors, dL_first_channel):
    """Oracle backward of the same Gaussians with `colors` on black and the loss weights on channel 0 only."""
    cam = sc.camera
    o = gs_oracle.Oracle()
    o.forward(np.zeros(3, np.float32), sc.means3D, colors, sc.opacity, sc.scales, sc.scale_modifier, sc.rotations,
              cam.world_view_transform, cam.full_proj_transform, cam.tanfovx, cam.tanfovy, cam.height, cam.width)
    dL = np.zeros((3, cam.height, cam.width), np.float32)
    dL[0] = dL_first_channel
    return o.backward(dL)


def inputs_for(sc, o, dL, dD=None, dA=None):
    """What the closed form is fed: the CPU oracle's dL_dmean2D / dL_dconic of the colour loss and, with depth / alpha weights, of
    those losses too -- the oracle backwards of colours (z, z, z) and (1, 1, 1) on black, whose g2 / gc add -- plus
    dz = dL/dcolour[:, 0] of the (z, z, z) one.  -> (g2, gc, dz or None)."""
    ref = o.backward(dL)
    g2, gc, dz = ref["dL_dmean2D"].astype(np.float64), ref["dL_dconic"].astype(np.float64), None
    if dD is not None:
        z = o.get("depths").reshape(-1, 1).repeat(3, 1).astype(np.float32)
        rz = _oracle_trick(sc, z, dD)
        r1 = _oracle_trick(sc, np.ones((sc.P, 3), np.float32), dA)
        g2 = g2 + rz["dL_dmean2D"] + r1["dL_dmean2D"]
        gc = gc + rz["dL_dconic"] + r1["dL_dconic"]
        dz = rz["dL_dcolor"][:, 0].astype(np.float64)
    return g2, gc, dz


@functools.lru_cache(maxsize=None)
def oracle_inputs(name, maps):
    sc, o, unstable, (dL, dD, dA) = case(name)
    return inputs_for(sc, o, dL, dD, dA) if maps else inputs_for(sc, o, dL)


def render_losses(sc, o, V, PV, dL, dD=None, dA=None):
    """Float64 torch_ref renders with the (4, 4) float64 tensors V / PV in the graph -> (colour loss, depth + alpha loss or None);
    the maps are the colour trick's: colours (z, z, z) with z = the view-space depth THROUGH V, and (1, 1, 1), on black.  Tile
    membership comes from the oracle's radii / means2D."""
    from oracle import torch_ref
    cam = sc.camera
    t64 = lambda a: torch.tensor(np.asarray(a, dtype=np.float64))  # noqa: E731
    m, s, r, op, col = t64(sc.means3D), t64(sc.scales), t64(sc.rotations), t64(sc.opacity), t64(sc.colors)
    common = (V, PV, cam.tanfovx, cam.tanfovy, cam.height, cam.width, torch.tensor(o.get("radii")), torch.tensor(o.get("means2D")),
              sc.scale_modifier)
    img, _ = torch_ref.render(m, s, r, op, col, t64(sc.bg), *common)
    colour, maps = (img * t64(dL)).sum(), None
    if dD is not None:
        black = torch.zeros(3, dtype=torch.float64)
        z = m @ V[:3, 2] + V[3, 2]                   # view[2] x + view[6] y + view[10] z + view[14]
        img_z, _ = torch_ref.render(m, s, r, op, z[:, None].expand(-1, 3), black, *common)
        img_1, _ = torch_ref.render(m, s, r, op, torch.ones(sc.P, 3, dtype=torch.float64), black, *common)
        maps = (img_z[0] * t64(dD)).sum() + (img_1[0] * t64(dA)).sum()
    return colour, maps


@functools.lru_cache(maxsize=None)
def autograd_truth(name, maps):
    """Float64 autograd of torch_ref.render with V and PV as leaves -> dict(colour=(32,), maps=(32,) or None): [dL/dV | dL/dPV] of
    the colour loss and of the depth + alpha loss.  The unstable pixels carry no weight."""
    sc, o, unstable, (dL, dD, dA) = case(name)
    cam = sc.camera
    V = torch.tensor(cam.world_view_transform.astype(np.float64), requires_grad=True)
    PV = torch.tensor(cam.full_proj_transform.astype(np.float64), requires_grad=True)
    colour, extra = render_losses(sc, o, V, PV, dL, dD if maps else None, dA if maps else None)
    flat = lambda g: np.concatenate([g[0].numpy().reshape(-1), g[1].numpy().reshape(-1)])  # noqa: E731
    return dict(colour=flat(torch.autograd.grad(colour, (V, PV))), maps=flat(torch.autograd.grad(extra, (V, PV))) if maps else None)


def worst_ratio(have, want, S):
    """max_k |have_k - want_k| / S_k over the entries with S_k > 0; entries with S_k == 0 must agree exactly."""
    have, want, S = (np.asarray(a, dtype=np.float64).reshape(-1) for a in (have, want, S))
    dead = S == 0
    assert np.array_equal(have[dead], want[dead])
    return float((np.abs(have - want)[~dead] / S[~dead]).max()) if (~dead).any() else 0.0


# ---- tests --------------------------------------------------------------------------------------------------------------------
def test_closed_form_matches_float64_autograd_on_both_scenes():
    for name in ("G", "C"):
        sc, o, unstable, _ = case(name)
        g2, gc, _ = oracle_inputs(name, False)
        c = scene_contributions(sc, o, g2, gc)
        S = np.abs(c).sum(0)
        want = autograd_truth(name, name == "G")["colour"]
        ratio = worst_ratio(c.sum(0), want, S)
        print(f"scene {name}: unstable share {unstable.mean():.4f}, closed form vs autograd worst err/S = {ratio:.3e}")
        assert ratio <= 1e-5, (name, ratio)
        assert np.all(want[STRUCTURAL_ZEROS] == 0) and np.all(c[:, STRUCTURAL_ZEROS] == 0)
        live = [k for k in range(32) if k not in STRUCTURAL_ZEROS]
        assert np.all(S[live] > 0)
        # the J^T dM2 term is visible at the device's bar: without it the sum leaves 1e-4 S_k on some entry
        no_jt = scene_contributions(sc, o, g2, gc, with_jt=False).sum(0)
        assert worst_ratio(no_jt, want, S) > 1e-4, name
    sc, o, _, _ = case("C")
    radii = o.get("radii")
    cl = clamped_mask(sc, radii)
    assert cl.sum() >= 1, "scene C must bin a Gaussian with a clamped coordinate"
    g2, gc, _ = oracle_inputs("C", False)
    c = scene_contributions(sc, o, g2, gc)
    share = (np.abs(c[cl]).sum(0)[:16] / np.maximum(np.abs(c).sum(0)[:16], 1e-300)).max()
    print(f"scene C: {int((radii > 0).sum())} binned, {int(cl.sum())} clamped, carrying up to {share:.3f} of a view entry's absolute sum")
    assert share > 0.01


def test_depth_term_matches_the_three_render_colour_trick():
    sc, o, unstable, _ = case("G")
    g2, gc, dz = oracle_inputs("G", True)
    assert np.abs(dz).max() > 0
    c = scene_contributions(sc, o, g2, gc, dz=dz)
    S = np.abs(c).sum(0)
    truth = autograd_truth("G", True)
    want = truth["colour"] + truth["maps"]
    ratio = worst_ratio(c.sum(0), want, S)
    print(f"scene G, colour + depth + alpha: closed form vs autograd worst err/S = {ratio:.3e}")
    assert ratio <= 1e-5, ratio
    # the dz term is visible at the device's bar
    no_dz = scene_contributions(sc, o, g2, gc).sum(0)
    assert worst_ratio(no_dz, want, S) > 1e-4


def _header_params():
    text = open(os.path.join(ROOT, "include", "segs_raster.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = {}
    for m in re.finditer(r"\b(segs_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", text):
        out[m.group(1)] = [" ".join(p.split()) for p in m.group(2).split(",")]
    return out


def test_camera_entry_points_are_exported_and_bound_with_the_header_signatures():
    import ctypes as C
    from segs_slam_amd import _capi
    _capi.build()
    lib = _capi.lib()
    params = _header_params()
    for base in ("segs_rasterize_backward", "segs_rasterize_backward_resident"):
        twin, cam = base + "_depth", base + "_camera"
        assert hasattr(lib, cam), cam
        p_twin, p_cam = params[twin], params[cam]
        at = p_twin.index("void* stream")
        assert len(p_cam) == len(p_twin) + 1 and p_cam[at].startswith("const segs_camera_grads*"), (cam, p_cam[at])
        assert [p.split()[-1] for p in p_cam[:at] + p_cam[at + 1:]] == [p.split()[-1] for p in p_twin], cam
        res, args = _capi.SYMBOLS[cam]
        assert args[:at] + args[at + 1:] == _capi.SYMBOLS[twin][1] and args[at] == C.c_void_p and res == _capi.SYMBOLS[twin][0]
    base, cam = "segs_debug_preprocess_backward", "segs_debug_preprocess_backward_camera"
    assert hasattr(lib, cam)
    p_base, p_cam = params[base], params[cam]
    assert p_cam[:-3] == p_base[:-1] and p_cam[-3] == "const float* dL_dz" and p_cam[-2].startswith("const segs_camera_grads*")
    assert p_cam[-1] == "void* stream"
    res, args = _capi.SYMBOLS[cam]
    assert args == _capi.SYMBOLS[base][1][:-1] + [C.c_void_p] * 3 and res == C.c_int
    assert params["segs_camera_grad_temp_bytes"] == ["int rows"]
    assert _capi.SYMBOLS["segs_camera_grad_temp_bytes"] == (C.c_size_t, [C.c_int])
    assert [f for f, _ in _capi.CameraGrads._fields_] == ["dL_dviewmatrix", "dL_dprojmatrix", "temp"]
    assert C.sizeof(_capi.CameraGrads) == 3 * C.sizeof(C.c_void_p) and _capi.CameraGrads().temp is None
    # one 24-float row per 256-Gaussian workgroup, and room to align the base
    prev = 0
    for rows in (0, 1, 256, 257, 3000, 3_000_000):
        b = lib.segs_camera_grad_temp_bytes(rows)
        assert b >= (rows + 255) // 256 * 24 * 4 + 16 and b >= prev
        prev = b


def test_camera_paths_refuse_cpu_tensors_and_the_engine_allocates_the_matrices():
    import pytest
    from segs_slam_amd.gaussian_rasterizer import (GaussianRasterizationSettings, GaussianRasterizer, rasterizeGaussiansWithCameraGrad)
    e = torch.empty(0)
    rs = GaussianRasterizationSettings(16, 16, 1.0, 1.0, torch.zeros(3), 1.0, torch.eye(4), torch.eye(4), 0, torch.zeros(3), False)
    V, PV = torch.eye(4, requires_grad=True), torch.eye(4, requires_grad=True)
    with pytest.raises(RuntimeError, match="GPU"):
        rasterizeGaussiansWithCameraGrad(torch.zeros(4, 3), torch.zeros(4, 3), torch.zeros(4, 3), torch.zeros(4, 1), torch.zeros(4, 3),
                                         torch.zeros(4, 4), e, V, PV, rs)
    with pytest.raises(RuntimeError, match="GPU"):
        GaussianRasterizer(rs).forward_with_camera_grad(torch.zeros(4, 3), torch.zeros(4, 3), torch.zeros(4, 1), True, True, False,
                                                        torch.zeros(4, 3), scales=torch.zeros(4, 3), rotations=torch.zeros(4, 4),
                                                        viewmatrix=V, projmatrix=PV)
    from segs_slam_amd.raster_engine import RasterEngine
    eng = RasterEngine(4, 16, 16, "cpu", camera_grad=True)
    assert eng.camera_grad and eng.dL_dviewmatrix.shape == (4, 4) and eng.dL_dprojmatrix.shape == (4, 4)
    plain = RasterEngine(4, 16, 16, "cpu")
    assert plain.dL_dviewmatrix is None and plain.dL_dprojmatrix is None and not plain.camera_grad
