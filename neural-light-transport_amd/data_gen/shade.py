"""Renders of a mesh without Blender: nlt_render_direct (csrc/raycast.hip) for the colours and the anti-aliased coverage,
data_gen/mesh.py's two ray casts for the geometry, data_gen/render.py's `render_sample` for every buffer of a `trainvali_*`
sample.  One point light, Lambert + GGX, hard shadows, box-filtered supersampling; on request (`render_global`,
nlt_render_global) the light is a sphere sampled at several points and every sample gathers one diffuse bounce.  Not Cycles
(DESIGN.md section 8 lists what stays out of scope).  Host code here is the material's per-corner arrays, the two sample tables
of the global renders and the plumbing around the launches."""
import functools
import math

import numpy as np
import torch

from .. import _capi as C
from .mesh import camera_matrix, corner_normals, render_geometry
from .render import _params
from .rig import GOLDEN_ANGLE, fibonacci_sphere


class Material:
    """kd: one diffuse colour (r, g, b), or vertex_rgb [V,3]: a colour per mesh vertex, blended over each triangle.  ks: the
    specular reflectance at normal incidence (Schlick's F0), roughness: the GGX alpha.  smooth: shade on area-weighted vertex
    normals (`mesh.corner_normals`) instead of the geometric normal."""

    def __init__(self, kd=(0.8, 0.8, 0.8), vertex_rgb=None, ks=0.04, roughness=0.5, smooth=True):
        self.kd = tuple(float(x) for x in kd)
        if len(self.kd) != 3:
            raise ValueError("kd must be (r, g, b), got %r" % (kd,))
        self.vertex_rgb = None if vertex_rgb is None else np.ascontiguousarray(vertex_rgb, np.float64).reshape(-1, 3)
        self.ks, self.roughness, self.smooth = float(ks), float(roughness), bool(smooth)
        self._for = None

    def arrays(self, mesh):
        """(tri_normals, tri_rgb): float64 [T,3,3] tensors on the mesh's device, or None; built once per mesh."""
        if self._for is None or self._for[0] is not mesh:
            dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(mesh.device)
            if self.vertex_rgb is not None and len(self.vertex_rgb) != len(mesh.vertices):
                raise ValueError("vertex_rgb has %d rows for %d vertices" % (len(self.vertex_rgb), len(mesh.vertices)))
            self._for = (mesh, dev(corner_normals(mesh)) if self.smooth else None,
                         None if self.vertex_rgb is None else dev(self.vertex_rgb[mesh.tris]))
        return self._for[1:]

    def to_json(self):
        return dict(kd=list(self.kd), vertex_rgb=self.vertex_rgb is not None, ks=self.ks, roughness=self.roughness, smooth=self.smooth)


def spp_side(spp):
    """Samples per pixel -> samples per pixel side: a perfect square from 1 to 64, as data_gen/render.py's --spp 64."""
    side = math.isqrt(int(spp)) if int(spp) == spp and spp > 0 else 0
    if side * side != spp or not 1 <= side <= 8:
        raise ValueError("spp must be a perfect square from 1 to 64, got %r" % (spp,))
    return side


def render_direct(mesh, cam, light, imh, spp, material, intensity=1.0):
    """-> (rgb_linear float32 [imh*imw,3], coverage float32 [imh*imw]) on the mesh's device, row-major pixels."""
    cam, light = _params(cam), _params(light)
    _, inv, (imh, imw) = camera_matrix(cam, imh)
    tri_normals, tri_rgb = material.arrays(mesh)
    return C.render_direct(*mesh.bvh, mesh.n_tris, tri_normals, tri_rgb, inv.reshape(-1), cam['position'], imh, imw, spp_side(spp),
                           light['position'], intensity, material.kd, material.ks, material.roughness)


def _deal(points, n, n_sets):
    """points [n * n_sets, c] -> [n_sets, n, c], point q to set q mod n_sets (its row q // n_sets): every set covers the domain."""
    out = np.ascontiguousarray(points.reshape(n, n_sets, points.shape[1]).transpose(1, 0, 2))
    out.setflags(write=False)
    return out


@functools.lru_cache(None)
def bounce_table(n_b, n_sets):
    """float64 [n_sets, n_b, 2]: one sunflower (Fibonacci) set of n_b * n_sets points of the unit disc -- point q at radius
    sqrt((q + 1/2) / N), azimuth q * the golden angle -- dealt round-robin.  Lifted to the hemisphere by the kernel
    (dz = sqrt(1 - dx^2 - dy^2)) they are cosine-weighted directions.  Deterministic, read-only, cached."""
    n_b, n_sets = int(n_b), int(n_sets)
    if n_b < 0 or n_sets < 1:
        raise ValueError("bounce_table: n_b >= 0 and n_sets >= 1 expected, got %d, %d" % (n_b, n_sets))
    total = n_b * n_sets
    q = np.arange(total, dtype=np.float64)
    r = np.sqrt((q + 0.5) / max(total, 1))
    phi = q * GOLDEN_ANGLE
    return _deal(np.stack((r * np.cos(phi), r * np.sin(phi)), 1), n_b, n_sets)


@functools.lru_cache(None)
def light_table(n_l, n_sets):
    """float64 [n_sets, n_l, 3]: one Fibonacci sphere (`rig.fibonacci_sphere`) of n_l * n_sets unit vectors, normalised once more,
    dealt round-robin.  Deterministic, read-only, cached."""
    n_l, n_sets = int(n_l), int(n_sets)
    if n_l < 1 or n_sets < 1:
        raise ValueError("light_table: n_l >= 1 and n_sets >= 1 expected, got %d, %d" % (n_l, n_sets))
    p = fibonacci_sphere(n_l * n_sets)
    return _deal(p / np.sqrt((p * p).sum(1))[:, None], n_l, n_sets)


@functools.lru_cache(None)
def _table_on(kind, n, n_sets, device):
    return torch.from_numpy((bounce_table if kind == 'bounce' else light_table)(n, n_sets).copy()).to(device)


def render_global(mesh, cam, light, imh, spp, material, intensity=1.0, bounces=0, light_samples=1, light_size=None):
    """nlt_render_global: `render_direct` with the light a sphere sampled at `light_samples` points per sample and `bounces`
    cosine-weighted bounce rays per sample (one diffuse bounce each).  light_size = None: the light JSON's `size` is the sphere's
    radius (Blender's meaning of the field; 0 when it has none).  Each of the spp samples of a pixel has a table set of its own.
    -> (rgb_linear float32 [imh*imw,3], coverage float32 [imh*imw], rgb_indirect float32 [imh*imw,3]): rgb_linear includes
    rgb_indirect."""
    cam, light = _params(cam), _params(light)
    _, inv, (imh, imw) = camera_matrix(cam, imh)
    tri_normals, tri_rgb = material.arrays(mesh)
    side = spp_side(spp)
    bounces, light_samples = int(bounces), int(light_samples)
    if not 0 <= bounces <= 64 or not 1 <= light_samples <= 64:
        raise ValueError("bounces from 0 to 64 and light_samples from 1 to 64 expected, got %d, %d" % (bounces, light_samples))
    radius = float(light.get('size', 0.0) if light_size is None else light_size)
    if not (radius >= 0.0 and math.isfinite(radius)):
        raise ValueError("the light's size must be finite and >= 0, got %r" % (radius,))
    dev = str(mesh.device)
    return C.render_global(*mesh.bvh, mesh.n_tris, tri_normals, tri_rgb, inv.reshape(-1), cam['position'], imh, imw, side,
                           light['position'], intensity, material.kd, material.ks, material.roughness, radius,
                           _table_on('light', light_samples, side * side, dev),
                           _table_on('bounce', bounces, side * side, dev) if bounces else None)


def to_uint8(x):
    """The writer's rule for a [0,1] image (util/vis.py:write_arr): clip, times 255, truncate."""
    return (x.clamp(0.0, 1.0) * 255.0).to(torch.uint8)


def render_view(mesh, cached_unwrap, cam, light, imh, uvs, spp, material, exposure, intensity=1.0, bounces=0, light_samples=1,
                light_size=None):
    """A complete `trainvali_*` sample for `write_sample`: rgb_camspc = sRGB(clip01(exposure * rgb_linear)) through
    nlt_relight_finish, alpha = the coverage, both as uint8 by `to_uint8`; the geometry buffers from `render_geometry` (`backproject`
    + `shadow` at the pixel centres, then `render_sample`, which zeroes uv2cam where alpha < 255: partially covered edge pixels
    drop out as in a Blender capture).  With the defaults (no bounce rays, one light sample, no light_size) the colours are
    `render_direct`'s, a point light; otherwise `render_global`'s.  The geometry buffers (lvis, the shadow mask) are those of the
    light's centre either way, as in a Blender capture with a sized light."""
    cam, light = _params(cam), _params(light)
    if bounces == 0 and light_samples == 1 and light_size is None:
        rgb_linear, coverage = render_direct(mesh, cam, light, imh, spp, material, intensity)
    else:
        rgb_linear, coverage, _ = render_global(mesh, cam, light, imh, spp, material, intensity, bounces, light_samples, light_size)
    _, _, (imh, imw) = camera_matrix(cam, imh)
    srgb = C.relight_finish(rgb_linear.view(1, imh * imw, 3), exposure, True)
    return render_geometry(mesh, cached_unwrap, cam, light, imh, uvs, rgb_camspc=to_uint8(srgb).view(imh, imw, 3),
                           alpha=to_uint8(coverage).view(imh, imw))
