"""Direct-lighting renders of a mesh without Blender: nlt_render_direct (csrc/raycast.hip) for the colours and the anti-aliased
coverage, data_gen/mesh.py's two ray casts for the geometry, data_gen/render.py's `render_sample` for every buffer of a
`trainvali_*` sample.  One point light, Lambert + GGX, hard shadows, box-filtered supersampling: not Cycles (DESIGN.md section 8
lists what stays out of scope).  Host code here is the material's per-corner arrays and the plumbing around the launches."""
import math

import numpy as np
import torch

from .. import _capi as C
from .mesh import camera_matrix, corner_normals, render_geometry
from .render import _params


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


def to_uint8(x):
    """The writer's rule for a [0,1] image (util/vis.py:write_arr): clip, times 255, truncate."""
    return (x.clamp(0.0, 1.0) * 255.0).to(torch.uint8)


def render_view(mesh, cached_unwrap, cam, light, imh, uvs, spp, material, exposure, intensity=1.0):
    """A complete `trainvali_*` sample for `write_sample`: rgb_camspc = sRGB(clip01(exposure * rgb_linear)) through
    nlt_relight_finish, alpha = the coverage, both as uint8 by `to_uint8`; the geometry buffers from `render_geometry` (`backproject`
    + `shadow` at the pixel centres, then `render_sample`, which zeroes uv2cam where alpha < 255: partially covered edge pixels
    drop out as in a Blender capture)."""
    cam, light = _params(cam), _params(light)
    rgb_linear, coverage = render_direct(mesh, cam, light, imh, spp, material, intensity)
    _, _, (imh, imw) = camera_matrix(cam, imh)
    srgb = C.relight_finish(rgb_linear.view(1, imh * imw, 3), exposure, True)
    return render_geometry(mesh, cached_unwrap, cam, light, imh, uvs, rgb_camspc=to_uint8(srgb).view(imh, imw, 3),
                           alpha=to_uint8(coverage).view(imh, imw))
