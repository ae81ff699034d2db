"""python -m nlt_amd.data_gen.capture_main: a mesh in, a whole capture out -- every `trainvali_*` sample of cameras x lights with
its render (data_gen/shade.py: direct lighting by a point light, or with --bounces / --light_samples / --light_size one diffuse
bounce and a spherical light), a few `test_*` samples at held-out rig positions (these carry rgb_camspc too: the
truth can be rendered), the neighbour tables, the diffuse bases and the index `datasets.nlt.load_store` reads.  No Blender.

    python -m nlt_amd.data_gen.capture_main --mesh bunny.ply --uv_unwrap unwrap.pickle --outroot out/bunny --n_cams 8 --n_lights 12 \\
        --n_test 2 --imh 512 --uvs 1024 --spp 16 [--bounces 8 --light_samples 4 --light_size 0.1]

--uv_unwrap smart [--angle_limit 89 --area_weight 1 --margin 0.002] unwraps the mesh here (data_gen/unwrap.py), writes the
table to <outroot>.uv.pickle and records the unwrap in <outroot>.capture.json.
"""
import math
from argparse import ArgumentParser
from glob import glob
from os.path import join

import numpy as np

from . import get_neighbors as _nn
from . import postproc
from .mesh import Mesh, dense_unwrap
from .render import write_sample
from .rig import light_stage
from .shade import Material, render_view, spp_side
from .unwrap import add_unwrap_flags, check_unwrap_flags, load_or_unwrap, write_unwrap
from .util import dump_json, load_json


def parse_args(argv=None):
    p = ArgumentParser(description=__doc__.split('\n')[0])
    p.add_argument('--mesh', required=True, help="the object's mesh, .ply or .obj, in world coordinates")
    p.add_argument('--uv_unwrap', required=True, help="the cached .pickle of data_gen/uv_unwrap.py, an .obj whose `vt` are the unwrap, or `smart`: "
                   "unwrap the mesh here")
    add_unwrap_flags(p)
    p.add_argument('--outroot', required=True, help="the capture's directory; the index goes to <outroot>.json")
    p.add_argument('--n_cams', type=int, default=8)
    p.add_argument('--n_lights', type=int, default=8)
    p.add_argument('--n_test', type=int, default=1, help="test_* samples at held-out rig positions")
    p.add_argument('--imh', type=int, default=512, help="image height (the width follows the camera's sensor)")
    p.add_argument('--uvs', type=int, default=1024, help="size of the square texture map")
    p.add_argument('--spp', type=int, default=16, help="samples per pixel, a perfect square from 1 to 64")
    p.add_argument('--radius', type=float, default=None, help="rig radius (default: 4.5 x the mesh box's half diagonal)")
    p.add_argument('--hemisphere', action='store_true', help="cameras and lights on the upper half only")
    p.add_argument('--cams_dir', default=None, help="a directory of cam .json files instead of generated cameras")
    p.add_argument('--lights_dir', default=None, help="a directory of light .json files instead of generated lights")
    p.add_argument('--kd', default='0.8,0.8,0.8', help="diffuse colour r,g,b")
    p.add_argument('--ks', type=float, default=0.04)
    p.add_argument('--roughness', type=float, default=0.5)
    p.add_argument('--flat', action='store_true', help="shade on the geometric normal, not on vertex normals")
    p.add_argument('--intensity', type=float, default=1.0)
    p.add_argument('--exposure', type=float, default=None, help="default: `default_exposure`")
    p.add_argument('--bounces', type=int, default=0, help="bounce rays per sample (one diffuse bounce each), 0 to 64; 0: direct light only")
    p.add_argument('--light_samples', type=int, default=1, help="points of the light's sphere per sample, 1 to 64")
    p.add_argument('--light_size', type=float, default=None, help="radius of the lights' sphere, written to the light JSONs as `size` "
                   "(default: the JSONs' own size, used only with --bounces or --light_samples)")
    p.add_argument('--device', default='cuda')
    args = p.parse_args(argv)
    args.kd = tuple(float(x) for x in args.kd.split(','))
    if len(args.kd) != 3:
        p.error("--kd takes r,g,b")
    if not 0 <= args.bounces <= 64 or not 1 <= args.light_samples <= 64:
        p.error("--bounces takes 0 to 64, --light_samples 1 to 64")
    if args.light_size is not None and not (args.light_size >= 0.0 and math.isfinite(args.light_size)):
        p.error("--light_size takes a finite radius >= 0")
    check_unwrap_flags(p, args)
    try:
        spp_side(args.spp)
    except ValueError as e:
        p.error(str(e))
    return args


def default_exposure(light_distance, intensity=1.0):
    """One number for a whole capture: a white Lambert surface (kd = 1) facing a light `light_distance` away has linear radiance
    intensity / (pi * distance^2); the exposure maps it to 0.8.  A rule of the direct light alone: the bounce light and the
    light's size of a global render (--bounces, --light_samples, --light_size) do not enter it."""
    return 0.8 * math.pi * float(light_distance) ** 2 / float(intensity)


def mesh_box(mesh):
    """(centre, half diagonal) of the box around the mesh's finite triangle vertices."""
    v = mesh.tri_verts.reshape(-1, 3)
    v = v[np.isfinite(v).all(1)]
    lo, hi = v.min(0), v.max(0)
    return (lo + hi) / 2, float(np.linalg.norm(hi - lo)) / 2


def neighbor_tables(cams, lights, test_cams, test_lights, device='cuda'):
    """data_gen/get_neighbors.py: every camera / light, held-out ones included, against the physical ones."""
    return (_nn.get_neighbors(list(cams) + list(test_cams), list(cams), device=device),
            _nn.get_neighbors(list(lights) + list(test_lights), list(lights), device=device))


def write_capture(mesh, unwrap, outroot, cams, lights, test_pairs=(), imh=512, uvs=1024, spp=16, material=None, exposure=None,
                  intensity=1.0, rig=None, workers=None, bounces=0, light_samples=1, light_size=None, unwrap_record=None):
    """Writes `trainvali_%09d_{cam}_{light}` for the full product cams x lights and `test_%09d_{cam}_{light}` for every
    (cam, light) of test_pairs, then `postproc.postprocess` and `<outroot>.capture.json` (exposure, intensity, material, rig)
    beside the index.  unwrap: the {face: rows} table or its dense form.  exposure = None: `default_exposure` at the mean distance
    of the lights from the mesh box's centre.  bounces, light_samples, light_size: `shade.render_view`'s (the defaults are its
    direct-lighting render) and recorded in capture.json.  unwrap_record: `Unwrap.record()` when the unwrap was computed for this
    capture; capture.json then carries it as `unwrap` (else it has no such entry).  Returns (the index `postprocess` wrote, the capture.json dict)."""
    material = material or Material()
    if isinstance(unwrap, dict) and 'uv' not in unwrap:
        unwrap = dense_unwrap(unwrap)
    if len({c['name'] for c in cams}) != len(cams) or len({l['name'] for l in lights}) != len(lights):
        raise ValueError("camera and light names must be unique")
    centre, _ = mesh_box(mesh)
    if exposure is None:
        exposure = default_exposure(np.mean([np.linalg.norm(np.asarray(l['position']) - centre) for l in lights]), intensity)
    test_pairs = list(test_pairs)
    nn = neighbor_tables(cams, lights, [c for c, _ in test_pairs], [l for _, l in test_pairs], device=mesh.device)
    n = 0
    for cam in cams:
        for light in lights:
            sample = render_view(mesh, unwrap, cam, light, imh, uvs, spp, material, exposure, intensity, bounces, light_samples, light_size)
            write_sample(join(outroot, 'trainvali_%09d_%s_%s' % (n, cam['name'], light['name'])), sample, cam, light, nn, workers=workers)
            n += 1
    for t, (cam, light) in enumerate(test_pairs):
        sample = render_view(mesh, unwrap, cam, light, imh, uvs, spp, material, exposure, intensity, bounces, light_samples, light_size)
        write_sample(join(outroot, 'test_%09d_%s_%s' % (t, cam['name'], light['name'])), sample, cam, light, nn, workers=workers)
    index = postproc.postprocess(outroot, device=mesh.device, workers=workers)
    info = dict(exposure=float(exposure), intensity=float(intensity), spp=int(spp), imh=int(imh), uvs=int(uvs), material=material.to_json(),
                rig=rig, cams=[c['name'] for c in cams], lights=[l['name'] for l in lights],
                test=[[c['name'], l['name']] for c, l in test_pairs], bounces=int(bounces), light_samples=int(light_samples),
                light_size=None if light_size is None else float(light_size))
    if unwrap_record is not None:
        info['unwrap'] = unwrap_record
    dump_json(info, outroot.rstrip('/') + '.capture.json')
    return index, info


def _load_dir(d):
    objs = [load_json(f) for f in sorted(glob(join(d, '*.json')))]
    if not objs:
        raise FileNotFoundError("no .json file in %s" % d)
    return objs


def build_rig(args, centre, half_diagonal):
    """(cams, lights, test_pairs, the rig's record for capture.json) from the arguments."""
    radius = args.radius if args.radius is not None else 4.5 * half_diagonal
    rig = dict(radius=float(radius), target=[float(x) for x in centre], hemisphere=bool(args.hemisphere))
    cams, lights = light_stage(args.n_cams, args.n_lights, radius, centre, hemisphere=args.hemisphere)
    if args.cams_dir:
        cams, rig['cams_dir'] = _load_dir(args.cams_dir), args.cams_dir
    if args.lights_dir:
        lights, rig['lights_dir'] = _load_dir(args.lights_dir), args.lights_dir
    test_cams, test_lights = light_stage(args.n_test, args.n_test, radius, centre, hemisphere=args.hemisphere, cam_prefix='VC',
                                         light_prefix='VL', phase=1.0) if args.n_test > 0 else ([], [])
    if args.light_size is not None:                      # the sphere's radius, where Blender keeps it: in every light's JSON
        lights = [dict(l, size=float(args.light_size)) for l in lights]
        test_lights = [dict(l, size=float(args.light_size)) for l in test_lights]
    return cams, lights, list(zip(test_cams, test_lights)), rig


def main(argv=None):
    args = parse_args(argv)
    mesh = Mesh.load(args.mesh, device=args.device)
    unwrap, computed = load_or_unwrap(args, mesh)
    if computed is not None:
        write_unwrap(args.outroot.rstrip('/') + '.uv.pickle', computed.table())
    cams, lights, test_pairs, rig = build_rig(args, *mesh_box(mesh))
    material = Material(kd=args.kd, ks=args.ks, roughness=args.roughness, smooth=not args.flat)
    return write_capture(mesh, unwrap, args.outroot, cams, lights, test_pairs, args.imh, args.uvs, args.spp, material, args.exposure,
                         args.intensity, rig, bounces=args.bounces, light_samples=args.light_samples, light_size=args.light_size,
                         unwrap_record=None if computed is None else computed.record())


if __name__ == '__main__':
    main()
