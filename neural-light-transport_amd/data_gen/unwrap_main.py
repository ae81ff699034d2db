"""python -m nlt_amd.data_gen.unwrap_main: data_gen/uv_unwrap.py without Blender -- a mesh file in, the cached UV-unwrap pickle
out ({face: [[loop, vert, u, v], ...]}; the flags and their defaults are that script's, plus the packing margin).

    python -m nlt_amd.data_gen.unwrap_main --mesh bunny.ply --outpath bunny_uv.pickle [--angle_limit 89] [--area_weight 1] [--margin 0.002]
"""
from argparse import ArgumentParser

from .mesh import Mesh
from .unwrap import check_params, smart_unwrap, write_unwrap


def parse_args(argv=None):
    p = ArgumentParser(description=__doc__.split('\n')[0])
    p.add_argument('--mesh', required=True, help="the object's mesh, .ply or .obj, in world coordinates")
    p.add_argument('--outpath', required=True, help="output .pickle (the extension is added when missing)")
    p.add_argument('--angle_limit', type=float, default=89., help="angle limit; lower for more projection groups, and higher for less distortion")
    p.add_argument('--area_weight', type=float, default=1., help="area weight used to weight projection vectors; higher for fewer islands")
    p.add_argument('--margin', type=float, default=0.002, help="the gap around every island, in UV units")
    p.add_argument('--device', default='cuda')
    args = p.parse_args(argv)
    try:
        check_params(args.angle_limit, args.area_weight, args.margin, 256)
    except ValueError as e:
        p.error(str(e))
    return args


def main(argv=None):
    args = parse_args(argv)
    unwrap = smart_unwrap(Mesh.load(args.mesh, device=None), args.angle_limit, args.area_weight, args.margin, device=args.device)
    path = write_unwrap(args.outpath, unwrap.table())
    print("%s: %d projection groups, %d islands, scale %.6g" % (path, len(unwrap.vectors), len(unwrap.island_labels), unwrap.scale))
    return path, unwrap


if __name__ == '__main__':
    main()
