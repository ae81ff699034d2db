"""python -m nlt_amd.data_gen.render_main: data_gen/render.py:main without the two Cycles renders -- a mesh file, a cam.json and a
light.json in, one `test_*` sample directory out (no rgb_camspc: ground truth needs a renderer; alpha is the binary hit mask).

    python -m nlt_amd.data_gen.render_main --mesh bunny.ply --uv_unwrap unwrap.pickle --cam_json P28.json --light_json L330.json \\
        --cam_nn_json cam_nn.json --light_nn_json light_nn.json --imh 512 --uvs 1024 --outdir out/test_000000000_P28_L330

--uv_unwrap smart [--angle_limit 89 --area_weight 1 --margin 0.002] unwraps the mesh here (data_gen/unwrap.py).
"""
from argparse import ArgumentParser

from .mesh import Mesh, dense_unwrap, render_geometry
from .render import write_sample
from .unwrap import add_unwrap_flags, check_unwrap_flags, load_or_unwrap


def parse_args(argv=None):
    p = ArgumentParser(description=__doc__.split('\n')[0])
    p.add_argument('--mesh', required=True, help="the object's mesh, .ply or .obj, in world coordinates")
    p.add_argument('--uv_unwrap', required=True, help="the cached .pickle of data_gen/uv_unwrap.py, an .obj whose `vt` are the unwrap, or `smart`: "
                   "unwrap the mesh here")
    add_unwrap_flags(p)
    p.add_argument('--cam_json', required=True)
    p.add_argument('--light_json', required=True)
    p.add_argument('--cam_nn_json', required=True, help="camera -> nearest neighbour")
    p.add_argument('--light_nn_json', required=True, help="light -> nearest neighbour")
    p.add_argument('--imh', type=int, default=256, help="image height (the width follows the camera's sensor)")
    p.add_argument('--uvs', type=int, default=256, help="size of the square texture map")
    p.add_argument('--outdir', required=True)
    p.add_argument('--debug', action='store_true', help="also write the three *_camspc_repro.png")
    p.add_argument('--device', default='cuda')
    args = p.parse_args(argv)
    check_unwrap_flags(p, args)
    return args


def main(argv=None):
    args = parse_args(argv)
    mesh = Mesh.load(args.mesh, device=args.device)
    unwrap, _ = load_or_unwrap(args, mesh)
    sample = render_geometry(mesh, unwrap if 'uv' in unwrap else dense_unwrap(unwrap), args.cam_json, args.light_json, args.imh, args.uvs)
    return write_sample(args.outdir, sample, args.cam_json, args.light_json, (args.cam_nn_json, args.light_nn_json), debug=args.debug)


if __name__ == '__main__':
    main()
