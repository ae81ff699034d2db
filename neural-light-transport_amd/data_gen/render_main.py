"""python -m nlt_amd.data_gen.render_main: data_gen/render.py:main without the two Cycles renders -- a mesh file, a cam.json and a
light.json in, one `test_*` sample directory out (no rgb_camspc: ground truth needs a renderer; alpha is the binary hit mask).

    python -m nlt_amd.data_gen.render_main --mesh bunny.ply --uv_unwrap unwrap.pickle --cam_json P28.json --light_json L330.json \\
        --cam_nn_json cam_nn.json --light_nn_json light_nn.json --imh 512 --uvs 1024 --outdir out/test_000000000_P28_L330
"""
from argparse import ArgumentParser

from .mesh import Mesh, dense_unwrap, render_geometry, unwrap_from_obj
from .render import write_sample


def parse_args(argv=None):
    p = ArgumentParser(description=__doc__.split('\n')[0])
    p.add_argument('--mesh', required=True, help="the object's mesh, .ply or .obj, in world coordinates")
    p.add_argument('--uv_unwrap', required=True, help="the cached .pickle of data_gen/uv_unwrap.py, or an .obj whose `vt` are the unwrap")
    p.add_argument('--cam_json', required=True)
    p.add_argument('--light_json', required=True)
    p.add_argument('--cam_nn_json', required=True, help="camera -> nearest neighbour")
    p.add_argument('--light_nn_json', required=True, help="light -> nearest neighbour")
    p.add_argument('--imh', type=int, default=256, help="image height (the width follows the camera's sensor)")
    p.add_argument('--uvs', type=int, default=256, help="size of the square texture map")
    p.add_argument('--outdir', required=True)
    p.add_argument('--debug', action='store_true', help="also write the three *_camspc_repro.png")
    p.add_argument('--device', default='cuda')
    return p.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    mesh = Mesh.load(args.mesh, device=args.device)
    if args.uv_unwrap.lower().endswith('.obj'):
        unwrap = unwrap_from_obj(Mesh.load(args.uv_unwrap, device=None))
    else:
        import pickle
        with open(args.uv_unwrap, 'rb') as h:
            unwrap = pickle.load(h)
    sample = render_geometry(mesh, dense_unwrap(unwrap), args.cam_json, args.light_json, args.imh, args.uvs)
    return write_sample(args.outdir, sample, args.cam_json, args.light_json, (args.cam_nn_json, args.light_nn_json), debug=args.debug)


if __name__ == '__main__':
    main()
