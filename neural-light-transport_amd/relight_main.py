"""`python -m nlt_amd.relight_main --ckpt <prefix> --cam C27 --envmap probe.hdr [--turns N]`: one camera's view relit under
an environment map, optionally as a turn of the probe about +z (N frames, 2 pi / N apart).

The config beside the checkpoint, the restored net and the aggregated observation features are `nlt_test_main`'s; the view's
per-light renders, the probe's per-light weights and their combination are `relight`'s.  Written under
`<outroot>/<xname>/vis_relight/ckpt-N/<cam>/<probe>/`: `frame_%03d.png` (`util.vis.write_arr` of `relight()`'s image),
`linear.npy` ([turns,imh,imw,3] float32, before exposure and encoding) and, with more than one frame, `turn.apng`."""
import argparse
import logging
import math
import os
from os.path import basename, join, splitext

import numpy as np

from . import nlt_test, nlt_test_main, relight as R
from .util import vis as V

logger = logging.getLogger('relight')


def run(ckpt, cam, envmap, turns=1, exposure=1.0, n_obs_batches=1, center=(0.0, 0.0, 0.0), fps=24, store=None, device='cuda',
        config=None, seed=None):
    """Returns (outdir, result of `relight.relight`).  store: the resident capture (None: `load_store(data_root)`); config: a
    parsed config in place of the one beside the checkpoint; seed: of the shuffle that picks the observation batches."""
    from . import trainvali
    from .datasets import get_dataset_class
    from .datasets.nlt import load_store
    config_ini = nlt_test_main.get_config_ini(ckpt)
    if config is None:
        config = trainvali.read_config(config_ini)
    data_root = config.get('DEFAULT', 'data_root')
    if store is None:
        store = load_store(data_root, device)
    model = nlt_test_main.restore_model(config, ckpt, device)
    feat_agg = nlt_test.extract_feat(model, nlt_test_main.make_datapipe('train', config, store, device, seed), n_obs_batches)
    dataset = get_dataset_class(config.get('DEFAULT', 'dataset'))(
        config, 'train', store=store, k=config.getint('DEFAULT', 'k', fallback=1), device=device)

    lights = R.load_lights(data_root)
    samples = R.view_samples(store, cam)
    dirs = R.light_directions([lights[name] for _, name in samples], center)
    turns = max(1, int(turns))
    weights = R.envmap_weights(R.read_envmap(envmap), dirs, rotations=[2.0 * math.pi * t / turns for t in range(turns)], device=device)
    out = R.relight(model, dataset, cam, weights, feat_agg=feat_agg, exposure=exposure)

    name = basename(ckpt)
    outdir = join(config_ini[:-4], 'vis_relight', name[:-3] if name.endswith('.pt') else name, cam, splitext(basename(envmap))[0])
    os.makedirs(outdir, exist_ok=True)
    image = V.to_numpy(out['image'])
    frames = [V.write_arr(image[t], join(outdir, 'frame_%03d.png' % t)) for t in range(turns)]
    np.save(join(outdir, 'linear.npy'), V.to_numpy(out['linear']))
    if turns > 1:
        V.make_apng(frames, duration=1.0 / fps, outpath=join(outdir, 'turn.apng'))
    logger.info("%d relit frame(s) of %s (%d lights) at\n\t%s", turns, cam, len(samples), outdir)
    return outdir, out


def parse_args(argv=None):
    p = argparse.ArgumentParser(prog='nlt_amd.relight_main', description="Relight one camera's view under an environment map.")
    p.add_argument('--ckpt', required=True, help="path to checkpoint (prefix `ckpt-N`, or a native `ckpt-N.pt`)")
    p.add_argument('--cam', required=True, help="camera name, as in the sample ids (trainvali_*_<cam>_<light>)")
    p.add_argument('--envmap', required=True, help="lat-long probe, z-up: .npy [He,We,3] or Radiance .hdr")
    p.add_argument('--turns', type=int, default=1, help="frames of one full turn of the probe about +z")
    p.add_argument('--exposure', type=float, default=1.0, help="factor on the linear result before clipping / encoding")
    p.add_argument('--n_obs_batches', type=int, default=1, help="number of observation batches used for the observation path")
    p.add_argument('--center', default='0,0,0', help="x,y,z the light directions are taken from")
    p.add_argument('--fps', type=int, default=24, help="frames per second of the animated PNG")
    return p.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    logging.basicConfig(level=logging.INFO)
    center = tuple(float(x) for x in args.center.split(','))
    if len(center) != 3:
        raise ValueError("--center takes x,y,z, got %r" % args.center)
    return run(args.ckpt, args.cam, args.envmap, turns=args.turns, exposure=args.exposure, n_obs_batches=args.n_obs_batches,
               center=center, fps=args.fps)


if __name__ == '__main__':             # python -m nlt_amd.relight_main: hand over to the package's own copy of this module
    from .relight_main import main as _main
    _main()
