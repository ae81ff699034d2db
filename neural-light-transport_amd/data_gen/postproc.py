"""data_gen/postproc.py on HIP: UV albedo, diffuse bases and their camera-space remap (:53-82), and the data index (:89-122)."""
from glob import glob
from os.path import basename, exists, isdir, join, relpath

import numpy as np
import torch

from .. import _capi as C
from .util import dump_json, encode_pool, remap


def compute_albedo(rgb_uv_frames):
    """postproc.py:53-64: rgb_uv_frames [F,H,W,3] uint8 (every trainvali rgb.png) -> float64 [H,W,3]."""
    return C.albedo(rgb_uv_frames.contiguous())


def compute_diffuse_bases(albedo, lvis_frames, uv2cam=None):
    """postproc.py:66-82: diffuse.png = albedo * lvis (uint8, truncating) for every frame; with
    uv2cam [F,imh,imw,2] (fp16 as stored) also diffuse_camspc.png.  Returns (diffuse, diffuse_camspc)."""
    diffuse = C.diffuse_base(albedo, lvis_frames.contiguous())
    cam = None
    if uv2cam is not None:
        cam = [remap(diffuse[f], uv2cam[f]) for f in range(diffuse.shape[0])]
    return diffuse, cam


def _sample_dirs(data_root, pattern='*'):
    """xm.os.sortglob(data_root, pattern), sub-directories only."""
    return [d for d in sorted(glob(join(data_root, pattern))) if isdir(d)]


def _stack(arrays, what):
    if len({a.shape for a in arrays}) != 1:
        raise NotImplementedError("'%s' comes in several shapes: %s" % (what, sorted({a.shape for a in arrays})))
    return np.stack(arrays)


def postprocess(data_root, out_json=None, chunk=64, device='cuda', workers=None):
    """postproc.py:main.  The albedo is the sum of every `trainvali_*/rgb.png` in sorted directory order (a float64 sum
    depends on its order; nlt_albedo adds in frame order) over the whole capture; then diffuse.png and diffuse_camspc.png of
    every sample directory, `chunk` frames per nlt_diffuse_bases launch -- the albedo being complete before the first chunk,
    the chunk size changes no byte -- and the index (`gen_file_list`).  PNG decode / encode runs on a thread pool of
    min(16, number of files) threads; `pool.map` keeps the directory order of everything that is summed or stacked."""
    from ..datasets.nlt import read_png
    from ..util.vis import write_img
    dev = torch.device(device)
    rgb_paths = [join(d, 'rgb.png') for d in _sample_dirs(data_root, 'trainvali_*')]
    if not rgb_paths:
        raise FileNotFoundError("no trainvali_* sample under %s: nothing to average the albedo from" % data_root)
    with encode_pool(len(rgb_paths), workers) as pool:
        frames = list(pool.map(read_png, rgb_paths))                # in directory order
    albedo = compute_albedo(torch.from_numpy(_stack(frames, 'rgb')).to(dev))
    del frames
    dirs = _sample_dirs(data_root)
    chunk = max(1, int(chunk))
    for at in range(0, len(dirs), chunk):
        part = dirs[at:at + chunk]
        with encode_pool(2 * len(part), workers) as pool:
            lvis = list(pool.map(read_png, [join(d, 'lvis.png') for d in part]))
            uv2cam = list(pool.map(np.load, [join(d, 'uv2cam.npy') for d in part]))
        diffuse, cam = C.diffuse_bases(albedo, torch.from_numpy(_stack(lvis, 'lvis')).to(dev),
                                       torch.from_numpy(_stack(uv2cam, 'uv2cam')).to(dev))
        diffuse, cam = diffuse.cpu().numpy(), cam.cpu().numpy()
        jobs = [(diffuse[i], join(d, 'diffuse.png')) for i, d in enumerate(part)] + \
               [(cam[i], join(d, 'diffuse_camspc.png')) for i, d in enumerate(part)]
        with encode_pool(len(jobs), workers) as pool:
            list(pool.map(lambda j: write_img(*j), jobs))
    return gen_file_list(data_root, out_json)


def gen_file_list(data_root, out_json=None):
    """postproc.py:89-122: the `<data_root>.json` index nlt/datasets/nlt.py (here datasets/nlt.py:load_store) reads -- per
    sample directory, in sorted order, the paths of its files relative to data_root and whether all of them exist."""
    if out_json is None:
        out_json = data_root.rstrip('/') + '.json'
    filelist = {}
    for config_dir in _sample_dirs(data_root):
        id_ = basename(config_dir)
        entry = {'cam': 'cam.json', 'cvis': 'cvis.png', 'diffuse': 'diffuse.png', 'light': 'light.json', 'lvis': 'lvis.png',
                 'nn': 'nn.json', 'uv2cam': 'uv2cam.npy'}
        if id_.startswith('trainvali_'):
            entry.update(alpha='alpha.png', rgb='rgb.png', rgb_camspc='rgb_camspc.png')
        paths = {k: join(config_dir, v) for k, v in entry.items()}
        filelist[id_] = {k: relpath(v, data_root) for k, v in paths.items()}
        filelist[id_]['complete'] = all(exists(v) for v in paths.values())
    dump_json(filelist, out_json)
    return filelist
