"""data_gen/util.py on HIP (remap) and on the host (JSON, names)."""
import json
from os import makedirs
from os.path import basename, dirname, exists

import torch

from .. import _capi as C


def remap(src, mapping, force_kbg=True):
    """data_gen/util.py:45-58: cv2.remap(src, mapping*w, mapping*h, INTER_LINEAR) with the top-left
    source texel (where the background samples from) forced black.
    src [h,w(,c)] uint8 or float32; mapping [H,W,>=2] in [0,1], x first (float64/32/16)."""
    return C.remap_bilinear(src.contiguous(), mapping.contiguous(), force_kbg)


def add_b_ch(img_rg):
    """data_gen/util.py:61-64."""
    assert img_rg.dim() == 3 and img_rg.shape[2] == 2, "Input should be HxWx2"
    return torch.cat((img_rg, torch.zeros_like(img_rg[:, :, :1])), 2)


def to_float16(data):
    """data_gen/util.py:67-70 save_float16_npy, minus the file write."""
    return data.to(torch.float16)


def load_json(json_path):
    """data_gen/util.py:23-26."""
    with open(json_path, 'r') as h:
        return json.load(h)


def dump_json(data, path):
    """data_gen/util.py:29-37: pretty dump (indent 4, sorted keys); the directory is made if missing."""
    dir_ = dirname(path)
    if dir_ and not exists(dir_):
        makedirs(dir_, exist_ok=True)
    with open(path, 'w') as h:
        json.dump(data, h, indent=4, sort_keys=True)


def name_from_json_path(json_path):
    """data_gen/util.py:73-74."""
    return basename(json_path)[:-len('.json')]


def encode_pool(n_files, workers=None):
    """The thread pool PNG encode / decode runs on (zlib releases the GIL): min(16, number of files) threads -- never sized
    by os.cpu_count(), which shows a shared host's CPUs, not this process's."""
    from concurrent.futures import ThreadPoolExecutor
    return ThreadPoolExecutor(max_workers=max(1, min(16, n_files) if workers is None else int(workers)))
