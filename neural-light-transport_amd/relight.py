"""Relighting a view under an environment map from its one-light-at-a-time (OLAT) renders.

The capture is a light stage: `trainvali_*_{cam}_{light}` is the full product of cameras and point lights.  A view under a
lat-long radiance probe is the linear combination of that view's per-light renders, every light weighted by the probe's
solid-angle integral over the directions nearest to it (the HDRI relighting of the paper; the reference never published the
step).  The per-light weights, the accumulation and the final encode are HIP kernels (csrc/relight.hip); the renders are
`Model.call`'s, unchanged.

Lat-long convention (ours, z-up as in the Blender scenes): pixel (i, j) of an [He, We, 3] probe looks along
    d = (sin t cos p, sin t sin p, cos t),   t = pi (i + 1/2) / He,   p = 2 pi (j + 1/2) / We - pi,
and covers the solid angle dO = sin t * (pi / He) * (2 pi / We): row 0 is +z (up), the centre column looks along +x, columns
to the right of it turn towards +y.  A rotation R turns a pixel direction d into R . d before its nearest light is looked up.

    lights = load_lights(data_root)                          # {light name: position}
    samples = view_samples(dataset.store, 'C27')             # [(id, light name)], sorted by light name
    dirs = light_directions([lights[n] for _, n in samples])
    weights = envmap_weights(read_envmap('probe.hdr'), dirs, rotations=[0.0, 0.1, 0.2])
    out = relight(model, dataset, 'C27', weights, feat_agg=feat_agg)     # {'linear', 'image'} [R,imh,imw,3]
"""
import json
import re
from os.path import exists, join

import numpy as np
import torch

from . import _capi as C


# ---------------------------------------------------------------- the capture's lights and views
def _read_index(data_root):
    status = data_root.rstrip('/') + '.json'
    if not exists(status):
        raise FileNotFoundError("Data status JSON not found at \n\t%s" % status)
    with open(status) as h:
        return json.load(h)


def _cam_light(id_):
    """'trainvali_{i:09d}_{cam}_{light}' -> (cam, light), as the hold-out rule splits it (datasets/nlt.py:_glob)."""
    parts = id_.split('_')
    return parts[-2], parts[-1]


def load_lights(data_root):
    """{light name: position (three floats)} from the `light` entry (`light.json`: `name`, `position`) of every complete
    `trainvali_*` sample in `<data_root>.json`.  Two samples that give one name different positions raise ValueError."""
    lights, first = {}, {}
    for id_, entry in sorted(_read_index(data_root).items()):
        if not id_.startswith('trainvali_') or not entry.get('complete'):
            continue
        with open(join(data_root, entry['light'])) as h:
            light = json.load(h)
        name, pos = str(light['name']), tuple(float(x) for x in light['position'])
        if len(pos) != 3:
            raise ValueError("%s: light '%s' has a position of %d numbers" % (id_, name, len(pos)))
        if name in lights and lights[name] != pos:
            raise ValueError("light '%s' has two positions: %s in %s, %s in %s" % (name, lights[name], first[name], pos, id_))
        if name not in lights:
            lights[name], first[name] = pos, id_
    return lights


def view_samples(store_or_data_root, cam):
    """[(id, light name)] of every complete `trainvali_*_{cam}_{light}` sample, sorted by light name.  Taken from the index (a
    resident store's `ids` / `complete`, or `<data_root>.json`), not from a train / vali split: the hold-out rule scatters one
    camera's lights over both.  A camera without samples raises ValueError naming the cameras there are."""
    if isinstance(store_or_data_root, str):
        index = _read_index(store_or_data_root)
        ids = [i for i in sorted(index) if index[i].get('complete')]
    else:
        store = store_or_data_root
        complete = store.get('complete')
        ids = [i for n, i in enumerate(store['ids']) if complete is None or complete[n]]
    ids = [i for i in ids if i.startswith('trainvali_')]
    found = sorted((_cam_light(i)[1], i) for i in ids if _cam_light(i)[0] == cam)
    if not found:
        raise ValueError("no complete trainvali sample of camera '%s'; cameras: %s" % (cam, ', '.join(sorted({_cam_light(i)[0] for i in ids})) or 'none'))
    names = [n for n, _ in found]
    if len(set(names)) != len(names):
        raise ValueError("camera '%s' has several samples of one light: %s" % (cam, sorted({n for n in names if names.count(n) > 1})))
    return [(i, n) for n, i in found]


def light_directions(positions, center=(0.0, 0.0, 0.0)):
    """[L,3] positions -> [L,3] float32 unit vectors from `center` towards each light (normalised in float64)."""
    p = np.asarray(positions, np.float64).reshape(-1, 3) - np.asarray(center, np.float64).reshape(1, 3)
    norm = np.sqrt((p * p).sum(1, keepdims=True))
    if not (norm > 0).all():
        raise ValueError("a light sits at the centre %s: it has no direction" % (tuple(center),))
    return (p / norm).astype(np.float32)


# ---------------------------------------------------------------- probe -> weights
def rotations_about_z(angles):
    """[R] angles (radians, counter-clockwise seen from +z) -> [R,3,3] float32 rotation matrices."""
    a = np.asarray(angles, np.float64).reshape(-1)
    rot = np.zeros((a.size, 3, 3), np.float64)
    rot[:, 0, 0], rot[:, 0, 1], rot[:, 1, 0], rot[:, 1, 1], rot[:, 2, 2] = np.cos(a), -np.sin(a), np.sin(a), np.cos(a), 1.0
    return rot.astype(np.float32)


def envmap_weights(envmap, dirs, rotations=None, normalize=True, device='cuda'):
    """[He,We,3] linear radiance (lat-long, z-up: the module's docstring), [L,3] unit light directions -> [R,L,3] float32 on
    `device`: W[r,l,c] = sum of envmap[p,c] dO(p) over the pixels p whose direction, turned by rotation r, is nearest light l
    (largest dot product, ties to the lowest l).  rotations: None (the identity, R = 1), an [R,3,3] array, or a list of angles
    about +z.  The kernel returns the raw solid-angle integrals; normalize divides them, on the host, by sum_{l,c} W[l,c] / 3
    of the identity-rotation probe -- a uniform white probe then sums to 1 over the lights."""
    t32 = lambda a: (a.detach() if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))).to(
        device=device, dtype=torch.float32).contiguous()
    identity = np.eye(3, dtype=np.float32)[None]
    if rotations is None:
        rot = identity
    else:
        rot = rotations.detach().cpu().numpy() if torch.is_tensor(rotations) else np.asarray(rotations, np.float64)
        rot = rotations_about_z(rot) if rot.ndim <= 1 else rot.astype(np.float32)
        if rot.ndim != 3 or rot.shape[1:] != (3, 3):
            raise ValueError("rotations: None, [R,3,3] matrices or a list of angles expected, got shape %s" % (rot.shape,))
    with_identity = normalize and rotations is not None
    if with_identity:
        rot = np.concatenate((identity, rot))
    w = C.envmap_light_weights(t32(envmap), t32(dirs), t32(rot))
    if normalize:
        host = w.detach().cpu().numpy().astype(np.float64)          # ([R,L,3]: a few KB; the division is host arithmetic)
        total = host[0].sum() / 3.0
        if not total > 0:
            raise ValueError("the probe's energy is %g: nothing to normalise by" % total)
        host = (host[1:] if with_identity else host) / total
        w = torch.from_numpy(host.astype(np.float32)).to(w.device)
    return w.contiguous()


# ---------------------------------------------------------------- the relit view
def relight(model, dataset, cam, weights, feat_agg=None, chunk=None, exposure=1.0):
    """The view of camera `cam` under the probe(s) `weights` [R,L,3] (`envmap_weights`; light l = the l-th of
    `view_samples(dataset.store, cam)`) -> {'linear': [R,imh,imw,3], 'image': [R,imh,imw,3]} on the device.
    The view's samples are loaded `chunk` lights at a time (default: the config's `bs`; the short last chunk is kept) and
    rendered by `Model.call` -- with feat_agg (`nlt_test.extract_feat`) as `obs_override`, the fused query-only plan of the
    inference mode; else with the samples' own neighbours.  Every chunk's `pred_camspc` goes straight to the accumulation on
    the current stream, in light order; `linear` is sum_l weights[r,l] * lin(clip01(pred_l)) (one fmaf per light, so the
    chunk size changes no bit) and `image` = enc(clip01(exposure * linear)).  lin / enc: the identity when the config's
    `linear_space` is set, else the sRGB decode / encode -- `image` is in the space the model's own `pred_camspc` is in."""
    config = model.config
    is_linear = config.getboolean('DEFAULT', 'linear_space')
    chunk = config.getint('DEFAULT', 'bs') if chunk is None else int(chunk)
    if chunk <= 0:
        raise ValueError("chunk must be positive, got %d" % chunk)
    samples = view_samples(dataset.store, cam)
    if not torch.is_tensor(weights) or weights.dim() != 3 or weights.shape[1] != len(samples) or weights.shape[2] != 3:
        raise ValueError("weights: an [R,%d,3] tensor expected (camera '%s' has %d lights), got %s"
                         % (len(samples), cam, len(samples), tuple(weights.shape) if torch.is_tensor(weights) else type(weights).__name__))
    weights = weights.detach().to(dtype=torch.float32).contiguous()
    ids = [i for i, _ in samples]
    acc = None
    for l0 in range(0, len(ids), chunk):
        batch = dataset.load_batch(ids[l0:l0 + chunk])
        pred_camspc = model.call(batch, 'test', obs_override=feat_agg)[0]
        if acc is None:
            weights = weights.to(pred_camspc.device)
            acc = torch.zeros((weights.shape[0],) + tuple(pred_camspc.shape[1:]), device=pred_camspc.device, dtype=torch.float32)
        C.relight_accumulate(pred_camspc.contiguous(), weights, l0, acc, is_linear)
    return {'linear': acc, 'image': C.relight_finish(acc, exposure, not is_linear)}


# ---------------------------------------------------------------- probes on disk
_HDR_RES = re.compile(r'^-Y (\d+) \+X (\d+)$')


def decode_hdr(data):
    """The bytes of a Radiance picture -> [H,W,3] float32.  RGBE pixels (value = mantissa * 2^(e - 136), e = 0: black), flat or
    new-style run-length encoded scanlines, `-Y H +X W` orientation; anything else raises ValueError."""
    end = data.find(b'\n\n')
    if not (data.startswith(b'#?RADIANCE') or data.startswith(b'#?RGBE')) or end < 0:
        raise ValueError("not a Radiance picture (no '#?RADIANCE' header)")
    for line in data[:end].split(b'\n')[1:]:
        if line.startswith(b'FORMAT=') and line.strip() != b'FORMAT=32-bit_rle_rgbe':
            raise ValueError("unsupported %s (32-bit_rle_rgbe only)" % line.decode('ascii', 'replace'))
    nl = data.find(b'\n', end + 2)
    res = _HDR_RES.match(data[end + 2:max(nl, 0)].decode('ascii', 'replace').strip())
    if nl < 0 or res is None:
        raise ValueError("unsupported resolution line %r ('-Y H +X W' only)" % data[end + 2:max(nl, end + 2)])
    h, w = int(res.group(1)), int(res.group(2))
    if h <= 0 or w <= 0:
        raise ValueError("empty picture: %d x %d" % (h, w))
    buf = np.frombuffer(data, np.uint8, offset=nl + 1)
    rgbe = np.empty((h, w, 4), np.uint8)
    at = 0
    for y in range(h):
        if at + 4 > buf.size:
            raise ValueError("scanline %d: the file ends early" % y)
        if 8 <= w <= 32767 and buf[at] == 2 and buf[at + 1] == 2 and not buf[at + 2] & 0x80:      # new-style RLE
            if (int(buf[at + 2]) << 8 | int(buf[at + 3])) != w:
                raise ValueError("scanline %d: run-length header says %d pixels, the picture has %d"
                                 % (y, int(buf[at + 2]) << 8 | int(buf[at + 3]), w))
            at += 4
            for ch in range(4):
                x = 0
                while x < w:
                    if at + 2 > buf.size:
                        raise ValueError("scanline %d: the file ends early" % y)
                    count = int(buf[at])
                    if count > 128:                                  # a run
                        count -= 128
                        if x + count > w:
                            raise ValueError("scanline %d: a run passes the end of the line" % y)
                        rgbe[y, x:x + count, ch] = buf[at + 1]
                        at += 2
                    else:                                            # literals
                        if count == 0 or x + count > w or at + 1 + count > buf.size:
                            raise ValueError("scanline %d: bad literal count %d" % (y, count))
                        rgbe[y, x:x + count, ch] = buf[at + 1:at + 1 + count]
                        at += 1 + count
                    x += count
        else:                                                        # flat
            if at + 4 * w > buf.size:
                raise ValueError("scanline %d: the file ends early" % y)
            line = buf[at:at + 4 * w].reshape(w, 4)
            if ((line[:, 0] == 1) & (line[:, 1] == 1) & (line[:, 2] == 1)).any():
                raise ValueError("scanline %d: old-style run-length encoding is not supported" % y)
            rgbe[y] = line
            at += 4 * w
    e = rgbe[:, :, 3].astype(np.int32)
    scale = np.where(e > 0, np.ldexp(1.0, e - 136), 0.0)
    return (rgbe[:, :, :3].astype(np.float64) * scale[:, :, None]).astype(np.float32)


def read_envmap(path):
    """A probe as [He,We,3] float32 linear radiance: `.npy` ([He,We,3] floats) or Radiance `.hdr` (`decode_hdr`).  No EXR."""
    low = path.lower()
    if low.endswith('.npy'):
        a = np.load(path)
        if a.ndim != 3 or a.shape[2] != 3 or a.dtype.kind != 'f':
            raise ValueError("%s: a float [He,We,3] array expected, got %s %s" % (path, a.dtype, a.shape))
        return np.ascontiguousarray(a, dtype=np.float32)
    if low.endswith('.hdr') or low.endswith('.pic'):
        with open(path, 'rb') as h:
            return decode_hdr(h.read())
    raise ValueError("%s: .npy and Radiance .hdr probes only" % path)
