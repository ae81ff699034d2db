"""data_gen/render.py:209-351 on HIP: view / light cosine maps and the bidirectional UV <-> camera
mapping.  `intersect` is the dict render.py builds from xm.blender.camera.backproject_to_3d
(render.py:142-148), here in DENSE form over the imh x imw pixel grid (row-major, xys order):
    'locs', 'normals'  [P,3] float64 CUDA        'valid' [P] uint8 (loc is not None and the hit
    'face_i' [P] int64 (only for the mapping)     object is the subject, render.py:219,267,302)
    'occluded' [P] uint8 (only for the light: the result of the reference's BVH shadow rays,
                          render.py:238-254)
The reference's list-of-Vector form is converted with `dense_intersect`; data_gen/mesh.py casts the rays itself
(`backproject`, `shadow`) for a camera and a light that are not in a capture."""
import os
from os.path import join

import numpy as np
import torch

from .. import _capi as C
from .util import dump_json, encode_pool, load_json, name_from_json_path


def dense_intersect(intersect, obj_name, device='cuda', occluded=None):
    """render.py's {'obj_names','locs','normals','face_i'} lists (None where the ray missed) -> dense."""
    n = len(intersect['locs'])
    valid = np.array([l is not None and o == obj_name for l, o in zip(intersect['locs'], intersect['obj_names'])])
    zero = (0.0, 0.0, 0.0)
    locs = np.array([tuple(l) if v else zero for l, v in zip(intersect['locs'], valid)], np.float64).reshape(n, 3)
    normals = np.array([tuple(x) if v else zero for x, v in zip(intersect['normals'], valid)], np.float64).reshape(n, 3)
    out = {'locs': torch.from_numpy(locs).to(device), 'normals': torch.from_numpy(normals).to(device),
           'valid': torch.from_numpy(valid.astype(np.uint8)).to(device)}
    if 'face_i' in intersect:
        out['face_i'] = np.array([-1 if (f is None or not v) else f for f, v in zip(intersect['face_i'], valid)], np.int64)
    if occluded is not None:
        out['occluded'] = torch.from_numpy(np.asarray(occluded, np.uint8)).to(device)
    return out


def _im_hw(xys):
    xys = np.asarray(xys)
    return int(xys[:, 1].max()) + 1, int(xys[:, 0].max()) + 1


def calc_view_cosines(cam_loc, xys, intersect, obj_name=None):
    """render.py:209-228 -> float64 [imh,imw]."""
    imh, imw = _im_hw(xys)
    cos, _ = C.cosine_map(intersect['locs'], intersect['normals'], intersect['valid'], None, cam_loc, want_u8=False)
    return cos.view(imh, imw)


def calc_light_cosines(light_loc, xys, cam_intersect, obj=None):
    """render.py:231-276 -> float64 [imh,imw]; cast shadows come in through cam_intersect['occluded']."""
    imh, imw = _im_hw(xys)
    cos, _ = C.cosine_map(cam_intersect['locs'], cam_intersect['normals'], cam_intersect['valid'],
                          cam_intersect.get('occluded'), light_loc, want_u8=False)
    return cos.view(imh, imw)


def cosines_to_uint8(src_loc, intersect, imh, imw, light=False):
    """render.py:162-171 in one launch: the cosine map clipped to [0,1] and TRUNCATED to uint8."""
    _, q = C.cosine_map(intersect['locs'], intersect['normals'], intersect['valid'],
                        intersect.get('occluded') if light else None, src_loc, want_float=False)
    return q.view(imh, imw)


def grid_query_unstruct(uvs, values, grid_res, method=None):
    """xiuminglib/img.py:289-431 for the one method NLT uses (griddata / nearest + max_l1_interp)."""
    method = method or {'func': 'griddata'}
    if method.get('func') != 'griddata' or method.get('func_underlying', 'linear') != 'nearest':
        raise NotImplementedError(method)
    fill = method.get('fill_value', (0,))
    if len(set(fill)) != 1:
        raise NotImplementedError("per-channel fill values")
    max_l1 = method.get('max_l1_interp', np.inf)
    if max_l1 is None or not np.isfinite(max_l1):
        raise NotImplementedError("unbounded max_l1_interp")
    if values.dim() == 1:
        values = values.view(-1, 1)
    h, w = grid_res
    out = C.uv_index_map(uvs.contiguous(), values.contiguous(), h, w, int(max_l1), float(fill[0]))
    return out[:, :, 0] if out.shape[2] == 1 else out


def _params(x):
    """A camera / light as render.py's load_json gives it: the dict itself, or the path of its .json."""
    return load_json(x) if isinstance(x, str) else x


def _sample_hw(intersect, rgb_camspc, alpha):
    for img in (alpha, rgb_camspc):
        if img is not None:
            return int(img.shape[0]), int(img.shape[1])
    if 'hw' in intersect:
        return tuple(int(x) for x in intersect['hw'])
    if intersect['valid'].dim() == 2:
        return tuple(intersect['valid'].shape)
    raise ValueError("the camera resolution is unknown: give alpha or rgb_camspc, intersect['hw'] = (imh, imw), or a 2-D 'valid'")


def render_sample(intersect, cached_unwrap, cam, light, uvs, rgb_camspc=None, alpha=None, max_l1_interp=4):
    """render.py:main after Blender (lines 150-179): the bidirectional mapping, then every per-sample buffer in two launches
    (nlt_capture_camspc over the camera pixels, nlt_capture_uvspc over the UV texels).

    intersect: the dense form of `dense_intersect` (with 'face_i'; 'occluded' from the caller's shadow rays, absent = none).
    cam, light: the dicts of cam.json / light.json (or their paths); only 'position' is read here.
    rgb_camspc [imh,imw,3|4] uint8 and alpha [imh,imw] uint8 as Blender rendered them (tensors or arrays); rgb_camspc = None is
    a test sample without ground truth (no rgb), alpha = None masks nothing.
    Returns {file name: device tensor}, one entry per file `write_sample` writes, plus '_uv2cam' / '_cam2uv' / '_alpha' (the float64
    maps and the mask: the debug re-projections and the tests read them)."""
    cam, light = _params(cam), _params(light)
    dev = intersect['valid'].device
    as_dev = lambda a: None if a is None else (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).to(dev).contiguous()
    rgb_camspc, alpha = as_dev(rgb_camspc), as_dev(alpha)
    imh, imw = _sample_hw(intersect, rgb_camspc, alpha)
    if alpha is not None and alpha.dim() != 2:
        raise ValueError("alpha must be [imh,imw], got %s" % (tuple(alpha.shape),))
    xs, ys = np.meshgrid(range(imw), range(imh))
    xys = np.dstack((xs, ys)).reshape(-1, 2)                        # render.py:136-142
    uv2cam, cam2uv = calc_bidir_mapping(cached_unwrap, None, xys, intersect, uvs, max_l1_interp)
    cvis_c, lvis_c, uv2cam_f16, uv2cam_png = C.capture_camspc(
        intersect['locs'].reshape(-1, 3), intersect['normals'].reshape(-1, 3), intersect['valid'].reshape(-1),
        None if intersect.get('occluded') is None else intersect['occluded'].reshape(-1),
        cam['position'], light['position'], alpha, uv2cam.contiguous())
    cvis, lvis, rgb, cam2uv_f16, cam2uv_png = C.capture_uvspc(cam2uv.contiguous(), cvis_c, lvis_c, rgb_camspc)
    sample = {'uv2cam.png': uv2cam_png, 'cam2uv.png': cam2uv_png, 'uv2cam.npy': uv2cam_f16, 'cam2uv.npy': cam2uv_f16,
              'lvis_camspc.png': lvis_c, 'cvis_camspc.png': cvis_c, 'cvis.png': cvis, 'lvis.png': lvis,
              '_uv2cam': uv2cam, '_cam2uv': cam2uv, '_alpha': alpha}
    if rgb_camspc is not None:
        sample['rgb_camspc.png'], sample['rgb.png'] = rgb_camspc, rgb
    if alpha is not None:
        sample['alpha.png'] = alpha
    return sample


def _neighbors(nn, cam, light):
    """render.py:200-206: {'cam': cam_nn[cam_name], 'light': light_nn[light_name]}.  nn: that dict itself, or the pair
    (cam_nn, light_nn) of neighbour tables (dicts or .json paths), looked up by the camera's / light's name."""
    if isinstance(nn, dict):
        return nn
    name = lambda x: name_from_json_path(x) if isinstance(x, str) else x['name']
    cam_nn, light_nn = (_params(t) for t in nn)
    return {'cam': cam_nn[name(cam)], 'light': light_nn[name(light)]}


def write_sample(outdir, sample, cam, light, nn, debug=False, workers=None):
    """render.py:156-206: writes one sample directory -- the PNGs (through util/vis.py:write_img, PIL), the two float16 .npy
    maps, cam.json / light.json (copied when a path is given, dumped when a dict) and nn.json.  debug: also the three
    `*_camspc_repro.png` of render.py:180-194.  One device-to-host copy per buffer, then the encodes on a thread pool of
    min(16, number of files) threads (`workers` overrides it; 1 = in order on one thread).  Returns the file names written."""
    from shutil import copyfile
    from ..util.vis import write_img
    files = {k: v for k, v in sample.items() if not k.startswith('_')}
    if debug:                                                       # render.py:186-188: back through uv2cam (masked, float64)
        uv2cam = sample['_uv2cam']
        if sample['_alpha'] is not None:
            uv2cam = torch.where((sample['_alpha'] < 255).unsqueeze(-1), torch.zeros_like(uv2cam), uv2cam)
        for k in ('cvis', 'lvis', 'rgb'):
            if k + '.png' in files:
                files[k + '_camspc_repro.png'] = C.remap_bilinear(files[k + '.png'], uv2cam.contiguous())
    host = {k: v.cpu().numpy() for k, v in files.items()}
    os.makedirs(outdir, exist_ok=True)

    def put(name):
        if name.endswith('.npy'):
            np.save(join(outdir, name), host[name])
        else:
            write_img(host[name], join(outdir, name))
    with encode_pool(len(host), workers) as pool:
        list(pool.map(put, sorted(host)))
    for name, x in (('cam.json', cam), ('light.json', light)):
        if isinstance(x, str):
            copyfile(x, join(outdir, name))
        else:
            dump_json(x, join(outdir, name))
    dump_json(_neighbors(nn, cam, light), join(outdir, 'nn.json'))
    return sorted(host) + ['cam.json', 'light.json', 'nn.json']


def calc_bidir_mapping(cached_unwrap, obj_name, xys, intersect, uvs, max_l1_interp=4):
    """render.py:279-351.  cached_unwrap: the {face: [[loop, vert, u, v], ...]} table of
    data_gen/uv_unwrap.py:53-74 (dict, or a path to its pickle), or its dense form {'uv': float64 [F,Vmax,2], 'counts': [F]}
    (data_gen/mesh.py:dense_unwrap), which builds the same sample list with array indexing instead of a Python loop over the
    hit pixels.  Returns (uv2cam [imh,imw,2], cam2uv [uvs,uvs,2]) float64 in [0,1]."""
    if isinstance(cached_unwrap, str):
        import pickle
        with open(cached_unwrap, 'rb') as h:
            cached_unwrap = pickle.load(h)
    imh, imw = _im_hw(xys)
    xys = np.asarray(xys)
    face_i = np.asarray(intersect['face_i'])
    hit = np.nonzero(face_i >= 0)[0]
    if isinstance(cached_unwrap, dict) and 'uv' in cached_unwrap and 'counts' in cached_unwrap:
        table, counts = np.asarray(cached_unwrap['uv'], np.float64), np.asarray(cached_unwrap['counts'])
        faces = face_i[hit]
        n = counts[faces]
        if faces.size and (faces.max() >= len(counts) or n.min() <= 0):
            raise KeyError("a hit face has no entry in the dense unwrap table")
        uv = table[faces][np.arange(table.shape[1])[None, :] < n[:, None]]      # row-major: pixel-major, then the face's vertices
        xy = np.repeat(xys[hit].astype(np.float64), n, 0)
    else:
        cam_locs, uv_list = [], []
        for p in hit:                                           # pixel-major, then the face's vertices: the
            uv = np.asarray(cached_unwrap[int(face_i[p])])[:, 2:]      # reference's sample order (render.py:299-317)
            uv_list.append(uv)
            cam_locs.append(np.repeat(xys[p:p + 1].astype(np.float64), uv.shape[0], 0))
        uv = np.vstack(uv_list)
        xy = np.vstack(cam_locs)
    dev = intersect['valid'].device
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float64)).to(dev)
    method = {'func': 'griddata', 'func_underlying': 'nearest', 'fill_value': (0,), 'max_l1_interp': max_l1_interp}
    # UV -> camera: locations are camera pixels (v up), values the face-vertex UVs (y down)   render.py:305-309
    uv2cam = grid_query_unstruct(t(np.stack((xy[:, 0] / float(imw), 1 - xy[:, 1] / float(imh)), 1)),
                                 t(np.stack((uv[:, 0], 1 - uv[:, 1]), 1)), (imh, imw), method)
    # camera -> UV: locations are the face-vertex UVs, values the camera pixel (y down)       render.py:311-315
    cam2uv = grid_query_unstruct(t(uv), t(np.stack((xy[:, 0] / float(imw), xy[:, 1] / float(imh)), 1)),
                                 (uvs, uvs), method)
    return uv2cam, cam2uv
