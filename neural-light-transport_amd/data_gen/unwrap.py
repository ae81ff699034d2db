"""A mesh -> the {face: [[loop, vert, u, v], ...]} table of data_gen/uv_unwrap.py, without Blender: smart projection restated on
csrc/unwrap.hip (include/nlt_hip.h: "UV unwrap").  The kernels find the projection vectors, the groups, the islands, the island
boxes and the UVs; host code here is the two cosines of the angle limit, one orthonormal frame per vector, the shelf packing of
a few hundred rectangles, and the pickle.  Not Blender's result: what differs is listed in DESIGN.md section 8.

No welding is done: islands are joined through shared vertex INDICES, so a mesh whose faces share no index (a triangle soup, an
.obj written with one vertex per corner) gives one island per face."""
import math
import pickle

import numpy as np
import torch

from .. import _capi as C

PACK_SHRINK = 0.97
_PACK_MAX_STEPS = 1024                                  # 0.97^1024 ~ 3e-14: by then every box is its margin alone


def projection_basis(vec):
    """vec: a unit vector -> (U, V), float64, orthonormal, with cross(U, V) = vec.  V = cross(vec, a) / |cross(vec, a)| for the
    coordinate axis a on which vec is smallest (ties to the first axis), U = cross(V, vec): sqrt and divide only.  For
    vec = (0, 0, 1): U = (1, 0, 0), V = (0, 1, 0)."""
    n = np.asarray(vec, np.float64).reshape(3)
    a = np.zeros(3)
    a[int(np.argmin(np.abs(n)))] = 1.0
    v = np.cross(n, a)
    v = v / np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
    u = np.cross(v, n)
    u = u / np.sqrt((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2])
    return u + 0.0, v + 0.0                             # (+ 0.0: no -0.0 in a frame)


def _shelves(tw, th, order, scale, margin):
    """Shelf placement of the turned boxes at `scale`, left to right in rows of width 1, each box grown by `margin` on every
    side -> (offsets of the boxes' lower-left corners [I,2], fits)."""
    off = np.zeros((len(tw), 2))
    x = y = row = 0.0
    for i in order:
        w, h = tw[i] * scale + 2 * margin, th[i] * scale + 2 * margin
        if w > 1.0:
            return off, False
        if x > 0.0 and x + w > 1.0:
            x, y, row = 0.0, y + row, 0.0
        off[i] = (x + margin, y + margin)
        x, row = x + w, max(row, h)
        if y + row > 1.0:
            return off, False
    return off, True


def pack_islands(wh, labels, margin):
    """wh [I,2]: the islands' box sizes (pu extent, pv extent); labels [I]: their labels (the tie-break) -> (scale, rot bool [I],
    offsets float64 [I,2]).  An island taller than wide is turned by a proper quarter turn (not mirrored); islands go by turned
    height, descending, ties to the lower label, onto shelves of width 1; a box of turned size (w, h) occupies
    [x, x + w scale + 2 margin] x [y, y + h scale + 2 margin] and its lower-left corner is offset = (x + margin, y + margin).
    One scale for all: min(1 / sqrt(sum w h), (1 - 2 margin) / max turned width), then times 0.97 until the shelves fit in the
    unit square (shelf feasibility is not monotone in the scale, so a bisection would be wrong)."""
    wh = np.asarray(wh, np.float64).reshape(-1, 2)
    labels = np.asarray(labels).reshape(-1)
    margin = float(margin)
    if not 0.0 <= margin < 0.5:
        raise ValueError("margin must lie in [0, 0.5), got %r" % margin)
    rot = wh[:, 1] > wh[:, 0]
    tw, th = np.where(rot, wh[:, 1], wh[:, 0]), np.where(rot, wh[:, 0], wh[:, 1])
    order = sorted(range(len(wh)), key=lambda i: (-th[i], labels[i]))
    area, widest = float((wh[:, 0] * wh[:, 1]).sum()), float(tw.max()) if len(tw) else 0.0
    scale = min(1.0 / math.sqrt(area) if area > 0 else math.inf, (1.0 - 2 * margin) / widest if widest > 0 else math.inf)
    if not math.isfinite(scale):
        scale = 1.0
    per_row = math.floor(1.0 / (2 * margin)) if margin > 0 else math.inf     # a box is at least 2 margin wide and high
    for _ in range(_PACK_MAX_STEPS if len(wh) <= per_row * per_row else 0):
        offsets, fits = _shelves(tw, th, order, scale, margin)
        if fits:
            return scale, rot, offsets
        scale *= PACK_SHRINK
    raise ValueError("%d islands do not fit the unit square with a margin of %g" % (len(wh), margin))


class Unwrap:
    """What `smart_unwrap` returns.  dense: {'uv' float64 [F,Vmax,2], 'counts' int64 [F]} as `calc_bidir_mapping` takes it;
    vectors [K,3]; groups int32 [F] (-1: a degenerate face); labels int32 [F] (the smallest face index of the face's island, -1);
    island_labels [I] (ascending) and boxes [I,4] = (umin, vmin, umax, vmax) of the projected islands; scale, rot bool [I],
    offsets [I,2]: `pack_islands`' answer; params, rounds: what was asked and how many rounds stages b and d took."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def table(self):
        """{face: float64 [n,4] of (loop, vert, u, v)}, loop indices cumulative over the faces: the pickle's content."""
        uv, out, loop = self.dense['uv'], {}, 0
        for fi, f in enumerate(self.faces):
            k = len(f)
            out[fi] = np.concatenate((np.arange(loop, loop + k, dtype=np.float64)[:, None], np.asarray(f, np.float64)[:, None], uv[fi, :k]), 1)
            loop += k
        return out

    def record(self):
        """The `unwrap` entry of <outroot>.capture.json."""
        return dict(method='smart', **self.params, groups=int(len(self.vectors)), islands=int(len(self.island_labels)), scale=float(self.scale))


def mesh_arrays(mesh_or_dict):
    """(vertices float64 [V,3], faces: lists of vertex indices, loop_verts int32 [L], face_off int32 [F+1])."""
    verts, faces = (mesh_or_dict['vertices'], mesh_or_dict['faces']) if isinstance(mesh_or_dict, dict) else (mesh_or_dict.vertices, mesh_or_dict.faces)
    verts = np.ascontiguousarray(np.asarray(verts, np.float64).reshape(-1, 3))
    faces = [list(f) for f in faces]
    counts = np.array([len(f) for f in faces], np.int64)
    if not len(faces) or not len(verts) or counts.sum() == 0:
        raise ValueError("the mesh has no face")
    if max(len(verts), int(counts.sum())) >= 2 ** 31:
        raise ValueError("the mesh is too large: 2^31 or more vertices or loops")
    face_off = np.concatenate(([0], np.cumsum(counts))).astype(np.int32)
    loop_verts = np.fromiter((v for f in faces for v in f), np.int64, int(counts.sum()))
    if loop_verts.min() < 0 or loop_verts.max() >= len(verts):
        raise ValueError("a face names a vertex outside 0 .. %d" % (len(verts) - 1))
    return verts, faces, loop_verts.astype(np.int32), face_off


def check_params(angle_limit, area_weight, margin, max_groups):
    if not 1.0 <= float(angle_limit) <= 89.0:
        raise ValueError("angle_limit takes 1 to 89 degrees, got %r" % (angle_limit,))
    if not 0.0 <= float(area_weight) <= 1.0:
        raise ValueError("area_weight takes 0 to 1, got %r" % (area_weight,))
    if not 0.0 <= float(margin) < 0.5:
        raise ValueError("margin must lie in [0, 0.5), got %r" % (margin,))
    if int(max_groups) < 1:
        raise ValueError("max_groups must be at least 1")


def angle_cosines(angle_limit):
    """(cos(limit / 2), cos(limit)): the only trigonometry of the unwrap, done here."""
    return math.cos(math.radians(float(angle_limit) / 2)), math.cos(math.radians(float(angle_limit)))


def island_numbers(labels):
    """labels int [F] -> (the distinct labels >= 0 in ascending order [I], island int32 [F]: the face's position in them, -1)."""
    labels = np.asarray(labels)
    uniq = np.unique(labels[labels >= 0])
    island = np.where(labels >= 0, np.searchsorted(uniq, np.maximum(labels, 0)), -1).astype(np.int32)
    return uniq, island


def smart_unwrap(mesh_or_dict, angle_limit=66., area_weight=0., margin=0.002, max_groups=256, device='cuda', intermediates=False):
    """Smart-projection unwrap of a `Mesh` (its world-space `vertices`, after matrix_world) or a `load_mesh` dict -> `Unwrap`.
    The defaults are those of xm.blender.object.smart_uv_unwrap.  angle_limit: 1 to 89 degrees (lower: more projection groups);
    area_weight: 0 to 1, how much a face's area weighs in its group's vector; margin: the gap kept around every island, in UV
    units; more than max_groups projection vectors raise ValueError.  No welding: faces that share no vertex index share no
    island (a triangle soup gives one island per face).  intermediates: also keep n, unit [F,3], area, ok [F] and puv [L,2]."""
    check_params(angle_limit, area_weight, margin, max_groups)
    verts, faces, loop_verts, face_off = mesh_arrays(mesh_or_dict)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    d_verts, d_lv, d_fo = dev(verts), dev(loop_verts), dev(face_off)
    cos_half, cos_full = angle_cosines(angle_limit)
    aw = float(area_weight)
    n, unit, area, ok = C.unwrap_frames(d_verts, d_lv, d_fo)
    vectors, seeds = C.unwrap_vectors(unit, area, ok, cos_half, cos_full, aw, 1.0 - aw, int(max_groups))
    group = C.unwrap_assign(unit, ok, vectors.contiguous())
    label, loop_face, island_rounds = C.unwrap_islands(d_lv, d_fo, len(verts), group)
    vec_host, labels = vectors.cpu().numpy(), label.cpu().numpy()
    frames = np.stack([np.stack(projection_basis(v)) for v in vec_host])
    island_labels, island = island_numbers(labels)
    d_island = dev(island)
    puv, boxes = C.unwrap_boxes(d_verts, d_lv, loop_face, group, d_island, dev(frames), len(island_labels))
    boxes_host = boxes.cpu().numpy()
    scale, rot, offsets = pack_islands(boxes_host[:, 2:] - boxes_host[:, :2], island_labels, margin)
    vmax = int(np.diff(face_off).max())
    uv = C.unwrap_uv(puv, d_fo, d_island, boxes, dev(rot.astype(np.uint8)), dev(offsets), scale, vmax)
    host = lambda t: t.cpu().numpy()
    extra = dict(n=host(n).T.copy(), unit=host(unit).T.copy(), area=host(area), ok=host(ok), puv=host(puv)) if intermediates else {}
    return Unwrap(dense={'uv': uv.cpu().numpy(), 'counts': np.diff(face_off).astype(np.int64)}, faces=faces, vectors=vec_host,
                  groups=group.cpu().numpy(), labels=labels, island_labels=island_labels, boxes=boxes_host, scale=float(scale), rot=rot,
                  offsets=offsets, frames=frames, seeds=seeds, rounds=dict(vectors=len(seeds), islands=int(island_rounds)),
                  params=dict(angle_limit=float(angle_limit), area_weight=aw, margin=float(margin)), **extra)


def write_unwrap(path, table):
    """The pickle data_gen/uv_unwrap.py writes: {face index: float64 [n,4] of (loop, vert, u, v)}; the `.pickle` extension is
    forced as there.  Returns the path written."""
    path = path if path.endswith('.pickle') else path + '.pickle'
    with open(path, 'wb') as h:
        pickle.dump({int(f): np.asarray(rows, np.float64) for f, rows in table.items()}, h)
    return path


def read_unwrap(path):
    with open(path, 'rb') as h:
        return pickle.load(h)


def add_unwrap_flags(parser):
    """--angle_limit / --area_weight / --margin of the CLIs that take `--uv_unwrap smart` (None: not given)."""
    parser.add_argument('--angle_limit', type=float, default=None, help="with --uv_unwrap smart: 1 to 89 degrees; lower for more "
                        "projection groups (default 89, as data_gen/uv_unwrap.py)")
    parser.add_argument('--area_weight', type=float, default=None, help="with --uv_unwrap smart: 0 to 1, weight of the faces' areas "
                        "in a projection vector (default 1, as data_gen/uv_unwrap.py)")
    parser.add_argument('--margin', type=float, default=None, help="with --uv_unwrap smart: the gap around every island, in UV units "
                        "(default 0.002)")


def check_unwrap_flags(parser, args):
    """Without `--uv_unwrap smart` the three flags are an error, not ignored; with it, the defaults are filled in and checked."""
    given = [n for n in ('angle_limit', 'area_weight', 'margin') if getattr(args, n) is not None]
    if args.uv_unwrap != 'smart':
        if given:
            parser.error("--%s is used with --uv_unwrap smart only" % given[0])
        return
    for name, default in (('angle_limit', 89.0), ('area_weight', 1.0), ('margin', 0.002)):
        if getattr(args, name) is None:
            setattr(args, name, default)
    try:
        check_params(args.angle_limit, args.area_weight, args.margin, 256)
    except ValueError as e:
        parser.error(str(e))


def load_or_unwrap(args, mesh):
    """The `--uv_unwrap` argument of capture_main / render_main -> (the table or dense unwrap, the `Unwrap` when it was computed
    here, else None)."""
    from .mesh import Mesh, unwrap_from_obj
    if args.uv_unwrap == 'smart':
        u = smart_unwrap(mesh, args.angle_limit, args.area_weight, args.margin, device=mesh.device)
        return u.dense, u
    if args.uv_unwrap.lower().endswith('.obj'):
        return unwrap_from_obj(Mesh.load(args.uv_unwrap, device=None)), None
    return read_unwrap(args.uv_unwrap), None
