"""TEST-ONLY: the float64 NumPy restatement csrc/unwrap.hip is held to, bit for bit -- stages a-e and g of include/nlt_hip.h's
"UV unwrap", operation by operation (NumPy's element-wise ufuncs never fuse a multiply with an add): the fan sums, the 256-wide
tree sum, the tie rules, union-find for the islands, exact min / max for the boxes.  `projection_basis` and `pack_islands` are
the package's own host code (tests/test_host_unwrap.py holds them to properties) and are called, not restated.  Also the small
meshes the host and GPU tests share."""
import numpy as np

from nlt_amd.data_gen import unwrap as U
from raycast_ref import BUNNY, CUBE, cross, dot, icosphere           # noqa: F401  (re-exported for the tests)


def mesh_arrays(verts, faces):
    """(verts float64 [V,3], loop_verts int32 [L], face_off int32 [F+1]) without the package's range checks."""
    counts = np.array([len(f) for f in faces], np.int64)
    return (np.ascontiguousarray(np.asarray(verts, np.float64).reshape(-1, 3)), np.array([v for f in faces for v in f], np.int32),
            np.concatenate(([0], np.cumsum(counts))).astype(np.int32))


# --------------------------------------------------------------------------------------------------------------------- a
def frames(verts, loop_verts, face_off):
    """-> n [F,3], unit [F,3], area [F], ok uint8 [F]."""
    counts = np.diff(face_off)
    nf, vmax = len(counts), int(counts.max())
    idx = np.zeros((nf, vmax), np.int64)
    good = counts >= 3
    for j in range(vmax):
        has = counts > j
        idx[has, j] = loop_verts[face_off[:-1][has] + j]
        good &= ~has | ((idx[:, j] >= 0) & (idx[:, j] < len(verts)))
    p = verts[np.clip(idx, 0, len(verts) - 1)]
    n = np.zeros((nf, 3))
    with np.errstate(all='ignore'):
        for i in range(1, vmax - 1):
            use = good & (counts > i + 1)
            c = cross(p[:, i] - p[:, 0], p[:, i + 1] - p[:, 0])
            n[use] = n[use] + c[use]
        length = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
        ok = good & np.isfinite(length) & (length > 0)
        unit = np.where(ok[:, None], n / length[:, None], 0.0)
        area = np.where(ok, 0.5 * length, 0.0)
    return n, unit, area, ok.astype(np.uint8)


# --------------------------------------------------------------------------------------------------------------------- b
def tree_sum(x):
    """x [N,C] -> [C]: blocks of 256 in order, padded with +0.0; inside a block x[i] += x[i+s] for s = 128 .. 1; the block results
    by the same rule until one is left."""
    x = np.asarray(x, np.float64)
    while True:
        nb = (len(x) + 255) // 256
        pad = np.zeros((nb * 256, x.shape[1]))
        pad[:len(x)] = x
        b = pad.reshape(nb, 256, -1)
        s = 128
        while s >= 1:
            b[:, :s] = b[:, :s] + b[:, s:2 * s]
            s //= 2
        x = b[:, 0].copy()
        if nb == 1:
            return x[0]


def _first(mask_values, mask, largest):
    """Index of the largest / smallest value among `mask`, ties to the lowest index; -1 when the mask is empty."""
    if not mask.any():
        return -1
    v = np.where(mask, mask_values, -np.inf if largest else np.inf)
    return int(np.argmax(v) if largest else np.argmin(v))


def vectors(unit, area, ok, cos_half, cos_full, aw, omw, max_groups=256):
    """-> (vectors [K,3], the seeds).  ValueError as the package raises it."""
    okb = ok.astype(bool)
    remaining = okb.copy()
    seed = _first(area, okb, True)
    if seed < 0:
        raise ValueError("no face with an area")
    vecs, seeds, best = [], [], None
    while True:
        if len(seeds) >= max_groups:
            raise ValueError("more than max_groups projection vectors")
        gathered = remaining & ((np.arange(len(area)) == seed) | (dot(unit, unit[seed][None, :]) > cos_half))
        remaining &= ~gathered
        w = (area * aw) + omw
        s = tree_sum(np.where(gathered[:, None], unit * w[:, None], 0.0))
        vec = s / np.sqrt((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2])
        vecs.append(vec)
        seeds.append(seed)
        d = np.where(okb, dot(unit, vec[None, :]), 0.0)
        best = d if best is None else np.where(okb, np.where(d > best, d, best), 0.0)
        seed = _first(best, remaining, False)
        if seed < 0 or best[seed] >= cos_full:
            return np.array(vecs), seeds


# --------------------------------------------------------------------------------------------------------------------- c
def assign(unit, ok, vecs):
    d = np.stack([dot(unit, v[None, :]) for v in vecs], 1)
    return np.where(ok.astype(bool), np.argmax(d, 1), -1).astype(np.int32)                  # (argmax: the first maximum)


# --------------------------------------------------------------------------------------------------------------------- d
def islands(loop_verts, face_off, n_verts, group):
    """Union-find over the links of include/nlt_hip.h -> label int32 [F]: the smallest face index of the component, -1."""
    counts = np.diff(face_off)
    loop_face = np.repeat(np.arange(len(counts)), counts)
    nxt = np.arange(len(loop_verts)) + 1
    last = face_off[1:][loop_face] - 1
    nxt = np.where(np.arange(len(loop_verts)) == last, face_off[:-1][loop_face], nxt)
    a, b = loop_verts.astype(np.int64), loop_verts[nxt].astype(np.int64)
    keys = np.minimum(a, b) * int(n_verts) + np.maximum(a, b)
    order = np.argsort(keys, kind='stable')
    ks = keys[order]
    parent = list(range(len(counts)))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for i in np.nonzero(ks[1:] == ks[:-1])[0]:
        fa, fb = int(loop_face[order[i]]), int(loop_face[order[i + 1]])
        if group[fa] >= 0 and group[fa] == group[fb]:
            ra, rb = find(fa), find(fb)
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)
    return np.array([find(f) if group[f] >= 0 else -1 for f in range(len(counts))], np.int32), loop_face.astype(np.int32)


# --------------------------------------------------------------------------------------------------------------------- e
def boxes(verts, loop_verts, loop_face, group, island, frames_, n_islands):
    """-> (puv [L,2], boxes [I,4] = (umin, vmin, umax, vmax))."""
    isl, g = island[loop_face], group[loop_face]
    use = (isl >= 0) & (g >= 0)
    p = verts[np.where(use, loop_verts, 0)]
    fr = np.asarray(frames_)[np.maximum(g, 0)]
    with np.errstate(all='ignore'):
        pu = np.where(use, dot(p, fr[:, 0]) + 0.0, 0.0)
        pv = np.where(use, dot(p, fr[:, 1]) + 0.0, 0.0)
    box = np.stack([np.full(n_islands, np.inf)] * 2 + [np.full(n_islands, -np.inf)] * 2, 1)
    np.minimum.at(box[:, 0], isl[use], pu[use]); np.minimum.at(box[:, 1], isl[use], pv[use])
    np.maximum.at(box[:, 2], isl[use], pu[use]); np.maximum.at(box[:, 3], isl[use], pv[use])
    return np.stack((pu, pv), 1), box


# --------------------------------------------------------------------------------------------------------------------- g
def uvs(puv, face_off, island, box, rot, offsets, scale):
    counts = np.diff(face_off)
    vmax = int(counts.max())
    uv = np.zeros((len(counts), vmax, 2))
    for j in range(vmax):
        f = np.nonzero((counts > j) & (island >= 0))[0]
        i, p = island[f], puv[face_off[:-1][f] + j]
        turned = np.asarray(rot, bool)[i]
        lu = np.where(turned, p[:, 1] - box[i, 1], p[:, 0] - box[i, 0])
        lv = np.where(turned, box[i, 2] - p[:, 0], p[:, 1] - box[i, 1])
        uv[f, j, 0] = lu * scale + offsets[i, 0]
        uv[f, j, 1] = lv * scale + offsets[i, 1]
    return uv


def unwrap(verts, faces, angle_limit=66., area_weight=0., margin=0.002, max_groups=256):
    """Everything `smart_unwrap` returns, from the restatement: a dict of arrays under the `Unwrap` attribute names, plus n, unit
    [F,3], area, ok and puv."""
    verts, loop_verts, face_off = mesh_arrays(verts, faces)
    cos_half, cos_full = U.angle_cosines(angle_limit)
    aw = float(area_weight)
    n, unit, area, ok = frames(verts, loop_verts, face_off)
    vecs, seeds = vectors(unit, area, ok, cos_half, cos_full, aw, 1.0 - aw, max_groups)
    group = assign(unit, ok, vecs)
    labels, loop_face = islands(loop_verts, face_off, len(verts), group)
    fr = np.stack([np.stack(U.projection_basis(v)) for v in vecs])
    island_labels, island = U.island_numbers(labels)
    puv, box = boxes(verts, loop_verts, loop_face, group, island, fr, len(island_labels))
    scale, rot, offsets = U.pack_islands(box[:, 2:] - box[:, :2], island_labels, margin)
    uv = uvs(puv, face_off, island, box, rot, offsets, scale)
    return dict(n=n, unit=unit, area=area, ok=ok, vectors=vecs, seeds=seeds, groups=group, labels=labels, island_labels=island_labels,
                island=island, frames=fr, puv=puv, boxes=box, scale=scale, rot=rot, offsets=offsets, uv=uv,
                counts=np.diff(face_off).astype(np.int64), loop_face=loop_face)


# ---------------------------------------------------------------------------------------------------------------------
# meshes
# ---------------------------------------------------------------------------------------------------------------------
def cube_mesh():
    from nlt_amd.data_gen.mesh import load_mesh
    m = load_mesh(CUBE)
    return m['vertices'], m['faces']


def bunny_mesh():
    from nlt_amd.data_gen.mesh import load_mesh
    m = load_mesh(BUNNY)
    return m['vertices'], m['faces']


def grid_mesh(n, quads=False):
    """A flat n x n grid of cells in the plane z = 0, counter-clockwise seen from +z: 2 n n triangles, or n n quads."""
    xs, ys = np.meshgrid(np.arange(n + 1, dtype=np.float64), np.arange(n + 1, dtype=np.float64))
    verts = np.stack((xs.reshape(-1) * 0.25, ys.reshape(-1) * 0.25, np.zeros((n + 1) ** 2)), 1)
    faces = []
    for j in range(n):
        for i in range(n):
            a, b, c, d = j * (n + 1) + i, j * (n + 1) + i + 1, (j + 1) * (n + 1) + i + 1, (j + 1) * (n + 1) + i
            faces += [[a, b, c, d]] if quads else [[a, b, c], [a, c, d]]
    return verts, faces


def soup_mesh(n, seed):
    """n random triangles that share no vertex index (raycast_ref.soup): one island per face."""
    from raycast_ref import soup
    return soup(n, seed).reshape(-1, 3), [[3 * i, 3 * i + 1, 3 * i + 2] for i in range(n)]


def tetrahedron():
    v = np.array([(1, 1, 1), (1, -1, -1), (-1, 1, -1), (-1, -1, 1)], np.float64)
    return v, [[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]]


def octahedron():
    v = np.array([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)], np.float64)
    return v, [[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]]


def two_triangles(folded):
    """Two triangles sharing the edge (0, 1): coplanar in z = 0, or the second folded up by 90 degrees."""
    v = np.array([(0, 0, 0), (1, 0, 0), (0.5, 1, 0), (0.5, 0, 1) if folded else (0.5, -1, 0)], np.float64)
    return v, [[0, 1, 2], [1, 0, 3]]


def mixed_mesh():
    """Triangles, quads and a pentagon on a bent strip (two planes meeting at 60 degrees), sharing edges."""
    c, s = 0.5, 3 ** 0.5 / 2
    v = np.array([(0, 0, 0), (1, 0, 0), (2, 0, 0), (0, 1, 0), (1, 1, 0), (2, 1, 0), (0.5, 1.8, 0), (2 + c, 0, s), (2 + c, 1, s),
                  (2 + 2 * c, 0.5, 2 * s), (1.5, 1.7, 0), (2.2, 1.5, 0)], np.float64)
    return v, [[0, 1, 4, 3], [1, 2, 5, 4], [3, 4, 6], [2, 7, 8, 5], [7, 9, 8], [4, 5, 11, 10, 6]]


def ribbon(n, seed):
    """A coplanar strip of n triangles whose faces are randomly permuted: labels travel far and against the index order."""
    k = n // 2 + 2
    verts = np.zeros((2 * k, 3))
    verts[0::2, 0] = np.arange(k) * 0.1
    verts[1::2, 0] = np.arange(k) * 0.1
    verts[1::2, 1] = 0.1
    faces = []
    for i in range(n):
        a = i
        faces.append([a, a + 2, a + 1] if i % 2 == 0 else [a, a + 1, a + 2])
    perm = np.random.default_rng(seed).permutation(n)
    return verts, [faces[i] for i in perm]


def partition(labels):
    """The partition of the faces a label array stands for: a set of frozensets (degenerate faces, label -1, left out)."""
    out = {}
    for f, l in enumerate(labels):
        if l >= 0:
            out.setdefault(int(l), []).append(f)
    return {frozenset(v) for v in out.values()}
