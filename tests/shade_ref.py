"""TEST-ONLY: the float64 NumPy brute force nlt_render_direct (csrc/raycast.hip) is held to, bit for bit -- the direct-lighting
definition of include/nlt_hip.h written out operation by operation on top of tests/raycast_ref.py (`closest`, `shadow`, the
camera-ray rule, `unit_towards`): every sample against every triangle, the samples of a pixel summed in (j, i) order, one rounding
to float32.  NumPy's element-wise ufuncs never fuse a multiply with an add.  Besides the two outputs it returns, per sample, what
the non-vacuity conditions of the tests count (hit, flipped, lit, cast shadow, spec)."""
import numpy as np

import raycast_ref as R

PI = 3.141592653589793


def sample_rays(cam_mat_inv, cam_loc, px, py):
    """The camera-ray rule of raycast_ref.camera_rays at the (fractional) pixel positions px, py [P]."""
    m = np.asarray(cam_mat_inv, np.float64).reshape(4, 4)
    h = [((m[r, 0] * px + m[r, 1] * py) + m[r, 2]) + m[r, 3] for r in range(4)]
    to = np.stack((h[0] / h[3], h[1] / h[3], h[2] / h[3]), -1)
    return R.unit_towards(np.asarray(cam_loc, np.float64), to)[0]


def blend(a, w, u, v):
    """a [P,3,3] (corner, component) -> (w a0 + u a1) + v a2."""
    return (w[:, None] * a[:, 0] + u[:, None] * a[:, 1]) + v[:, None] * a[:, 2]


def g1(c, a2):
    return (2.0 * c) / (c + np.sqrt(a2 + (1.0 - a2) * (c * c)))


def shade_sample(tri_verts, cam_mat_inv, cam_loc, px, py, light, intensity, kd, ks, alpha, tri_normals=None, tri_rgb=None):
    """One sample per entry of px, py -> dict(radiance [P,3] (0 where the sample adds nothing), hit, flipped, facing (ci > 0),
    shadowed (hit, facing, occluded), lit, spec [P])."""
    cam_loc, light = np.asarray(cam_loc, np.float64), np.asarray(light, np.float64)
    d = sample_rays(cam_mat_inv, cam_loc, px, py)
    t, tri, _ = R.closest(np.broadcast_to(cam_loc, d.shape), d, tri_verts)
    hit = tri >= 0
    k = np.maximum(tri, 0)
    with np.errstate(all='ignore'):
        loc = cam_loc + t[:, None] * d
        v0 = tri_verts[k, 0]
        e1, e2 = tri_verts[k, 1] - v0, tri_verts[k, 2] - v0
        c = R.cross(e1, e2)
        n = c / np.sqrt(R.dot(c, c))[:, None]
        p = R.cross(d, e2)
        inv = 1.0 / R.dot(e1, p)
        s = cam_loc - v0
        u = R.dot(s, p) * inv
        q = R.cross(s, e1)
        v = R.dot(d, q) * inv
        w = (1.0 - u) - v
        if tri_normals is not None:
            m = blend(np.asarray(tri_normals, np.float64)[k], w, u, v)
            lm = np.sqrt(R.dot(m, m))
            ok = np.isfinite(lm) & (lm > 0.0)
            n = np.where(ok[:, None], m / lm[:, None], n)
        wo, _ = R.unit_towards(loc, cam_loc)
        co = R.dot(n, wo)
        flipped = hit & (co < 0.0)
        n = np.where(flipped[:, None], -n, n)
        co = np.where(flipped, -co, co)
        kdv = blend(np.asarray(tri_rgb, np.float64)[k], w, u, v) if tri_rgb is not None else \
            np.broadcast_to(np.asarray(kd, np.float64), loc.shape)
        wl = light - loc
        r2 = R.dot(wl, wl)
        wi = wl / np.sqrt(r2)[:, None]
        ci = R.dot(n, wi)
        facing = hit & (ci > 0.0)
        occ = R.shadow(tri_verts, np.where(facing[:, None], loc, 0.0), facing.astype(np.uint8), light) > 0
        lit = facing & ~occ
        a2 = alpha * alpha
        hv = wi + wo
        h = hv / np.sqrt(R.dot(hv, hv))[:, None]
        nh, vh = R.dot(n, h), R.dot(wo, h)
        dd = (nh * nh) * (a2 - 1.0) + 1.0
        D = a2 / (PI * (dd * dd))
        m1 = 1.0 - vh
        m2 = m1 * m1
        m5 = (m2 * m2) * m1
        F = ks + (1.0 - ks) * m5
        spec = (((D * g1(ci, a2)) * g1(co, a2)) * F) / ((4.0 * ci) * co)
        spec = np.where(co > 0.0, spec, 0.0)
        e = (intensity / r2) * ci
        rad = e[:, None] * (kdv / PI + spec[:, None])
    return dict(radiance=np.where(lit[:, None], rad, 0.0), hit=hit, flipped=flipped, facing=facing, shadowed=facing & occ, lit=lit,
                spec=np.where(lit, spec, 0.0))


def render(tri_verts, cam_mat_inv, cam_loc, imh, imw, spp_side, light, intensity=1.0, kd=(0.8, 0.8, 0.8), ks=0.04, alpha=0.5,
           tri_normals=None, tri_rgb=None):
    """-> dict(rgb float32 [P,3], coverage float32 [P]; per pixel the counts over its samples: hits, flipped, shadowed, lit,
    spec_lit (lit samples with spec != 0))."""
    xs, ys = np.meshgrid(np.arange(imw, dtype=np.float64), np.arange(imh, dtype=np.float64))
    x, y = xs.reshape(-1), ys.reshape(-1)
    S = int(spp_side)
    acc = np.zeros((x.size, 3))
    counts = {k: np.zeros(x.size, np.int64) for k in ('hits', 'flipped', 'shadowed', 'lit', 'spec_lit')}
    for j in range(S):
        py = y + ((2 * j + 1) / float(2 * S) - 0.5)
        for i in range(S):
            px = x + ((2 * i + 1) / float(2 * S) - 0.5)
            s = shade_sample(tri_verts, cam_mat_inv, cam_loc, px, py, light, intensity, kd, ks, alpha, tri_normals, tri_rgb)
            acc = acc + s['radiance']
            counts['hits'] += s['hit']; counts['flipped'] += s['flipped']; counts['shadowed'] += s['shadowed']
            counts['lit'] += s['lit']; counts['spec_lit'] += s['lit'] & (s['spec'] != 0.0)
    n = float(S * S)
    out = dict(rgb=(acc / n).astype(np.float32), coverage=(counts['hits'].astype(np.float64) / n).astype(np.float32))
    out.update(counts)
    return out
