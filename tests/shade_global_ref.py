"""TEST-ONLY: the float64 NumPy brute force nlt_render_global (csrc/raycast.hip) is held to, bit for bit -- the global-render
definition of include/nlt_hip.h written out operation by operation on top of tests/shade_ref.py (the camera-ray rule, `blend`,
`g1`) and tests/raycast_ref.py (`hit_distances`, `closest`, `unit_towards`): every ray against every triangle, the primary's
triangle masked out per bounce ray, the light points and bounce rays of a sample summed in k order, the samples of a pixel in
(j, i) order, one rounding to float32.  Rays that a rule leaves out (a miss, a back-facing light point, a bounce ray below the
geometric surface) are not cast; that changes no bit.  Besides the three outputs it returns, per pixel, what the non-vacuity
conditions of the tests count."""
import numpy as np

import raycast_ref as R
import shade_ref as S

PI = S.PI
COUNTS = ('hits', 'flipped', 'light_unoccluded', 'light_occluded', 'light_not_facing', 'bounce_skipped', 'bounce_missed', 'bounce_hit',
          'secondary_lit', 'secondary_shadowed', 'secondary_not_facing', 'secondary_flipped')


def cast(o, d, tri_verts, active, skip=None):
    """Closest hits of the rays (o, d)[active] -> (t [P], +inf elsewhere; tri [P], -1 elsewhere).  skip [P]: the original triangle
    index each ray passes over."""
    t = np.full(len(d), np.inf)
    tri = np.full(len(d), -1, np.int32)
    idx = np.nonzero(active)[0]
    o = np.broadcast_to(o, d.shape)
    for a in range(0, len(idx), 256):
        r = idx[a:a + 256]
        tt = R.hit_distances(np.ascontiguousarray(o[r]), d[r], tri_verts)
        if skip is not None:
            tt[np.arange(len(r)), skip[r]] = np.inf
        k = tt.argmin(1)                                            # the first minimum: ties to the lowest index
        t[r] = tt[np.arange(len(r)), k]
        tri[r] = np.where(t[r] == np.inf, -1, k)
    return t, tri


def surface(tri_verts, k, o, d, kd, tri_normals, tri_rgb):
    """ng, the shading normal (not flipped) and kd at triangle k [P] hit by the ray (o, d): shade_ref.shade_sample's operations."""
    v0 = tri_verts[k, 0]
    e1, e2 = tri_verts[k, 1] - v0, tri_verts[k, 2] - v0
    c = R.cross(e1, e2)
    ng = c / np.sqrt(R.dot(c, c))[:, None]
    p = R.cross(d, e2)
    inv = 1.0 / R.dot(e1, p)
    s = o - v0
    u = R.dot(s, p) * inv
    q = R.cross(s, e1)
    v = R.dot(d, q) * inv
    w = (1.0 - u) - v
    n = ng
    if tri_normals is not None:
        m = S.blend(np.asarray(tri_normals, np.float64)[k], w, u, v)
        lm = np.sqrt(R.dot(m, m))
        ok = np.isfinite(lm) & (lm > 0.0)
        n = np.where(ok[:, None], m / lm[:, None], ng)
    kdv = S.blend(np.asarray(tri_rgb, np.float64)[k], w, u, v) if tri_rgb is not None else \
        np.broadcast_to(np.asarray(kd, np.float64), ng.shape)
    return ng, n, kdv


def lit_from(tri_verts, light, loc, n, active):
    """-> r2, wi, ci, facing (active, ci > 0), occluded (facing, and the shadow ray from `light` does not reach loc)."""
    wl = light - loc
    r2 = R.dot(wl, wl)
    wi = wl / np.sqrt(r2)[:, None]
    ci = R.dot(n, wi)
    facing = active & (ci > 0.0)
    ds, full = R.unit_towards(light, loc)
    t, tri = cast(light, ds, tri_verts, facing)
    reach = np.abs(t - full) <= 1e-8 + 1e-5 * np.abs(full)
    return r2, wi, ci, facing, facing & (tri >= 0) & ~reach


def render(tri_verts, cam_mat_inv, cam_loc, imh, imw, spp_side, light, intensity=1.0, kd=(0.8, 0.8, 0.8), ks=0.04, alpha=0.5,
           tri_normals=None, tri_rgb=None, light_radius=0.0, light_pts=None, bounce_pts=None):
    """light_pts [n_lsets, n_l, 3] (None: one set of one point, (0, 0, 1)), bounce_pts [n_bsets, n_b, 2] or None (n_b = 0) ->
    dict(rgb, rgb_indirect float32 [P,3], coverage float32 [P], direct float64 [P,3] (D / S^2), and per pixel the COUNTS over its
    samples, light points and bounce rays)."""
    tri_verts = np.asarray(tri_verts, np.float64)
    cam_loc, light = np.asarray(cam_loc, np.float64), np.asarray(light, np.float64)
    lpts = np.array([[[0.0, 0.0, 1.0]]]) if light_pts is None else np.asarray(light_pts, np.float64)
    bpts = np.zeros((1, 0, 2)) if bounce_pts is None else np.asarray(bounce_pts, np.float64)
    n_lsets, n_l = lpts.shape[:2]
    n_bsets, n_b = bpts.shape[:2]
    xs, ys = np.meshgrid(np.arange(imw, dtype=np.float64), np.arange(imh, dtype=np.float64))
    x, y = xs.reshape(-1), ys.reshape(-1)
    P, sps = x.size, int(spp_side)
    D, I = np.zeros((P, 3)), np.zeros((P, 3))
    cnt = {k: np.zeros(P, np.int64) for k in COUNTS}
    il, nb, a2 = intensity / float(n_l), float(n_b), alpha * alpha
    with np.errstate(all='ignore'):
        for j in range(sps):
            py = y + ((2 * j + 1) / float(2 * sps) - 0.5)
            for i in range(sps):
                px = x + ((2 * i + 1) / float(2 * sps) - 0.5)
                s = j * sps + i
                d = S.sample_rays(cam_mat_inv, cam_loc, px, py)
                t, tri = cast(cam_loc, d, tri_verts, np.ones(P, bool))
                hit = tri >= 0
                k = np.maximum(tri, 0)
                loc = cam_loc + t[:, None] * d
                ng, n, kdv = surface(tri_verts, k, cam_loc, d, kd, tri_normals, tri_rgb)
                wo, _ = R.unit_towards(loc, cam_loc)
                co = R.dot(n, wo)
                flipped = hit & (co < 0.0)
                n = np.where(flipped[:, None], -n, n)
                co = np.where(flipped, -co, co)
                cnt['hits'] += hit; cnt['flipped'] += flipped
                # ---- the direct term
                a = np.zeros((P, 3))
                for kk in range(n_l):
                    L = light + light_radius * lpts[s % n_lsets, kk]
                    r2, wi, ci, facing, occ = lit_from(tri_verts, L, loc, n, hit)
                    lit = facing & ~occ
                    hv = wi + wo
                    h = hv / np.sqrt(R.dot(hv, hv))[:, None]
                    nh, vh = R.dot(n, h), R.dot(wo, h)
                    dd = (nh * nh) * (a2 - 1.0) + 1.0
                    Dg = a2 / (PI * (dd * dd))
                    m1 = 1.0 - vh
                    m2 = m1 * m1
                    m5 = (m2 * m2) * m1
                    F = ks + (1.0 - ks) * m5
                    spec = (((Dg * S.g1(ci, a2)) * S.g1(co, a2)) * F) / ((4.0 * ci) * co)
                    spec = np.where(co > 0.0, spec, 0.0)
                    e = (il / r2) * ci
                    a = a + np.where(lit[:, None], e[:, None] * (kdv / PI + spec[:, None]), 0.0)
                    cnt['light_unoccluded'] += lit; cnt['light_occluded'] += occ; cnt['light_not_facing'] += hit & ~facing
                D = D + a
                if n_b == 0:
                    continue
                # ---- the indirect term
                cg = R.dot(ng, wo)
                ngf = np.where((cg < 0.0)[:, None], -ng, ng)
                nx, ny, nz = n[:, 0], n[:, 1], n[:, 2]
                sg = np.where(nz >= 0.0, 1.0, -1.0)
                fa = -1.0 / (sg + nz)
                fb = (nx * ny) * fa
                t1 = np.stack((1.0 + (sg * (nx * nx)) * fa, sg * fb, -sg * nx), -1)
                t2 = np.stack((fb, sg + (ny * ny) * fa, -ny), -1)
                b = np.zeros((P, 3))
                for kk in range(n_b):
                    dx, dy = bpts[s % n_bsets, kk]
                    qz = (1.0 - dx * dx) - dy * dy
                    dz = np.sqrt(qz if qz > 0.0 else 0.0)
                    wv = (dx * t1 + dy * t2) + dz * n
                    wb = wv / np.sqrt(R.dot(wv, wv))[:, None]
                    go = hit & (R.dot(ngf, wb) > 0.0)
                    tb, tri2 = cast(loc, wb, tri_verts, go, skip=k)
                    hit2 = tri2 >= 0
                    k2 = np.maximum(tri2, 0)
                    loc2 = loc + tb[:, None] * wb
                    _, n2, kd2 = surface(tri_verts, k2, loc, wb, kd, tri_normals, tri_rgb)
                    fl2 = hit2 & (R.dot(n2, wb) > 0.0)
                    n2 = np.where(fl2[:, None], -n2, n2)
                    r2, wi, ci, facing, occ = lit_from(tri_verts, light, loc2, n2, hit2)
                    lit2 = facing & ~occ
                    e = (intensity / r2) * ci
                    b = b + np.where(lit2[:, None], e[:, None] * (kd2 / PI), 0.0)
                    cnt['bounce_skipped'] += hit & ~go; cnt['bounce_missed'] += go & ~hit2; cnt['bounce_hit'] += hit2
                    cnt['secondary_lit'] += lit2; cnt['secondary_shadowed'] += occ; cnt['secondary_not_facing'] += hit2 & ~facing
                    cnt['secondary_flipped'] += fl2
                I = I + np.where(hit[:, None], (kdv * b) / nb, 0.0)
        count = float(sps * sps)
        out = dict(rgb=((D + I) / count).astype(np.float32), rgb_indirect=(I / count).astype(np.float32),
                   coverage=(cnt['hits'].astype(np.float64) / count).astype(np.float32), direct=D / count)
    out.update(cnt)
    return out
