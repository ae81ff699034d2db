"""TEST-ONLY: float64 NumPy restatements of the three definitions of csrc/relight.hip (include/nlt_hip.h), as straight loops --
nothing vectorised beyond one probe row / one light at a time.  The reference of tests/test_host_relight.py,
tests/test_gpu_relight.py and tools/bench_relight.py.

Lat-long convention (z-up): pixel (i, j) of an [He, We] probe looks along (sin t cos p, sin t sin p, cos t) with
t = pi (i + 1/2) / He, p = 2 pi (j + 1/2) / We - pi, and covers dO = sin t * (pi / He) * (2 pi / We)."""
import numpy as np


def pixel_directions(he, we):
    """[he, we, 3] float64 unit vectors."""
    d = np.zeros((he, we, 3), np.float64)
    for i in range(he):
        t = np.pi * (i + 0.5) / he
        p = 2.0 * np.pi * (np.arange(we) + 0.5) / we - np.pi
        d[i, :, 0], d[i, :, 1], d[i, :, 2] = np.sin(t) * np.cos(p), np.sin(t) * np.sin(p), np.cos(t)
    return d


def solid_angles(he, we):
    """[he] float64: dO of a pixel of row i."""
    return np.array([np.sin(np.pi * (i + 0.5) / he) * (np.pi / he) * (2.0 * np.pi / we) for i in range(he)], np.float64)


def nearest_lights(he, we, dirs, rot):
    """(index [R, he, we] of the light with the largest dot product under each rotation, ties to the lowest index;
    margin [R, he, we] between the best and the second-best dot product, inf with one light)."""
    dirs, rot = np.asarray(dirs, np.float64), np.asarray(rot, np.float64)
    d = pixel_directions(he, we)
    idx = np.zeros((rot.shape[0], he, we), np.int64)
    margin = np.full((rot.shape[0], he, we), np.inf)
    for r in range(rot.shape[0]):
        for i in range(he):
            dots = (d[i] @ rot[r].T) @ dirs.T                       # [we, L]: dirs[l] . (rot[r] . d)
            idx[r, i] = np.argmax(dots, 1)                          # (first maximum: the lowest index)
            if dirs.shape[0] > 1:
                top = np.partition(dots, -2, axis=1)                # (the two largest, in order, at the end)
                margin[r, i] = top[:, -1] - top[:, -2]
    return idx, margin


def envmap_light_weights(envmap, dirs, rot, idx=None):
    """out[r, l, c] = sum over the pixels p whose nearest light under rot[r] is l of envmap[p, c] * dO(p); float64 [R, L, 3].
    idx: `nearest_lights`' answer where the caller has it already."""
    envmap = np.asarray(envmap, np.float64)
    he, we, _ = envmap.shape
    if idx is None:
        idx, _ = nearest_lights(he, we, dirs, rot)
    omega = solid_angles(he, we)
    out = np.zeros((idx.shape[0], np.asarray(dirs).shape[0], 3), np.float64)
    for r in range(idx.shape[0]):
        for i in range(he):
            for j in range(we):
                out[r, idx[r, i, j]] += envmap[i, j] * omega[i]
    return out


def srgb_decode(v):
    v = np.asarray(v, np.float64)
    return np.where(v < 0.04045, v / 12.92, ((np.maximum(v, 0.04045) + 0.055) / 1.055) ** 2.4)


def srgb_encode(v):
    v = np.asarray(v, np.float64)
    return np.where(v > 0.0031308, 1.055 * np.maximum(v, 0.0031308) ** (1.0 / 2.4) - 0.055, v * 12.92)


def relight_accumulate(acc, pred, weights, l0, is_linear):
    """acc [R, texels, 3] + sum over the chunk's lights of weights[r, l0 + l, c] * lin(clip01(pred[l])), light by light; float64."""
    acc = np.array(acc, np.float64)
    pred, weights = np.asarray(pred, np.float64), np.asarray(weights, np.float64)
    for l in range(pred.shape[0]):
        v = np.clip(pred[l], 0.0, 1.0)
        if not is_linear:
            v = srgb_decode(v)
        for r in range(weights.shape[0]):
            acc[r] += weights[r, l0 + l][None, :] * v
    return acc


def relight_finish(acc, exposure, to_srgb):
    v = np.clip(float(exposure) * np.asarray(acc, np.float64), 0.0, 1.0)
    return srgb_encode(v) if to_srgb else v


def random_rotations(n, seed):
    """[n, 3, 3] float32: the identity first, then seeded random rotations (QR of a Gaussian matrix, determinant +1)."""
    rng = np.random.default_rng(seed)
    out = [np.eye(3)]
    while len(out) < n:
        q, r = np.linalg.qr(rng.standard_normal((3, 3)))
        q = q * np.sign(np.diag(r))[None, :]
        if np.linalg.det(q) < 0:
            q[:, 0] = -q[:, 0]
        out.append(q)
    return np.stack(out[:n]).astype(np.float32)


def random_directions(n, seed):
    """[n, 3] float32 unit vectors, uniform on the sphere."""
    v = np.random.default_rng(seed).standard_normal((n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def encode_rgbe(img):
    """[H, W, 3] float -> [H, W, 4] uint8 RGBE (mantissa = floor(v * 256 / 2^e') of the largest channel's exponent e', e = e' + 128):
    decodes to mantissa * 2^(e - 136)."""
    img = np.asarray(img, np.float64)
    out = np.zeros(img.shape[:2] + (4,), np.uint8)
    for i in range(img.shape[0]):
        for j in range(img.shape[1]):
            m = img[i, j].max()
            if m < 1e-32:
                continue
            _, e = np.frexp(m)
            out[i, j, :3] = np.floor(img[i, j] * 256.0 / 2.0 ** e).astype(np.uint8)
            out[i, j, 3] = e + 128
    return out


def hdr_bytes(rgbe, rle):
    """A Radiance picture of the RGBE pixels [H, W, 4]: flat scanlines, or new-style run-length encoded ones (W >= 8)."""
    h, w, _ = rgbe.shape
    body = bytearray()
    for y in range(h):
        if not rle:
            body += rgbe[y].tobytes()
            continue
        assert 8 <= w <= 32767
        body += bytes((2, 2, w >> 8, w & 255))
        for ch in range(4):
            line, x = rgbe[y, :, ch], 0
            while x < w:
                run = 1
                while x + run < w and run < 127 and line[x + run] == line[x]:
                    run += 1
                if run >= 3:
                    body += bytes((128 + run, int(line[x])))
                    x += run
                else:
                    lit = 1
                    while x + lit < w and lit < 128 and not (x + lit + 2 < w and line[x + lit] == line[x + lit + 1] == line[x + lit + 2]):
                        lit += 1
                    body += bytes((lit,)) + line[x:x + lit].tobytes()
                    x += lit
    return b'#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n' + ('-Y %d +X %d\n' % (h, w)).encode() + bytes(body)
