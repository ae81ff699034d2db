"""The capture writer at the released data-generation shape: python tools/bench_capture.py [--im 512] [--uvs 1024] [--frames 64]
[--rounds 7] [--passes 200] [--out DIR]

Three comparisons, the two forms of each alternated round by round in one process, every shape warmed first, device events
around a synchronised window (host clock for the file writes):
  sample   per-sample device work: the two fused launches (capture_camspc, capture_uvspc) against the same buffers through the
           adapters that were there before them (two cosine_map, three remap_bilinear, the torch masking / clip / casts)
  diffuse  diffuse bases of `frames` frames: diffuse_bases (one launch) against compute_diffuse_bases (one launch + a Python
           loop of `frames` remaps)
  write    write_sample of one sample (device -> host copies + PNG / .npy encode): thread pool against one thread; with the
           share of a sample's wall time (fused device work + write) the host side takes
The outputs of the two forms are compared bit for bit before anything is timed.  Prints medians and spreads (max - min over the
rounds) and one JSON line."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nlt_amd                                                    # noqa: E402,F401
from nlt_amd import _capi as C                                    # noqa: E402
from nlt_amd.data_gen import postproc, render                     # noqa: E402


def inputs(im, uvs, frames, dev='cuda'):
    g = torch.Generator(device=dev).manual_seed(im + uvs)
    R = lambda *s: torch.rand(s, device=dev, generator=g, dtype=torch.float64)
    U = lambda *s: torch.randint(0, 256, s, device=dev, generator=g, dtype=torch.uint8)
    p = im * im
    unit = lambda *s: R(*s) * 1.1 - 0.05
    cam2uv = unit(uvs, uvs, 2) * (R(uvs, uvs, 1) > 0.3)           # 30 % background texels, as an unwrapped subject leaves
    return dict(locs=R(p, 3) * 4 - 2, normals=R(p, 3) * 2 - 1, valid=(R(p) > 0.2).to(torch.uint8), occluded=(R(p) < 0.3).to(torch.uint8),
                alpha=torch.where(R(im, im) > 0.2, 255, 0).to(torch.uint8), uv2cam=unit(im, im, 2), cam2uv=cam2uv.contiguous(),
                rgba=U(im, im, 4), cam=(0.3, -2.5, 1.0), light=(-1.0, 0.5, 2.0),
                albedo=R(uvs, uvs, 3), lvis=U(frames, uvs, uvs), uv2cam_f16=unit(frames, im, im, 2).to(torch.float16))


def sample_fused(x):
    cvis_c, lvis_c, u16, upng = C.capture_camspc(x['locs'], x['normals'], x['valid'], x['occluded'], x['cam'], x['light'], x['alpha'], x['uv2cam'])
    cvis, lvis, rgb, c16, cpng = C.capture_uvspc(x['cam2uv'], cvis_c, lvis_c, x['rgba'])
    return cvis_c, lvis_c, u16, upng, cvis, lvis, rgb, c16, cpng


def _map_files(m):
    png = torch.cat(((m.clamp(0, 1) * 255).to(torch.uint8), torch.zeros_like(m[:, :, :1], dtype=torch.uint8)), 2)
    return m.to(torch.float16), png


def sample_separate(x):
    _, cvis_c = C.cosine_map(x['locs'], x['normals'], x['valid'], None, x['cam'], want_float=False)
    _, lvis_c = C.cosine_map(x['locs'], x['normals'], x['valid'], x['occluded'], x['light'], want_float=False)
    im = x['alpha'].shape
    cvis_c, lvis_c = cvis_c.view(im), lvis_c.view(im)
    masked = torch.where((x['alpha'] < 255).unsqueeze(-1), torch.zeros_like(x['uv2cam']), x['uv2cam'])
    u16, upng = _map_files(masked)
    c16, cpng = _map_files(x['cam2uv'])
    cvis, lvis = C.remap_bilinear(cvis_c, x['cam2uv']), C.remap_bilinear(lvis_c, x['cam2uv'])
    rgb = C.remap_bilinear(x['rgba'][:, :, :3].contiguous(), x['cam2uv'])
    return cvis_c, lvis_c, u16, upng, cvis, lvis, rgb, c16, cpng


def diffuse_fused(x):
    return C.diffuse_bases(x['albedo'], x['lvis'], x['uv2cam_f16'])


def diffuse_separate(x):
    d, cam = postproc.compute_diffuse_bases(x['albedo'], x['lvis'], x['uv2cam_f16'])
    return d, torch.stack(cam)


def same(a, b, what):
    for i, (s, t) in enumerate(zip(a, b)):
        if s.dtype == torch.float16:                              # the separate form casts with torch, whose float64 -> float16
            n = int((s.view(torch.int16) != t.view(torch.int16)).sum())          # is not the contract (NumPy's single rounding is)
            if n:
                print("%s: output %d: torch's float64 -> float16 cast differs from the fused launch in %d of %d elements" % (what, i, n, s.numel()))
        elif not torch.equal(s, t):
            raise SystemExit("%s: output %d of the two forms differs" % (what, i))


def alternate(forms, rounds, window):
    """{name: [seconds or ms per round]}: `window(fn)` measures one form; the order rotates every round."""
    names, out = list(forms), {k: [] for k in forms}
    for r in range(rounds):
        s = r % len(names)
        for k in names[s:] + names[:s]:
            out[k].append(window(forms[k]))
    return out


def device_ms(passes):
    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(passes):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / passes
    return window


def report(title, ms, unit='ms'):
    rec = {}
    for k, v in ms.items():
        rec[k] = {'median': statistics.median(v), 'spread': max(v) - min(v)}
        print("%-8s %-10s %10.4f %s  (spread %.4f over %d rounds)" % (title, k, rec[k]['median'], unit, rec[k]['spread'], len(v)))
    return rec


def bench(im, uvs, frames, rounds, passes, out_dir):
    if not torch.cuda.is_available():
        raise SystemExit("bench_capture needs the GPU: nothing here is timed without one")
    x = inputs(im, uvs, frames)
    same(sample_fused(x), sample_separate(x), 'sample')
    same(diffuse_fused(x), diffuse_separate(x), 'diffuse')
    for fn in (sample_fused, sample_separate, diffuse_fused, diffuse_separate):   # every shape warmed
        fn(x); fn(x)
    torch.cuda.synchronize()
    out = {'im': im, 'uvs': uvs, 'frames': frames, 'rounds': rounds, 'passes': passes}
    out['sample_ms'] = report('sample', alternate({'fused': lambda: sample_fused(x), 'separate': lambda: sample_separate(x)},
                                                  rounds, device_ms(passes)))
    out['diffuse_ms'] = report('diffuse', alternate({'fused': lambda: diffuse_fused(x), 'separate': lambda: diffuse_separate(x)},
                                                    rounds, device_ms(max(1, passes // 10))))
    # the files of one sample: the device tensors are there already; the clock runs over the copies and the encodes
    f = sample_fused(x)
    sample = {'cvis_camspc.png': f[0], 'lvis_camspc.png': f[1], 'uv2cam.npy': f[2], 'uv2cam.png': f[3], 'cvis.png': f[4], 'lvis.png': f[5],
              'rgb.png': f[6], 'cam2uv.npy': f[7], 'cam2uv.png': f[8], 'rgb_camspc.png': x['rgba'], 'alpha.png': x['alpha'], '_uv2cam': None,
              '_alpha': None}
    cam, light, nn = {'name': 'P01', 'position': list(x['cam'])}, {'name': 'L1', 'position': list(x['light'])}, {'cam': 'P02', 'light': 'L2'}
    with tempfile.TemporaryDirectory(dir=out_dir) as tmp:
        def write(workers):
            def run():
                t0 = time.perf_counter()
                render.write_sample(os.path.join(tmp, 's'), sample, cam, light, nn, workers=workers)
                return (time.perf_counter() - t0) * 1e3
            return run
        write(None)(); write(1)()
        out['write_ms'] = report('write', alternate({'pool': write(None), 'one_thread': write(1)}, rounds, lambda fn: fn()))
    dev, host = out['sample_ms']['fused']['median'], out['write_ms']['pool']['median']
    out['host_share_of_a_sample'] = host / (host + dev)
    print("host share of a sample's wall time (pool write / (pool write + fused device work)): %.4f" % out['host_share_of_a_sample'])
    return out


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--im', type=int, default=512)
    ap.add_argument('--uvs', type=int, default=1024)
    ap.add_argument('--frames', type=int, default=64)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--passes', type=int, default=200)
    ap.add_argument('--out', default=None, help="directory the temporary sample files go under (default: the system's)")
    a = ap.parse_args()
    print(json.dumps(bench(a.im, a.uvs, a.frames, a.rounds, a.passes, a.out)))
