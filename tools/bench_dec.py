"""Timing of the decoder tail and the fused train ends alone at the bench shape (BASELINE config 3: 4 frames, 1024^2) and at config
5's (2 frames, 2048^2): the two fused expanding blocks L10 (16 outputs, input 128^2 x (32 | 128)) and L11 (8 outputs, input 256^2 x
(16 | 64)), their inference-mode form (query half of an interleaved skip map + bias map), the last block + head (inference, training
and inference-mode forms), its backward and the front backward at k = 1.  NLT_DEC_GENERIC=1 selects the generic expanding-block
kernel, NLT_HIP_LIB=<other build> another library, for an A/B (one fresh process each)."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nlt_amd import capi as C                                    # noqa: E402
from ab_front import time_it                                     # noqa: E402


def main():
    print("lib:", C.LIB_PATH)
    g = torch.Generator(device='cuda').manual_seed(0)
    U = lambda *s: torch.rand(s, device='cuda', generator=g) - 0.5
    E = lambda *s: torch.empty(s, device='cuda')
    Z = lambda *s: torch.zeros(s, device='cuda')
    for (n, uv) in ((4, 1024), (2, 2048)):
        for c, div in ((16, 8), (8, 4)):
            h = w = uv // div
            x, skip = U(n, h, w, 2 * c), U(n, h, w, 8 * c)
            w2, b2, w1, b1 = U(2, 2, c, 10 * c), U(c), U(2, 2, c, c), U(c)
            out = torch.empty(n, 2 * h, 2 * w, c, device='cuda')
            t = time_it(lambda: C.dec_block_forward(x, 2 * c, skip, 8 * c, n, h, w, w2, b2, w1, b1, c, 0.3, out))
            flops = 2 * n * h * w * 10 * c * 4 * c + 2 * n * 4 * h * w * 4 * c * c
            moved = 4 * n * h * w * (10 * c + 4 * c)
            print("n %d uv %4d  C %2d (input %4d^2): %.4f ms   %5.1f TFLOP/s  %5.2f TB/s   checksum %.6e"
                  % (n, uv, c, h, t, flops / t / 1e9, moved / t / 1e9, float(out.double().sum())))
            w2q, bmap = U(2, 2, c, 6 * c), U(1, 2 * h, 2 * w, c)
            t = time_it(lambda: C.dec_block_forward_map(x, skip, 8 * c, n, h, w, w2q, w1, b1, c, 0.3, bmap, out))
            print("n %d uv %4d  dec_block_forward_map C %2d: %.4f ms   checksum %.6e" % (n, uv, c, t, float(out.double().sum())))
        h2 = w2_ = uv // 2
        x, fm1, skip3 = U(n, h2, w2_, 8), U(n, h2, w2_, 32), U(n, uv, uv, 3)
        ws2, bs2, ws1, bs1, wh = U(2, 2, 4, 40), U(4), U(2, 2, 4, 4), U(4), U(4, 3)
        pred, u, v = E(n, uv, uv, 3), E(n, uv, uv, 4), E(n, uv, uv, 4)
        t = time_it(lambda: C.back_forward(x, fm1, skip3, n, h2, w2_, ws2, bs2, ws1, bs1, wh, 0.3, pred))
        print("n %d uv %4d  back_forward: %.4f ms   checksum %.6e" % (n, uv, t, float(pred.double().sum())))
        ws2q, bmap = U(2, 2, 4, 24), U(1, uv, uv, 4)
        t = time_it(lambda: C.back_forward_map(x, fm1, 32, skip3, n, h2, w2_, ws2q, ws1, bs1, wh, 0.3, bmap, pred))
        print("n %d uv %4d  back_forward_map: %.4f ms   checksum %.6e" % (n, uv, t, float(pred.double().sum())))
        t = time_it(lambda: C.back_forward_train(x, fm1, skip3, n, h2, w2_, ws2, bs2, ws1, bs1, wh, 0.3, pred, u, v))
        print("n %d uv %4d  back_forward_train: %.4f ms   checksum %.6e" % (n, uv, t, float(pred.double().sum() + u.double().sum())))
        dpred, dx, dfm1 = U(n, uv, uv, 3), E(n, h2, w2_, 8), E(n, h2, w2_, 32)
        gr = [Z(m) for m in (640, 4, 64, 4, 12, 3)]
        t = time_it(lambda: C.back_backward(x, fm1, u, v, dpred, n, h2, w2_, ws2, ws1, wh, 0.3, dx, dfm1, *gr))
        print("n %d uv %4d  back_backward: %.4f ms   checksum %.6e" % (n, uv, t, float(dx.double().sum() + dfm1.double().sum())))
        base, cvis, lvis, nn_rgb, nn_base = U(n, uv, uv, 3), U(n, uv, uv, 1), U(n, uv, uv, 1), U(n, 1, uv, uv, 3), U(n, 1, uv, uv, 3)
        dy1q, dy1o = U(n, h2, w2_, 16), U(n, 1, h2, w2_, 16)
        wts = (U(1, 1, 5, 16), U(16), U(1, 1, 3, 16), U(16), U(2, 2, 32, 16), U(2, 2, 16, 16), U(1, 1, 36, 3))
        gr = [Z(m) for m in (80, 16, 48, 16, 2048, 16, 1024, 16, 108)]
        t = time_it(lambda: C.front_backward(base, cvis, lvis, nn_rgb, nn_base, n, 1, uv, uv, dy1q, dy1o, dpred, wts, gr))
        print("n %d uv %4d  front_backward k 1: %.4f ms" % (n, uv, t))
        del x, fm1, skip3, pred, u, v, dpred, dx, dfm1, base, cvis, lvis, nn_rgb, nn_base, dy1q, dy1o
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
