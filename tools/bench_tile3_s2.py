"""The seven stride-2 encoder launches of the default workload (4 frames x 4 observations, 1024^2 UV, depth 256) on every form of
the three-term split conv that takes them, each launch alone: streaming (nlt_conv_tile3_forward), resident (nlt_conv_tile3r_forward,
where a group's weights fit LDS) and texels direct (nlt_conv_tile3d_forward, where the library has it), at 32 and 64 output channels
per workgroup.  ROUNDS alternated rounds of REPS launches per form; per line the median of the rounds and their max - min, in ms,
and the fp32-equivalent TFLOP/s of the median.  python tools/bench_tile3_s2.py [nprod]"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nlt_amd import capi as C                                    # noqa: E402

ROUNDS, REPS = 5, 20
NPROD = int(sys.argv[1]) if len(sys.argv) > 1 else 9


def timeit(fn):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / REPS


# (label, cin, cout, input resolution, frames, observations per frame)
CASES = [('L4.o.s2', 64, 128, 128, 4, 4), ('L5.o.s2', 128, 256, 64, 4, 4), ('L6.o.s2', 256, 256, 32, 4, 4),
         ('L3.q.s2', 64, 64, 256, 4, 1), ('L4.q.s2', 128, 128, 128, 4, 1), ('L5.q.s2', 256, 256, 64, 4, 1), ('L6.q.s2', 512, 256, 32, 4, 1)]
mode = C.CONV_K2S2
print("nprod %d; ms per launch: median of %d rounds of %d (max - min), fp32-equivalent TF of the median" % (NPROD, ROUNDS, REPS))
for name, cin, cout, res, frames, kobs in CASES:
    g = torch.Generator(device='cuda').manual_seed(1)
    src = torch.randn((frames * kobs, res, res, cin), device='cuda', generator=g)
    wk = torch.randn((2, 2, cin, cout), device='cuda', generator=g) * (0.5 / (cin ** 0.5))
    bias = torch.zeros(cout, device='cuda')
    out = torch.empty((frames * kobs, res // 2, res // 2, cout), device='cuda')
    flops = 2 * frames * kobs * (res // 2) ** 2 * 4 * cin * cout
    forms = {}
    for tn in (32, 64):
        if cout % tn:
            continue
        p3 = C.pack_conv_tile3_weights(mode, wk, cin, cout, tn)
        args = (mode, src, cin, cin, frames, kobs, res, res, p3, bias, cout, tn, out, cout, None, 0)
        forms['stream.%d' % tn] = (lambda a=args: C.conv_tile3_forward(*a, nprod=NPROD))
        if C.conv_tile3r_plan(mode, cin, tn) is not None:
            forms['resident.%d' % tn] = (lambda a=args: C.conv_tile3r_forward(*a, nprod=NPROD))
        if hasattr(C, 'conv_tile3d_forward'):
            forms['direct.%d' % tn] = (lambda a=args: C.conv_tile3d_forward(*a, nprod=NPROD))
        if kobs > 1:                                              # the observations as frames of their own (`lds_hints` + 256)
            unf = (mode, src, cin, cin, frames * kobs, 1) + args[6:]
            forms['stream.u.%d' % tn] = (lambda a=unf: C.conv_tile3_forward(*a, nprod=NPROD))
            if hasattr(C, 'conv_tile3d_forward'):
                forms['direct.u.%d' % tn] = (lambda a=unf: C.conv_tile3d_forward(*a, nprod=NPROD))
    for fn in forms.values():                                     # (first launches: code objects, LDS limits)
        fn()
    times = {k: [] for k in forms}
    for _ in range(ROUNDS):
        for k, fn in forms.items():
            times[k].append(timeit(fn))
    for k, ts in times.items():
        med = statistics.median(ts)
        print("%-8s %4d -> %3d %4d^2 k %d  %-12s %.4f (%.4f)  %6.1f TF" % (name, cin, cout, res, kobs, k, med, max(ts) - min(ts), flops / med / 1e9))
