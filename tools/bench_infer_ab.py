"""The reference's inference mode (Model.call(obs_override=feat_agg), fused query-only plan) under precision = fp32 and bf16 in
ONE process: four alternated pairs of timed legs (100 steps each, tape replays, profiler off) after warm-up, the rel-L2 of `pred`
between the two plans on the same weights, and at 2048^2 the per-launch table of the bf16 leg.  Depth 256, camera 512^2.
   python tools/bench_infer_ab.py [UVxFRAMES ...] [out=FILE]      default sizes: 1024x4 1024x16 2048x2"""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nlt_amd                                                   # noqa: E402
import bench                                                     # noqa: E402
from nlt_amd import nlt_test                                     # noqa: E402
from nlt_amd.engine import OpTimer                               # noqa: E402
from nlt_amd.models import get_model_class                       # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith('out=')]
out = ([open(a[4:], 'a') for a in sys.argv[1:] if a.startswith('out=')] + [None])[0]


def say(s):
    print(s, flush=True)
    if out is not None:
        out.write(s + '\n'); out.flush()


depth, cam = 256, 512
dev = torch.device('cuda')
sizes = [(int(a), int(b)) for a, b in (s.split('x') for s in args)] or [(1024, 4), (1024, 16), (2048, 2)]
for uv, n in sizes:
    models = {}
    for prec in ('fp32', 'bf16'):
        pm = get_model_class('nlt')(nlt_amd.make_config(depth=depth, uvh=uv, uvw=uv, imh=cam, imw=cam, precision=prec)).build(dev)
        pm.register_trainable()
        models[prec] = pm
    train = [bench.synth_device_batch(n, uv, cam, 1, dev, seed=10)]
    batches = [bench.synth_device_batch(n, uv, cam, 1, dev, seed=i) for i in range(3)]
    agg = nlt_test.extract_feat(models['fp32'], train)
    # pred distance between the two plans on ONE model (same weights)
    pm = models['bf16']
    p16 = pm.call(batches[0], 'test', obs_override=agg)[3]['pred'].clone()
    pm.plan.precision = 'fp32'
    p32 = pm.call(batches[0], 'test', obs_override=agg)[3]['pred'].clone()
    pm.plan.precision = 'bf16'
    torch.cuda.synchronize()
    d = float((p16.double() - p32.double()).norm() / p32.double().norm())
    say("uv %d frames %d: pred rel-L2 bf16 plan vs fp32 plan (same weights) %.3e" % (uv, n, d))
    for prec, pm in models.items():                              # warm-up: trials, tape record, replays
        for i in range(12):
            pm.call(batches[i % 3], 'test', obs_override=agg)
    torch.cuda.synchronize()
    steps = 100
    legs = {'fp32': [], 'bf16': []}
    for pair in range(4):
        for prec in ('fp32', 'bf16'):
            pm = models[prec]
            for i in range(6):
                pm.call(batches[i % 3], 'test', obs_override=agg)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(steps):
                pm.call(batches[i % 3], 'test', obs_override=agg)
            torch.cuda.synchronize()
            legs[prec].append(1e3 * (time.perf_counter() - t0) / steps)
    for prec in legs:
        say("uv %d frames %d %s: legs ms/step %s  (min %.4f max %.4f; %.2f G texel/s at the median; ovr plan %s, replays %d)"
            % (uv, n, prec, ' '.join('%.4f' % x for x in legs[prec]), min(legs[prec]), max(legs[prec]),
               n * uv * uv / (sorted(legs[prec])[len(legs[prec]) // 2] * 1e-3) / 1e9, models[prec].plan._ovr is not None,
               models[prec].plan.tape_replays))
    m32, m16 = sorted(legs['fp32'])[2], sorted(legs['bf16'])[2]
    say("uv %d frames %d: bf16 / fp32 = %.3f (fp32 spread %.1f %%)" % (uv, n, m16 / m32, 100 * (max(legs['fp32']) - min(legs['fp32'])) / m32))
    if uv == 2048:
        pm = models['bf16']
        t = OpTimer(); pm.plan.timer = t
        for i in range(3):
            pm.call(batches[i % 3], 'test', obs_override=agg)
        rec = t.collect(); pm.plan.timer = None
        tab = sorted(((r[1] / r[0], l) for l, r in rec.items()), reverse=True)
        tot = sum(x for x, _ in tab)
        for x, l in tab:
            say("%-12s %8.4f ms %5.1f%%  %7.1f TFLOP/s  %7.1f GB/s" % (l, x, 100 * x / tot, t.flops.get(l, 0) / x / 1e9,
                                                                       t.moved.get(l, rec[l][2]) / x / 1e6))
        say("bf16 2048^2: sum of launches %.3f ms (%d launches)" % (tot, len(tab)))
    del models, batches, train, agg
    torch.cuda.empty_cache()
