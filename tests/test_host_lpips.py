"""CPU: the host side of the LPIPS loss and metric -- the weights loader on `.npz` and on `.pb` graphs written by the encoder
below, the model wiring, the refusals, the dynamic-range rules and the argument checks of the C entry points."""
import struct

import numpy as np
import pytest

import nlt_amd
from nlt_amd import capi as C
from nlt_amd import losses, lpips_weights, metric
from nlt_amd.models import get_model_class
import lpips_ref as R

W = R.random_weights(3)


# ---------------------------------------------------------------------------------------- a test-side GraphDef encoder
def _varint(n):
    out = bytearray()
    n &= (1 << 64) - 1
    while n > 0x7f:
        out.append((n & 0x7f) | 0x80)
        n >>= 7
    out.append(n)
    return bytes(out)


def _vi(field, v):
    return _varint(field << 3) + _varint(v)


def _ld(field, b):
    return _varint(field << 3 | 2) + _varint(len(b)) + bytes(b)


def _tensor_proto(a, payload):
    a = np.asarray(a)
    dt = {'f': 1, 'i': 3}[a.dtype.kind]
    shape = b''.join(_ld(2, _vi(1, d)) for d in a.shape)
    out = _vi(1, dt) + _ld(2, shape)
    if dt == 3:
        return out + _ld(7, b''.join(_varint(int(v)) for v in a.reshape(-1)))           # int_val, packed
    flat = a.astype('<f4').reshape(-1)
    if payload == 'content':
        return out + _ld(4, flat.tobytes())
    if payload == 'packed':
        return out + _ld(5, flat.tobytes())
    if payload == 'fixed32':
        return out + b''.join(_varint(5 << 3 | 5) + struct.pack('<f', v) for v in flat)
    raise ValueError(payload)


def _const(name, a, payload='content'):
    a = np.asarray(a)
    attrs = _ld(5, _ld(1, b'dtype') + _ld(2, _vi(6, 1 if a.dtype.kind == 'f' else 3)))
    attrs += _ld(5, _ld(1, b'value') + _ld(2, _ld(8, _tensor_proto(a, payload))))
    return _ld(1, _ld(1, name.encode()) + _ld(2, b'Const') + attrs)


def _op(name, op, inputs):
    return _ld(1, _ld(1, name.encode()) + _ld(2, op.encode()) + b''.join(_ld(3, i.encode()) for i in inputs))


def graphdef(w, layout='OIHW', payload='content', drop=None):
    """A frozen graph holding the network's constants in graph order, with decoys between them."""
    nodes = [_op('0', 'Placeholder', []), _const('perm', np.array([0, 3, 1, 2], np.int32)), _const('two', np.float32(2.0), 'packed')]
    small = 'fixed32' if payload == 'packed' else 'packed'
    nodes += [_const('shift', np.asarray(R.SHIFT, np.float32).reshape(1, 3, 1, 1), small),
              _const('scale', np.asarray(R.SCALE, np.float32).reshape(1, 3, 1, 1), small)]
    for l in range(1, 6):
        k = w['conv%d_weight' % l]
        if layout == 'HWIO':
            k = np.transpose(k, (2, 3, 1, 0))
        if drop != 'conv%d_weight' % l:
            nodes.append(_const('features.%d.weight' % l, k, payload))
        if drop != 'conv%d_bias' % l:
            nodes.append(_const('features.%d.bias' % l, w['conv%d_bias' % l], payload))
        nodes += [_op('conv%d' % l, 'Conv2D', ['x', 'features.%d.weight' % l]), _const('eps%d' % l, np.float32(1e-10), 'fixed32')]
    for l in range(1, 6):
        lin = w['lin%d' % l]
        lin = lin.reshape(1, -1, 1, 1) if layout == 'OIHW' else lin.reshape(1, 1, -1, 1)
        if drop != 'lin%d' % l:
            nodes.append(_const('lin%d.model.1.weight' % l, lin, payload))
    nodes.append(_const('shape', np.array([-1, 1, 1, 1], np.int32)))
    return b''.join(nodes)


# ---------------------------------------------------------------------------------------- the loader
def _same(got, w):
    assert sorted(got) == sorted(list(w) + ['shift', 'scale'])
    for k, v in w.items():
        assert got[k].dtype == np.float32 and np.array_equal(got[k], v.reshape(got[k].shape)), k
    assert np.array_equal(got['shift'], np.float32(R.SHIFT)) and np.array_equal(got['scale'], np.float32(R.SCALE))


def test_npz_round_trip_defaults_and_readable_errors(tmp_path):
    p = str(tmp_path / 'w.npz')
    np.savez(p, **W)
    _same(lpips_weights.load(p), W)
    np.savez(p, **dict(W, lin3=W['lin3'].reshape(1, -1, 1, 1), shift=np.float32([-.1, -.2, -.3])))
    got = lpips_weights.load(p)
    assert got['lin3'].shape == (384,) and np.array_equal(got['shift'], np.float32([-.1, -.2, -.3]))
    bad = dict(W)
    del bad['conv4_bias']
    np.savez(p, **bad)
    with pytest.raises(ValueError, match="conv4_bias.*missing"):
        lpips_weights.load(p)
    np.savez(p, **dict(W, conv2_weight=W['conv2_weight'][:, :, :3]))
    with pytest.raises(ValueError, match="conv2_weight.*shape"):
        lpips_weights.load(p)
    nan = W['conv1_bias'].copy()
    nan[5] = np.nan
    np.savez(p, **dict(W, conv1_bias=nan))
    with pytest.raises(ValueError, match="conv1_bias.*non-finite"):
        lpips_weights.load(p)
    np.savez(p, **dict(W, extra=np.zeros(3, np.float32)))
    with pytest.raises(ValueError, match="unexpected"):
        lpips_weights.load(p)
    with pytest.raises(ValueError, match="npz"):
        lpips_weights.load(str(tmp_path / 'w.txt'))
    with pytest.raises(OSError):
        lpips_weights.load(str(tmp_path / 'absent.npz'))


@pytest.mark.parametrize('layout', ['OIHW', 'HWIO'])
@pytest.mark.parametrize('payload', ['content', 'packed'])
def test_pb_reader_on_encoded_graphs(tmp_path, layout, payload):
    p = str(tmp_path / 'net.pb')
    with open(p, 'wb') as f:
        f.write(graphdef(W, layout, payload))
    _same(lpips_weights.load(p), W)
    names = [n for n, _ in lpips_weights.float_consts(graphdef(W, layout, payload))]
    assert 'perm' not in names and 'shape' not in names and 'two' in names and names.index('shift') < names.index('features.1.weight')


@pytest.mark.parametrize('drop', ['conv3_weight', 'conv5_bias', 'lin2'])
def test_pb_reader_raises_when_a_tensor_is_missing(drop):
    with pytest.raises(ValueError, match='expected'):
        lpips_weights.from_graphdef(graphdef(W, drop=drop))


def test_pb_reader_raises_on_a_second_affine_candidate_and_a_short_payload():
    extra = _const('mean', np.float32([.1, -.2, .3]).reshape(1, 3, 1, 1))
    with pytest.raises(ValueError, match='shift'):
        lpips_weights.from_graphdef(graphdef(W) + extra)
    short = _ld(1, _ld(1, b'k') + _ld(2, b'Const') + _ld(5, _ld(1, b'value') + _ld(2, _ld(8,
                _vi(1, 1) + _ld(2, _ld(2, _vi(1, 4))) + _ld(4, np.zeros(3, '<f4').tobytes())))))
    with pytest.raises(ValueError, match='holds 3 values'):
        lpips_weights.float_consts(short)


def test_blob_layout_is_the_library_s():
    assert lpips_weights.blob_floats() == C.lib().nlt_lpips_weights_floats() == 2470856
    b = lpips_weights.blob(lpips_weights.validate(W))
    off = lpips_weights.blob_offsets()
    assert all(o % 4 == 0 for name, (o, _) in off.items() if name != 'scale')
    assert np.array_equal(b[:3], np.float32(R.SHIFT)) and np.array_equal(b[3:6], np.float32(R.SCALE))
    for l in range(1, 6):
        o, shape = off['conv%d_weight' % l]
        assert np.array_equal(b[o:o + int(np.prod(shape))].reshape(shape), R.keras(W, l))
        o, shape = off['conv%d_bias' % l]
        assert np.array_equal(b[o:o + shape[0]], W['conv%d_bias' % l])
        o, shape = off['lin%d' % l]
        assert np.array_equal(b[o:o + shape[0]], W['lin%d' % l])
    assert off['lin5'][0] + 256 == b.size


# ---------------------------------------------------------------------------------------- model wiring and refusals
def _model(loss, **kw):
    return get_model_class('nlt')(nlt_amd.make_config(depth=256, uvh=64, uvw=64, imh=32, imw=32, loss=loss, **kw))


def test_released_loss_string_parses_with_a_weights_file(tmp_path, monkeypatch):
    monkeypatch.delenv(lpips_weights.ENV, raising=False)
    p = str(tmp_path / 'w.npz')
    np.savez(p, **W)
    pm = _model('barron,1e+0lpips', lpips_weights=p)
    assert [(w, type(f)) for w, f in pm.wloss] == [(1.0, losses.Barron), (1.0, losses.LPIPS)]
    assert pm.wloss[1][1].per_ch is False
    _same(pm.wloss[1][1].arrays, W)
    monkeypatch.setenv(lpips_weights.ENV, p)                     # the environment variable serves when the key is absent
    assert [(w, type(f)) for w, f in _model('0.5lpips,l2').wloss] == [(0.5, losses.LPIPS), (1.0, losses.L2)]


def test_refusals(tmp_path, monkeypatch):
    monkeypatch.delenv(lpips_weights.ENV, raising=False)
    with pytest.raises(NotImplementedError, match='lpips_weights'):
        _model('barron,1e+0lpips')
    with pytest.raises(NotImplementedError):
        _model('l1')
    with pytest.raises(NotImplementedError, match='per_ch'):
        losses.LPIPS(W, per_ch=True)
    with pytest.raises(NotImplementedError, match='NLT_LPIPS_WEIGHTS'):
        metric.LPIPS(np.float32)
    bad = str(tmp_path / 'bad.npz')
    np.savez(bad, conv1_weight=np.zeros(3, np.float32))
    with pytest.raises(ValueError):                              # validated when the model is constructed, not at the first step
        _model('lpips', lpips_weights=bad)


def test_metric_lpips_dynamic_range_rules_are_psnr_s():
    for dt in (np.float32, np.float64, 'float16', 'uint8', np.uint16):
        assert metric.LPIPS(dt, weight_pb=W).drange == metric.PSNR(dt).drange
    assert metric.LPIPS('uint8', W).drange == 255.0 and metric.LPIPS(np.uint16, W).drange == 65535.0
    for dt in (np.int32, np.int8, bool):
        with pytest.raises(NotImplementedError):
            metric.LPIPS(dt, W)


def test_metric_lpips_input_handling(monkeypatch):
    calls = []

    def lpips_loss(pred, gt, blob, want_grad):
        calls.append((tuple(pred.shape), float(pred.max()), bool(want_grad)))
        import torch
        return torch.arange(pred.shape[0], dtype=torch.float32) + 0.5, None
    monkeypatch.setattr(C, 'lpips_loss', lpips_loss)
    monkeypatch.setattr(metric, 'DEVICE', 'cpu')
    m = metric.LPIPS('uint8', W)
    x = np.full((32, 40, 3), 255, np.uint8)
    assert m(x, x) == 0.5 and calls[-1] == ((1, 32, 40, 3), 1.0, False)                  # divided by the dynamic range
    assert m(x[..., 0], x[..., 0]) == 0.5 and calls[-1][0] == (1, 32, 40, 3)             # one channel is tripled
    assert m(x[..., :1], x[..., :1]) == 0.5 and calls[-1][0] == (1, 32, 40, 3)
    assert m.batch(np.stack([x, x]), np.stack([x, x])) == [0.5, 1.5]
    with pytest.raises(AssertionError):
        m(x, x[:, :39])
    with pytest.raises(NotImplementedError):
        m(np.zeros((32, 32, 4), np.uint8), np.zeros((32, 32, 4), np.uint8))


# ---------------------------------------------------------------------------------------- the C argument checks
def test_bad_arguments_return_status_codes_without_a_gpu():
    L = C.lib()
    assert L.nlt_lpips_workspace_floats(1, 30, 64, 1) == -1 and L.nlt_lpips_workspace_floats(1, 64, 30, 0) == -1
    assert L.nlt_lpips_workspace_floats(0, 64, 64, 0) == -1
    # (1,31,31): float64 partial + accumulator, then the maps of 2 frames: f1 7x7x64, pool1 3x3x64, f2 3x3x192, pool2 1x192, f3, f4, f5
    assert L.nlt_lpips_workspace_floats(1, 31, 31, 0) == 4 + 2 * (49 * 64 + 9 * 64 + 9 * 192 + 192 + 384 + 256 + 256)
    assert L.nlt_lpips_workspace_floats(1, 31, 31, 1) == L.nlt_lpips_workspace_floats(1, 31, 31, 0) + 2 * 49 * 64
    assert L.nlt_lpips_head_workspace_floats(2, 65) == 2 * (2 * 2 + 2) and L.nlt_lpips_head_workspace_floats(0, 65) == -1
    P, n = 4096, None                                            # a non-null aligned fake pointer: checked, never dereferenced here
    need = L.nlt_lpips_workspace_floats(1, 31, 31, 1)
    assert L.nlt_lpips_loss(n, n, 1, 31, 31, n, n, 0, n, n, n) == -1
    assert L.nlt_lpips_loss(P, P, 1, 31, 31, P, P, need, n, P, n) == -1
    assert L.nlt_lpips_loss(P, P, 1, 30, 31, P, P, 1 << 30, P, P, n) == -2
    assert L.nlt_lpips_loss(P, P, 1, 31, 30, P, P, 1 << 30, P, n, n) == -2
    assert L.nlt_lpips_loss(P, P, 1, 31, 31, P, P, need - 1, P, P, n) == -1
    assert L.nlt_lpips_loss(P, P, 1, 31, 31, P, P + 4, need, P, P, n) == -1              # 16-byte aligned workspace
    assert L.nlt_lpips_conv1_forward(n, 1, 31, 31, P, P, P, P, n) == -1 and L.nlt_lpips_conv1_forward(P, 1, 10, 31, P, P, P, P, n) == -2
    assert L.nlt_lpips_conv1_backward_data(P, 1, 31, 31, P, P, n, n) == -1
    assert L.nlt_lpips_conv2_forward(P, 1, 3, 3, P, n, P, n) == -1 and L.nlt_lpips_conv2_backward_data(P, 0, 3, 3, P, P, n) == -1
    assert L.nlt_lpips_pool_forward(P, 1, 2, 7, 64, P, n) == -2 and L.nlt_lpips_pool_backward(P, n, 1, 7, 7, 64, P, n) == -1
    assert L.nlt_lpips_head_forward(P, P, 1, 9, 192, P, P, 3, P, n) == -1 and L.nlt_lpips_head_forward(P, P, 1, 9, 576, P, P, 4, P, n) == -2
    assert L.nlt_lpips_head_backward(P, P, 1, 9, 192, P, n, n, n) == -1 and L.nlt_lpips_head_backward(P, P, 1, 9, 576, P, n, P, n) == -2
