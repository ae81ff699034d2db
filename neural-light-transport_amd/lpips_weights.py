"""Weights of the LPIPS v0.1 "alex / lin" network (csrc/lpips.hip) -- host only: parsing, validation and the packed blob.

The reference names `third_party/lpips/net-lin_alex_v0.1.pb` (nlt/losses.py:121-135), a frozen TensorFlow graph that is not
part of its tree (.MISSING_LARGE_BLOBS), so no weights are bundled here either.  A user who has that file, or the same weights
from the published PyTorch package saved as an `.npz`, points the config key `lpips_weights` (not a reference key) or the
environment variable NLT_LPIPS_WEIGHTS at it.

`.npz`: the published PyTorch layout -- conv{1..5}_weight (O,I,kh,kw), conv{1..5}_bias (O,), lin{1..5} (C,) (any shape with
that many elements), optional shift / scale (3,).

`.pb`  STATUS: the GraphDef reader is RESTATED from the published protobuf definitions (graph.proto, node_def.proto,
attr_value.proto, tensor.proto) on ckpt.py's field walker and is NOT PINNED: no real `net-lin_alex_v0.1.pb` has ever been read
by it; it is exercised only against graphs written by the test-side encoder of tests/test_host_lpips.py.  It collects every
float Const tensor in graph order and identifies them by shape alone; if that does not give exactly the expected set it
raises and never guesses further.  Parity of csrc/lpips.hip with a real TF LPIPS graph is equally unpinned (tests/lpips_ref.py
restates the published definition).
"""
import os
import struct

import numpy as np

from .ckpt import _proto

CHANNELS = (3, 64, 192, 384, 256, 256)
KERNELS = (11, 5, 3, 3, 3)
SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)
ENV = 'NLT_LPIPS_WEIGHTS'
KEY = 'lpips_weights'


def conv_shape(l):
    """(O, I, kh, kw) of conv l = 1..5."""
    return (CHANNELS[l], CHANNELS[l - 1], KERNELS[l - 1], KERNELS[l - 1])


def configured_path(config=None):
    """The weights file the config key `lpips_weights` or, failing that, NLT_LPIPS_WEIGHTS names; None when neither is set."""
    path = None
    if config is not None:
        path = config.get('DEFAULT', KEY, fallback=None)
    path = path or os.environ.get(ENV)
    return path if path and path.strip() and path.strip() != 'None' else None


def validate(w, source='weights'):
    """-> {name: contiguous float32 array} with exactly the expected names and shapes (lin flattened; shift / scale defaulted);
    ValueError naming the array otherwise."""
    out = {}
    w = dict(w)
    for l in range(1, 6):
        for name, shape in (('conv%d_weight' % l, conv_shape(l)), ('conv%d_bias' % l, (CHANNELS[l],)), ('lin%d' % l, (CHANNELS[l],))):
            if name not in w:
                raise ValueError("%s: array '%s' is missing" % (source, name))
            a = np.asarray(w.pop(name))
            if name.startswith('lin'):
                if a.size != shape[0]:
                    raise ValueError("%s: '%s' has %d elements, expected %d" % (source, name, a.size, shape[0]))
                a = a.reshape(shape)
            if tuple(a.shape) != shape:
                raise ValueError("%s: '%s' has shape %s, expected %s" % (source, name, tuple(a.shape), shape))
            out[name] = a
    for name, default in (('shift', SHIFT), ('scale', SCALE)):
        a = np.asarray(w.pop(name, default))
        if a.size != 3:
            raise ValueError("%s: '%s' has %d elements, expected 3" % (source, name, a.size))
        out[name] = a.reshape(3)
    if w:
        raise ValueError("%s: unexpected arrays %s" % (source, sorted(w)))
    for name, a in out.items():
        if a.dtype.kind != 'f':
            raise ValueError("%s: '%s' is %s, expected a float array" % (source, name, a.dtype))
        if not np.isfinite(a).all():
            raise ValueError("%s: '%s' holds non-finite values" % (source, name))
        out[name] = np.ascontiguousarray(a, dtype=np.float32)
    if not (out['scale'] > 0).all():
        raise ValueError("%s: 'scale' must be positive" % source)
    return out


def load(path):
    """The validated arrays of an `.npz` or `.pb` file; a readable ValueError / OSError otherwise."""
    ext = os.path.splitext(path)[1].lower()
    if ext == '.npz':
        with np.load(path, allow_pickle=False) as z:
            return validate({k: z[k] for k in z.files}, path)
    if ext == '.pb':
        with open(path, 'rb') as f:
            return validate(from_graphdef(f.read(), path), path)
    raise ValueError("%s: LPIPS weights come as .npz (published PyTorch layout) or .pb (frozen TF graph)" % path)


# ------------------------------------------------------------------------------------------------------------ GraphDef
def _tensor(buf):
    """TensorProto -> float32 array, or None when it is not DT_FLOAT."""
    m = _proto(buf)
    if m.get(1, [0])[0] != 1:                                   # DT_FLOAT
        return None
    shape = []
    for sh in m.get(2, []):                                     # TensorShapeProto
        for dim in _proto(sh).get(2, []):
            shape.append(_proto(dim).get(1, [0])[0])
    count = int(np.prod(shape, dtype=np.int64)) if shape else 1
    if 4 in m:                                                  # tensor_content: raw little-endian bytes
        a = np.frombuffer(m[4][0], dtype='<f4')
    else:                                                       # float_val: packed (bytes) or one fixed32 per value
        vals = []
        for v in m.get(5, []):
            if isinstance(v, bytes):
                vals.extend(np.frombuffer(v, dtype='<f4').tolist())
            else:
                vals.append(struct.unpack('<f', struct.pack('<I', v))[0])
        a = np.asarray(vals, dtype=np.float32)
        if a.size == 1 and count > 1:                           # one value stands for all of them
            a = np.full(count, a[0], dtype=np.float32)
    if a.size != count:
        raise ValueError("Const tensor of shape %s holds %d values" % (tuple(shape), a.size))
    return a.astype(np.float32).reshape(shape)


def float_consts(buf):
    """Every float Const tensor of a serialized GraphDef, in graph order: [(node name, array)]."""
    out = []
    for node in _proto(buf).get(1, []):                         # GraphDef.node
        m = _proto(node)
        if m.get(2, [b''])[0] != b'Const':
            continue
        for entry in m.get(5, []):                              # NodeDef.attr: map<string, AttrValue>
            e = _proto(entry)
            if e.get(1, [b''])[0] != b'value':
                continue
            for t in _proto(e[2][0]).get(8, []):                # AttrValue.tensor
                a = _tensor(t)
                if a is not None:
                    out.append((m.get(1, [b''])[0].decode('utf-8', 'replace'), a))
    return out


def from_graphdef(buf, source='graph'):
    """The arrays of `validate`'s input from a frozen graph, identified by shape (module docstring).  Conv kernels come OIHW or
    HWIO (unambiguous at these shapes); graph order breaks the 256 / 256 ties; shift is the all-negative (1,3,1,1)-like tensor,
    scale the all-positive one."""
    convs, biases, lins, affine = [], [], [], []
    oihw = {conv_shape(l): l for l in range(1, 6)}
    hwio = {(s[2], s[3], s[1], s[0]): l for s, l in oihw.items()}
    for name, a in float_consts(buf):
        shape = tuple(a.shape)
        if shape in oihw:
            convs.append((shape[0], a))
        elif shape in hwio:
            convs.append((shape[3], np.transpose(a, (3, 2, 0, 1))))
        elif a.ndim == 1 and a.size in CHANNELS[1:]:
            biases.append(a)
        elif a.ndim >= 2 and a.size == 3 and max(shape) == 3:
            affine.append(a.reshape(3))
        elif a.ndim >= 2 and a.size in CHANNELS[1:] and max(shape) == a.size:
            lins.append(a.reshape(-1))
        # anything else (scalars, other shapes) is not part of the network's parameters
    want = list(CHANNELS[1:])
    for what, got in (('conv kernels', [c for c, _ in convs]), ('biases', [b.size for b in biases]), ('lin tensors', [x.size for x in lins])):
        if got != want:
            raise ValueError("%s: expected %s with %s channels in graph order, found %s" % (source, what, want, got))
    neg = [a for a in affine if (a < 0).all()]
    pos = [a for a in affine if (a > 0).all()]
    if len(affine) != 2 or len(neg) != 1 or len(pos) != 1:
        raise ValueError("%s: expected one all-negative shift and one all-positive scale tensor of 3 values, found %d candidates"
                         % (source, len(affine)))
    out = {'shift': neg[0], 'scale': pos[0]}
    for l in range(1, 6):
        out['conv%d_weight' % l] = convs[l - 1][1]
        out['conv%d_bias' % l] = biases[l - 1]
        out['lin%d' % l] = lins[l - 1]
    return out


# ------------------------------------------------------------------------------------------------------------ the blob
def blob_floats():
    """Length of the packed blob: what nlt_lpips_weights_floats() answers."""
    n = 8
    for l in range(1, 6):
        n += int(np.prod(conv_shape(l))) + 2 * CHANNELS[l]
    return n


def blob(w):
    """Validated arrays -> the float32 blob nlt_lpips_loss reads (include/nlt_hip.h): shift, scale, 2 unused, then each conv's
    Keras array (kh,kw,I,O) and bias, then lin1 .. lin5."""
    parts = [w['shift'], w['scale'], np.zeros(2, np.float32)]
    for l in range(1, 6):
        parts += [np.transpose(w['conv%d_weight' % l], (2, 3, 1, 0)).reshape(-1), w['conv%d_bias' % l]]
    parts += [w['lin%d' % l] for l in range(1, 6)]
    out = np.ascontiguousarray(np.concatenate([np.asarray(p, np.float32).reshape(-1) for p in parts]))
    assert out.size == blob_floats()
    return out


def blob_offsets():
    """{name: (offset, Keras shape)} of the arrays inside the blob (the layer-level entry points take them one by one)."""
    out, at = {'shift': (0, (3,)), 'scale': (3, (3,))}, 8
    for l in range(1, 6):
        o, i, kh, kw = conv_shape(l)
        out['conv%d_weight' % l] = (at, (kh, kw, i, o)); at += o * i * kh * kw
        out['conv%d_bias' % l] = (at, (o,)); at += o
    for l in range(1, 6):
        out['lin%d' % l] = (at, (CHANNELS[l],)); at += CHANNELS[l]
    return out
