"""Reading and writing the reference's TensorFlow checkpoints (`ckpt-N.index` + `ckpt-N.data-00000-of-00001`) without TensorFlow.

The reference saves `tf.train.Checkpoint(step=..., optimizer=..., net=model)` (nlt/trainvali.py:134-141) and restores
`tf.train.Checkpoint(net=model)` for inference (nlt/nlt_test.py:68-73); the model's trainable layers are reachable as
`net_{query,obs}_layer{i}` attributes (nlt/models/base.py:79-101), so the variables are stored under
    net/net_query_layer0/kernel/.ATTRIBUTES/VARIABLE_VALUE                        (plain Conv2D: L0, head)
    net/net_query_layer3/layer_with_weights-1/bias/.ATTRIBUTES/VARIABLE_VALUE      (Keras Sequential blocks)
This module parses the on-disk "tensor bundle" format -- an SSTable index in TensorFlow's copy of the LevelDB table
format whose values are BundleEntryProto messages, plus raw little-endian tensor bytes in the data shard(s) -- and
maps those keys onto `Model.load_weights`' structure (Keras array layouts are kept as they are).

STATUS: format restated from the published layouts (tensorflow/core/lib/io/table_format.txt,
tensorflow/core/protobuf/tensor_bundle.proto); no TensorFlow is installable here, so it is exercised only against
bundles written by the test-side writer in tests/test_host_ckpt.py (round trip), not against a real TF file.
Snappy-compressed index blocks (TF writes the bundle index uncompressed) are rejected loudly.

The other direction -- `write_bundle`, `save_reference_checkpoint` (weights, Adam-AMSGrad slots, `optimizer/iter`, `step`,
`save_counter`, the object graph), `restore_reference_checkpoint`, `ReferenceCheckpointManager` -- has the same STATUS, and a
weaker one where it says so: NO TENSORFLOW PROGRAM HAS EVER READ THESE FILES.  The writer and the reader are both restated
from the published formats; they agree with each other and with the independent test-side writer (tests/test_host_ckpt.py:
the data shard byte for byte), nothing more.  Two parts rest on MEMORY of the published source alone, with no document to
restate them from: the string-tensor layout and checksum rule (`_string_payload`, after tensor_bundle.cc's string writer) and
the field numbers of TrackableObjectGraph (`_object_graph`, after trackable_object_graph.proto).  A TF object-based `restore`
finds its keys through that graph, so a mistake in either is exactly what a first real hand-over would show;
tests/golden/make_tf_golden.py stays the path to a pin against a real file.
"""
import os
import re
import struct
import tempfile

import numpy as np

TABLE_MAGIC = 0xdb4775248b80fb57
DTYPES = {1: np.float32, 2: np.float64, 3: np.int32, 9: np.int64, 10: np.bool_, 14: None, 19: np.float16}   # 14: bfloat16
DT_STRING = 7
_ENUMS = {np.dtype(v): k for k, v in DTYPES.items() if v is not None}

_CRC_TABLE = None


def _table():
    global _CRC_TABLE
    if _CRC_TABLE is None:
        tab = []
        for i in range(256):
            c = i
            for _ in range(8):
                c = (c >> 1) ^ 0x82f63b78 if c & 1 else c >> 1
            tab.append(c)
        _CRC_TABLE = tab
    return _CRC_TABLE


def _crc_raw(data, c):
    """The table-driven register update over `data` from register value c (no initial / final inversion)."""
    tab = _table()
    for b in data:
        c = tab[(c ^ b) & 0xff] ^ (c >> 8)
    return c


def _zeros_operator(nbytes):
    """The GF(2)-linear map "feed nbytes zero bytes" on the 32-bit register, as its 32 column images."""
    tab = _table()
    cols = [tab[(1 << i) & 0xff] ^ ((1 << i) >> 8) for i in range(32)]        # one zero byte
    apply_ = lambda m, v: _xor_cols(m, v)
    result = [1 << i for i in range(32)]                                       # identity
    while nbytes:
        if nbytes & 1:
            result = [apply_(cols, v) for v in result]
        cols = [apply_(cols, v) for v in cols]
        nbytes >>= 1
    return result


def _xor_cols(cols, v):
    out, i = 0, 0
    while v:
        if v & 1:
            out ^= cols[i]
        v >>= 1
        i += 1
    return out


def crc32c(data, crc=0):
    """CRC-32C (Castagnoli), the checksum of table blocks and bundle entries.  Large buffers are cut into equal chunks
    whose registers advance together in NumPy (the update is linear over GF(2), so chunk results combine exactly)."""
    data = bytes(data)
    n = len(data)
    if n < (1 << 12) or crc:
        return _crc_raw(data, crc ^ 0xffffffff) ^ 0xffffffff
    chunks = max(64, min(4096, n >> 7))
    m = -(-n // chunks)
    buf = np.zeros(chunks * m, np.uint8)
    buf[chunks * m - n:] = np.frombuffer(data, np.uint8)                       # leading zeros leave a zero register at zero
    cols = buf.reshape(chunks, m)
    tab = np.array(_table(), np.uint32)
    state = np.zeros(chunks, np.uint32)
    for i in range(m):
        state = tab[(state ^ cols[:, i]) & 0xff] ^ (state >> 8)
    zm = _zeros_operator(m)
    total = 0
    for r in state.tolist():
        total = _xor_cols(zm, total) ^ r                                       # register(A || B) = Z_len(B)(register(A)) ^ register(B)
    init = _xor_cols(_zeros_operator(n), 0xffffffff)                          # what the 0xffffffff initial value turns into
    return (total ^ init) ^ 0xffffffff


def _mask(c):
    return (((c >> 15) | (c << 17)) + 0xa282ead8) & 0xffffffff


def masked_crc(data):
    return _mask(crc32c(data))


def _varint(buf, pos):
    out, shift = 0, 0
    while True:
        b = buf[pos]
        pos += 1
        out |= (b & 0x7f) << shift
        if not b & 0x80:
            return out, pos
        shift += 7


def _block(buf, offset, size, verify=True):
    """Entries (key, value) of one table block at [offset, offset + size); the 5-byte trailer follows it."""
    data = buf[offset:offset + size]
    ctype = buf[offset + size]
    if ctype != 0:
        raise NotImplementedError("compressed table block (type %d): the bundle index is expected uncompressed" % ctype)
    if verify:
        stored, = struct.unpack_from('<I', buf, offset + size + 1)
        if stored != masked_crc(bytes(data) + bytes([ctype])):
            raise ValueError("table block checksum mismatch at offset %d" % offset)
    num_restarts, = struct.unpack_from('<I', data, len(data) - 4)
    end = len(data) - 4 - 4 * num_restarts
    pos, key, out = 0, b'', []
    while pos < end:
        shared, pos = _varint(data, pos)
        unshared, pos = _varint(data, pos)
        vlen, pos = _varint(data, pos)
        key = key[:shared] + bytes(data[pos:pos + unshared])
        pos += unshared
        out.append((key, bytes(data[pos:pos + vlen])))
        pos += vlen
    return out


def _proto(buf):
    """Minimal protobuf wire decoding: {field number: [values]}; varints as int, length-delimited as bytes."""
    pos, out = 0, {}
    while pos < len(buf):
        tag, pos = _varint(buf, pos)
        field, wt = tag >> 3, tag & 7
        if wt == 0:
            v, pos = _varint(buf, pos)
        elif wt == 1:
            v = struct.unpack_from('<Q', buf, pos)[0]; pos += 8
        elif wt == 2:
            n, pos = _varint(buf, pos)
            v = bytes(buf[pos:pos + n]); pos += n
        elif wt == 5:
            v = struct.unpack_from('<I', buf, pos)[0]; pos += 4
        else:
            raise ValueError("unsupported protobuf wire type %d" % wt)
        out.setdefault(field, []).append(v)
    return out


def _entry(value):
    """BundleEntryProto -> (dtype enum, shape, shard_id, offset, size, crc32c or None)."""
    m = _proto(value)
    shape = []
    for sh in m.get(2, []):                                  # TensorShapeProto
        for dim in _proto(sh).get(2, []):                    # repeated Dim
            shape.append(_proto(dim).get(1, [0])[0])
    if 7 in m:
        raise NotImplementedError("sliced (partitioned) variables")
    return (m.get(1, [0])[0], tuple(shape), m.get(3, [0])[0], m.get(4, [0])[0], m.get(5, [0])[0],
            m[6][0] if 6 in m else None)


def _index_entries(prefix, verify):
    """[(key, BundleEntryProto bytes)] of the index table in file order (the header under b'' first), and the shard count."""
    with open(prefix + '.index', 'rb') as f:
        index = memoryview(f.read())
    if len(index) < 48 or struct.unpack_from('<Q', index, len(index) - 8)[0] != TABLE_MAGIC:
        raise ValueError("%s.index is not a TensorFlow table file" % prefix)
    foot = len(index) - 48
    _, pos = _varint(index, foot)                            # metaindex handle: offset, size (unused)
    _, pos = _varint(index, pos)
    ioff, pos = _varint(index, pos)
    isize, pos = _varint(index, pos)
    entries = []
    for _, handle in _block(index, ioff, isize, verify):
        off, p = _varint(handle, 0)
        size, _ = _varint(handle, p)
        entries += _block(index, off, size, verify)
    header = dict(entries).get(b'')
    num_shards = _proto(header).get(1, [1])[0] if header else 1
    if header and _proto(header).get(2, [0])[0] != 0:
        raise NotImplementedError("big-endian bundle")
    return entries, num_shards


def _payloads(prefix, verify, want):
    """(key, dtype enum, shape, raw bytes, entry crc32c or None) of every entry whose dtype enum `want` accepts."""
    entries, num_shards = _index_entries(prefix, verify)
    shards = {}
    for key, value in entries:
        if key == b'':
            continue
        dtype, shape, shard, offset, size, crc = _entry(value)
        if not want(dtype):
            continue
        if shard not in shards:
            with open('%s.data-%05d-of-%05d' % (prefix, shard, num_shards), 'rb') as f:
                shards[shard] = f.read()
        raw = shards[shard][offset:offset + size]
        if len(raw) != size:
            raise ValueError("%s: data shard too short for %r" % (prefix, key))
        yield key, dtype, shape, raw, crc


def read_bundle(prefix, verify=True):
    """{variable key: numpy array} of every numeric tensor in the checkpoint `prefix` (e.g. '.../checkpoints/ckpt-100').
    Strings (the object graph proto), variants, ... are skipped, unread and unchecked: `read_strings` reads those."""
    out = {}
    for key, dtype, shape, raw, crc in _payloads(prefix, verify, lambda d: DTYPES.get(d) is not None):
        if verify and crc is not None and masked_crc(raw) != crc:
            raise ValueError("%s: checksum mismatch for %r" % (prefix, key))
        out[key.decode()] = np.frombuffer(raw, dtype=DTYPES[dtype]).reshape(shape).copy()
    return out


def read_strings(prefix, verify=True):
    """{key: bytes (scalar) or list of bytes} of every DT_STRING tensor, by the layout of `_string_payload`; with `verify`
    both of its checksums are checked (an entry without a crc32c field, which the test-side writer leaves out, has none)."""
    out = {}
    for key, _, shape, raw, crc in _payloads(prefix, verify, lambda d: d == DT_STRING):
        count, pos, lengths, running = int(np.prod(shape, dtype=np.int64)), 0, [], 0
        try:
            for _ in range(count):
                n, pos = _varint(raw, pos)
                lengths.append(n)
                running = crc32c(struct.pack('<I' if n <= 0xffffffff else '<Q', n), running)
        except IndexError:
            raise ValueError("%s: string tensor %r is cut short" % (prefix, key))
        if crc is not None:
            if len(raw) != pos + 4 + sum(lengths):
                raise ValueError("%s: string tensor %r has the wrong size" % (prefix, key))
            if verify:
                if struct.unpack_from('<I', raw, pos)[0] != _mask(running):
                    raise ValueError("%s: length checksum mismatch for %r" % (prefix, key))
                if _mask(crc32c(raw[pos + 4:], crc32c(raw[pos:pos + 4], running))) != crc:
                    raise ValueError("%s: checksum mismatch for %r" % (prefix, key))
            pos += 4
        elems = []
        for n in lengths:
            elems.append(bytes(raw[pos:pos + n]))
            pos += n
        out[key.decode()] = elems[0] if shape == () else elems
    return out


_KEY = re.compile(r'^net/net_(query|obs)_layer(\d+)/(?:layer_with_weights-(\d+)/)?(kernel|bias)/\.ATTRIBUTES/VARIABLE_VALUE$')


def reference_weights(prefix, verify=True):
    """Checkpoint -> {'query': [[(kernel, bias), ...] per layer], 'obs': [...]} as `Model.load_weights` takes it
    (Keras layouts: Conv2D (kh,kw,Cin,Cout), Conv2DTranspose (kh,kw,Cout,Cin))."""
    return _weights_of(read_bundle(prefix, verify), prefix)


def _weights_of(bundle, prefix):
    found, other = {}, []
    for key, arr in bundle.items():
        m = _KEY.match(key)
        if m:
            net, layer, conv, what = m.group(1), int(m.group(2)), int(m.group(3) or 0), m.group(4)
            found.setdefault(net, {}).setdefault(layer, {}).setdefault(conv, {})[what] = arr
        elif key.startswith('net/') and key.endswith('/.ATTRIBUTES/VARIABLE_VALUE') and '/.OPTIMIZER_SLOT/' not in key:
            other.append(key)
    if other:
        # norm layers (gamma / beta / moving_*) would shift the layer_with_weights-N numbering: refuse instead of misaligning
        raise NotImplementedError("%s: the checkpoint holds network variables that are not conv kernels / biases (%s%s); only "
                                  "the norm = None branch can be imported" % (prefix, other[0], ', ...' if len(other) > 1 else ''))
    if 'query' not in found:
        raise ValueError("%s: no net/net_query_layer*/... variables (is this an NLT checkpoint?)" % prefix)
    out = {}
    for net, layers in found.items():
        out[net] = []
        for li in range(max(layers) + 1):
            convs = layers.get(li)
            if convs is None:
                raise ValueError("%s: %s layer %d has no variables" % (prefix, net, li))
            for c in sorted(convs):
                missing = [w for w in ('kernel', 'bias') if w not in convs[c]]
                if missing:
                    raise ValueError("%s: net_%s_layer%d (conv %d) has no %s variable" % (prefix, net, li, c, ' / '.join(missing)))
            out[net].append([(convs[c]['kernel'], convs[c]['bias']) for c in sorted(convs)])
    out.setdefault('obs', [])
    return out


def load_reference_checkpoint(model, prefix, verify=True):
    """Loads a reference checkpoint into a built nlt_amd model (same architecture keys in its config)."""
    return model.load_weights(reference_weights(prefix, verify))


# ------------------------------------------------------------------------------------------------------------ writing
def _enc_varint(n):
    out = bytearray()
    while n > 0x7f:
        out.append((n & 0x7f) | 0x80)
        n >>= 7
    out.append(n)
    return bytes(out)


def _pb_varint(field, v):
    return _enc_varint(field << 3) + _enc_varint(v)


def _pb_bytes(field, b):
    return _enc_varint(field << 3 | 2) + _enc_varint(len(b)) + bytes(b)


class _BlockBuilder:
    """One table block (table_format.txt): entries `shared | unshared | value length | key suffix | value`, keys
    prefix-compressed against their predecessor except at a restart point, then the restart offsets and their count."""

    def __init__(self, restart_interval):
        self.interval, self.buf, self.restarts, self.count, self.last = restart_interval, bytearray(), [0], 0, b''

    def add(self, key, value):
        shared = 0
        if self.count and self.count % self.interval == 0:
            self.restarts.append(len(self.buf))
        elif self.count:
            while shared < min(len(key), len(self.last)) and key[shared] == self.last[shared]:
                shared += 1
        self.buf += _enc_varint(shared) + _enc_varint(len(key) - shared) + _enc_varint(len(value)) + key[shared:] + value
        self.count, self.last = self.count + 1, key

    def size(self):
        return len(self.buf) + 4 * len(self.restarts) + 4

    def finish(self):
        """The block and its 5-byte trailer: type 0 (uncompressed) + the masked CRC of block and type byte."""
        block = bytes(self.buf) + b''.join(struct.pack('<I', r) for r in self.restarts) + struct.pack('<I', len(self.restarts))
        return block + b'\x00' + struct.pack('<I', masked_crc(block + b'\x00'))


def _sstable(entries, block_size, restart_interval):
    """The SSTable holding sorted (key, value) `entries`: data blocks, an empty metaindex block, the index block (one entry
    per data block: its last key -> its handle), the 48-byte footer."""
    out, index, blk = bytearray(), _BlockBuilder(1), None

    def flush():
        data = blk.finish()
        index.add(blk.last, _enc_varint(len(out)) + _enc_varint(len(data) - 5))
        out.extend(data)
    for key, value in entries:
        if blk is None:
            blk = _BlockBuilder(restart_interval)
        blk.add(key, value)
        if blk.size() >= block_size:
            flush()
            blk = None
    if blk is not None:
        flush()
    handles = b''
    for block in (_BlockBuilder(restart_interval), index):
        data = block.finish()
        handles += _enc_varint(len(out)) + _enc_varint(len(data) - 5)
        out.extend(data)
    return bytes(out) + handles + b'\x00' * (40 - len(handles)) + struct.pack('<Q', TABLE_MAGIC)


def _string_payload(elems):
    """(payload, entry crc32c) of a DT_STRING tensor.  RESTATED FROM MEMORY of tensor_bundle.cc's string writer, not from a
    document: the varint64 length of every element; 4 bytes holding the masked CRC-32C taken over those lengths as fixed-width
    little-endian integers (uint32 where the length fits, uint64 otherwise); the elements' bytes.  The entry's crc32c is the
    mask of the running CRC carried on over the 4 checksum bytes and the elements' bytes."""
    lengths, running = b'', 0
    for e in elems:
        lengths += _enc_varint(len(e))
        running = crc32c(struct.pack('<I' if len(e) <= 0xffffffff else '<Q', len(e)), running)
    check = struct.pack('<I', _mask(running))
    body = b''.join(elems)
    return lengths + check + body, _mask(crc32c(body, crc32c(check, running)))


def _bundle_entry(dtype, shape, offset, size, crc):
    """BundleEntryProto; like any proto3 writer, fields at their default (shard_id 0, offset 0) are left out."""
    dims = b''.join(_pb_bytes(2, _pb_varint(1, d) if d else b'') for d in shape)
    return (_pb_varint(1, dtype) + _pb_bytes(2, dims) + (_pb_varint(4, offset) if offset else b'')
            + (_pb_varint(5, size) if size else b'') + _enc_varint(6 << 3 | 5) + struct.pack('<I', crc))


def write_bundle(prefix, tensors, block_size=262144, restart_interval=16):
    """Writes {key: NumPy array (float32 / float64 / int32 / int64 / bool / float16) or bytes (a scalar DT_STRING)} as the
    tensor bundle `read_bundle` reads: one data shard with the payloads in sorted key order, little-endian, unpadded, and
    the index table.  `block_size` is this writer's own choice (no reader depends on it).  Both files are written under
    temporary names and renamed into place, the shard first: a reader never meets an index without its shard."""
    if block_size < 1 or restart_interval < 1:
        raise ValueError("block_size and restart_interval must be positive")
    items = []
    for key, value in tensors.items():
        if not isinstance(value, (bytes, bytearray)):
            value = np.asarray(value)
            value = value.astype(value.dtype.newbyteorder('<'), copy=False)
            if value.dtype not in _ENUMS:
                raise TypeError("%r: dtype %s cannot be written" % (key, value.dtype))
        items.append((key.encode(), value))
    items.sort(key=lambda kv: kv[0])
    if items and items[0][0] == b'':
        raise ValueError("the empty key is the bundle header's")
    directory = os.path.dirname(os.path.abspath(prefix))
    names = (prefix + '.data-00000-of-00001', prefix + '.index')
    temps = []
    try:
        entries = [(b'', _pb_varint(1, 1) + _pb_bytes(3, _pb_varint(1, 1)))]   # num_shards 1, (endianness LITTLE = 0,) version {producer 1}
        fd, tmp = tempfile.mkstemp(dir=directory, prefix=os.path.basename(names[0]) + '.', suffix='.tmp')
        temps.append(tmp)
        with os.fdopen(fd, 'wb') as f:
            offset = 0
            for key, value in items:
                if isinstance(value, (bytes, bytearray)):
                    dtype, shape = DT_STRING, ()
                    payload, crc = _string_payload([bytes(value)])
                else:
                    dtype, shape = _ENUMS[value.dtype], value.shape
                    payload = value.tobytes()
                    crc = masked_crc(payload)
                entries.append((key, _bundle_entry(dtype, shape, offset, len(payload), crc)))
                f.write(payload)
                offset += len(payload)
        fd, tmp = tempfile.mkstemp(dir=directory, prefix=os.path.basename(names[1]) + '.', suffix='.tmp')
        temps.append(tmp)
        with os.fdopen(fd, 'wb') as f:
            f.write(_sstable(entries, block_size, restart_interval))
        for tmp, name in zip(temps, names):
            os.replace(tmp, name)
        temps = []
    finally:
        for tmp in temps:
            if os.path.exists(tmp):
                os.remove(tmp)
    return prefix


# ------------------------------------------------------------------------------- tf.train.Checkpoint(step, optimizer, net)
_VALUE = '/.ATTRIBUTES/VARIABLE_VALUE'
_SLOT = '/.OPTIMIZER_SLOT/optimizer/'
SLOTS = ('m', 'v', 'vhat')                       # Keras Adam(amsgrad=True)'s slot names
OBJECT_GRAPH_KEY = '_CHECKPOINTABLE_OBJECT_GRAPH'


def _variable_prefixes(model):
    """'net/net_<name>_layer<i>[/layer_with_weights-<j>]/{kernel,bias}' of every variable in canonical order (query layers,
    then obs layers; kernel, then bias: `Model._conv_layers`, `Model.bucket_to_variables`).  Refuses what `reference_weights`
    could not import again, so that round trips stay closed."""
    from .networks.elements import ChannelNorm, Conv2D, Sequential
    out = []
    for net in ('query', 'obs'):
        for li, layer in enumerate(model.net[net].layers):
            where = 'net_%s_layer%d' % (net, li)
            if isinstance(layer, Conv2D):
                convs, mids = [layer], ['']
            else:
                convs = []
                for sub in layer.layers:
                    if isinstance(sub, ChannelNorm):
                        # gamma / beta (moving_*) would shift the layer_with_weights-N numbering of the block's convs
                        raise NotImplementedError("%s holds network variables that are not conv kernels / biases (the gamma / "
                                                  "beta of norm = %s); only the norm = None branch can be exported" % (where, sub.name))
                    if isinstance(sub, Sequential) and sub.all_convs():
                        raise NotImplementedError("%s holds network variables that are not conv kernels / biases of the block "
                                                  "itself (a nested Sequential: upconv, pool != None); it cannot be exported" % where)
                    if isinstance(sub, Conv2D):
                        convs.append(sub)
                mids = ['/layer_with_weights-%d' % j for j in range(len(convs))]
            for c, mid in zip(convs, mids):
                if c.kernel is None:
                    raise ValueError("%s has no variables yet: build() the model first" % where)
                out += ['net/%s%s/kernel' % (where, mid), 'net/%s%s/bias' % (where, mid)]
    return out


def _object_graph(keys):
    """The serialized TrackableObjectGraph that names every key of `keys`.  FIELD NUMBERS RESTATED FROM MEMORY of
    trackable_object_graph.proto: graph.nodes = 1; node.children = 1 (ObjectReference: node_id = 1, local_name = 2),
    node.attributes = 2 (SerializedTensor: name = 1, full_name = 2, checkpoint_key = 3), node.slot_variables = 3
    (SlotVariableReference: original_variable_node_id = 1, slot_name = 2, slot_variable_node_id = 3).  Node 0 is the root;
    below it the children are exactly the path components of the keys; a slot variable is a node of its own, referred to
    from the `optimizer` node."""
    nodes = [{'children': {}, 'attributes': [], 'slots': []}]

    def new_node():
        nodes.append({'children': {}, 'attributes': [], 'slots': []})
        return len(nodes) - 1

    def walk(path):
        at = 0
        for name in path:
            if name not in nodes[at]['children']:
                nodes[at]['children'][name] = new_node()
            at = nodes[at]['children'][name]
        return at
    attribute = lambda path, key: _pb_bytes(1, b'VARIABLE_VALUE') + _pb_bytes(2, '/'.join(path).encode()) + _pb_bytes(3, key.encode())
    plain = sorted(k for k in keys if _SLOT not in k)
    for key in plain:
        path = key[:-len(_VALUE)].split('/')
        nodes[walk(path)]['attributes'].append(attribute(path, key))
    for key in sorted(k for k in keys if _SLOT in k):
        variable, slot = key[:-len(_VALUE)].split(_SLOT)
        at = new_node()
        nodes[at]['attributes'].append(attribute(variable.split('/') + [slot], key))
        nodes[walk(['optimizer'])]['slots'].append(_pb_varint(1, walk(variable.split('/'))) + _pb_bytes(2, slot.encode()) + _pb_varint(3, at))
    out = b''
    for node in nodes:
        out += _pb_bytes(1, b''.join([_pb_bytes(1, _pb_varint(1, i) + _pb_bytes(2, name.encode())) for name, i in node['children'].items()]
                                     + [_pb_bytes(2, a) for a in node['attributes']] + [_pb_bytes(3, s) for s in node['slots']]))
    return out


def read_object_graph(prefix, verify=True):
    """The checkpoint's object graph as a list of nodes {'children': [(node_id, local_name)], 'attributes': [{'name',
    'full_name', 'checkpoint_key'}], 'slot_variables': [{'original_variable_node_id', 'slot_name', 'slot_variable_node_id'}]};
    the string tensor's checksums are verified by the rule of `_string_payload`."""
    strings = read_strings(prefix, verify)
    if OBJECT_GRAPH_KEY not in strings:
        raise ValueError("%s: no %s entry" % (prefix, OBJECT_GRAPH_KEY))
    text = lambda m, f: m.get(f, [b''])[0].decode()
    nodes = []
    for raw in _proto(strings[OBJECT_GRAPH_KEY]).get(1, []):
        m = _proto(raw)
        children = [_proto(c) for c in m.get(1, [])]
        attributes = [_proto(a) for a in m.get(2, [])]
        slots = [_proto(s) for s in m.get(3, [])]
        nodes.append({'children': [(c.get(1, [0])[0], text(c, 2)) for c in children],
                      'attributes': [{'name': text(a, 1), 'full_name': text(a, 2), 'checkpoint_key': text(a, 3)} for a in attributes],
                      'slot_variables': [{'original_variable_node_id': s.get(1, [0])[0], 'slot_name': text(s, 2),
                                          'slot_variable_node_id': s.get(3, [0])[0]} for s in slots]})
    return nodes


def save_reference_checkpoint(model, prefix, optimizer=None, step=None, save_counter=None):
    """Writes what the reference's `tf.train.Checkpoint(step=..., optimizer=..., net=model)` saves (nlt/trainvali.py:134-141)
    under `prefix`: every kernel / bias in Keras layout, float32, exactly `Model.get_weights()`; with `optimizer` its m / v /
    vhat per variable, `optimizer/iter` (int64 = optimizer.t) and the float32 scalars learning_rate, beta_1, beta_2, decay
    (0.0); with `step` the int32 `step` (`tf.Variable(0)` is int32); with `save_counter` the int64 one; and the object graph.

    Saving reads the device and changes nothing on it: the weights and each optimizer bucket come over as host copies and
    are cut into variables on the host -- no write to `flat_params`, no `mark_weights_updated()`, no device allocation.
    Models `reference_weights` could not import (norm layers with gamma / beta; nested Sequentials: upconv) are refused
    with NotImplementedError before anything is written."""
    names = _variable_prefixes(model)
    if optimizer is not None and optimizer.model is not model:
        raise ValueError("the optimizer belongs to another model")
    weights = model.get_weights()
    arrays = [a for net in ('query', 'obs') for convs in weights[net] for kb in convs for a in kb]
    assert len(arrays) == len(names)
    tensors = {name + _VALUE: np.asarray(a, np.float32) for name, a in zip(names, arrays)}
    if optimizer is not None:
        for slot in SLOTS:
            host = getattr(optimizer, slot).detach().cpu()                    # the whole bucket once; cut per variable on the host
            for name, t in zip(names, model.bucket_to_variables(host)):
                tensors[name + _SLOT + slot + _VALUE] = t.numpy()
        tensors['optimizer/iter' + _VALUE] = np.array(optimizer.t, np.int64)
        for name, v in (('learning_rate', optimizer.lr), ('beta_1', optimizer.b1), ('beta_2', optimizer.b2), ('decay', 0.0)):
            tensors['optimizer/%s%s' % (name, _VALUE)] = np.array(v, np.float32)
    if step is not None:
        tensors['step' + _VALUE] = np.array(int(step), np.int32)
    if save_counter is not None:
        tensors['save_counter' + _VALUE] = np.array(int(save_counter), np.int64)
    tensors[OBJECT_GRAPH_KEY] = _object_graph(list(tensors))
    return write_bundle(prefix, tensors)


def _sorted_variable_prefixes(bundle):
    """The conv variables a bundle holds, as prefixes in canonical order (query before obs, by layer, by conv, kernel first)."""
    found = []
    for key in bundle:
        m = _KEY.match(key)
        if m:
            found.append((m.group(1) != 'query', int(m.group(2)), int(m.group(3) or 0), m.group(4) != 'kernel', key[:-len(_VALUE)]))
    return [f[-1] for f in sorted(found)]


def _optimizer_state_of(bundle, prefix):
    out = {slot: [] for slot in SLOTS}
    for name in _sorted_variable_prefixes(bundle):
        for slot in SLOTS:
            key = name + _SLOT + slot + _VALUE
            if key not in bundle:
                raise ValueError("%s holds no optimizer state: %s is missing" % (prefix, key))
            out[slot].append(bundle[key])
    if 'optimizer/iter' + _VALUE not in bundle:
        raise ValueError("%s holds no optimizer state: optimizer/iter%s is missing" % (prefix, _VALUE))
    out['t'] = int(bundle['optimizer/iter' + _VALUE])
    return out


def reference_optimizer_state(prefix, verify=True):
    """{'t': optimizer/iter, 'm' / 'v' / 'vhat': [array per variable, canonical order]} of a checkpoint the reference's (or
    this project's) train loop wrote: `AdamAMSGrad.load_state_dict`'s structure.  ValueError names the first missing slot."""
    return _optimizer_state_of(read_bundle(prefix, verify), prefix)


def restore_reference_checkpoint(model, prefix, optimizer=None, verify=True):
    """The reference's `ckpt.restore(latest_checkpoint)` (nlt/util/io.py:32-35, called at nlt/trainvali.py:141): loads the net, with `optimizer` also its Adam-AMSGrad
    slots and iteration count (a net-only file is then a ValueError, raised before anything is overwritten); returns the saved
    `step`, or None when the file has none (`tf.train.Checkpoint(net=model)`).  The optimizer's hyper-parameters stay what
    this process's config set them to."""
    import torch
    bundle = read_bundle(prefix, verify)
    weights = _weights_of(bundle, prefix)
    state = _optimizer_state_of(bundle, prefix) if optimizer is not None else None
    model.load_weights(weights)
    if getattr(model, 'flat_params', None) is not None:
        model.mark_weights_updated()
    if state is not None:
        optimizer.load_state_dict({k: (v if k == 't' else [torch.from_numpy(a) for a in v]) for k, v in state.items()})
    step = bundle.get('step' + _VALUE)
    return None if step is None else int(step)


class ReferenceCheckpointManager:
    """The `tf.train.CheckpointManager(ckpt, directory, max_to_keep)` of nlt/trainvali.py:139-141,194: numbered saves
    `directory/ckpt-N` (N = the save counter, 1-based, continued from the state file by a fresh manager), the oldest ones
    beyond `max_to_keep` deleted, and the text-format `checkpoint` state file with names relative to the directory."""
    STATE = 'checkpoint'
    SUFFIXES = ('.index', '.data-00000-of-00001')

    def __init__(self, directory, max_to_keep=None):
        if max_to_keep is not None and max_to_keep < 1:
            raise ValueError("max_to_keep must be None or positive")
        self.directory, self.max_to_keep = directory, max_to_keep
        os.makedirs(directory, exist_ok=True)
        self._names, latest = [], None
        state = os.path.join(directory, self.STATE)
        if os.path.exists(state):
            with open(state) as f:
                for line in f:
                    m = re.match(r'\s*(model_checkpoint_path|all_model_checkpoint_paths)\s*:\s*"(.*)"\s*$', line)
                    if m and m.group(1) == 'model_checkpoint_path':
                        latest = m.group(2)
                    elif m:
                        self._names.append(m.group(2))
        if latest is not None and latest not in self._names:
            self._names.append(latest)
        m = re.search(r'-(\d+)$', latest or '')
        self.save_counter = int(m.group(1)) if m else 0

    @property
    def checkpoints(self):
        return [os.path.join(self.directory, n) for n in self._names]

    @property
    def latest_checkpoint(self):
        return os.path.join(self.directory, self._names[-1]) if self._names else None

    def save(self, model, optimizer, step):
        name = 'ckpt-%d' % (self.save_counter + 1)
        save_reference_checkpoint(model, os.path.join(self.directory, name), optimizer, step, save_counter=self.save_counter + 1)
        self.save_counter += 1
        self._names.append(name)
        drop = self._names[:-self.max_to_keep] if self.max_to_keep else []
        self._names = self._names[len(drop):]
        text = 'model_checkpoint_path: "%s"\n' % name + ''.join('all_model_checkpoint_paths: "%s"\n' % n for n in self._names)
        fd, tmp = tempfile.mkstemp(dir=self.directory, prefix=self.STATE + '.', suffix='.tmp')
        with os.fdopen(fd, 'w') as f:
            f.write(text)
        os.replace(tmp, os.path.join(self.directory, self.STATE))
        for old in drop:                                    # (after the state file stopped naming them)
            for suffix in self.SUFFIXES:
                path = os.path.join(self.directory, old + suffix)
                if os.path.exists(path):
                    os.remove(path)
        return os.path.join(self.directory, name)
