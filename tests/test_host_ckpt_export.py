"""CPU: nlt_amd.ckpt WRITES the reference's checkpoint format -- the tensor bundle (`write_bundle`), what
`tf.train.Checkpoint(step, optimizer, net)` saves (`save_reference_checkpoint`: weights, Adam-AMSGrad slots, optimizer/iter,
step, save_counter, the object graph), the way back (`restore_reference_checkpoint`, `reference_optimizer_state`,
`read_object_graph`) and the `CheckpointManager` (`ReferenceCheckpointManager`, trainvali.save_reference / resume_reference).

Every comparison is bit equality: the feature only copies values.  No TensorFlow exists here: the product's writer is held
against the product's reader, against the independent writer of tests/test_host_ckpt.py (data shard byte for byte) and against
the few lines of index parsing below -- not against a file TensorFlow wrote or read (said so in ckpt.py's STATUS).

`read_bundle` keeps skipping string tensors (tests/test_host_ckpt.py pins that), so the round trip compares its dict with the
numeric part of what was written and reads the `bytes` value back through `read_strings`."""
import os
import struct

import numpy as np
import pytest
import torch

import nlt_amd
from nlt_amd import ckpt, trainvali
from nlt_amd.models import get_model_class
from oracle import nlt_oracle as O
import fake_capi
import test_host_ckpt as TW
import test_host_generic as G
from test_host_orchestration import make, cpu_batch

V = '/.ATTRIBUTES/VARIABLE_VALUE'
SHARD = '.data-00000-of-00001'


def _tensors():
    rng = np.random.default_rng(3)
    return {'a/f32': rng.standard_normal((1, 1, 5, 16)).astype(np.float32),
            'a/i32': np.array(-7, np.int32),
            'b/i64': np.array([2 ** 40, -1, 0], np.int64),
            'b/bool': np.array([[True, False], [False, True]]),
            'c/f16': rng.standard_normal((3, 2)).astype(np.float16),
            'c/empty': np.zeros((0,), np.float32)}


def _same_dict(got, want):
    assert sorted(got) == sorted(want)
    for k, v in want.items():
        assert got[k].dtype == v.dtype and got[k].shape == v.shape and got[k].tobytes() == v.tobytes(), k


# ---- an index reader of the test's own: footer -> index block -> data blocks (table_format.txt)
def _vi(buf, pos):
    out, shift = 0, 0
    while True:
        b = buf[pos]; pos += 1
        out |= (b & 0x7f) << shift
        if b < 0x80:
            return out, pos
        shift += 7


def _block_entries(buf, off, size):
    blk = buf[off:off + size]
    assert buf[off + size] == 0                                              # uncompressed
    n_restarts, = struct.unpack_from('<I', blk, size - 4)
    end, pos, key, out = size - 4 - 4 * n_restarts, 0, b'', []
    restarts = struct.unpack_from('<%dI' % n_restarts, blk, end)
    while pos < end:
        at = pos
        shared, pos = _vi(blk, pos); unshared, pos = _vi(blk, pos); vlen, pos = _vi(blk, pos)
        assert shared == 0 or at not in restarts                             # a restart point holds a full key
        key = key[:shared] + blk[pos:pos + unshared]; pos += unshared
        out.append((key, blk[pos:pos + vlen])); pos += vlen
    return out


def _fields(buf):
    """{field: last value} of a flat protobuf message (varint / length-delimited / fixed32 only)."""
    pos, out = 0, {}
    while pos < len(buf):
        tag, pos = _vi(buf, pos)
        if tag & 7 == 0:
            v, pos = _vi(buf, pos)
        elif tag & 7 == 2:
            n, pos = _vi(buf, pos); v = buf[pos:pos + n]; pos += n
        else:
            assert tag & 7 == 5
            v, = struct.unpack_from('<I', buf, pos); pos += 4
        out[tag >> 3] = v
    return out


def _data_blocks(prefix):
    """[[(key, value), ...] per data block] of prefix.index, and the index block's own keys."""
    buf = open(prefix + '.index', 'rb').read()
    assert len(buf) >= 48 and struct.unpack_from('<Q', buf, len(buf) - 8)[0] == 0xdb4775248b80fb57
    pos = len(buf) - 48
    moff, pos = _vi(buf, pos); msize, pos = _vi(buf, pos); ioff, pos = _vi(buf, pos); isize, pos = _vi(buf, pos)
    assert set(buf[pos:len(buf) - 8]) <= {0}                                 # zero padding up to the magic
    assert _block_entries(buf, moff, msize) == []                            # the empty metaindex block
    blocks, seps = [], []
    for sep, handle in _block_entries(buf, ioff, isize):
        off, p = _vi(handle, 0); size, _ = _vi(handle, p)
        blocks.append(_block_entries(buf, off, size)); seps.append(sep)
    return blocks, seps


# ------------------------------------------------------------------------------------------------ 1-4: the bundle
@pytest.mark.parametrize('block_size', [None, 64])
def test_bundle_round_trip(tmp_path, block_size):
    """(1) every dtype, the shapes (), (0,), (1,1,5,16), and a bytes value; default block size, and one at which the header
    and 7 keys span >= 3 data blocks."""
    t = _tensors()
    prefix = str(tmp_path / 'b')
    kw = {} if block_size is None else {'block_size': block_size, 'restart_interval': 2}
    assert ckpt.write_bundle(prefix, dict(t, **{'b/text': b'\x00object graph\xff' * 9}), **kw) == prefix
    assert sorted(os.listdir(tmp_path)) == ['b' + SHARD, 'b.index']          # no temporary file is left
    _same_dict(ckpt.read_bundle(prefix, verify=True), t)
    assert ckpt.read_strings(prefix) == {'b/text': b'\x00object graph\xff' * 9}
    blocks, _ = _data_blocks(prefix)
    assert (len(blocks) >= 3) if block_size else (len(blocks) == 1)
    with pytest.raises(TypeError):
        ckpt.write_bundle(str(tmp_path / 'c'), {'x': np.zeros(2, np.complex64)})
    assert sorted(os.listdir(tmp_path)) == ['b' + SHARD, 'b.index']


def test_data_shard_is_byte_identical_to_the_independent_writers(tmp_path):
    """(2) same float32 / int64 tensors through tests/test_host_ckpt.py's writer and the product's: one data shard, byte for
    byte, and the product's reader returns the same dict from both."""
    rng = np.random.default_rng(4)
    t = TW.reference_keys(O.OracleModel(depth=32, uvh=64, uvw=64, imh=32, imw=32, seed=2).numpy_weights())
    t['step' + V] = np.array(1234, np.int64)
    t['optimizer/iter' + V] = np.array(77, np.int64)
    t['odd'] = rng.standard_normal((3, 5, 7)).astype(np.float32)
    TW.write_bundle(str(tmp_path / 'theirs'), t)
    ckpt.write_bundle(str(tmp_path / 'ours'), t)
    assert open(str(tmp_path / 'ours') + SHARD, 'rb').read() == open(str(tmp_path / 'theirs') + SHARD, 'rb').read()
    _same_dict(ckpt.read_bundle(str(tmp_path / 'ours')), ckpt.read_bundle(str(tmp_path / 'theirs')))


@pytest.mark.parametrize('block_size', [None, 100])
def test_index_read_by_a_parser_of_the_tests_own(tmp_path, block_size):
    """(3) footer -> index block -> data blocks: the header first, every key once, in sorted order, offset + size tiling the
    shard without gaps, each entry's crc32c the masked CRC of its payload, each separator inside its legal range."""
    t = _tensors()
    prefix = str(tmp_path / 'b')
    ckpt.write_bundle(prefix, t, **({} if block_size is None else {'block_size': block_size}))
    blocks, seps = _data_blocks(prefix)
    entries = [e for b in blocks for e in b]
    assert entries[0][0] == b''
    head = _fields(entries[0][1])
    assert head.get(1) == 1 and head.get(2, 0) == 0 and _fields(head[3]).get(1) == 1   # num_shards, LITTLE, version.producer
    assert [k for k, _ in entries[1:]] == sorted(k.encode() for k in t)
    for i, (b, sep) in enumerate(zip(blocks, seps)):
        assert sep >= b[-1][0] and (i + 1 == len(blocks) or sep < blocks[i + 1][0][0])
    shard, at = open(prefix + SHARD, 'rb').read(), 0
    enum = {np.dtype(np.float32): 1, np.dtype(np.int32): 3, np.dtype(np.int64): 9, np.dtype(np.bool_): 10, np.dtype(np.float16): 19}
    for k, v in entries[1:]:
        f, want = _fields(v), t[k.decode()]
        assert f[1] == enum[want.dtype] and f.get(3, 0) == 0 and f.get(4, 0) == at and f.get(5, 0) == want.nbytes
        payload = shard[at:at + want.nbytes]
        assert payload == want.tobytes() and f[6] == ckpt.masked_crc(payload)
        at += want.nbytes
    assert at == len(shard)


def test_corruption_is_caught(tmp_path):
    """(4) one flipped byte in the shard, then one in an index data block, then one in the string tensor."""
    prefix = str(tmp_path / 'b')
    ckpt.write_bundle(prefix, dict(_tensors(), zz=b'some text'), block_size=100)

    def flipped(suffix, at):
        raw = bytearray(open(prefix + suffix, 'rb').read())
        raw[at] ^= 0x10
        open(prefix + suffix, 'wb').write(bytes(raw))
    good = open(prefix + SHARD, 'rb').read()
    flipped(SHARD, 40)                                                       # inside 'a/f32' (the first payload, 320 bytes)
    with pytest.raises(ValueError, match='checksum'):
        ckpt.read_bundle(prefix)
    open(prefix + SHARD, 'wb').write(good)
    assert ckpt.read_bundle(prefix) and ckpt.read_strings(prefix) == {'zz': b'some text'}
    flipped(SHARD, len(good) - 2)                                            # inside the string's bytes: read_strings checks them
    with pytest.raises(ValueError, match='checksum'):
        ckpt.read_strings(prefix)
    open(prefix + SHARD, 'wb').write(good)
    flipped('.index', 10)                                                    # inside the first data block
    with pytest.raises(ValueError, match='checksum'):
        ckpt.read_bundle(prefix)


# --------------------------------------------------------------------------------- 5-7: tf.train.Checkpoint's contents
def _trainable(depth=256, seed=1, **kw):
    _, pm = make(depth, 64, 32, loss='l2', **kw)
    pm.build('cpu'); pm.register_trainable()
    with torch.no_grad():
        pm.flat_params.mul_(1.0 + 0.01 * seed)                               # different weights per instance
    pm.mark_weights_updated()
    return pm, nlt_amd.optim.AdamAMSGrad(pm, 1e-3)


def _slot_keys(weights):
    return [k[:-len(V)] + '/.OPTIMIZER_SLOT/optimizer/' + s + V for k in TW.reference_keys(weights) for s in ('m', 'v', 'vhat')]


def test_keys_and_dtypes(tmp_path):
    """(5) net alone: exactly test_host_ckpt.reference_keys; with optimizer, step and save counter: the slot, optimizer/*,
    step and save_counter keys too, with the dtypes TensorFlow gives them."""
    _, pm = make(256, 64, 32)
    want = TW.reference_keys(pm.get_weights())
    prefix = str(tmp_path / 'net')
    assert ckpt.save_reference_checkpoint(pm, prefix) == prefix
    got = ckpt.read_bundle(prefix)
    _same_dict(got, want)
    assert list(ckpt.read_strings(prefix)) == ['_CHECKPOINTABLE_OBJECT_GRAPH']
    pm, opt = _trainable(32)
    opt.t = 5
    with torch.no_grad():
        opt.m.normal_(); opt.v.uniform_(); opt.vhat.uniform_()
    ckpt.save_reference_checkpoint(pm, str(tmp_path / 'all'), opt, step=12, save_counter=3)
    got = ckpt.read_bundle(str(tmp_path / 'all'))
    w = pm.get_weights()
    scalars = {'optimizer/iter' + V: np.array(5, np.int64), 'optimizer/learning_rate' + V: np.array(1e-3, np.float32),
               'optimizer/beta_1' + V: np.array(0.9, np.float32), 'optimizer/beta_2' + V: np.array(0.999, np.float32),
               'optimizer/decay' + V: np.array(0.0, np.float32), 'step' + V: np.array(12, np.int32),
               'save_counter' + V: np.array(3, np.int64)}
    assert sorted(got) == sorted(list(TW.reference_keys(w)) + _slot_keys(w) + list(scalars))
    _same_dict({k: got[k] for k in scalars}, scalars)
    sd = opt.state_dict()
    for i, k in enumerate(TW.reference_keys(w)):                             # (its insertion order is the canonical one)
        for s in ('m', 'v', 'vhat'):
            slot = got[k[:-len(V)] + '/.OPTIMIZER_SLOT/optimizer/' + s + V]
            assert slot.dtype == np.float32 and slot.tobytes() == sd[s][i].numpy().tobytes() and slot.shape == tuple(sd[s][i].shape)
    assert float(np.abs(got[_slot_keys(w)[0]]).sum()) > 0


@pytest.mark.parametrize('kw', [dict(depth=256), dict(depth=32, kernel=3), dict(depth=256, use_obs=False), dict(depth=32, act='elu')],
                         ids=lambda kw: '+'.join('%s=%s' % x for x in kw.items()))
def test_identity_through_a_model(tmp_path, kw):
    """(6) export, `load_reference_checkpoint` into a freshly initialised model: every kernel and bias bit for bit."""
    kw = dict(kw)
    depth = kw.pop('depth')
    _, pm = G.make(depth, 64, 32, **kw)
    prefix = str(tmp_path / 'ckpt-1')
    ckpt.save_reference_checkpoint(pm, prefix)
    fresh = get_model_class('nlt')(nlt_amd.make_config(depth=depth, uvh=64, uvw=64, imh=32, imw=32, **kw))
    fresh.build('cpu')
    a, b = fresh.get_weights(), pm.get_weights()
    assert not np.array_equal(a['query'][1][0][0], b['query'][1][0][0])
    ckpt.load_reference_checkpoint(fresh, prefix)
    a, n = fresh.get_weights(), 0
    for net in ('query', 'obs'):
        assert len(a[net]) == len(b[net])
        for la, lb in zip(a[net], b[net]):
            assert len(la) == len(lb)
            for (ka, ba), (kb, bb) in zip(la, lb):
                assert ka.dtype == np.float32 and ka.shape == kb.shape and ka.tobytes() == kb.tobytes() and ba.tobytes() == bb.tobytes()
                n += 1
    assert n == len(pm._conv_layers())


def test_object_graph_is_self_consistent(tmp_path):
    """(7) every variable key is found by walking `children` from node 0 along its path components; every slot key through a
    `slot_variables` entry of the optimizer node that names the variable's own node; no node is unreachable."""
    pm, opt = _trainable(32)
    prefix = str(tmp_path / 'ckpt-1')
    ckpt.save_reference_checkpoint(pm, prefix, opt, step=4, save_counter=1)
    nodes = ckpt.read_object_graph(prefix)
    keys = list(ckpt.read_bundle(prefix))
    assert sorted(name for _, name in nodes[0]['children']) == ['net', 'optimizer', 'save_counter', 'step']

    def walk(path):
        at = 0
        for name in path:
            (at,) = [i for i, n in nodes[at]['children'] if n == name]
        return at

    def key_of(node):
        (a,) = nodes[node]['attributes']
        assert a['name'] == 'VARIABLE_VALUE'
        return a['checkpoint_key']
    reached = {0}

    def mark(path):
        at = 0
        for name in path:
            at = dict((n, i) for i, n in nodes[at]['children'])[name]
            reached.add(at)
    plain = [k for k in keys if '/.OPTIMIZER_SLOT/' not in k]
    slots = [k for k in keys if '/.OPTIMIZER_SLOT/' in k]
    assert len(slots) == 3 * len([k for k in plain if k.startswith('net/')]) > 0
    for k in plain:
        path = k[:-len(V)].split('/')
        assert key_of(walk(path)) == k
        mark(path)
    refs = nodes[walk(['optimizer'])]['slot_variables']
    assert len(refs) == len(slots) and all(not n['slot_variables'] for i, n in enumerate(nodes) if i != walk(['optimizer']))
    by_key = {key_of(r['slot_variable_node_id']): r for r in refs}
    for k in slots:
        variable, slot = k[:-len(V)].split('/.OPTIMIZER_SLOT/optimizer/')
        r = by_key[k]
        assert r['slot_name'] == slot and r['original_variable_node_id'] == walk(variable.split('/'))
        reached.add(r['slot_variable_node_id'])
    assert reached == set(range(len(nodes)))
    # below `net` the children are exactly the keys' path components
    assert sorted(n for _, n in nodes[walk(['net'])]['children']) == sorted({k.split('/')[1] for k in plain if k.startswith('net/')})
    assert sorted(n for _, n in nodes[walk(['net', 'net_query_layer1'])]['children']) == ['layer_with_weights-0', 'layer_with_weights-1']
    assert sorted(n for _, n in nodes[walk(['net', 'net_query_layer0'])]['children']) == ['bias', 'kernel']


# ------------------------------------------------------------------------------------------------- 8-10: resuming
def test_resume_on_the_cpu_path_into_the_other_bucket_layout(monkeypatch, tmp_path):
    """(8) two steps, export; a fresh model + optimizer built with the other NLT_GRAD_RANGES layout restores the step, opt.t,
    m / v / vhat and the weights per variable -- and the step after lands on the same weights."""
    fake_capi.install(monkeypatch)
    b = cpu_batch(*O.synth_batch(2, 64, 64, 32, 32, 32, 32, k=1, seed=21))
    pm, opt = _trainable(256, seed=1)
    for _ in range(2):
        trainvali.distributed_train_step(pm, b, opt, 2)
    prefix = str(tmp_path / 'ckpt-2')
    before = (pm.flat_params.detach().clone(), pm.flat_params._version, pm._epoch[0])
    ckpt.save_reference_checkpoint(pm, prefix, opt, step=2)
    assert torch.equal(pm.flat_params.detach(), before[0]) and (pm.flat_params._version, pm._epoch[0]) == before[1:]
    monkeypatch.setenv('NLT_GRAD_RANGES', '2')
    pm2, opt2 = _trainable(256, seed=2)
    monkeypatch.delenv('NLT_GRAD_RANGES')
    assert [s[0] for s in pm2._slots] != [s[0] for s in pm._slots]
    epoch = pm2._epoch[0]
    assert ckpt.restore_reference_checkpoint(pm2, prefix, opt2) == 2
    assert opt2.t == opt.t == 2 and pm2._epoch[0] > epoch

    def same_state():
        for a_, b_ in zip(pm2.bucket_to_variables(pm2.flat_params), pm.bucket_to_variables(pm.flat_params)):
            assert torch.equal(a_, b_)
        sa, sb = opt2.state_dict(), opt.state_dict()
        for k in ('m', 'v', 'vhat'):
            assert len(sa[k]) == len(sb[k]) == len(pm._slots)
            for a_, b_ in zip(sa[k], sb[k]):
                assert torch.equal(a_, b_)
    same_state()
    assert float(opt2.vhat.abs().sum()) > 0
    state = ckpt.reference_optimizer_state(prefix)
    assert state['t'] == 2 and all(np.array_equal(a_, b_.numpy()) for a_, b_ in zip(state['vhat'], opt.state_dict()['vhat']))
    la, _ = trainvali.distributed_train_step(pm, b, opt, 2)
    lb, _ = trainvali.distributed_train_step(pm2, b, opt2, 2)
    assert la.numpy().tobytes() == lb.numpy().tobytes()
    same_state()
    # a net-only file: fine for inference (returns no step), refused -- before anything is overwritten -- with an optimizer
    ckpt.save_reference_checkpoint(pm, str(tmp_path / 'net'))
    pm3, opt3 = _trainable(256, seed=3)
    kept = pm3.flat_params.detach().clone()
    with pytest.raises(ValueError, match=r'net_query_layer0/kernel/\.OPTIMIZER_SLOT/optimizer/m'):
        ckpt.restore_reference_checkpoint(pm3, str(tmp_path / 'net'), opt3)
    with pytest.raises(ValueError, match=r'OPTIMIZER_SLOT/optimizer/m'):
        ckpt.reference_optimizer_state(str(tmp_path / 'net'))
    assert torch.equal(pm3.flat_params.detach(), kept) and opt3.t == 0
    assert ckpt.restore_reference_checkpoint(pm3, str(tmp_path / 'net')) is None
    assert all(torch.equal(a_, b_) for a_, b_ in zip(pm3.bucket_to_variables(pm3.flat_params), pm.bucket_to_variables(pm.flat_params)))


@pytest.mark.parametrize('kw,why', [(dict(norm='layer'), 'gamma'), (dict(pool='avg'), 'upconv')])
def test_models_the_importer_refuses_are_refused(tmp_path, kw, why):
    """(9) norm layers with gamma / beta, nested Sequentials (upconv): NotImplementedError, and no file is left behind."""
    _, pm = G.make(32, 64, 32, **kw)
    with pytest.raises(NotImplementedError, match=why):
        ckpt.save_reference_checkpoint(pm, str(tmp_path / 'ckpt-1'))
    pm.build('cpu'); pm.register_trainable()
    with pytest.raises(NotImplementedError, match='not conv kernels / biases'):
        ckpt.ReferenceCheckpointManager(str(tmp_path)).save(pm, nlt_amd.optim.AdamAMSGrad(pm, 1e-3), 1)
    assert os.listdir(tmp_path) == []


def test_manager_keeps_numbers_prunes_and_resumes(tmp_path):
    """(10) three saves with max_to_keep = 2; the state file; a new manager continues the count; an empty directory."""
    pm, opt = _trainable(32)
    d = str(tmp_path / 'checkpoints')
    empty = ckpt.ReferenceCheckpointManager(d, max_to_keep=2)
    kept = (pm.flat_params.detach().clone(), pm.flat_params._version, pm._epoch[0])
    assert empty.latest_checkpoint is None and empty.checkpoints == []
    assert trainvali.resume_reference(empty, pm, opt) == 0
    assert torch.equal(pm.flat_params.detach(), kept[0]) and (pm.flat_params._version, pm._epoch[0]) == kept[1:] and opt.t == 0
    mgr = empty
    for step in (10, 20, 30):
        opt.t = step
        with torch.no_grad():
            pm.flat_params.add_(0.001)
        assert trainvali.save_reference(mgr, pm, opt, step) == os.path.join(d, 'ckpt-%d' % (step // 10))
    assert sorted(os.listdir(d)) == ['checkpoint', 'ckpt-2' + SHARD, 'ckpt-2.index', 'ckpt-3' + SHARD, 'ckpt-3.index']
    assert open(os.path.join(d, 'checkpoint')).read() == ('model_checkpoint_path: "ckpt-3"\nall_model_checkpoint_paths: "ckpt-2"\n'
                                                          'all_model_checkpoint_paths: "ckpt-3"\n')
    assert mgr.checkpoints == [os.path.join(d, 'ckpt-2'), os.path.join(d, 'ckpt-3')]
    again = ckpt.ReferenceCheckpointManager(d, max_to_keep=2)
    assert again.latest_checkpoint == os.path.join(d, 'ckpt-3') and again.checkpoints == mgr.checkpoints
    pm2, opt2 = _trainable(32, seed=2)
    assert trainvali.resume_reference(again, pm2, opt2) == 30 and opt2.t == 30
    assert all(torch.equal(a_, b_) for a_, b_ in zip(pm2.bucket_to_variables(pm2.flat_params), pm.bucket_to_variables(pm.flat_params)))
    assert int(ckpt.read_bundle(again.latest_checkpoint)['save_counter' + V]) == 3
    assert again.save(pm2, opt2, 40) == os.path.join(d, 'ckpt-4')
    assert again.checkpoints == [os.path.join(d, 'ckpt-3'), os.path.join(d, 'ckpt-4')] and not os.path.exists(os.path.join(d, 'ckpt-2.index'))
    assert int(ckpt.read_bundle(again.latest_checkpoint)['save_counter' + V]) == 4
