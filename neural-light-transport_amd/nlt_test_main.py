"""The driver of the reference's nlt/nlt_test.py (:47-75,130-158) restated on `nlt_test.extract_feat` / `nlt_test.infer`:
config from the checkpoint's path, the net alone restored, observation features averaged over the first training batches, the
test set rendered and rolled up.  `python -m nlt_amd.nlt_test_main --ckpt <prefix>` calls `main`; the package also binds
`get_config_ini`, `make_datapipe`, `restore_model`, `run`, `parse_args` and `main` into `nlt_amd.nlt_test`, where the reference
keeps them (`nlt_test.run(...)`)."""
import argparse
import logging
from glob import glob
from os.path import basename, join

from . import nlt_test

logger = logging.getLogger('nlt_test')


def get_config_ini(ckpt):
    """nlt/nlt_test.py:47-48: `<outroot>/<xname>/checkpoints/ckpt-N` -> `<outroot>/<xname>.ini`, the copy `trainvali.run` left."""
    return '/'.join(ckpt.split('/')[:-2]) + '.ini'


def make_datapipe(mode, config, store=None, device='cuda', seed=None):
    """nlt/nlt_test.py:51-58.  The reference batches the test set by the config's `bs` too (datasets/base.py:61-73), which
    is what `--batch_size_override` acts on; `Dataset` alone defaults to one frame per test batch."""
    from .datasets import get_dataset_class
    dataset = get_dataset_class(config.get('DEFAULT', 'dataset'))(
        config, mode, store=store, k=config.getint('DEFAULT', 'k', fallback=1), device=device)
    dataset.bs = config.getint('DEFAULT', 'bs')
    return dataset.build_pipeline(seed=seed, no_batch=config.getboolean('DEFAULT', 'no_batch'))


def restore_model(config, ckpt, device='cuda'):
    """nlt/nlt_test.py:61-75: the config's model, built, with the NET ALONE restored (`tf.train.Checkpoint(net=model)`,
    `.expect_partial()`: optimizer slots and step in the file are left unread) -- from a reference-format prefix `ckpt-N`, or
    from a native `ckpt-N.pt` file of `trainvali.save_checkpoint`."""
    from . import ckpt as ckptlib, trainvali
    from .models import get_model_class
    model = get_model_class(config.get('DEFAULT', 'model'))(config)
    model.build(device)
    model.register_trainable()
    if ckpt.endswith('.pt'):
        trainvali.restore_checkpoint(ckpt, model)
    else:
        ckptlib.restore_reference_checkpoint(model, ckpt)
    return model


def run(ckpt, batch_size_override=None, n_obs_batches=1, fps=24, store=None, device='cuda', lanes=1, config=None, seed=None):
    """`main` of nlt/nlt_test.py:130-158: the config beside the run's directory (`get_config_ini`; or `config`, parsed),
    the restored net, `extract_feat` over the first `n_obs_batches` training batches (<= 0: all), `infer` over the test set
    into `<ini[:-4]>/vis_test/<basename(ckpt)>_pred/batch<i>` and the compilation next to it.  Returns (model, outroot,
    view_at).  store: the resident capture (None: `load_store(data_root)`); lanes: `infer`'s batches in flight; seed: of the
    shuffle that decides WHICH training batches come first (None: drawn, as the reference's unseeded shuffle)."""
    from . import trainvali
    config_ini = get_config_ini(ckpt)
    if config is None:
        config = trainvali.read_config(config_ini)
    if batch_size_override is not None:
        config.set('DEFAULT', 'bs', str(batch_size_override))

    # Model
    model = restore_model(config, ckpt, device)

    # Datasets
    datapipe_train = make_datapipe('train', config, store, device, seed)
    datapipe_test = make_datapipe('test', config, store, device)

    # Extract features from observations
    feat_agg = nlt_test.extract_feat(model, datapipe_train, n_obs_batches)

    # Run inference on the test data
    outroot = join(config_ini[:-4], 'vis_test', basename(ckpt) + '_pred')
    nlt_test.infer(model, datapipe_test, feat_agg, outroot, lanes=lanes)

    # Compile all visualized batches into a consolidated view
    batch_vis_dirs = sorted(glob(join(outroot, '*')))
    outpref = outroot.rstrip('/')
    view_at = model.compile_batch_vis(batch_vis_dirs, outpref, 'test', fps=fps)
    logger.info("Compilation available for viewing at\n\t%s", view_at)
    return model, outroot, view_at


def parse_args(argv=None):
    """The reference's flags (nlt/nlt_test.py:33-41)."""
    p = argparse.ArgumentParser(prog='nlt_amd.nlt_test_main', description="Average observation features, then render the test set.")
    p.add_argument('--ckpt', default='/path/to/ckpt-100', help="path to checkpoint (prefix only)")
    p.add_argument('--batch_size_override', type=int, default=None,
                   help="use a batch size different than what was used during training")
    p.add_argument('--n_obs_batches', type=int, default=1, help="number of observation batches used for the observation path")
    p.add_argument('--fps', type=int, default=24, help="frames per second for the result video")
    return p.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    logging.basicConfig(level=logging.INFO)
    return run(args.ckpt, batch_size_override=args.batch_size_override, n_obs_batches=args.n_obs_batches, fps=args.fps)


if __name__ == '__main__':             # python -m nlt_amd.nlt_test_main: hand over to the package's own copy of this module
    from .nlt_test_main import main as _main
    _main()
