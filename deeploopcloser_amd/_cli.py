"""The argparse surface shared by the training CLIs (train_sdav: train-sdav.py, train_da: DenoisingAutoencoderVariant.py's
main): the reference's flags and defaults verbatim, then the port's own."""
import logging
import sys

import numpy as np


def add_reference_arguments(parser, stacked):
    """train-sdav.py:6-27 (stacked=True) / DenoisingAutoencoderVariant.py:262-285 (stacked=False), verbatim."""
    parser.add_argument('operation', choices=['train', 'transform'], help='Operation to perform')
    parser.add_argument('--dataset_dir', help='Path to the dataset directory', required=True)
    parser.add_argument('--dataset_ext', help='Extension of the image files in the dataset directory', required=True)
    parser.add_argument('--input_shape', help='Shape of the input layer', type=int, nargs=2, default=[30, 1681])
    if stacked:
        parser.add_argument('--hidden_units', help='Number of hidden units', type=int, nargs='+',
                            default=[2500, 2500, 2500, 2500, 2500])
    else:
        parser.add_argument('--hidden_units', help='Number of hidden units', type=int, default=2500)
    parser.add_argument('--batch_size', help='Batch size for training', type=int, default=10)
    parser.add_argument('--corruption_level', help='Percentage of input vector to corrupt', type=float, default=0.3)
    parser.add_argument('--sparse_penalty', help='Penalty weight for the sparsity constraint', type=float, default=1.0)
    parser.add_argument('--sparse_level', help='Threshold factor for the sparsity constraint', type=float, default=0.05)
    parser.add_argument('--consecutive_penalty', help='Penalty weight for consecutive constraint', type=float, default=0.2)
    parser.add_argument('--learning_rate', help='Learning rate', type=float, default=0.1)
    parser.add_argument('--epochs', help='Number of epochs to train each batch', type=int, default=100)
    parser.add_argument('--verbose', help='Verbosity level for operations', type=bool, default=True)


def add_port_arguments(parser):
    """Flags the reference does not have."""
    parser.add_argument('--seed', help='Seed of the initial weights and of the corruption masks', type=int, default=0)
    parser.add_argument('--key_points', help='Patch centres: the Harris detector (the stand-in for SURF) or a fixed grid',
                        choices=['harris', 'grid'], default='harris')
    parser.add_argument('--save', metavar='PREFIX', help='train: write the weights to PREFIX-... .npz', default=None)
    parser.add_argument('--load', metavar='PATH', help='Start from the weights in this .npz', default=None)
    parser.add_argument('--out', metavar='FILE', help='transform: write the descriptors to this .npy', default=None)


def dataset_pattern(conf):
    return ('%s/*.%s' % (conf.dataset_dir, conf.dataset_ext)).replace('*..', '*.').replace('//', '/')   # train-sdav.py:42


def key_points_fn(name, n_patches):
    if name == 'grid':
        from .input import grid_key_points
        return lambda shape: grid_key_points(shape, n_patches)
    return None


def run(conf, make_model, transform):
    """The operation on the model make_model() builds (an SDA or a DA): 0 on success, 1 on an empty dataset (checked
    before any device is touched)."""
    from glob import glob
    from .input import load_frames
    logging.basicConfig(format='%(asctime)s %(message)s', datefmt='%m/%d/%Y %H:%M:%S', stream=sys.stderr)
    pattern = dataset_pattern(conf)
    if not glob(pattern):
        logging.getLogger().error("Specified dataset is empty or could not find dataset")   # InputGenerator.py:21-23
        return 1
    model = make_model()
    logging.getLogger().setLevel(logging.INFO if conf.verbose else logging.WARNING)       # (after the model's own setting)
    frames = load_frames(pattern, conf.input_shape, key_points_fn(conf.key_points, conf.input_shape[0]),
                         device=model.engine.device)
    if conf.load:
        model.load_weights(conf.load)
    if conf.operation == 'train':
        model.checkpoint_file = conf.save
        model.fit_dataset(frames)
    else:
        d = transform(model, np.stack(frames))
        logging.info("descriptors %s" % (d.shape,))
        if conf.out:
            np.save(conf.out, d)
    return 0
