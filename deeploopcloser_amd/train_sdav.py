"""python -m deeploopcloser_amd.train_sdav train|transform -- train-sdav.py on MI355X.

The reference's flags and defaults (train-sdav.py:6-27) and dataset pattern (:42), then the port's: --seed,
--key_points {harris,grid}, --save PREFIX (PREFIX-layer<i>.npz after each layer), --load PATH (an SDA .npz) and
--out FILE (transform: the descriptors [frames*P, hidden_units[-1]] as .npy).  train fits an SDA greedily
(deeploopcloser_amd.sda) and logs one loss line per batch; transform encodes the dataset through the stack (the
reference's transform does nothing).  Files are visited in sorted order.  An empty dataset logs the reference's message
and exits 1.
"""
import sys
from argparse import ArgumentParser

from ._cli import add_port_arguments, add_reference_arguments, run


def build_parser():
    parser = ArgumentParser(description='Use this main file to train the network')
    add_reference_arguments(parser, stacked=True)
    add_port_arguments(parser)
    return parser


def main(argv=None):
    conf = build_parser().parse_args(argv)
    from .sda import SDA

    def make_model():
        return SDA(conf.input_shape, conf.hidden_units, sparse_level=conf.sparse_level, sparse_penalty=conf.sparse_penalty,
                   consecutive_penalty=conf.consecutive_penalty, batch_size=conf.batch_size,
                   learning_rate=conf.learning_rate, epochs=conf.epochs, corruption_level=conf.corruption_level,
                   seed=conf.seed)
    return run(conf, make_model, lambda m, x: m.transform(x))


if __name__ == '__main__':
    sys.exit(main())
