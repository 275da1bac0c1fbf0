"""python -m deeploopcloser_amd.train_da train|transform -- DenoisingAutoencoderVariant.py's main (:262-309) on MI355X.

The reference's flags and defaults, then the port's (shared with train_sdav): --seed, --key_points {harris,grid},
--save PREFIX (PREFIX-<global_step>.npz after the fit), --load PATH (a DA .npz) and --out FILE (transform: the hidden
responses [frames*P, hidden_units] as .npy).  Files are visited in sorted order.  An empty dataset logs the reference's
message and exits 1.
"""
import sys
from argparse import ArgumentParser

from ._cli import add_port_arguments, add_reference_arguments, run


def build_parser():
    parser = ArgumentParser(description='Use this main file to train the network')
    add_reference_arguments(parser, stacked=False)
    add_port_arguments(parser)
    return parser


def main(argv=None):
    conf = build_parser().parse_args(argv)
    from .sdav import DA

    def make_model():
        return DA(conf.input_shape, conf.hidden_units, sparse_level=conf.sparse_level, sparse_penalty=conf.sparse_penalty,
                  consecutive_penalty=conf.consecutive_penalty, batch_size=conf.batch_size,
                  learning_rate=conf.learning_rate, epochs=conf.epochs, corruption_level=conf.corruption_level,
                  seed=conf.seed)
    return run(conf, make_model, lambda m, x: m.transform_tensor(x).cpu().numpy())


if __name__ == '__main__':
    sys.exit(main())
