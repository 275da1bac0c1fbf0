"""python -m deeploopcloser_amd.train_vlad DATASET_DIR --words K --iters I --seed S --save FILE [--weights W --pattern G]

Fits the codebook of loop_closure --pool vlad: the dataset's frames (sorted) -> patches -> SDAV descriptors -> Vlad.fit
-> FILE, an .npz with centroids [K, H], norm, seed and the inertia of every Lloyd step.  One line on stdout: the rows, the
words, the steps taken and the first and last inertia.  The fit is a function of the frames in their order, the
weights and the seed.
"""
import argparse
import sys

import numpy as np


def build_parser():
    ap = argparse.ArgumentParser(description="fit a VLAD codebook on the SDAV patch descriptors of a dataset")
    ap.add_argument("dataset_path")
    ap.add_argument("--pattern", default="*.ppm")
    ap.add_argument("--weights", help=".npz written by SDAV.save_weights")
    ap.add_argument("--words", type=int, default=16)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--norm", choices=["intra", "none"], default="intra")
    ap.add_argument("--batch", type=int, default=256, help="frames encoded per step")
    ap.add_argument("--save", required=True, metavar="FILE")
    return ap


def main(argv=None):
    ap = build_parser()
    args = ap.parse_args(argv)
    from . import _lib as L
    if not 1 <= args.words <= L.DLC_VLAD_MAX_WORDS:
        ap.error("--words must be 1..%d" % L.DLC_VLAD_MAX_WORDS)
    if args.iters < 1:
        ap.error("--iters must be >= 1")
    if args.batch < 1:
        ap.error("--batch must be >= 1")
    from .loop_closure import _frame_files, describe_sdav
    try:
        files = _frame_files(args.dataset_path, args.pattern)
    except ValueError as err:
        ap.error(str(err))
    import torch
    from .sdav import SDAV
    from .vlad import Vlad
    net = SDAV()
    if args.weights:
        net.load_weights(args.weights)
    p, h = net.input_shape[0], net.hidden_units[-1]
    if len(files) * p < args.words:
        ap.error("--words: %d words for the %d patches of %d frames" % (args.words, len(files) * p, len(files)))
    desc = torch.cat([describe_sdav(files[lo:lo + args.batch], net).view(-1, h) for lo in range(0, len(files), args.batch)])
    v = Vlad(n_words=args.words, norm=args.norm, seed=args.seed).fit(desc, iters=args.iters)
    v.save(args.save)
    print("codebook\trows\t%d\twords\t%d\twidth\t%d\tsteps\t%d\tinertia_first\t%.17g\tinertia_last\t%.17g"
          % (desc.shape[0], args.words, h, v.n_iter_, v.inertia_[0], v.inertia_[-1]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
