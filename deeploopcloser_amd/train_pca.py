"""python -m deeploopcloser_amd.train_pca DATASET_DIR [--pool vlad --codebook book.npz] --components M [--no-whiten]
[--eps E] [--basis f32|f64] [--max-rows N --seed S] --save FILE [--weights W --pattern G]

Fits the model of loop_closure --pca: the dataset's frames (sorted) -> patches -> SDAV descriptors -> the frame
descriptor (their concatenation, or with --pool vlad their VLAD pooling over the codebook) -> Pca.fit -> FILE, an .npz
with mean, basis, variance, scale, whiten, eps and n_rows.  One line on stdout: the rows, the width, the components and
the share of the training rows' variance the kept components hold.  The fit is a function of the frames in their order,
the weights, the codebook and the seed.
"""
import argparse
import sys

import numpy as np


def build_parser():
    ap = argparse.ArgumentParser(description="fit the PCA (and whitening) of the SDAV frame descriptors of a dataset")
    ap.add_argument("dataset_path")
    ap.add_argument("--pattern", default="*.ppm")
    ap.add_argument("--weights", help=".npz written by SDAV.save_weights")
    ap.add_argument("--pool", choices=["flatten", "vlad"], default=None)
    ap.add_argument("--codebook", default=None, metavar="FILE", help="with --pool vlad: the .npz written by train_vlad")
    ap.add_argument("--components", type=int, required=True, metavar="M")
    ap.add_argument("--no-whiten", action="store_true")
    ap.add_argument("--eps", type=float, default=0.0)
    ap.add_argument("--basis", choices=["f64", "f32"], default="f64")
    ap.add_argument("--max-rows", type=int, default=4096)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--batch", type=int, default=256, help="frames encoded per step")
    ap.add_argument("--save", required=True, metavar="FILE")
    return ap


def main(argv=None):
    ap = build_parser()
    args = ap.parse_args(argv)
    from . import _lib as L
    if not 1 <= args.components <= L.DLC_PCA_MAX_COMPONENTS:
        ap.error("--components must be 1..%d" % L.DLC_PCA_MAX_COMPONENTS)
    if not (args.eps >= 0.0 and np.isfinite(args.eps)):
        ap.error("--eps must be finite and >= 0")
    if args.max_rows < 2:
        ap.error("--max-rows must be >= 2")
    if args.batch < 1:
        ap.error("--batch must be >= 1")
    if (args.pool == "vlad") != (args.codebook is not None):
        ap.error("--pool vlad needs --codebook" if args.pool == "vlad" else "--codebook needs --pool vlad")
    from .loop_closure import _frame_files, describe_sdav
    try:
        files = _frame_files(args.dataset_path, args.pattern)
    except ValueError as err:
        ap.error(str(err))
    import torch
    from .pca import Pca
    from .sdav import SDAV
    net = SDAV()
    if args.weights:
        net.load_weights(args.weights)
    pool = None
    if args.pool == "vlad":
        from .vlad import Vlad
        try:
            pool = Vlad.load(args.codebook)
        except (OSError, ValueError, KeyError) as err:
            ap.error("--codebook: %s" % err)
        if pool.width != net.hidden_units[-1]:
            ap.error("--codebook: its words are %d wide, the encoder's descriptors %d" % (pool.width, net.hidden_units[-1]))
    rows = torch.cat([describe_sdav(files[lo:lo + args.batch], net, pool=pool) for lo in range(0, len(files), args.batch)])
    p = Pca(args.components, whiten=not args.no_whiten, eps=args.eps, basis=args.basis, max_rows=args.max_rows, seed=args.seed)
    try:
        p.fit(rows)
    except ValueError as err:
        ap.error(str(err))
    p.save(args.save)
    total = p.total_variance_                    # of the rows the fit took: the trace of their covariance
    print("pca\trows\t%d\twidth\t%d\tcomponents\t%d\tvariance_kept\t%.17g"
          % (p.n_rows, p.width, p.dim, float(p.explained_variance_.sum()) / total if total > 0 else 0.0))
    return 0


if __name__ == "__main__":
    sys.exit(main())
