"""python -m deeploopcloser_amd.train_lsh DATASET_DIR [--pool vlad --codebook book.npz] [--pca pca.npz] --bits B [--seed S]
[--no-center] --save FILE [--weights W --pattern G]

Fits the model of loop_closure --hash: the dataset's frames (sorted) -> patches -> SDAV descriptors -> the frame
descriptor (their concatenation, or with --pool vlad their VLAD pooling over the codebook; with --pca its projection) ->
Lsh.fit -> FILE, an .npz with seed, n_bits, width and mean.  The hyperplanes are a function of the seed, the bits and
the width (lsh.lsh_planes) and are not stored; what is learned is the column mean the rows are centred by (--no-center:
none).  One line on stdout: the rows, the width, the bits, a code's bytes and whether the model centres.
"""
import argparse
import sys


def build_parser():
    ap = argparse.ArgumentParser(description="fit the sign-random-projection hash of the SDAV frame descriptors of a dataset")
    ap.add_argument("dataset_path")
    ap.add_argument("--pattern", default="*.ppm")
    ap.add_argument("--weights", help=".npz written by SDAV.save_weights")
    ap.add_argument("--pool", choices=["flatten", "vlad"], default=None)
    ap.add_argument("--codebook", default=None, metavar="FILE", help="with --pool vlad: the .npz written by train_vlad")
    ap.add_argument("--pca", default=None, metavar="FILE", help="hash the rows projected by the .npz written by train_pca")
    ap.add_argument("--bits", type=int, required=True, metavar="B")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--no-center", action="store_true")
    ap.add_argument("--batch", type=int, default=256, help="frames encoded per step")
    ap.add_argument("--save", required=True, metavar="FILE")
    return ap


def main(argv=None):
    ap = build_parser()
    args = ap.parse_args(argv)
    from . import _lib as L
    if not 1 <= args.bits <= L.DLC_LSH_MAX_BITS:
        ap.error("--bits must be 1..%d" % L.DLC_LSH_MAX_BITS)
    if not 0 <= args.seed < 1 << 64:
        ap.error("--seed must be 0..2^64-1")
    if args.batch < 1:
        ap.error("--batch must be >= 1")
    if (args.pool == "vlad") != (args.codebook is not None):
        ap.error("--pool vlad needs --codebook" if args.pool == "vlad" else "--codebook needs --pool vlad")
    from .loop_closure import _frame_files, describe_sdav, describe_sdav_compact
    try:
        files = _frame_files(args.dataset_path, args.pattern)
    except ValueError as err:
        ap.error(str(err))
    import torch
    from .lsh import Lsh
    from .sdav import SDAV
    net = SDAV()
    if args.weights:
        net.load_weights(args.weights)
    pool = compact = None
    if args.pool == "vlad":
        from .vlad import Vlad
        try:
            pool = Vlad.load(args.codebook)
        except (OSError, ValueError, KeyError) as err:
            ap.error("--codebook: %s" % err)
        if pool.width != net.hidden_units[-1]:
            ap.error("--codebook: its words are %d wide, the encoder's descriptors %d" % (pool.width, net.hidden_units[-1]))
    if args.pca is not None:
        from .pca import Pca
        try:
            compact = Pca.load(args.pca)
        except (OSError, ValueError, KeyError) as err:
            ap.error("--pca: %s" % err)
    describe = (lambda fs: describe_sdav(fs, net, pool=pool)) if compact is None else \
        (lambda fs: describe_sdav_compact(fs, net, pool=pool, pca=compact))
    try:
        rows = torch.cat([describe(files[lo:lo + args.batch]) for lo in range(0, len(files), args.batch)])
        h = Lsh(args.bits, seed=args.seed, center=not args.no_center).fit(rows)
    except ValueError as err:
        ap.error(str(err))
    h.save(args.save)
    print("lsh\trows\t%d\twidth\t%d\tbits\t%d\tbytes\t%d\tcentered\t%d" % (rows.shape[0], h.width, h.n_bits, h.dim, int(h.center)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
