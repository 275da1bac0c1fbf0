"""deeploopcloser_amd -- MI355X-native loop-closure descriptor-and-match engine.

The hot path of nschejtman/deepLoopCloser (encode -> all-vs-all similarity ->
top-k match) as hand-written HIP kernels for gfx950 behind the C ABI of
include/dlc.h, with the reference's Python call surface on top:

    SDAV, DA, SDA                 (src/sdav/network; python -m deeploopcloser_amd.train_sdav / .train_da: the CLIs)
    CnnVtl                        (src/cnn_vtl/network)
    CvInputParser                 (src/sdav/input; key-points supplied by the caller)
    SimilarityCalculator          (src/sdav/similarity; + SimilarityStream: one new frame against the resident ones)
    DistanceCalculator            (src/cnn_vtl/similarity; + distance_rows: a rectangular set of pairs in one call;
                                   + CnnVtlKeyframeDatabase: k nearest by that distance, or the distance rows themselves)
    SeqSlam, DifferenceCalculator, SadKeyframeDatabase   (SeqSLAM's own front-end: patch-normalised grey thumbnails compared
                                   by the sum of absolute differences -- no weights; new)
        shift=S, width=w on them, on Engine.sad_rows and on SeqSlamLoopClosureDetector: the best of the lateral shifts -S .. S
    Ldb, HammingCalculator, HammingKeyframeDatabase, LdbLoopClosureDetector   (a binary place descriptor: the global LDB code of
                                   a grey thumbnail, 64 bytes a frame, compared by Hamming distance -- no weights; new)
    MathUtils                     (src/utils/MathUtils.py)
    tensor_wrapper (tw)           (src/utils/TensorflowWrapper.py)
    encode / match / match_topk   (BASELINE.json north_star; new)
    sequence_topk / sequence_scores / slope_offsets / contrast_normalize   (sequence-consistent search over a score matrix; new)
        steps=(d_min, d_max) on them and on the detectors: the elastic search, a chain that steps back d_min..d_max key-frames per frame
    sequence_chains (and chains=True on sequence_topk / sequence_peaks / the detectors): the L matched key-frames behind a candidate; new
    peak_topk / sequence_peaks / uniqueness_ratio   (distinct-place candidates: picks more than `suppress` columns apart; new)
    LoopClosureDetector, SdavLoopClosureDetector, CnnVtlLoopClosureDetector, SeqSlamLoopClosureDetector   (streaming; all take sequence=L, suppress=W)
    fuse_scores, FusedLoopClosureDetector   (multi-descriptor fusion: score rows normalised per row, weighted and summed; new)
    PlaceTracker, track_places (and track= on the detectors): a Viterbi filter over score rows with a "no loop" state -- the place per frame and the smoothed labelling of the traversal; new
    Vlad, vlad_frame_descriptors (and pool= on describe_sdav, loop_closure --pool vlad; python -m deeploopcloser_amd.train_vlad): a k-means codebook of patch descriptors and VLAD pooling -- one orderless row per frame in front of KeyframeDatabase; new
    Pca (and loop_closure.describe_sdav_compact(pool=, pca=), pca= on sdav_place_descriptors_from_frames, loop_closure --pca; python -m deeploopcloser_amd.train_pca): PCA and whitening of a pooled row down to the <= 4096 columns the cosine top-k stores, by a projection whose sum order is stated -- the same bits alone or in a batch; new
    Lsh, lsh_planes, HashedLoopClosureDetector (and Engine.lsh_quantize / lsh_hash, loop_closure --hash; python -m deeploopcloser_amd.train_lsh): sign-random-projection hashes -- a float descriptor scaled to int8, the signs of its exact integer products with seeded +-1 hyperplanes on the int8 matrix cores, packed: a deep descriptor at 128 bytes a key-frame on the Hamming path; new
    GeometricVerifier, verify_candidates (and Engine.verify_pairs, loop_closure --verify): geometric verification of loop candidates -- the frames' patches matched, every two-match similarity of the matched key-points tried in integer arithmetic, the agreeing matches counted: exact, a function of the pair alone; new
    ground_truth / pr_curve_cells / recall_at / pr_curve_queries / PRCurve / LoopClosureEvaluator   (ground-truth evaluation: PR curves, average precision, recall@K; new)

Importing the package is cheap and works without a GPU; constructing any of
the classes needs libdlc_hip.so and a visible MI355X and raises otherwise.
"""
from . import _lib
from .math_utils import MathUtils
from .engine import Engine, default_engine
from .sdav import SDAV, DA
from .sda import SDA
from .cnn_vtl import CnnVtl
from .similarity import SimilarityCalculator, SimilarityStream
from .distance import DistanceCalculator, CnnVtlKeyframeDatabase
from .seqslam import SeqSlam, DifferenceCalculator, SadKeyframeDatabase
from .ldb import Ldb, HammingCalculator, HammingKeyframeDatabase
from .matching import encode, match, match_topk, KeyframeDatabase, MatchPipeline, flatten_frame_descriptors, vlad_frame_descriptors
from .dist import ShardedKeyframeDatabase, shard_bounds, merge_topk_torch
from .input import CvInputParser, KeyPoint, grid_key_points, harris_key_points, read_ppm
from . import tensor_wrapper
from . import sequence
from .sequence import slope_offsets, sequence_topk, sequence_scores, sequence_chains, contrast_normalize, peak_topk, sequence_peaks, uniqueness_ratio
from .loop_closure import LoopClosureDetector, SdavLoopClosureDetector, CnnVtlLoopClosureDetector, SeqSlamLoopClosureDetector
from .loop_closure import LdbLoopClosureDetector
from .loop_closure import FusedLoopClosureDetector
from . import fusion
from .fusion import fuse_scores
from . import tracking
from .tracking import PlaceTracker, track_places
from . import vlad
from .vlad import Vlad
from . import pca
from .pca import Pca
from . import lsh
from .lsh import Lsh, lsh_planes
from .loop_closure import HashedLoopClosureDetector
from . import verification
from .verification import GeometricVerifier, verify_candidates
from . import evaluate
from .evaluate import ground_truth, pr_curve_cells, recall_at, pr_curve_queries, PRCurve, LoopClosureEvaluator

__all__ = ["Lsh", "lsh_planes", "HashedLoopClosureDetector", "Ldb", "HammingCalculator", "HammingKeyframeDatabase", "LdbLoopClosureDetector", "GeometricVerifier", "verify_candidates", "Pca", "Vlad", "vlad_frame_descriptors", "PlaceTracker", "track_places", "fuse_scores", "FusedLoopClosureDetector", "ground_truth", "pr_curve_cells", "recall_at", "pr_curve_queries", "PRCurve", "LoopClosureEvaluator", "slope_offsets", "sequence_topk", "sequence_scores", "sequence_chains", "contrast_normalize", "peak_topk", "sequence_peaks", "uniqueness_ratio", "LoopClosureDetector", "SdavLoopClosureDetector", "CnnVtlLoopClosureDetector", "SeqSlamLoopClosureDetector", "SeqSlam", "DifferenceCalculator", "SadKeyframeDatabase", "CnnVtlKeyframeDatabase", "SimilarityStream", "SDAV", "DA", "SDA", "CnnVtl", "SimilarityCalculator", "DistanceCalculator", "MathUtils", "tensor_wrapper", "CvInputParser",
           "grid_key_points", "harris_key_points", "KeyPoint", "read_ppm",
           "encode", "match", "match_topk", "KeyframeDatabase", "MatchPipeline", "ShardedKeyframeDatabase", "Engine",
           "default_engine", "shard_bounds", "merge_topk_torch", "flatten_frame_descriptors"]
