"""Streaming loop-closure queries over the resident top-k engine.

The reference stops at the all-vs-all matrices (create_similarity_matrix.py:29-38,
create_distance_matrix.py:30-36); what a SLAM front-end asks is the streaming form of the same
comparison: "does the frame that just arrived look like a place seen a while ago?".  A
LoopClosureDetector keeps every key-frame's descriptor resident in HBM (KeyframeDatabase.append),
matches each new frame against the key-frames more than `exclusion` frames older with the MFMA
top-k path and reports the candidates whose cosine score reaches `threshold`.

    python -m deeploopcloser_amd.loop_closure DATASET_DIR --network cnn_vtl --k 5 --threshold 0.9
    python -m deeploopcloser_amd.loop_closure DATASET_DIR --network seqslam --metric sad --sequence 10 --contrast 5

--network seqslam --metric sad is SeqSLAM itself, front to back and without weights: patch-normalised grey thumbnails
(--size, --patch, --strength), their sums of absolute differences, then the sequence search (SeqSlamLoopClosureDetector).

    python -m deeploopcloser_amd.loop_closure DATASET_DIR --network ldb --metric hamming --sequence 10

--network ldb --metric hamming is the binary route, also without weights: the global LDB code of a grey thumbnail (--size,
--levels; 64 bytes a frame by default), Hamming distances, then everything the seqslam route has behind its rows
(LdbLoopClosureDetector).

    python -m deeploopcloser_amd.loop_closure DATASET_DIR --network sdav --metric cosine --hash lsh.npz --sequence 10

--hash FILE (the model of python -m deeploopcloser_amd.train_lsh) takes the deep descriptor to the binary route: the frame
descriptor -- flattened or VLAD-pooled, PCA-projected or not -- is hashed by the signs of random projections (lsh.Lsh; 128
bytes a key-frame at 1024 bits) and searched by Hamming distance with everything the ldb route has behind its rows
(HashedLoopClosureDetector).

    python -m deeploopcloser_amd.loop_closure DATASET_DIR --fuse sad,distance --sequence 10

--fuse MEMBER,MEMBER[,...] (sad, distance, cosine) runs several descriptors side by side and ranks by ONE fused score:
each member's rows normalised (--fuse-norm zscore | minmax | none), weighted (--fuse-weights) and summed, higher is better
(FusedLoopClosureDetector; dlc_fuse_rows, include/dlc.h).  sad is SeqSLAM's thumbnails (--size, --patch, --strength,
--shift); distance and cosine share one CnnVtl forward per batch (--weights).

With --sequence L --chains every candidate line is followed by one line `chain<TAB>frame:key-frame<TAB>...`: the L pairs
the candidate was matched along, oldest frame first (the detectors' chains=True; dlc_sequence_chains /
dlc_sequence_elastic_chains, include/dlc.h).

With --positions FILE --radius R (one line of one or two integers per frame: where it was taken) the run is judged
against ground truth: after the stream one line `pr<TAB>queries<TAB>..<TAB>loops<TAB>..<TAB>ap<TAB>..<TAB>recall_at_p1
<TAB>..<TAB>best_f1<TAB>..<TAB>threshold<TAB>..` on stderr (evaluate.LoopClosureEvaluator over the best candidate of
every frame), and with --pr-curve OUT.tsv the whole curve.  stdout is unchanged.

Batching never changes a result: a batch of B frames is matched in one call against the longest
prefix any of its frames may see, each frame keeping to the key-frames old enough for IT inside the
selection (dlc_cosine_topk_older).  The same lists come from a match with k+B-1 candidates per frame
followed by each frame's first k candidates that are old enough (first_k_eligible below, the form
the engine call is tested against: at most B-1 of the extra rows are too recent for a frame).
"""
import argparse
import contextlib
import glob
import os
import sys
import time

import numpy as np
import torch

from . import _lib as L
from .matching import KeyframeDatabase


def first_k_eligible(scores, idx, limit, k):
    """Rows of (scores, idx) [B, kk] sorted best-first -> the first k entries per row whose id is
    below that row's limit [B], order kept; missing slots are (-inf, -1)."""
    ok = (idx >= 0) & (idx < limit.unsqueeze(1))
    order = torch.argsort((~ok).to(torch.int8), dim=1, stable=True)[:, :k]
    s, i, ok = scores.gather(1, order), idx.gather(1, order), ok.gather(1, order)
    s = torch.where(ok, s, torch.full_like(s, float("-inf")))
    i = torch.where(ok, i, torch.full_like(i, -1))
    if s.shape[1] < k:                                   # fewer candidates than k were requested
        pad = k - s.shape[1]
        s = torch.cat([s, s.new_full((s.shape[0], pad), float("-inf"))], 1)
        i = torch.cat([i, i.new_full((i.shape[0], pad), -1)], 1)
    return s, i


def _sequence_search(sequence, slopes, contrast, k, dtype, lower_is_better=False, suppress=None, steps=None, chains=False,
                     track=None, suppress_alone=False, length_alone=None):
    """A detector's sequence search (_SequenceRows over rows of `dtype`), or None without sequence=L -- what needs
    sequence=L is refused then; suppress_alone: `suppress` is not, the detector serves it; length_alone: the L that
    stands for sequence=None, the search is made all the same."""
    if sequence is None:
        if track is not None:
            raise ValueError("track needs sequence=L (L = 1 searches the frame scores themselves)")
        if chains:
            raise ValueError("chains needs sequence=L")
        if slopes is not None:
            raise ValueError("slopes needs sequence=L")
        if steps is not None:
            raise ValueError("steps needs sequence=L")
        if contrast is not None:
            raise ValueError("contrast needs sequence=L")
        if suppress is not None and not suppress_alone:
            raise ValueError("suppress needs sequence=L (L = 1 ranks by the frame scores themselves)")
        if length_alone is None:
            return None
        sequence = length_alone
    return _SequenceRows(sequence, slopes, k, dtype, contrast, lower_is_better, suppress, steps, chains, track)


def _loops(values, ids, first_id, limit, lower_is_better=False, chains=None):
    """[(frame id, matched frame id, value)] of the candidates whose value is at or above `limit` (at or below it with
    lower_is_better; None: every candidate), row by row, best first.  The value is a Python int where the values are
    integers, else a float.  chains [B, k, L] (a detector's third result with chains=True): every entry gains a fourth
    element, the candidate's L (frame id, key-frame id) pairs, oldest frame first -- the last pair is the entry's own."""
    v, i = values.cpu().numpy(), ids.cpu().numpy()
    ok = i >= 0
    if limit is not None:
        ok &= (v <= limit) if lower_is_better else (v >= limit)
    found = [(first_id + int(r), int(i[r, c]), v[r, c].item()) for r, c in zip(*np.nonzero(ok))]
    if chains is None:
        return found
    ch = chains.cpu().numpy()
    length = ch.shape[2]
    return [f + ([(f[0] - (length - 1) + t, int(ch[r, c, t])) for t in range(length)],)
            for f, (r, c) in zip(found, zip(*np.nonzero(ok)))]


class _StreamingDetector:
    """What every streaming detector is made of: the search options, checked and kept once; the sequence step; the result
    of frames that have no candidate; loops() and len().  A detector says where it differs with class attributes --

        ROW_DTYPE        the rows its kernels form and the sequence search sums: int64 or float64
        LOWER_IS_BETTER  the order of merit: distances (True) or scores
        LIMIT            its threshold's name: the keyword of its constructor and the attribute that holds it
        ALONE_DTYPE      the dtype of scores without sequence=L (float64; the cosine detector's float32)
        K_MAX            the largest k without sequence=L (None: any -- the SDAV detector's ranking of whole rows)
        SUPPRESS_ALONE   `suppress` is served without sequence=L too (the byte rows' peak selection, the fused rows)
        LENGTH_ALONE     the L that stands for sequence=None (the fused detector's 1; None: no sequence search then)

    -- creates its store (`_store`, what len() counts) and forms its rows.  The options are the same on all of them; what
    each does to the rows, launch by launch, is _SequenceRows' to tell:

    sequence = L (None: off, every path as it is without it; 1..64) asks whether the match holds over the last L frames: a
    pair (frame t, older frame j) is scored by the SUM of the L frame values along a line through (t, j) of the row
    matrix, the best over the lines of `slopes` (an int32 table [1..16, L]; default sequence.slope_offsets(L)), and the k
    best sums are the candidates (dlc_sequence_topk, include/dlc.h; Milford & Wyeth, ICRA 2012).  The detector keeps the
    last L - 1 rows resident in front of each batch's rows, so the lists do not depend on how the frames were batched;
    frame t's line may only touch values of frames old enough for the frame that produced them (row t - s offers the
    frames below t - s - exclusion), and a frame with fewer than L - 1 predecessors gets empty slots.  The detector's
    threshold is then compared with that SUM of L values, not with one value: a mean of 0.9 is threshold = 0.9 * L.

    contrast = R (None: off; needs sequence=L, R in 1..32): local contrast normalisation of the rows in front of the
    sequence search.  Values are then the float64 sums of L normalised values, the threshold is compared with that sum,
    and an empty slot is (-inf, -1) -- (+inf, -1) where lower is better.

    suppress = W (None: off; needs sequence=L, L = 1 allowed): the k candidates are k PLACES -- the best key-frame, then
    the best one more than W key-frames from it, and so on -- instead of one peak and its neighbours.  Values, dtypes and
    empty slots are as without it.

    steps = (d_min, d_max) (None: off; needs sequence=L, excludes slopes; 0 <= d_min <= d_max <= 8): the ELASTIC search --
    the best chain of L frame values that steps back d_min .. d_max key-frames from frame to frame, in place of the best
    straight line: a revisit whose speed changes inside the L frames (dlc_sequence_elastic_topk, include/dlc.h).  Values,
    dtypes, empty slots, contrast and suppress are as with the lines.

    chains = True (needs sequence=L; with or without contrast, suppress and steps): query_and_insert returns a third
    tensor, chain int32 [B, k, L] -- for every candidate the key-frame id each of the last L frames was matched to, oldest
    frame first; -1 where the slot is empty.  loops(..., chains=chain) lists them as pairs.

    track = {steps, jump, gate, null_score, history} (needs sequence=L, L = 1 allowed; on every detector that searches
    through _SequenceRows): a tracking.PlaceTracker runs over the same rows, after `contrast` and with the same limits.  It
    is `detector.tracker`: tracker.path() is the smoothed labelling of every frame so far.  query_and_insert returns what
    it returns without."""

    ROW_DTYPE, LOWER_IS_BETTER, LIMIT, ALONE_DTYPE = torch.int64, False, "threshold", torch.float64
    K_MAX, SUPPRESS_ALONE, LENGTH_ALONE = L.DLC_MAX_K, False, None

    def __init__(self, k, limit, exclusion, sequence, slopes, contrast, suppress, steps, chains, track):
        if self.K_MAX is None:
            if k < 1:
                raise ValueError("k must be >= 1")
        elif not 1 <= k <= self.K_MAX:
            raise ValueError("k=%d outside 1..%d" % (k, self.K_MAX))
        if exclusion < 0:
            raise ValueError("exclusion must be >= 0")
        if self.LOWER_IS_BETTER:                             # a distance: a whole number, behind `contrast` any number
            if limit is not None and limit < 0 and contrast is None:
                raise ValueError("%s must be >= 0 (or None)" % self.LIMIT)
            limit = limit if limit is None else (int if contrast is None else float)(limit)
        if self.SUPPRESS_ALONE and suppress is not None and not 0 <= suppress < 1 << 63:
            raise ValueError("suppress=%d outside 0..2^63-1" % suppress)      # (else _SequenceRows looks at it)
        self.k, self.exclusion = int(k), int(exclusion)
        setattr(self, self.LIMIT, limit)
        self.sequence = None if sequence is None else int(sequence)
        self.contrast = None if contrast is None else int(contrast)
        self.suppress = None if suppress is None else int(suppress)
        self.chains = bool(chains)
        self._seq = _sequence_search(self.sequence, slopes, self.contrast, self.k, self.ROW_DTYPE, self.LOWER_IS_BETTER,
                                     self.suppress, steps, self.chains, track, self.SUPPRESS_ALONE, self.LENGTH_ALONE)
        self.slopes = self.steps = self.tracker = None
        if self._seq is not None:
            self.slopes, self.steps, self.tracker = self._seq.slopes, self._seq.steps, self._seq.tracker

    def __len__(self):
        return len(self._store)

    def query_and_insert(self, descriptors):
        """The next B frames (ids len(self) .. len(self)+B-1) -> (values [B, k], ids [B, k] int64) on the device, best
        first, an empty slot where fewer than k key-frames are old enough; the frames are key-frames themselves
        afterwards.  With sequence=L a value is the sum of the L frame values along the best line.  With chains=True a
        third tensor, chain [B, k, L] int32.  What goes in, the values' dtype and the empty slot are the detector's."""
        raise NotImplementedError

    def _sequence_step(self, engine, b, first, capacity, fill):
        """sequence=L: frames first .. first + b - 1, frame first + r against the key-frames below first + r - exclusion.
        fill(out) forms their rows [b, first + b] with the detector's kernel where the search wants them -- behind the
        L - 1 rows before them -- and the search's lists are the step's."""
        fill(self._seq.raw_rows(b, capacity, engine)[:, :first + b])
        return self._seq.search(engine, b, first + b, first - self.exclusion)

    def _empty(self, b, device):
        """The result for b frames none of which has a candidate, (fill, -1) in every slot [b, k]: scores are -inf, float64
        with sequence=L and ALONE_DTYPE without; distances -1, int64, and behind `contrast` +inf, float64.  With chains
        the chain [b, k, L] too, -1 everywhere."""
        if not self.LOWER_IS_BETTER:
            fill, dtype = float("-inf"), self.ALONE_DTYPE if self.sequence is None else torch.float64
        elif self.contrast is not None:
            fill, dtype = float("inf"), torch.float64
        else:
            fill, dtype = -1, self.ROW_DTYPE
        out = (torch.full((b, self.k), fill, dtype=dtype, device=device),
               torch.full((b, self.k), -1, dtype=torch.int64, device=device))
        return out + (torch.full((b, self.k, self.sequence), -1, dtype=torch.int32, device=device),) if self.chains else out

    def loops(self, values, ids, first_id, chains=None):
        """[(frame id, matched key-frame id, value)] of the candidates at or above the detector's threshold -- at or below
        it where lower is better; all of them where it is None -- the value with sequence=L being the sum of the L frame
        values along the candidate's line.  chains: the third result of query_and_insert with chains=True -- every entry
        then ends in the candidate's L (frame id, key-frame id) pairs, oldest first."""
        return _loops(values, ids, first_id, getattr(self, self.LIMIT), self.LOWER_IS_BETTER, chains)


class LoopClosureDetector(_StreamingDetector):
    """The cosine detector: every new frame against the key-frames more than `exclusion` frames older, the k best by the
    cosine path's fp64 score (dlc_cosine_topk_older), candidates at or above `threshold`.  Without `sequence` that is the
    fused top-k, no score rows are formed, and scores are float32.

    The options are _StreamingDetector's.  With sequence=L the rows summed are the scores' ordering KEYS -- int64,
    round-half-even(score * 2^40), the integer the top-k itself ranks by (dlc_cosine_score_rows into a resident int64
    buffer that keeps the last L - 1 rows, then dlc_sequence_topk on int64): the sums are exact and free of summation
    order, the ranking (sum, then the older frame) is the top-k's own rule, and sequence=1 returns the ids of
    sequence=None index for index.  A frame with fewer than L - 1 predecessors gets (-inf, -1).  Scores are then float64,
    key sum * 2^-40 (exact), and `threshold` is compared with that SUM of L scores, not with one score, as the SDAV
    detector's is.  (Descriptors that hold a NaN or an infinity have the key INT64_MIN + 1; sums of several of them wrap.)
    With contrast=R there is no 2^-40 rescale, the keys' scale cancels, and an empty slot is (-inf, -1).  track= sees the
    int64 key rows, so jump, gate and null_score are integers in units of 2^-40."""

    ALONE_DTYPE = torch.float32

    def __init__(self, dim, k=5, threshold=0.9, exclusion=30, dtype="bf16", center=False, capacity=4096,
                 device=None, sequence=None, slopes=None, contrast=None, suppress=None, steps=None, chains=False, track=None):
        super().__init__(k, float(threshold), exclusion, sequence, slopes, contrast, suppress, steps, chains, track)
        self.db = self._store = KeyframeDatabase.empty(dim, capacity=capacity, dtype=dtype, center=center, device=device)

    @property
    def max_batch(self):
        """Largest number of frames one engine call takes (one 256-query tile of the score pass)."""
        return 256

    def query_and_insert(self, descriptors):
        """The next B frames' descriptors [B, dim] (ids len(self) .. len(self)+B-1) ->
        (scores [B,k] float32, ids [B,k] int64) on the device, best first, (-inf, -1) where fewer
        than k key-frames are old enough; the frames are then key-frames themselves.  With sequence=L the
        scores are float64: the sum of the L scores along the best line.  With chains=True a third tensor, chain
        [B, k, L] int32."""
        x = self.db._as_float(descriptors)
        if x.dim() != 2:
            raise ValueError("descriptors must be [B, dim]")
        outs = [self._step(x[lo:lo + self.max_batch]) for lo in range(0, x.shape[0], self.max_batch)]
        if not outs:
            return self._empty(0, self.db.engine.device)
        if len(outs) == 1:                                   # (torch.cat of one tensor is a copy: two launches per batch)
            return outs[0]
        return tuple(torch.cat(t) for t in zip(*outs))

    def _step(self, x):
        db, k = self.db, self.k
        b = x.shape[0]
        g0, _ = db.append(x)                               # normalised once, used as query and as key-frame
        g0 -= db.row_offset
        q = db.rows[g0:g0 + b]
        if self._seq is not None:
            s, i, *chain = self._sequence_step(db.engine, b, g0, db.capacity, lambda out: db.score_keys(
                q, limit0=g0 - self.exclusion, limit_step=1, out=out))
            if self.contrast is not None:                    # fp64 sums of normalised values as they are
                return (s, i, *chain)
            # key sums -> scores: |sum| < 2^53 for L <= 64, so the conversion and the power of two are exact
            return (torch.where(i >= 0, s.to(torch.float64) * 2.0 ** -40, float("-inf")), i, *chain)
        n_search = g0 + b - 1 - self.exclusion             # what the newest frame of the batch may see
        if n_search <= 0:
            return self._empty(b, db.engine.device)
        # one score pass over what the newest frame may see; frame j of the batch keeps to the rows below g0 - exclusion + j
        # (dlc_cosine_topk_older -- the lists of a k + b - 1 match followed by dlc_topk_keep_older / first_k_eligible)
        return db.engine.match_topk(q, db.rows[:n_search], k, older_than=g0 - self.exclusion)


class _SequenceRows:
    """The resident score rows of a detector with sequence=L: a [L - 1 + batch, ld] buffer of `dtype` whose first L - 1
    rows are the context -- the score rows of the L - 1 frames before the batch -- and whose next rows receive the
    batch's.  ld is the store's capacity, so a row never moves while the store does not grow.  It also holds what the
    sequence search of those rows takes, checked: `slopes`, an int32 table [1..16, L] (default sequence.slope_offsets(L)),
    and a k within the search's range.  A detector gets the batch's rows' destination (raw_rows), fills them with its own
    kernel and calls search().

    contrast = R (1..32) puts SeqSLAM's local contrast normalisation in front of the sequence search: the batch's raw
    rows, of `dtype`, go into an engine workspace (raw_rows), dlc_contrast_rows (include/dlc.h) writes every cell as
    (x - mean) / std over the R key-frames on either side of it, within the frame's own row and what it may see, behind
    the context rows (normalise) -- the buffer is float64 then -- and the lines are summed over that.  A stretch of
    key-frames that resembles every frame goes flat; a true revisit stands out from its neighbours.  A row's
    normalisation depends on that row alone, so the context rows stay valid and the lists still do not depend on the
    batching.

    steps = (d_min, d_max) (0 <= d_min <= d_max <= 8; excludes `slopes`) makes the search elastic: the best chain of L
    cells that steps back d_min .. d_max key-frames per frame instead of the best straight line
    (dlc_sequence_elastic_topk, include/dlc.h) -- the same window, limits, first output row, dense scores and poison
    word, and a cell still depends on the L rows behind it alone.

    suppress = W (>= 0) makes the k candidates distinct places: the sequence search writes the batch's dense cell scores
    and dlc_peak_topk_rows (include/dlc.h) picks from them -- the best cell, then the best one more than W key-frames
    from every earlier pick -- under the same limits, order of merit and poison word.  A dense score depends on the rows
    behind it alone, so these lists do not depend on the batching either.

    chains = True adds the candidates' chains: after the picks, over the same window, limits and order, the column each
    of the L frames of a candidate was matched to, oldest frame first (dlc_sequence_chains, with steps
    dlc_sequence_elastic_chains, include/dlc.h: one more launch, formed again for the k cells of every row alone, so the
    picks of `suppress` are served too).  A chain depends on the L rows behind its cell alone.

    track = a dict of tracking.PlaceTracker's options (steps, jump, gate, null_score, history) runs a place tracker
    beside the search: every batch's rows go through PlaceTracker.update exactly as the search reads them -- behind the
    contrast front, the same columns and limits, the detector's order of merit -- before the search itself.  `tracker` is
    that PlaceTracker (None without track=): tracker.path() is the smoothed labelling of every frame so far, last_place
    the filtered places of the last batch.  The search's lists are what they are without it."""

    def __init__(self, length, slopes, k, dtype, contrast=None, lower_is_better=False, suppress=None, steps=None, chains=False,
                 track=None):
        from .engine import check_steps
        from .sequence import slope_offsets
        if not 1 <= length <= 64:
            raise ValueError("sequence=%d outside 1..64" % length)
        if not 1 <= k <= L.DLC_MAX_K:
            raise ValueError("k=%d outside 1..%d" % (k, L.DLC_MAX_K))
        if steps is not None and slopes is not None:
            raise ValueError("steps and slopes exclude each other")
        self.steps, self.slopes = None if steps is None else check_steps(steps), None
        if self.steps is None:
            self.slopes = slope_offsets(length) if slopes is None else np.ascontiguousarray(slopes, dtype=np.int32)
            if self.slopes.ndim != 2 or self.slopes.shape[1] != length or not 1 <= self.slopes.shape[0] <= 16:
                raise ValueError("slopes must be an int32 table [1..16, %d]" % length)
        if contrast is not None and not 1 <= contrast <= 32:
            raise ValueError("contrast=%d outside 1..32" % contrast)
        if suppress is not None and not 0 <= suppress < 1 << 63:
            raise ValueError("suppress=%d outside 0..2^63-1" % suppress)
        self.length, self.k, self.lower_is_better, self.suppress = length, k, lower_is_better, suppress
        self.chains = bool(chains)
        self.contrast, self.raw_dtype, self._raw = contrast, dtype, None
        self._raw_item = torch.empty((), dtype=dtype).element_size()
        self.context, self.dtype, self.buf = length - 1, dtype if contrast is None else torch.float64, None
        self.tracker = self.last_place = None
        if track is not None:
            self.set_track(track)

    def set_track(self, track):
        """track=: the place tracker of these rows, before the first of them."""
        from .tracking import PlaceTracker
        if not isinstance(track, dict) or not set(track) <= {"steps", "jump", "gate", "null_score", "history"}:
            raise ValueError("track must be a dict of steps, jump, gate, null_score, history")
        if self.buf is not None:
            raise ValueError("track: the stream has begun")
        self.tracker = PlaceTracker(lower_is_better=self.lower_is_better, **track)
        return self.tracker

    def batch_rows(self, b, capacity, device):
        """Where the next batch's b score rows go: rows L - 1 .. L - 2 + b (the buffer is re-laid, the context kept, when
        the store has grown past its leading dimension or the batch is larger than any before)."""
        ctx, buf = self.context, self.buf
        if buf is None or buf.shape[1] < capacity or buf.shape[0] < ctx + b:
            new = torch.empty((ctx + max(b, 0 if buf is None else buf.shape[0] - ctx),
                               capacity if buf is None else max(capacity, buf.shape[1])), dtype=self.dtype, device=device)
            if buf is not None and ctx:
                new[:ctx, :buf.shape[1]] = buf[:ctx]
            self.buf = buf = new
        return buf[ctx:ctx + b]

    def raw_rows(self, b, capacity, engine):
        """Where the detector's kernels write the next batch's b rows, [b, capacity]: the buffer's own rows, or with
        contrast=R a workspace of the raw type (the current stream's, as the rows' consumers are)."""
        if self.contrast is None:
            return self.batch_rows(b, capacity, engine.device)
        size = b * capacity * self._raw_item
        self._raw = engine.workspace("contrast_raw", size)[:size].view(self.raw_dtype).view(b, capacity)
        return self._raw

    def normalise(self, engine, n, limit0):
        """contrast=R: the raw rows' first n columns, row r offering limit0 + r of them, normalised into the buffer's
        batch rows (one launch on the current stream).  Without contrast the rows are already there."""
        if self.contrast is not None:
            raw = self._raw
            engine.contrast_rows(raw[:, :n], self.contrast, limit0=limit0, limit_step=1,
                                 out=self.batch_rows(raw.shape[0], raw.shape[1], engine.device)[:, :n])

    def window(self, b):
        """The context rows and the batch's b rows behind them: what the sequence search reads."""
        return self.buf[:self.context + b]

    def advance(self, b):
        """The last L - 1 rows of the window become the next batch's context."""
        ctx, buf = self.context, self.buf
        if ctx:
            keep = buf[b:b + ctx]
            buf[:ctx] = keep.clone() if b < ctx else keep             # (source and destination overlap for short batches)

    def track(self, engine, b, n, limit0):
        """track=: the batch's b rows, as the search is about to read them, through the place tracker."""
        if self.tracker is not None:
            self.tracker.engine = engine
            self.last_place = self.tracker.update(self.buf[self.context:self.context + b], n=n, limit0=limit0, limit_step=1)[0]

    def search(self, engine, b, n, limit0, poison=None):
        """(values [b, k], ids [b, k]) of the batch's b frames, whose raw rows are written: over the first n columns, the
        batch's row r offering limit0 + r of them and every context row one fewer than the row behind it (matrix row m
        is the frame L - 1 - m before the batch's first; rows of frames before the stream began offer nothing and are never
        read).  With chains a third tensor, chain [b, k, L] int32.  Then the last L - 1 rows become the next batch's
        context."""
        self.normalise(engine, n, limit0)
        self.track(engine, b, n, limit0)
        search = engine.sequence_topk if self.steps is None else engine.sequence_elastic_topk
        s, i, _, dense = search(self.window(b), self.length, self.slopes if self.steps is None else self.steps,
                                k=self.k if self.suppress is None else None, row0=self.context, n=n,
                                limit0=limit0 - self.context, limit_step=1, lower_is_better=self.lower_is_better,
                                dense=self.suppress is not None, poison=poison)
        if self.suppress is not None:                              # k places: picks more than `suppress` key-frames apart
            s, i = engine.peak_topk_rows(dense, self.k, self.suppress, limit0=limit0, limit_step=1,
                                         lower_is_better=self.lower_is_better,
                                         absent=-1 if dense.dtype == torch.int64 else None, poison=poison)
        chain = ()
        if self.chains:                                            # the alignment behind every pick, over the same window
            form = engine.sequence_chains if self.steps is None else engine.sequence_elastic_chains
            chain = form(self.window(b), self.length, self.slopes if self.steps is None else self.steps, i, row0=self.context,
                         n=n, limit0=limit0 - self.context, limit_step=1, lower_is_better=self.lower_is_better,
                         poison=poison)[:1]
        self.advance(b)
        return (s, i, *chain)


class SdavLoopClosureDetector(_StreamingDetector):
    """The same question asked with the REFERENCE's similarity (SimilarityCalculator.similarity_score,
    src/sdav/similarity/SimilarityCalculator.py:12-49) instead of the cosine of flattened descriptors: every new frame's
    [P, H] SDAV descriptors are scored against all resident frames more than `exclusion` frames older through the
    streaming filter (similarity.SimilarityStream: the older frames' panel is resident, nothing is re-quantised), and the
    k best (score descending, ties -> the older frame) at or above `threshold` are the loop candidates.

    The options are _StreamingDetector's, over float64 score rows (without `sequence` the k best of a frame's row,
    dlc_topk_rows_f64, for any k; with it the search's own 1..DLC_MAX_K).  An empty slot is (-inf, -1), with contrast=R
    too.  What is this detector's own is the stream's POISON word: a poisoned stream answers (NaN, -1) in every slot --
    with contrast, suppress and steps as without them -- and -1 in every cell of a chain; submit() / result() launch the
    contrast normalisation on the stream of the rows' consumers, and with chains=True result() returns the third tensor
    as query_and_insert does."""

    ROW_DTYPE, K_MAX = torch.float64, None

    def __init__(self, score_source, patches=30, width=2500, k=5, threshold=float("-inf"), exclusion=30, capacity=1024,
                 device=None, sequence=None, slopes=None, contrast=None, suppress=None, steps=None, chains=False, track=None,
                 **stream_args):
        from .similarity import SimilarityStream
        super().__init__(k, float(threshold), exclusion, sequence, slopes, contrast, suppress, steps, chains, track)
        self._slots, self._pending, self._tickets = [{}, {}], None, 0      # submit() / result(): two batches in flight
        self.stream = self._store = SimilarityStream(score_source, patches=patches, width=width, capacity=capacity,
                                                     device=device, **stream_args)

    def query_and_insert(self, frames):
        """frames [B, P, H] (ids len(self) .. + B - 1) -> (scores [B, k] float64, ids [B, k] int64) on the device, best first,
        (-inf, -1) where fewer than k frames are old enough; the frames are resident afterwards.  A POISONED stream (a value
        outside its fixed range or a NaN was appended, now or earlier: `poisoned`, SimilarityStream.stats[1]) returns
        (NaN, -1) in every slot -- "these scores mean nothing", visible in the tensors themselves without a host read;
        loops() raises.  With chains=True a third tensor, chain [B, k, L] int32."""
        if self._pending is not None:                                 # a submitted batch's rows are ranked before this one's,
            self._flush()                                             # and nothing is in flight when the stream grows
        st = self.stream
        eng = st.engine
        x = eng.to_device(frames, torch.float64)
        if x.dim() == 2:
            x = x.unsqueeze(0)
        b = x.shape[0]
        first = st.append(x)                                          # all B frames become resident: one quantisation launch
        if first + b - 1 == 0:                                        # the very first frame alone: nothing older
            if self._seq is not None:                                 # (its row offers nothing, and is context all the same)
                self._seq.batch_rows(b, st.capacity, eng.device)
                self._seq.track(eng, b, 1, 0)                         # (the tracker counts every frame)
                self._seq.advance(b)
            return self._nothing_older(b)
        # frame first + r against every older frame, all B of them in one pair of launches (dlc_sdav_stream_query_batch):
        # rows[r, :first + r]
        if self._seq is None:
            rows = st.query_batch(first, b)
        else:
            rows = eng.sdav_stream_query_batch(st.state, st.desc, first, b, st.score, st.a, st.b,
                                               out=self._seq.raw_rows(b, st.capacity, eng), stats=st.stats)
        return self._rank(rows, first, b)

    def _rank(self, rows, first, b):
        """The lists of stream frames first .. first + b - 1 from their score rows -- one launch for the batch, which reads
        the stream's poison word and answers (NaN, -1) everywhere when it is set.  Without sequence=L the k best of the
        frames old enough (dlc_topk_rows_f64: score descending, ties -> the older frame); with it the rows sit where
        the search's raw_rows put them, and the last L - 1 of them become the next batch's context."""
        if self._seq is None:
            return self.stream.engine.topk_rows_f64(rows, first - self.exclusion, 1, self.k, poison=self.poisoned)
        return self._seq.search(self.stream.engine, b, first + b - 1, first - self.exclusion, poison=self.poisoned)

    def _nothing_older(self, b):
        """(-inf, -1) in every slot of b frames' lists; (NaN, -1) once the stream is poisoned."""
        s, *rest = self._empty(b, self.stream.engine.device)
        return (torch.where(self.poisoned != 0, float("nan"), s), *rest)

    # ---- two batches in flight ------------------------------------------------------------------------------------------
    # query_and_insert runs a batch's six launches one behind the other: copy, quantisation, the strip's product kernel (200
    # of the 275 us at 32 frames against 1063), resolution, scores, ranking.  Only the product kernel needs the whole chip.
    # submit() / result() give it the engine's second stream to itself and keep the rest on the caller's: batch b's copy +
    # quantisation run beside batch b - 1's products, batch b - 1's resolution + scores + ranking beside batch b's (what
    # may run beside what: include/dlc.h, dlc_sdav_stream_query_batch_staged).  Everything the caller touches -- the frames
    # going in, the lists coming out -- lives on the caller's stream; the second stream only ever carries product kernels.
    # The lists are the lists query_and_insert returns, bit for bit.
    PIPELINE_MIN_BATCH = 8                                            # below it there is no strip (include/dlc.h)

    def submit(self, frames):
        """frames [B, P, H] -> ticket.  The frames become resident; result(ticket) hands out (scores [B, k], ids [B, k]) --
        to be fetched before the second submit() after this one (a slot's buffers are reused then).  Batches of fewer than
        8 frames, the very first batch and a batch that makes the stream grow go through query_and_insert (no overlap)."""
        st, eng = self.stream, self.stream.engine
        x = eng.to_device(frames, torch.float64)
        if x.dim() == 2:
            x = x.unsqueeze(0)
        if x.dim() != 3 or x.shape[1] != st.p or x.shape[2] != st.h:       # (before a ticket is spent on it)
            raise ValueError("frames must be [B, %d, %d]" % (st.p, st.h))
        b, first = x.shape[0], len(st)
        t = self._tickets
        self._tickets += 1
        main, side = torch.cuda.current_stream(eng.device), eng.side_stream
        slot = self._slots[t % 2]
        if b < self.PIPELINE_MIN_BATCH or first == 0 or first + b > st.capacity:
            self._flush()                                              # (a growing stream re-quantises everything: nothing in flight)
            main.wait_stream(side)
            slot.update({"ticket": t, "out": self.query_and_insert(x)})
            return t
        need = eng.lib.dlc_sdav_stream_query_batch_workspace_bytes(st.capacity, st.p, b)
        if slot.get("ws") is None or slot["ws"].numel() < need:
            slot["ws"] = torch.empty(int(need), dtype=torch.uint8, device=eng.device)
        if slot.get("rows") is None or slot["rows"].shape[0] < b or slot["rows"].shape[1] < st.capacity:
            slot["rows"] = torch.empty((b, st.capacity), dtype=torch.float64, device=eng.device)
        st.append(x)                                                   # copy + quantisation: beside the previous batch's products
        quantised = torch.cuda.Event()
        quantised.record(main)                                         # (also behind the last use of this slot's buffers, two tickets ago)
        side.wait_event(quantised)
        rows = slot["rows"][:b]
        eng.sdav_stream_query_batch_staged(st.state, st.desc, first, b, st.score, 1, rows, slot["ws"], st.a, st.b, stats=st.stats,
                                           stream=side)
        products = torch.cuda.Event()
        products.record(side)
        self._flush()                                                  # the previous batch's second half: beside this batch's products
        slot.update({"ticket": t, "first": first, "b": b, "products": products, "out": None})
        self._pending = t
        return t

    def _flush(self):
        """The second half of the batch whose products are in flight -- resolution + scores + ranking, on the caller's stream
        behind that batch's product kernel."""
        if self._pending is None:
            return
        st, eng = self.stream, self.stream.engine
        slot = self._slots[self._pending % 2]
        torch.cuda.current_stream(eng.device).wait_event(slot["products"])
        rows = slot["rows"][:slot["b"]] if self._seq is None else self._seq.raw_rows(slot["b"], st.capacity, eng)
        eng.sdav_stream_query_batch_staged(st.state, st.desc, slot["first"], slot["b"], st.score, 2, rows, slot["ws"], st.a, st.b,
                                           stats=st.stats)
        slot["out"] = self._rank(rows, slot["first"], slot["b"])
        self._pending = None

    def result(self, ticket):
        """(scores [B, k] float64, ids [B, k] int64) of a submitted batch, in the current stream's order; with chains=True
        (scores, ids, chain [B, k, L] int32)."""
        if not self._tickets - 2 <= ticket < self._tickets:
            raise ValueError("SdavLoopClosureDetector.result: ticket %r is not in flight" % (ticket,))
        if self._pending == ticket:
            self._flush()
        slot = self._slots[ticket % 2]
        if slot.get("ticket") != ticket or slot.get("out") is None:
            raise ValueError("SdavLoopClosureDetector.result: ticket %r is not in flight" % (ticket,))
        return slot["out"]

    @property
    def poisoned(self):
        """Device int64 [1] (a view of SimilarityStream.stats): non-zero once a descriptor value outside the stream's fixed
        range (or a NaN / infinity) has been appended.  No host synchronisation to look at it on the device."""
        return self.stream.stats[1:2]

    def _check_poison(self):
        if int(self.stream.stats[1]) != 0:
            raise RuntimeError("SdavLoopClosureDetector: a descriptor value outside the stream's fixed range (or a NaN / "
                               "infinity) was appended -- the filter's error bound does not hold, every later row is NaN; "
                               "create the stream with a value_range / column_centre that covers the data")

    def loops(self, scores, ids, first_id, chains=None):
        """[(frame id, older frame id, score)] at or above the threshold; raises when the stream has been poisoned (a value
        outside its fixed range: SimilarityStream.stats[1]).  chains: the third result of query_and_insert / result with
        chains=True -- every entry then ends in the candidate's L (frame id, older frame id) pairs, oldest first."""
        found = super().loops(scores, ids, first_id, chains)
        self._check_poison()
        return found


class _ByteRowsLoopClosureDetector(_StreamingDetector):
    """What the streaming detectors over byte descriptors and int64 lower-is-better rows share (CnnVtlLoopClosureDetector:
    cnn_vtl distance rows; SeqSlamLoopClosureDetector: SAD rows; LdbLoopClosureDetector: Hamming rows): the checks of the
    store's shape, query_and_insert and the path without `sequence` -- the batch's rows into a resident buffer, then the
    peak selection over them.  A subclass names its threshold (LIMIT), creates its database and forms the rows of a batch
    (_rows_into)."""

    LOWER_IS_BETTER, LIMIT, SUPPRESS_ALONE = True, None, True
    _rows = None                                             # without sequence: the batch's rows [b, capacity]

    def __init__(self, dim, k, limit, exclusion, capacity, sequence, slopes, contrast, suppress, steps, chains, track):
        super().__init__(k, limit, exclusion, sequence, slopes, contrast, suppress, steps, chains, track)
        if dim < 1 or capacity < 1:
            raise ValueError("dim and capacity must be positive")

    def _rows_into(self, q, limit0, out):
        """The rows of the stored queries q against the database, query r in its first limit0 + r cells, into out."""
        raise NotImplementedError

    def query_and_insert(self, descriptors):
        """The next B frames' byte descriptors [B, dim] (ids len(self) .. len(self)+B-1) -> (value [B, k] int64,
        ids [B, k] int64) on the device, nearest first, (-1, -1) where fewer than k frames are old enough; the frames are
        key-frames afterwards.  With sequence=L value is the sum of the L frame values along the best line.  With
        chains=True a third tensor, chain [B, k, L] int32."""
        db = self.db
        x = db.engine.to_device(descriptors)
        if x.dim() == 1:
            x = x.unsqueeze(0)
        first, _ = db.append(x)
        b = x.shape[0]
        if self._seq is None:
            return self._alone(first, b)
        if b == 0:
            return self._empty(0, db.engine.device)
        q = db.rows[first:first + b]
        return self._sequence_step(db.engine, b, first, db.capacity, lambda out: self._rows_into(q, first - self.exclusion, out))

    def _alone(self, first, b):
        """Without sequence=L: the rows of frames first .. first + b - 1, then the k picks of every row, more than
        `suppress` (None: 0) key-frames apart."""
        db = self.db
        if b == 0:
            return self._empty(0, db.engine.device)
        if self._rows is None or self._rows.shape[0] < b or self._rows.shape[1] < db.capacity:
            self._rows = torch.empty((b if self._rows is None else max(b, self._rows.shape[0]), db.capacity),
                                     dtype=torch.int64, device=db.engine.device)
        rows = self._rows[:b, :first + b]
        self._rows_into(db.rows[first:first + b], first - self.exclusion, rows)
        return db.engine.peak_topk_rows(rows, self.k, self.suppress or 0, limit0=first - self.exclusion, limit_step=1,
                                        lower_is_better=True)


class CnnVtlLoopClosureDetector(_ByteRowsLoopClosureDetector):
    """The streaming question asked with the REFERENCE's cnn_vtl measure (DistanceCalculator.calculate_distance,
    src/cnn_vtl/similarity/DistanceCalculator.py:4-12) instead of the cosine of the descriptors: every new frame's int8
    descriptor is compared with all resident frames more than `exclusion` frames older, and the k nearest (distance
    ascending, ties -> the older frame) at or below `max_distance` (all of them when None) are the loop candidates.
    A batch of B frames is one top-k launch: frame first + r sees the frames below first + r - exclusion
    (dlc_cnnvtl_distance_topk with limit_step = 1), so the lists do not depend on how the frames are batched.  That is the
    one path of its own -- the fused top-k, no distance rows are formed, and no `suppress` without `sequence`.

    The options are _StreamingDetector's, over int64 distance rows, the smallest sums the candidates
    (dlc_cnnvtl_distance_rows into a resident int64 buffer that keeps the last L - 1 rows, then dlc_sequence_topk with
    lower_is_better).  A frame with fewer than L - 1 predecessors gets (-1, -1).  max_distance is then compared with the
    sequence sum -- L distances, not one -- as the SDAV detector's threshold is with its sum of scores.  With contrast=R
    distances stay lower-is-better (the standard deviation is positive); dist is then float64, max_distance may be
    negative, and an empty slot is (+inf, -1).  With suppress=W, k = 2 and W = R_window / 2 the two distances are
    OpenSeqSLAM's min_value and min_value_2nd (sequence.uniqueness_ratio)."""

    LIMIT, SUPPRESS_ALONE = "max_distance", False

    def __init__(self, dim, k=5, max_distance=None, exclusion=30, capacity=4096, device=None, sequence=None, slopes=None,
                 contrast=None, suppress=None, steps=None, chains=False, track=None):
        super().__init__(dim, k, max_distance, exclusion, capacity, sequence, slopes, contrast, suppress, steps, chains,
                         track)
        from .distance import CnnVtlKeyframeDatabase
        self.db = self._store = CnnVtlKeyframeDatabase.empty(dim, capacity=capacity, device=device)

    def _rows_into(self, q, limit0, out):
        self.db.distances(q, limit0=limit0, limit_step=1, out=out)

    def _alone(self, first, b):
        """Without sequence=L: one fused top-k launch, no rows are formed (and none for b = 0 either)."""
        db = self.db
        return db.engine.cnnvtl_distance_topk(db.rows[first:first + b], db.rows, self.k, d=db.dim,
                                              limit0=first - self.exclusion, limit_step=1)




class SeqSlamLoopClosureDetector(_ByteRowsLoopClosureDetector):
    """The streaming question asked the way SeqSLAM asks it (Milford & Wyeth, ICRA 2012): every new frame's descriptor -- a
    patch-normalised grey thumbnail, uint8 [dim] (seqslam.SeqSlam) -- is compared with all resident frames more than
    `exclusion` frames older by the sum of absolute differences, and the k with the smallest difference (ties -> the older
    frame) at or below `max_difference` (all of them when None) are the loop candidates.  No weights are involved.

    Without `sequence` a batch's difference rows go into a resident int64 buffer (dlc_sad_u8_rows, frame first + r seeing
    the frames below first + r - exclusion) and dlc_peak_topk_rows picks from them, lower is better; suppress = W (default
    0: a plain top-k) keeps the picks more than W key-frames apart.  (-1, -1) where fewer than k frames are old enough.

    sequence = L is CnnVtlLoopClosureDetector(sequence=L) with these rows in place of the cnn_vtl distance rows: a pair
    (frame t, older frame j) is scored by the SUM of the L differences along a line through (t, j), the smallest over the
    lines of `slopes`; the detector keeps the last L - 1 rows resident (_SequenceRows: int64, lower_is_better), and
    contrast = R, suppress = W, steps = (d_min, d_max) and chains = True mean what they mean there -- with contrast the
    sums are float64 and an empty slot is (+inf, -1).  max_difference is then compared with the sequence sum.

    shift = S with width = w (the thumbnail's columns, dim a multiple of it; S in 0..min(DLC_MAX_SHIFT, w - 1)): every row
    formed, in either form, is the shifted row (dlc_sad_u8_shift_rows: the best of the lateral shifts -S .. S, on the
    plain SAD's scale), and everything behind the rows works on it unchanged.  The winning shifts are not returned here;
    db.differences(..., return_shift=True) gives them.

    In both forms the lists do not depend on how the frames are batched."""

    LIMIT = "max_difference"

    def __init__(self, dim, k=5, max_difference=None, exclusion=30, capacity=4096, device=None, sequence=None, slopes=None,
                 contrast=None, suppress=None, steps=None, chains=False, shift=None, width=None, track=None):
        super().__init__(dim, k, max_difference, exclusion, capacity, sequence, slopes, contrast, suppress, steps, chains,
                         track)
        if shift is not None and shift < 0:
            raise ValueError("shift=%d must be >= 0" % shift)
        if shift:                                            # (None or 0: the plain rows, as Engine.sad_rows takes them)
            if width is None:
                raise ValueError("shift needs width, the thumbnail's columns")
            if width < 1 or dim % width != 0:
                raise ValueError("dim=%d is not a multiple of width=%d" % (dim, width))
            if not 0 <= shift <= min(L.DLC_MAX_SHIFT, width - 1):
                raise ValueError("shift=%d outside 0..min(%d, width - 1 = %d)" % (shift, L.DLC_MAX_SHIFT, width - 1))
        self.shift = None if shift is None else int(shift)
        self.width = None if width is None else int(width)
        from .seqslam import SadKeyframeDatabase
        self.db = self._store = SadKeyframeDatabase.empty(dim, capacity=capacity, device=device)

    def _rows_into(self, q, limit0, out):
        self.db.differences(q, limit0=limit0, limit_step=1, out=out, shift=self.shift, width=self.width)


class LdbLoopClosureDetector(_ByteRowsLoopClosureDetector):
    """SeqSlamLoopClosureDetector over BINARY descriptors: every new frame's packed bits, uint8 [dim] (ldb.Ldb), are
    compared with all resident frames more than `exclusion` frames older by Hamming distance (dlc_hamming_rows), and the k
    with the smallest distance (ties -> the older frame) at or below `max_distance` (all of them when None) are the loop
    candidates.  No weights are involved, and a key-frame is dim bytes -- 64 for Ldb's defaults.

    Everything behind the rows is SeqSlamLoopClosureDetector's, word for word: without `sequence` dlc_peak_topk_rows over
    a resident int64 buffer (suppress = W keeps the picks more than W key-frames apart); sequence = L, slopes, contrast =
    R, suppress = W, steps = (d_min, d_max), chains = True and track as there, max_distance then compared with the
    sequence sum.  There is no lateral shift.  The lists do not depend on how the frames are batched."""

    LIMIT = "max_distance"

    def __init__(self, dim, k=5, max_distance=None, exclusion=30, capacity=4096, device=None, sequence=None, slopes=None,
                 contrast=None, suppress=None, steps=None, chains=False, track=None):
        super().__init__(dim, k, max_distance, exclusion, capacity, sequence, slopes, contrast, suppress, steps, chains,
                         track)
        from .ldb import HammingKeyframeDatabase
        self.db = self._store = HammingKeyframeDatabase.empty(dim, capacity=capacity, device=device)

    def _rows_into(self, q, limit0, out):
        self.db.distances(q, limit0=limit0, limit_step=1, out=out)


class HashedLoopClosureDetector(LdbLoopClosureDetector):
    """LdbLoopClosureDetector over the HASHES of float descriptors: every batch of rows [B, lsh.width] (float64, float32
    or bfloat16; NumPy or tensors) goes through `lsh` (lsh.Lsh: the mean taken off, int8, the signs of the products with
    its hyperplanes -- dlc_lsh_quantize_i8, dlc_lsh_hash_i8) and the codes, lsh.dim bytes a key-frame, through that
    detector's body as they are: a deep descriptor searched at the binary path's cost.  Every option is
    LdbLoopClosureDetector's, and so are the lists, those of that detector fed the same codes; max_distance is a Hamming
    distance (with sequence=L the sum along the line).  A code depends on its row and the model alone, so the lists do
    not depend on how the frames are batched."""

    def __init__(self, lsh, k=5, max_distance=None, exclusion=30, capacity=4096, device=None, sequence=None, slopes=None,
                 contrast=None, suppress=None, steps=None, chains=False, track=None):
        if getattr(lsh, "dim", None) is None or not hasattr(lsh, "transform_tensor"):
            raise ValueError("lsh must be an lsh.Lsh")
        super().__init__(lsh.dim, k=k, max_distance=max_distance, exclusion=exclusion, capacity=capacity, device=device,
                         sequence=sequence, slopes=slopes, contrast=contrast, suppress=suppress, steps=steps, chains=chains,
                         track=track)
        self.lsh = lsh

    def query_and_insert(self, descriptors):
        """The next B frames' float descriptors [B, lsh.width] -> what LdbLoopClosureDetector.query_and_insert returns for
        their codes."""
        x = descriptors if isinstance(descriptors, torch.Tensor) else np.asarray(descriptors)
        if x.ndim == 1:
            x = x[None]
        if x.shape[0] == 0:
            return super().query_and_insert(torch.empty((0, self.lsh.dim), dtype=torch.uint8, device=self.db.engine.device))
        return super().query_and_insert(self.lsh.transform_tensor(x))


FUSE_MEMBERS = ("cosine", "distance", "sad")
FUSE_NORMS = ("zscore", "minmax", "none")


class FusedLoopClosureDetector(_StreamingDetector):
    """The streaming question asked with SEVERAL descriptors at once: every member keeps its own key-frame store and
    forms its own raw rows per batch -- each new frame against the key-frames more than `exclusion` frames older -- and
    ONE dlc_fuse_rows (include/dlc.h) turns them into one row: each member's row normalised within itself (`norm`:
    "zscore", "minmax" or "none"), the sign of the distances turned, weighted (`weights`: None = all 1, or one finite
    number per member) and summed.  The fused row is float64 and higher is better; the k best cells are the candidates.
    A hand-crafted descriptor and a deep one fail in different places; what both agree on stands out of the sum.

    members: a list of specs, all on one engine --
        ("cosine", dim, {"dtype": "bf16", "center": False})   KeyframeDatabase, its fp64 cosine scores (scores_f64)
        ("distance", dim)                                     CnnVtlKeyframeDatabase, the cnn_vtl distance (distances)
        ("sad", dim, {"shift": S, "width": w})                SadKeyframeDatabase, SeqSLAM's SAD (differences)
    (the dict is optional).  query_and_insert takes one [B, dim_i] tensor per member, all with the same B.

    The fused rows go where the sequence search keeps its rows (_SequenceRows: float64, L = 1 when sequence is None, so
    suppress = W works without sequence, as in the SeqSLAM detector) and sequence = L, slopes, contrast = R,
    suppress = W, steps = (d_min, d_max) and chains = True mean what they mean in the other detectors.  A fused row
    depends on its frame's raw rows alone (the row sums of dlc_fuse_rows do not depend on the batch), so the lists do not
    depend on how the frames are batched.  Results are (scores float64 [B, k], ids int64 [B, k][, chain]), (-inf, -1)
    in empty slots; `threshold` (None: all k) is compared with the fused score -- with sequence=L the sum of L of them."""

    ROW_DTYPE, SUPPRESS_ALONE, LENGTH_ALONE = torch.float64, True, 1

    def __init__(self, members, weights=None, norm="zscore", k=5, threshold=None, exclusion=30, capacity=4096, device=None,
                 sequence=None, slopes=None, contrast=None, suppress=None, steps=None, chains=False):
        from .distance import CnnVtlKeyframeDatabase
        from .seqslam import SadKeyframeDatabase
        members = [tuple(m) if isinstance(m, (tuple, list)) else (m,) for m in members]
        if not 1 <= len(members) <= L.DLC_MAX_FUSE:
            raise ValueError("%d members outside 1..%d" % (len(members), L.DLC_MAX_FUSE))
        if capacity < 1:
            raise ValueError("capacity must be positive")
        if norm not in FUSE_NORMS:
            raise ValueError("norm=%r is none of %s" % (norm, ", ".join(FUSE_NORMS)))
        w = np.ones(len(members)) if weights is None else np.asarray(weights, dtype=np.float64).reshape(-1)
        if w.shape[0] != len(members) or not np.isfinite(w).all():
            raise ValueError("weights must be %d finite numbers" % len(members))
        super().__init__(k, None if threshold is None else float(threshold), exclusion, sequence, slopes, contrast, suppress,
                         steps, chains, None)                # (track: start_tracking)
        self.weights, self.norm = [float(v) for v in w], norm
        self.kinds, self.dbs, self._options = [], [], []
        for spec in members:
            if not 2 <= len(spec) <= 3 or spec[0] not in FUSE_MEMBERS:
                raise ValueError("a member is (kind, dim[, options]) with kind one of %s" % ", ".join(FUSE_MEMBERS))
            kind, dim, opt = spec[0], int(spec[1]), dict(spec[2]) if len(spec) == 3 and spec[2] else {}
            allowed = {"cosine": ("dtype", "center"), "distance": (), "sad": ("shift", "width")}[kind]
            if set(opt) - set(allowed):
                raise ValueError("member %s takes the options %s" % (kind, ", ".join(allowed) or "(none)"))
            if kind == "cosine":
                db = KeyframeDatabase.empty(dim, capacity=capacity, dtype=opt.get("dtype", "bf16"),
                                            center=opt.get("center", False), device=device)
            elif kind == "distance":
                db = CnnVtlKeyframeDatabase.empty(dim, capacity=capacity, device=device)
            else:
                shift, width = opt.get("shift"), opt.get("width")
                if shift:
                    if width is None or width < 1 or dim % width != 0:
                        raise ValueError("sad: shift needs width, the thumbnail's columns, with dim a multiple of it")
                    if not 0 <= shift <= min(L.DLC_MAX_SHIFT, width - 1):
                        raise ValueError("sad: shift=%d outside 0..min(%d, width - 1 = %d)" % (shift, L.DLC_MAX_SHIFT, width - 1))
                db = SadKeyframeDatabase.empty(dim, capacity=capacity, device=device)
            self.kinds.append(kind)
            self.dbs.append(db)
            self._options.append(opt)
        self._store, self.engine = self.dbs[0], self.dbs[0].engine
        self.lower_is_better = [kind != "cosine" for kind in self.kinds]

    def start_tracking(self, track):
        """What track= is on the other detectors (LoopClosureDetector), asked for before the first frame: a
        tracking.PlaceTracker over the fused rows, behind `contrast`, with the search's limits.  Returns it; it is
        `detector.tracker` from then on."""
        self.tracker = self._seq.set_track(track)
        return self.tracker

    def _member_rows(self, i, first, b, out):
        """Member i's raw rows of frames first .. first + b - 1 against the key-frames, each frame the ones old enough."""
        db, kind, lim = self.dbs[i], self.kinds[i], first - self.exclusion
        q = db.rows[first:first + b]
        if kind == "cosine":
            db.scores_f64(q, limit0=lim, limit_step=1, out=out)
        elif kind == "distance":
            db.distances(q, limit0=lim, limit_step=1, out=out)
        else:
            db.differences(q, limit0=lim, limit_step=1, out=out, shift=self._options[i].get("shift"),
                           width=self._options[i].get("width"))

    def query_and_insert(self, descriptors):
        """The next B frames, one descriptor tensor [B, dim_i] per member in the members' order (floats for cosine, int8
        for distance, uint8 for sad; ids len(self) .. len(self)+B-1) -> (scores [B, k] float64, ids [B, k] int64) on the
        device, best first, (-inf, -1) where fewer than k key-frames are old enough; the frames are key-frames
        afterwards.  With chains=True a third tensor, chain [B, k, L] int32."""
        descriptors = list(descriptors)
        if len(descriptors) != len(self.dbs):
            raise ValueError("query_and_insert: %d descriptor tensors for %d members" % (len(descriptors), len(self.dbs)))
        eng = self.engine
        xs = []
        for db, kind, x in zip(self.dbs, self.kinds, descriptors):
            x = db._as_float(x) if kind == "cosine" else eng.to_device(x)
            xs.append(x.unsqueeze(0) if x.dim() == 1 else x)
        b = int(xs[0].shape[0])
        if any(x.dim() != 2 or x.shape[0] != b for x in xs):
            raise ValueError("query_and_insert: every member's descriptors must be [B, dim] with one B")
        if b == 0:
            return self._empty(0, eng.device)
        first = len(self)
        for db, x in zip(self.dbs, xs):
            if db.append(x)[0] != first:
                raise RuntimeError("FusedLoopClosureDetector: the members' stores are out of step")
        capacity, n = max(db.capacity for db in self.dbs), first + b
        raws = []
        for i, kind in enumerate(self.kinds):
            dtype = torch.float64 if kind == "cosine" else torch.int64
            ws = eng.workspace("fuse_member_%d" % i, b * capacity * 8)[:b * capacity * 8]
            raws.append(ws.view(dtype).view(b, capacity)[:, :n])
            self._member_rows(i, first, b, raws[-1])
        return self._sequence_step(eng, b, first, capacity, lambda out: eng.fuse_rows(
            raws, weights=self.weights, lower_is_better=self.lower_is_better, norm=self.norm, limit0=first - self.exclusion,
            limit_step=1, out=out))


SDAV_CLI_PATCHES = 30       # patches of a frame of the CLI's SDAV: the concatenation is 30 * 2500 wide
SDAV_CLI_WIDTH = 2500       # columns of a patch descriptor of the CLI's SDAV: the reference's network (SDAV.py:31-32), --weights or not


def _frame_files(dataset_path, pattern):
    files = sorted(glob.glob(os.path.join(dataset_path, pattern)))
    if not files:
        raise ValueError("Specified dataset is empty or could not find dataset")        # InputGenerator.py:21-23
    return files


def describe_sdav(files, network=None, key_points_fn=None, pool=None):
    """Frames -> one [30*2500] place descriptor per frame (patches -> SDAV.transform, flattened), a DEVICE tensor: the
    uint8 frames go up once, grey / key-points / patches / encoder run back to back in HBM (pipeline.py).
    pool: a fitted vlad.Vlad -- the frame's patch descriptors are pooled into one orderless VLAD row [K * H] instead of
    being concatenated; None: the concatenation, as ever."""
    desc = _describe_sdav_flat(files, network, key_points_fn)
    if pool is None:
        return desc
    p = (network.input_shape[0] if network is not None else 30)
    return pool.transform_tensor(desc.view(len(files) * p, -1), patches=p)


def describe_sdav_compact(files, network=None, key_points_fn=None, pool=None, pca=None):
    """describe_sdav, then the rows projected by a fitted pca.Pca of their width (75 000 for the concatenation, K * 2500
    behind a pool) to [frames, M]: the compact descriptor KeyframeDatabase stores.  pca None: describe_sdav's rows."""
    desc = describe_sdav(files, network, key_points_fn, pool)
    return desc if pca is None else pca.transform_tensor(desc)


def _describe_sdav_flat(files, network=None, key_points_fn=None, return_key_points=False):
    """return_key_points: (the rows, the int32 [frames, P, 2] device tensor of the points the patches were cut at) -- frames
    of one size only."""
    from . import pipeline
    from .input import read_ppm
    from .sdav import SDAV
    network = network or SDAV()
    p = network.input_shape[0]
    frames = [read_ppm(f) for f in files]
    if any(fr.shape != frames[0].shape for fr in frames):
        if return_key_points:
            raise ValueError("key-points are returned for frames of one size only")
        # a chunk of frames of several sizes (the reference parses them one by one, CvInputParser.py:30-33): each frame's
        # patches are gathered on the device on its own, as drivers.create_similarity_matrix does
        from .input import CvInputParser
        parser = CvInputParser(p, int(round(np.sqrt(network.input_shape[1]))))
        x = torch.stack([parser.parse_tensor(fr, key_points_fn(fr.shape[:2]) if key_points_fn else None) for fr in frames])
        return network.transform_tensor(x).view(len(files), -1)
    kp = None
    if key_points_fn:
        kp = pipeline.key_point_array([key_points_fn(fr.shape[:2]) for fr in frames], p, network.engine)
    if return_key_points:
        desc, pts = pipeline.sdav_descriptors_from_frames(np.stack(frames), network, key_points=kp, return_key_points=True)
        return desc.view(len(files), -1), pts
    desc = pipeline.sdav_descriptors_from_frames(np.stack(frames), network, key_points=kp)
    return desc.view(len(files), -1)


def describe_cnn_vtl(files, network=None, as_int8=False):
    """Frames -> CnnVtl int8 descriptors [B, D'] as float32 for the cosine engine (as_int8: as they are, for the distance
    search), a DEVICE tensor (pipeline.py)."""
    from . import pipeline
    from .cnn_vtl import CnnVtl
    from .input import read_ppm
    frames = np.stack([read_ppm(f)[..., ::-1] for f in files])           # BGR, as create_distance_matrix.py:23
    network = network or CnnVtl(input_shape=[len(files)] + list(frames.shape[1:]))
    desc = pipeline.cnn_vtl_descriptors_from_frames(frames, network)
    return desc if as_int8 else desc.to(torch.float32)


def chain_line(pairs):
    """The CLI's line under a candidate: `chain`, then the L frame:key-frame pairs, oldest frame first, tab-separated."""
    return "chain\t" + "\t".join("%d:%d" % p for p in pairs)


def _model_widths(ap, args, option):
    """--codebook, --pca or --hash (`option`, given): (the width its .npz was fitted to, the width of what reaches it in
    the stream) -- a patch descriptor in front of --codebook; the frame descriptor in front of --pca, the concatenation
    or behind --pool vlad the codebook's K words; in front of --hash that, or --pca's M.  A file that cannot be read so is
    the parser's error `--option: ...`."""
    def read(name, key, axis=None):
        with np.load(getattr(args, name), allow_pickle=False) as z:
            return int(z[key] if axis is None else z[key].shape[axis])
    try:
        if option == "codebook":
            return read("codebook", "centroids", 1), SDAV_CLI_WIDTH
        frame = (read("codebook", "centroids", 0) if args.pool == "vlad" else SDAV_CLI_PATCHES) * SDAV_CLI_WIDTH
        if option == "pca":
            return read("pca", "basis", 0), frame
        return read("hash", "width"), frame if args.pca is None else read("pca", "basis", 1)
    except (OSError, ValueError, KeyError, IndexError) as err:
        ap.error("--%s: %s" % (option, err))


def main(argv=None):
    ap = argparse.ArgumentParser(description="stream the frames of a dataset through the loop-closure detector")
    ap.add_argument("dataset_path")
    ap.add_argument("--pattern", default="*.ppm")
    ap.add_argument("--network", choices=["sdav", "cnn_vtl", "seqslam", "ldb"], default="cnn_vtl",
                    help="the descriptor: SDAV, CnnVtl, SeqSLAM's patch-normalised grey thumbnail (needs no weights; "
                         "goes with --metric sad) or the binary LDB code of a grey thumbnail (needs no weights; goes with "
                         "--metric hamming)")
    ap.add_argument("--weights", help=".npz written by SDAV.save_weights (sdav) / AlexNet .npy blob (cnn_vtl)")
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--threshold", type=float, default=None,
                    help="report candidates at or above this score (default: 0.9 for cosine, all k for similarity)")
    ap.add_argument("--metric", choices=["cosine", "distance", "similarity", "sad", "hamming"], default="cosine",
                    help="cosine of the descriptors, the reference's cnn_vtl distance (needs --network cnn_vtl), the "
                         "reference's SDAV similarity (needs --network sdav; the distinctive score comes from the first batch) "
                         "SeqSLAM's sum of absolute differences (needs --network seqslam) or the Hamming distance of binary "
                         "codes (needs --network ldb)")
    ap.add_argument("--sequence", type=int, default=None, metavar="L",
                    help="--metric similarity, sad or hamming: rank by the sum of the scores along a line of L frames (sequence search)")
    ap.add_argument("--contrast", type=int, default=None, metavar="R",
                    help="with --sequence: normalise every score against the R key-frames on either side of it first "
                         "(SeqSLAM's local contrast normalisation), R in 1..32")
    ap.add_argument("--suppress", type=int, default=None, metavar="W",
                    help="with --sequence: report distinct places -- every candidate more than W frames from the better "
                         "ones of its frame (the windowed peak selection)")
    ap.add_argument("--steps", default=None, metavar="DMIN:DMAX",
                    help="with --sequence: the elastic search -- from frame to frame the matched key-frame steps back "
                         "DMIN..DMAX key-frames (0 <= DMIN <= DMAX <= 8) instead of following a straight line")
    ap.add_argument("--track", default=None, metavar="JUMP:GATE:NULL",
                    help="with --sequence: a place tracker over the same score rows (a Viterbi filter with a no-loop state): "
                         "JUMP the cost of changing place, GATE of entering or leaving `no loop`, NULL the score of a frame "
                         "that closes no loop; after the stream one line `track FRAME KEYFRAME` for every frame the "
                         "smoothed path places")
    ap.add_argument("--track-steps", default=None, metavar="DMIN:DMAX",
                    help="with --track: the key-frames a place advances per frame at no cost (default 0:2)")
    ap.add_argument("--chains", action="store_true",
                    help="with --sequence: under every candidate a line `chain` with the L frame:key-frame pairs it was "
                         "matched along, oldest frame first")
    ap.add_argument("--max-distance", type=float, default=None,
                    help="--metric distance or hamming: report candidates at or below this distance, an integer (hamming "
                         "with --sequence: the sum along the line, and any number with --contrast; default: all k)")
    ap.add_argument("--max-difference", type=float, default=None,
                    help="--metric sad: report candidates at or below this difference (with --sequence: the sum along the "
                         "line; default: all k)")
    ap.add_argument("--size", default=None, metavar="HxW",
                    help="--network seqslam or ldb: the thumbnail's rows x columns (default: 32x64 for seqslam, 48x48 for ldb)")
    ap.add_argument("--levels", default=None, metavar="G,G[,...]",
                    help="--network ldb: 1 to 4 grid sizes, strictly ascending, each 2..8; twice each must divide both sides "
                         "of --size (default: 2,3,4)")
    ap.add_argument("--patch", type=int, default=8, help="--network seqslam: side of the normalisation tiles, 1..64")
    ap.add_argument("--strength", type=int, default=32,
                    help="--network seqslam: descriptor byte = 128 + strength * z-score, 1..127")
    ap.add_argument("--shift", type=int, default=None, metavar="S",
                    help="--network seqslam: compare over the lateral shifts -S .. S of the thumbnail's columns and keep the "
                         "best (a place revisited a little to the side), 0 <= S <= %d and S < W of --size" % L.DLC_MAX_SHIFT)
    ap.add_argument("--fuse", default=None, metavar="MEMBER,MEMBER[,...]",
                    help="multi-descriptor fusion: two or three of sad (SeqSLAM's thumbnails: --size, --patch, --strength, "
                         "--shift), distance and cosine (both from one CnnVtl forward per batch), each member's rows "
                         "normalised, weighted and summed into one score, higher is better (FusedLoopClosureDetector); "
                         "goes with --sequence, --contrast, --suppress, --steps, --chains and --positions, not with "
                         "--network / --metric")
    ap.add_argument("--fuse-weights", default=None, metavar="W,W[,...]",
                    help="with --fuse: one finite weight per member (default: all 1)")
    ap.add_argument("--fuse-norm", choices=list(FUSE_NORMS), default=None,
                    help="with --fuse: how each member's row is normalised before the sum (default: zscore)")
    ap.add_argument("--pool", choices=["flatten", "vlad"], default=None,
                    help="--network sdav --metric cosine: the frame descriptor -- flatten, the concatenation of the patch "
                         "descriptors (the default), or vlad, their orderless VLAD pooling over the codebook of --codebook")
    ap.add_argument("--codebook", default=None, metavar="FILE",
                    help="with --pool vlad: the .npz written by python -m deeploopcloser_amd.train_vlad")
    ap.add_argument("--pca", default=None, metavar="FILE",
                    help="--network sdav --metric cosine: project the frame descriptor (of either --pool) with the .npz "
                         "written by python -m deeploopcloser_amd.train_pca before it is stored and matched")
    ap.add_argument("--hash", default=None, metavar="FILE",
                    help="--network sdav --metric cosine: hash the frame descriptor (of either --pool, behind --pca if "
                         "given) with the .npz written by python -m deeploopcloser_amd.train_lsh and search the codes by "
                         "Hamming distance: everything --metric hamming takes behind its rows goes with it (--max-distance, "
                         "--sequence, --contrast, --suppress, --steps, --chains, --track)")
    ap.add_argument("--exclusion", type=int, default=30)
    ap.add_argument("--batch", type=int, default=16, help="frames encoded and matched per step")
    ap.add_argument("--dtype", choices=["bf16", "f16"], default="bf16")
    ap.add_argument("--encoder-dtype", choices=["float64", "f16x2"], default="float64",
                    help="the encoder's arithmetic: float64 (parity with the reference) or f16x2, the tolerance mode of "
                         "SDAV / CnnVtl on the fp16 matrix cores (--dtype is the cosine database's storage type)")
    ap.add_argument("--no-latency-mode", action="store_true",
                    help="keep the one-pass GEMMs (bit-identical to a large-batch encode) for small batches too")
    ap.add_argument("--positions", default=None, metavar="FILE",
                    help="ground truth: a text file with one line per frame, in the order of the sorted files, of one or two "
                         "integers (a distance along the route or a frame index, or x and y); after the stream one line "
                         "`pr` on stderr: average precision, recall at 100 %% precision and the best F1 of the best "
                         "candidate per frame over every threshold (needs --radius)")
    ap.add_argument("--radius", type=int, default=None, metavar="R",
                    help="with --positions: a key-frame within R of a frame's position is the same place")
    ap.add_argument("--pr-curve", default=None, metavar="OUT.tsv",
                    help="with --positions: write the curve there -- threshold, tp, fp, precision, recall; strictest first")
    ap.add_argument("--verify", type=int, default=None, metavar="MIN_INLIERS",
                    help="--network sdav: geometric verification of every candidate (verification.GeometricVerifier) -- the "
                         "frames' patches are matched, a 2-D transform is fitted to the matched key-points and a candidate "
                         "with fewer than MIN_INLIERS agreeing matches is not reported; every `loop` line is followed by "
                         "one line `verify<TAB>inliers<TAB>matches`")
    ap.add_argument("--verify-tol", type=int, default=None, metavar="T", help="with --verify: the inlier tolerance in pixels, 0..255 (3)")
    ap.add_argument("--verify-model", choices=["similarity", "translation"], default=None,
                    help="with --verify: rotation + scale + translation from two matches (default), or translation from one")
    ap.add_argument("--verify-max-scale", type=float, default=None, metavar="S",
                    help="with --verify: the similarity's scale stays within [1 / S, S], 1..16 (2)")
    args = ap.parse_args(argv)
    if args.verify is None and (args.verify_tol is not None or args.verify_model is not None or args.verify_max_scale is not None):
        ap.error("--verify-tol, --verify-model and --verify-max-scale need --verify")
    if args.verify is not None:
        if args.fuse is not None or args.network != "sdav":
            ap.error("--verify needs --network sdav (the patch descriptors and key-points are the SDAV front-end's)")
        if args.verify < 0:
            ap.error("--verify must be >= 0")
        if args.chains:
            ap.error("--verify excludes --chains")
        args.verify_tol = 3 if args.verify_tol is None else args.verify_tol
        if not 0 <= args.verify_tol <= 255:
            ap.error("--verify-tol must be 0..255")
        args.verify_model = args.verify_model or "similarity"
        args.verify_max_scale = 2.0 if args.verify_max_scale is None else args.verify_max_scale
        if not 1.0 <= args.verify_max_scale <= 16.0:
            ap.error("--verify-max-scale must be 1..16")
    if args.fuse is None and (args.fuse_weights is not None or args.fuse_norm is not None):
        ap.error("--fuse-weights and --fuse-norm need --fuse")
    if args.fuse is not None:
        args.fuse = [v.strip() for v in args.fuse.split(",")]
        if not 2 <= len(args.fuse) <= len(FUSE_MEMBERS) or any(v not in FUSE_MEMBERS for v in args.fuse) or \
                len(set(args.fuse)) != len(args.fuse):
            ap.error("--fuse takes two or three different members of %s, comma-separated" % ", ".join(FUSE_MEMBERS))
        if args.network != "cnn_vtl" or args.metric != "cosine":
            ap.error("--fuse chooses the descriptors and the measures itself: it excludes --network and --metric")
        if args.fuse_weights is None:
            args.fuse_weights = [1.0] * len(args.fuse)
        else:
            try:
                args.fuse_weights = [float(v) for v in args.fuse_weights.split(",")]
            except ValueError:
                ap.error("--fuse-weights must be numbers, comma-separated")
            if len(args.fuse_weights) != len(args.fuse):
                ap.error("--fuse-weights: %d weights for %d members" % (len(args.fuse_weights), len(args.fuse)))
            if not all(np.isfinite(v) for v in args.fuse_weights):
                ap.error("--fuse-weights must be finite")
        args.fuse_norm = args.fuse_norm or "zscore"
    if args.pool == "vlad":
        if args.fuse is not None or args.network != "sdav" or args.metric != "cosine":
            ap.error("--pool vlad needs --network sdav --metric cosine")
        if args.codebook is None:
            ap.error("--pool vlad needs --codebook")
    elif args.codebook is not None:
        ap.error("--codebook needs --pool vlad")
    if args.codebook is not None:
        have, want = _model_widths(ap, args, "codebook")
        if have != want:
            ap.error("--codebook: its words are %d wide, the encoder's descriptors %d" % (have, want))
    if args.pca is not None:
        if args.fuse is not None or args.network != "sdav" or args.metric != "cosine":
            ap.error("--pca needs --network sdav --metric cosine")
        have, want = _model_widths(ap, args, "pca")
        if have != want:
            ap.error("--pca: its rows are %d wide, the frame descriptor %d" % (have, want))
    if args.hash is not None:
        if args.fuse is not None or args.network != "sdav" or args.metric != "cosine":
            ap.error("--hash needs --network sdav --metric cosine")
        if args.verify is not None:
            ap.error("--hash excludes --verify")
        have, want = _model_widths(ap, args, "hash")
        if have != want:
            ap.error("--hash: its rows are %d wide, the frame descriptor %d" % (have, want))
    hamming = args.metric == "hamming" or args.hash is not None      # the rows behind the descriptor are Hamming rows
    thumbnails = args.network == "seqslam" or (args.fuse is not None and "sad" in args.fuse)
    if args.metric == "distance" and args.network != "cnn_vtl":
        ap.error("--metric distance needs --network cnn_vtl")
    if args.metric == "similarity" and args.network != "sdav":
        ap.error("--metric similarity needs --network sdav")
    if (args.network == "seqslam") != (args.metric == "sad"):
        ap.error("--network seqslam and --metric sad need each other")
    if (args.network == "ldb") != (args.metric == "hamming"):
        ap.error("--network ldb and --metric hamming need each other")
    if args.levels is not None and args.network != "ldb":
        ap.error("--levels needs --network ldb")
    if args.size is None:
        args.size = "48x48" if args.network == "ldb" else "32x64"
    if args.max_distance is not None and not (hamming and args.contrast is not None):
        if args.max_distance < 0 or args.max_distance != int(args.max_distance):
            ap.error("--max-distance must be a non-negative integer (any number with --metric hamming --contrast)")
        args.max_distance = int(args.max_distance)
    if args.shift is not None and not thumbnails:
        ap.error("--shift needs --network seqslam (or --fuse with sad)")
    if thumbnails or args.network == "ldb":
        try:
            args.size = tuple(int(v) for v in args.size.lower().split("x"))
        except ValueError:
            args.size = ()
        if len(args.size) != 2 or min(args.size) < 1 or args.size[0] * args.size[1] > 65536:
            ap.error("--size must be HxW, two positive integers with H * W <= 65536")
    if args.network == "ldb":
        from .ldb import ldb_bits
        try:
            args.levels = (2, 3, 4) if args.levels is None else tuple(int(v) for v in args.levels.split(","))
            ldb_bits(args.levels)
        except ValueError:
            ap.error("--levels must be 1 to 4 integers, strictly ascending, each 2..8")
        if any(v % (2 * g) for g in args.levels for v in args.size):
            ap.error("--levels: twice every grid size must divide both sides of --size")
    if thumbnails:
        if not 1 <= args.patch <= 64:
            ap.error("--patch must be 1..64")
        if not 1 <= args.strength <= 127:
            ap.error("--strength must be 1..127")
        if args.shift is not None and not 0 <= args.shift <= min(L.DLC_MAX_SHIFT, args.size[1] - 1):
            ap.error("--shift must be 0..%d and below the W of --size" % L.DLC_MAX_SHIFT)
        if args.max_difference is not None and args.contrast is None:
            if args.max_difference < 0 or args.max_difference != int(args.max_difference):
                ap.error("--max-difference must be a non-negative integer (any number with --contrast)")
            args.max_difference = int(args.max_difference)
    if args.sequence is not None and args.metric not in ("similarity", "sad", "hamming") and args.fuse is None and not hamming:
        ap.error("--sequence needs --metric similarity, sad or hamming (or --fuse)")
    if args.sequence is not None and not 1 <= args.sequence <= 64:
        ap.error("--sequence must be 1..64")
    if args.contrast is not None and args.sequence is None:
        ap.error("--contrast needs --sequence")
    if args.contrast is not None and not 1 <= args.contrast <= 32:
        ap.error("--contrast must be 1..32")
    if args.suppress is not None and args.sequence is None and args.fuse is None:
        ap.error("--suppress needs --sequence (or --fuse)")
    if args.suppress is not None and args.suppress < 0:
        ap.error("--suppress must be >= 0")
    if args.steps is not None:
        if args.sequence is None:
            ap.error("--steps needs --sequence")
        try:
            d_min, d_max = (int(x) for x in args.steps.split(":"))
        except ValueError:
            ap.error("--steps must be DMIN:DMAX")
        if not 0 <= d_min <= d_max <= L.DLC_MAX_STEP:
            ap.error("--steps must be DMIN:DMAX with 0 <= DMIN <= DMAX <= %d" % L.DLC_MAX_STEP)
        args.steps = (d_min, d_max)
    if args.chains and args.sequence is None:
        ap.error("--chains needs --sequence")
    if args.track_steps is not None and args.track is None:
        ap.error("--track-steps needs --track")
    if args.track is not None:
        if args.sequence is None:
            ap.error("--track needs --sequence")
        try:
            jump, gate, null = (float(x) for x in args.track.split(":"))
            d_min, d_max = (0, 2) if args.track_steps is None else (int(x) for x in args.track_steps.split(":"))
        except ValueError:
            ap.error("--track must be JUMP:GATE:NULL (numbers) and --track-steps DMIN:DMAX")
        if not (np.isfinite(jump) and np.isfinite(gate) and jump >= 0 and gate >= 0) or np.isnan(null):
            ap.error("--track: JUMP and GATE must be finite and not negative, NULL a number")
        if not 0 <= d_min <= d_max <= L.DLC_MAX_STEP:
            ap.error("--track-steps must be DMIN:DMAX with 0 <= DMIN <= DMAX <= %d" % L.DLC_MAX_STEP)
        args.track = dict(steps=(d_min, d_max), jump=jump, gate=gate, null_score=null)
    if args.threshold is None and args.fuse is None:             # (--fuse: every candidate, as the fused scale is the norm's)
        args.threshold = float("-inf") if args.metric == "similarity" else 0.9

    if args.positions is None and (args.radius is not None or args.pr_curve is not None):
        ap.error("--radius and --pr-curve need --positions")
    if args.positions is not None and args.radius is None:
        ap.error("--positions needs --radius")
    if args.radius is not None and args.radius < 0:
        ap.error("--radius must be >= 0")

    files = _frame_files(args.dataset_path, args.pattern)
    if args.positions is not None:
        from .evaluate import read_positions
        try:
            args.positions = read_positions(args.positions)
        except (OSError, ValueError) as err:
            ap.error("--positions: %s" % err)
        if len(args.positions) != len(files):
            ap.error("--positions: %d lines for %d frames" % (len(args.positions), len(files)))
    from .engine import default_engine
    eng = default_engine()
    latency = args.batch <= 16 and not args.no_latency_mode      # split-K encode GEMMs: ~8x lower latency per frame
    with (eng.latency_mode() if latency else contextlib.nullcontext()):
        return _stream(args, files)


def _fused_describe(args, files):
    """--fuse: one descriptor tensor per member and batch -- the thumbnails for sad, ONE CnnVtl forward for distance and
    cosine."""
    from .input import read_ppm
    thumbs = cnn = None
    if "sad" in args.fuse:
        from . import pipeline
        from .seqslam import SeqSlam
        thumbs = SeqSlam(size=args.size, patch=args.patch, strength=args.strength)
    if "distance" in args.fuse or "cosine" in args.fuse:
        from .cnn_vtl import CnnVtl
        cnn = CnnVtl(input_shape=[args.batch] + list(read_ppm(files[0]).shape), dtype=args.encoder_dtype)
        if args.weights:
            cnn.load_alexnet_npy(args.weights)

    def describe(fs):
        deep = describe_cnn_vtl(fs, cnn, as_int8=True) if cnn is not None else None
        sad = pipeline.seqslam_descriptors_from_frames(np.stack([read_ppm(f) for f in fs]), thumbs) if thumbs is not None else None
        return [sad if m == "sad" else (deep if m == "distance" else deep.to(torch.float32)) for m in args.fuse]
    return describe


def _detector(args, desc, n_files):
    """The stream's detector, made when the first batch's descriptors `desc` are there: their widths are the store's."""
    shared = dict(k=args.k, exclusion=args.exclusion, capacity=max(4096, n_files))
    search = dict(sequence=args.sequence, contrast=args.contrast, suppress=args.suppress, steps=args.steps, chains=args.chains,
                  track=args.track)
    if args.fuse is not None:
        options = {"sad": {} if args.shift is None else {"shift": args.shift, "width": args.size[1]},
                   "cosine": {"dtype": args.dtype, "center": True}, "distance": {}}
        track = search.pop("track")                              # (asked for before the first frame, not at construction)
        det = FusedLoopClosureDetector([(m, d.shape[1], options[m]) for m, d in zip(args.fuse, desc)], weights=args.fuse_weights,
                                       norm=args.fuse_norm, threshold=args.threshold, **shared, **search)
        if track is not None:
            det.start_tracking(track)
        return det
    if args.metric == "similarity":
        # the reference takes the distinctive score from the whole dataset (SimilarityCalculator.py:20-27); a stream
        # has only seen its first batch when it must fix it
        shared["capacity"] = max(1024, n_files)
        return SdavLoopClosureDetector(desc, patches=desc.shape[1], width=desc.shape[2], threshold=args.threshold, **shared,
                                       **search)
    if args.metric == "distance":
        return CnnVtlLoopClosureDetector(desc.shape[1], max_distance=args.max_distance, **shared)
    if args.metric == "sad":
        return SeqSlamLoopClosureDetector(desc.shape[1], max_difference=args.max_difference, shift=args.shift,
                                          width=None if args.shift is None else args.size[1], **shared, **search)
    if getattr(args, "hash", None) is not None:              # (callers that build the namespace themselves may not know --hash)
        from .lsh import Lsh
        return HashedLoopClosureDetector(Lsh.load(args.hash), max_distance=args.max_distance, **shared, **search)
    if args.metric == "hamming":
        return LdbLoopClosureDetector(desc.shape[1], max_distance=args.max_distance, **shared, **search)
    return LoopClosureDetector(desc.shape[1], threshold=args.threshold, dtype=args.dtype, center=True, **shared)


def _stream(args, files):
    fused = args.fuse is not None
    verifier = None
    local = []                                                   # --verify: the batch's (patch descriptors, key-points)
    if fused:
        describe = _fused_describe(args, files)
    elif args.network == "sdav":
        from .sdav import SDAV
        net = SDAV(dtype=args.encoder_dtype)
        if args.weights:
            net.load_weights(args.weights)
        pool = compact = None
        if args.pool == "vlad":
            from .vlad import Vlad
            pool = Vlad.load(args.codebook)
        describe = (lambda fs: describe_sdav(fs, net)) if pool is None else (lambda fs: describe_sdav(fs, net, pool=pool))
        if getattr(args, "pca", None) is not None:         # (callers that build the namespace themselves may not know --pca)
            from .pca import Pca
            compact = Pca.load(args.pca)
            describe = lambda fs: describe_sdav_compact(fs, net, pool=pool, pca=compact)
        if getattr(args, "verify", None) is not None:
            from .verification import GeometricVerifier, keep_accepted
            patches = net.input_shape[0]
            verifier = GeometricVerifier(patches=patches, width=net.hidden_units[-1], capacity=max(1024, len(files)),
                                         min_inliers=args.verify, model=args.verify_model, tol=args.verify_tol,
                                         max_scale=args.verify_max_scale)

            def describe(fs):
                # the frames' patch descriptors and key-points stay behind for the verifier; the place rows are formed
                # from the same descriptors as without --verify
                flat, pts = _describe_sdav_flat(fs, net, return_key_points=True)
                local[:] = [flat.view(len(fs), patches, -1), pts]
                rows = flat if pool is None else pool.transform_tensor(flat.view(len(fs) * patches, -1), patches=patches)
                return rows if compact is None else compact.transform_tensor(rows)
    elif args.network == "seqslam":
        from . import pipeline
        from .input import read_ppm
        from .seqslam import SeqSlam
        net = SeqSlam(size=args.size, patch=args.patch, strength=args.strength)
        describe = lambda fs: pipeline.seqslam_descriptors_from_frames(np.stack([read_ppm(f) for f in fs]), net)
    elif args.network == "ldb":
        from . import pipeline
        from .input import read_ppm
        from .ldb import Ldb
        net = Ldb(size=args.size, levels=args.levels)
        describe = lambda fs: pipeline.ldb_descriptors_from_frames(np.stack([read_ppm(f) for f in fs]), net)
    else:
        from .cnn_vtl import CnnVtl
        from .input import read_ppm
        shape = read_ppm(files[0]).shape
        net = CnnVtl(input_shape=[args.batch] + list(shape), dtype=args.encoder_dtype)
        if args.weights:
            net.load_alexnet_npy(args.weights)
        describe = lambda fs: describe_cnn_vtl(fs, net, as_int8=args.metric == "distance")
    judge = None
    if args.positions is not None:
        from .evaluate import LoopClosureEvaluator, pr_line
        judge = LoopClosureEvaluator(args.positions, args.radius, args.exclusion,
                                     lower_is_better=not fused and (args.metric in ("distance", "sad", "hamming") or
                                                                    getattr(args, "hash", None) is not None))
    det = None
    lat = []                                                     # wall-clock per step: file read -> descriptors -> match -> candidates on the host
    for lo in range(0, len(files), args.batch):
        chunk = files[lo:lo + args.batch]
        t0 = time.perf_counter()
        desc = describe(chunk)
        if not fused and args.metric == "similarity":
            desc = desc.view(len(chunk), net.input_shape[0], -1)         # [B, P, H]: the frames' patch descriptors
        if det is None:
            det = _detector(args, desc, len(files))
        s, i, *chain = det.query_and_insert(desc)
        verdict = None
        if verifier is not None:
            # the batch's frames become resident, then every candidate is verified: rejected slots leave the lists
            verifier.append(*local)
            inl, nm = verifier.verify(lo, i)
            s, i, inl, nm = keep_accepted(inl >= verifier.min_inliers, s, i, float("-inf"), inl, nm)
            ids, inl, nm = i.cpu().numpy(), inl.cpu().numpy(), nm.cpu().numpy()
            verdict = {(lo + r, int(ids[r, c])): (int(inl[r, c]), int(nm[r, c])) for r, c in zip(*np.nonzero(ids >= 0))}
        found = det.loops(s, i, lo, *chain)                      # (the one host read of the step)
        lat.append(((time.perf_counter() - t0) * 1e3, len(chunk)))
        if judge is not None:
            judge.add(s, i, lo)                                  # (every candidate, whatever the reporting threshold)
        for frame, match, score, *pairs in found:
            print(("loop\t%d\t%s\t%d\t%s\t" + ("%d" if isinstance(score, int) else "%.4f"))
                  % (frame, os.path.basename(files[frame]), match, os.path.basename(files[match]), score))
            if pairs:
                print(chain_line(pairs[0]))
            if verdict is not None:
                print("verify\t%d\t%d" % verdict[(frame, match)])
    if args.track is not None:                                   # the smoothed labelling of the whole stream
        for frame, place in enumerate(det.tracker.path().cpu().tolist()):
            if place >= 0:
                print("track\t%d\t%d" % (frame, place))
    print("frames\t%d\tkey-frames\t%d" % (len(files), len(det)), file=sys.stderr)
    # the first step pays one-time costs (the library's first launches, workspaces, the database's reservation): reported apart
    steady = lat[1:] if len(lat) > 1 else lat
    ms = np.array([m for m, _ in steady])
    per_frame = float(ms.sum() / max(1, sum(c for _, c in steady)))
    print("latency\tbatch\t%d\tsteps\t%d\tfirst_step_ms\t%.2f\tms_per_step_median\t%.3f\tms_per_step_max\t%.3f\tms_per_frame\t%.3f"
          % (args.batch, len(lat), lat[0][0], float(np.median(ms)), float(ms.max()), per_frame), file=sys.stderr)
    if judge is not None:
        curve, _ = judge.result()
        print(pr_line(judge.queries, curve), file=sys.stderr)
        if args.pr_curve is not None:
            with open(args.pr_curve, "w") as f:
                f.write("threshold\ttp\tfp\tprecision\trecall\n")
                for t, tp, fp, p, r in curve.rows():
                    f.write(("%d" if isinstance(t, int) else "%.17g") % t + "\t%d\t%d\t%.6f\t%.6f\n" % (tp, fp, p, r))
    return 0


if __name__ == "__main__":
    sys.exit(main())
