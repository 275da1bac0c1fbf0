"""Place tracking over score rows: a belief carried from frame to frame, with a state for "this frame closes no loop".

The sequence searches ask whether a match holds over the last L frames; PlaceTracker runs the max-plus (Viterbi)
recursion of dlc_track_rows (include/dlc.h) over the whole traversal.  Per frame it keeps, for every key-frame, the best
score of any labelling of the frames so far that ends there -- a place advances steps = (d_min, d_max) key-frames per
frame at no cost, moves anywhere else for `jump`, and enters or leaves "no loop" for `gate` -- and the same for "no loop",
which scores `null_score` per frame.  update() answers the filtered place of each new frame; path() walks the kept
back-pointers and answers the best labelling of every frame so far, a key-frame or -1.  Every value is one maximum over
exact values and one addition, so the result is exact on integer rows and does not depend on the batching."""
import numpy as np
import torch

from . import _lib as L
from .engine import check_steps, default_engine
from .sequence import _on_device


class PlaceTracker:
    """steps, jump, gate, null_score, lower_is_better: as Engine.track_rows takes them (null_score NaN or None: no
    no-loop state).  history=True keeps the int8 back-pointers of every frame (one byte per frame and key-frame) for
    path(); without it only update() is available."""

    def __init__(self, steps=(0, 2), jump=0.0, gate=0.0, null_score=None, lower_is_better=False, history=True, device=None):
        self.steps = check_steps(steps)
        self.jump, self.gate = float(jump), float(gate)
        self.null_score = float("nan") if null_score is None else float(null_score)
        if not (np.isfinite(self.jump) and np.isfinite(self.gate) and self.jump >= 0 and self.gate >= 0):
            raise ValueError("PlaceTracker: jump and gate must be finite and not negative")
        self.lower_is_better, self.history = bool(lower_is_better), bool(history)
        self.engine = default_engine(device)
        self.reset()

    def reset(self):
        """Forget the traversal: the next row is a first row again."""
        self.frames, self.n, self.dtype = 0, 0, None
        self._V = self._head = self._back = self._backU = self._g = self._place_last = None
        self._numpy = False

    def _grow(self, b, n, dtype):
        e = self.engine
        if self.dtype is None:
            self.dtype = e._OUT_DTYPES[dtype]
            self._V, self._head = e.track_state(n, dtype)
        elif e._OUT_DTYPES[dtype] != self.dtype:
            raise ValueError("PlaceTracker: the rows were %s before" % ("int64" if self.dtype == torch.int64 else "float"))
        if n < self.n:
            raise ValueError("PlaceTracker: n=%d is below the %d columns of the rows before" % (n, self.n))
        if n > self._V.shape[0]:                                    # the new entries hold the absent mark
            new, _ = e.track_state(max(n, 2 * self._V.shape[0]), dtype)
            new[:self._V.shape[0]] = self._V
            self._V = new
        self.n = n
        if not self.history:
            return
        rows = self.frames + b
        if self._back is None or rows > self._back.shape[0] or n > self._back.shape[1]:
            old = self._back
            have = (0, 0) if old is None else tuple(old.shape)    # a side that grows at least doubles
            shape = tuple(h if w <= h else max(w, 2 * h) for w, h in zip((rows, n), have))
            self._back = torch.full(shape, L.DLC_TRACK_ABSENT, dtype=torch.int8, device=e.device)
            backU = torch.full((shape[0],), L.DLC_TRACK_ABSENT, dtype=torch.int8, device=e.device)
            g = torch.full((shape[0],), -1, dtype=torch.int64, device=e.device)
            if old is not None:
                self._back[:self.frames, :old.shape[1]] = old[:self.frames]
                backU[:self.frames], g[:self.frames] = self._backU[:self.frames], self._g[:self.frames]
            self._backU, self._g = backU, g

    def update(self, rows, n=None, limit0=None, limit_step=0, plan=None):
        """The next frames' score rows [B, >= n] (NumPy or a device tensor; fp64, fp32 or int64; n None: every column;
        n may grow from call to call), row r offering its first clamp(limit0 + r * limit_step, 0, n) cells (limit0
        None = n).  Returns (place [B] int64, G [B], U [B]): the filtered place of each frame (-1 = no loop), the best
        place's value and the no-loop state's (fp64, int64 for int64 rows; absent = NaN / INT64_MIN)."""
        e = self.engine
        rows, self._numpy = _on_device(e, rows)
        b = rows.shape[0]
        n = rows.shape[1] if n is None else int(n)
        if b == 0:
            out = (torch.empty(0, dtype=torch.int64, device=e.device),) + tuple(
                torch.empty(0, dtype=e._OUT_DTYPES.get(rows.dtype, torch.float64), device=e.device) for _ in range(2))
        else:
            if rows.dtype not in e._OUT_DTYPES or not 1 <= n <= rows.shape[1]:
                raise ValueError("PlaceTracker: rows must be [B, >= n] float64, float32 or int64, n >= 1")
            self._grow(b, n, rows.dtype)
            back = self._back[self.frames:self.frames + b] if self.history else False
            place, g, G, U, backU, _, _ = e.track_rows(rows, self._V, self._head, self.steps, self.jump, self.gate, self.null_score,
                                                      n=n, limit0=limit0, limit_step=limit_step,
                                                      lower_is_better=self.lower_is_better, plan=plan, back=back)
            if self.history:
                self._backU[self.frames:self.frames + b] = backU
                self._g[self.frames:self.frames + b] = g
                self._place_last = place[-1:].clone()
            self.frames += b
            out = (place, G, U)
        return tuple(t.cpu().numpy() for t in out) if self._numpy else out

    def path(self, end=None):
        """int64 [frames]: the best labelling of every frame so far that ends in the last frame's filtered place (end: a
        key-frame or -1 instead) -- a key-frame, or -1 for no loop (NumPy if the last update took NumPy)."""
        if not self.history:
            raise ValueError("PlaceTracker: path() needs history=True")
        e = self.engine
        if self.frames == 0:
            path = torch.empty(0, dtype=torch.int64, device=e.device)
        else:
            path = e.track_backtrace(self._back[:self.frames], self._backU[:self.frames], self._g[:self.frames],
                                     L.DLC_TRACK_END_FILTERED if end is None else int(end), self._place_last, n=self.n)
        return path.cpu().numpy() if self._numpy else path


def track_places(matrix, steps=(0, 2), jump=0.0, gate=0.0, null_score=None, lower_is_better=False, n=None, limit0=None,
                 limit_step=0, plan=None):
    """(place, path, G, U) of a whole score matrix [frames, n] (NumPy in -> NumPy out, a device tensor in -> tensors
    out): PlaceTracker.update over all rows at once and PlaceTracker.path."""
    t = PlaceTracker(steps, jump, gate, null_score, lower_is_better)
    place, G, U = t.update(matrix, n=n, limit0=limit0, limit_step=limit_step, plan=plan)
    return place, t.path(), G, U
