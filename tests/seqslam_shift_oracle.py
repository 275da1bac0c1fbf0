"""NumPy restatement of dlc_sad_u8_shift_rows (include/dlc.h), written from the header's text: for every pair a loop over
the shifts in the stated order 0, -1, +1, ..., -S, +S, the overlap's sum of absolute differences, the rescaling
floor(sad * w / (w - |s|)) and a strict `<` to replace -- int64 throughout.  No tiling, no masks, no shortcuts.

shift_rows_composed is a second, independent form built only from the plain sad_rows oracle: cropped copies of both
operands for each shift, then the rescaling and a running minimum."""
import numpy as np

import seqslam_oracle as sq


def shift_order(S):
    """0, -1, +1, -2, +2, ..., -S, +S."""
    order = [0]
    for k in range(1, S + 1):
        order += [-k, k]
    return order


def shift_rows(q, db, h, w, S):
    """(int64 [Q, N] values, int8 [Q, N] shifts) by the definition."""
    q, db = np.asarray(q), np.asarray(db)
    assert q.dtype == np.uint8 and db.dtype == np.uint8 and q.shape[1] == h * w and db.shape[1] == h * w and 0 <= S < w
    qi = q.reshape(-1, h, w).astype(np.int64)
    di = db.reshape(-1, h, w).astype(np.int64)
    out = np.empty((qi.shape[0], di.shape[0]), dtype=np.int64)
    shift = np.empty(out.shape, dtype=np.int8)
    for r in range(qi.shape[0]):
        best = best_s = None
        for s in shift_order(S):
            x0, x1 = max(0, -s), min(w, w - s)                       # the x with 0 <= x < w and 0 <= x + s < w
            sad = np.abs(qi[r][None, :, x0:x1] - di[:, :, x0 + s:x1 + s]).sum(axis=(1, 2), dtype=np.int64)
            v = (sad * np.int64(w)) // np.int64(w - abs(s))
            if best is None:
                best, best_s = v, np.zeros(v.shape, dtype=np.int8)
            else:
                better = v < best
                best = np.where(better, v, best)
                best_s = np.where(better, np.int8(s), best_s)
        out[r], shift[r] = best, best_s
    return out, shift


def shift_rows_composed(q, db, h, w, S):
    """The same from seqslam_oracle.sad_rows alone: per shift, contiguous cropped copies of both operands."""
    q, db = np.asarray(q), np.asarray(db)
    q3, d3 = q.reshape(-1, h, w), db.reshape(-1, h, w)
    best = shift = None
    for s in shift_order(S):
        k = abs(s)
        qc = q3[:, :, k:] if s < 0 else q3[:, :, :w - k]              # query columns x, key-frame columns x + s
        dc = d3[:, :, :w - k] if s < 0 else d3[:, :, k:]
        sad = sq.sad_rows(np.ascontiguousarray(qc).reshape(len(q3), -1), np.ascontiguousarray(dc).reshape(len(d3), -1))
        v = sad * w // (w - k)
        if best is None:
            best, shift = v, np.zeros(v.shape, dtype=np.int8)
        else:
            better = v < best
            best, shift = np.where(better, v, best), np.where(better, np.int8(s), shift)
    return best, shift
