"""cnn_vtl descriptor distance with the reference's call surface
(src/cnn_vtl/similarity/DistanceCalculator.py:8-12) on MI355X, plus the full
N x N loop of src/cnn_vtl/create_distance_matrix.py:30-36 as one call."""
import numpy as np
import torch

from .engine import default_engine


class _PairBuffers:
    """Per-length buffers of the per-pair entry point: a caller that keeps the reference's O(N^2) Python loop
    (create_distance_matrix.py:30-36) calls it once per pair, so nothing is allocated per call -- a page-locked host row
    pair, its device image (rows padded to 16 bytes), the 2 x 2 result and a page-locked word to read it back into."""

    def __init__(self, engine, n):
        self.n = n
        self.ld = (n + 15) // 16 * 16
        self.host = torch.zeros((2, self.ld), dtype=torch.int8).pin_memory()
        self.host_np = self.host.numpy()
        self.dev = torch.zeros((2, self.ld), dtype=torch.int8, device=engine.device)
        self.out = torch.empty((2, 2), dtype=torch.int64, device=engine.device)
        self.res = torch.zeros((1,), dtype=torch.int64).pin_memory()


class DistanceCalculator:
    _pair = {}

    @staticmethod
    def calculate_distance(desc1, desc2):
        """sum_k popcount(|a_k ^ b_k|) on int8 (DistanceCalculator.py:4-12) -> numpy int64."""
        a = np.asarray(desc1, dtype=np.int8).reshape(-1)
        b = np.asarray(desc2, dtype=np.int8).reshape(-1)
        n = min(a.size, b.size)                                   # zip() stops at the shorter one
        if n == 0:
            return np.int64(0)
        e = default_engine()
        key = (e.device.index, n)
        buf = DistanceCalculator._pair.get(key)
        if buf is None:
            if len(DistanceCalculator._pair) > 16:
                DistanceCalculator._pair.clear()
            buf = DistanceCalculator._pair[key] = _PairBuffers(e, n)
        buf.host_np[0, :n] = a[:n]
        buf.host_np[1, :n] = b[:n]
        buf.dev.copy_(buf.host, non_blocking=True)
        e.cnnvtl_distance_matrix(buf.dev, d=n, out=buf.out)
        buf.res.copy_(buf.out.view(-1)[1:2], non_blocking=True)
        torch.cuda.current_stream(e.device).synchronize()
        return np.int64(buf.res[0].item())

    @staticmethod
    def distance_matrix(descriptors):
        """Full N x N matrix incl. the diagonal (create_distance_matrix.py:30-36), int64."""
        e = default_engine()
        d = e.to_device(descriptors, torch.int8)
        if d.dim() != 2:
            raise ValueError("descriptors must be [N, D] int8")
        return e.cnnvtl_distance_matrix(d).cpu().numpy()

    @staticmethod
    def distance_rows(queries, descriptors):
        """The per-pair loop for a rectangular set of pairs: calculate_distance(queries[r], descriptors[j]) for every
        r and j as one call (dlc_cnnvtl_distance_rows) -> numpy int64 [Q, N]."""
        q = np.ascontiguousarray(np.asarray(queries, dtype=np.int8))
        x = np.ascontiguousarray(np.asarray(descriptors, dtype=np.int8))
        if q.ndim != 2 or x.ndim != 2 or q.shape[1] != x.shape[1]:
            raise ValueError("distance_rows: queries [Q, D] and descriptors [N, D] with one D")
        e = default_engine()
        return e.cnnvtl_distance_rows(e.to_device(q, torch.int8), e.to_device(x, torch.int8)).cpu().numpy()


class _ByteRowStore:
    """What the resident byte-descriptor stores share (CnnVtlKeyframeDatabase here, seqslam.SadKeyframeDatabase): rows of
    `DTYPE` bytes zero-padded to a multiple of 16 (the row kernels' alignment) in a capacity-reserved buffer that doubles
    when an append() outgrows it; `rows` is the view of the first len(db) rows.  KIND names the descriptors in errors."""

    DTYPE, KIND = None, None

    def __init__(self, descriptors, capacity=None, device=None):
        self.engine = default_engine(device)
        x = self.engine.to_device(descriptors)
        if x.dim() != 2 or x.dtype != self.DTYPE:
            raise ValueError("%s descriptors must be [n, dim] %s" % (self.KIND, self._dtype_name()))
        if x.shape[1] < 1:
            raise ValueError("%s descriptors must have dim >= 1" % self.KIND)
        self.dim = int(x.shape[1])
        self._n = 0
        n = int(x.shape[0])
        cap = max(n, 1 if capacity is None else int(capacity))
        self._store = torch.zeros((cap, self.stored_width(self.dim)), dtype=self.DTYPE, device=self.engine.device)
        if n:
            self._store[:n, :self.dim] = x
            self._n = n

    @classmethod
    def _dtype_name(cls):
        return str(cls.DTYPE).split(".")[-1]

    @staticmethod
    def stored_width(dim):
        return (int(dim) + 15) // 16 * 16

    @classmethod
    def empty(cls, dim, capacity=4096, device=None):
        """A database of `dim`-byte descriptors with no key-frames yet and room for `capacity`."""
        if dim < 1 or capacity < 1:
            raise ValueError("%s.empty: dim and capacity must be positive" % cls.__name__)
        eng = default_engine(device)
        return cls(torch.empty((0, int(dim)), dtype=cls.DTYPE, device=eng.device), capacity=capacity, device=device)

    @property
    def rows(self):
        """[len, stored_width(dim)]: the stored rows, padding bytes included."""
        return self._store[:self._n]

    @property
    def capacity(self):
        return self._store.shape[0]

    def __len__(self):
        return self._n

    def reserve(self, capacity):
        """Room for at least `capacity` key-frames (one device-to-device copy when it grows)."""
        if capacity > self.capacity:
            grown = torch.zeros((int(capacity), self._store.shape[1]), dtype=self.DTYPE, device=self.engine.device)
            grown[:self._n] = self._store[:self._n]
            self._store = grown

    def append(self, descriptors):
        """Store further key-frames [B, dim]; returns their ids (first, last+1).  Stream-ordered on the current stream."""
        x = self.engine.to_device(descriptors)
        if x.dim() != 2 or x.dtype != self.DTYPE or x.shape[1] != self.dim:
            raise ValueError("append: descriptors must be [B, %d] %s" % (self.dim, self._dtype_name()))
        b = int(x.shape[0])
        if self._n + b > self.capacity:
            self.reserve(max(2 * self.capacity, self._n + b))
        self._store[self._n:self._n + b, :self.dim] = x
        first = self._n
        self._n += b
        return first, first + b

    def _queries(self, who, queries):
        """Query rows for the row kernels: [Q, dim], or stored rows [Q, stored_width(dim)] (the padding is ignored)."""
        q = self.engine.to_device(queries)
        if q.dim() == 1:
            q = q.unsqueeze(0)
        if q.dim() != 2 or q.dtype != self.DTYPE or q.shape[1] not in (self.dim, self._store.shape[1]):
            raise ValueError("%s: queries must be [Q, %d] %s" % (who, self.dim, self._dtype_name()))
        return q


class CnnVtlKeyframeDatabase(_ByteRowStore):
    """cnn_vtl key-frame descriptors (int8 [n, dim]) resident in HBM, searched by the reference's distance.

    Rows are stored zero-padded to a multiple of 16 bytes (the top-k kernel's row alignment) in a capacity-reserved
    buffer that doubles when an append() outgrows it; `rows` is the view of the first len(db) rows.  nearest() is
    dlc_cnnvtl_distance_topk: distance ascending, ties -> the lower id, (-1, -1) past the rows there are; distances() is
    dlc_cnnvtl_distance_rows: the [Q, len(db)] distances themselves, for callers that rank them another way (the
    sequence search)."""

    FORMAT = "dlc-cnnvtl-keyframes-v1"
    DTYPE, KIND = torch.int8, "cnn_vtl"

    def prefix(self, n):
        """The first n key-frames as a database of their own (a copy: a database owns its reservation)."""
        if not 0 <= n <= self._n:
            raise ValueError("prefix: n=%d outside 0..%d" % (n, self._n))
        return CnnVtlKeyframeDatabase(self._store[:n, :self.dim], device=self.engine.device)

    def nearest(self, queries, k, limit0=None, limit_step=0):
        """(dist [Q, k] int64, ids [Q, k] int64) on the device: the k stored key-frames nearest to each query row
        ([Q, dim] int8) by the reference's distance.  limit0 / limit_step: query r sees the first limit0 + r * limit_step
        key-frames (default: all)."""
        q = self.engine.to_device(queries)
        if q.dim() == 1:
            q = q.unsqueeze(0)
        if q.dim() != 2 or q.dtype != torch.int8 or q.shape[1] != self.dim:
            raise ValueError("nearest: queries must be [Q, %d] int8" % self.dim)
        return self.engine.cnnvtl_distance_topk(q, self.rows, int(k), d=self.dim,
                                                limit0=self._n if limit0 is None else limit0, limit_step=limit_step)

    def distances(self, queries, limit0=None, limit_step=0, out=None):
        """int64 [Q, len(self)] on the device: the reference's distance of each query row to every stored key-frame, as
        rows (dlc_cnnvtl_distance_rows).  queries: [Q, dim] int8, or stored rows [Q, stored_width(dim)] such as a slice
        of `rows` (the padding is ignored).  limit0 / limit_step: query r is written in its first limit0 + r * limit_step cells only (default: all); the others
        keep what `out` held (a caller-kept int64 [Q, len(self)] tensor or row-strided view), or hold -1 when the result
        is allocated here."""
        q = self._queries("distances", queries)
        return self.engine.cnnvtl_distance_rows(q, self.rows, d=self.dim, limit0=limit0, limit_step=limit_step, out=out)

    # ---- on-disk format: one .npz ------------------------------------------------------------------------------------
    def save(self, path):
        """The descriptors' raw bytes [n, dim] and dim."""
        np.savez(path, rows_i8=self.rows[:, :self.dim].cpu().numpy(), dim=np.array(self.dim, dtype=np.int64),
                 format=np.array(self.FORMAT))

    @classmethod
    def load(cls, path, capacity=None, device=None):
        z = np.load(path)
        if "format" not in z or str(z["format"]) != cls.FORMAT:
            raise ValueError("%s is not a %s file" % (path, cls.FORMAT))
        rows = z["rows_i8"].astype(np.int8, copy=False).reshape(-1, int(z["dim"]))
        return cls(torch.from_numpy(np.ascontiguousarray(rows)), capacity=capacity, device=device)


def distance_topk(desc_q, desc_db, k):
    """(dist [Q, k] int64, idx [Q, k] int64) numpy arrays: the k rows of desc_db [N, D] int8 nearest to each row of
    desc_q [Q, D] int8 by the reference's distance; distance ascending, ties -> the lower row, (-1, -1) past N."""
    q = np.ascontiguousarray(np.asarray(desc_q, dtype=np.int8))
    db = np.ascontiguousarray(np.asarray(desc_db, dtype=np.int8))
    if q.ndim != 2 or db.ndim != 2 or q.shape[1] != db.shape[1]:
        raise ValueError("distance_topk: desc_q [Q, D] and desc_db [N, D] with one D")
    e = default_engine()
    dist, idx = e.cnnvtl_distance_topk(e.to_device(q, torch.int8), e.to_device(db, torch.int8), int(k))
    return dist.cpu().numpy(), idx.cpu().numpy()
