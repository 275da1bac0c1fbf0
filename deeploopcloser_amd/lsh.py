"""Sign-random-projection hashes on MI355X: a float place descriptor -> a packed binary code that the Hamming path
(ldb.HammingKeyframeDatabase, LdbLoopClosureDetector and everything behind its rows) serves unchanged.

    lsh_planes                 the +-1 hyperplanes of a seed, int8 [n_bits, D]: a model file needs the seed only
    Lsh                        rows -> codes, uint8 [B, row bytes]: the mean taken off, each row scaled to int8
                               (dlc_lsh_quantize_i8), the sign of its integer products with the planes (dlc_lsh_hash_i8)

Bit t is the side of hyperplane t the row lies on, so for random planes P(a bit differs) = angle / pi (Charikar, STOC
2002), and a few hundred to a few thousand bits rank places nearly as the cosine does (Suenderhauf et al., IROS 2015): a
4096-wide bf16 descriptor, 8 KB a key-frame, becomes 128 bytes at 1024 bits.  The products are formed on int8 operands
on the matrix cores, so every sum is an exact integer: a code is a function of the row and the model alone, whatever
the batch or the launch plan.  Both definitions are stated in include/dlc.h.  HashedLoopClosureDetector
(loop_closure.py) is the streaming form.
"""
import numpy as np
import torch

from . import _lib as L
from .engine import default_engine

FIELDS = ("seed", "n_bits", "width", "mean")
_M64 = (1 << 64) - 1


def mix64(z):
    """The splitmix64 finaliser on uint64 arrays (anything np.asarray takes), all arithmetic mod 2^64:
    z += 0x9E3779B97F4A7C15; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9; z = (z ^ (z >> 27)) * 0x94D049BB133111EB;
    z ^ (z >> 31).  mix64(0) = 0xE220A8397B1DCDAF."""
    z = np.atleast_1d(np.asarray(z, dtype=np.uint64)) + np.uint64(0x9E3779B97F4A7C15)      # (arrays wrap silently)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def lsh_planes(n_bits, D, seed=0):
    """int8 [n_bits, D] of +-1, a function of (n_bits, D, seed) alone: with W = ceil(D / 64) and word(t, j) =
    mix64(mix64(seed) + t * W + j) (mod 2^64), planes[t][d] = +1 if bit d % 64 of word(t, d // 64) is set, else -1."""
    n_bits, D = int(n_bits), int(D)
    if not 1 <= n_bits <= L.DLC_LSH_MAX_BITS or not 1 <= D <= L.DLC_LSH_MAX_D:
        raise ValueError("lsh_planes: n_bits=%d outside 1..%d or D=%d outside 1..%d" % (n_bits, L.DLC_LSH_MAX_BITS, D, L.DLC_LSH_MAX_D))
    w = (D + 63) // 64
    base = mix64(np.array([int(seed) & _M64], dtype=np.uint64))
    index = np.arange(n_bits * w, dtype=np.uint64).reshape(n_bits, w)              # t * W + j
    words = mix64(base + index).astype("<u8")
    bits = np.unpackbits(words.view(np.uint8).reshape(n_bits, w * 8), axis=1, bitorder="little")[:, :D]
    return np.ascontiguousarray(bits.astype(np.int8) * np.int8(2) - np.int8(1))


class Lsh:
    """Lsh(n_bits=1024, seed=0, device=None, center=True): fit() learns the column mean of training rows (center=False: none, and
    fit() only fixes the width), transform() hashes rows [B, width] -> uint8 [B, dim].  Rows are float64, float32 or
    bfloat16 -- or int8, taken as already quantised, which needs center=False.  The planes are lsh_planes(n_bits, width,
    seed), kept on the device.  Codes of two models do not compare."""

    def __init__(self, n_bits=1024, seed=0, device=None, center=True):
        if int(n_bits) != n_bits or not 1 <= n_bits <= L.DLC_LSH_MAX_BITS:
            raise ValueError("Lsh: n_bits=%r outside 1..%d" % (n_bits, L.DLC_LSH_MAX_BITS))
        if int(seed) != seed or not 0 <= seed <= _M64:
            raise ValueError("Lsh: seed=%r outside 0..2^64-1" % (seed,))
        self.n_bits, self.seed, self.center = int(n_bits), int(seed), bool(center)
        self.engine = default_engine(device)
        self.mean = self.planes = None             # device tensors: float64 [width] (centred models), int8 [n_bits, width]
        self.width = None                          # columns of a row the model takes, D (None before there is one)

    @property
    def dim(self):
        """Bytes of a code: 16 * ceil(n_bits / 128)."""
        return 16 * ((self.n_bits + 127) // 128)

    def _set(self, width, mean):
        width = int(width)
        if not 1 <= width <= L.DLC_LSH_MAX_D:
            raise ValueError("Lsh: rows of %d columns outside 1..%d" % (width, L.DLC_LSH_MAX_D))
        dev = self.engine.device
        planes = torch.zeros((self.n_bits, (width + 15) // 16 * 16), dtype=torch.int8, device=dev)     # rows 16 bytes apart
        planes[:, :width] = torch.from_numpy(lsh_planes(self.n_bits, width, self.seed)).to(dev)
        self.planes, self.width = planes[:, :width], width
        self.mean = None
        if mean is not None:
            m = mean if isinstance(mean, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(mean, dtype=np.float64))
            self.mean = m.to(dev).to(torch.float64).contiguous()

    def fit(self, rows):
        """The column mean of `rows` [N, D] (NumPy or a tensor; taken as float64): dlc_kmeans_step's mean with one word,
        the defined mean Pca.fit uses.  center=False: only the width is taken."""
        t = rows if isinstance(rows, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(rows, dtype=np.float64)))
        if t.dim() != 2 or t.shape[0] < 1 or t.shape[1] < 1:
            raise ValueError("Lsh.fit: rows must be [rows, D]")
        mean = None
        if self.center:
            eng = self.engine
            x = t.to(eng.device).to(torch.float64).contiguous()
            if not bool(torch.isfinite(x).all().item()):
                raise ValueError("Lsh.fit: the rows hold a NaN or an infinity")
            mean = eng.kmeans_step(x, torch.zeros((1, x.shape[1]), dtype=torch.float64, device=eng.device))[0][0]
        self._set(t.shape[1], mean)
        return self

    def transform_tensor(self, x, out=None, plan="auto"):
        """[rows, width] on the device -> the codes uint8 [rows, dim] on the device.  out: a caller-kept uint8
        [rows, >= dim] tensor or row view, rows of a HammingKeyframeDatabase for one."""
        eng = self.engine
        x = eng.to_device(x) if not isinstance(x, torch.Tensor) or x.device != eng.device else x
        if x.dim() != 2:
            raise ValueError("Lsh.transform: rows must be [rows, D]")
        if self.width is None:
            if self.center:
                raise ValueError("Lsh.transform: no model -- fit() or load() first")
            self._set(x.shape[1], None)                            # (nothing to learn: the width is the first rows')
        if x.shape[1] != self.width:
            raise ValueError("Lsh.transform: the rows are %d wide, the model %d" % (x.shape[1], self.width))
        if x.dtype == torch.int8:
            if self.mean is not None:
                raise ValueError("Lsh.transform: int8 rows are taken as quantised already and need center=False")
            q = x
        else:
            if x.dtype not in (torch.float64, torch.float32, torch.bfloat16):
                x = x.to(torch.float64)
            q = eng.lsh_quantize(x, self.mean)
        return eng.lsh_hash(q, self.planes, out=out, plan=plan)

    def transform(self, x, plan="auto"):
        """As transform_tensor; a NumPy input (float64, float32 or int8; anything else as float64) gives a NumPy result."""
        if isinstance(x, torch.Tensor):
            return self.transform_tensor(x, plan=plan)
        a = np.asarray(x)
        if a.dtype not in (np.float64, np.float32, np.int8):
            a = a.astype(np.float64)
        return self.transform_tensor(self.engine.to_device(np.ascontiguousarray(a)), plan=plan).cpu().numpy()

    # ---- persistence ---------------------------------------------------------
    def save(self, path):
        """An .npz with seed, n_bits, width and mean (empty for a model that is not centred)."""
        if self.width is None:
            raise ValueError("Lsh.save: no model")
        with open(path, "wb") as f:              # (np.savez would append .npz to a bare name)
            np.savez(f, seed=np.array(self.seed, dtype=np.uint64), n_bits=np.array(self.n_bits, dtype=np.int64),
                     width=np.array(self.width, dtype=np.int64),
                     mean=self.mean.cpu().numpy() if self.mean is not None else np.zeros(0))

    @classmethod
    def load(cls, path, device=None):
        with np.load(path, allow_pickle=False) as z:
            missing = [k for k in FIELDS if k not in z.files]
            if missing:
                raise ValueError("Lsh.load: %s lacks %s" % (path, ", ".join(missing)))
            width, mean = int(z["width"]), np.asarray(z["mean"], dtype=np.float64)
            if mean.shape not in ((0,), (width,)):
                raise ValueError("Lsh.load: the mean of %s does not fit rows of %d columns" % (path, width))
            h = cls(int(z["n_bits"]), seed=int(z["seed"]), center=mean.shape[0] > 0, device=device)
            h._set(width, mean if mean.shape[0] else None)
        return h
