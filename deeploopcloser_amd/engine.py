"""Thin host layer over the C ABI: holds tensors in PyTorch-ROCm, passes raw
device pointers + the current HIP stream to libdlc_hip.so.  PyTorch is used for
device memory, streams and torch.distributed only; every computation below
runs in the hand-written HIP kernels.
"""
import collections
import contextlib
import ctypes as C
import weakref

import numpy as np
import torch

from . import _lib as L

_TORCH_TO_DLC = {torch.bfloat16: L.DLC_BF16, torch.float16: L.DLC_F16, torch.float32: L.DLC_F32,
                 torch.float64: L.DLC_F64, torch.int8: L.DLC_I8}
_NAME_TO_TORCH = {"bf16": torch.bfloat16, "bfloat16": torch.bfloat16, "f16": torch.float16, "fp16": torch.float16,
                  "float16": torch.float16, "f32": torch.float32, "float32": torch.float32, "f64": torch.float64,
                  "float64": torch.float64}

SCRATCH_BYTES = 256 << 20   # default split-K scratch per engine (Engine.set_scratch)
K_STEP = 64   # the score GEMM's K step: stored descriptor rows are padded to a multiple of it


TopK = collections.namedtuple("TopK", "scores idx scores_f64 status")


_RAW_STREAM = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def torch_dtype(name):
    if isinstance(name, torch.dtype):
        return name
    try:
        return _NAME_TO_TORCH[str(name).lower()]
    except KeyError:
        raise ValueError("unknown dtype %r" % (name,))


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _limits(n, limit0, limit_step):
    """(limit0, limit_step) as the library takes them: row r offers its first clamp(limit0 + r * limit_step, 0, n) cells,
    limit0 None = n."""
    return n if limit0 is None else int(limit0), int(limit_step)


def _absent(absent):
    """(has_absent, absent) as the library takes them; None: no value marks a cell as absent."""
    return int(absent is not None), 0 if absent is None else int(absent)


def check_steps(steps):
    """(d_min, d_max) of an elastic sequence search's steps, checked: two integers, 0 <= d_min <= d_max <= 8."""
    try:
        d_min, d_max = steps
        ok = int(d_min) == d_min and int(d_max) == d_max and 0 <= d_min <= d_max <= L.DLC_MAX_STEP
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError("steps=%r: need (d_min, d_max) with 0 <= d_min <= d_max <= %d" % (steps, L.DLC_MAX_STEP))
    return int(d_min), int(d_max)


class Engine:
    """One engine per device / rank (wraps a dlc_ctx)."""

    def __init__(self, device=None):
        self.lib = L.load()
        if not torch.cuda.is_available():
            raise RuntimeError("deeploopcloser_amd needs a visible MI355X (torch.cuda.is_available() is False); "
                               "there is no CPU fallback")
        if device is None:
            device = torch.cuda.current_device()
        self.device = torch.device("cuda", device if isinstance(device, int) else torch.device(device).index or 0)
        self._dev_index = self.device.index
        ctx = C.c_void_p()
        rc = self.lib.dlc_create(self.device.index, C.byref(ctx))
        if rc != L.DLC_OK:
            raise L.DlcError("dlc_create(%d) failed: %s" % (self.device.index, self.lib.dlc_status_string(rc).decode()))
        self.ctx = ctx
        self._ws = {}
        self._scratch = None
        # The copy streams of run_chunked / for_each_chunk, created NOW and touched once: the HIP runtime deals its few
        # hardware queues (4 by default) to streams in the order they come to life, and two streams on one queue run one
        # after the other.  Created lazily -- behind whatever streams the application had made by then (a MatchPipeline per
        # database, ...) -- an upload stream landed on the compute stream's queue and upload, kernels and download of
        # SDAV.transform(ndarray) stopped overlapping: 47 ms instead of 36 (docs/LAB.md 11.6; GPU_MAX_HW_QUEUES=8 hid it).
        self._s_in, self._s_out = torch.cuda.Stream(device=self.device), torch.cuda.Stream(device=self.device)
        # ONE second stream per engine, shared by every MatchPipeline of the engine and by SDAV.train_steps' mask draws: the
        # default four hardware queues are taken (caller's stream, upload, download, this one) and a fifth stream would
        # share a queue with one of them.  Users of it are ordered among themselves (two pipelines' select / exchange /
        # merge stages run one behind the other; results are the same, ordering is by events); an application that needs
        # two pipelines overlapping independently gives each its own Engine (dlc_create is cheap) -- one per database.
        self.side_stream = torch.cuda.Stream(device=self.device)
        for st in (self._s_in, self._s_out, self.side_stream):
            torch.cuda.Event().record(st)

    def set_scratch(self, nbytes=SCRATCH_BYTES):
        """Latency mode: lend the context `nbytes` of HBM for the split-K form of the dense GEMMs
        (a single frame: SDAV layers with 30 rows, conv3-5 with 130 output pixels -- 5-8x lower
        encode latency); 0 turns it off.  OFF by default: one-pass GEMMs make an encode bit-identical
        whatever the batch it is part of, split-K changes the summation order (by ~1e-16 relative)."""
        torch.cuda.synchronize(self.device)         # nothing in flight may still use the old buffer
        t = torch.empty(int(nbytes), dtype=torch.uint8, device=self.device) if nbytes else None
        self._check(self.lib.dlc_set_scratch(self.ctx, _ptr(t) if t is not None else None, int(nbytes)))
        self._scratch = t              # keeps the previous buffer alive until the context has the new one

    @contextlib.contextmanager
    def latency_mode(self, nbytes=SCRATCH_BYTES):
        """`with engine.latency_mode():` -- split-K scratch on inside the block (no-op if already on)."""
        if self._scratch is not None:
            yield
            return
        self.set_scratch(nbytes)
        try:
            yield
        finally:
            self.set_scratch(0)

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.dlc_destroy(self.ctx)
            self.ctx = None
            self._scratch = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- helpers -------------------------------------------------------------
    def _check(self, rc):
        L.raise_for_status(self.lib, self.ctx, rc)

    def _raw_stream(self):
        """The current stream's handle as an int (torch._C._cuda_getCurrentRawStream: a tenth of the cost of building a
        torch.cuda.Stream object, which three calls per batch of a streaming detector made a quarter of its host time)."""
        if _RAW_STREAM is not None:
            return _RAW_STREAM(self._dev_index)
        return torch.cuda.current_stream(self.device).cuda_stream      # (a torch build without the private fast path)

    def _stream(self):
        return C.c_void_p(self._raw_stream())

    WORKSPACE_STREAMS = 4      # per name: the workspaces of at most this many streams are kept (least recently used out)

    def workspace(self, key, nbytes):
        """Named scratch tensor of at least nbytes, one per (name, current stream): calls on different streams must not
        share a workspace (a match keeps its group maxima there between its kernels).  A caller that rotates streams
        does not grow memory without bound: per name the WORKSPACE_STREAMS most recently used streams keep theirs, an
        evicted one is released once its stream has finished with it (the caching allocator's record_stream)."""
        nbytes = max(int(nbytes), 256)
        k = (key, self._raw_stream())
        t = self._ws.pop(k, None)
        if t is None or t.numel() < nbytes:
            t = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        self._ws[k] = t                                   # (re-)inserted last: dicts keep insertion order
        if len(self._ws) <= self.WORKSPACE_STREAMS:       # (cannot hold more than that many of one name)
            return t
        same = [kk for kk in self._ws if kk[0] == key]
        for kk in same[:max(0, len(same) - self.WORKSPACE_STREAMS)]:
            old = self._ws.pop(kk)
            old.record_stream(torch.cuda.ExternalStream(kk[1], device=self.device) if kk[1] else torch.cuda.default_stream(self.device))
        return t

    def _check_out(self, name, t, shape, dtype):
        """Caller-supplied buffers reach the kernels as raw pointers: refuse anything that is not exactly
        the contiguous tensor the kernel will write."""
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != tuple(shape) or t.dtype != dtype or \
                not t.is_contiguous() or t.device != self.device:
            raise ValueError("%s must be a contiguous %s tensor of shape %s on %s" % (name, dtype, tuple(shape), self.device))
        return t

    @staticmethod
    def _wrote(t):
        """The library has written (or is about to write) t through its raw pointer: torch must see that as the in-place
        write it is -- the version counter t shares with its base and its views moves, and whatever was derived from the
        old contents and keyed on the version (the unit_rows() mark) is outdated, as after any torch-side write."""
        torch.autograd.graph.increment_version(t)

    def to_device(self, x, dtype=None):
        if isinstance(x, torch.Tensor):
            t = x.to(self.device)
            if dtype is not None and t.dtype != dtype:
                t = t.to(dtype)
            return t.contiguous()
        a = np.ascontiguousarray(np.asarray(x))
        t = self.upload(a) if a.nbytes >= self.STAGED_MIN_BYTES else None
        if t is None:
            if not a.flags.writeable:
                a = a.copy()
            t = torch.from_numpy(a).to(self.device)
        if dtype is not None and t.dtype != dtype:
            t = t.to(dtype)
        return t

    # ---- pageable host arrays <-> HBM through the context's pinned staging ring (dlc_host_to_device / dlc_device_to_host)
    STAGED_MIN_BYTES = 4 << 20

    @staticmethod
    def _torch_dtype_of(a):
        try:
            return torch.from_numpy(np.empty(0, dtype=a.dtype)).dtype
        except TypeError:
            return None

    def upload(self, a, out=None, stream=None):
        """C-contiguous numpy array -> device tensor of the same shape / dtype (None if torch has no such dtype).
        Returns when `a` has been consumed; the tensor is ready in `stream` order (default: the current stream)."""
        dt = self._torch_dtype_of(a)
        if dt is None or not a.flags.c_contiguous:
            return None
        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        if out is None:
            with torch.cuda.stream(st):
                out = torch.empty(a.shape, dtype=dt, device=self.device)
        else:
            self._wrote(out)
        if a.nbytes:
            self._check(self.lib.dlc_host_to_device(self.ctx, C.c_void_p(out.data_ptr()), C.c_void_p(a.ctypes.data), a.nbytes,
                                                     C.c_void_p(st.cuda_stream)))
        return out

    # Result arrays handed to the caller.  A fresh pageable array costs the kernel a page fault and a zeroed page per
    # 4 KiB (638 MB of SDAV descriptors: 24 ms on top of a 13 ms copy), so large results live in page-locked blocks of
    # torch's caching host allocator instead: an ordinary ndarray for the caller (its base keeps the block), filled by
    # the DMA engine directly -- no staging copy -- and recycled once the caller drops it.  At most PINNED_RESULT_CAP
    # bytes of such results are alive at a time; past that (a caller that keeps everything) results are pageable again.
    PINNED_RESULT_CAP = 4 << 30
    _pinned_live = 0

    def _release_pinned(self, nbytes):
        self._pinned_live -= nbytes

    def result_array(self, shape, torch_dt):
        """(ndarray, pinned uint8 tensor behind it or None) for a result of `shape` / torch dtype."""
        np_dt = torch.empty(0, dtype=torch_dt).numpy().dtype
        nbytes = int(np.prod(shape, dtype=np.int64)) * np_dt.itemsize
        if nbytes >= self.STAGED_MIN_BYTES and self._pinned_live + nbytes <= self.PINNED_RESULT_CAP:
            try:
                t = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
            except RuntimeError:
                t = None
            if t is not None:
                self._pinned_live += nbytes
                weakref.finalize(t, self._release_pinned, nbytes)
                return t.numpy().view(np_dt).reshape(shape), t
        return np.empty(shape, dtype=np_dt), None

    def download(self, t, out=None, stream=None):
        """Device tensor -> numpy array (a fresh one, or `out`: C-contiguous, same bytes), read in `stream` order; blocks
        until the array is complete."""
        t = t.contiguous()
        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        if out is None:
            out, pin = self.result_array(tuple(t.shape), t.dtype)
            if pin is not None:
                with torch.cuda.stream(st):
                    pin.copy_(t.reshape(-1).view(torch.uint8), non_blocking=True)
                st.synchronize()
                return out
        if out.nbytes != t.numel() * t.element_size() or not out.flags.c_contiguous:
            raise ValueError("download: out must be a C-contiguous array of %d bytes" % (t.numel() * t.element_size()))
        if out.nbytes:
            self._check(self.lib.dlc_device_to_host(self.ctx, C.c_void_p(out.ctypes.data), C.c_void_p(t.data_ptr()), out.nbytes,
                                                     C.c_void_p(st.cuda_stream)))
        return out

    def run_chunked(self, x, chunk, compute):
        """The reference's NumPy-in / NumPy-out contract without serialising on the link: x [N, ...] (numpy) is cut
        into chunks of `chunk` items; the upload of chunk c+1 (copy stream 1), compute(device chunk) -> device tensor
        of chunk c (the current stream) and the download of chunk c-1's result (copy stream 2, into the returned
        array) overlap.  compute must be batch-invariant (every kernel of this library is); results are concatenated
        along dimension 0."""
        x = np.ascontiguousarray(x)
        n = x.shape[0]
        dev = self.device
        dt = self._torch_dtype_of(x)
        if dt is None:
            raise ValueError("run_chunked: unsupported array dtype %s" % x.dtype)
        cur = torch.cuda.current_stream(dev)
        chunk = max(1, min(int(chunk), n))
        bufs = [torch.empty((chunk,) + tuple(x.shape[1:]), dtype=dt, device=dev) for _ in range(2 if n > chunk else 1)]
        self._s_in.wait_stream(cur)                 # the buffers' memory may still be in use by earlier work of this stream
        free_ev = [None, None]
        state = {"out": None, "pin": None, "row": 0}
        pend = None

        def flush(y, done, items):
            if state["out"] is None:
                per = y.shape[0] // items
                state["out"], state["pin"] = self.result_array((n * per,) + tuple(y.shape[1:]), y.dtype)
            self._s_out.wait_event(done)
            r0 = state["row"]
            if state["pin"] is not None:              # page-locked result: the DMA engine writes it, nobody waits
                row_bytes = y.numel() // max(1, y.shape[0]) * y.element_size()
                with torch.cuda.stream(self._s_out):
                    state["pin"][r0 * row_bytes:(r0 + y.shape[0]) * row_bytes].copy_(y.reshape(-1).view(torch.uint8), non_blocking=True)
                y.record_stream(self._s_out)
            else:
                self.download(y, out=state["out"][r0:r0 + y.shape[0]], stream=self._s_out)
            state["row"] = r0 + y.shape[0]

        for c, lo in enumerate(range(0, n, chunk)):
            hi = min(lo + chunk, n)
            b = c % len(bufs)
            if free_ev[b] is not None:
                self._s_in.wait_event(free_ev[b])     # chunk c-2's kernels have read this buffer
            self.upload(x[lo:hi], out=bufs[b][:hi - lo], stream=self._s_in)
            up = torch.cuda.Event()
            up.record(self._s_in)
            cur.wait_event(up)
            y = compute(bufs[b][:hi - lo]).contiguous()
            done = torch.cuda.Event()
            done.record(cur)
            free_ev[b] = done
            if pend is not None:
                flush(*pend)                          # blocks the host while the GPU works on chunk c
            pend = (y, done, hi - lo)
        if pend is not None:
            flush(*pend)
        cur.wait_stream(self._s_in)
        self._s_out.synchronize()                     # the result is complete in host memory
        return state["out"]

    def for_each_chunk(self, x, chunk, consume, first=None):
        """The upload half of run_chunked for results that STAY on the device: x [N, ...] (numpy, pageable) is cut into
        chunks of `chunk` items, the upload of chunk c+1 (copy stream, pinned staging ring) overlaps consume(device
        chunk, lo, hi) of chunk c on the current stream.  consume must be done with its chunk in stream order (it may keep
        results, not the chunk: the two buffers are reused).  first: items of the first chunk (default `chunk`) -- nothing
        overlaps ITS upload, so a short first chunk starts the kernels sooner.  Returns when everything has been
        SUBMITTED; the current stream is ordered behind the last upload."""
        x = np.ascontiguousarray(x)
        n = x.shape[0]
        dev = self.device
        dt = self._torch_dtype_of(x)
        if dt is None:
            raise ValueError("for_each_chunk: unsupported array dtype %s" % x.dtype)
        cur = torch.cuda.current_stream(dev)
        chunk = max(1, min(int(chunk), n))
        first = chunk if first is None else max(1, min(int(first), chunk))
        bufs = [torch.empty((chunk,) + tuple(x.shape[1:]), dtype=dt, device=dev) for _ in range(2 if n > first else 1)]
        self._s_in.wait_stream(cur)                 # the buffers' memory may still be in use by earlier work of this stream
        free_ev = [None, None]
        starts = [0] + list(range(first, n, chunk))
        for c, lo in enumerate(starts):
            hi = min(lo + (first if c == 0 else chunk), n)
            b = c % len(bufs)
            if free_ev[b] is not None:
                self._s_in.wait_event(free_ev[b])     # chunk c-2's kernels have read this buffer
            self.upload(x[lo:hi], out=bufs[b][:hi - lo], stream=self._s_in)
            up = torch.cuda.Event()
            up.record(self._s_in)
            cur.wait_event(up)
            consume(bufs[b][:hi - lo], lo, hi)
            free_ev[b] = torch.cuda.Event()
            free_ev[b].record(cur)
        for b_ in bufs:
            b_.record_stream(cur)

    # ---- dense layers -----------------------------------------------------------
    def gemm_bias_act(self, a, b, bias=None, act=L.DLC_ACT_NONE, blayout=L.DLC_B_KN, out=None):
        """out[M,N] = act(a[M,K] . b + bias) in a's dtype (float64 / float32)."""
        if a.dim() != 2 or b.dim() != 2:
            raise ValueError("gemm_bias_act: operands must be 2-D")
        if a.dtype not in (torch.float64, torch.float32) or b.dtype != a.dtype:
            raise ValueError("gemm_bias_act: float64 or float32 operands of one dtype")
        a, b = a.contiguous(), b.contiguous()
        m, k = a.shape
        n = b.shape[1] if blayout == L.DLC_B_KN else b.shape[0]
        kb = b.shape[0] if blayout == L.DLC_B_KN else b.shape[1]
        if kb != k:
            raise ValueError("gemm_bias_act: inner dimensions differ (%d vs %d)" % (k, kb))
        if bias is not None:
            bias = bias.contiguous()
            if bias.numel() != n or bias.dtype != a.dtype:
                raise ValueError("gemm_bias_act: bias must be [N] of the operand dtype")
        if out is None:
            out = torch.empty((m, n), dtype=a.dtype, device=self.device)
        elif not isinstance(out, torch.Tensor) or tuple(out.shape) != (m, n) or out.dtype != a.dtype or \
                out.stride(1) != 1 or out.stride(0) < n or out.device != self.device:
            raise ValueError("gemm_bias_act: out must be a [%d, %d] %s tensor with unit column stride on %s"
                             % (m, n, a.dtype, self.device))
        self._check(self.lib.dlc_gemm_bias_act(self.ctx, _TORCH_TO_DLC[a.dtype], blayout, act, m, n, k, _ptr(a),
                                                a.stride(0), _ptr(b), b.stride(0), _ptr(bias), _ptr(out),
                                                out.stride(0), self._stream()))
        return out

    def bias_act(self, a, bias=None, act=L.DLC_ACT_NONE):
        a = a.contiguous()
        a2 = a.reshape(-1, a.shape[-1])
        out = torch.empty_like(a2)
        if bias is not None:
            bias = bias.to(a.dtype).contiguous()
            if bias.numel() != a2.shape[1]:
                raise ValueError("bias_act: bias must have the row width")
        self._check(self.lib.dlc_bias_act(self.ctx, _TORCH_TO_DLC[a.dtype], act, a2.shape[0], a2.shape[1], _ptr(a2),
                                           a2.stride(0), _ptr(bias), _ptr(out), out.stride(0), self._stream()))
        return out.reshape(a.shape)

    def _encode_out(self, out, rows, cols, dt, what):
        """The caller's result tensor for an encode ([rows, cols], contiguous, on this device), or a new one."""
        if out is None:
            return torch.empty((rows, cols), dtype=dt, device=self.device)
        if out.dtype != dt or tuple(out.shape) != (rows, cols) or not out.is_contiguous() or out.device != self.device:
            raise ValueError("%s: out must be a contiguous %s [%d, %d] tensor on %s" % (what, dt, rows, cols, self.device))
        return out

    def sdav_encode(self, x2d, weights, biases, out=None):
        """sigmoid chain on x2d [rows, K0]; weights[l] is [dims[l], dims[l+1]].  out: where the result goes (a caller that
        collects the chunks of a sequence hands its slice: no copy behind the call)."""
        dt = x2d.dtype
        if dt not in (torch.float64, torch.float32):
            raise ValueError("sdav_encode: float64 or float32")
        x2d = x2d.contiguous()
        n_layers = len(weights)
        dims = [x2d.shape[1]] + [w.shape[1] for w in weights]
        for l, w in enumerate(weights):
            if w.dtype != dt or w.shape[0] != dims[l] or not w.is_contiguous():
                raise ValueError("sdav_encode: W[%d] must be a contiguous [%d, *] %s tensor" % (l, dims[l], dt))
        rows = x2d.shape[0]
        dims_c = (C.c_int64 * (n_layers + 1))(*dims)
        w_c = (C.c_void_p * n_layers)(*[w.data_ptr() for w in weights])
        b_c = (C.c_void_p * n_layers)(*[(b.data_ptr() if b is not None else 0) for b in biases])
        need = self.lib.dlc_sdav_encode_workspace_bytes(rows, dims_c, n_layers, _TORCH_TO_DLC[dt])
        ws = self.workspace("sdav", need)
        out = self._encode_out(out, rows, dims[-1], dt, "sdav_encode")
        self._check(self.lib.dlc_sdav_encode(self.ctx, _TORCH_TO_DLC[dt], rows, n_layers, dims_c, _ptr(x2d), w_c, b_c,
                                              _ptr(out), _ptr(ws), ws.numel(), self._stream()))
        return out

    def sdav_split_panels(self, weights):
        """The tolerance-mode encoder's prepared weights (dlc_sdav_split_prepare): fp64 weights [dims[l], dims[l+1]] -> one
        uint8 device tensor holding, per layer, the two transposed fp16 pieces of W 2^s and 2^s."""
        n_layers = len(weights)
        dims = [weights[0].shape[0]] + [w.shape[1] for w in weights]
        for l, w in enumerate(weights):
            if w.dtype != torch.float64 or w.shape[0] != dims[l] or not w.is_contiguous() or w.device != self.device:
                raise ValueError("sdav_split_panels: W[%d] must be a contiguous float64 [%d, *] tensor on %s" % (l, dims[l], self.device))
        dims_c = (C.c_int64 * (n_layers + 1))(*dims)
        need = self.lib.dlc_sdav_split_panels_bytes(n_layers, dims_c)
        panels = torch.empty(int(need), dtype=torch.uint8, device=self.device)
        w_c = (C.c_void_p * n_layers)(*[w.data_ptr() for w in weights])
        self._check(self.lib.dlc_sdav_split_prepare(self.ctx, n_layers, dims_c, w_c, _ptr(panels), panels.numel(), self._stream()))
        return panels

    def sdav_encode_split(self, x2d, dims, panels, biases, out=None):
        """The sigmoid chain on x2d [rows, dims[0]] (fp64) in the tolerance mode (three fp16 MFMA products per layer,
        include/dlc.h: dlc_sdav_encode_split) -> fp64 [rows, dims[-1]]."""
        if x2d.dtype != torch.float64 or x2d.dim() != 2 or x2d.shape[1] != dims[0]:
            raise ValueError("sdav_encode_split: x must be float64 [rows, %d]" % dims[0])
        x2d = x2d.contiguous()
        n_layers = len(dims) - 1
        rows = x2d.shape[0]
        dims_c = (C.c_int64 * (n_layers + 1))(*dims)
        b_c = (C.c_void_p * n_layers)(*[(b.data_ptr() if b is not None else 0) for b in biases])
        need = self.lib.dlc_sdav_encode_split_workspace_bytes(rows, dims_c, n_layers)
        ws = self.workspace("sdav_split", need)
        out = self._encode_out(out, rows, dims[-1], torch.float64, "sdav_encode_split")
        self._check(self.lib.dlc_sdav_encode_split(self.ctx, rows, n_layers, dims_c, _ptr(x2d), _ptr(panels), b_c, _ptr(out),
                                                    _ptr(ws), ws.numel(), self._stream()))
        return out

    # ---- CnnVtl tolerance mode (include/dlc.h: dlc_cnnvtl_encode_split) --------------------
    @staticmethod
    def _conv_geom_c(geom):
        """geom: per layer (kh, kw, cin, cout, stride, pad_top, pad_left, oh, ow, act, pool) -> the C int32 array."""
        flat = [int(v) for g in geom for v in g]
        if not geom or len(flat) != 11 * len(geom):
            raise ValueError("geometry: 11 integers per layer")
        return (C.c_int32 * len(flat))(*flat)

    def cnnvtl_split_panels(self, geom, weights):
        """The tolerance-mode CnnVtl's prepared weights (dlc_cnnvtl_split_prepare): fp64 kernels [kh*kw*cin, cout] -> one
        uint8 device tensor holding, per layer, the two fp16 pieces of W 2^s and 2^s."""
        n_layers = len(geom)
        for l, (g, w) in enumerate(zip(geom, weights)):
            if w.dtype != torch.float64 or tuple(w.shape) != (g[0] * g[1] * g[2], g[3]) or not w.is_contiguous() or w.device != self.device:
                raise ValueError("cnnvtl_split_panels: W[%d] must be a contiguous float64 [%d, %d] tensor on %s"
                                 % (l, g[0] * g[1] * g[2], g[3], self.device))
        geom_c = self._conv_geom_c(geom)
        need = self.lib.dlc_cnnvtl_split_panels_bytes(n_layers, geom_c)
        if need == 0:
            raise ValueError("cnnvtl_split_panels: bad geometry")
        panels = torch.empty(int(need), dtype=torch.uint8, device=self.device)
        w_c = (C.c_void_p * n_layers)(*[w.data_ptr() for w in weights])
        self._check(self.lib.dlc_cnnvtl_split_prepare(self.ctx, n_layers, geom_c, w_c, _ptr(panels), panels.numel(), self._stream()))
        return panels

    def _cnnvtl_split_ws(self, n, h, w, c, geom_c, n_layers):
        need = self.lib.dlc_cnnvtl_encode_split_workspace_bytes(n, h, w, c, n_layers, geom_c)
        if need == 0:
            raise ValueError("cnnvtl tolerance mode: bad shape or geometry (1 .. 65535 frames per call)")
        return self.workspace("cnnvtl_split", need)

    def cnnvtl_encode_split(self, x, geom, s2d, panels, biases, columns, status, feats=False):
        """Frames x [n, h, w, c] (uint8, float32 or float64, on the device) -> int8 [n, columns.numel()] in the tolerance
        mode (dlc_cnnvtl_encode_split).  status: int32 [1] device tensor the call ORs its non-finite flags into.
        feats=True: also the layers' pre-quantisation fp32 outputs, (bytes, [fp32 [n, oh, ow, cout] per layer])."""
        dt = {torch.uint8: L.DLC_U8, torch.float32: L.DLC_F32, torch.float64: L.DLC_F64}.get(x.dtype)
        if dt is None or x.dim() != 4 or x.device != self.device:
            raise ValueError("cnnvtl_encode_split: frames must be a uint8 / float32 / float64 [n, h, w, c] tensor on %s" % self.device)
        x = x.contiguous()
        n, h, w, c = x.shape
        n_layers = len(geom)
        geom_c = self._conv_geom_c(geom)
        ws = self._cnnvtl_split_ws(n, h // s2d, w // s2d, c * s2d * s2d, geom_c, n_layers)
        b_c = (C.c_void_p * n_layers)(*[(b.data_ptr() if b is not None else 0) for b in biases])
        out = torch.empty((n, columns.numel()), dtype=torch.int8, device=self.device)
        fs = [torch.empty((n, g[7], g[8], g[3]), dtype=torch.float32, device=self.device) for g in geom] if feats else None
        f_c = (C.c_void_p * n_layers)(*[f.data_ptr() for f in fs]) if feats else None
        self._check(self.lib.dlc_cnnvtl_encode_split(self.ctx, dt, _ptr(x), n, h, w, c, s2d, n_layers, geom_c, _ptr(panels), b_c,
                                                      _ptr(columns), columns.numel(), _ptr(out), f_c, _ptr(status), _ptr(ws),
                                                      ws.numel(), self._stream()))
        return (out, fs) if feats else out

    def cnnvtl_layers_split(self, x, in_shape, geom, layer_a, layer_b, panels, biases, status=None):
        """Debug / test entry (dlc_cnnvtl_layers_split): layers layer_a .. layer_b of the tolerance mode on x, layer_a's own
        fp32 input [n, h, w, c]; in_shape = (h, w, c) of LAYER 0's input.  -> the layers' fp32 outputs."""
        if x.dtype != torch.float32 or x.dim() != 4 or x.device != self.device:
            raise ValueError("cnnvtl_layers_split: x must be a float32 [n, h, w, c] tensor on %s" % self.device)
        x = x.contiguous()
        n = x.shape[0]
        n_layers = len(geom)
        geom_c = self._conv_geom_c(geom)
        ws = self._cnnvtl_split_ws(n, in_shape[0], in_shape[1], in_shape[2], geom_c, n_layers)
        b_c = (C.c_void_p * n_layers)(*[(b.data_ptr() if b is not None else 0) for b in biases])
        if status is None:
            status = torch.zeros(1, dtype=torch.int32, device=self.device)
        fs = [torch.empty((n, g[7], g[8], g[3]), dtype=torch.float32, device=self.device) for g in geom[layer_a:layer_b + 1]]
        f_c = (C.c_void_p * len(fs))(*[f.data_ptr() for f in fs])
        self._check(self.lib.dlc_cnnvtl_layers_split(self.ctx, _ptr(x), n, in_shape[0], in_shape[1], in_shape[2], n_layers, geom_c,
                                                      layer_a, layer_b, _ptr(panels), b_c, f_c, _ptr(status), _ptr(ws), ws.numel(),
                                                      self._stream()))
        return fs

    def train_workspace(self, layer, batch, patches, weights):
        """A workspace tensor of dlc_sdav_train_step's size for this shape (for a caller that keeps its own)."""
        n_layers = len(weights)
        dims = [weights[0].shape[0]] + [w.shape[1] for w in weights]
        dims_c = (C.c_int64 * (n_layers + 1))(*dims)
        need = self.lib.dlc_sdav_train_workspace_bytes(batch, patches, dims_c, n_layers, layer)
        if need == 0:
            raise ValueError("sdav_train_step: batch must be >= 2 frames, layer in range")
        return torch.empty(int(need), dtype=torch.uint8, device=self.device)

    def sdav_train_step(self, layer, x2d, batch, patches, masks, weights, b_enc, b_dec, sparse_level, sparse_penalty,
                        consecutive_penalty, learning_rate, loss_out=None, ws=None):
        """One in-place SGD step of `layer` (fp64 tensors on this device); loss_out: 4 doubles; ws: the caller's own
        workspace (train_workspace) instead of the engine's."""
        n_layers = len(weights)
        dims = [weights[0].shape[0]] + [w.shape[1] for w in weights]
        dims_c = (C.c_int64 * (n_layers + 1))(*dims)
        for t in [x2d] + list(masks[:layer + 1]) + list(weights[:layer + 1]) + list(b_enc[:layer + 1]) + [b_dec]:
            if t.dtype != torch.float64 or not t.is_contiguous():
                raise ValueError("sdav_train_step: contiguous float64 tensors expected")
        m_c = (C.c_void_p * n_layers)(*[(masks[l].data_ptr() if l <= layer else 0) for l in range(n_layers)])
        w_c = (C.c_void_p * n_layers)(*[w.data_ptr() for w in weights])
        b_c = (C.c_void_p * n_layers)(*[b.data_ptr() for b in b_enc])
        need = self.lib.dlc_sdav_train_workspace_bytes(batch, patches, dims_c, n_layers, layer)
        if need == 0:
            raise ValueError("sdav_train_step: batch must be >= 2 frames, layer in range")
        if ws is None:
            ws = self.workspace("train", need)
        else:
            self._check_ws(ws)
        self._check(self.lib.dlc_sdav_train_step(self.ctx, layer, batch, patches, n_layers, dims_c, _ptr(x2d), m_c, w_c,
                                                  b_c, _ptr(b_dec), float(sparse_level), float(sparse_penalty),
                                                  float(consecutive_penalty), float(learning_rate), _ptr(loss_out),
                                                  _ptr(ws), ws.numel(), self._stream()))

    def random_mask(self, out, n_zeros, seed, counter):
        """Exactly n_zeros zeros among ones, uniformly placed, into the fp64 tensor `out` (dlc_random_mask_f64)."""
        if out.dtype != torch.float64 or not out.is_contiguous() or out.device != self.device:
            raise ValueError("random_mask: contiguous float64 tensor on %s expected" % (self.device,))
        self._check(self.lib.dlc_random_mask_f64(self.ctx, _ptr(out), out.numel(), int(n_zeros), int(seed) & (2 ** 64 - 1),
                                                  int(counter) & (2 ** 64 - 1), self._stream()))
        return out

    def salt_pepper_mask(self, zeros, ones, n_zeros, seed, counter):
        """The DA's static salt-and-pepper masks (dlc_salt_pepper_mask_f64) into two fp64 tensors of one size: exactly
        n_zeros zeros in `zeros`, and in `ones` a fair bit (salt) at each of those zeros, 0 elsewhere."""
        for name, t in (("zeros", zeros), ("ones", ones)):
            if t.dtype != torch.float64 or not t.is_contiguous() or t.device != self.device:
                raise ValueError("salt_pepper_mask: %s must be a contiguous float64 tensor on %s" % (name, self.device))
        if zeros.numel() != ones.numel() or zeros.data_ptr() == ones.data_ptr():
            raise ValueError("salt_pepper_mask: two distinct tensors of one size")
        self._check(self.lib.dlc_salt_pepper_mask_f64(self.ctx, _ptr(zeros), _ptr(ones), zeros.numel(), int(n_zeros),
                                                       int(seed) & (2 ** 64 - 1), int(counter) & (2 ** 64 - 1),
                                                       self._stream()))
        return zeros, ones

    @staticmethod
    def even_pitch(cols):
        """The row pitch of a corrupted input x~ (dlc_da_corrupt_f64 / dlc_da_train_step): odd widths get a zero column."""
        return cols + (cols & 1)

    def da_corrupt(self, x2d, zeros, ones, out=None):
        """x~ = zeros * x + ones (dlc_da_corrupt_f64): x2d [rows, K] fp64 and the masks of its size -> [rows, even_pitch(K)]
        (the pad column zero), into `out` when given."""
        rows, k = x2d.shape
        for name, t in (("x", x2d), ("zeros", zeros), ("ones", ones)):
            if t.dtype != torch.float64 or not t.is_contiguous() or t.device != self.device or t.numel() != rows * k:
                raise ValueError("da_corrupt: %s must be a contiguous float64 tensor of %d elements on %s" % (name, rows * k, self.device))
        if out is None:
            out = torch.empty((rows, self.even_pitch(k)), dtype=torch.float64, device=self.device)
        self._check_out("da_corrupt: out", out, (rows, self.even_pitch(k)), torch.float64)
        self._check(self.lib.dlc_da_corrupt_f64(self.ctx, _ptr(x2d), _ptr(zeros), _ptr(ones), rows, k, _ptr(out),
                                                 out.stride(0), self._stream()))
        return out

    def da_train_workspace(self, batch, patches, in_units, hidden_units):
        """A workspace tensor of dlc_da_train_step's size for this shape."""
        need = self.lib.dlc_da_train_workspace_bytes(batch, patches, in_units, hidden_units)
        if need == 0:
            raise ValueError("da_train_step: batch must be >= 2 frames")
        return torch.empty(int(need), dtype=torch.uint8, device=self.device)

    def da_train_step(self, x2d, xt, batch, patches, w, b_enc, b_dec, sparse_level, sparse_penalty, consecutive_penalty,
                      learning_rate, loss_out=None, ws=None):
        """One in-place SGD step of a DA (dlc_da_train_step): x2d [batch*patches, K] the clean batch, xt its corruption
        [batch*patches, even_pitch(K)] (da_corrupt), w [K, N], b_enc [N], b_dec [K]; loss_out: 4 doubles; ws: the caller's
        own workspace (da_train_workspace) instead of the engine's."""
        k, n = w.shape
        rows = batch * patches
        for name, t, shape in (("x", x2d, (rows, k)), ("x_tilde", xt, (rows, self.even_pitch(k))), ("W", w, (k, n)),
                               ("b_enc", b_enc, (n,)), ("b_dec", b_dec, (k,))):
            self._check_out("da_train_step: " + name, t, shape, torch.float64)
        if loss_out is not None:
            self._check_out("da_train_step: loss_out", loss_out, (4,), torch.float64)
        need = self.lib.dlc_da_train_workspace_bytes(batch, patches, k, n)
        if need == 0:
            raise ValueError("da_train_step: batch must be >= 2 frames")
        if ws is None:
            ws = self.workspace("da_train", need)
        else:
            self._check_ws(ws)
        self._check(self.lib.dlc_da_train_step(self.ctx, batch, patches, k, n, _ptr(x2d), _ptr(xt), _ptr(w), _ptr(b_enc),
                                                _ptr(b_dec), float(sparse_level), float(sparse_penalty),
                                                float(consecutive_penalty), float(learning_rate), _ptr(loss_out),
                                                _ptr(ws), ws.numel(), self._stream()))

    # ---- SDAV patch front-end --------------------------------------------------------------
    def rgb_to_gray(self, rgb):
        rgb = rgb.contiguous()
        if rgb.dtype != torch.uint8 or rgb.shape[-1] != 3:
            raise ValueError("rgb_to_gray: uint8 [..., 3] expected")
        gray = torch.empty(rgb.shape[:-1], dtype=torch.uint8, device=self.device)
        self._check(self.lib.dlc_rgb_to_gray_u8(self.ctx, _ptr(rgb), gray.numel(), _ptr(gray), self._stream()))
        return gray

    def harris_keypoints(self, gray, n):
        """gray uint8 [F,H,W] -> (points int32 [F,n,2] as cv2-style (x = column, y = row), responses int64
        [F,n], counts int32 [F]); (-1,-1) / 0 past a frame's count.  The build's stand-in for SURF."""
        gray = gray.contiguous()
        if gray.dtype != torch.uint8 or gray.dim() != 3:
            raise ValueError("harris_keypoints: uint8 [F, H, W] expected")
        f, h, w = gray.shape
        need = self.lib.dlc_harris_keypoints_workspace_bytes(f, h, w)
        if need == 0 or n < 1:
            raise ValueError("harris_keypoints: needs n >= 1 and frames of at least 7x7 pixels")
        ws = self.workspace("harris", need)
        pts = torch.empty((f, n, 2), dtype=torch.int32, device=self.device)
        resp = torch.empty((f, n), dtype=torch.int64, device=self.device)
        cnt = torch.empty((f,), dtype=torch.int32, device=self.device)
        self._check(self.lib.dlc_harris_keypoints_u8(self.ctx, _ptr(gray), f, h, w, n, _ptr(pts), _ptr(resp), _ptr(cnt),
                                                      _ptr(ws), ws.numel(), self._stream()))
        return pts, resp, cnt

    def extract_patches(self, gray, key_points, patch_size, dtype=torch.float64):
        """gray uint8 [F,H,W], key_points int32 [F,P,2] -> [F,P,patch_size^2] pixel/255."""
        gray, key_points = gray.contiguous(), key_points.contiguous()
        f, h, w = gray.shape
        p = key_points.shape[1]
        out = torch.empty((f, p, patch_size * patch_size), dtype=dtype, device=self.device)
        self._check(self.lib.dlc_extract_patches(self.ctx, _ptr(gray), f, h, w, _ptr(key_points), p, patch_size,
                                                  _TORCH_TO_DLC[dtype], _ptr(out), self._stream()))
        return out

    # ---- CnnVtl pieces ---------------------------------------------------------------
    def im2col(self, x, kh, kw, stride, pad_top, pad_left, oh, ow):
        n, h, w, c = x.shape
        cols = torch.empty((n * oh * ow, kh * kw * c), dtype=torch.float64, device=self.device)
        self._check(self.lib.dlc_im2col_nhwc_f64(self.ctx, _ptr(x), n, h, w, c, kh, kw, stride, pad_top, pad_left, oh,
                                                  ow, _ptr(cols), self._stream()))
        return cols

    def conv2d(self, x, kernel2d, bias, kh, kw, stride, pad_top, pad_left, oh, ow, act, frame_keys=None):
        """NHWC fp64 convolution + bias + activation as an implicit GEMM (no im2col matrix).
        kernel2d is the HWIO kernel reshaped [kh*kw*c, cout].  frame_keys ([n, 2] int64 from
        frame_minmax_keys()): the minimum / maximum of every frame's outputs is folded into it on the way."""
        x = x.contiguous()
        n, h, w, c = x.shape
        cout = kernel2d.shape[1]
        out = torch.empty((n, oh, ow, cout), dtype=torch.float64, device=self.device)
        if frame_keys is None:
            self._check(self.lib.dlc_conv2d_nhwc_f64(self.ctx, _ptr(x), n, h, w, c, _ptr(kernel2d), _ptr(bias), kh, kw, cout,
                                                      stride, pad_top, pad_left, oh, ow, act, _ptr(out), self._stream()))
        else:
            self._check_keys(frame_keys, n)
            self._check(self.lib.dlc_conv2d_nhwc_f64_stats(self.ctx, _ptr(x), n, h, w, c, _ptr(kernel2d), _ptr(bias), kh, kw,
                                                            cout, stride, pad_top, pad_left, oh, ow, act, _ptr(out),
                                                            _ptr(frame_keys), self._stream()))
        return out

    def _check_keys(self, keys, n):
        if not isinstance(keys, torch.Tensor) or keys.dtype != torch.int64 or tuple(keys.shape) != (n, 2) or \
                not keys.is_contiguous() or keys.device != self.device:
            raise ValueError("frame keys must be a contiguous [%d, 2] int64 tensor on %s" % (n, self.device))

    def frame_minmax_keys(self, n):
        """[n, 2] ordered keys, initialised to 'nothing seen', for conv2d(frame_keys=) / quant_gather()."""
        keys = torch.empty((n, 2), dtype=torch.int64, device=self.device)
        self._check(self.lib.dlc_cnnvtl_frame_minmax_init(self.ctx, _ptr(keys), n, self._stream()))
        return keys

    def quant_gather(self, segments, columns, frame_keys):
        """minmax_quant_gather with the per-frame range taken from frame_keys (folded by the convolutions)."""
        n = segments[0].shape[0]
        self._check_keys(frame_keys, n)
        segs = [s.reshape(n, -1).contiguous() for s in segments]
        ptrs = (C.c_void_p * len(segs))(*[s.data_ptr() for s in segs])
        sizes = (C.c_int64 * len(segs))(*[s.shape[1] for s in segs])
        minmax = torch.empty((n, 2), dtype=torch.float64, device=self.device)
        out = torch.empty((n, columns.numel()), dtype=torch.int8, device=self.device)
        self._check(self.lib.dlc_quant_gather_i8(self.ctx, ptrs, sizes, len(segs), n, _ptr(columns), columns.numel(),
                                                  _ptr(frame_keys), _ptr(minmax), _ptr(out), self._stream()))
        return out

    def space_to_depth(self, x, s):
        """NHWC fp64 [n,h,w,c] -> [n, h/s, w/s, s*s*c] (block s; dlc_space_to_depth_nhwc_f64)."""
        x = x.contiguous()
        n, h, w, c = x.shape
        y = torch.empty((n, h // s, w // s, s * s * c), dtype=torch.float64, device=self.device)
        self._check(self.lib.dlc_space_to_depth_nhwc_f64(self.ctx, _ptr(x), n, h, w, c, s, _ptr(y), self._stream()))
        return y

    def maxpool3x3s2(self, x):
        n, h, w, c = x.shape
        y = torch.empty((n, (h - 3) // 2 + 1, (w - 3) // 2 + 1, c), dtype=torch.float64, device=self.device)
        self._check(self.lib.dlc_maxpool3x3s2_nhwc_f64(self.ctx, _ptr(x), n, h, w, c, _ptr(y), self._stream()))
        return y

    def minmax_quant_gather(self, segments, columns):
        n = segments[0].shape[0]
        segs = [s.reshape(n, -1).contiguous() for s in segments]
        ptrs = (C.c_void_p * len(segs))(*[s.data_ptr() for s in segs])
        sizes = (C.c_int64 * len(segs))(*[s.shape[1] for s in segs])
        minmax = torch.empty((n, 2), dtype=torch.float64, device=self.device)
        out = torch.empty((n, columns.numel()), dtype=torch.int8, device=self.device)
        self._check(self.lib.dlc_minmax_quant_gather_i8(self.ctx, ptrs, sizes, len(segs), n, _ptr(columns),
                                                         columns.numel(), _ptr(minmax), _ptr(out), self._stream()))
        return out

    # ---- reference-semantics match ---------------------------------------------------
    def distinctive_score(self, dataset, mu, sigma, with_range=False):
        """Distinctive score [H] of a dataset [..., H]; with_range=True: (score, range) where range (3 + 2 H int64 words on
        the device) is what the pass learned about the columns' extremes -- pass it to sdav_similarity_matrix(range=) for
        the SAME tensor and that call does not read the descriptors again to find them."""
        d2 = dataset.reshape(-1, dataset.shape[-1]).contiguous()
        score = torch.empty(d2.shape[1], dtype=torch.float64, device=self.device)
        rng = torch.empty(self.lib.dlc_sdav_range_words(d2.shape[1]), dtype=torch.int64, device=self.device) if with_range else None
        self._check(self.lib.dlc_sdav_distinctive_score(self.ctx, _ptr(d2), d2.shape[0], d2.shape[1], float(mu),
                                                         float(sigma), _ptr(score), _ptr(rng), self._stream()))
        return (score, rng) if with_range else score

    def sdav_similarity_matrix(self, desc, score, a=10.0, b=-10.0, want_int64=True, force_f64=False, no_host_sync=False,
                               chunk_bytes=0, stats=None, direct_pairs=None, range=None):
        """All-vs-all SDAV similarity of desc [N,P,H] (fp64) -> (out fp64 [N,N], out int64 [N,N] or None).
        force_f64: the fp64 Gram form instead of the int8 arg-min filter (same matrix); no_host_sync: never read the
        flag word back (graph-capturable; a dataset with NaN / inf then yields NaN and stats[1] = 1, and no sample decides
        whether the filter is worth running); chunk_bytes: bound of one product block (0 = 8 GiB); stats: int64 [2] device
        tensor ([0] arg-mins evaluated directly, [1] why the fp64 form ran instead: bit 0 NaN / inf, bit 1 the sample's
        verdict), direct_pairs: uint8 [N,N] device tensor marking the frame pairs with a directly evaluated arg-min
        (include/dlc.h)."""
        desc = desc.contiguous()
        n, p, h = desc.shape
        flags = (L.DLC_SIM_FORCE_F64 if force_f64 else 0) | (L.DLC_SIM_NO_HOST_SYNC if no_host_sync else 0)
        if stats is not None:
            self._check_out("stats", stats, (2,), torch.int64)
        if direct_pairs is not None:
            self._check_out("direct_pairs", direct_pairs, (n, n), torch.uint8)
        if range is not None:
            self._check_out("range", range, (self.lib.dlc_sdav_range_words(h),), torch.int64)
        out = torch.empty((n, n), dtype=torch.float64, device=self.device)
        out_i = torch.empty((n, n), dtype=torch.int64, device=self.device) if want_int64 else None
        need = self.lib.dlc_sdav_similarity_workspace_bytes(n, p, h, flags, int(chunk_bytes))
        ws = self.workspace("sim", need)
        self._check(self.lib.dlc_sdav_similarity_matrix(self.ctx, _ptr(desc), n, p, h, _ptr(score), float(a), float(b),
                                                         _ptr(out), _ptr(out_i), flags, int(chunk_bytes), _ptr(range),
                                                         _ptr(stats), _ptr(direct_pairs), _ptr(ws), ws.numel(), self._stream()))
        return out, out_i

    # ---- streaming similarity: one new frame against the resident older ones (dlc_sdav_stream_*) ----
    def sdav_stream_state(self, capacity, p, h, lo=0.0, hi=1.0, col_centre=None):
        """State of a similarity stream whose values satisfy lo <= x - col_centre[k] <= hi (col_centre: [h] fp64 on the
        device, or None for zeros)."""
        need = self.lib.dlc_sdav_stream_state_bytes(int(capacity), int(p), int(h))
        if need == 0:
            raise ValueError("streaming similarity: P <= 32 patches and H <= 32768 (got %d, %d)" % (p, h))
        if col_centre is not None:
            self._check_out("col_centre", col_centre, (int(h),), torch.float64)
        state = torch.zeros(int(need), dtype=torch.uint8, device=self.device)
        self._check(self.lib.dlc_sdav_stream_init(self.ctx, _ptr(state), state.numel(), int(capacity), int(p), int(h), float(lo),
                                                   float(hi), _ptr(col_centre), self._stream()))
        return state

    def sdav_stream_append(self, state, desc, n_old, n_total, score):
        cap, p, h = desc.shape
        self._check(self.lib.dlc_sdav_stream_append(self.ctx, _ptr(state), state.numel(), cap, p, h, _ptr(desc), int(n_old),
                                                     int(n_total), _ptr(score), self._stream()))

    def sdav_stream_query(self, state, desc, f, score, a=10.0, b=-10.0, out=None, stats=None):
        cap, p, h = desc.shape
        if out is None:
            out = torch.empty((max(int(f), 0),), dtype=torch.float64, device=self.device)
        if stats is not None:
            self._check_out("stats", stats, (2,), torch.int64)
        self._check(self.lib.dlc_sdav_stream_query(self.ctx, _ptr(state), state.numel(), cap, p, h, _ptr(desc), int(f), _ptr(score),
                                                    float(a), float(b), _ptr(out), _ptr(stats), self._stream()))
        return out

    def sdav_stream_query_batch(self, state, desc, f_first, n_queries, score, a=10.0, b=-10.0, out=None, stats=None):
        """Rows of the resident frames f_first .. f_first + n_queries - 1 against the frames older than each, in one pair of
        launches: out [n_queries, ld >= f_first + n_queries - 1] fp64, row q valid in its first f_first + q entries."""
        cap, p, h = desc.shape
        ld = max(1, int(f_first) + int(n_queries) - 1)
        if out is None:
            out = torch.empty((int(n_queries), ld), dtype=torch.float64, device=self.device)
        else:
            self._check_out("out", out, (int(n_queries), out.shape[1]), torch.float64)
        if stats is not None:
            self._check_out("stats", stats, (2,), torch.int64)
        need = self.lib.dlc_sdav_stream_query_batch_workspace_bytes(cap, p, int(n_queries))
        ws = self.workspace("stream_batch", need)
        self._check(self.lib.dlc_sdav_stream_query_batch(self.ctx, _ptr(state), state.numel(), cap, p, h, _ptr(desc), int(f_first),
                                                          int(n_queries), _ptr(score), float(a), float(b), _ptr(out), out.shape[1],
                                                          _ptr(stats), _ptr(ws), ws.numel(), self._stream()))
        return out

    def sdav_stream_query_batch_staged(self, state, desc, f_first, n_queries, score, stage, out, ws, a=10.0, b=-10.0, stats=None,
                                       stream=None):
        """One half of the strip form of sdav_stream_query_batch (include/dlc.h): stage 1 = the product kernel into the
        caller's workspace ws, stage 2 = resolution + scores into out [n_queries, ld] -- for callers that run a batch's
        stage 2 beside the next batch's stage 1 (loop_closure.SdavLoopClosureDetector.submit).  stream: a torch stream
        (default: the current one)."""
        cap, p, h = desc.shape
        self._check_out("out", out, (int(n_queries), out.shape[1]), torch.float64)
        if stats is not None:
            self._check_out("stats", stats, (2,), torch.int64)
        st = C.c_void_p(stream.cuda_stream) if stream is not None else self._stream()
        self._check(self.lib.dlc_sdav_stream_query_batch_staged(self.ctx, _ptr(state), state.numel(), cap, p, h, _ptr(desc),
                                                                 int(f_first), int(n_queries), _ptr(score), float(a), float(b),
                                                                 _ptr(out), out.shape[1], _ptr(stats), _ptr(ws), ws.numel(),
                                                                 int(stage), st))
        return out

    def topk_rows_f64(self, scores, limit0, limit_step, k, poison=None):
        """(scores [rows, k] fp64, idx [rows, k] int64) of the k best of the first limit0 + r * limit_step entries of row r of
        scores [rows, ld] (fp64): score descending, ties -> the lower index, NaN never; (-inf, -1) where fewer.
        poison: a device int64 [1] read by the kernel; non-zero -> every slot (NaN, -1)."""
        self._check_out("scores", scores, tuple(scores.shape), torch.float64)
        if poison is not None:
            self._check_out("poison", poison, (1,), torch.int64)
        rows, ld = scores.shape
        o_s = torch.empty((rows, k), dtype=torch.float64, device=self.device)
        o_i = torch.empty((rows, k), dtype=torch.int64, device=self.device)
        self._check(self.lib.dlc_topk_rows_f64(self.ctx, _ptr(scores), rows, ld, int(limit0), int(limit_step), int(k), _ptr(o_s),
                                                _ptr(o_i), _ptr(poison), self._stream()))
        return o_s, o_i

    def cnnvtl_distance_matrix(self, desc, d=None, out=None):
        """All-vs-all popcount(|a ^ b|) distances of int8 descriptors [N, D] -> int64 [N, N].  d: the descriptor length
        when desc's rows are padded (to a multiple of 4 bytes); out: a caller-kept [N, N] int64 tensor."""
        desc = desc.contiguous()
        n = desc.shape[0]
        if d is None:
            d = desc.shape[1]
            if d % 4:       # rows on 4-byte boundaries let the kernel load words (the bytes past d are masked there)
                padded = torch.zeros((n, (d + 15) // 16 * 16), dtype=torch.int8, device=self.device)
                padded[:, :d] = desc
                desc = padded
        if out is None:
            out = torch.empty((n, n), dtype=torch.int64, device=self.device)
        else:
            self._check_out("out", out, (n, n), torch.int64)
        self._check(self.lib.dlc_cnnvtl_distance_matrix(self.ctx, _ptr(desc), n, int(d), desc.stride(0), _ptr(out),
                                                         self._stream()))
        return out

    def _rows16(self, x, d):
        """x [n, >= d] int8 as rows the top-k kernel takes (16-byte aligned base and stride): x itself when it already is,
        else a zero-padded copy of its first d columns."""
        if x.stride(1) == 1 and x.stride(0) % 16 == 0 and x.data_ptr() % 16 == 0 and x.stride(0) >= d:
            return x
        padded = torch.zeros((x.shape[0], (d + 15) // 16 * 16), dtype=torch.int8, device=self.device)
        padded[:, :d] = x[:, :d]
        return padded

    def _int8_pair(self, who, q, db, d, dtype=torch.int8):
        """The checks of the distance calls' operands q [Q, >= d], db [N, >= d] (int8 -- or `dtype`, the other byte type
        -- on the device) -> d (None: the rows' one width)."""
        if not isinstance(q, torch.Tensor) or not isinstance(db, torch.Tensor) or q.dim() != 2 or db.dim() != 2 or \
                q.dtype != dtype or db.dtype != dtype:
            raise ValueError("%s: q and db must be 2-D %s" % (who, str(dtype).split(".")[-1]))
        if q.device != self.device or db.device != self.device:
            raise ValueError("%s: q and db must be on %s" % (who, self.device))
        if d is None:
            if q.shape[1] != db.shape[1]:
                raise ValueError("%s: q and db widths differ (%d, %d)" % (who, q.shape[1], db.shape[1]))
            d = q.shape[1]
        d = int(d)
        if d > q.shape[1] or d > db.shape[1]:
            raise ValueError("%s: d=%d exceeds the rows' width" % (who, d))
        return d

    def _rows_out(self, what, t, rows, n, dtype, kind, fill=None, wider=False):
        """The [rows, n] result of a call that writes each row's offered cells only: allocated (and filled with `fill`,
        "not offered", unless None) when t is None, else the caller-kept t, checked -- `what` and `kind` name it in the
        error ("cosine_score_rows: out", "a float64"); wider: t may have more than n columns."""
        if t is None:
            t = torch.empty((rows, n), dtype=dtype, device=self.device)
            if fill is not None:
                t.fill_(fill)
        elif not isinstance(t, torch.Tensor) or t.dim() != 2 or t.shape[0] != rows or \
                (t.shape[1] < n if wider else t.shape[1] != n) or t.dtype != dtype or t.device != self.device or \
                (t.shape[1] > 1 and t.stride(1) != 1) or (rows > 1 and t.stride(0) < n):
            raise ValueError("%s must be %s tensor of shape (%d, %s%d) on %s with unit column stride and rows at least %d "
                             "apart" % (what, kind, rows, ">= " if wider else "", n, self.device, n))
        return t

    @staticmethod
    def _ld_out(t, rows, width):
        """The pitch the library is told for a result _rows_out has passed: one row has none of its own."""
        return t.stride(0) if rows > 1 else width

    @staticmethod
    def _row_strided(t, rows, width):
        """A checked 2-D operand [rows, >= width] -> (t, ld): a view with unit column stride and rows at least `width`
        apart is taken as it is, anything else made contiguous."""
        if t.stride(1) != 1 or (rows > 1 and t.stride(0) < width):
            t = t.contiguous()
        return t, t.stride(0) if rows > 1 else max(width, t.stride(0))

    def _f64_vector(self, who, what, v, n):
        """An optional fp64 vector [n] on the device (a mean, a scale): None, or v made contiguous."""
        if v is None:
            return None
        if not isinstance(v, torch.Tensor) or v.dtype != torch.float64 or v.device != self.device or tuple(v.shape) != (n,):
            raise ValueError("%s: %s must be a float64 tensor [%d] on %s" % (who, what, n, self.device))
        return v.contiguous()

    @staticmethod
    def _split_plan(who, plan, rows, codes, max_rows):
        """The plan word of a call whose "split" plan takes at most max_rows rows -> its code (codes: word -> code)."""
        if plan not in codes:
            raise ValueError("%s: plan=%r is none of %s" % (who, plan, sorted(codes)))
        if plan == "split" and rows > max_rows:
            raise ValueError("%s: plan 'split' takes at most %d rows, not %d" % (who, max_rows, rows))
        return codes[plan]

    def cnnvtl_distance_topk(self, q, db, k, d=None, limit0=None, limit_step=0, out=None):
        """(dist [Q, k] int64, idx [Q, k] int64): the k rows of db [N, D] int8 nearest to each query row of q [Q, D] int8 by
        the cnn_vtl distance, distance ascending, ties -> the lower row; query r sees the first min(N, limit0 + r *
        limit_step) rows (limit0 None = N); (-1, -1) where it sees fewer than k.  d: the descriptor length when the rows are
        padded (the bytes past d are ignored); out: a caller-kept (dist, idx) pair."""
        d = self._int8_pair("cnnvtl_distance_topk", q, db, d)
        if not 1 <= k <= L.DLC_MAX_K:
            raise ValueError("cnnvtl_distance_topk: k=%d outside 1..%d" % (k, L.DLC_MAX_K))
        nq, n = q.shape[0], db.shape[0]
        if out is None:
            dist = torch.empty((nq, k), dtype=torch.int64, device=self.device)
            idx = torch.empty((nq, k), dtype=torch.int64, device=self.device)
        else:
            dist = self._check_out("out[0] (dist)", out[0], (nq, k), torch.int64)
            idx = self._check_out("out[1] (idx)", out[1], (nq, k), torch.int64)
        if nq == 0:
            return dist, idx
        if n == 0 or d == 0:
            dist.fill_(-1)
            idx.fill_(-1)
            return dist, idx
        q = self._rows16(q, d)
        db = self._rows16(db, d)
        need = self.lib.dlc_cnnvtl_distance_topk_workspace_bytes(nq, n, d, k)
        ws = self.workspace("distance_topk", need)
        self._check(self.lib.dlc_cnnvtl_distance_topk(self.ctx, _ptr(q), nq, q.stride(0), _ptr(db), n, db.stride(0), d,
                                                       *_limits(n, limit0, limit_step), int(k),
                                                       _ptr(dist), _ptr(idx), _ptr(ws), ws.numel(), self._stream()))
        return dist, idx

    def _byte_rows(self, who, dtype, fn, q, db, d, limit0, limit_step, out):
        """The plain row call `fn` (dlc_cnnvtl_distance_rows, dlc_sad_u8_rows, dlc_hamming_rows: one contract) behind the
        public method `who` on rows of the byte type `dtype`."""
        d = self._int8_pair(who, q, db, d, dtype=dtype)
        nq, n = q.shape[0], db.shape[0]
        out = self._rows_out(who + ": out", out, nq, n, torch.int64, "an int64", None if limit0 is None else -1)
        if nq == 0 or n == 0:
            return out
        if d == 0:                                               # empty descriptors: every distance is 0
            lim0, step = _limits(n, limit0, limit_step)
            lim = lim0 + step * torch.arange(nq, device=self.device)
            out.masked_fill_(torch.arange(n, device=self.device)[None, :] < lim[:, None], 0)
            return out
        q = self._rows16(q.view(torch.int8), d).view(dtype)
        db = self._rows16(db.view(torch.int8), d).view(dtype)
        self._check(fn(self.ctx, _ptr(q), nq, q.stride(0), _ptr(db), n, db.stride(0), d, *_limits(n, limit0, limit_step),
                       _ptr(out), self._ld_out(out, nq, n), self._stream()))
        self._wrote(out)
        return out

    def cnnvtl_distance_rows(self, q, db, d=None, limit0=None, limit_step=0, out=None):
        """int64 [Q, N]: the cnn_vtl distance of every query row of q [Q, D] int8 to the rows of db [N, D] int8
        (dlc_cnnvtl_distance_rows, include/dlc.h), exact.  Query r is written in its first clamp(limit0 + r * limit_step,
        0, N) cells (limit0 None = N: all of them); the other cells keep what `out` held, and hold -1 -- "not offered",
        as sequence_scores writes it -- when the engine allocates the result.  d: the descriptor length when the rows
        are padded (the bytes past d are ignored); out: a caller-kept int64 [Q, N] tensor, which may be a view whose rows
        lie further apart than N (its columns past N are left alone too)."""
        return self._byte_rows("cnnvtl_distance_rows", torch.int8, self.lib.dlc_cnnvtl_distance_rows, q, db, d, limit0,
                               limit_step, out)

    # ---- SeqSLAM front-end: patch-normalised thumbnails, SAD difference rows ------------------------------------------
    def seqslam_describe(self, gray, size, patch, strength, out=None):
        """uint8 [F, h * w]: SeqSLAM's descriptor of every frame of gray (uint8 [F, H, W] on the device) -- the frame
        area-resized to size = (h, w), then patch-normalised over patch x patch tiles to 128 + strength * z-score
        (dlc_seqslam_describe_u8, include/dlc.h), exact.  out: a caller-kept uint8 [F, >= h * w] tensor or row-strided view
        (a database's rows: the bytes past h * w of a row keep their value); the result is its first h * w columns."""
        if not isinstance(gray, torch.Tensor) or gray.dtype != torch.uint8 or gray.dim() != 3 or gray.device != self.device:
            raise ValueError("seqslam_describe: uint8 [F, H, W] on %s expected" % self.device)
        gray = gray.contiguous()
        h, w = (int(v) for v in size)
        f, hh, ww = gray.shape
        if h < 1 or w < 1:
            raise ValueError("seqslam_describe: size=%r must be positive" % (size,))
        out = self._rows_out("seqslam_describe: out", out, f, h * w, torch.uint8, "a uint8", wider=True)
        if f == 0:
            return out[:, :h * w]
        self._check(self.lib.dlc_seqslam_describe_u8(self.ctx, _ptr(gray), f, hh, ww, h, w, int(patch), int(strength),
                                                      _ptr(out), self._ld_out(out, f, h * w), self._stream()))
        self._wrote(out)
        return out[:, :h * w]

    def _rows16_u8(self, x, d):
        """_rows16 for uint8 rows."""
        return self._rows16(x.view(torch.int8), d).view(torch.uint8)

    def sad_rows(self, q, db, d=None, limit0=None, limit_step=0, out=None, shift=None, width=None, shift_out=None):
        """int64 [Q, N]: the sum of absolute differences of every query row of q [Q, D] uint8 to the rows of db [N, D]
        uint8 (dlc_sad_u8_rows, include/dlc.h), exact.  Query r is written in its first clamp(limit0 + r * limit_step,
        0, N) cells (limit0 None = N: all of them); the other cells keep what `out` held, and hold -1, "not offered",
        when the engine allocates the result.  d: the descriptor length when the rows are padded (the bytes past d are
        ignored); out: a caller-kept int64 [Q, N] tensor, which may be a view whose rows lie further apart than N (its
        columns past N are left alone too).
        shift = S (1 .. min(DLC_MAX_SHIFT, width - 1); None or 0: the plain rows) with width = w, the thumbnail's columns
        (d a multiple of it): the best of the lateral shifts -S .. S, rescaled to the plain SAD's scale
        (dlc_sad_u8_shift_rows, include/dlc.h), exact.  shift_out: True, or a caller-kept int8 [Q, N] tensor or
        row-strided view -- the call then returns (out, shift_out), the winning shift of every written cell (0 in the
        cells that were not offered when it is allocated here)."""
        if not shift:                                            # None or 0: today's path, call for call
            if shift_out is not None and shift_out is not False:
                raise ValueError("sad_rows: shift_out needs shift")
            return self._byte_rows("sad_rows", torch.uint8, self.lib.dlc_sad_u8_rows, q, db, d, limit0, limit_step, out)
        d = self._int8_pair("sad_rows", q, db, d, dtype=torch.uint8)
        if width is None:
            raise ValueError("sad_rows: shift needs width, the thumbnail's columns")
        shift, width = int(shift), int(width)
        if width < 1 or d < width or d % width != 0:
            raise ValueError("sad_rows: d=%d is not a multiple of width=%d" % (d, width))
        if not 0 <= shift <= min(L.DLC_MAX_SHIFT, width - 1):
            raise ValueError("sad_rows: shift=%d outside 0..min(%d, width - 1 = %d)" % (shift, L.DLC_MAX_SHIFT, width - 1))
        nq, n = q.shape[0], db.shape[0]
        out = self._rows_out("sad_rows: out", out, nq, n, torch.int64, "an int64", None if limit0 is None else -1)
        want_shift = shift_out is not None and shift_out is not False
        sh = None
        if want_shift:
            sh = self._rows_out("sad_rows: shift_out", None if shift_out is True else shift_out, nq, n, torch.int8, "an int8",
                                None if limit0 is None else 0)
        if nq > 0 and n > 0 and d > 0:
            q = self._rows16_u8(q, d)
            db = self._rows16_u8(db, d)
            self._check(self.lib.dlc_sad_u8_shift_rows(
                self.ctx, _ptr(q), nq, q.stride(0), _ptr(db), n, db.stride(0), d // width, width, shift,
                *_limits(n, limit0, limit_step), _ptr(out), self._ld_out(out, nq, n),
                None if sh is None else _ptr(sh), 0 if sh is None else self._ld_out(sh, nq, n), self._stream()))
            self._wrote(out)
            if sh is not None:
                self._wrote(sh)
        return (out, sh) if want_shift else out

    # ---- binary place descriptors: global LDB codes, Hamming rows ------------------------------------------------------
    @staticmethod
    def _ldb_levels(levels):
        """levels as the C int array of the LDB calls and the row's bytes (dlc_ldb_row_bytes: 0 refuses the list)."""
        try:
            arr = (C.c_int * len(levels))(*(int(g) for g in levels))
        except (TypeError, ValueError):
            raise ValueError("ldb: levels=%r must be a sequence of integers" % (levels,))
        return arr, len(arr)

    def ldb_row_bytes(self, levels):
        """Bytes of an LDB row for `levels`: 16 * ceil(bits / 128) (dlc_ldb_row_bytes); ValueError for a list that is not
        1 to 4 grid sizes, strictly ascending, each 2..8."""
        arr, n = self._ldb_levels(levels)
        nb = int(self.lib.dlc_ldb_row_bytes(arr, n))
        if nb == 0:
            raise ValueError("ldb: levels=%r must be 1 to 4 grid sizes, strictly ascending, each 2..8" % (tuple(levels),))
        return nb

    def ldb_describe(self, gray, size, levels, out=None):
        """uint8 [F, row_bytes]: the global LDB code of every frame of gray (uint8 [F, H, W] on the device) -- the frame
        area-resized to size = (h, w), then per grid size of `levels` three bits per pair of cells: sum, horizontal and
        vertical gradient compared (dlc_ldb_describe_u8, include/dlc.h), exact.  out: a caller-kept uint8
        [F, >= row_bytes] tensor or row-strided view (a database's rows: the bytes past row_bytes of a row keep their
        value); the result is its first row_bytes columns."""
        if not isinstance(gray, torch.Tensor) or gray.dtype != torch.uint8 or gray.dim() != 3 or gray.device != self.device:
            raise ValueError("ldb_describe: uint8 [F, H, W] on %s expected" % self.device)
        gray = gray.contiguous()
        h, w = (int(v) for v in size)
        f, hh, ww = gray.shape
        if h < 1 or w < 1:
            raise ValueError("ldb_describe: size=%r must be positive" % (size,))
        nb = self.ldb_row_bytes(levels)
        arr, n = self._ldb_levels(levels)
        out = self._rows_out("ldb_describe: out", out, f, nb, torch.uint8, "a uint8", wider=True)
        if f == 0:
            return out[:, :nb]
        self._check(self.lib.dlc_ldb_describe_u8(self.ctx, _ptr(gray), f, hh, ww, h, w, arr, n, _ptr(out),
                                                  self._ld_out(out, f, nb), self._stream()))
        self._wrote(out)
        return out[:, :nb]

    def hamming_rows(self, q, db, d=None, limit0=None, limit_step=0, out=None):
        """int64 [Q, N]: the Hamming distance of every query row of q [Q, D] uint8 to the rows of db [N, D] uint8, bytes
        as packed bits (dlc_hamming_rows, include/dlc.h), exact.  Query r is written in its first clamp(limit0 + r *
        limit_step, 0, N) cells (limit0 None = N: all of them); the other cells keep what `out` held, and hold -1, "not
        offered", when the engine allocates the result.  d: the descriptor's bytes when the rows are padded (the bytes
        past d are ignored); out: a caller-kept int64 [Q, N] tensor, which may be a view whose rows lie further apart than
        N (its columns past N are left alone too)."""
        return self._byte_rows("hamming_rows", torch.uint8, self.lib.dlc_hamming_rows, q, db, d, limit0, limit_step, out)

    # ---- sign-random-projection hashes: float rows -> int8 rows -> packed sign bits ------------------------------------
    _LSH_DTYPES = {torch.float64: L.DLC_F64, torch.float32: L.DLC_F32, torch.bfloat16: L.DLC_BF16}
    _LSH_PLANS = {"auto": L.DLC_LSH_PLAN_AUTO, "one_pass": L.DLC_LSH_PLAN_ONE_PASS, "split": L.DLC_LSH_PLAN_SPLIT}

    def lsh_quantize(self, x, mean=None, out=None):
        """int8 [rows, D]: every row of x [rows, D] (float64, float32 or bfloat16 on the device; a row-strided view is
        taken as it is) scaled to -127 .. 127 by its own largest magnitude, after `mean` (float64 [D]; None: nothing) is
        taken off -- q = rint((x - mean) * (127 / max |x - mean|)) in fp64, ties to even; a row that is all zero or holds
        a NaN or an infinity becomes zeros (dlc_lsh_quantize_i8, include/dlc.h).  A row's bytes depend on that row and
        the mean alone.  out: a caller-kept int8 [rows, >= D] tensor or row-strided view (the bytes past D of a row keep
        their value); the result is its first D columns.  Allocated here, the rows lie a multiple of 16 bytes apart, as
        lsh_hash takes them without a copy."""
        if not isinstance(x, torch.Tensor) or x.dim() != 2 or x.dtype not in self._LSH_DTYPES or x.device != self.device:
            raise ValueError("lsh_quantize: x must be a 2-D float64, float32 or bfloat16 tensor on %s" % self.device)
        rows, d = x.shape
        if rows < 1 or d < 1:
            raise ValueError("lsh_quantize: x is [%d, %d]: nothing to do" % (rows, d))
        if d > L.DLC_LSH_MAX_D or rows >= 1 << 31:
            raise ValueError("lsh_quantize: rows=%d, D=%d outside rows < 2^31, D <= %d" % (rows, d, L.DLC_LSH_MAX_D))
        x, ldx = self._row_strided(x, rows, d)
        mean = self._f64_vector("lsh_quantize", "mean", mean, d)
        if out is None:
            out = torch.empty((rows, (d + 15) // 16 * 16), dtype=torch.int8, device=self.device)
        else:
            out = self._rows_out("lsh_quantize: out", out, rows, d, torch.int8, "an int8", wider=True)
        self._check(self.lib.dlc_lsh_quantize_i8(self.ctx, self._LSH_DTYPES[x.dtype], _ptr(x), rows, d, ldx, _ptr(mean), _ptr(out),
                                                  self._ld_out(out, rows, d), self._stream()))
        self._wrote(out)
        return out[:, :d]

    def lsh_row_bytes(self, bits):
        """Bytes of a hash row of `bits` bits: 16 * ceil(bits / 128) (dlc_lsh_row_bytes); ValueError outside 1..8192."""
        nb = int(self.lib.dlc_lsh_row_bytes(int(bits))) if -1 << 31 <= int(bits) < 1 << 31 else 0
        if nb == 0:
            raise ValueError("lsh: bits=%r outside 1..%d" % (bits, L.DLC_LSH_MAX_BITS))
        return nb

    def lsh_hash(self, q, planes, bits=None, out=None, plan="auto"):
        """uint8 [rows, row_bytes]: bit t of row r is 1 iff the integer product of q[r] and planes[t] is positive (a tie is
        0), bit t & 7 of byte t >> 3; the bits past `bits` are 0 (dlc_lsh_hash_i8, include/dlc.h).  q [rows, D] and planes
        [>= bits, D] are int8 on the device, any values; bits None: every plane.  The sums are exact on the int8 matrix
        cores, so a row's code depends on that row and the planes alone -- not on its batch or the plan ("one_pass": a
        workgroup walks all of D; "split", <= 64 rows: pieces of D are spread over the chip; "auto" chooses).  out: a
        caller-kept uint8 [rows, >= row_bytes] tensor or row-strided view -- rows of a HammingKeyframeDatabase, say; the
        bytes past row_bytes of a row keep their value -- and the result is its first row_bytes columns."""
        d = self._int8_pair("lsh_hash", q, planes, None)
        rows, n = q.shape[0], planes.shape[0]
        bits = n if bits is None else int(bits)
        if rows < 1 or d < 1 or not 1 <= bits <= n:
            raise ValueError("lsh_hash: q [%d, %d], %d planes and bits=%d: nothing to do" % (rows, d, n, bits))
        if d > L.DLC_LSH_MAX_D or rows >= 1 << 31:
            raise ValueError("lsh_hash: rows=%d, D=%d outside rows < 2^31, D <= %d" % (rows, d, L.DLC_LSH_MAX_D))
        nb = self.lsh_row_bytes(bits)
        code = self._split_plan("lsh_hash", plan, rows, self._LSH_PLANS, L.DLC_LSH_SPLIT_MAX_ROWS)
        out = self._rows_out("lsh_hash: out", out, rows, nb, torch.uint8, "a uint8", wider=True)
        q = self._rows16(q, d)
        planes = self._rows16(planes, d)
        need = self.lib.dlc_lsh_hash_workspace_bytes(rows, d, bits, code)
        ws = self.workspace("lsh_hash", need) if need else None
        self._check(self.lib.dlc_lsh_hash_i8(self.ctx, _ptr(q), rows, d, q.stride(0), _ptr(planes), bits, planes.stride(0), _ptr(out),
                                              self._ld_out(out, rows, nb), code, _ptr(ws), ws.numel() if ws is not None else 0,
                                              self._stream()))
        self._wrote(out)
        return out[:, :nb]

    _SEQ_DTYPES = {torch.float64: L.DLC_F64, torch.float32: L.DLC_F32, torch.int64: L.DLC_I64}
    # the dtype of what a score-row call derives from its rows: int64 from int64 rows, else float64
    _OUT_DTYPES = {torch.float64: torch.float64, torch.float32: torch.float64, torch.int64: torch.int64}

    def _check_poison(self, who, poison, is_int):
        """A poison word that is given: a device int64 [1] -- which marks fp64 outputs, so int64 rows take none."""
        if is_int:
            raise ValueError("%s: the poison word marks fp64 outputs; int64 rows have none" % who)
        self._check_out("poison", poison, (1,), torch.int64)

    def _score_matrix(self, who, scores, n, nothing):
        """The checks of a score-matrix operand [rows, >= n] (fp64, fp32 or int64 on the device) -> (scores, rows, n, ld):
        a row-strided view is taken as it is, anything else made contiguous."""
        if not isinstance(scores, torch.Tensor) or scores.dim() != 2 or scores.dtype not in self._SEQ_DTYPES:
            raise ValueError("%s: scores must be a 2-D float64, float32 or int64 tensor" % who)
        if scores.device != self.device:
            raise ValueError("%s: scores must be on %s" % (who, self.device))
        rows = scores.shape[0]
        n = scores.shape[1] if n is None else int(n)
        if rows < 1 or n < 1 or n > scores.shape[1]:
            raise ValueError("%s: scores [%d, %d] with n=%d: nothing to %s" % (who, rows, scores.shape[1], n, nothing))
        scores, ld = self._row_strided(scores, rows, n)
        return scores, rows, n, ld

    def _offset_table(self, who, offsets, length):
        """The HOST table offsets [V, L] of a line search as the library takes it: (V, the int32 table's pointer)."""
        off = np.ascontiguousarray(np.asarray(offsets), dtype=np.int32)
        if off.ndim != 2 or off.shape[1] != int(length) or not np.array_equal(off, np.asarray(offsets)):
            raise ValueError("%s: offsets must be an integer table [n_slopes, L=%d]" % (who, int(length)))
        return off.shape[0], off.ctypes.data_as(C.POINTER(C.c_int32))      # (the pointer keeps the array alive)

    def sequence_topk(self, scores, length, offsets, k=None, row0=0, n=None, limit0=None, limit_step=0, lower_is_better=False,
                      dense=False, poison=None):
        """The sequence search of dlc_sequence_topk (include/dlc.h) over scores [rows, >= n] (fp64, fp32 or int64 on the
        device; a row-strided view is taken as it is): the sum of L frame scores along each line of the HOST table
        offsets [V, L] (int32) through every cell, the best valid line per cell, and per row r >= row0 the k best cells
        among its first clamp(limit0 + r * limit_step, 0, n) (limit0 None = n).  Returns (scores [rows - row0, k],
        idx int64, slope int32, dense): fp64 scores (int64 for int64 input); k None -> no lists (None three times);
        dense: the [rows - row0, n] cell scores as well (NaN / -1 where a cell is not offered), else None.
        poison: a device int64 [1] read by the kernels; non-zero -> every fp64 slot NaN, idx and slope -1."""
        mat = self._score_matrix("sequence_topk", scores, n, "search")
        table = self._offset_table("sequence_topk", offsets, length)
        return self._sequence_search("sequence_topk", self.lib.dlc_sequence_topk, self.lib.dlc_sequence_topk_workspace_bytes, mat,
                                     length, table[:1], table, k, row0, limit0, limit_step, lower_is_better, dense, poison)

    def sequence_elastic_topk(self, scores, length, steps, k=None, row0=0, n=None, limit0=None, limit_step=0,
                              lower_is_better=False, dense=False, poison=None):
        """The elastic sequence search of dlc_sequence_elastic_topk (include/dlc.h) over scores [rows, >= n] (fp64, fp32 or
        int64 on the device; a row-strided view is taken as it is): the best chain of L frame scores that ends in each
        cell and steps back steps = (d_min, d_max) key-frames per frame, 0 <= d_min <= d_max <= 8, and per row r >= row0
        the k best cells among its first clamp(limit0 + r * limit_step, 0, n) (limit0 None = n).  Returns (scores
        [rows - row0, k], idx int64, span int32, dense) as sequence_topk does, the span -- the key-frames the chosen chain
        covers -- in the slope's place.  poison: as in sequence_topk."""
        mat = self._score_matrix("sequence_elastic_topk", scores, n, "search")
        steps = check_steps(steps)
        if not 1 <= int(length) <= 64:
            raise ValueError("sequence_elastic_topk: L=%d outside 1..64" % int(length))
        return self._sequence_search("sequence_elastic_topk", self.lib.dlc_sequence_elastic_topk,
                                     self.lib.dlc_sequence_elastic_topk_workspace_bytes, mat, length, steps, steps, k, row0,
                                     limit0, limit_step, lower_is_better, dense, poison)

    def _sequence_search(self, who, call, size, mat, length, size_args, call_args, k, row0, limit0, limit_step, lower_is_better,
                         dense, poison):
        """What the two searches do alike once each has checked its table or steps: the other checks, the three lists,
        the workspace, the dense buffer and the call.  call, size: dlc_<who> and dlc_<who>_workspace_bytes; size_args:
        what `size` takes between L and k; call_args: what `call` takes between L and lower_is_better."""
        scores, rows, n, ld = mat
        if not 0 <= int(row0) < rows:
            raise ValueError("%s: row0=%d outside 0..%d" % (who, row0, rows - 1))
        if k is None and not dense:
            raise ValueError("%s: neither lists (k) nor the dense scores were asked for" % who)
        if k is not None and not 1 <= k <= L.DLC_MAX_K:
            raise ValueError("%s: k=%d outside 1..%d" % (who, k, L.DLC_MAX_K))
        if poison is not None:
            self._check_poison(who, poison, scores.dtype == torch.int64)
        out_dtype = self._OUT_DTYPES[scores.dtype]
        ro = rows - int(row0)
        o_s = o_i = o_v = seq = ws = None
        if k is not None:
            o_s = torch.empty((ro, k), dtype=out_dtype, device=self.device)
            o_i = torch.empty((ro, k), dtype=torch.int64, device=self.device)
            o_v = torch.empty((ro, k), dtype=torch.int32, device=self.device)
            need = size(rows, n, int(length), *size_args, int(k))
            if need == 0:
                raise ValueError("%s: L=%d, k=%d, n=%d outside the supported sizes" % (who, length, k, n))
            ws = self.workspace(who, need)
        if dense:
            seq = torch.empty((ro, n), dtype=out_dtype, device=self.device)
        self._check(call(
            self.ctx, self._SEQ_DTYPES[scores.dtype], _ptr(scores), rows, int(row0), n, ld, *_limits(n, limit0, limit_step),
            int(length), *call_args, int(bool(lower_is_better)), 1 if k is None else int(k), _ptr(o_s), _ptr(o_i), _ptr(o_v),
            _ptr(seq), n, _ptr(poison), _ptr(ws), ws.numel() if ws is not None else 0, self._stream()))
        return o_s, o_i, o_v, seq

    def _chain_args(self, who, scores, length, idx, row0, n, poison):
        """The checks the two chain calls share -> (scores, rows, n, ld, idx [rows - row0, k] int64 contiguous, k)."""
        scores, rows, n, ld = self._score_matrix(who, scores, n, "search")
        if not 1 <= int(length) <= 64:
            raise ValueError("%s: L=%d outside 1..64" % (who, int(length)))
        if not 0 <= int(row0) < rows:
            raise ValueError("%s: row0=%d outside 0..%d" % (who, row0, rows - 1))
        if not isinstance(idx, torch.Tensor) or idx.dim() != 2 or idx.dtype != torch.int64 or idx.device != self.device:
            raise ValueError("%s: idx must be an int64 tensor [rows - row0, k] on %s" % (who, self.device))
        if idx.shape[0] != rows - int(row0) or not 1 <= idx.shape[1] <= L.DLC_MAX_K:
            raise ValueError("%s: idx [%d, %d]: need [%d, 1..%d]" % (who, idx.shape[0], idx.shape[1], rows - int(row0), L.DLC_MAX_K))
        if poison is not None:
            self._check_poison(who, poison, scores.dtype == torch.int64)
        return scores, rows, n, ld, idx.contiguous(), idx.shape[1]

    def _sequence_chains(self, who, call, scores, length, call_args, idx, row0, n, limit0, limit_step, lower_is_better, cells, poison,
                         with_slope):
        """What the two chain calls do alike on top of _chain_args: the outputs and the call -> (chain, cells, slope).
        call: dlc_<who>; call_args: what it takes between L and lower_is_better; with_slope: it writes the winning slope
        as well."""
        scores, rows, n, ld, idx, k = self._chain_args(who, scores, length, idx, row0, n, poison)
        shape = (rows - int(row0), k, int(length))
        chain = torch.empty(shape, dtype=torch.int32, device=self.device)
        o_c = torch.empty(shape, dtype=self._OUT_DTYPES[scores.dtype], device=self.device) if cells else None
        slope = torch.empty(shape[:2], dtype=torch.int32, device=self.device) if with_slope else None
        self._check(call(
            self.ctx, self._SEQ_DTYPES[scores.dtype], _ptr(scores), rows, int(row0), n, ld, *_limits(n, limit0, limit_step),
            int(length), *call_args, int(bool(lower_is_better)), k, _ptr(idx), _ptr(chain), _ptr(o_c),
            *((_ptr(slope),) if with_slope else ()), _ptr(poison), self._stream()))
        return chain, o_c, slope

    def sequence_elastic_chains(self, scores, length, steps, idx, row0=0, n=None, limit0=None, limit_step=0,
                                lower_is_better=False, cells=False, poison=None):
        """The chains of dlc_sequence_elastic_chains (include/dlc.h): for every candidate end column idx[r - row0, i] (the
        idx of sequence_elastic_topk or of peak_topk_rows over its dense scores; -1: an empty slot) of the elastic
        search over scores with the same length, steps, row0, n, limits and order, the L matched columns, oldest frame
        first.  Returns (chain int32 [rows - row0, k, L], cells or None): cells=True adds the matrix cells along the chain
        (fp64, int64 for int64 scores), which summed oldest first give the candidate's score bit for bit.  A slot that
        is no chain (empty, past the row's limit, no valid chain, poisoned) holds -1 and NaN / -1."""
        return self._sequence_chains("sequence_elastic_chains", self.lib.dlc_sequence_elastic_chains, scores, length,
                                     check_steps(steps), idx, row0, n, limit0, limit_step, lower_is_better, cells, poison,
                                     False)[:2]

    def sequence_chains(self, scores, length, offsets, idx, row0=0, n=None, limit0=None, limit_step=0, lower_is_better=False,
                        cells=False, poison=None):
        """The chains of dlc_sequence_chains (include/dlc.h): for every candidate end column idx[r - row0, i] of the line
        search over scores with the same length, HOST table offsets [V, L], row0, n, limits and order, the L columns of
        its winning line, oldest frame first.  Returns (chain int32 [rows - row0, k, L], cells or None, slope int32
        [rows - row0, k]): the cells summed NEWEST first give the candidate's score bit for bit; slope is the row of the
        table that won.  A slot that is no chain holds -1 (cells NaN / -1, slope -1)."""
        table = self._offset_table("sequence_chains", offsets, length)
        return self._sequence_chains("sequence_chains", self.lib.dlc_sequence_chains, scores, length, table, idx, row0, n, limit0,
                                     limit_step, lower_is_better, cells, poison, True)

    def contrast_rows(self, scores, radius, n=None, limit0=None, limit_step=0, out=None):
        """SeqSLAM's local contrast normalisation of score rows (dlc_contrast_rows, include/dlc.h): fp64 [rows, n], cell
        (r, j) = (x - mean) / sample std over the cells j - radius .. j + radius of row r, clipped to the row's first
        clamp(limit0 + r * limit_step, 0, n) cells (limit0 None = n), 0.0 where the window holds fewer than two cells or is
        constant; each window summed on its own in fp64, left to right, so a row does not depend on its batch.  scores
        [rows, >= n]: fp64, fp32 or int64 on the device (a row-strided view is taken as it is).  Cells that are not
        offered keep what `out` held, and hold NaN -- "not offered", as sequence_scores writes it -- when the engine
        allocates the result.  out: a caller-kept fp64 tensor whose first n columns are written (out[:, :n] is returned);
        its rows may lie further apart than its width (a row-strided view is taken as it is)."""
        scores, rows, n, ld = self._score_matrix("contrast_rows", scores, n, "normalise")
        if not 1 <= int(radius) <= 32:
            raise ValueError("contrast_rows: radius=%d outside 1..32" % int(radius))
        out = self._rows_out("contrast_rows: out", out, rows, n, torch.float64, "a float64",
                             float("nan") if limit0 is not None or limit_step != 0 else None, wider=True)
        self._check(self.lib.dlc_contrast_rows(self.ctx, self._SEQ_DTYPES[scores.dtype], _ptr(scores), rows, n, ld,
                                                *_limits(n, limit0, limit_step), int(radius), _ptr(out),
                                                self._ld_out(out, rows, n), self._stream()))
        self._wrote(out)
        return out[:, :n]

    _FUSE_NORMS = {"none": L.DLC_FUSE_NONE, "zscore": L.DLC_FUSE_ZSCORE, "minmax": L.DLC_FUSE_MINMAX}
    _FUSE_PLANS = {None: L.DLC_FUSE_PLAN_AUTO, "auto": L.DLC_FUSE_PLAN_AUTO, "row": L.DLC_FUSE_PLAN_ROW,
                   "slab": L.DLC_FUSE_PLAN_SLAB}

    def fuse_rows(self, sources, weights=None, lower_is_better=False, norm="zscore", n=None, limit0=None, limit_step=0,
                  out=None, plan=None):
        """Several score rows of the same frames against the same key-frames fused into one (dlc_fuse_rows,
        include/dlc.h): fp64 [rows, n], higher is better, cell (r, j) = the sum over the sources, in their order, of
        weights[i] * the source's cell normalised within ITS row's first clamp(limit0 + r * limit_step, 0, n) cells
        (limit0 None = n) -- norm "zscore": (x - mean) / sample std, "minmax": (x - min) / (max - min), "none": x -- with
        the sign turned for a source that is lower_is_better (a bool, or one per source).  Every row sum is the TREE of
        dlc.h, so a row does not depend on its batch or on the plan.  sources: 1..8 matrices [rows, >= n], each fp64, fp32
        or int64 on the device (a row-strided view is taken as it is); weights: None (all 1) or one finite number per
        source.  Cells that are not offered keep what `out` held, and hold NaN when the engine allocates the result.
        out: as contrast_rows takes it.  plan: None / "auto", "row" or "slab" (dlc.h)."""
        sources = list(sources)
        if not 1 <= len(sources) <= L.DLC_MAX_FUSE:
            raise ValueError("fuse_rows: %d sources outside 1..%d" % (len(sources), L.DLC_MAX_FUSE))
        m = len(sources)
        if norm not in self._FUSE_NORMS:
            raise ValueError("fuse_rows: norm=%r is none of %s" % (norm, sorted(self._FUSE_NORMS)))
        if plan not in self._FUSE_PLANS:
            raise ValueError("fuse_rows: plan=%r is none of auto, row, slab" % (plan,))
        w = np.ones(m, dtype=np.float64) if weights is None else np.asarray(weights, dtype=np.float64).reshape(-1)
        if w.shape[0] != m or not np.isfinite(w).all():
            raise ValueError("fuse_rows: weights must be %d finite numbers" % m)
        lib = np.asarray(lower_is_better, dtype=bool).reshape(-1)
        if lib.shape[0] == 1:
            lib = np.repeat(lib, m)
        if lib.shape[0] != m:
            raise ValueError("fuse_rows: lower_is_better must be a bool or one per source (%d)" % m)
        mats, lds = [], []
        for i, s in enumerate(sources):
            s, rows_i, n_i, ld = self._score_matrix("fuse_rows: source %d" % i, s, n, "fuse")
            if i and (rows_i, n_i) != (rows, n):
                raise ValueError("fuse_rows: source %d is [%d, %d], source 0 [%d, %d]" % (i, rows_i, n_i, rows, n))
            rows, n = rows_i, n_i
            mats.append(s)
            lds.append(ld)
        out = self._rows_out("fuse_rows: out", out, rows, n, torch.float64, "a float64",
                             float("nan") if limit0 is not None or limit_step != 0 else None, wider=True)
        ws, need = None, 0
        if self._FUSE_PLANS[plan] != L.DLC_FUSE_PLAN_ROW:
            need = self.lib.dlc_fuse_rows_workspace_bytes(rows, n, m)
            if need == 0:
                raise ValueError("fuse_rows: rows=%d, n=%d outside the supported sizes" % (rows, n))
            ws = self.workspace("fuse_rows", need)
        self._check(self.lib.dlc_fuse_rows(
            self.ctx, m, (C.c_int * m)(*[self._SEQ_DTYPES[s.dtype] for s in mats]),
            (C.c_void_p * m)(*[s.data_ptr() for s in mats]), (C.c_int64 * m)(*lds), (C.c_double * m)(*w.tolist()),
            (C.c_int * m)(*[int(v) for v in lib]), rows, n, *_limits(n, limit0, limit_step),
            self._FUSE_NORMS[norm], self._FUSE_PLANS[plan], _ptr(out), self._ld_out(out, rows, n), _ptr(ws),
            ws.numel() if ws is not None else 0, self._stream()))
        self._wrote(out)
        return out[:, :n]

    _VLAD_NORMS = {"none": L.DLC_VLAD_NORM_NONE, "intra": L.DLC_VLAD_NORM_INTRA}

    def _f64_rows(self, who, what, t, width=None):
        """The checks of an fp64 operand [rows, H] on the device -> (t, rows, H, ld): a row-strided view is taken as it
        is (its padding columns are never read), anything else made contiguous."""
        if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.dtype != torch.float64 or t.device != self.device:
            raise ValueError("%s: %s must be a 2-D float64 tensor on %s" % (who, what, self.device))
        rows, h = t.shape
        if rows < 1 or h < 1:
            raise ValueError("%s: %s is [%d, %d]: nothing to do" % (who, what, rows, h))
        if width is not None and h != width:
            raise ValueError("%s: %s is %d wide, the rows are %d" % (who, what, h, width))
        t, ld = self._row_strided(t, rows, h)
        return t, rows, h, ld

    def _codebook(self, who, centroids, width):
        c, k, _, ldc = self._f64_rows(who, "the codebook", centroids, width)
        if k > L.DLC_VLAD_MAX_WORDS or k * width >= 1 << 31:
            raise ValueError("%s: a codebook of %d words x %d outside 1..%d words, K * H < 2^31" % (who, k, width,
                                                                                                  L.DLC_VLAD_MAX_WORDS))
        return c, k, ldc

    def vlad_assign(self, x, centroids, with_dist=False):
        """a int32 [rows]: the nearest word of every row of x [rows, H] (fp64 on the device) in the codebook [K, H] by the
        squared distance DIST of include/dlc.h (dlc_vlad_assign) -- the lowest index among equals, -1 for a row whose
        distances are all NaN.  with_dist: (a, the distances fp64 [rows])."""
        x, rows, h, ldx = self._f64_rows("vlad_assign", "x", x)
        c, k, ldc = self._codebook("vlad_assign", centroids, h)
        a = torch.empty(rows, dtype=torch.int32, device=self.device)
        d = torch.empty(rows, dtype=torch.float64, device=self.device) if with_dist else None
        self._check(self.lib.dlc_vlad_assign(self.ctx, _ptr(x), rows, h, ldx, _ptr(c), k, ldc, _ptr(a), _ptr(d), self._stream()))
        return (a, d) if with_dist else a

    def vlad_encode(self, x, centroids, patches=30, norm="intra", out=None, with_assign=False):
        """VLAD descriptors fp64 [frames, K * H] of x [frames * patches, H] (fp64 on the device; frame f owns rows
        f * patches ..) against the codebook [K, H] (dlc_vlad_encode, include/dlc.h): per word the sum of the residuals
        x - c_k of the frame's patches assigned to it, in patch order; norm "intra": every word's block divided by its
        L2 norm, "none": as summed.  The global L2 normalisation is the database's (KeyframeDatabase / normalize).  A
        frame's row does not depend on its batch.  out: a float64 tensor [frames, >= K * H] with unit column stride to
        write into (columns past K * H keep their bits).  with_assign: (out, the assignments int32 [frames * patches])."""
        if norm not in self._VLAD_NORMS:
            raise ValueError("vlad_encode: norm=%r is none of %s" % (norm, sorted(self._VLAD_NORMS)))
        patches = int(patches)
        if not 1 <= patches <= L.DLC_VLAD_MAX_PATCHES:
            raise ValueError("vlad_encode: patches=%d outside 1..%d" % (patches, L.DLC_VLAD_MAX_PATCHES))
        x, rows, h, ldx = self._f64_rows("vlad_encode", "x", x)
        if rows % patches:
            raise ValueError("vlad_encode: %d rows are no whole number of frames of %d patches" % (rows, patches))
        frames = rows // patches
        c, k, ldc = self._codebook("vlad_encode", centroids, h)
        out = self._rows_out("vlad_encode: out", out, frames, k * h, torch.float64, "a float64", wider=True)
        a = torch.empty(rows, dtype=torch.int32, device=self.device) if with_assign else None
        need = self.lib.dlc_vlad_encode_workspace_bytes(frames, patches, h, k)
        if need == 0:
            raise ValueError("vlad_encode: frames=%d, H=%d, K=%d outside the supported sizes" % (frames, h, k))
        ws = self.workspace("vlad_encode", need)
        self._check(self.lib.dlc_vlad_encode(self.ctx, _ptr(x), frames, patches, h, ldx, _ptr(c), k, ldc, self._VLAD_NORMS[norm],
                                             _ptr(out), self._ld_out(out, frames, k * h), _ptr(a), _ptr(ws), ws.numel(), self._stream()))
        self._wrote(out)
        return (out[:, :k * h], a) if with_assign else out[:, :k * h]

    def kmeans_step(self, x, centroids, prev_assign=None):
        """One Lloyd step of dlc_kmeans_step (include/dlc.h) over x [rows, H] (fp64 on the device) from the codebook
        [K, H]: (new codebook fp64 [K, H], assignments int32 [rows], counts int64 [K], inertia fp64 [1], changed int64
        [1]) -- all device tensors, nothing is read back.  Member sums run in row order within blocks of 1024 rows and by
        a fixed tree over the blocks, so the step is a function of its operands' bits; an empty word keeps its centre.
        changed counts the rows whose assignment differs from prev_assign (int32 [rows]; None: every row)."""
        x, rows, h, ldx = self._f64_rows("kmeans_step", "x", x)
        c, k, ldc = self._codebook("kmeans_step", centroids, h)
        if prev_assign is not None:
            self._check_out("kmeans_step: prev_assign", prev_assign, (rows,), torch.int32)
        c_out = torch.empty((k, h), dtype=torch.float64, device=self.device)
        a = torch.empty(rows, dtype=torch.int32, device=self.device)
        counts = torch.empty(k, dtype=torch.int64, device=self.device)
        inertia = torch.empty(1, dtype=torch.float64, device=self.device)
        changed = torch.empty(1, dtype=torch.int64, device=self.device)
        need = self.lib.dlc_kmeans_step_workspace_bytes(rows, h, k)
        if need == 0:
            raise ValueError("kmeans_step: rows=%d, H=%d, K=%d outside the supported sizes" % (rows, h, k))
        ws = self.workspace("kmeans_step", need)
        self._check(self.lib.dlc_kmeans_step(self.ctx, _ptr(x), rows, h, ldx, _ptr(c), k, ldc, _ptr(c_out), h, _ptr(prev_assign),
                                             _ptr(a), _ptr(counts), _ptr(inertia), _ptr(changed), _ptr(ws), ws.numel(),
                                             self._stream()))
        return c_out, a, counts, inertia, changed

    _PCA_PLANS = {"auto": L.DLC_PCA_PLAN_AUTO, "one_pass": L.DLC_PCA_PLAN_ONE_PASS, "split": L.DLC_PCA_PLAN_SPLIT}

    def pca_project(self, x, basis, mean=None, scale=None, out=None, plan="auto"):
        """((x - mean) . basis) * scale, fp64 [rows, M], of x [rows, D] (fp64 on the device) against the basis [D, M]
        (fp64 or fp32, component c in column c), mean fp64 [D] and scale fp64 [M] (either None: left out) --
        dlc_pca_project, include/dlc.h: serial chains over chunks of 1024 columns of x, the chunks added in order, so a
        row's bits depend on the row and the model alone, not on its batch or the plan.  plan "one_pass": a workgroup
        walks all of D; "split" (<= 64 rows): the chunks are spread over the chip; "auto" chooses.  out: a float64
        tensor [rows, >= M] with unit column stride to write into (columns past M keep their bits)."""
        x, rows, d, ldx = self._f64_rows("pca_project", "x", x)
        if not isinstance(basis, torch.Tensor) or basis.dim() != 2 or basis.dtype not in (torch.float64, torch.float32) or \
                basis.device != self.device or basis.shape[0] != d or basis.shape[1] < 1:
            raise ValueError("pca_project: the basis must be a float64 or float32 tensor [%d, M] on %s" % (d, self.device))
        m = basis.shape[1]
        if m > L.DLC_PCA_MAX_COMPONENTS:
            raise ValueError("pca_project: %d components outside 1..%d" % (m, L.DLC_PCA_MAX_COMPONENTS))
        basis, ldb = self._row_strided(basis, d, m)
        mean = self._f64_vector("pca_project", "mean", mean, d)
        scale = self._f64_vector("pca_project", "scale", scale, m)
        out = self._rows_out("pca_project: out", out, rows, m, torch.float64, "a float64", wider=True)
        code = self._split_plan("pca_project", plan, rows, self._PCA_PLANS, L.DLC_PCA_SPLIT_MAX_ROWS)
        if rows >= 1 << 31 or d >= 1 << 31:
            raise ValueError("pca_project: rows=%d, D=%d outside the supported sizes" % (rows, d))
        need = self.lib.dlc_pca_project_workspace_bytes(rows, d, m, code)
        ws = self.workspace("pca_project", need) if need else None
        self._check(self.lib.dlc_pca_project(
            self.ctx, _ptr(x), rows, d, ldx, _ptr(mean), L.DLC_F64 if basis.dtype == torch.float64 else L.DLC_F32, _ptr(basis), m,
            ldb, _ptr(scale), _ptr(out), self._ld_out(out, rows, m), code, _ptr(ws), ws.numel() if ws is not None else 0, self._stream()))
        self._wrote(out)
        return out[:, :m]

    _VERIFY_MODELS = {"similarity": L.DLC_VERIFY_SIMILARITY, "translation": L.DLC_VERIFY_TRANSLATION}

    def _patch_store(self, who, what, desc, pts):
        """The checks of a frame store -> (desc, pts, frames, P, H, ld): descriptors fp64 [frames, P, H] or
        [frames * P, H] on the device (a row-strided 2-D view is taken as it is) and points int32 [frames, P, 2]."""
        if not isinstance(pts, torch.Tensor) or pts.dim() != 3 or pts.shape[2] != 2 or pts.dtype != torch.int32 or \
                pts.device != self.device or pts.shape[0] < 1 or pts.shape[1] < 1:
            raise ValueError("%s: %s points must be an int32 tensor [frames, P, 2] on %s" % (who, what, self.device))
        frames, p = pts.shape[0], pts.shape[1]
        if isinstance(desc, torch.Tensor) and desc.dim() == 3:
            if desc.shape[0] != frames or desc.shape[1] != p:
                raise ValueError("%s: %s descriptors %s do not go with points %s" % (who, what, tuple(desc.shape), tuple(pts.shape)))
            desc = desc.contiguous().view(frames * p, desc.shape[2])
        desc, rows, h, ld = self._f64_rows(who, "%s descriptors" % what, desc)
        if rows != frames * p:
            raise ValueError("%s: %d %s descriptor rows are not %d frames of %d patches" % (who, rows, what, frames, p))
        return desc, pts.contiguous(), frames, p, h, ld

    def verify_pairs(self, q_desc, q_pts, db_desc, db_pts, cand, model="similarity", tol=3, max_scale=2.0, mutual=True,
                     with_mask=False, with_match=False):
        """Geometric verification of loop candidates (dlc_verify_pairs, include/dlc.h): for every pair (query frame r,
        key-frame cand[r, s]) the patches are matched by DIST (nearest neighbour, mutual: cross-checked), a 2-D
        `model` ("similarity": rotation + uniform scale + translation from two matches; "translation": from one) is
        fitted to the matched key-points by trying EVERY hypothesis in integer arithmetic, and the matches within `tol`
        pixels of the best one are counted.  Exact and a function of the pair alone.

        q_desc fp64 [Q, P, H] (or [Q * P, H]) with q_pts int32 [Q, P, 2]; db_desc / db_pts the same for N key-frames;
        cand int64 [Q, k] (ids outside 0..N-1 give 0 inliers).  max_scale: the similarity's scale must lie within
        [1 / s, s], 1 <= s <= 16, taken as round(16 s) / 16; None: no bound.  Points are (x, y) with 0 <= x, y <= 8191;
        any other point is absent, (-1, -1) being what the Harris pass writes past a frame's point count.
        -> (inliers int32 [Q, k], n_matches int32 [Q, k]) on the device; with_mask: + hyp int32 [Q, k, 2] and mask int64
        [Q, k] (bit p: match p is an inlier; the uint64 word of the C ABI); with_match: + match int32 [Q, k, P]."""
        who = "verify_pairs"
        if model not in self._VERIFY_MODELS:
            raise ValueError("%s: model=%r is none of %s" % (who, model, sorted(self._VERIFY_MODELS)))
        if int(tol) != tol or not 0 <= tol <= 255:
            raise ValueError("%s: tol=%r outside 0..255" % (who, tol))
        s16 = 0
        if max_scale is not None:
            s16 = int(round(16 * float(max_scale)))
            if not 16 <= s16 <= 256:
                raise ValueError("%s: max_scale=%r outside 1..16" % (who, max_scale))
        qd, qp, q, p, h, ldq = self._patch_store(who, "query", q_desc, q_pts)
        dd, dp, n, p2, h2, ldd = self._patch_store(who, "key-frame", db_desc, db_pts)
        if p != p2 or h != h2:
            raise ValueError("%s: queries of %d patches x %d against key-frames of %d x %d" % (who, p, h, p2, h2))
        if p > L.DLC_VERIFY_MAX_PATCHES:
            raise ValueError("%s: %d patches outside 1..%d" % (who, p, L.DLC_VERIFY_MAX_PATCHES))
        if not isinstance(cand, torch.Tensor) or cand.dim() != 2 or cand.dtype != torch.int64 or cand.device != self.device or \
                cand.shape[0] != q or not 1 <= cand.shape[1] <= L.DLC_MAX_K:
            raise ValueError("%s: cand must be an int64 tensor [%d, 1..%d] on %s" % (who, q, L.DLC_MAX_K, self.device))
        k = cand.shape[1]
        cand, ld_cand = self._row_strided(cand, q, k)
        need = self.lib.dlc_verify_pairs_workspace_bytes(q, k, p)
        if need == 0:
            raise ValueError("%s: Q=%d, k=%d, P=%d outside the supported sizes" % (who, q, k, p))
        ws = self.workspace("verify_pairs", need)
        inliers = torch.empty((q, k), dtype=torch.int32, device=self.device)
        matches = torch.empty((q, k), dtype=torch.int32, device=self.device)
        hyp = torch.empty((q, k, 2), dtype=torch.int32, device=self.device) if with_mask else None
        mask = torch.empty((q, k), dtype=torch.int64, device=self.device) if with_mask else None
        match = torch.empty((q, k, p), dtype=torch.int32, device=self.device) if with_match else None
        self._check(self.lib.dlc_verify_pairs(
            self.ctx, _ptr(qd), ldq, _ptr(qp), q, _ptr(dd), ldd, _ptr(dp), n, p, h, _ptr(cand), ld_cand, k,
            self._VERIFY_MODELS[model], int(tol), s16, int(bool(mutual)), _ptr(inliers), _ptr(matches), _ptr(hyp), _ptr(mask),
            _ptr(match), None, _ptr(ws), ws.numel(), self._stream()))
        out = (inliers, matches)
        if with_mask:
            out += (hyp, mask)
        if with_match:
            out += (match,)
        return out

    def peak_topk_rows(self, scores, k, suppress, n=None, limit0=None, limit_step=0, lower_is_better=False, absent=None,
                       poison=None):
        """(scores [rows, k], idx [rows, k] int64): distinct-place candidates, the windowed peak top-k of
        dlc_peak_topk_rows (include/dlc.h).  Per row of scores [rows, >= n] (fp64, fp32 or int64 on the device; a
        row-strided view is taken as it is) the best cell among its first clamp(limit0 + r * limit_step, 0, n) (limit0
        None = n), then the best one more than `suppress` columns from it, and so on: k picks, best first, ties -> the
        lower column.  A NaN is never taken; absent (int64 rows only): a value that marks a cell as not there (the -1 of
        sequence_scores).  Scores are fp64 (int64 for int64 rows); empty slots (-inf or +inf, -1), (-1, -1) for int64.
        poison: a device int64 [1] read by the kernels; non-zero -> every fp64 slot (NaN, -1)."""
        scores, rows, n, ld = self._score_matrix("peak_topk_rows", scores, n, "pick from")
        k, suppress = int(k), int(suppress)
        if not 1 <= k <= L.DLC_MAX_K:
            raise ValueError("peak_topk_rows: k=%d outside 1..%d" % (k, L.DLC_MAX_K))
        if not 0 <= suppress < 1 << 63:
            raise ValueError("peak_topk_rows: suppress=%d outside 0..2^63-1" % suppress)
        is_int = scores.dtype == torch.int64
        if absent is not None and not is_int:
            raise ValueError("peak_topk_rows: absent is for int64 rows (a float row marks absence with NaN)")
        if poison is not None:
            self._check_poison("peak_topk_rows", poison, is_int)
        o_s = torch.empty((rows, k), dtype=self._OUT_DTYPES[scores.dtype], device=self.device)
        o_i = torch.empty((rows, k), dtype=torch.int64, device=self.device)
        need = self.lib.dlc_peak_topk_rows_workspace_bytes(rows, n, k)
        if need == 0:
            raise ValueError("peak_topk_rows: rows=%d, n=%d outside the supported sizes" % (rows, n))
        ws = self.workspace("peak_topk_rows", need)
        self._check(self.lib.dlc_peak_topk_rows(
            self.ctx, self._SEQ_DTYPES[scores.dtype], _ptr(scores), rows, n, ld, *_limits(n, limit0, limit_step),
            int(bool(lower_is_better)), suppress, *_absent(absent), k, _ptr(o_s), _ptr(o_i), _ptr(poison), _ptr(ws), ws.numel(),
            self._stream()))
        return o_s, o_i

    _TRACK_PLANS = {None: L.DLC_TRACK_AUTO, "auto": L.DLC_TRACK_AUTO, "resident": L.DLC_TRACK_RESIDENT, "rows": L.DLC_TRACK_ROWS}

    def track_state(self, n, dtype):
        """A fresh state of track_rows for rows of `dtype`: (V [n], head [4]) -- V float64 (int64 for int64 rows) holding
        the absent mark, NaN / INT64_MIN, and an all-zero head."""
        out = self._OUT_DTYPES[dtype]
        mark = float("nan") if out == torch.float64 else -(1 << 63)
        return (torch.full((int(n),), mark, dtype=out, device=self.device), torch.zeros(4, dtype=torch.int64, device=self.device))

    def track_rows(self, scores, V, head, steps=(0, 2), jump=0.0, gate=0.0, null_score=float("nan"), n=None, limit0=None,
                   limit_step=0, lower_is_better=False, plan=None, back=False, dense=False):
        """Place tracking, the max-plus filter of dlc_track_rows (include/dlc.h), over the next rows of a traversal:
        scores [rows, >= n] (fp64, fp32 or int64 on the device; a row-strided view is taken as it is), row r offering its
        first clamp(limit0 + r * limit_step, 0, n) cells (limit0 None = n).  V [>= n] and head [4] are the state
        (track_state), updated in place.  steps = (d_min, d_max): the key-frames a place may advance per frame at no
        cost; jump: the cost of any other place; gate: the cost of entering or leaving "no loop"; null_score: what a
        frame that closes no loop scores, NaN = there is no such state.  Returns (place, g, G, U, backU, back, dense):
        per row the filtered place (int64, -1 = no loop), the best column g, its value G and the no-loop value U (fp64,
        int64 for int64 rows; absent = NaN / INT64_MIN), the no-loop state's back-pointer (int8); back: the cells'
        back-pointers int8 [rows, n] (back=True, or an int8 tensor [rows, >= n] to write them into), else None; dense:
        V of every row [rows, n], else None.  plan: None / "auto", "resident" (n <= 8192) or "rows"."""
        who = "track_rows"
        scores, rows, n, ld = self._score_matrix(who, scores, n, "track")
        d_min, d_max = check_steps(steps)
        if plan not in self._TRACK_PLANS:
            raise ValueError("%s: plan=%r is none of auto, resident, rows" % (who, plan))
        out_dtype = self._OUT_DTYPES[scores.dtype]
        if not isinstance(V, torch.Tensor) or V.dim() != 1 or V.dtype != out_dtype or V.device != self.device or V.shape[0] < n \
                or not V.is_contiguous():
            raise ValueError("%s: V must be a contiguous %s tensor [>= %d] on %s" % (who, out_dtype, n, self.device))
        self._check_out("head", head, (4,), torch.int64)
        o_back = None
        if isinstance(back, torch.Tensor):
            if back.dim() != 2 or back.dtype != torch.int8 or back.device != self.device or back.shape[0] != rows \
                    or back.shape[1] < n or back.stride(1) != 1 or (rows > 1 and back.stride(0) < n):
                raise ValueError("%s: back must be an int8 tensor [%d, >= %d] on %s with unit column stride" % (who, rows, n, self.device))
            o_back = back
        elif back:
            o_back = torch.empty((rows, n), dtype=torch.int8, device=self.device)
        ld_back = 0 if o_back is None else self._ld_out(o_back, rows, n)
        o_dense = torch.empty((rows, n), dtype=out_dtype, device=self.device) if dense else None
        place, g = (torch.empty(rows, dtype=torch.int64, device=self.device) for _ in range(2))
        o_G, o_U = (torch.empty(rows, dtype=out_dtype, device=self.device) for _ in range(2))
        o_bu = torch.empty(rows, dtype=torch.int8, device=self.device)
        need = self.lib.dlc_track_rows_workspace_bytes(rows, n, self._TRACK_PLANS[plan])
        if need == 0:
            raise ValueError("%s: rows=%d, n=%d outside what plan %r takes" % (who, rows, n, plan))
        ws = self.workspace(who, need)
        self._check(self.lib.dlc_track_rows(
            self.ctx, self._SEQ_DTYPES[scores.dtype], _ptr(scores), rows, n, ld, *_limits(n, limit0, limit_step), d_min, d_max,
            int(bool(lower_is_better)), float(jump), float(gate), float(null_score), self._TRACK_PLANS[plan], _ptr(V), _ptr(head),
            _ptr(place), _ptr(g), _ptr(o_G), _ptr(o_U), _ptr(o_bu), _ptr(o_back), ld_back, _ptr(o_dense), n, _ptr(ws), ws.numel(),
            self._stream()))
        for t in (V, head) + ((back,) if isinstance(back, torch.Tensor) else ()):
            self._wrote(t)
        return place, g, o_G, o_U, o_bu, o_back, o_dense

    def track_backtrace(self, back, backU, g, end=L.DLC_TRACK_END_FILTERED, place_last=None, n=None):
        """The labelling behind a state (dlc_track_backtrace, include/dlc.h): back int8 [rows, >= n], backU int8 [rows] and
        g int64 [rows] are track_rows' outputs for every row of a traversal so far; end: the last row's state to start
        from -- a column, -1 for no loop, or DLC_TRACK_END_FILTERED (the default): place_last, a device int64 [1], the last
        row's filtered place.  Returns path int64 [rows]: every row's key-frame, -1 = no loop, -2 where no path exists."""
        who = "track_backtrace"
        if not isinstance(back, torch.Tensor) or back.dim() != 2 or back.dtype != torch.int8 or back.device != self.device \
                or back.shape[0] < 1 or back.stride(1) != 1:
            raise ValueError("%s: back must be an int8 tensor [rows, >= n] on %s" % (who, self.device))
        rows = back.shape[0]
        n = back.shape[1] if n is None else int(n)
        if not 1 <= n <= back.shape[1]:
            raise ValueError("%s: n=%d outside 1..%d" % (who, n, back.shape[1]))
        self._check_out("backU", backU, (rows,), torch.int8)
        self._check_out("g", g, (rows,), torch.int64)
        end = int(end)
        if end == L.DLC_TRACK_END_FILTERED:
            self._check_out("place_last", place_last, (1,), torch.int64)
        elif not -1 <= end < n:
            raise ValueError("%s: end=%d is no column of %d, -1 or DLC_TRACK_END_FILTERED" % (who, end, n))
        path = torch.empty(rows, dtype=torch.int64, device=self.device)
        self._check(self.lib.dlc_track_backtrace(
            self.ctx, rows, n, _ptr(back), self._ld_out(back, rows, n), _ptr(backU), _ptr(g),
            _ptr(place_last if end == L.DLC_TRACK_END_FILTERED else None), end, _ptr(path), self._stream()))
        return path

    def _truth_mask(self, who, truth, rows, n):
        """The checks of a truth mask [rows, >= n] (uint8 or bool on the device; non-zero = a true match) -> (truth, ld):
        a row-strided view is taken as it is, anything else made contiguous."""
        if not isinstance(truth, torch.Tensor) or truth.dim() != 2 or truth.dtype not in (torch.uint8, torch.bool):
            raise ValueError("%s: truth must be a 2-D uint8 or bool tensor" % who)
        if truth.device != self.device:
            raise ValueError("%s: truth must be on %s" % (who, self.device))
        if truth.shape[0] != rows or truth.shape[1] < n:
            raise ValueError("%s: truth [%d, %d] does not cover scores [%d, %d]" % (who, truth.shape[0], truth.shape[1], rows, n))
        if truth.dtype == torch.bool:
            truth = truth.view(torch.uint8)
        return self._row_strided(truth, rows, n)

    def sorted_thresholds(self, thresholds, is_int):
        """The threshold table pr_cell_counts hands to the library, on the device: the numbers of `thresholds` (a sequence
        or a tensor) ascending and distinct in the order of dlc.h -- -0.0 below +0.0, two thresholds -- as float64, or as
        int64 for int64 rows (which take integers only).  A NaN, no threshold or more than 4096 distinct ones: ValueError."""
        t = thresholds if isinstance(thresholds, torch.Tensor) else torch.as_tensor(np.asarray(thresholds))
        if is_int and (t.is_floating_point() or t.dtype == torch.bool):
            raise ValueError("pr_cell_counts: int64 rows take integer thresholds")
        t = t.reshape(-1).to(device=self.device, dtype=torch.int64 if is_int else torch.float64)
        if not is_int:
            if bool(t.isnan().any()):
                raise ValueError("pr_cell_counts: a threshold is NaN")
            # the bits of a double as a signed integer, the magnitude of the negatives flipped: ordered as the numbers
            # are, the two zeros apart; the flip is its own inverse
            flip = lambda b: torch.where(b < 0, b ^ 0x7FFFFFFFFFFFFFFF, b)
            t = flip(torch.unique(flip(t.view(torch.int64)))).view(torch.float64)
        else:
            t = torch.unique(t)
        if not 1 <= t.numel() <= 4096:
            raise ValueError("pr_cell_counts: %d distinct thresholds outside 1..4096" % t.numel())
        return t.contiguous()

    def pr_cell_counts(self, scores, truth, thresholds, n=None, limit0=None, limit_step=0, lower_is_better=False, absent=None):
        """(pos [T + 1], neg [T + 1]) int64: the cell-level decisions behind a precision-recall curve, dlc_pr_cell_counts
        (include/dlc.h).  Every cell row r of scores [rows, >= n] offers (its first clamp(limit0 + r * limit_step, 0, n),
        limit0 None = n; never a NaN, nor `absent` in int64 rows) falls into the bin #{i : t_i <= x} (#{i : t_i < x} with
        lower_is_better) of the thresholds and is counted there as a positive (truth [rows, >= n] non-zero) or a negative.
        thresholds: any sequence or tensor of numbers; they are sorted and de-duplicated here (T = what is left, 1..4096),
        a NaN is refused."""
        scores, rows, n, ld = self._score_matrix("pr_cell_counts", scores, n, "count")
        truth, ldt = self._truth_mask("pr_cell_counts", truth, rows, n)
        is_int = scores.dtype == torch.int64
        if absent is not None and not is_int:
            raise ValueError("pr_cell_counts: absent is for int64 rows (a float row marks absence with NaN)")
        t = self.sorted_thresholds(thresholds, is_int)
        pos = torch.empty(t.numel() + 1, dtype=torch.int64, device=self.device)
        neg = torch.empty(t.numel() + 1, dtype=torch.int64, device=self.device)
        need = self.lib.dlc_pr_cell_counts_workspace_bytes(rows, n, t.numel())
        if need == 0:
            raise ValueError("pr_cell_counts: rows=%d, n=%d outside the supported sizes" % (rows, n))
        ws = self.workspace("pr_cell_counts", need)
        self._check(self.lib.dlc_pr_cell_counts(
            self.ctx, self._SEQ_DTYPES[scores.dtype], _ptr(scores), rows, n, ld, *_limits(n, limit0, limit_step),
            int(bool(lower_is_better)), *_absent(absent),
            _ptr(truth), ldt, _ptr(t), t.numel(), _ptr(pos), _ptr(neg), _ptr(ws), ws.numel(), self._stream()))
        return pos, neg

    def positive_rank_rows(self, scores, truth, n=None, limit0=None, limit_step=0, lower_is_better=False, absent=None):
        """(rank [rows], idx [rows], npos [rows]) int64: the retrieval protocol, dlc_positive_rank_rows (include/dlc.h).
        Per row of scores [rows, >= n]: idx = the best offered cell that truth [rows, >= n] marks (ties -> the lower
        column), rank = the number of offered cells that beat it (its slot in the row's top-k list), npos = the number of
        offered marked cells; (-1, -1, 0) for a row without one.  Offered as in peak_topk_rows."""
        scores, rows, n, ld = self._score_matrix("positive_rank_rows", scores, n, "rank")
        truth, ldt = self._truth_mask("positive_rank_rows", truth, rows, n)
        if absent is not None and scores.dtype != torch.int64:
            raise ValueError("positive_rank_rows: absent is for int64 rows (a float row marks absence with NaN)")
        rank, idx, npos = (torch.empty(rows, dtype=torch.int64, device=self.device) for _ in range(3))
        need = self.lib.dlc_positive_rank_rows_workspace_bytes(rows, n)
        if need == 0:
            raise ValueError("positive_rank_rows: rows=%d, n=%d outside the supported sizes" % (rows, n))
        ws = self.workspace("positive_rank_rows", need)
        self._check(self.lib.dlc_positive_rank_rows(
            self.ctx, self._SEQ_DTYPES[scores.dtype], _ptr(scores), rows, n, ld, *_limits(n, limit0, limit_step),
            int(bool(lower_is_better)), *_absent(absent),
            _ptr(truth), ldt, _ptr(rank), _ptr(idx), _ptr(npos), _ptr(ws), ws.numel(), self._stream()))
        return rank, idx, npos

    # ---- cosine + top-k -----------------------------------------------------------------
    @staticmethod
    def stored_width(d):
        """Width of a stored descriptor row: d zero-padded to a multiple of 64."""
        return (d + K_STEP - 1) // K_STEP * K_STEP

    def normalize(self, x, dtype="bf16", center=False, out=None):
        """Rows of x [n,d] (float32/float64) -> stored descriptors [n, d_pad]
        (bf16/fp16, L2-normalised, zero-padded to a multiple of 64), into `out` if given."""
        dt = torch_dtype(dtype)
        if dt not in (torch.bfloat16, torch.float16):
            raise ValueError("stored descriptor dtype must be bf16 or fp16")
        if x.dtype not in (torch.float32, torch.float64):
            raise ValueError("normalize: float32 or float64 input")
        x = x.contiguous()
        n, d = x.shape
        ldd = self.stored_width(d)
        if out is None:
            out = torch.empty((n, ldd), dtype=dt, device=self.device)
        elif out.shape != (n, ldd) or out.dtype != dt or not out.is_contiguous() or out.device != self.device:
            raise ValueError("normalize: out must be a contiguous [%d, %d] %s tensor on %s" % (n, ldd, dt, self.device))
        if n > 0:
            self._check(self.lib.dlc_l2_normalize_rows(self.ctx, _TORCH_TO_DLC[x.dtype], _ptr(x), n, d, x.stride(0),
                                                        1 if center else 0, _TORCH_TO_DLC[dt], _ptr(out), ldd,
                                                        self._stream()))
        # the mark unit_rows() looks for: THIS tensor object, at this version, holds rows of norm <= 1.005.  A view or a copy
        # does not carry it and an in-place write outdates it -- torch's own or the library's through a raw pointer
        # (_wrote: upload(out=), this call) -- then the match measures the norms instead of trusting
        self._wrote(out)
        out._dlc_unit_rows = out._version
        return out

    @staticmethod
    def unit_rows(t):
        """True when t is a tensor normalize() wrote and nothing has written to it since: its rows are what the cosine
        certificate's static tau is derived for (include/dlc.h, NORMS)."""
        return getattr(t, "_dlc_unit_rows", None) == t._version

    def max_row_norm(self, rows, out=None):
        """Device float [1]: max(out, the largest L2 norm of the stored rows [n, d]) rounded up (dlc_max_row_norm); out
        starts at 0 when not given.  What a database of rows normalize() did NOT write owes the certificate."""
        if rows.dim() != 2 or rows.dtype not in (torch.bfloat16, torch.float16) or rows.stride(1) != 1:
            raise ValueError("max_row_norm: stored rows [n, d] (bf16 / fp16, contiguous rows)")
        if out is None:
            out = torch.zeros((1,), dtype=torch.float32, device=self.device)
        else:
            self._check_out("out", out, (1,), torch.float32)
        if rows.shape[0] > 0:
            self._check(self.lib.dlc_max_row_norm(self.ctx, _TORCH_TO_DLC[rows.dtype], _ptr(rows), rows.shape[0],
                                                   rows.stride(0), rows.shape[1], _ptr(out), self._stream()))
        return out

    def cosine_tau_scale(self, q, db_max_norm=None, out=None, stream=None):
        """[Q] floats: what query i's certificate multiplies tau by, max(1, |q_i| R / 1.01) with R = db_max_norm (a device
        float [1] from max_row_norm; None: the database rows are normalize()'s) -- dlc_cosine_tau_scale."""
        if q.dim() != 2 or q.dtype not in (torch.bfloat16, torch.float16) or q.stride(1) != 1:
            raise ValueError("cosine_tau_scale: stored queries [Q, d] (bf16 / fp16, contiguous rows)")
        if out is None:
            out = torch.empty((q.shape[0],), dtype=torch.float32, device=self.device)
        else:
            self._check_out("out", out, (q.shape[0],), torch.float32)
        if db_max_norm is not None:
            self._check_out("db_max_norm", db_max_norm, (1,), torch.float32)
        st = C.c_void_p(stream.cuda_stream) if stream is not None else self._stream()
        if q.shape[0] > 0:
            self._check(self.lib.dlc_cosine_tau_scale(self.ctx, _TORCH_TO_DLC[q.dtype], _ptr(q), q.shape[0], q.stride(0),
                                                       q.shape[1], _ptr(db_max_norm), _ptr(out), st))
        return out

    def _check_stored(self, q, db):
        if q.dim() != 2 or db.dim() != 2 or q.shape[1] != db.shape[1]:
            raise ValueError("stored descriptors must be 2-D with one width")
        if q.dtype != db.dtype or q.dtype not in (torch.bfloat16, torch.float16):
            raise ValueError("stored descriptors must both be bf16 or both fp16")
        if q.stride(1) != 1 or db.stride(1) != 1:
            raise ValueError("stored descriptor rows must be contiguous")

    def match_topk(self, q, db, k, row_offset=0, out=None, details=False, older_than=None, tau_scale=None):
        """Top-k cosine match of stored queries q [Q,d] against stored db [N,d].
        Returns (scores [Q,k] float32, idx [Q,k] int64 with row_offset added); with details=True a
        TopK(scores, idx, scores_f64, status): the fp64 scores the order was decided on and, per query,
        0 = certified by the selection, 2 = resolved by the exhaustive pass (include/dlc.h).
        older_than = L: query i only sees db rows below L + i (dlc_cosine_topk_older; (-inf, -1) where it sees fewer than k).
        tau_scale: None states that q and db are normalize()'s rows; otherwise cosine_tau_scale(q, max_row_norm(db))
        (KeyframeDatabase.match_topk keeps track of that by itself)."""
        self._check_stored(q, db)
        nq, d = q.shape
        if tau_scale is not None:
            self._check_out("tau_scale", tau_scale, (nq,), torch.float32)
        n = db.shape[0]
        need = self.lib.dlc_cosine_topk_workspace_bytes(nq, n, d, k)
        if need == 0:
            raise ValueError("match_topk: k=%d outside 1..%d (or empty operand)" % (k, L.DLC_MAX_K))
        if older_than is None:
            need += self.lib.dlc_cosine_topk_prune_bytes(nq, n, d, k)      # room for the pruned score pass's state (dlc.h)
        ws = self.workspace("topk", need)
        if out is None:
            scores = torch.empty((nq, k), dtype=torch.float32, device=self.device)
            idx = torch.empty((nq, k), dtype=torch.int64, device=self.device)
        else:
            scores = self._check_out("out[0] (scores)", out[0], (nq, k), torch.float32)
            idx = self._check_out("out[1] (idx)", out[1], (nq, k), torch.int64)
        s64 = torch.empty((nq, k), dtype=torch.float64, device=self.device) if details else None
        status = torch.empty((nq,), dtype=torch.int32, device=self.device) if details else None
        if older_than is None:
            self._check(self.lib.dlc_cosine_topk(self.ctx, _TORCH_TO_DLC[q.dtype], _ptr(q), nq, q.stride(0), _ptr(db), n,
                                                  db.stride(0), d, k, row_offset, _ptr(scores), _ptr(s64), _ptr(idx),
                                                  _ptr(status), _ptr(tau_scale), _ptr(ws), ws.numel(), self._stream()))
        else:
            self._check(self.lib.dlc_cosine_topk_older(self.ctx, _TORCH_TO_DLC[q.dtype], _ptr(q), nq, q.stride(0), _ptr(db), n,
                                                        db.stride(0), d, k, row_offset, int(older_than), _ptr(scores),
                                                        _ptr(s64), _ptr(idx), _ptr(status), _ptr(tau_scale), _ptr(ws),
                                                        ws.numel(), self._stream()))
        return TopK(scores, idx, s64, status) if details else (scores, idx)

    def topk_workspace_bytes(self, nq, n, d, k):
        need = self.lib.dlc_cosine_topk_workspace_bytes(nq, n, d, k)
        if need == 0:
            raise ValueError("k=%d outside 1..%d (or empty operand)" % (k, L.DLC_MAX_K))
        return need

    def score_error_bound(self, nq, n, d, k):
        """tau of the plan a [nq, d] x [n, d] top-k match takes: |fp32 score of the score pass - fp64 score| <= tau."""
        return float(self.lib.dlc_cosine_score_error_bound(nq, n, d, k))

    def score_error_bound_any_plan(self, d):
        """The largest tau any plan has for descriptors of (stored) width d: what a sharded merge certifies with -- the same
        number on every rank, whatever plan its shard's size picks."""
        return float(self.lib.dlc_cosine_score_error_bound_any_plan(d))

    def score_groups(self, q, db, k, ws, stream=None):
        """Stage 1 of match_topk (the MFMA score GEMM) into the caller's workspace tensor."""
        self._check_stored(q, db)
        self._check_ws(ws)
        st = C.c_void_p(stream.cuda_stream) if stream is not None else self._stream()
        self._check(self.lib.dlc_cosine_score_groups(self.ctx, _TORCH_TO_DLC[q.dtype], _ptr(q), q.shape[0], q.stride(0),
                                                      _ptr(db), db.shape[0], db.stride(0), q.shape[1], k, _ptr(ws),
                                                      ws.numel(), st))

    def select_topk(self, q, db, k, ws, scores, idx, row_offset=0, coop=False, stream=None, scores_f64=None, status=None,
                    tau_scale=None, hints=True, serial=False):
        """Stage 2 of match_topk (selection, fp64 re-score, final top-k, certificate, exhaustive pass) from the workspace.
        hints=False re-scores every selected group whole (DLC_SELECT_NO_HINTS): the same results, more rows gathered.
        serial=True selects without the threshold filter (DLC_SELECT_SERIAL): the same results, for tests."""
        self._check_stored(q, db)
        self._check_ws(ws)
        self._check_out("scores", scores, (q.shape[0], k), torch.float32)
        self._check_out("idx", idx, (q.shape[0], k), torch.int64)
        if scores_f64 is not None:
            self._check_out("scores_f64", scores_f64, (q.shape[0], k), torch.float64)
        if status is not None:
            self._check_out("status", status, (q.shape[0],), torch.int32)
        st = C.c_void_p(stream.cuda_stream) if stream is not None else self._stream()
        self._check(self.lib.dlc_cosine_select_topk(self.ctx, _TORCH_TO_DLC[q.dtype], _ptr(q), q.shape[0], q.stride(0),
                                                     _ptr(db), db.shape[0], db.stride(0), q.shape[1], k, row_offset,
                                                     _ptr(scores), _ptr(scores_f64), _ptr(idx), _ptr(status),
                                                     _ptr(tau_scale), _ptr(ws), ws.numel(),
                                                     (L.DLC_SELECT_COOP if coop else 0) |
                                                     (0 if hints else L.DLC_SELECT_NO_HINTS) |
                                                     (L.DLC_SELECT_SERIAL if serial else 0), st))

    def _check_ws(self, ws):
        if not isinstance(ws, torch.Tensor) or ws.dtype != torch.uint8 or not ws.is_contiguous() or ws.device != self.device:
            raise ValueError("workspace must be a contiguous uint8 tensor on %s" % (self.device,))

    def groups_per_query(self, k):
        kg = self.lib.dlc_cosine_groups_per_query(k)
        if kg == 0:
            raise ValueError("k=%d outside 1..%d" % (k, L.DLC_MAX_K))
        return kg

    def select_groups(self, q, db, k, ws, grp_ids, grp_max, coop=False, stream=None, serial=False):
        """Stage 2a: the kg best groups of every query: shard-local ids [Q,kg] and grp_max [Q,kg+1] = their maxima +
        (last column) the best maximum among the groups that are not listed.  serial=True: DLC_SELECT_SERIAL."""
        self._check_stored(q, db)
        self._check_ws(ws)
        kg = self.groups_per_query(k)
        self._check_out("grp_ids", grp_ids, (q.shape[0], kg), torch.int32)
        self._check_out("grp_max", grp_max, (q.shape[0], kg + 1), torch.float32)
        st = C.c_void_p(stream.cuda_stream) if stream is not None else self._stream()
        self._check(self.lib.dlc_cosine_select_groups(self.ctx, _TORCH_TO_DLC[q.dtype], _ptr(q), q.shape[0], q.stride(0),
                                                       _ptr(db), db.shape[0], db.stride(0), q.shape[1], k, _ptr(ws),
                                                       ws.numel(), _ptr(grp_ids), _ptr(grp_max),
                                                       (L.DLC_SELECT_COOP if coop else 0) |
                                                       (L.DLC_SELECT_SERIAL if serial else 0), st))

    def rescore_topk(self, q, db, k, grp_ids, grp_max, scores_f64, idx, bound=None, all_max=None, row_offset=0, coop=False,
                     stream=None, tau_scale=None):
        """Stage 2b: fp64 re-score of the listed groups (filtered against all shards' maxima when all_max
        [parts, Q, kg+1] is given): the shard's part of the top-k (fp64 scores, rows) and bound [Q] = the best fp32
        score any row outside the surviving groups of all shards can have."""
        self._check_stored(q, db)
        kg = self.groups_per_query(k)
        self._check_out("grp_ids", grp_ids, (q.shape[0], kg), torch.int32)
        self._check_out("grp_max", grp_max, (q.shape[0], kg + 1), torch.float32)
        self._check_out("scores_f64", scores_f64, (q.shape[0], k), torch.float64)
        self._check_out("idx", idx, (q.shape[0], k), torch.int64)
        if bound is not None:
            self._check_out("bound", bound, (q.shape[0],), torch.float32)
        if all_max is not None:
            self._check_out("all_max", all_max, (all_max.shape[0], q.shape[0], kg + 1), torch.float32)
        st = C.c_void_p(stream.cuda_stream) if stream is not None else self._stream()
        parts = 0 if all_max is None else all_max.shape[0]
        self._check(self.lib.dlc_cosine_rescore_topk(self.ctx, _TORCH_TO_DLC[q.dtype], _ptr(q), q.shape[0], q.stride(0),
                                                      _ptr(db), db.shape[0], db.stride(0), q.shape[1], k, row_offset,
                                                      _ptr(grp_ids), _ptr(grp_max), _ptr(all_max), parts, _ptr(scores_f64),
                                                      _ptr(idx), _ptr(bound), _ptr(tau_scale),
                                                      L.DLC_SELECT_COOP if coop else 0, st))

    def exhaustive_topk(self, q, db, k, ws, lower, tau, status, scores_f64, idx, scores=None, row_offset=0, stream=None,
                        tau_scale=None):
        """The exhaustive pass of the sharded protocol for the queries with status == 1: lower [Q] fp64 = the k-th score
        found so far; this shard's exact top-k over every group whose maximum (in `ws`, the workspace of the score
        pass) is >= lower - tau replaces scores_f64 / idx (and scores) of those queries; their status becomes 2."""
        self._check_stored(q, db)
        self._check_ws(ws)
        nq = q.shape[0]
        self._check_out("lower", lower, (nq,), torch.float64)
        self._check_out("status", status, (nq,), torch.int32)
        self._check_out("scores_f64", scores_f64, (nq, k), torch.float64)
        self._check_out("idx", idx, (nq, k), torch.int64)
        if scores is not None:
            self._check_out("scores", scores, (nq, k), torch.float32)
        st = C.c_void_p(stream.cuda_stream) if stream is not None else self._stream()
        self._check(self.lib.dlc_cosine_exhaustive_topk(self.ctx, _TORCH_TO_DLC[q.dtype], _ptr(q), nq, q.stride(0), _ptr(db),
                                                         db.shape[0], db.stride(0), q.shape[1], k, row_offset, _ptr(lower), 1,
                                                         float(tau), _ptr(tau_scale), _ptr(status), _ptr(scores),
                                                         _ptr(scores_f64), _ptr(idx), _ptr(ws), ws.numel(), st))

    def topk_merge_packed(self, gathered, nq, k, out, bound=None, tau=0.0, scores_f64=None, status=None, tau_scale=None):
        """Merge an all-gather of packed per-shard results: gathered is uint8 [parts, nq*k*16], each part = int64 idx
        [nq,k] followed by float64 scores [nq,k].  With bound [nq] / tau the merge certifies into status [nq]."""
        parts = gathered.shape[0]
        self._check_out("gathered", gathered, (parts, nq * k * 16), torch.uint8)
        base = gathered.data_ptr()
        o_s = self._check_out("out[0] (scores)", out[0], (nq, k), torch.float32)
        o_i = self._check_out("out[1] (idx)", out[1], (nq, k), torch.int64)
        if bound is not None:
            self._check_out("bound", bound, (nq,), torch.float32)
        if scores_f64 is not None:
            self._check_out("scores_f64", scores_f64, (nq, k), torch.float64)
        if status is not None:
            self._check_out("status", status, (nq,), torch.int32)
        self._check(self.lib.dlc_topk_merge_strided(self.ctx, C.c_void_p(base + nq * k * 8), nq * k * 2,
                                                     C.c_void_p(base), nq * k * 2, parts, nq, k, _ptr(bound), float(tau),
                                                     _ptr(tau_scale), _ptr(o_s), _ptr(scores_f64), _ptr(o_i), _ptr(status),
                                                     self._stream()))
        return o_s, o_i

    def topk_keep_older(self, scores, idx, limit0, k):
        """Row b of best-first (scores, idx) [B, kk] -> its first k entries with 0 <= id < limit0 + b, (-inf, -1) after."""
        scores, idx = scores.contiguous(), idx.contiguous()
        if scores.dim() != 2 or idx.shape != scores.shape or scores.dtype != torch.float32 or idx.dtype != torch.int64:
            raise ValueError("topk_keep_older: scores float32 / idx int64 of one shape [B, kk]")
        b, kk = scores.shape
        o_s = torch.empty((b, k), dtype=torch.float32, device=self.device)
        o_i = torch.empty((b, k), dtype=torch.int64, device=self.device)
        self._check(self.lib.dlc_topk_keep_older(self.ctx, _ptr(scores), _ptr(idx), b, kk, int(limit0), int(k), _ptr(o_s),
                                                  _ptr(o_i), self._stream()))
        return o_s, o_i

    def topk_merge(self, scores_f64, idx, out=None, details=False):
        """Merge [parts, Q, k] per-shard results (fp64 scores: the order is decided on them) into the global [Q, k]:
        (scores float32, idx); with details=True a TopK with the merged fp64 scores too."""
        scores_f64, idx = scores_f64.contiguous(), idx.contiguous()
        if scores_f64.dim() != 3 or idx.shape != scores_f64.shape or scores_f64.dtype != torch.float64 or \
                idx.dtype != torch.int64:
            raise ValueError("topk_merge: scores float64 / idx int64 of one shape [parts, Q, k]")
        parts, nq, k = scores_f64.shape
        if out is None:
            o_s = torch.empty((nq, k), dtype=torch.float32, device=self.device)
            o_i = torch.empty((nq, k), dtype=torch.int64, device=self.device)
        else:
            o_s = self._check_out("out[0] (scores)", out[0], (nq, k), torch.float32)
            o_i = self._check_out("out[1] (idx)", out[1], (nq, k), torch.int64)
        o_64 = torch.empty((nq, k), dtype=torch.float64, device=self.device) if details else None
        self._check(self.lib.dlc_topk_merge(self.ctx, _ptr(scores_f64), _ptr(idx), parts, nq, k, _ptr(o_s), _ptr(o_64),
                                             _ptr(o_i), self._stream()))
        return TopK(o_s, o_i, o_64, None) if details else (o_s, o_i)

    def cosine_scores(self, q, db):
        self._check_stored(q, db)
        nq, d = q.shape
        n = db.shape[0]
        s = torch.empty((nq, n), dtype=torch.float32, device=self.device)
        need = self.lib.dlc_cosine_scores_workspace_bytes(nq, n, d)          # split-K partials; 0 for most shapes
        ws = self.workspace("scores", need) if need else None
        self._check(self.lib.dlc_cosine_scores(self.ctx, _TORCH_TO_DLC[q.dtype], _ptr(q), nq, q.stride(0), _ptr(db), n,
                                                db.stride(0), d, _ptr(s), s.stride(0), _ptr(ws) if need else None,
                                                need, self._stream()))
        return s

    def cosine_score_rows(self, q, db, limit0=None, limit_step=0, out=None, keys=False, out_keys=None):
        """The cosine path's score as rows (dlc_cosine_score_rows, include/dlc.h): float64 [Q, N], the fp64 score of every
        stored query row of q [Q, d] against the stored rows of db [N, d] (bf16 / fp16, one dtype, one width: a multiple
        of 8) -- bit for bit the number match_topk(details=True) reports for that pair -- and / or its ordering keys,
        int64 [Q, N] = round-half-even(score * 2^40), the integer the cosine path ranks by.  Query r is written in its
        first clamp(limit0 + r * limit_step, 0, N) cells (limit0 None = N: all of them); the other cells keep what the
        caller's tensor held, and hold NaN (scores) / INT64_MIN (keys) -- "not offered" -- where the engine allocates.
        out / out_keys: caller-kept float64 / int64 [Q, N] tensors, which may be views whose rows lie further apart than
        N, both with one row stride (their columns past N are left alone too).  Returns the scores; with keys=True (or
        out_keys given) the keys -- (scores, keys) when `out` is given as well."""
        if q.dim() != 2 or db.dim() != 2 or q.dtype != db.dtype or q.dtype not in (torch.bfloat16, torch.float16):
            raise ValueError("cosine_score_rows: q and db must be 2-D, both bf16 or both fp16")
        if q.device != self.device or db.device != self.device:
            raise ValueError("cosine_score_rows: q and db must be on %s" % self.device)
        if q.shape[1] != db.shape[1]:
            raise ValueError("cosine_score_rows: q and db widths differ (%d, %d)" % (q.shape[1], db.shape[1]))
        if q.stride(1) != 1 or db.stride(1) != 1:
            raise ValueError("cosine_score_rows: stored descriptor rows must be contiguous")
        nq, d = q.shape
        n = db.shape[0]
        want_keys = bool(keys) or out_keys is not None
        want_scores = out is not None or not want_keys

        def result(t, dtype, name, fill):
            return self._rows_out("cosine_score_rows: " + name, t, nq, n, dtype, "a %s" % dtype,
                                  None if limit0 is None else fill)

        o_s = result(out, torch.float64, "out", float("nan")) if want_scores else None
        o_k = result(out_keys, torch.int64, "out_keys", -(1 << 63)) if want_keys else None
        both = o_s is not None and o_k is not None
        ret = (o_s, o_k) if both else (o_k if o_k is not None else o_s)
        if nq == 0 or n == 0:
            return ret
        if d == 0:
            raise ValueError("cosine_score_rows: empty descriptors")
        ld_out = self._ld_out(o_s if o_s is not None else o_k, nq, n)
        if both and nq > 1 and o_k.stride(0) != ld_out:
            raise ValueError("cosine_score_rows: out and out_keys must have one row stride (%d, %d)" % (ld_out, o_k.stride(0)))
        self._check(self.lib.dlc_cosine_score_rows(self.ctx, _TORCH_TO_DLC[q.dtype], _ptr(q), nq, q.stride(0), _ptr(db), n,
                                                    db.stride(0), d, *_limits(n, limit0, limit_step),
                                                    _ptr(o_s), _ptr(o_k), ld_out, self._stream()))
        for t in (o_s, o_k):
            if t is not None:
                self._wrote(t)
        return ret

    # ---- profiling hooks for bench.py ---------------------------------------------------
    def set_profiling(self, enabled):
        self._check(self.lib.dlc_set_profiling(self.ctx, 1 if enabled else 0))

    def set_prune_mode(self, mode):
        """dlc_set_prune_mode: "on" (default), "off" (match_topk's score pass writes every group maximum and hint) or
        "keep" (tests: a repeated identical match_topk starts from its own final threshold; include/dlc.h)."""
        self._check(self.lib.dlc_set_prune_mode(self.ctx, {"on": L.DLC_PRUNE_ON, "off": L.DLC_PRUNE_OFF,
                                                           "keep": L.DLC_PRUNE_KEEP}[mode]))

    def profile_gemm_ms(self, capacity=256):
        """Durations (ms) of the last product-kernel launches (score GEMM, dense and Gram GEMMs;
        one entry per launch, split-K reduces not included), from HIP events recorded on the
        launch stream (blocks until they complete)."""
        buf = (C.c_float * capacity)()
        n = self.lib.dlc_profile_gemm_ms(self.ctx, buf, capacity)
        if n < 0:
            self._check(n)
        return [float(buf[i]) for i in range(n)]


_default = {}


def default_engine(device=None):
    """Process-wide engine for the current (or given) device."""
    if device is None:
        if not torch.cuda.is_available():
            L.load()   # raises ImportError first if the library itself is missing
            raise RuntimeError("deeploopcloser_amd needs a visible MI355X; there is no CPU fallback")
        device = torch.cuda.current_device()
    elif not isinstance(device, int):
        device = torch.device(device).index or 0      # one engine per GPU, whatever names it
    if device not in _default:
        _default[device] = Engine(device)
    return _default[device]
