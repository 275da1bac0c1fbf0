"""SDAV / DA encoders with the reference's call surface, running on MI355X.

Mirrors src/sdav/network/SDAV.py (class SDAV: ctor :14, hyper-parameters
:30-39, transform :293-302) and src/sdav/network/DenoisingAutoencoderVariant.py
(class DA: ctor :15-26, transform :254-259).  The forward chain is one C-ABI
call (dlc_sdav_encode): five fp64 MFMA GEMMs with fused bias + sigmoid,
weights resident in HBM instead of a checkpoint restore / re-initialisation on
every call (SDAV.py:232-240).

Differences a caller can see, all deliberate:
  * weights are drawn ONCE at construction (seeded N(0,1), the reference's
    initialiser SDAV.py:189-217) or loaded with load_weights(); the reference
    re-draws them on every transform() when no checkpoint exists;
  * fit / fit_dataset run the reference's per-layer SGD
    (SDAV.py:242-288) through dlc_sdav_train_step; the masking noise comes from a seeded
    torch generator; checkpoints are .npz files (save_weights), not TF checkpoints;
    a batch of a single frame (NaN loss in the reference) is rejected / skipped;
  * get_dataset needs key-points: the reference's SURF detector is not available, the
    default is the build's Harris detector (input.harris_key_points) unless key_points_fn(shape) is given.
"""
import logging

import numpy as np
import torch

from . import _lib as L
from .engine import default_engine


def _init_weights(dims, seed, dtype, device, scale="reference"):
    rng = np.random.RandomState(seed)
    ws, bs = [], []
    for k, n in zip(dims[:-1], dims[1:]):
        w = rng.standard_normal((k, n))
        if scale == "fan_in":
            w = w / np.sqrt(k)
        ws.append(torch.from_numpy(w).to(device=device, dtype=dtype).contiguous())
        bs.append(torch.zeros(n, dtype=dtype, device=device))
    return ws, bs


class SDAV:
    """The reference's SDAV network (SDAV.py).  dtype "float64" (default) matches the reference; "float32" runs the
    same chain in fp32; "f16x2" is the tolerance mode (include/dlc.h: dlc_sdav_encode_split), whose inputs must lie in
    [-16, 16]: a row holding a larger value, an infinity or a NaN comes out as NaN, the other rows are unaffected."""

    def __init__(self, verbosity=logging.WARNING, seed=0, dtype="float64", device=None, weight_scale="reference",
                 hidden_units=None):
        self.logger = logging.getLogger()
        self.logger.setLevel(verbosity)
        self._define_params()
        if hidden_units is not None:
            # NOT the reference's network (SDAV.py:31-32 fixes five layers of 2500): other widths for the same chain, e.g.
            # [2500, 2500, 2500, 2500, 4096] -- the 4096-d patch descriptors BASELINE.json's north_star speaks of
            # ("may be reported additionally, labelled non-reference")
            hu = [int(h) for h in hidden_units]
            if not hu or any(h <= 0 for h in hu):
                raise ValueError("hidden_units: a non-empty list of positive layer widths")
            self.hidden_units = hu
        self.losses = []
        self.engine = default_engine(device)
        # "f16x2": the tolerance mode -- parameters and results stay float64, transform() runs every layer as three fp16 MFMA
        # products of two-piece splits (descriptor relative L2 <= 2e-5 against the fp64 chain; include/dlc.h:
        # dlc_sdav_encode_split); training always runs the fp64 kernels
        self.mode = "f16x2" if dtype == "f16x2" else "exact"
        self.dtype = {"float64": torch.float64, "float32": torch.float32, "f16x2": torch.float64}[dtype]
        # the tolerance mode's prepared weights, keyed on (where the weights live, _weights_gen).  The training kernels
        # update the weights in place through raw pointers -- neither data_ptr() nor torch's version counter moves -- so
        # every entry that can change a weight steps _weights_gen itself (SDAV.py:232-240,293-302: transform always sees the
        # current variables)
        self._panels = None
        self._weights_gen = 0
        dims = [self.input_shape[1]] + list(self.hidden_units)
        self._weights, self._biases = _init_weights(dims, seed, self.dtype, self.engine.device, weight_scale)
        self._biases_dec = [torch.zeros(k, dtype=self.dtype, device=self.engine.device) for k in dims[:-1]]   # :193-217
        self._mask_seed, self._mask_counter = int(seed) + 1, 0
        self.global_step = 0
        self._step_graphs = {}
        self.checkpoint_file = None                 # set to a path prefix to save after each layer (:273-275)
        logging.info("Done initializing sdav")

    def _define_params(self):                      # SDAV.py:30-39
        self.input_shape = [30, 1681]
        self.hidden_units = [2500, 2500, 2500, 2500, 2500]
        self.default_batch_size = 10
        self.sparse_level = 0.05
        self.sparse_penalty = 1.0
        self.consecutive_penalty = 0.2
        self.learning_rate = 0.1
        self.epochs = 100
        self.corruption_level = 0.3

    def get_layer_input_shape(self, layer_n):      # SDAV.py:165-169
        if layer_n == 0:
            return self.input_shape
        return [self.input_shape[0], self.hidden_units[layer_n - 1]]

    def get_layers_input_shapes(self):             # SDAV.py:290-291
        return list(map(self.get_layer_input_shape, range(1, 6)))

    # ---- weights ------------------------------------------------------------------
    def set_weights(self, weights, biases=None):
        """weights: list of 5 arrays [in,out] (W_le of SDAV.py:188-217)."""
        dims = [self.input_shape[1]] + list(self.hidden_units)
        if len(weights) != len(self.hidden_units):
            raise ValueError("expected %d weight matrices" % len(self.hidden_units))
        ws, bs = [], []
        for l, w in enumerate(weights):
            w = self.engine.to_device(w, self.dtype)
            if tuple(w.shape) != (dims[l], dims[l + 1]):
                raise ValueError("W[%d] must be %s, got %s" % (l, (dims[l], dims[l + 1]), tuple(w.shape)))
            b = biases[l] if biases is not None else np.zeros(dims[l + 1])
            b = self.engine.to_device(b, self.dtype)
            if b.numel() != dims[l + 1]:
                raise ValueError("b[%d] must have %d entries" % (l, dims[l + 1]))
            ws.append(w)
            bs.append(b)
        self._weights, self._biases = ws, bs
        self._weights_changed()

    def _weights_changed(self):
        """Called by everything that writes a weight (set_weights / load_weights, train_step, train_steps -- eager and
        graph replay -- and through them fit / fit_dataset): the f16x2 panels of the old values must not be used again."""
        self._weights_gen += 1
        self._panels = None

    def get_weights(self):
        return [w.cpu().numpy() for w in self._weights], [b.cpu().numpy() for b in self._biases]

    def load_weights(self, path):
        """.npz with w0..w4 / b0..b4 (our own format; TF-1 checkpoints are unreadable here)."""
        z = np.load(path)
        n = len(self.hidden_units)
        self.set_weights([z["w%d" % l] for l in range(n)], [z["b%d" % l] for l in range(n)])
        if "bd0" in z:
            self._biases_dec = [self.engine.to_device(z["bd%d" % l], self.dtype) for l in range(n)]
            self.global_step = int(z["global_step"])

    def save_weights(self, path):
        ws, bs = self.get_weights()
        np.savez(path, **{"w%d" % l: w for l, w in enumerate(ws)}, **{"b%d" % l: b for l, b in enumerate(bs)},
                 **{"bd%d" % l: b.cpu().numpy() for l, b in enumerate(self._biases_dec)},
                 global_step=np.array(self.global_step))

    # ---- encode ---------------------------------------------------------------------
    def transform_tensor(self, x, out=None):
        """x: [B,30,1681] on any device -> torch tensor [B*30, 2500] on the GPU (out: the caller's contiguous tensor of that
        shape and the network's dtype to write it into)."""
        x = self.engine.to_device(x, self.dtype)
        if x.dim() != 3 or list(x.shape[1:]) != list(self.input_shape):
            raise ValueError("expected input of shape [B, %d, %d], got %s" %
                             (self.input_shape[0], self.input_shape[1], tuple(x.shape)))
        if x.shape[0] == 0:
            return out if out is not None else torch.empty((0, self.hidden_units[-1]), dtype=self.dtype, device=self.engine.device)
        x2 = x.reshape(x.shape[0] * x.shape[1], x.shape[2])      # flat_batch, TensorflowWrapper.py:13-15
        if self.mode == "f16x2":
            sig = (self._weights_gen,) + tuple((w.data_ptr(), w._version) for w in self._weights)
            if self._panels is None or self._panels[0] != sig:
                self._panels = (sig, self.engine.sdav_split_panels(self._weights))
            dims = [self.input_shape[1]] + list(self.hidden_units)
            return self.engine.sdav_encode_split(x2, dims, self._panels[1], self._biases, out=out)
        return self.engine.sdav_encode(x2, self._weights, self._biases, out=out)

    def transform(self, x, chunk_frames=256):
        """SDAV.transform (SDAV.py:293-302): numpy in, numpy FLAT [B*30, 2500] float64 out.
        A host array is encoded in chunks of `chunk_frames` frames whose upload, five GEMMs and download overlap
        (Engine.run_chunked; pinned staging inside the library): the encode is batch-invariant, so the result is bit
        for bit what one call on the whole batch gives."""
        if isinstance(x, torch.Tensor):
            return self.engine.download(self.transform_tensor(x).to(torch.float64))
        x = np.asarray(x)
        if x.ndim != 3 or list(x.shape[1:]) != list(self.input_shape):
            raise ValueError("expected input of shape [B, %d, %d], got %s" %
                             (self.input_shape[0], self.input_shape[1], tuple(x.shape)))
        if x.shape[0] == 0:
            return np.empty((0, self.hidden_units[-1]), dtype=np.float64)
        if x.dtype not in (np.float64, np.float32):
            x = x.astype(np.float64)
        return self.engine.run_chunked(x, chunk_frames, lambda c: self.transform_tensor(c).to(torch.float64))

    # ---- training (SDAV.py:242-288) ---------------------------------------------------------------
    def _mask(self, layer_n):
        """random_mask (TensorflowWrapper.py:148-156): round(P*K*level) zeros, shuffled, [P, K] -- a new draw per call."""
        p, k = self.get_layer_input_shape(layer_n)
        m = torch.empty((p, k), dtype=torch.float64, device=self.engine.device)
        self._fill_mask(m, layer_n)
        return m

    def train_step(self, layer_n, x, masks=None):
        """One sess.run(self.train_steps[layer_n]) (SDAV.py:262) on batch x [B,30,1681]; returns
        {loss, cd, cs, cc} (GPU tensor of 4 doubles) evaluated before the update."""
        if self.dtype != torch.float64:
            raise ValueError("training runs in float64, like the reference")
        x = self.engine.to_device(x, torch.float64)
        if x.dim() != 3 or list(x.shape[1:]) != list(self.input_shape):
            raise ValueError("expected input of shape [B, %d, %d]" % tuple(self.input_shape))
        if x.shape[0] < 2:
            raise ValueError("a training batch needs at least 2 frames (the consecutive-frame loss term)")
        if masks is None:
            masks = [self._mask(l) for l in range(layer_n + 1)]
        masks = [self.engine.to_device(m, torch.float64) for m in masks]
        loss = torch.empty(4, dtype=torch.float64, device=self.engine.device)
        self.engine.sdav_train_step(layer_n, x.reshape(-1, x.shape[2]), x.shape[0], x.shape[1], masks, self._weights,
                                    self._biases, self._biases_dec[layer_n], self.sparse_level, self.sparse_penalty,
                                    self.consecutive_penalty, self.learning_rate, loss_out=loss)
        self.global_step += 1
        self._weights_changed()
        return loss

    def _fill_mask(self, m, layer_n):
        """A fresh random_mask into an existing [P, K] tensor: one HIP kernel (exact count, uniform placement), the draw a
        function of (the network's seed, a counter stepped per mask)."""
        n = m.numel()
        n_zeros = int(np.round(n * float(self.corruption_level)))
        self.engine.random_mask(m, n_zeros, self._mask_seed, self._mask_counter)
        self._mask_counter += 1

    def train_steps(self, layer_n, x, n_steps):
        """n_steps consecutive sess.run(self.train_steps[layer_n]) on ONE batch (the inner loop of SDAV.fit_dataset /
        SDAV.fit, SDAV.py:257-263: `for step in range(epochs)`), fresh masking noise for every step as the reference's
        corrupt() draws it per run.  The step -- ~20 launches of a few microseconds of work each at the reference's batch of
        10 frames -- is captured ONCE as a HIP graph over fixed buffers (batch, masks, workspace, loss) and replayed:
        what is left per step is the masks' regeneration in place and one graph launch.  Returns the loss tensor
        {loss, cd, cs, cc} of the last step (before its update), as train_step does; same arithmetic, same results."""
        if self.dtype != torch.float64:
            raise ValueError("training runs in float64, like the reference")
        x = self.engine.to_device(x, torch.float64)
        if x.dim() != 3 or list(x.shape[1:]) != list(self.input_shape):
            raise ValueError("expected input of shape [B, %d, %d]" % tuple(self.input_shape))
        if x.shape[0] < 2:
            raise ValueError("a training batch needs at least 2 frames (the consecutive-frame loss term)")
        eng = self.engine
        # everything the captured launches point at -- the parameters, the split-K scratch of latency_mode -- and every
        # scalar they carry: the hyper-parameters are kernel arguments baked into the captured graph, so a change
        # (a learning-rate decay between batches) must force a new capture, as the eager train_step would honour it
        sig = (tuple(w.data_ptr() for w in self._weights), tuple(b.data_ptr() for b in self._biases),
               self._biases_dec[layer_n].data_ptr(), eng._scratch.data_ptr() if eng._scratch is not None else 0,
               float(self.learning_rate), float(self.sparse_level), float(self.sparse_penalty), float(self.consecutive_penalty))
        key = (layer_n, x.shape[0])
        g = self._step_graphs.get(key)
        if g is None or g["sig"] != sig:
            if len(self._step_graphs) > 8:
                self._step_graphs.clear()
            # TWO sets of masks, one graph over each: the next step's masks are drawn on a second stream while this step's
            # graph runs (the draw is one workgroup's 32 us -- a fifteenth of the step when it ran in front of every replay)
            g = {"sig": sig, "x": torch.empty_like(x),
                 "masks": [[torch.empty(tuple(self.get_layer_input_shape(l)), dtype=torch.float64, device=eng.device)
                            for l in range(layer_n + 1)] for _ in range(2)],
                 "loss": torch.zeros(4, dtype=torch.float64, device=eng.device), "graph": None,
                 "drawn": [torch.cuda.Event(), torch.cuda.Event()], "used": [torch.cuda.Event(), torch.cuda.Event()],
                 "ws": eng.train_workspace(layer_n, x.shape[0], x.shape[1], self._weights)}     # its own: the graphs keep pointing at it
            self._step_graphs[key] = g
        g["x"].copy_(x)

        def one_step(b):
            eng.sdav_train_step(layer_n, g["x"].reshape(-1, x.shape[2]), x.shape[0], x.shape[1], g["masks"][b], self._weights,
                                self._biases, self._biases_dec[layer_n], self.sparse_level, self.sparse_penalty,
                                self.consecutive_penalty, self.learning_rate, loss_out=g["loss"], ws=g["ws"])

        main, side = torch.cuda.current_stream(eng.device), eng.side_stream
        # ... where a step draws more than one mask (measured per step, replayed: layer 2 1.36 -> 1.26 ms, layer 4 2.18 ->
        # 2.02; at layer 0 the two cross-stream waits per step cost more than its one draw hides, 0.469 -> 0.489: there the
        # draw stays in front of the replay, on the caller's stream)
        beside = layer_n >= 1

        def draw(b, after=None):
            """Step's masks into set b on the second stream, behind `after` (the last step that read that set)."""
            if not beside:
                for l, m in enumerate(g["masks"][b]):
                    self._fill_mask(m, l)
                return
            if after is not None:
                side.wait_event(after)
            with torch.cuda.stream(side):
                for l, m in enumerate(g["masks"][b]):
                    self._fill_mask(m, l)
                g["drawn"][b].record(side)

        done = 0
        if g["graph"] is None and n_steps >= 3:
            # one eager step first: kernel attributes and the allocator's pools exist before the capture
            for l, m in enumerate(g["masks"][0]):
                self._fill_mask(m, l)
            one_step(0)
            done = 1
            torch.cuda.synchronize(eng.device)
            graphs = []
            for b in range(2):
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):                # (a capture records the launches, it does not run them)
                    one_step(b)
                graphs.append(graph)
            g["graph"] = graphs
        if done < n_steps:
            start = torch.cuda.Event()
            start.record(main)                               # (the sets' last readers are behind this point of the caller's stream)
            draw(done % 2, start)
        for i in range(done, n_steps):
            b = i % 2
            if beside:
                main.wait_event(g["drawn"][b])
            if g["graph"] is not None:
                g["graph"][b].replay()
            else:
                one_step(b)
            if beside:
                g["used"][b].record(main)
            if i + 1 < n_steps:
                draw(1 - b, g["used"][1 - b] if i > done else start)
        self.global_step += n_steps
        self._weights_changed()
        return g["loss"]

    def get_dataset(self, file_pattern: str, key_points_fn=None):
        """Generator of parsed frames [30, 1681] (SDAV.py:219-221, InputGenerator.py:17-27)."""
        from glob import glob
        from .input import CvInputParser, read_ppm
        files = glob(file_pattern)
        if len(files) == 0:
            logging.getLogger().error("Specified dataset is empty or could not find dataset")   # InputGenerator.py:21-23
        parser = CvInputParser(self.input_shape[0], int(round(np.sqrt(self.input_shape[1]))))

        def gen():
            for f in files:
                img = read_ppm(f)
                yield parser.parse(img, key_points_fn(img.shape[:2]) if key_points_fn else None)
        return gen()

    def fit_dataset(self, dataset):
        """SDAV.fit_dataset (:242-275): batches of default_batch_size frames; for each layer, for
        each batch, `epochs` SGD steps on that layer's loss; a checkpoint after each layer."""
        frames = [np.asarray(f, dtype=np.float64) for f in dataset]
        bs = self.default_batch_size
        batches = [np.stack(frames[i:i + bs]) for i in range(0, len(frames), bs)]
        # a 10-frame batch is 300 rows: the step's GEMMs are latency-bound without split-K (6.0 -> 2.8 ms)
        with self.engine.latency_mode():
            for i in range(len(self.hidden_units)):
                logging.info("Fitting layer %d" % i)
                for batch_n, b in enumerate(batches):
                    if b.shape[0] < 2:
                        logging.warning("skipping a batch of %d frame(s): the loss needs >= 2" % b.shape[0])
                        continue
                    xb = self.engine.to_device(b, torch.float64)
                    if self.logger.isEnabledFor(logging.INFO):       # a loss line per step (the reference's log): step by step
                        for step in range(self.epochs):
                            loss = self.train_step(i, xb)
                            logging.info("    Layer:%d Batch:%d fit, Epoch:%d/%d, Loss:%s" %
                                         (i, batch_n, step + 1, self.epochs, float(loss[0].item())))
                    else:
                        self.train_steps(i, xb, self.epochs)         # the same steps, replayed as one HIP graph each
                if self.checkpoint_file:
                    self.save_weights("%s-%d.npz" % (self.checkpoint_file, self.global_step))

    def fit(self, x):
        """SDAV.fit (:277-288): the whole array as one batch, `epochs` steps per layer."""
        xb = self.engine.to_device(x, torch.float64)
        with self.engine.latency_mode():
            for i in range(len(self.hidden_units)):
                self.train_steps(i, xb, self.epochs)


class DA:
    """One denoising-autoencoder layer; only the transform path
    (DenoisingAutoencoderVariant.py:116-119, 254-259)."""

    def __init__(self, input_shape, hidden_units, sparse_level=0.05, sparse_penalty=1.0, consecutive_penalty=0.2,
                 batch_size=10, learning_rate=0.1, epochs=100, layer_n=0, corruption_level=0.3, seed=0,
                 dtype="float64", device=None):
        if (not isinstance(input_shape, (list, tuple)) or len(input_shape) != 2 or
                any((not isinstance(v, (int, np.integer))) or v <= 0 for v in input_shape)):
            raise ValueError("input_shape must be a list of two positive ints")      # v8n rule, :89-90
        if not isinstance(hidden_units, (int, np.integer)) or hidden_units <= 0:
            raise ValueError("hidden_units must be a positive int")                  # :83-84
        self.input_shape = list(input_shape)
        self.hidden_units = int(hidden_units)
        self.sparse_level, self.sparse_penalty = sparse_level, sparse_penalty
        self.consecutive_penalty, self.batch_size = consecutive_penalty, batch_size
        self.learning_rate, self.epochs = learning_rate, epochs
        self.corruption_level, self.layer_n = corruption_level, layer_n
        self.engine = default_engine(device)
        self.dtype = {"float64": torch.float64, "float32": torch.float32}[dtype]
        ws, bs = _init_weights([self.input_shape[1], self.hidden_units], seed, self.dtype, self.engine.device)
        self._w0, self._b0 = ws[0], bs[0]

    def set_weights(self, w, b=None):
        w = self.engine.to_device(w, self.dtype)
        if tuple(w.shape) != (self.input_shape[1], self.hidden_units):
            raise ValueError("W must be %s" % ((self.input_shape[1], self.hidden_units),))
        self._w0 = w
        self._b0 = self.engine.to_device(b if b is not None else np.zeros(self.hidden_units), self.dtype)

    def transform(self, x, batch_n: int = -1):
        x = self.engine.to_device(x, self.dtype)
        if list(x.shape) != self.input_shape:
            raise ValueError("expected input of shape %s, got %s" % (self.input_shape, tuple(x.shape)))
        h = self.engine.gemm_bias_act(x, self._w0, self._b0, act=L.DLC_ACT_SIGMOID)
        return h.to(torch.float64).cpu().numpy()
