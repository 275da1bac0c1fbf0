"""SDAV / DA encoders with the reference's call surface, running on MI355X.

Mirrors src/sdav/network/SDAV.py (class SDAV: ctor :14, hyper-parameters
:30-39, transform :293-302) and src/sdav/network/DenoisingAutoencoderVariant.py
(class DA: ctor :15-26, transform :254-259; its greedy training :103-243 through
dlc_da_train_step, see DA).  The forward chain is one C-ABI
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


def _is_number(v):
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, (bool, np.bool_))


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))


def validate_da_params(input_shape, hidden_units, sparse_level, sparse_penalty, consecutive_penalty, batch_size,
                       learning_rate, epochs, layer_n, corruption_level):
    """DA._validate_params (DenoisingAutoencoderVariant.py:66-90) as ValueErrors, with two deliberate differences: ints
    pass for the float parameters and layer_n = 0 passes (the reference's own rules reject its defaults: `positive()`
    on layer_n = 0, `float_()` on SDA's sparse_penalty = 1).  Touches no device."""
    if (not isinstance(input_shape, (list, tuple)) or len(input_shape) != 2 or
            any(not _is_int(v) or v <= 0 for v in input_shape)):
        raise ValueError("input_shape must be a list of two positive ints")      # v8n rule, :89-90
    if not _is_int(hidden_units) or hidden_units <= 0:
        raise ValueError("hidden_units must be a positive int")                  # :83-84
    for name, v in (("learning_rate", learning_rate), ("sparse_level", sparse_level)):          # :70-72
        if not _is_number(v) or not v > 0:
            raise ValueError("%s must be a positive number, got %r" % (name, v))
    for name, v in (("sparse_penalty", sparse_penalty), ("consecutive_penalty", consecutive_penalty),
                    ("corruption_level", corruption_level)):                                    # :74-77
        if not _is_number(v) or not 0 <= v <= 1:
            raise ValueError("%s must lie in [0, 1], got %r" % (name, v))
    if not _is_int(layer_n) or layer_n < 0:
        raise ValueError("layer_n must be an int >= 0, got %r" % (layer_n,))
    for name, v in (("batch_size", batch_size), ("epochs", epochs)):                           # :79-83
        if not _is_int(v) or v <= 0:
            raise ValueError("%s must be a positive int, got %r" % (name, v))


class DA:
    """One denoising-autoencoder layer (DenoisingAutoencoderVariant.py): transform (:116-119, 254-259) and greedy
    training (:103-148 step, :182-202 corruption, :210-243 fit_dataset) through dlc_da_train_step.

    Defined where the reference is not:
      * weights N(0,1), biases zero (:92-101), drawn once at construction from the seed: np.random.RandomState(seed) at
        layer_n 0, RandomState([seed, layer_n]) above it (the layers of an SDA draw apart);
      * the static salt-and-pepper corruption -- int(batch_size*P*K*corruption_level) zeros over the whole flat batch,
        salt on half of them -- is a function of (seed, layer_n) (dlc_salt_pepper_mask_f64), drawn once and reused for
        every batch and step, as the reference's graph constant is;
      * training is float64 only; a batch must hold exactly batch_size frames (the masks' shape), at least 2;
      * the reference never checkpoints (`step + 1 % 10` is never 0, :234); here checkpoint_file (a path prefix, None by
        default) saves an .npz at the end of fit_dataset; fit() visits files in sorted order (input.load_frames);
      * validation (validate_da_params) accepts layer_n >= 0 and ints for the float parameters, and runs before any
        device is touched.
    """

    def __init__(self, input_shape, hidden_units, sparse_level=0.05, sparse_penalty=1.0, consecutive_penalty=0.2,
                 batch_size=10, learning_rate=0.1, epochs=100, layer_n=0, corruption_level=0.3, seed=0,
                 dtype="float64", device=None):
        validate_da_params(input_shape, hidden_units, sparse_level, sparse_penalty, consecutive_penalty, batch_size,
                           learning_rate, epochs, layer_n, corruption_level)
        self.input_shape = [int(v) for v in input_shape]
        self.hidden_units = int(hidden_units)
        self.sparse_level, self.sparse_penalty = sparse_level, sparse_penalty
        self.consecutive_penalty, self.batch_size = consecutive_penalty, int(batch_size)
        self.learning_rate, self.epochs = learning_rate, int(epochs)
        self.corruption_level, self.layer_n = corruption_level, int(layer_n)
        self.seed = int(seed)
        self.engine = default_engine(device)
        self.dtype = {"float64": torch.float64, "float32": torch.float32}[dtype]
        w_seed = self.seed if self.layer_n == 0 else [self.seed & 0xffffffff, self.layer_n]
        ws, bs = _init_weights([self.input_shape[1], self.hidden_units], w_seed, self.dtype, self.engine.device)
        self._w0, self._b0 = ws[0], bs[0]
        self._b1 = torch.zeros(self.input_shape[1], dtype=self.dtype, device=self.engine.device)      # :99-101
        self._masks = None
        self._step_graph = None
        self.global_step = 0
        self.checkpoint_file = None

    # ---- weights ------------------------------------------------------------------
    def set_weights(self, w, b=None, b_dec=None):
        w = self.engine.to_device(w, self.dtype)
        if tuple(w.shape) != (self.input_shape[1], self.hidden_units):
            raise ValueError("W must be %s" % ((self.input_shape[1], self.hidden_units),))
        b = self.engine.to_device(b if b is not None else np.zeros(self.hidden_units), self.dtype)
        bd = self.engine.to_device(b_dec if b_dec is not None else np.zeros(self.input_shape[1]), self.dtype)
        if b.numel() != self.hidden_units or bd.numel() != self.input_shape[1]:
            raise ValueError("b must have %d entries, b_dec %d" % (self.hidden_units, self.input_shape[1]))
        self._w0, self._b0, self._b1 = w.contiguous(), b.reshape(-1).contiguous(), bd.reshape(-1).contiguous()

    def get_weights(self):
        """(W [in, hidden], b_enc [hidden], b_dec [in]) as float64 host arrays."""
        return tuple(t.to(torch.float64).cpu().numpy() for t in (self._w0, self._b0, self._b1))

    def save_weights(self, path):
        w, b, bd = self.get_weights()
        np.savez(path, w=w, b_enc=b, b_dec=bd, global_step=np.array(self.global_step))

    def load_weights(self, path):
        z = np.load(path)
        self.set_weights(z["w"], z["b_enc"], z["b_dec"])
        self.global_step = int(z["global_step"])

    # ---- encode ---------------------------------------------------------------------
    def transform(self, x, batch_n: int = -1):
        x = self.engine.to_device(x, self.dtype)
        if list(x.shape) != self.input_shape:
            raise ValueError("expected input of shape %s, got %s" % (self.input_shape, tuple(x.shape)))
        h = self.engine.gemm_bias_act(x, self._w0, self._b0, act=L.DLC_ACT_SIGMOID)
        return h.to(torch.float64).cpu().numpy()

    def transform_tensor(self, x):
        """A batch x [B, P, in] (or [rows, in]) on any device -> sigmoid(x W + b_enc) [B*P, hidden] on the GPU."""
        x = self.engine.to_device(x, self.dtype)
        if x.dim() not in (2, 3) or x.shape[-1] != self.input_shape[1] or (x.dim() == 3 and x.shape[1] != self.input_shape[0]):
            raise ValueError("expected input of shape [B, %d, %d], got %s" % (self.input_shape[0], self.input_shape[1],
                                                                              tuple(x.shape)))
        x2 = x.reshape(-1, self.input_shape[1])
        if x2.shape[0] == 0:
            return torch.empty((0, self.hidden_units), dtype=self.dtype, device=self.engine.device)
        return self.engine.gemm_bias_act(x2, self._w0, self._b0, act=L.DLC_ACT_SIGMOID)

    # ---- training -----------------------------------------------------------------
    def corruption_masks(self):
        """The static (zeros, ones) masks [batch_size*P, in] (_corrupt_tensor, :182-202), drawn on first use: read-only
        views for tests -- training reads the masks themselves."""
        m = self._corruption_masks()
        return tuple(t.view(self.batch_size * self.input_shape[0], self.input_shape[1]).detach().clone() for t in m)

    def _corruption_masks(self):
        if self._masks is None:
            n = self.batch_size * self.input_shape[0] * self.input_shape[1]
            zeros = torch.empty(n, dtype=torch.float64, device=self.engine.device)
            ones = torch.empty(n, dtype=torch.float64, device=self.engine.device)
            self.engine.salt_pepper_mask(zeros, ones, int(n * self.corruption_level), self.seed, self.layer_n)
            self._masks = (zeros, ones)
        return self._masks

    def _check_batch(self, x):
        if self.dtype != torch.float64:
            raise ValueError("training runs in float64, like the reference")
        x = self.engine.to_device(x, torch.float64)
        if x.dim() != 3 or list(x.shape[1:]) != self.input_shape:
            raise ValueError("expected a batch of shape [%d, %d, %d], got %s" % (self.batch_size, self.input_shape[0],
                                                                                 self.input_shape[1], tuple(x.shape)))
        if x.shape[0] < 2:
            raise ValueError("a training batch needs at least 2 frames (the consecutive-frame loss term)")
        if x.shape[0] != self.batch_size:
            raise ValueError("a training batch holds batch_size=%d frames (the corruption masks' shape), got %d"
                             % (self.batch_size, x.shape[0]))
        return x.contiguous()

    def _step(self, x2, xt, loss, ws=None):
        self.engine.da_train_step(x2, xt, self.batch_size, self.input_shape[0], self._w0, self._b0, self._b1,
                                  self.sparse_level, self.sparse_penalty, self.consecutive_penalty, self.learning_rate,
                                  loss_out=loss, ws=ws)

    def train_step(self, x):
        """One sess.run(self.train_step) (:231) on a batch x [batch_size, P, in]; returns {loss, cd, cs, cc} (GPU tensor
        of 4 doubles) evaluated before the update."""
        x = self._check_batch(x)
        zeros, ones = self._corruption_masks()
        x2 = x.reshape(-1, self.input_shape[1])
        xt = self.engine.da_corrupt(x2, zeros, ones)
        loss = torch.empty(4, dtype=torch.float64, device=self.engine.device)
        self._step(x2, xt, loss)
        self.global_step += 1
        return loss

    def train_steps(self, x, n_steps):
        """n_steps consecutive train_step on ONE batch (the inner loop of fit_dataset, :230-236).  x~ is fixed within a
        batch, so it is formed once here; the step is captured ONCE as a HIP graph over fixed buffers (batch, x~,
        workspace, loss) and replayed, re-captured when a parameter tensor, the split-K scratch or a hyper-parameter (a
        kernel argument baked into the graph) changes -- as SDAV.train_steps.  Same arithmetic as train_step, same bits.
        Returns the loss tensor {loss, cd, cs, cc} of the last step (before its update)."""
        x = self._check_batch(x)
        eng = self.engine
        sig = (self._w0.data_ptr(), self._b0.data_ptr(), self._b1.data_ptr(),
               eng._scratch.data_ptr() if eng._scratch is not None else 0,
               float(self.learning_rate), float(self.sparse_level), float(self.sparse_penalty), float(self.consecutive_penalty))
        g = self._step_graph
        if g is None or g["sig"] != sig:
            rows = self.batch_size * self.input_shape[0]
            g = {"sig": sig, "x": torch.empty((rows, self.input_shape[1]), dtype=torch.float64, device=eng.device),
                 "xt": torch.empty((rows, eng.even_pitch(self.input_shape[1])), dtype=torch.float64, device=eng.device),
                 "loss": torch.zeros(4, dtype=torch.float64, device=eng.device), "graph": None,
                 "ws": eng.da_train_workspace(self.batch_size, self.input_shape[0], self.input_shape[1], self.hidden_units)}
            self._step_graph = g
        zeros, ones = self._corruption_masks()
        g["x"].copy_(x.reshape(-1, self.input_shape[1]))
        eng.da_corrupt(g["x"], zeros, ones, out=g["xt"])

        def one_step():
            self._step(g["x"], g["xt"], g["loss"], ws=g["ws"])

        done = 0
        if g["graph"] is None and n_steps >= 3:
            one_step()                                       # eager first: kernel attributes and pools exist before capture
            done = 1
            torch.cuda.synchronize(eng.device)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):                    # (a capture records the launches, it does not run them)
                one_step()
            g["graph"] = graph
        for _ in range(done, n_steps):
            if g["graph"] is not None:
                g["graph"].replay()
            else:
                one_step()
        self.global_step += n_steps
        return g["loss"]

    def _fit_batches(self, batches):
        """fit_dataset's loop over device batches [b, P, in]: `epochs` steps per full batch, a short batch ends the fit
        with the reference's warning (:224-228); one loss line per batch (the last step's, before its update)."""
        with self.engine.latency_mode():
            for batch_n, b in enumerate(batches):
                if b.shape[0] != self.batch_size:
                    logging.warning("Ignored last batch because it was smaller than the specified batch size. To avoid "
                                    "this choose a batch size that is a factor of the dataset size.")
                    break
                loss = self.train_steps(b, self.epochs)
                if logging.getLogger().isEnabledFor(logging.INFO):
                    logging.info("    Layer:%d Batch:%d fit, Epoch:%d/%d, Loss:%s" %
                                 (self.layer_n, batch_n, self.epochs, self.epochs, float(loss[0].item())))
        if self.checkpoint_file:
            self.save_weights("%s-%d.npz" % (self.checkpoint_file, self.global_step))

    def fit_dataset(self, dataset):
        """DA.fit_dataset (:210-243): frames [P, in] (host or device) in batches of batch_size."""
        frames = [self.engine.to_device(f, torch.float64) for f in dataset]
        bs = self.batch_size
        self._fit_batches([torch.stack(frames[i:i + bs]) for i in range(0, len(frames), bs)])

    def fit(self, file_pattern, key_points_fn=None):
        """DA.fit (:204-208): the parsed frames of the files matching file_pattern (sorted), then fit_dataset."""
        from .input import load_frames
        logging.info("  Layer:%d fit" % self.layer_n)
        self.fit_dataset(load_frames(file_pattern, self.input_shape, key_points_fn, device=self.engine.device))
