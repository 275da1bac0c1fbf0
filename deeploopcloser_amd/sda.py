"""SDA: a stack of DA layers trained greedily, one layer at a time, on MI355X.

Mirrors src/sdav/network/StackedDenoisingAutoencoderVariants.py (class SDA: ctor :12-41, validation :51-72, layers
:74-84, fit :90-100), the network train-sdav.py builds.  Layer 0 fits on the parsed frames; layer i fits on the frames
mapped through layers 0..i-1.  Each layer is a DA (sdav.py) and every step is dlc_da_train_step.

Defined where the reference is not ("defined where undefined"):
  * trained lower layers: the reference's DA never checkpoints (`step + 1 % 10 == 0` is never true,
    DenoisingAutoencoderVariant.py:234), so its chained `previous_layer.transform` re-initialises random weights on every
    call (:168-174, :254-259); here layer i learns from the TRAINED layers 0..i-1;
  * seeded draws: layer i's weights and its static salt-and-pepper masks are functions of (seed, i) (DA);
  * validation accepts ints for the float parameters (the reference's `float_()` rejects its own sparse_penalty = 1)
    and runs before any device is acquired;
  * files are visited in sorted order (input.load_frames; the reference's glob order is the file system's, and the
    consecutive-frame term depends on it);
  * the reference's SDA has no transform; this one has transform (the chained encoders) and weight persistence.
"""
import logging

import numpy as np
import torch

from .engine import default_engine
from .sdav import DA, _is_int, validate_da_params


def validate_sda_params(input_shape, hidden_units, sparse_level, sparse_penalty, consecutive_penalty, batch_size,
                        learning_rate, epochs, corruption_level):
    """SDA._validate_params (:51-72) as ValueErrors (ints pass for the float parameters).  Touches no device."""
    if not isinstance(hidden_units, (list, tuple)) or len(hidden_units) < 2 or \
            any(not _is_int(h) or h <= 0 for h in hidden_units):
        raise ValueError("hidden_units must be a list of at least two positive ints")          # :57
    for i, h in enumerate(hidden_units):
        validate_da_params(input_shape if i == 0 else [input_shape[0], hidden_units[i - 1]], h, sparse_level,
                           sparse_penalty, consecutive_penalty, batch_size, learning_rate, epochs, i, corruption_level)


class SDA:
    """The reference's SDA with `seed`, `device` and `verbosity` added."""

    def __init__(self, input_shape, hidden_units, sparse_level=0.05, sparse_penalty=1, consecutive_penalty=0.2,
                 batch_size=10, learning_rate=0.1, epochs=100, corruption_level=0.3, seed=0, device=None,
                 verbosity=logging.WARNING):
        validate_sda_params(input_shape, hidden_units, sparse_level, sparse_penalty, consecutive_penalty, batch_size,
                            learning_rate, epochs, corruption_level)
        logging.getLogger().setLevel(verbosity)
        self.input_shape = [int(v) for v in input_shape]
        self.hidden_units = [int(h) for h in hidden_units]
        self.sparse_level, self.sparse_penalty = sparse_level, sparse_penalty
        self.consecutive_penalty, self.batch_size = consecutive_penalty, int(batch_size)
        self.learning_rate, self.epochs = learning_rate, int(epochs)
        self.corruption_level = corruption_level
        self.seed = int(seed)
        self.engine = default_engine(device)
        self.checkpoint_file = None                 # a path prefix: "<prefix>-layer<i>.npz" after layer i is trained
        self._layers = []
        for i, h in enumerate(self.hidden_units):   # _define_model (:74-84)
            shape = self.input_shape if i == 0 else [self.input_shape[0], self.hidden_units[i - 1]]
            self._layers.append(DA(shape, h, sparse_level=sparse_level, sparse_penalty=sparse_penalty,
                                   consecutive_penalty=consecutive_penalty, batch_size=self.batch_size,
                                   learning_rate=learning_rate, epochs=self.epochs, layer_n=i,
                                   corruption_level=corruption_level, seed=self.seed, device=self.engine.device))

    @property
    def layers(self):
        return list(self._layers)

    # ---- training -----------------------------------------------------------------
    def fit_dataset(self, frames):
        """Greedy layer-wise fit on frames [P, input_shape[1]] (host or device).  The frames are uploaded once; layer i's
        inputs for the whole dataset are computed once, on the device, from layer i-1's trained encoder and stay
        resident, one tensor per batch, until layer i + 1's are made from them."""
        eng = self.engine
        bs, p = self.batch_size, self.input_shape[0]
        with eng.latency_mode():
            data = [eng.to_device(f, torch.float64) for f in frames]
            feats = [torch.stack(data[i:i + bs]) for i in range(0, len(data), bs)]
            del data
            for i, layer in enumerate(self._layers):
                logging.info("Fitting layer %d" % i)
                if i > 0:
                    prev = self._layers[i - 1]
                    feats = [prev.transform_tensor(c).view(c.shape[0], p, prev.hidden_units) for c in feats]
                layer._fit_batches(feats)
                if self.checkpoint_file:
                    self.save_weights("%s-layer%d.npz" % (self.checkpoint_file, i))

    def fit(self, file_pattern, key_points_fn=None):
        """SDA.fit (:90-100) on the parsed frames of the files matching file_pattern (sorted order)."""
        from .input import load_frames
        logging.info("Fit SDAV")
        self.fit_dataset(load_frames(file_pattern, self.input_shape, key_points_fn, device=self.engine.device))

    # ---- encode ---------------------------------------------------------------------
    def transform_tensor(self, x):
        """x [B, P, input_shape[1]] on any device -> [B*P, hidden_units[-1]] float64 on the GPU: the trained encoders
        chained."""
        x = self.engine.to_device(x, torch.float64)
        if x.dim() != 3 or list(x.shape[1:]) != self.input_shape:
            raise ValueError("expected input of shape [B, %d, %d], got %s" % (self.input_shape[0], self.input_shape[1],
                                                                              tuple(x.shape)))
        h = x.reshape(-1, self.input_shape[1])
        for layer in self._layers:
            h = layer.transform_tensor(h)
        return h

    def transform(self, x, chunk_frames=256):
        """x [B, P, input_shape[1]] -> numpy float64 [B*P, hidden_units[-1]], in chunks of chunk_frames frames."""
        if isinstance(x, torch.Tensor):
            return self.transform_tensor(x).cpu().numpy()
        x = np.asarray(x, dtype=np.float64)
        if x.ndim != 3 or list(x.shape[1:]) != self.input_shape:
            raise ValueError("expected input of shape [B, %d, %d], got %s" % (self.input_shape[0], self.input_shape[1],
                                                                              tuple(x.shape)))
        out = np.empty((x.shape[0] * x.shape[1], self.hidden_units[-1]), dtype=np.float64)
        for f0 in range(0, x.shape[0], chunk_frames):
            f1 = min(f0 + chunk_frames, x.shape[0])
            out[f0 * x.shape[1]:f1 * x.shape[1]] = self.transform_tensor(x[f0:f1]).cpu().numpy()
        return out

    # ---- weights ------------------------------------------------------------------
    def get_weights(self):
        """[(W, b_enc, b_dec) per layer] as float64 host arrays."""
        return [layer.get_weights() for layer in self._layers]

    def set_weights(self, weights):
        """weights: one (W, b_enc) or (W, b_enc, b_dec) per layer."""
        if len(weights) != len(self._layers):
            raise ValueError("expected the weights of %d layers, got %d" % (len(self._layers), len(weights)))
        for layer, wb in zip(self._layers, weights):
            layer.set_weights(*wb)

    def save_weights(self, path):
        z = {"hidden_units": np.array(self.hidden_units), "input_shape": np.array(self.input_shape)}
        for i, layer in enumerate(self._layers):
            w, b, bd = layer.get_weights()
            z.update({"w%d" % i: w, "b%d" % i: b, "bd%d" % i: bd, "global_step%d" % i: np.array(layer.global_step)})
        np.savez(path, **z)

    def load_weights(self, path):
        z = np.load(path)
        if list(z["hidden_units"]) != self.hidden_units or list(z["input_shape"]) != self.input_shape:
            raise ValueError("%s holds an SDA of input_shape %s, hidden_units %s; this one is %s, %s"
                             % (path, list(z["input_shape"]), list(z["hidden_units"]), self.input_shape, self.hidden_units))
        self.set_weights([(z["w%d" % i], z["b%d" % i], z["bd%d" % i]) for i in range(len(self._layers))])
        for i, layer in enumerate(self._layers):
            layer.global_step = int(z["global_step%d" % i])
