"""bore.models on MI355X: the classifier containers of the reference
(bore/models.py:9-45) with the Keras surface its call sites use
(README.rst:60-96; bore/plugins/hpbandster/base.py:145-194), backed by
libbore_hip.so.  ``Sequential`` stands in for ``tensorflow.keras.Sequential``:
same method names, argument meaning and defaults for the subset on the hot path.
"""
from __future__ import annotations

import warnings

import numpy as np
import torch

from . import _lib, ops
from . import shuffle as _shuffle
from .data import resolve_sample_weight
from .layers import Adam, BinaryCrossentropy, Dense, resolve_loss, resolve_optimizer
from .mixins import BatchMaximizableMixin, MaximizableMixin


class History:
    """What Keras ``fit`` returns: ``.history['loss']`` is the per-epoch logged loss.

    The losses are computed by the fit kernel either way; they are DOWNLOADED when first looked at.  ``fit`` itself
    no longer waits for its kernel (round 5): the caller's next lines -- README.rst:93-95 goes straight on to
    ``argmax`` -- run while the device fits, and a loop that never reads the history never pays for the copy."""

    def __init__(self, loss):
        self._loss, self._history = loss, None

    @property
    def history(self):
        if self._history is None:
            loss = self._loss() if callable(self._loss) else self._loss
            self._history = {"loss": [float(v) for v in loss]}
            self._loss = None
        return self._history

    @history.setter
    def history(self, value):        # (Keras' History.history is a plain attribute: callers may assign it)
        self._history, self._loss = value, None

    @property
    def epoch(self):
        return list(range(len(self.history["loss"])))


class Sequential:
    """Ordered stack of Dense layers living on one MI355X.

    State owned by the model across calls (reference: the live Keras object,
    bore/plugins/hpbandster/base.py:196-208): packed parameters ``theta`` in Keras
    ``get_weights()`` order, Adam slots ``m``, ``v`` and the iteration counter
    ``t`` -- so consecutive ``fit`` calls warm-start exactly like Keras.
    """

    def __init__(self, layers=None, name=None, seed=None, dtype_policy="float32"):
        """``dtype_policy``: "float32", or "mixed_bfloat16" (what
        ``tf.keras.mixed_precision.set_global_policy("mixed_bfloat16")`` does to a Keras model:
        float32 variables, bfloat16 compute; wide static shapes only, include/bore_hip.h enum
        bore_compute): fit, predict and the argmax objective all round like bfloat16 math;
        ``evaluate`` reads the float32 master weights."""
        if dtype_policy not in ("float32", "mixed_bfloat16"):
            raise ValueError(f"dtype_policy must be 'float32' or 'mixed_bfloat16', got {dtype_policy!r}")
        self.dtype_policy = dtype_policy
        self.name = name or "sequential"
        self.layers = []
        self._rs = np.random.RandomState(seed)
        self._shuffle_seed = int(self._rs.randint(0, 2**31 - 1)) if seed is None else int(seed)
        self._epochs_seen = 0
        self._desc = None
        self._input_dim = None
        self.theta = self.adam_m = self.adam_v = self.adam_t = None
        self._optimizer = Adam()
        self._loss = None
        self._metrics = []
        self._compiled = False
        for layer in layers or []:
            self.add(layer)

    # -- construction ----------------------------------------------------
    def add(self, layer):
        if not isinstance(layer, Dense):
            raise TypeError("only bore_amd.layers.Dense layers run on the HIP path")
        if self.theta is not None:
            raise RuntimeError("cannot add layers after the model has been built")
        if not self.layers and layer.input_dim is not None:
            self._input_dim = layer.input_dim
        self.layers.append(layer)
        if len(self.layers) > _lib.MAX_LAYERS:
            raise ValueError(f"at most {_lib.MAX_LAYERS} Dense layers are supported")

    @property
    def built(self):
        return self.theta is not None

    def build(self, input_dim=None):
        """Allocate + initialise the parameters (glorot_uniform kernels, zero biases)."""
        if self.built:
            return
        if not self.layers:
            raise RuntimeError("model has no layers")
        if input_dim is None:
            input_dim = self._input_dim
        if input_dim is None:
            raise RuntimeError("input dimension unknown: pass input_dim to the first Dense "
                               "layer or call the model on data first")
        dev = _lib.require_gpu()
        self._input_dim = int(input_dim)
        self._desc = _lib.make_desc(self._input_dim, [l.units for l in self.layers],
                                    [l.activation for l in self.layers],
                                    [l.l2_kernel for l in self.layers],
                                    [l.l2_bias for l in self.layers],
                                    compute="bfloat16" if self.dtype_policy == "mixed_bfloat16"
                                    else "float32")
        P = ops.param_count(self._desc)
        flat = np.stack([self._draw_initial() for _ in range(self._n_models)])     # (one model; an ensemble: its members)
        assert flat.shape == (self._n_models, P)
        self.theta = torch.from_numpy(flat).to(dev).contiguous()
        self.adam_m = torch.zeros_like(self.theta)
        self.adam_v = torch.zeros_like(self.theta)
        self.adam_t = torch.zeros(self._n_models, dtype=torch.int64, device=dev)

    _n_models = 1      # rows of theta

    def _draw_initial(self):
        """One model's packed initial parameters from the model's stream: glorot_uniform kernels, zero biases."""
        ws = []
        fan_in = self._input_dim
        for l in self.layers:
            limit = np.sqrt(6.0 / (fan_in + l.units))
            ws.append(self._rs.uniform(-limit, limit, size=(fan_in, l.units)).astype(np.float32))
            ws.append(np.zeros(l.units, dtype=np.float32))
            fan_in = l.units
        return np.concatenate([w.reshape(-1) for w in ws])

    def _ensure_built(self, x):
        if not self.built:
            self.build(np.shape(x)[-1])
        elif np.shape(x)[-1] != self._input_dim:
            raise ValueError(f"expected input dimension {self._input_dim}, got {np.shape(x)[-1]}")

    def compile(self, optimizer="adam", loss=None, metrics=None, **kwargs):
        self._optimizer = resolve_optimizer(optimizer)
        self._loss = resolve_loss(loss)
        self._metrics = list(metrics or [])
        for m in self._metrics:
            if m not in ("accuracy", "acc", "binary_accuracy"):
                raise NotImplementedError(f"metric {m!r} is not available on the HIP path")
        self._compiled = True

    def _check_loss(self):
        if not self._compiled or self._loss is None:
            raise RuntimeError("compile(optimizer=..., loss=...) the model before fit/evaluate")
        final = self.layers[-1]
        if final.units != 1:
            raise ValueError("the BORE classifier needs a single output unit")
        if self._loss.from_logits and final.activation != "linear":
            raise ValueError("BinaryCrossentropy(from_logits=True) needs a linear output layer")
        if not self._loss.from_logits and final.activation != "sigmoid":
            raise NotImplementedError(
                "binary_crossentropy on probabilities needs a sigmoid output layer (Keras then "
                "uses its logits); other output activations are not implemented")

    # -- data plumbing -----------------------------------------------------
    def _to_dev(self, a, dtype):
        if isinstance(a, torch.Tensor):
            return a.to(device=self.theta.device, dtype=dtype).contiguous()
        a = np.ascontiguousarray(np.asarray(a), dtype={torch.float32: np.float32,
                                                      torch.float64: np.float64}[dtype])
        return torch.from_numpy(a).to(self.theta.device)

    # -- Keras surface -------------------------------------------------------
    def _check_weights_supported(self, **given):
        """``sample_weight`` / ``class_weight`` reach the float32 kernels only: a bfloat16 model refuses them by name."""
        names = [k for k, v in given.items() if v is not None]
        if names and self.dtype_policy != "float32":
            raise _lib.UnsupportedError(f"{' / '.join(names)}: weighted fits are float32 only (this model's "
                                        f"dtype_policy is {self.dtype_policy!r})")

    def fit(self, x, y, batch_size=None, epochs=1, verbose=False, callbacks=None, shuffle=True,
            perm=None, sample_weight=None, class_weight=None, **kwargs):
        """Keras ``fit`` (README.rst:93; bore/plugins/hpbandster/base.py:184).  Any ``batch_size``
        (more than 64 rows: 64-row sub-tiles inside one Adam step, same sums).  ``perm``
        (epochs, N) is an extension: explicit per-epoch shuffles (used by the parity tests);
        default draws them on the device.

        ``callbacks``: objects with any of Keras' ``set_model``, ``on_train_begin``,
        ``on_epoch_begin``, ``on_epoch_end(epoch, logs)`` (logs = {"loss": ...}),
        ``on_train_end``.  Without callbacks the whole fit is ONE kernel; with them it is one
        launch per epoch, so that ``model.stop_training = True`` (early stopping) takes effect at
        the epoch boundary as in Keras -- same arithmetic either way (Adam state and the shuffle
        stream carry over between launches).

        ASYNCHRONOUS without callbacks: the call returns once the kernel is enqueued on the model's stream (launch
        errors -- bad arguments, an unsupported shape -- are raised here; the library checks ``hipGetLastError`` after
        every launch).  The returned ``History`` keeps the device tensor of the losses and downloads it when
        ``.history`` is first read; an error the device reports while the kernel RUNS surfaces at the next call that
        waits for the stream (``.history``, ``predict``, ``argmax``, ``get_weights``), as with any stream-ordered API.
        ``verbose=True`` or callbacks make the call wait.

        ``sample_weight`` ((N,) or (N, 1)) and ``class_weight`` (``{0: a, 1: b}``) as in Keras: a step minimises
        ``sum_i w_i loss_i / rows`` (the divisor is the row count), ``w_i`` the row's sample weight times its class's
        weight.  A weighted fit of a narrow static-shape network runs on that shape's kernels, in the time of its
        unweighted fit; every other network on the generic kernel flavour (or the streamed one).  The same bits under
        unit weights;
        ``UnsupportedError`` for a "mixed_bfloat16" model."""
        self._check_weights_supported(sample_weight=sample_weight, class_weight=class_weight)
        x = np.asarray(x) if not isinstance(x, torch.Tensor) else x
        self._ensure_built(x)
        self._check_loss()
        batch_size = 32 if batch_size is None else int(batch_size)
        if batch_size < 1:
            raise ValueError(f"batch_size must be positive, got {batch_size}")
        if not isinstance(x, torch.Tensor) and not isinstance(y, torch.Tensor):
            # host arrays (the reference's callers): features and labels cross PCIe in ONE copy
            xh = np.asarray(x, dtype=np.float32).reshape(-1, self._input_dim)
            N = xh.shape[0]
            w = resolve_sample_weight(N, y, sample_weight, class_weight)      # (raises before anything is copied)
            # (through a pinned staging buffer the model keeps: the copy is asynchronous and half the cost of one
            # from pageable memory, tools/xfer_probe.py; the buffer is reused once its last copy has been seen done)
            n_both = N * (self._input_dim + 1 + (w is not None))      # (the row weights ride behind the labels)
            st = getattr(self, "_stage", None)
            if st is None or st[0].numel() < n_both:
                st = self._stage = (torch.empty(max(2 * n_both, 1024), dtype=torch.float32).pin_memory(), torch.cuda.Event())
            else:
                st[1].synchronize()
            both = st[0].numpy()[:n_both]
            both[:N * self._input_dim] = xh.ravel()
            both[N * self._input_dim:N * (self._input_dim + 1)] = np.asarray(y).reshape(-1)     # (raises on a length mismatch)
            if w is not None:
                both[N * (self._input_dim + 1):] = w
            both = st[0][:n_both].to(self.theta.device, non_blocking=True)
            st[1].record()
            X = both[:N * self._input_dim].reshape(1, N, self._input_dim)
            z = both[N * self._input_dim:N * (self._input_dim + 1)].reshape(1, N)
            W = None if w is None else both[N * (self._input_dim + 1):].reshape(1, N)
        else:
            X = self._to_dev(x, torch.float32).reshape(1, -1, self._input_dim)
            N = X.shape[1]
            z = self._to_dev(np.asarray(y).reshape(-1) if not isinstance(y, torch.Tensor)
                             else y.reshape(-1), torch.float32).reshape(1, N)
            w = resolve_sample_weight(N, y, sample_weight, class_weight)
            W = None if w is None else torch.from_numpy(w).to(self.theta.device).reshape(1, N)
        return self._run_fit(X, z, W, N, epochs, batch_size, perm, shuffle, verbose, callbacks)

    def _run_fit(self, X, z, W, N, epochs, batch_size, perm, shuffle, verbose, callbacks, n_models=1):
        """The launches of ``fit`` behind the upload: X [L, N, D], z [L, N], W [L, N] or None on the device for the
        L = ``n_models`` models of ``theta`` (1: this model; an ensemble: its members, which share ``perm``).  The
        logged loss is the mean over the models."""
        epochs = int(epochs)
        if perm is None and not shuffle:
            perm = np.tile(np.arange(N, dtype=np.int32), (epochs, 1))
        if perm is not None:
            perm = np.asarray(perm)
            if perm.shape != (epochs, N) or not np.array_equal(np.sort(perm, axis=1),
                                                               np.tile(np.arange(N), (epochs, 1))):
                raise ValueError("perm must hold one permutation of range(N) per epoch")
            perm = torch.from_numpy(np.ascontiguousarray(perm, dtype=np.int32)) \
                .to(self.theta.device).reshape(1, epochs, N)
            if n_models > 1:
                perm = perm.expand(n_models, epochs, N).contiguous()
        o = self._optimizer
        logged = (lambda loss: loss[0]) if n_models == 1 else (lambda loss: loss.mean(dim=0))

        def launch(e0, n_epochs):
            kw = dict(seed=self._shuffle_seed, epoch0=self._epochs_seen, lr=o.learning_rate,
                      beta1=o.beta_1, beta2=o.beta_2, eps=o.epsilon, sample_weight=W)
            try:
                loss = ops.mlp_fit(self._desc, self.theta, self.adam_m, self.adam_v, self.adam_t, X, z,
                                   n_epochs, batch_size,
                                   perm=None if perm is None else perm[:, e0:e0 + n_epochs].contiguous(), **kw)
            except _lib.NeedsPermError:         # (BORE_E_NEEDS_PERM: a code, not a message)
                if perm is not None:
                    raise
                # A data set too long for the device to draw its shuffles in LDS (the reference's fit
                # takes whatever the record holds, README.rst:93): the SAME stream from its host
                # statement (bore_amd.shuffle), a few epochs per launch, read from memory by the kernel.
                chunk = max(1, min(n_epochs, (64 << 20) // (4 * N * n_models)))
                parts = []
                for c0 in range(0, n_epochs, chunk):
                    ne = min(chunk, n_epochs - c0)
                    pc = _shuffle.permutations(self._shuffle_seed, n_models, ne, N, epoch0=self._epochs_seen + c0)
                    pc = torch.from_numpy(pc).to(self.theta.device)
                    parts.append(ops.mlp_fit(self._desc, self.theta, self.adam_m, self.adam_v, self.adam_t,
                                             X, z, ne, batch_size, perm=pc, **kw))
                loss = torch.cat(parts, dim=1)
            self._epochs_seen += n_epochs
            return logged(loss)

        callbacks = list(callbacks or [])
        if not callbacks:
            loss = launch(0, epochs)                 # (enqueued: nothing waits for the kernel here)
            if verbose:
                for e, v in enumerate(loss.cpu().numpy()):
                    print(f"Epoch {e + 1}/{epochs} - loss: {float(v):.4f}")
            return History(lambda: loss.cpu().numpy())

        def call(name, *args):
            for cb in callbacks:
                fn = getattr(cb, name, None)
                if fn is not None:
                    fn(*args)

        self.stop_training = False
        call("set_model", self)
        call("on_train_begin", {})
        losses = []
        for e in range(epochs):
            call("on_epoch_begin", e, {})
            losses.append(float(launch(e, 1).cpu().numpy()[0]))
            call("on_epoch_end", e, {"loss": losses[-1]})
            if self.stop_training:
                break
        call("on_train_end", {})
        return History(np.asarray(losses, dtype=np.float32))

    def evaluate(self, x, y, batch_size=None, verbose=False, sample_weight=None, **kwargs):
        """Keras ``evaluate``: loss, or [loss, accuracy] when compiled with metrics.  ``sample_weight`` ((N,) or
        (N, 1)) weighs the loss, ``sum_i w_i loss_i / N``; the accuracy stays unweighted (Keras applies sample weights
        to ``weighted_metrics`` only)."""
        self._check_weights_supported(sample_weight=sample_weight)
        self._ensure_built(x)
        self._check_loss()
        X = self._to_dev(x, torch.float32).reshape(1, -1, self._input_dim)
        z = self._to_dev(np.asarray(y).reshape(-1), torch.float32).reshape(1, X.shape[1])
        w = resolve_sample_weight(X.shape[1], None, sample_weight, None)
        W = None if w is None else torch.from_numpy(w).to(self.theta.device).reshape(1, -1)
        loss, acc = ops.mlp_evaluate(self._desc, self.theta, X, z, sample_weight=W)
        if self._metrics:
            return [float(loss[0]), float(acc[0])]
        return float(loss[0])

    def predict(self, x, batch_size=None, verbose=0, **kwargs):
        """Keras ``predict``: (N, D) array -> (N, 1) float32 array."""
        self._ensure_built(x)
        X = self._to_dev(x, torch.float32).reshape(-1, self._input_dim)
        out = ops.mlp_forward(self._desc, self.theta, X)
        return out[0].cpu().numpy().reshape(-1, 1)

    def __call__(self, x, training=False):
        return self.predict(x)

    def get_weights(self):
        """Keras order [W1 (in,out), b1, W2, b2, ...] as float32 numpy arrays."""
        if not self.built:
            raise RuntimeError("model is not built yet")
        return self._unpack(self.theta[0].cpu().numpy())

    def _unpack(self, flat):
        """A packed parameter vector as the Keras-order list."""
        out, off, fan_in = [], 0, self._input_dim
        for l in self.layers:
            out.append(flat[off:off + fan_in * l.units].reshape(fan_in, l.units).copy())
            off += fan_in * l.units
            out.append(flat[off:off + l.units].copy())
            off += l.units
            fan_in = l.units
        return out

    def set_weights(self, weights):
        if not self.built:
            self.build(np.shape(weights[0])[0])
        cur = self.get_weights()
        if len(weights) != len(cur) or any(np.shape(a) != b.shape for a, b in zip(weights, cur)):
            raise ValueError("weight shapes do not match the model")
        flat = np.concatenate([np.asarray(w, dtype=np.float32).reshape(-1) for w in weights])
        self.theta.copy_(torch.from_numpy(flat).reshape(1, -1))

    def get_optimizer_state(self):
        """(m, v, t): Adam slots in Keras weight order + iteration counter (checkpointing)."""
        return (self.adam_m[0].cpu().numpy(), self.adam_v[0].cpu().numpy(), int(self.adam_t[0]))

    def set_optimizer_state(self, m, v, t):
        self.adam_m.copy_(torch.from_numpy(np.asarray(m, dtype=np.float32)).reshape(1, -1))
        self.adam_v.copy_(torch.from_numpy(np.asarray(v, dtype=np.float32)).reshape(1, -1))
        self.adam_t.fill_(int(t))

    def count_params(self):
        fan_in, n = self._input_dim, 0
        for l in self.layers:
            n += (fan_in or 0) * l.units + l.units
            fan_in = l.units
        return n

    def summary(self, print_fn=print):
        print_fn(f'Model: "{self.name}"')
        fan_in = self._input_dim
        for i, l in enumerate(self.layers):
            n = "?" if fan_in is None else fan_in * l.units + l.units
            print_fn(f" dense_{i} (Dense)  output (None, {l.units})  activation {l.activation}  "
                     f"params {n}")
            fan_in = l.units
        print_fn(f"Total params: {self.count_params() if self._input_dim else '?'}")


class DenseSequential(Sequential):
    """bore/models.py:9-21.  The reference's loop adds an input layer on ``i == 0`` and
    then falls through to the unconditional add, so ``num_layers`` yields
    ``num_layers + 1`` hidden layers; kept, as the reference's only
    in-repo caller (plugins/hpbandster/base.py:147-155) relies on whatever this builds."""

    def __init__(self, input_dim, output_dim, num_layers, num_units, layer_kws={},
                 final_layer_kws={}, **kwargs):
        super(DenseSequential, self).__init__(**kwargs)
        for i in range(num_layers):
            if not i:
                self.add(Dense(num_units, input_dim=input_dim, **layer_kws))
            self.add(Dense(num_units, **layer_kws))
        self.add(Dense(output_dim, **final_layer_kws))
        if self._input_dim is None:       # num_layers == 0
            self._input_dim = int(input_dim)


class Model(Sequential):
    """Stand-in for ``tensorflow.keras.Model`` restricted to a Dense stack (``layers=[...]``);
    the functional API is not provided (the LSTM factory below does not need it)."""


class MaximizableModel(MaximizableMixin, Model):
    pass


class MaximizableSequential(MaximizableMixin, Sequential):
    pass


class MaximizableDenseSequential(MaximizableMixin, DenseSequential):
    pass


class BatchMaximizableModel(BatchMaximizableMixin, Model):
    pass


class BatchMaximizableSequential(BatchMaximizableMixin, Sequential):
    pass


class BatchMaximizableDenseSequential(BatchMaximizableMixin, DenseSequential):
    pass


class EnsembleSequential(Sequential):
    """``members`` classifiers of one Dense stack, fitted together and read together (an extension over the reference;
    ``bore_amd.ensemble`` states the semantics).  ``theta``, ``adam_m``, ``adam_v`` are ``[K, P]`` and ``adam_t`` is
    ``[K]``: member k draws its own glorot initialisation from the model's seeded stream (member 0 first) and shuffles
    by its own stream (``model_index0 + k``).  ``fit`` is ONE ``ops.mlp_fit`` launch with ``n_models = K`` -- a
    workgroup per member, up to the device's compute units in about the time of one -- so member k's parameters, Adam
    slots and counter equal a lone model's fitted from that member's initial weights with the same seed and
    ``model_index0 = k``, bit for bit.  ``predict`` is the members' mean.

    Refused by name (``UnsupportedError``): ``dtype_policy="mixed_bfloat16"`` and, at build, a network only the
    streamed kernels take (``ops.mlp_streamed(desc) & 2``)."""

    def __init__(self, layers=None, members=4, beta=1.0, **kwargs):
        from .ensemble import check_beta, check_members
        self.members = check_members(members)
        self.beta = check_beta(beta)
        if kwargs.get("dtype_policy", "float32") == "mixed_bfloat16":
            raise _lib.UnsupportedError("an ensemble's members are float32 networks: dtype_policy='mixed_bfloat16' is "
                                        "not available")
        super(EnsembleSequential, self).__init__(layers, **kwargs)

    @property
    def _n_models(self):
        return self.members

    def build(self, input_dim=None):
        if self.built:
            return
        super(EnsembleSequential, self).build(input_dim)
        if ops.mlp_streamed(self._desc) & 2:
            self.theta = self.adam_m = self.adam_v = self.adam_t = None
            raise _lib.UnsupportedError("this network does not fit one workgroup's LDS (only the streamed kernels take "
                                        "it): ensembles keep every member's parameters in LDS")

    def _replicated(self, t):
        """[1, ...] -> [K, ...] on the device: every member sees the same rows."""
        return t.expand(self.members, *t.shape[1:]).contiguous()

    def fit(self, x, y, batch_size=None, epochs=1, verbose=False, callbacks=None, shuffle=True,
            perm=None, sample_weight=None, class_weight=None, **kwargs):
        """``Sequential.fit`` for all members in one launch per call (per epoch with callbacks): the data replicated on
        the device, ``sample_weight`` / ``class_weight`` and ``perm`` -- (epochs, N), shared by the members -- as
        there; the logged loss is the mean over the members."""
        x = np.asarray(x) if not isinstance(x, torch.Tensor) else x
        self._ensure_built(x)
        self._check_loss()
        batch_size = 32 if batch_size is None else int(batch_size)
        if batch_size < 1:
            raise ValueError(f"batch_size must be positive, got {batch_size}")
        X1 = self._to_dev(x, torch.float32).reshape(1, -1, self._input_dim)
        N = X1.shape[1]
        yv = y.reshape(-1) if isinstance(y, torch.Tensor) else np.asarray(y).reshape(-1)
        w = resolve_sample_weight(N, y, sample_weight, class_weight)
        X = self._replicated(X1)
        z = self._replicated(self._to_dev(yv, torch.float32).reshape(1, N))
        W = None if w is None else self._replicated(torch.from_numpy(w).to(self.theta.device).reshape(1, N))
        return self._run_fit(X, z, W, N, epochs, batch_size, perm, shuffle, verbose, callbacks, n_models=self.members)

    def predict_members(self, x):
        """(N, D) -> (K, N, 1) float32: every member's ``predict``."""
        self._ensure_built(x)
        X = self._to_dev(x, torch.float32).reshape(-1, self._input_dim)
        return ops.mlp_forward(self._desc, self.theta, X).cpu().numpy()[..., None]

    def _stats(self, x, beta):
        from .ensemble import ensemble_stats
        return ensemble_stats(self.predict_members(x)[..., 0], beta)

    def predict(self, x, batch_size=None, verbose=0, **kwargs):
        """The members' mean mu: (N, D) -> (N, 1) float32."""
        return self._stats(x, 0.0)[0].astype(np.float32).reshape(-1, 1)

    def predict_std(self, x):
        """The members' spread sigma = sqrt(var + 1e-12): (N, D) -> (N, 1) float32."""
        return self._stats(x, 0.0)[1].astype(np.float32).reshape(-1, 1)

    def predict_score(self, x):
        """The acquisition's score s = mu + beta sigma: (N, D) -> (N, 1) float32."""
        return self._stats(x, self.beta)[2].astype(np.float32).reshape(-1, 1)

    def evaluate(self, x, y, batch_size=None, verbose=False, sample_weight=None, **kwargs):
        """[mean member loss, accuracy of mu] (the loss alone without metrics).  The accuracy compares mu with 0.5, as
        the evaluate kernel compares a member's output (Keras' binary_accuracy), whatever the head."""
        self._ensure_built(x)
        self._check_loss()
        X1 = self._to_dev(x, torch.float32).reshape(1, -1, self._input_dim)
        zv = np.asarray(y).reshape(-1)
        z1 = self._to_dev(zv, torch.float32).reshape(1, X1.shape[1])
        w = resolve_sample_weight(X1.shape[1], None, sample_weight, None)
        W = None if w is None else self._replicated(torch.from_numpy(w).to(self.theta.device).reshape(1, -1))
        loss, _ = ops.mlp_evaluate(self._desc, self.theta, self._replicated(X1), self._replicated(z1), sample_weight=W)
        mean_loss = float(loss.mean())
        if not self._metrics:
            return mean_loss
        mu = self.predict(x)[:, 0]
        return [mean_loss, float(np.mean((mu > 0.5) == (zv.astype(np.float32) > 0.5)))]

    def _member(self, member):
        if isinstance(member, bool) or int(member) != member or not 0 <= int(member) < self.members:
            raise ValueError(f"member must be in 0..{self.members - 1}, got {member!r}")
        return int(member)

    def get_weights(self, member=0):
        """Keras-order weights of one member."""
        k = self._member(member)
        if not self.built:
            raise RuntimeError("model is not built yet")
        return self._unpack(self.theta[k].cpu().numpy())

    def set_weights(self, weights, member=0):
        k = self._member(member)
        if not self.built:
            self.build(np.shape(weights[0])[0])
        cur = self.get_weights(k)
        if len(weights) != len(cur) or any(np.shape(a) != b.shape for a, b in zip(weights, cur)):
            raise ValueError("weight shapes do not match the model")
        flat = np.concatenate([np.asarray(w, dtype=np.float32).reshape(-1) for w in weights])
        self.theta[k].copy_(torch.from_numpy(flat))

    def get_optimizer_state(self, member=0):
        k = self._member(member)
        return (self.adam_m[k].cpu().numpy(), self.adam_v[k].cpu().numpy(), int(self.adam_t[k]))

    def set_optimizer_state(self, m, v, t, member=0):
        k = self._member(member)
        self.adam_m[k].copy_(torch.from_numpy(np.asarray(m, dtype=np.float32)).reshape(-1))
        self.adam_v[k].copy_(torch.from_numpy(np.asarray(v, dtype=np.float32)).reshape(-1))
        self.adam_t[k] = int(t)


class EnsembleDenseSequential(EnsembleSequential):
    """``DenseSequential``'s stack (its ``num_layers + 1`` hidden layers included) as an ensemble."""

    def __init__(self, input_dim, output_dim, num_layers, num_units, layer_kws={}, final_layer_kws={}, **kwargs):
        super(EnsembleDenseSequential, self).__init__(**kwargs)
        for i in range(num_layers):
            if not i:
                self.add(Dense(num_units, input_dim=input_dim, **layer_kws))
            self.add(Dense(num_units, **layer_kws))
        self.add(Dense(output_dim, **final_layer_kws))
        if self._input_dim is None:       # num_layers == 0
            self._input_dim = int(input_dim)


class _MaximizableEnsembleMixin(MaximizableMixin):
    """``maxima`` / ``argmax`` over an ensemble: the objective is T(-s), s = mu + beta sigma.  The device route runs the
    ensemble kernels (``ops.ensemble_screen_topk``, ``ops.ensemble_lbfgsb_minimize``); ``restart_mode="lockstep"`` /
    ``"sequential"``, other SciPy methods, ``num_starts=0`` and callable transforms run on the host through
    ``ensemble.ensemble_score``, the members' f and g from ONE ``ops.mlp_value_and_input_grad`` launch with
    ``n_models = K``.  What the ensemble kernels refuse (K images too large for LDS, more than 64 inputs) takes that
    lock-step route with a ``RuntimeWarning``."""

    def _device_ops(self):
        beta = self.beta

        def screen(desc, theta, X_init, num_starts, want_pred=False):
            return ops.ensemble_screen_topk(desc, theta[None], X_init, num_starts, beta, want_score=want_pred)

        def restarts(desc, theta, x0, low, high, transform="identity", negate=True, **options):
            return ops.ensemble_lbfgsb_minimize(desc, theta[None], x0, low, high, beta, transform, negate, **options)

        return screen, restarts

    def _streamed(self, x=None):
        return False          # (refused at build)

    def _screen_values(self, X_init):
        """The NEGATED score -s of the candidates on the host (no transform: T is monotone)."""
        return -self.predict_score(X_init).squeeze(axis=-1)

    def _value_and_input_grad(self, X, transform, negate):
        """The hook base.convert takes: X [1, R, D] f64 device -> (val [1, R] f32, grad [1, R, D] f64), the host
        statement over the members' f and g."""
        from .ensemble import ensemble_score
        f, g = ops.mlp_value_and_input_grad(self._desc, self.theta, self._replicated(X), "identity", False)
        val, grad = ensemble_score(f.cpu().numpy(), g.cpu().numpy(), self.beta, transform, negate)
        return torch.from_numpy(val.astype(np.float32)[None]), torch.from_numpy(np.ascontiguousarray(grad)[None])


class MaximizableEnsembleSequential(_MaximizableEnsembleMixin, EnsembleSequential):
    """``MaximizableSequential(transform, ...)`` over ``members`` classifiers: ``MaximizableEnsembleSequential(transform,
    members=K, beta=1.0, seed=...)``."""


class MaximizableEnsembleDenseSequential(_MaximizableEnsembleMixin, EnsembleDenseSequential):
    """``MaximizableDenseSequential``'s constructor arguments plus ``members`` and ``beta``."""


class LSTMCell:
    """``tensorflow.keras.layers.LSTMCell(units, activation="tanh", kernel_regularizer=None,
    bias_regularizer=None)``: a record of the arguments StackedRecurrentFactory passes.  The other
    Keras defaults hold and are not settable here: recurrent activation the logistic sigmoid (TF 2.x),
    glorot_uniform kernel, orthogonal recurrent kernel, zero bias with the forget block at one."""

    def __init__(self, units, activation="tanh", kernel_regularizer=None, bias_regularizer=None, **kwargs):
        from .layers import ACTIVATIONS, _reg_factor
        if kwargs:
            raise NotImplementedError(f"LSTMCell arguments {sorted(kwargs)} are not available on the HIP path")
        if callable(activation) and hasattr(activation, "__name__"):
            activation = activation.__name__
        activation = "linear" if activation is None else activation
        if activation not in ACTIVATIONS:
            raise ValueError(f"activation {activation!r} is not supported on the HIP path (supported: {ACTIVATIONS})")
        self.units = int(units)
        self.activation = activation
        self.l2_kernel = _reg_factor(kernel_regularizer)
        self.l2_bias = _reg_factor(bias_regularizer)


def _orthogonal(rs, rows, cols):
    """Keras ``Orthogonal(gain=1)`` for a (rows, cols) kernel: QR of a standard normal draw of the taller
    shape, columns signed by diag(R), transposed back when wide."""
    a = rs.normal(0.0, 1.0, size=(max(rows, cols), min(rows, cols)))
    q, r = np.linalg.qr(a)
    q = q * np.sign(np.diag(r))
    return (q.T if rows < cols else q).astype(np.float32)


class StackedRecurrentFactory:
    """bore/models.py:48-104 on MI355X.  ``num_layers`` LSTM cells and a Dense head whose parameters the
    factory owns on the device (``theta``, one packed fp32 vector in get_weights() order); the
    networks it builds read the LIVE parameters, so training the many-to-many network changes every
    one-to-one network, also those built earlier.  ``seed`` (an extension) seeds the initialisation
    and the shuffles."""

    def __init__(self, input_dim, output_dim, num_layers=2, num_units=32, layer_kws={}, final_layer_kws={},
                 seed=None):
        self.input_dim = input_dim
        assert "return_sequences" not in layer_kws
        assert "activation" not in final_layer_kws
        self.cells = [LSTMCell(num_units, **layer_kws) for _ in range(num_layers)]
        self.final_layer = Dense(output_dim, **final_layer_kws)
        self.output_dim = int(output_dim)
        self.num_layers, self.num_units = int(num_layers), int(num_units)
        self._rs = np.random.RandomState(seed)
        self._shuffle_seed = int(self._rs.randint(0, 2**31 - 1)) if seed is None else int(seed)
        cell = self.cells[0] if self.cells else LSTMCell(num_units)
        self._desc = _lib.make_lstm_desc(
            input_dim, num_layers, num_units, cell.activation,
            [c.l2_kernel for c in self.cells] + [self.final_layer.l2_kernel],
            [c.l2_bias for c in self.cells] + [self.final_layer.l2_bias], output_dim=output_dim)
        self.theta = None

    def count_params(self):
        D, H, n = int(self.input_dim), self.num_units, 0
        for l in range(self.num_layers):
            n += ((H if l else D) + H + 1) * 4 * H
        return n + (H + 1) * self.output_dim

    def _initial_weights(self):
        D, H = int(self.input_dim), self.num_units
        ws = []
        for l in range(self.num_layers):
            fan_in = H if l else D
            limit = np.sqrt(6.0 / (fan_in + 4 * H))
            ws.append(self._rs.uniform(-limit, limit, size=(fan_in, 4 * H)).astype(np.float32))
            ws.append(_orthogonal(self._rs, H, 4 * H))
            b = np.zeros(4 * H, dtype=np.float32)
            b[H:2 * H] = 1.0                      # unit_forget_bias=True
            ws.append(b)
        limit = np.sqrt(6.0 / (H + self.output_dim))
        ws.append(self._rs.uniform(-limit, limit, size=(H, self.output_dim)).astype(np.float32))
        ws.append(np.zeros(self.output_dim, dtype=np.float32))
        return ws

    def _ensure_built(self, x=None):
        if x is not None and np.shape(x)[-1] != self.input_dim:
            raise ValueError(f"expected input dimension {self.input_dim}, got {np.shape(x)[-1]}")
        if self.theta is None:
            dev = _lib.require_gpu()
            flat = np.concatenate([w.reshape(-1) for w in self._initial_weights()])
            assert flat.size == self.count_params()
            self.theta = torch.from_numpy(flat).to(dev).reshape(1, -1).contiguous()

    def get_weights(self):
        self._ensure_built()
        flat = self.theta[0].cpu().numpy()
        D, H, out, off = int(self.input_dim), self.num_units, [], 0
        shapes = []
        for l in range(self.num_layers):
            shapes += [((H if l else D), 4 * H), (H, 4 * H), (4 * H,)]
        shapes += [(H, self.output_dim), (self.output_dim,)]
        for shp in shapes:
            n = int(np.prod(shp))
            out.append(flat[off:off + n].reshape(shp).copy())
            off += n
        return out

    def set_weights(self, weights):
        cur = self.get_weights()
        if len(weights) != len(cur) or any(np.shape(a) != b.shape for a, b in zip(weights, cur)):
            raise ValueError("weight shapes do not match the model")
        flat = np.concatenate([np.asarray(w, dtype=np.float32).reshape(-1) for w in weights])
        self.theta.copy_(torch.from_numpy(flat).reshape(1, -1))

    def build_many_to_many(self, mask_value=1e+9):
        """Masking -> RNN(cell, return_sequences=True) x L -> TimeDistributed(Dense): [n, T, D] -> [n, T, 1]
        logits, for fit / evaluate."""
        return ManyToManyNetwork(self, mask_value)

    def build_one_to_one(self, num_steps, transform=None, acquisition="lockstep"):
        """RepeatVector(num_steps) -> RNN x L (the last without sequences) -> Dense: [n, D] -> [n, 1], a
        maximizable network (predict / maxima / argmax).  ``acquisition`` (an extension): "lockstep" (default) --
        screening through ``predict`` and the restarts as SciPy's state machines on the host; "device" -- both on the
        device (``MaximizableOneToOneNetwork``: restart_mode = screen_mode = "device")."""
        if acquisition not in ("lockstep", "device"):
            raise ValueError(f"acquisition must be 'lockstep' or 'device', got {acquisition!r}")
        net = MaximizableOneToOneNetwork(transform, self, num_steps)
        if acquisition == "device":
            net.restart_mode = net.screen_mode = "device"
        return net


class _RecurrentNetwork:
    """What both networks share: the factory's live parameters."""

    def __init__(self, factory):
        self.factory = factory

    @property
    def theta(self):
        self.factory._ensure_built()
        return self.factory.theta

    @property
    def _desc(self):
        return self.factory._desc

    @property
    def _input_dim(self):
        return self.factory.input_dim

    def _ensure_built(self, x=None):
        self.factory._ensure_built(x)

    def _op(self, name, T):
        """``ops.lstm_<name>`` when the LDS kernels take this network over ``T`` steps, else ``ops.lstm_stream_<name>``
        (``ops.lstm_streamed``; a network neither takes raises there).  A function of (descriptor, T) alone, so the
        training network and a one-to-one network of the same T are always served by the same flavour."""
        return getattr(ops, ("lstm_stream_" if ops.lstm_streamed(self._desc, T) else "lstm_") + name)

    def get_weights(self):
        return self.factory.get_weights()

    def set_weights(self, weights):
        self.factory.set_weights(weights)

    def count_params(self):
        return self.factory.count_params()

    def summary(self, print_fn=print):
        f = self.factory
        print_fn(f'Model: "{self.name}"')
        for i, c in enumerate(f.cells):
            n = ((f.num_units if i else f.input_dim) + f.num_units + 1) * 4 * f.num_units
            print_fn(f" rnn_{i} (RNN/LSTMCell)  units {c.units}  activation {c.activation}  params {n}")
        print_fn(f" dense (Dense)  output {f.output_dim}  params {(f.num_units + 1) * f.output_dim}")
        print_fn(f"Total params: {f.count_params()}")


class ManyToManyNetwork(_RecurrentNetwork):
    """The training network of the factory (bore/models.py:64-82).  The Adam slots and counter belong to
    this network (its compiled optimizer) and persist across ``fit`` calls."""

    name = "many_to_many"

    def __init__(self, factory, mask_value=1e9):
        super().__init__(factory)
        self.mask_value = float(mask_value)
        self._optimizer, self._loss, self._metrics, self._compiled = Adam(), None, [], False
        self.adam_m = self.adam_v = self.adam_t = None
        self._epochs_seen = 0

    def compile(self, optimizer="adam", loss=None, metrics=None, **kwargs):
        self._optimizer = resolve_optimizer(optimizer)
        self._loss = resolve_loss(loss)
        self._metrics = list(metrics or [])
        for m in self._metrics:
            if m not in ("accuracy", "acc", "binary_accuracy"):
                raise NotImplementedError(f"metric {m!r} is not available on the HIP path")
        if self._loss is not None and not self._loss.from_logits:
            raise NotImplementedError("the recurrent classifier's head is linear: compile with "
                                      "BinaryCrossentropy(from_logits=True)")
        self._compiled = True

    def _check_loss(self):
        if not self._compiled or self._loss is None:
            raise RuntimeError("compile(optimizer=..., loss=...) the model before fit/evaluate")

    def _data(self, x, y=None):
        x = np.asarray(x, dtype=np.float32)
        if x.ndim != 3:
            raise ValueError(f"expected input sequences [n, T, D], got shape {x.shape}")
        self._ensure_built(x)
        n, T = x.shape[:2]
        if T > _lib.LSTM_MAX_STEPS:
            raise _lib.UnsupportedError(f"{T} steps > {_lib.LSTM_MAX_STEPS} (BORE_LSTM_MAX_STEPS)")
        dev = self.theta.device
        X = torch.from_numpy(np.ascontiguousarray(x)).to(dev).reshape(1, n, T, -1)
        if y is None:
            return X, None
        yv = np.asarray(y, dtype=np.float32).reshape(n, T)
        return X, torch.from_numpy(np.ascontiguousarray(yv)).to(dev).reshape(1, n, T)

    def _perm(self, epochs, N, shuffle, perm):
        dev = self.theta.device
        if perm is None and not shuffle:
            perm = np.tile(np.arange(N, dtype=np.int32), (epochs, 1))
        if perm is not None:
            perm = np.asarray(perm)
            if perm.shape != (epochs, N) or not np.array_equal(np.sort(perm, axis=1),
                                                               np.tile(np.arange(N), (epochs, 1))):
                raise ValueError("perm must hold one permutation of range(N) per epoch")
            return torch.from_numpy(np.ascontiguousarray(perm, dtype=np.int32)).to(dev).reshape(1, epochs, N)
        try:      # the shuffle stream of the Dense fit, drawn on the device
            return ops.shuffle_perm(self.factory._shuffle_seed, 1, epochs, N, epoch0=self._epochs_seen, device=dev)
        except _lib.UnsupportedError:          # (its host statement: the same permutations)
            p = _shuffle.permutations(self.factory._shuffle_seed, 1, epochs, N, epoch0=self._epochs_seen)
            return torch.from_numpy(p).to(dev)

    @staticmethod
    def _refuse_weights(**given):
        """The recurrent kernels take no row weights: refused by name instead of dropped."""
        names = [k for k, v in given.items() if v is not None]
        if names:
            raise _lib.UnsupportedError(f"{' / '.join(names)}: the recurrent classifier's kernels take no sample "
                                        "weights (weighted fits: the Dense models)")

    def fit(self, x, y, epochs=1, batch_size=None, callbacks=None, verbose=False, shuffle=True, perm=None,
            sample_weight=None, class_weight=None, **kwargs):
        """Keras ``fit`` over sequences (``perm`` (epochs, N): explicit shuffles, an extension).  Returns a
        ``History``; one launch for all epochs, or one per epoch when callbacks are given.  ``sample_weight`` and
        ``class_weight`` raise ``UnsupportedError``."""
        self._refuse_weights(sample_weight=sample_weight, class_weight=class_weight)
        self._check_loss()
        X, y = self._data(x, y)
        N = X.shape[1]
        batch_size = 32 if batch_size is None else int(batch_size)
        if batch_size < 1:
            raise ValueError(f"batch_size must be positive, got {batch_size}")
        epochs = int(epochs)
        if self.adam_m is None:
            self.adam_m = torch.zeros_like(self.theta)
            self.adam_v = torch.zeros_like(self.theta)
            self.adam_t = torch.zeros(1, dtype=torch.int64, device=self.theta.device)
        P = self._perm(epochs, N, shuffle, perm)
        o = self._optimizer
        fit_op = self._op("fit", X.shape[2])

        def launch(e0, n):
            loss = fit_op(self._desc, self.theta, self.adam_m, self.adam_v, self.adam_t, X, y, n, batch_size,
                                P[:, e0:e0 + n].contiguous(), mask_value=self.mask_value, lr=o.learning_rate,
                                beta1=o.beta_1, beta2=o.beta_2, eps=o.epsilon)
            self._epochs_seen += n
            return loss

        callbacks = list(callbacks or [])
        if not callbacks:
            loss = launch(0, epochs)
            if verbose:
                for e, v in enumerate(loss[0].cpu().numpy()):
                    print(f"Epoch {e + 1}/{epochs} - loss: {float(v):.4f}")
            return History(lambda: loss[0].cpu().numpy())

        def call(name, *args):
            for cb in callbacks:
                fn = getattr(cb, name, None)
                if fn is not None:
                    fn(*args)

        self.stop_training = False
        call("set_model", self)
        call("on_train_begin", {})
        losses = []
        for e in range(epochs):
            call("on_epoch_begin", e, {})
            losses.append(float(launch(e, 1)[0].cpu().numpy()[0]))
            call("on_epoch_end", e, {"loss": losses[-1]})
            if self.stop_training:
                break
        call("on_train_end", {})
        return History(np.asarray(losses, dtype=np.float32))

    def evaluate(self, x, y, batch_size=None, verbose=False, sample_weight=None, **kwargs):
        """[loss, accuracy] (loss alone without metrics) under the masking rules of bore_lstm_evaluate.
        ``sample_weight`` raises ``UnsupportedError``."""
        self._refuse_weights(sample_weight=sample_weight)
        self._check_loss()
        X, y = self._data(x, y)
        loss, acc = self._op("evaluate", X.shape[2])(self._desc, self.theta, X, y, mask_value=self.mask_value)
        if self._metrics:
            return [float(loss[0]), float(acc[0])]
        return float(loss[0])

    def predict(self, x, batch_size=None, verbose=0, **kwargs):
        """[n, T, D] -> (n, T, 1) float32 logits."""
        X, _ = self._data(x)
        out = self._op("forward", X.shape[2])(self._desc, self.theta, X, mask_value=self.mask_value)
        return out[0].cpu().numpy()[..., None]

    def __call__(self, x, training=False):
        return self.predict(x)

    def get_optimizer_state(self):
        """(m, v, t): Adam slots in get_weights() order + iteration counter."""
        return (self.adam_m[0].cpu().numpy(), self.adam_v[0].cpu().numpy(), int(self.adam_t[0]))


class OneToOneNetwork(_RecurrentNetwork):
    """The prediction network of the factory (bore/models.py:84-104)."""

    name = "one_to_one"

    def __init__(self, factory, num_steps):
        super().__init__(factory)
        self.num_steps = int(num_steps)
        if not 1 <= self.num_steps <= _lib.LSTM_MAX_STEPS:
            raise _lib.UnsupportedError(f"num_steps {num_steps} outside 1..{_lib.LSTM_MAX_STEPS} "
                                        "(BORE_LSTM_MAX_STEPS)")

    def predict(self, x, batch_size=None, verbose=0, **kwargs):
        """(n, D) -> (n, 1) float32."""
        x = np.asarray(x, dtype=np.float32).reshape(-1, int(self.factory.input_dim))
        self._ensure_built(x)
        X = torch.from_numpy(np.ascontiguousarray(x)).to(self.theta.device).reshape(1, x.shape[0], -1)
        out = self._op("forward", self.num_steps)(self._desc, self.theta, X, num_steps=self.num_steps)
        return out[0].cpu().numpy().reshape(-1, 1)

    def __call__(self, x, training=False):
        return self.predict(x)

    def _value_and_input_grad(self, X, transform, negate):
        """The hook base.convert takes for this network: X [1, R, D] f64 device."""
        return self._op("value_and_input_grad", self.num_steps)(self._desc, self.theta, X, self.num_steps, transform,
                                                                negate)


class MaximizableOneToOneNetwork(MaximizableMixin, OneToOneNetwork):
    """``MaximizableSequential(transform=...)`` of the one-to-one form: screening through
    bore_lstm_forward and argpartition on the host, the restarts as SciPy's L-BFGS-B state machines
    advanced together with one bore_lstm_value_and_input_grad launch per round (the bore_lstm_stream_* twins for a
    network the LDS kernels refuse: ``_RecurrentNetwork._op``).

    OPT-IN, ``restart_mode = screen_mode = "device"`` (``build_one_to_one(acquisition="device")``): screening and
    every restart's L-BFGS-B on the device, two calls per ``maxima`` (bore_lstm_stream_screen_topk,
    bore_lstm_stream_lbfgsb_minimize; up to 64 input dimensions and 16 384 candidates).  Those are the STREAMED
    kernels for every network, so a network that fits LDS is optimised on another f/g flavour than ``predict``'s
    (equal to float32 rounding, not bit for bit) -- one reason the class defaults stay what they were.  What the
    kernels refuse, a callable transform and a method other than L-BFGS-B take the default route with a
    ``RuntimeWarning`` that names the reason: the caller asked for the device."""

    restart_mode = "lockstep"
    screen_mode = "host"

    def _device_ops(self):
        T = self.num_steps

        def screen(desc, theta, X_init, num_starts, want_pred=False):
            return ops.lstm_stream_screen_topk(desc, theta, X_init, num_starts, T, want_pred=want_pred)

        def restarts(desc, theta, x0, low, high, transform="identity", negate=True, **options):
            return ops.lstm_stream_lbfgsb_minimize(desc, theta, x0, low, high, T, transform, negate, **options)

        return screen, restarts

    def _screening_refused(self, error):
        warnings.warn(f"screen_mode='device' cannot take this request ({error}); screening through predict and "
                      "argpartition on the host instead", RuntimeWarning, stacklevel=3)

    def _minimize_from(self, X0, bounds, method, options):
        if method != "L-BFGS-B" and self.restart_mode == "device":
            warnings.warn(f"restart_mode='device' runs L-BFGS-B only (got method={method!r}); running "
                          "scipy.optimize.minimize on the host around the f/g kernel instead", RuntimeWarning,
                          stacklevel=3)
        return super()._minimize_from(X0, bounds, method, options)


__all__ = ["Sequential", "DenseSequential", "Model", "MaximizableModel", "MaximizableSequential",
           "MaximizableDenseSequential", "BatchMaximizableModel", "BatchMaximizableSequential",
           "BatchMaximizableDenseSequential", "EnsembleSequential", "EnsembleDenseSequential",
           "MaximizableEnsembleSequential", "MaximizableEnsembleDenseSequential", "Dense", "BinaryCrossentropy", "Adam", "History",
           "LSTMCell", "StackedRecurrentFactory", "ManyToManyNetwork", "OneToOneNetwork",
           "MaximizableOneToOneNetwork"]
