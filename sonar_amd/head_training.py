"""Training of MLP heads over frozen SONAR embeddings, on the MI355X engine.

The recipe is part 4 of the reference's `examples/finetune_sonar_as_toxicity_classifier.ipynb` ("it would be much faster to
tokenize all the data in advance, and then to train only the head, feeding the embeddings directly to it"): an MLP head
on precomputed embeddings, AdamW with decoupled weight decay, warm-up and linear decay, gradient clipping.  MuTox
(`mutox/factory.py:15-38`, BCE with logits) and BLASER (`blaser/model.py:63-80`, MSE) are the same kind of head, and a
trained head is handed to `sonar_amd.heads` through `state_dict(layout)`.

Everything numerical runs in `libsonar_mi355.so` (`smi_head_trainer_*`, csrc/head_train.hip); there is no CPU path.  The
model and the optimizer have the semantics of `torch.nn` / `torch.optim.AdamW`; the storage contract (fp32 masters, fp16
shadow weights and activations, bf16 backward operands) is DESIGN.md 3.16.  The learning-rate schedule is computed here,
on the host, and passed per step.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, List, Optional, Sequence, Tuple, Union

import torch

from . import _lib
from .heads import ACTIVATIONS, BLASER_INPUT_FORMS, BlaserConfig

LOSSES = {"ce": 0, "bce": 1, "mse": 2}
SCHEDULES = ("constant", "linear")
LAYOUTS = ("mutox", "blaser", "classifier")


def schedule_factor(t: int, warmup: int, total: Optional[int], schedule: str) -> float:
    """Learning-rate factor of step t (counted from 1): `constant` is 1; `linear` is t/warmup for t <= warmup, then a linear
    decay that reaches 0 at step `total` (no decay while `total` is unknown)."""
    if schedule == "constant":
        return 1.0
    if t <= warmup:
        return t / warmup
    if total is None or total <= warmup:
        return 1.0
    return max(0.0, (total - t) / (total - warmup))


def blaser_linear_indices(n_hidden: int, dropout: float) -> List[int]:
    """Positions of the Linear modules in the `mlp` Sequential of blaser/model.py:63-80."""
    if n_hidden == 0:
        return [0]
    if dropout > 0:
        return [1 + 3 * i for i in range(n_hidden + 1)]
    return [2 * i for i in range(n_hidden + 1)]


def state_dict_keys(layout: str, n_layers: int, dropout: float = 0.0) -> List[str]:
    """Key prefixes (without `.weight` / `.bias`) of the n_layers Linear layers in a reference layout."""
    if layout == "mutox":
        if n_layers != 3:
            raise ValueError(f"the mutox layout has 3 Linear layers, this head has {n_layers}")
        return [f"model_all.{i}.1" for i in range(3)]
    if layout == "blaser":
        return [f"mlp.{i}" for i in blaser_linear_indices(n_layers - 1, dropout)]
    if layout == "classifier":
        if n_layers != 2:
            raise ValueError(f"the classifier layout is fc1 + classifier, this head has {n_layers} Linear layers")
        return ["fc1", "classifier"]
    raise ValueError(f"unknown layout {layout!r} {LAYOUTS}")


def default_init(dims: Sequence[int], seed: int) -> List[Tuple[torch.Tensor, torch.Tensor]]:
    """nn.Linear's default initialisation (uniform in +-1/sqrt(fan_in) for weight and bias), drawn on the host from a
    seeded generator."""
    g = torch.Generator().manual_seed(int(seed))
    layers = []
    for fan_in, fan_out in zip(dims[:-1], dims[1:]):
        bound = 1.0 / math.sqrt(fan_in)
        w = (torch.rand((fan_out, fan_in), generator=g) * 2 - 1) * bound
        b = (torch.rand((fan_out,), generator=g) * 2 - 1) * bound
        layers.append((w, b))
    return layers


def _validate(d_in, hidden_dims, out_dim, activation, loss, p_in, p_hidden, lr, weight_decay, warmup_steps, schedule,
              max_grad_norm, max_batch) -> None:
    if activation not in ACTIVATIONS:
        raise ValueError(f"unrecognized activation {activation!r} (TANH, RELU)")
    if loss not in LOSSES:
        raise ValueError(f"unrecognized loss {loss!r} (ce, bce, mse)")
    if schedule not in SCHEDULES:
        raise ValueError(f"unrecognized schedule {schedule!r} {SCHEDULES}")
    if d_in <= 0 or d_in % 64:
        raise ValueError(f"d_in {d_in} must be a positive multiple of 64")
    if len(hidden_dims) > 7:
        raise ValueError("at most 7 hidden layers")
    for h in hidden_dims:
        if h <= 0 or h % 128:
            raise ValueError(f"hidden width {h} must be a positive multiple of 128")
    if not 1 <= out_dim <= 8:
        raise ValueError(f"out_dim {out_dim} must be in 1..8")
    if loss == "ce" and out_dim < 2:
        raise ValueError("cross-entropy needs out_dim >= 2")
    for name, p in (("p_in", p_in), ("p_hidden", p_hidden)):
        if not 0.0 <= p < 1.0:
            raise ValueError(f"{name} {p} must be in [0, 1)")
    if not lr >= 0 or not weight_decay >= 0:
        raise ValueError("lr and weight_decay must be >= 0")
    if warmup_steps < 0:
        raise ValueError("warmup_steps must be >= 0")
    if max_grad_norm is not None and not max_grad_norm > 0:
        raise ValueError("max_grad_norm must be > 0 or None")
    if max_batch < 1:
        raise ValueError("max_batch must be >= 1")


class HeadTrainer:
    """An MLP head `[d_in, *hidden_dims, out_dim]` and its AdamW state on the device.

    activation: "TANH" / "RELU" after every hidden layer.  loss: "ce" (int labels, softmax cross-entropy, mean over rows),
    "bce" (float targets [rows, out], binary cross-entropy with logits, mean over all elements) or "mse".  p_in / p_hidden:
    dropout on the input / after every hidden activation.  schedule: "constant" or "linear" (warm-up `warmup_steps`, then
    linear decay to 0 at the last step of `fit`).  max_grad_norm: global-norm clipping, None = off.  seed: of the default
    initialisation, the epoch permutations and the dropout masks -- one seed, one run, bit for bit.  init: optional list of
    (weight [out, in], bias [out]) per Linear layer.  max_batch: the largest batch `fit` / `step` will see.
    """

    def __init__(self, d_in: int, hidden_dims: Sequence[int], out_dim: int, activation: str = "TANH", loss: str = "ce",
                 p_in: float = 0.0, p_hidden: float = 0.0, lr: float = 1e-4, weight_decay: float = 1e-3,
                 warmup_steps: int = 0, schedule: str = "linear", max_grad_norm: Optional[float] = 1.0, seed: int = 0,
                 device: Union[str, torch.device] = "cuda:0", init=None, max_batch: int = 512,
                 betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8):
        hidden_dims = [int(h) for h in hidden_dims]
        _validate(d_in, hidden_dims, out_dim, activation, loss, p_in, p_hidden, lr, weight_decay, warmup_steps, schedule,
                  max_grad_norm, max_batch)
        self.dims = [int(d_in), *hidden_dims, int(out_dim)]
        self.activation, self.loss = activation, loss
        self.p_in, self.p_hidden = float(p_in), float(p_hidden)
        self.lr, self.weight_decay = float(lr), float(weight_decay)
        self.warmup_steps, self.schedule, self.max_grad_norm = int(warmup_steps), schedule, max_grad_norm
        self.seed, self.max_batch, self.betas, self.eps = int(seed), int(max_batch), betas, float(eps)
        self.total_steps: Optional[int] = None
        self.blaser_config: Optional[BlaserConfig] = None
        self._t = 0
        self._handle = None
        n = len(self.dims) - 1
        layers = default_init(self.dims, self.seed) if init is None else [(w, b) for w, b in init]
        if len(layers) != n:
            raise ValueError(f"init has {len(layers)} layers, the head has {n}")
        for i, (w, b) in enumerate(layers):
            if tuple(w.shape) != (self.dims[i + 1], self.dims[i]) or tuple(b.shape) != (self.dims[i + 1],):
                raise ValueError(f"init layer {i}: weight {tuple(w.shape)} / bias {tuple(b.shape)} do not fit "
                                 f"{self.dims[i]} -> {self.dims[i + 1]}")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("the MI355X SONAR engine needs device='cuda[:i]' (no CPU path)")
        if not torch.cuda.is_available():
            raise RuntimeError("no HIP device visible: head training runs on the MI355X only (no CPU path)")
        self.lib = _lib.load()
        idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self.device = torch.device("cuda", idx)
        self._perm_gen = torch.Generator().manual_seed(self.seed + 1)
        arr = (_lib.smi_mlp_head_layer * n)()
        keep: list = []
        for i, (w, b) in enumerate(layers):
            for t, slot in ((w, "w"), (b, "b")):
                t = t.detach().float().contiguous()
                keep.append(t)
                setattr(arr[i], slot, _lib.smi_tensor(t.data_ptr(), _lib.SMI_F32, int(t.is_cuda), t.numel()))
            arr[i].out_dim = self.dims[i + 1]
        cfg = _lib.smi_head_trainer_config(
            input_dim=self.dims[0], n_layers=n, hidden_act=ACTIVATIONS[activation], loss=LOSSES[loss],
            max_batch=self.max_batch, reserved=0, p_in=self.p_in, p_hidden=self.p_hidden,
            seed=self.seed & (2 ** 64 - 1), beta1=betas[0], beta2=betas[1], eps=self.eps, weight_decay=self.weight_decay)
        handle = C.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(self.lib.smi_init(self.device.index))
            _lib.check(self.lib.smi_head_trainer_create(C.byref(cfg), arr, C.byref(handle)))
        self._handle = handle

    def __del__(self):
        h = getattr(self, "_handle", None)
        if h:
            self.lib.smi_head_trainer_destroy(h)
            self._handle = None

    # ---- constructors of the reference's heads ----
    @classmethod
    def for_mutox(cls, input_size: int = 1024, **kw) -> "HeadTrainer":
        """mutox/factory.py:15-38: Dropout(0.01) - Linear(input_size, 512) - ReLU - Linear(512, 128) - ReLU - Linear(128, 1),
        trained with BCE with logits."""
        kw.setdefault("p_in", 0.01)
        return cls(input_size, [512, 128], 1, activation="RELU", loss="bce", **kw)

    @classmethod
    def for_blaser(cls, config: BlaserConfig, **kw) -> "HeadTrainer":
        """blaser/model.py:63-80 for a BlaserConfig: the MLP over the 6 (COMET) or 4 (QE) feature blocks, `dropout` on the
        input and after every hidden activation, MSE against the human scores."""
        if config.input_form not in BLASER_INPUT_FORMS:
            raise ValueError(f"Unrecognized input format: {config.input_form}")
        if config.output_act:
            raise ValueError("training through BLASER's output Tanh (output_act=True) is not supported")
        if any(h <= 0 for h in config.hidden_dims):   # the reference skips them but keeps its leading Dropout: other keys
            raise ValueError(f"hidden_dims {list(config.hidden_dims)}: zero or negative widths are not supported")
        hidden = list(config.hidden_dims)
        p = float(config.dropout) if hidden else 0.0
        kw.setdefault("p_in", p)
        kw.setdefault("p_hidden", p)
        width = config.embedding_dim * (6 if config.input_form == "COMET" else 4)
        t = cls(width, hidden, config.output_dim, activation=config.activation, loss="mse", **kw)
        t.blaser_config = config
        return t

    @classmethod
    def for_classifier(cls, d_in: int = 1024, hidden: int = 8192, n_classes: int = 2, **kw) -> "HeadTrainer":
        """The head of the fine-tuning notebook: Linear(d_in, hidden) - Tanh - Dropout - Linear(hidden, n_classes) with
        cross-entropy.  The declared Tanh IS applied here; the notebook's own `forward` declares it and then skips it
        (it calls fc1, dropout, classifier), so a head trained there is a different function of the embedding."""
        kw.setdefault("activation", "TANH")
        return cls(d_in, [hidden], n_classes, loss="ce", **kw)

    # ---- helpers ----
    def _lr_at(self, t: int) -> float:
        return self.lr * schedule_factor(t, self.warmup_steps, self.total_steps, self.schedule)

    def _inputs(self, X: torch.Tensor) -> torch.Tensor:
        if X.dim() != 2 or X.shape[1] != self.dims[0]:
            raise ValueError(f"inputs must be [rows, {self.dims[0]}], got {tuple(X.shape)}")
        if X.dtype not in (torch.float16, torch.float32):
            X = X.float()
        return X.to(self.device).contiguous()

    def _targets(self, y: torch.Tensor, rows: int) -> torch.Tensor:
        out = self.dims[-1]
        if self.loss == "ce":
            if y.dim() != 1 or y.shape[0] != rows or y.dtype.is_floating_point:
                raise ValueError(f"cross-entropy labels must be integers of shape [{rows}]")
            if rows and (int(y.min()) < 0 or int(y.max()) >= out):
                raise ValueError(f"labels must be in 0..{out - 1}")
            return y.to(self.device, torch.int32).contiguous()
        if y.dim() == 1 and out == 1:
            y = y[:, None]
        if tuple(y.shape) != (rows, out):
            raise ValueError(f"targets must be [{rows}, {out}], got {tuple(y.shape)}")
        return y.to(self.device, torch.float32).contiguous()

    def _check_rows(self, rows: int) -> None:
        if rows < 1:
            raise ValueError("an empty batch")
        if rows > self.max_batch:
            raise ValueError(f"batch of {rows} rows above max_batch {self.max_batch}")

    # ---- training ----
    def fit(self, X: torch.Tensor, y: torch.Tensor, epochs: int, batch_size: int, shuffle: bool = True) -> torch.Tensor:
        """Train for `epochs` passes over (X, y) and return the per-step losses (fp32, CPU).  X is moved to the device once;
        every epoch draws one host permutation from the seeded generator; the last short batch of an epoch is kept.  The
        whole run is enqueued without a host synchronisation and the losses are read back once at the end."""
        if epochs < 1 or batch_size < 1:
            raise ValueError("epochs and batch_size must be >= 1")
        self._check_rows(batch_size)
        X = self._inputs(X)
        n = X.shape[0]
        if n < 1:
            raise ValueError("an empty dataset")
        y = self._targets(y, n)
        per_epoch = (n + batch_size - 1) // batch_size
        first = self._t
        self.total_steps = first + epochs * per_epoch
        xdt = _lib.smi_dtype_of(X.dtype)
        clip = float(self.max_grad_norm) if self.max_grad_norm is not None else 0.0
        keep = []
        with torch.cuda.device(self.device):
            stream = _lib.current_stream_ptr()
            _lib.check(self.lib.smi_head_trainer_reserve(self._handle, epochs * per_epoch))  # the loss record, once
            for _ in range(epochs):
                perm = None
                if shuffle:
                    perm = torch.randperm(n, generator=self._perm_gen).to(self.device)
                    keep.append(perm)
                for off in range(0, n, batch_size):
                    rows = min(batch_size, n - off)
                    _lib.check(self.lib.smi_head_trainer_step(
                        self._handle, X.data_ptr(), xdt, y.data_ptr(), perm.data_ptr() if perm is not None else None, off,
                        rows, self._lr_at(self._t + 1), clip, None, stream))
                    self._t += 1
            count = self._t - first
            host = (C.c_float * count)()
            _lib.check(self.lib.smi_head_trainer_losses(self._handle, first, count, host))
        return torch.tensor(list(host), dtype=torch.float32)

    def fit_blaser(self, src: torch.Tensor, mt: torch.Tensor, ref: Optional[torch.Tensor], scores: torch.Tensor,
                   epochs: int, batch_size: int, shuffle: bool = True) -> torch.Tensor:
        """`fit` on BLASER's features of (src, mt[, ref]) embeddings, computed by the engine's smi_head_featurize."""
        return self.fit(self.blaser_features(src, mt, ref), scores, epochs, batch_size, shuffle)

    def blaser_features(self, src: torch.Tensor, mt: torch.Tensor, ref: Optional[torch.Tensor] = None) -> torch.Tensor:
        """fp16 device features [rows, blocks * d] of blaser/model.py:95-125 (a `for_blaser` trainer)."""
        cfg = self.blaser_config
        if cfg is None:
            raise RuntimeError("blaser_features needs a trainer made by HeadTrainer.for_blaser")
        comet = cfg.input_form == "COMET"
        if comet and ref is None:
            raise ValueError("With the COMET input form of BLASER, a reference embedding must be provided.")
        ts = [t for t in ((src, mt, ref) if comet else (src, mt))]
        dt = torch.float16 if all(t.dtype == torch.float16 for t in ts) else torch.float32
        ts = [t.to(self.device, dt).contiguous() for t in ts]
        rows, d = ts[0].shape
        if any(t.shape != ts[0].shape for t in ts) or d != cfg.embedding_dim:
            raise ValueError(f"src, mt and ref embeddings must all be [rows, {cfg.embedding_dim}]")
        blocks = 6 if comet else 4
        feats = torch.empty(((rows + 127) // 128 * 128, blocks * d), dtype=torch.float16, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.smi_head_featurize(2 if comet else 1, ts[0].data_ptr(), ts[1].data_ptr(),
                                                   ts[2].data_ptr() if comet else None, _lib.smi_dtype_of(dt), rows, d,
                                                   int(cfg.norm_emb), feats.data_ptr(), _lib.current_stream_ptr()))
        return feats[:rows]

    def step(self, xb: torch.Tensor, yb: torch.Tensor) -> float:
        """One optimizer step on one batch; returns its loss."""
        xb = self._inputs(xb)
        self._check_rows(xb.shape[0])
        yb = self._targets(yb, xb.shape[0])
        loss = C.c_float()
        clip = float(self.max_grad_norm) if self.max_grad_norm is not None else 0.0
        with torch.cuda.device(self.device):
            _lib.check(self.lib.smi_head_trainer_step(self._handle, xb.data_ptr(), _lib.smi_dtype_of(xb.dtype),
                                                      yb.data_ptr(), None, 0, xb.shape[0], self._lr_at(self._t + 1), clip,
                                                      C.byref(loss), _lib.current_stream_ptr()))
        self._t += 1
        return loss.value

    def gradients(self, xb: torch.Tensor, yb: torch.Tensor) -> Tuple[float, List[Tuple[torch.Tensor, torch.Tensor]]]:
        """Loss and fp32 gradients [(dW, db) per Linear layer] of one batch with the dropout masks of the next step; no
        update."""
        xb = self._inputs(xb)
        self._check_rows(xb.shape[0])
        yb = self._targets(yb, xb.shape[0])
        total = sum(a * b + b for a, b in zip(self.dims[:-1], self.dims[1:]))
        flat = torch.empty(total, dtype=torch.float32)
        loss = C.c_float()
        with torch.cuda.device(self.device):
            _lib.check(self.lib.smi_head_trainer_gradients(self._handle, xb.data_ptr(), _lib.smi_dtype_of(xb.dtype),
                                                           yb.data_ptr(), None, 0, xb.shape[0], C.byref(loss),
                                                           flat.data_ptr(), _lib.current_stream_ptr()))
        out, o = [], 0
        for a, b in zip(self.dims[:-1], self.dims[1:]):
            out.append((flat[o:o + a * b].view(b, a).clone(), flat[o + a * b:o + a * b + b].clone()))
            o += a * b + b
        return loss.value, out

    # ---- inference and hand-over ----
    @torch.inference_mode()
    def predict(self, X: torch.Tensor, output_prob: bool = False) -> torch.Tensor:
        """Logits (or their sigmoid) of the current weights, through the calls `smi_mlp_head_forward` makes: fp32 [rows, out]
        on the device."""
        X = self._inputs(X)
        rows = X.shape[0]
        out = torch.empty((rows, self.dims[-1]), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            stream = _lib.current_stream_ptr()
            for lo in range(0, rows, self.max_batch):
                r = min(self.max_batch, rows - lo)
                feats = torch.empty(((r + 127) // 128 * 128, self.dims[0]), dtype=torch.float16, device=self.device)
                xs = X[lo:lo + r]
                _lib.check(self.lib.smi_head_featurize(0, xs.data_ptr(), None, None, _lib.smi_dtype_of(xs.dtype), r,
                                                       self.dims[0], 0, feats.data_ptr(), stream))
                _lib.check(self.lib.smi_head_trainer_forward(self._handle, feats.data_ptr(), r, 2 if output_prob else 0,
                                                             out[lo:lo + r].data_ptr(), stream))
        return out

    def parameters(self) -> List[Tuple[torch.Tensor, torch.Tensor]]:
        """The fp32 master weights [(W [out, in], b [out]) per Linear layer], on the CPU."""
        out = []
        with torch.cuda.device(self.device):
            for i, (a, b) in enumerate(zip(self.dims[:-1], self.dims[1:])):
                w, bias = torch.empty((b, a), dtype=torch.float32), torch.empty((b,), dtype=torch.float32)
                _lib.check(self.lib.smi_head_trainer_export(self._handle, i, w.data_ptr(), bias.data_ptr()))
                out.append((w, bias))
        return out

    def state_dict(self, layout: str = "classifier") -> Dict[str, torch.Tensor]:
        """The master weights under the reference's key names: "mutox" (`model_all.<i>.1.*`, mutox/factory.py), "blaser"
        (`mlp.<i>.*` with the indices blaser/model.py:63-80 gives for the configured dropout) or "classifier" (`fc1.*`,
        `classifier.*`, the notebook's head)."""
        dropout = self.blaser_config.dropout if self.blaser_config is not None else max(self.p_in, self.p_hidden)
        keys = state_dict_keys(layout, len(self.dims) - 1, dropout)
        sd = {}
        for k, (w, b) in zip(keys, self.parameters()):
            sd[f"{k}.weight"], sd[f"{k}.bias"] = w, b
        return sd
