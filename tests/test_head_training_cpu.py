"""CPU: the head-training restatement (tests/head_train_ref.py) against torch.autograd + torch.optim.AdamW, the dropout
hash, the checkpoint key layouts and the Python-side refusals of sonar_amd.head_training.  No device is touched."""
import math

import numpy as np
import pytest
import torch
from torch import nn

from sonar_amd import head_training as HT
from sonar_amd.heads import BlaserConfig
from tests import head_train_ref as R


def _problem(dims, loss, rows, seed):
    g = torch.Generator().manual_seed(seed)
    X = (0.5 * torch.randn(rows, dims[0], generator=g)).double().numpy()
    if loss == "ce":
        y = torch.randint(0, dims[-1], (rows,), generator=g).numpy()
    elif loss == "bce":
        y = torch.randint(0, 2, (rows, dims[-1]), generator=g).double().numpy()
    else:
        y = torch.tanh(torch.randn(rows, dims[-1], generator=g)).double().numpy()
    return X, y


class _TorchHead(nn.Module):
    """The same function in torch, float64: hidden weights enter through their fp16 value (straight-through), which is what
    'exact arithmetic on the fp16 shadow weights' means; the output layer is plain."""

    def __init__(self, init, activation):
        super().__init__()
        self.W = nn.ParameterList([nn.Parameter(w.double().clone()) for w, _ in init])
        self.b = nn.ParameterList([nn.Parameter(b.double().clone()) for _, b in init])
        self.act = torch.tanh if activation == "TANH" else torch.relu

    def forward(self, x):
        n = len(self.W)
        for l in range(n - 1):
            W = self.W[l]
            Wq = W + (torch.from_numpy(R.f16(W.detach().numpy())) - W).detach()
            x = self.act(x @ Wq.T + self.b[l])
        return x @ self.W[n - 1].T + self.b[n - 1]


@pytest.mark.parametrize("activation", ["TANH", "RELU"])
@pytest.mark.parametrize("loss", ["ce", "bce", "mse"])
def test_exact_mode_equals_torch_autograd_adamw(loss, activation):
    """10 steps of clip(1.0) + AdamW(lr 3e-3, wd 1e-3) + linear schedule (warm-up 3).  Both sides are float64, so the bound
    is a count of operations times 2^-52, not a measured number: per step every parameter goes through at most
    K = 64 + 128 + 128 + rows accumulated products in the forward and backward pass and some 40 more scalar operations
    (loss, clipping, AdamW); 10 steps, a factor 4 for the two passes re-using rounded intermediates."""
    dims, rows, steps, warm = [64, 128, 128, 2 if loss == "ce" else 1], 24, 10, 3
    init = HT.default_init(dims, 5)
    X, y = _problem(dims, loss, rows, 11)
    ref = R.RefTrainer(dims, activation, loss, lr=3e-3, weight_decay=1e-3, warmup_steps=warm, schedule="linear",
                       max_grad_norm=1.0, init=init, mirror=False)
    ref.total_steps = steps
    model = _TorchHead(init, activation)
    opt = torch.optim.AdamW(model.parameters(), lr=3e-3, weight_decay=1e-3, betas=(0.9, 0.999), eps=1e-8)
    sched = torch.optim.lr_scheduler.LambdaLR(
        opt, lambda s: (s + 1) / warm if s + 1 <= warm else (steps - (s + 1)) / (steps - warm))
    xt = torch.from_numpy(X)
    bound = 4 * steps * (sum(dims[:-1]) + rows + 40) * 2.0 ** -52
    for _ in range(steps):
        opt.zero_grad()
        out = model(xt)
        if loss == "ce":
            L = nn.functional.cross_entropy(out, torch.from_numpy(y))
        elif loss == "bce":
            L = nn.functional.binary_cross_entropy_with_logits(out, torch.from_numpy(y))
        else:
            L = nn.functional.mse_loss(out, torch.from_numpy(y))
        L.backward()
        nn.utils.clip_grad_norm_(model.parameters(), 1.0)
        opt.step()
        sched.step()
        Lr = ref.step(X, y)
        assert abs(Lr - L.item()) <= bound * max(1.0, abs(L.item()))
    for l in range(len(dims) - 1):
        for mine, theirs in ((ref.W[l], model.W[l]), (ref.b[l], model.b[l])):
            theirs = theirs.detach().numpy()
            assert np.abs(mine - theirs).max() <= bound * max(1.0, np.abs(theirs).max())


def test_mirrored_mode_stays_near_exact_mode():
    """The storage roundings move a gradient by a few 1e-3 norm-wise, not more (fp16 activations 2^-11, bf16 operands
    2^-9 each): a mirror that drifts further has a rounding in the wrong place."""
    dims = [64, 128, 2]
    init = HT.default_init(dims, 1)
    X, y = _problem(dims, "ce", 100, 2)
    ga = R.RefTrainer(dims, "TANH", "ce", init=init, mirror=True).forward_backward(X, y, 1)[1]
    gb = R.RefTrainer(dims, "TANH", "ce", init=init, mirror=False).forward_backward(X, y, 1)[1]
    for (wa, ba), (wb, bb) in zip(ga, gb):
        assert np.linalg.norm(wa - wb) <= 3 * 2.0 ** -8 * np.linalg.norm(wb)
        assert np.linalg.norm(ba - bb) <= 3 * 2.0 ** -8 * np.linalg.norm(bb)


def test_roundings():
    assert R.bf16(1.0 + 2.0 ** -8) == 1.0 and R.bf16(1.0 + 3 * 2.0 ** -8) == 1.0 + 2.0 ** -6   # ties to even
    assert R.bf16(-3.140625) == -3.140625 and R.bf16(0.0) == 0.0
    x = torch.randn(4096, dtype=torch.float32)
    assert np.array_equal(R.bf16(x.double().numpy()), x.bfloat16().double().numpy())
    assert np.array_equal(R.f16(x.double().numpy()), x.half().double().numpy())


@pytest.mark.parametrize("p", [0.01, 0.1, 0.25])
def test_dropout_mask_rate_and_independence(p):
    n = 1 << 20
    keep = R.keep_mask(1234, 1, 0, 1024, 1024, p)
    sigma = math.sqrt(p * (1 - p) / n)
    assert abs(keep.mean() - (1 - p)) <= 4 * sigma
    other_site = R.keep_mask(1234, 1, 1, 1024, 1024, p)
    other_step = R.keep_mask(1234, 2, 0, 1024, 1024, p)
    other_seed = R.keep_mask(1235, 1, 0, 1024, 1024, p)
    for o in (other_site, other_step, other_seed):
        # independent masks disagree on 2 p (1 - p) of the elements
        d = (keep != o).mean()
        assert abs(d - 2 * p * (1 - p)) <= 4 * math.sqrt(2 * p * (1 - p) / n)
    assert np.array_equal(keep, R.keep_mask(1234, 1, 0, 1024, 1024, p))
    # the key is row * width + col: the same flat position under another width is the same draw
    assert np.array_equal(keep.reshape(-1), R.keep_mask(1234, 1, 0, 512, 2048, p).reshape(-1))


def test_schedule():
    f = HT.schedule_factor
    assert [f(t, 4, 10, "linear") for t in (1, 2, 4)] == [0.25, 0.5, 1.0]
    assert f(7, 4, 10, "linear") == 0.5 and f(10, 4, 10, "linear") == 0.0
    assert f(1, 0, 10, "linear") == 0.9 and f(3, 0, None, "linear") == 1.0
    assert all(f(t, 4, 10, "constant") == 1.0 for t in (1, 5, 10))


def _shapes(module):
    return {k: tuple(v.shape) for k, v in module.state_dict().items()}


def _fake_state_dict(dims, keys):
    sd = {}
    for k, (w, b) in zip(keys, HT.default_init(dims, 0)):
        sd[k + ".weight"], sd[k + ".bias"] = w, b
    return sd


def test_state_dict_layout_mutox():
    """mutox/factory.py:15-38."""
    d = 64
    model_all = nn.Sequential(nn.Sequential(nn.Dropout(0.01), nn.Linear(d, 512)), nn.Sequential(nn.ReLU(), nn.Linear(512, 128)),
                              nn.Sequential(nn.ReLU(), nn.Linear(128, 1)))
    holder = nn.Module()
    holder.model_all = model_all
    sd = _fake_state_dict([d, 512, 128, 1], HT.state_dict_keys("mutox", 3))
    assert _shapes(holder) == {k: tuple(v.shape) for k, v in sd.items()}
    holder.load_state_dict(sd, strict=True)
    with pytest.raises(ValueError):
        HT.state_dict_keys("mutox", 2)


@pytest.mark.parametrize("dropout", [0.0, 0.1])
@pytest.mark.parametrize("hidden", [[], [256], [256, 128]])
def test_state_dict_layout_blaser(hidden, dropout):
    """blaser/model.py:63-80, module for module."""
    width, modules = 6 * 64, []
    if hidden:
        if dropout > 0:
            modules.append(nn.Dropout(p=dropout))
        nprev = width
        for h in hidden:
            modules += [nn.Linear(nprev, h), nn.Tanh()]
            nprev = h
            if dropout > 0:
                modules.append(nn.Dropout(p=dropout))
        modules.append(nn.Linear(nprev, 1))
    else:
        modules.append(nn.Linear(width, 1))
    holder = nn.Module()
    holder.mlp = nn.Sequential(*modules)
    sd = _fake_state_dict([width, *hidden, 1], HT.state_dict_keys("blaser", len(hidden) + 1, dropout))
    assert _shapes(holder) == {k: tuple(v.shape) for k, v in sd.items()}
    holder.load_state_dict(sd, strict=True)


def test_state_dict_layout_classifier():
    """The notebook's head: fc1, tanh, dropout, classifier."""
    holder = nn.Module()
    holder.fc1, holder.classifier = nn.Linear(1024, 8192), nn.Linear(8192, 2)
    sd = _fake_state_dict([1024, 8192, 2], HT.state_dict_keys("classifier", 2))
    holder.load_state_dict(sd, strict=True)
    with pytest.raises(ValueError):
        HT.state_dict_keys("classifier", 3)
    with pytest.raises(ValueError):
        HT.state_dict_keys("fairseq", 2)


@pytest.mark.parametrize("kw", [
    dict(d_in=100), dict(d_in=0), dict(hidden_dims=[200]), dict(hidden_dims=[128] * 8), dict(out_dim=9), dict(out_dim=0),
    dict(out_dim=1, loss="ce"), dict(activation="GELU"), dict(loss="hinge"), dict(schedule="cosine"),
    dict(p_in=1.0), dict(p_hidden=1.0), dict(p_in=-0.1), dict(lr=-1.0), dict(weight_decay=-1.0), dict(warmup_steps=-1),
    dict(max_grad_norm=0.0), dict(max_batch=0),
    dict(init=[(torch.zeros(128, 64), torch.zeros(128))]),
    dict(init=[(torch.zeros(128, 32), torch.zeros(128)), (torch.zeros(2, 128), torch.zeros(2))]),
])
def test_python_side_refusals(kw):
    """Every one is refused before the device is looked at, so the same errors show with and without an MI355X."""
    args = dict(d_in=64, hidden_dims=[128], out_dim=2, device="cpu")
    args.update(kw)
    with pytest.raises(ValueError):
        HT.HeadTrainer(**args)


def test_constructor_refusals():
    with pytest.raises(ValueError, match="output_act"):
        HT.HeadTrainer.for_blaser(BlaserConfig(embedding_dim=64, hidden_dims=[128], output_act=True), device="cpu")
    with pytest.raises(ValueError, match="zero or negative"):   # the reference would build [Dropout, Linear]: key mlp.1
        HT.HeadTrainer.for_blaser(BlaserConfig(embedding_dim=64, hidden_dims=[0]), device="cpu")
    with pytest.raises(ValueError, match="input format"):
        HT.HeadTrainer.for_blaser(BlaserConfig(input_form="XX"), device="cpu")


def test_no_device_raises():
    """There is no CPU path."""
    with pytest.raises(RuntimeError, match="no CPU path"):
        HT.HeadTrainer(64, [128], 2, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU path"):
        HT.HeadTrainer.for_mutox(64, device="cpu")
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU path"):
            HT.HeadTrainer(64, [128], 2, device="cuda:0")
