"""CPU restatement of the head-training contract (include/sonar_mi355.h: smi_head_trainer_*), in float64.

Two modes:
  mirror=True   every STORAGE rounding of the engine is applied where the engine applies it, and nothing else: fp16
                shadow weights and activations, the fp32 multiply + fp16 rounding of dropout, bf16 dz, bf16 conversion
                of A and of the shadow W on the way into the backward products, fp32 gradients / masters / moments, and
                the fp32 values of the scalar arguments (lr, betas, eps, weight decay).  The arithmetic between two
                storage points is exact (float64), so what remains against the engine is its fp32 accumulation order
                and the ulps of tanhf / expf.
  mirror=False  exact arithmetic on the fp16 shadow weights: only the hidden weights are rounded (to fp16) before use.

The dropout mask is the engine's pure function of (seed, step, site, row, col); the schedule is imported from the
package.  Flat parameter order everywhere: W0, b0, W1, b1, ... in nn.Linear layouts.
"""
import numpy as np

from sonar_amd.head_training import schedule_factor  # noqa: F401  (shared with the engine's host side)

GOLD = np.uint64(0x9E3779B97F4A7C15)
M1 = np.uint64(0xBF58476D1CE4E5B9)
M2 = np.uint64(0x94D049BB133111EB)


def f16(x):
    """RNE to fp16, back in float64."""
    return np.asarray(x, dtype=np.float64).astype(np.float16).astype(np.float64)


def f32(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


def bf16(x):
    """RNE to bf16 (8 significant bits) straight from float64; bf16 subnormals are outside the contract's range."""
    m, e = np.frexp(np.asarray(x, dtype=np.float64))
    return np.ldexp(np.rint(m * 256.0), e - 8)


def keep_mask(seed, step, site, rows, width, p):
    """[rows, width] bool: element kept iff u >= p, u = (mix(seed + GOLD * (key + 1)) >> 40) * 2^-24,
    key = (step*16 + site) * 2^40 + row*width + col; p is compared as the fp32 value the engine receives."""
    with np.errstate(over="ignore"):
        base = np.uint64(((int(step) * 16 + int(site)) << 40) % (1 << 64))
        idx = np.arange(rows * width, dtype=np.uint64).reshape(rows, width)
        z = np.uint64(int(seed) % (1 << 64)) + GOLD * (base + idx + np.uint64(1))
        z = (z ^ (z >> np.uint64(30))) * M1
        z = (z ^ (z >> np.uint64(27))) * M2
        z = z ^ (z >> np.uint64(31))
    u = (z >> np.uint64(40)).astype(np.float64) * 2.0 ** -24
    return u >= float(np.float32(p))


def loss_and_dlogits(logits, y, loss):
    """(mean loss, dL/dlogits) in float64; y int labels [rows] (ce) or float targets [rows, out]."""
    rows, out = logits.shape
    if loss == "ce":
        mx = logits.max(1, keepdims=True)
        e = np.exp(logits - mx)
        se = e.sum(1, keepdims=True)
        onehot = np.zeros_like(logits)
        onehot[np.arange(rows), y] = 1.0
        L = (np.log(se[:, 0]) + mx[:, 0] - logits[np.arange(rows), y]).mean()
        return L, (e / se - onehot) / rows
    y = np.asarray(y, dtype=np.float64).reshape(rows, out)
    if loss == "bce":
        e = np.exp(-np.abs(logits))
        L = (np.maximum(logits, 0.0) - logits * y + np.log1p(e)).mean()
        s = np.where(logits >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
        return L, (s - y) / (rows * out)
    d = logits - y
    return (d * d).mean(), 2.0 * d / (rows * out)


class RefTrainer:
    def __init__(self, dims, activation="TANH", loss="ce", p_in=0.0, p_hidden=0.0, lr=1e-4, weight_decay=1e-3,
                 warmup_steps=0, schedule="linear", max_grad_norm=1.0, seed=0, init=None, mirror=True,
                 betas=(0.9, 0.999), eps=1e-8):
        self.dims, self.activation, self.loss = list(dims), activation, loss
        self.p_in, self.p_hidden = float(np.float32(p_in)), float(np.float32(p_hidden))
        self.lr, self.warmup_steps, self.schedule, self.max_grad_norm = lr, warmup_steps, schedule, max_grad_norm
        self.seed, self.mirror = seed, mirror
        c = (lambda v: float(np.float32(v))) if mirror else float
        self.wd, self.b1, self.b2, self.eps = c(weight_decay), c(betas[0]), c(betas[1]), c(eps)
        self.W = [np.asarray(w, dtype=np.float64).copy() for w, _ in init]
        self.b = [np.asarray(b, dtype=np.float64).copy() for _, b in init]
        if mirror:
            self.W, self.b = [f32(w) for w in self.W], [f32(b) for b in self.b]
        self.mW, self.vW = [np.zeros_like(w) for w in self.W], [np.zeros_like(w) for w in self.W]
        self.mb, self.vb = [np.zeros_like(b) for b in self.b], [np.zeros_like(b) for b in self.b]
        self.t, self.total_steps = 0, None

    def _drop(self, h, step, site):
        """Dropout at `site` on stored values h: (dropped copy, keep-and-scale factor for the backward pass)."""
        p = self.p_in if site == 0 else self.p_hidden
        if p <= 0.0:
            return h, None
        keep = keep_mask(self.seed, step, site, h.shape[0], h.shape[1], p)
        if self.mirror:
            s32 = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
            a = np.where(keep, (h.astype(np.float32) * s32), np.float32(0.0)).astype(np.float16).astype(np.float64)
            return a, keep * float(s32)
        s = 1.0 / (1.0 - p)
        return np.where(keep, h * s, 0.0), keep * s

    def forward_backward(self, xb, yb, step):
        """-> (loss, [(gW, gb)]) of one batch with the masks of `step` (1-based)."""
        mir, nh = self.mirror, len(self.dims) - 2
        x = np.asarray(xb, dtype=np.float64)
        if mir and self.p_in <= 0.0:
            x = f16(x)
        a0, _ = self._drop(x, step, 0)
        acts, hs, factors = [a0], [], []
        Wsh = [f16(w) for w in self.W[:nh]]
        for l in range(nh):
            z = acts[-1] @ Wsh[l].T + self.b[l]
            h = np.tanh(z) if self.activation == "TANH" else np.maximum(z, 0.0)
            if mir:
                h = f16(h)
            a, fac = self._drop(h, step, l + 1)
            hs.append(h)
            factors.append(fac)
            acts.append(a)
        logits = acts[-1] @ self.W[nh].T + self.b[nh]
        L, d = loss_and_dlogits(logits, yb, self.loss)
        grads = [None] * (nh + 1)
        grads[nh] = (d.T @ acts[-1], d.sum(0))
        dA = d @ self.W[nh]
        for l in range(nh - 1, -1, -1):
            t = dA if factors[l] is None else dA * factors[l]
            h = hs[l]
            dz = t * (1.0 - h * h) if self.activation == "TANH" else np.where(h > 0, t, 0.0)
            if mir:
                dz = bf16(dz)
                grads[l] = (dz.T @ bf16(acts[l]), dz.sum(0))
                dA = dz @ bf16(Wsh[l])
            else:
                grads[l] = (dz.T @ acts[l], dz.sum(0))
                dA = dz @ Wsh[l]
        if mir:
            grads = [(f32(gw), f32(gb)) for gw, gb in grads]
        return float(L), grads

    def apply(self, grads, lr):
        """Clip + one AdamW step (torch.optim.AdamW, decoupled decay on every parameter)."""
        self.t += 1
        lr = float(np.float32(lr)) if self.mirror else float(lr)
        scale = 1.0
        if self.max_grad_norm is not None:
            norm = np.sqrt(sum((gw * gw).sum() + (gb * gb).sum() for gw, gb in grads))
            scale = min(1.0, self.max_grad_norm / (norm + 1e-6))
        bc1, bc2 = 1.0 - self.b1 ** self.t, 1.0 - self.b2 ** self.t
        rnd = f32 if self.mirror else (lambda v: v)
        for l, (gw, gb) in enumerate(grads):
            for P, Mo, Vo, g in ((self.W, self.mW, self.vW, gw), (self.b, self.mb, self.vb, gb)):
                g = g * scale
                p = P[l] * (1.0 - lr * self.wd)
                m = self.b1 * Mo[l] + (1.0 - self.b1) * g
                v = self.b2 * Vo[l] + (1.0 - self.b2) * g * g
                p = p - (lr / bc1) * (m / (np.sqrt(v) / np.sqrt(bc2) + self.eps))
                P[l], Mo[l], Vo[l] = rnd(p), rnd(m), rnd(v)

    def lr_at(self, t):
        return self.lr * schedule_factor(t, self.warmup_steps, self.total_steps, self.schedule)

    def step(self, xb, yb):
        L, grads = self.forward_backward(xb, yb, self.t + 1)
        self.apply(grads, self.lr_at(self.t + 1))
        return L

    def fit(self, X, y, epochs, batch_size, perms=None):
        """perms: one index array per epoch (None = in order), the permutations the engine's `fit` drew."""
        X, y = np.asarray(X), np.asarray(y)
        n = X.shape[0]
        per_epoch = (n + batch_size - 1) // batch_size
        self.total_steps = self.t + epochs * per_epoch
        losses = []
        for ep in range(epochs):
            order = np.arange(n) if perms is None else np.asarray(perms[ep])
            for off in range(0, n, batch_size):
                idx = order[off:off + batch_size]
                losses.append(self.step(X[idx], y[idx]))
        return np.array(losses)


def adamw_reference(p, g, m, v, step, lr, b1, b2, eps, wd, max_grad_norm):
    """float64 formula of one clipped AdamW step on flat vectors, with the fp32 values of the scalar arguments:
    -> (p, m, v, norm, scale)."""
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    lr, b1, b2, eps, wd = (float(np.float32(a)) for a in (lr, b1, b2, eps, wd))
    norm = np.sqrt((g * g).sum())
    scale = min(1.0, float(np.float32(max_grad_norm)) / (norm + 1e-6)) if max_grad_norm else 1.0
    g = g * scale
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    p = p * (1.0 - lr * wd) - (lr / bc1) * (m / (np.sqrt(v) / np.sqrt(bc2) + eps))
    return p, m, v, norm, scale
