"""Checker only: global-norm clip -> Adam -> soft update in float64 NumPy, written from the formulas
(torch.nn.utils.clip_grad_norm_, Kingma & Ba's Adam as torch.optim.Adam states it, ddpg_gumbel_fix.py:36-47), not from the kernel.

    total_norm = sqrt(sum over all tensors of sum g^2);  coef = min(1, max_norm / (total_norm + 1e-6))
    g = g * coef;  g = g + wd * p
    m = beta1 * m + (1 - beta1) * g;  v = beta2 * v + (1 - beta2) * g^2
    p = p - lr / (1 - beta1^t) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps)
    target = target * (1 - tau) + p * tau
"""
import numpy as np


class AdamF64(object):
    """State of one parameter set in float64.  ``params``: list of arrays (copied, any dtype)."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_norm=None, targets=None, tau=None):
        self.p = [np.array(x, dtype=np.float64) for x in params]
        self.m = [np.zeros_like(x) for x in self.p]
        self.v = [np.zeros_like(x) for x in self.p]
        self.t = None if targets is None else [np.array(x, dtype=np.float64) for x in targets]
        self.lr, self.betas, self.eps, self.wd, self.max_norm, self.tau = lr, betas, eps, weight_decay, max_norm, tau
        self.steps = [0] * len(self.p)
        self.total_norm = None

    def step(self, grads):
        """``grads``: one array or None per parameter (None: the parameter takes no part)."""
        live = [i for i, g in enumerate(grads) if g is not None]
        g64 = {i: np.asarray(grads[i], dtype=np.float64) for i in live}
        self.total_norm = float(np.sqrt(sum(float(np.sum(g64[i] * g64[i])) for i in live)))
        coef = 1.0
        if self.max_norm is not None:
            coef = min(1.0, self.max_norm / (self.total_norm + 1e-6))
        b1, b2 = self.betas
        for i in live:
            g = g64[i] * coef
            if self.wd:
                g = g + self.wd * self.p[i]
            self.steps[i] += 1
            t = self.steps[i]
            self.m[i] = b1 * self.m[i] + (1.0 - b1) * g
            self.v[i] = b2 * self.v[i] + (1.0 - b2) * g * g
            denom = np.sqrt(self.v[i]) / np.sqrt(1.0 - b2 ** t) + self.eps
            self.p[i] = self.p[i] - self.lr / (1.0 - b1 ** t) * self.m[i] / denom
            if self.t is not None:
                self.t[i] = soft_update_f64(self.t[i], self.p[i], self.tau)


def soft_update_f64(target, source, tau):
    return target * (1.0 - tau) + source * tau


def soft_update_f32(target, source, tau):
    """The float32 restatement the kernels promise: (1 - tau) formed in float64 and rounded once, both products rounded before the
    sum; tau == 1 copies."""
    target, source = np.asarray(target, dtype=np.float32), np.asarray(source, dtype=np.float32)
    if tau == 1.0:
        return source.copy()
    a = target * np.float32(1.0 - tau)
    b = source * np.float32(tau)
    return a + b
