"""Plain restatement of u3d_adamw_step_accum (include/u3d_hip.h): one object holds the flat buffers and counters, call() is one
micro-step.  dtype=torch.float32 follows the kernel's arithmetic in its order (scalars rounded to f32 first); dtype=torch.float64 is
the yardstick.  CPU tensors only; used by tests/test_accum_cpu.py and tests/test_accum_gpu.py."""
import math

import numpy as np
import torch

ACCUMULATED, APPLIED, DROPPED, HELD = 0, 1, 2, 3


class AccumRef:
    def __init__(self, param, k=1, dtype=torch.float32, lr=3e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, max_norm=0.0,
                 ema_decay=None, skip=None, exp_avg=None, exp_avg_sq=None):
        self.dtype = dtype
        self.s = np.float32 if dtype == torch.float32 else np.float64            # scalar type of the coefficients
        self.p = param.detach().cpu().to(dtype).clone()
        n = self.p.numel()
        self.m = torch.zeros_like(self.p) if exp_avg is None else exp_avg.detach().cpu().to(dtype).clone()
        self.v = torch.zeros_like(self.p) if exp_avg_sq is None else exp_avg_sq.detach().cpu().to(dtype).clone()
        self.acc = torch.zeros_like(self.p)
        self.k = int(k)
        # the decay the kernel sees is the float32 one in both variants
        self.d = None if ema_decay is None or ema_decay <= 0 else self.s(np.float32(ema_decay))
        self.ema = self.p.clone() if ema_decay is not None else None
        # hyper-parameters live in the f32 state vector: both variants start from those values
        f = lambda x: self.s(np.float32(x))                                      # noqa: E731
        self.lr, self.b1, self.b2, self.eps, self.wd, self.max_norm = f(lr), f(betas[0]), f(betas[1]), f(eps), f(weight_decay), f(max_norm)
        self.live = torch.ones(n, dtype=torch.bool)
        if skip is not None:                                                     # uint8 per 64-element chunk, 1 = untouched
            self.live = ~skip.detach().cpu().bool().repeat_interleave(64)[:n]
        self.step = 0            # state[0]
        self.coef = None         # state[1]
        self.norm = None         # state[4] / acc_state[6]
        self.fill = 0            # acc_state[1]
        self.applied = 0         # acc_state[2]
        self.dropped = 0         # acc_state[3]
        self.held = 0            # state[12]
        self.outcome = None      # acc_state[5]

    def tensors(self):
        return [self.p, self.m, self.v, self.acc] + ([self.ema] if self.ema is not None else [])

    def call(self, grad, hold=False):
        s, live = self.s, self.live
        if hold:
            self.held += 1
            self.outcome = HELD
            return self.outcome
        g = grad.detach().cpu().to(self.dtype)
        self.acc[live] += g[live]
        c = self.fill + 1
        if c < self.k:
            self.fill = c
            self.outcome = ACCUMULATED
            return self.outcome
        gbar = torch.where(live, self.acc, g) / float(s(self.k))
        tot = math.sqrt(float((gbar * gbar).double().sum())) if bool(torch.isfinite(gbar).all()) else float("nan")
        self.fill = 0
        self.norm = tot
        if not math.isfinite(tot):
            self.acc[live] = 0
            self.dropped += 1
            self.outcome = DROPPED
            return self.outcome
        coef = s(1)
        if self.max_norm > 0:
            coef = min(s(1), self.max_norm / (s(tot) + s(1e-6)))
        self.step += 1
        t = s(self.step)
        bc1, bc2 = s(1) - s(np.power(self.b1, t)), s(1) - s(np.power(self.b2, t))
        step_size, bc2_sqrt, decay = self.lr / bc1, s(np.sqrt(bc2)), s(1) - self.lr * self.wd
        self.coef = coef
        gr = gbar * float(coef)
        p, m, v = self.p * float(decay), self.m, self.v
        m = m + (gr - m) * float(s(1) - self.b1)
        v = float(self.b2) * v + float(s(1) - self.b2) * gr * gr
        denom = v.sqrt() / float(bc2_sqrt) + float(self.eps)
        p = p - float(step_size) * (m / denom)
        self.p[live], self.m[live], self.v[live] = p[live], m[live], v[live]
        if self.ema is not None and self.d is not None:
            e = self.ema + float(s(1) - self.d) * (self.p - self.ema)
            self.ema[live] = e[live]
        self.acc[live] = 0
        self.applied += 1
        self.outcome = APPLIED
        return self.outcome
