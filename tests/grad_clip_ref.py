"""NumPy float64 restatement of per-group gradient norms, the clip coefficient of torch.nn.utils.clip_grad_norm_ and AdamW on
clipped gradients (not a test module: tests/test_grad_clip_cpu.py pins it against torch in float64, tests/test_gpu_grad_clip.py
holds the device kernels to it)."""
import numpy as np


def group_sumsq(grads_by_group):
    """[sum(g^2) in float64] per group; grads_by_group: a list (one entry per group) of lists of arrays."""
    return np.array([sum(float(np.square(np.asarray(g, dtype=np.float64)).sum()) for g in grads) for grads in grads_by_group],
                    dtype=np.float64)


def norms(sumsq, scales):
    """(per-group norms, total norm) of gradients whose group g is multiplied by scales[g] before the update consumes it."""
    sumsq, scales = np.asarray(sumsq, dtype=np.float64), np.asarray(scales, dtype=np.float64)
    return np.sqrt(sumsq) * scales, float(np.sqrt((sumsq * scales * scales).sum()))


def clip_coef(total_norm, max_norm):
    """clip_grad_norm_: clamp(max_norm / (total_norm + 1e-6), max = 1)."""
    return min(1.0, float(max_norm) / (float(total_norm) + 1e-6))


def adamw_update(p, g, m, v, step, lr, betas, eps, weight_decay):
    """One torch.optim.AdamW step (in place) on float64 arrays; step >= 1."""
    b1, b2 = betas
    p *= 1.0 - lr * weight_decay
    m *= b1
    m += (1.0 - b1) * g
    v *= b2
    v += (1.0 - b2) * g * g
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    p -= (lr / bc1) * (m / (np.sqrt(v) / np.sqrt(bc2) + eps))


class ClippedAdamW:
    """groups: [{"params": [float64 arrays], "lr", "betas", "eps", "weight_decay"}].  step(grads_by_group, max_norm) clips by the
    global norm over every group (max_norm None: no clipping) and updates; returns (group norms, total norm, coef)."""

    def __init__(self, groups):
        self.groups = groups
        self.m = [[np.zeros_like(p) for p in g["params"]] for g in groups]
        self.v = [[np.zeros_like(p) for p in g["params"]] for g in groups]
        self.t = 0

    def step(self, grads_by_group, max_norm=None):
        gn, total = norms(group_sumsq(grads_by_group), np.ones(len(self.groups)))
        coef = clip_coef(total, max_norm) if max_norm is not None else 1.0
        self.t += 1
        for gi, group in enumerate(self.groups):
            for p, g, m, v in zip(group["params"], grads_by_group[gi], self.m[gi], self.v[gi]):
                adamw_update(p, np.asarray(g, dtype=np.float64) * coef, m, v, self.t, group["lr"], group["betas"], group["eps"],
                             group["weight_decay"])
        return gn, total, coef
